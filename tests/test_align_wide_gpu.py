"""GPU parity of both aligners on wide graphs, wide emission sets and long calls: amx_align_viterbi_dev and amx_bw_align_dev on the named
cases of tests/wide_graphs.py against the restatements, with the helpers and the bars of tests/test_align_gpu.py (every bit) and
tests/test_bw_gpu.py (discrete results equal, score within 2 f32 ulp, log_total within 1e-11, f32 weights equal in bits where their f64
share is further than 1e-11 from a boundary between two f32 values and within one ulp elsewhere).  tests/test_align_wide.py shows without
a GPU that each case reaches what it is named for, that ties decide its labels, and that at most 1 % of its items are exempted.

Every matrix has 10000 columns, rows 10003 words apart, and NaN in every column its segment's graph does not read.

Shapes (what the toys of the two older files do not reach).
  active, active_pruned, active_counted   2048 states whose active set grows 7, 43, 243, 743, 2048: the rank scan's cross-wave half, ties
                                          above rank 511, 32 survivor words; pruned: ranks and survivor bits with holes, three passes;
                                          counted: passes that are counted and not run
  fan64                                   64 arcs out of one state: ordinal 63, mask bit 63
  funnel                                  2047 arcs of one label into one state
  em256, em257, em4096, limits            the gather's second trip, row words 1 to 15, columns up to 9999; limits: 2048 states, 4096
                                          emissions, 4096 labels and a frame of 4096 items, the kernels' largest LDS requests
  items                                   frames of 64, 257, 513 and 1025 items and frames of 60 items of one weight
  arcs_fit, arcs_spill                    the last arc count that the Viterbi kernel keeps in LDS, and the first it reads from memory
  mixed_batch                             four recorded cases in one call with `limits`, and alone
  long_call                               300 segments of 0 to 3 frames behind 300 rows of another call: every loop of bw_scan_kernel twice

Item order.  With thousands of items per frame a few shares lie within the bar of an f32 boundary, where a legitimate one-ulp difference
may swap two neighbours.  check_items_wide therefore checks the order in two parts: each frame's device items are sorted by (weight
descending, label ascending) on the device's own weights, exactly; and brought into the restatement's order by (frame, label) they pass
check_batch as they are.  Frames without an exempted item must match the restatement's order element for element."""
import numpy as np
import pytest

from rasr_amd import _lib
from tests import align_reference as ar
from tests import bw_reference as br
from tests import wide_graphs as wg
from tests.test_align import bits, same
from tests.test_align_gpu import check_segment, device_align
from tests.test_align_wide import EXEMPT_CAP, baum_welch, executed_passes, exempt_share, segments, viterbi
from tests.test_bw import POSTERIOR_BAR
from tests.test_bw_gpu import check_batch, device_bw

pytestmark = pytest.mark.gpu
NC, LD = wg.N_COLUMNS, wg.LD
ROWS_BEFORE = {"long_call": 300}


def _torch():
    import torch
    return torch


def viterbi_on_device(ctx, name, handle=None):
    """one call over a case: the device's (label, emission, arc_score, result) per segment and the counters"""
    c = wg.case(name)
    l, e, s, res, counters = device_align(ctx, c["graphs"], c["off"], c["scores"], handle=handle, ld=LD, rows_before=ROWS_BEFORE.get(name, 0), n_columns=NC, **c["cfg"])
    off = c["off"]
    return [(l[off[i]:off[i + 1]], e[off[i]:off[i + 1]], s[off[i]:off[i + 1]], res[i]) for i in range(len(res))], counters


def bw_on_device(ctx, name, handle=None):
    c = wg.case(name)
    return device_bw(ctx, c["graphs"], c["off"], c["scores"], handle=handle, ld=LD, rows_before=ROWS_BEFORE.get(name, 0), n_columns=NC, **c["cfg"])


def check_items_wide(got, ioff, results, wants, off, what):
    """check_batch with the order of a frame's items checked in two parts (see above)"""
    f, l, e, w, o, share = br.flat_items(wants, off)
    assert np.array_equal(ioff, o) and np.array_equal(got["frame"], f), what
    # (a) sorted on the device's own weights
    gw, gl = got["weight"], got["label"]
    inside = f[1:] == f[:-1]
    ordered = (gw[:-1] > gw[1:]) | ((gw[:-1] == gw[1:]) & (gl[:-1] < gl[1:]))
    assert ordered[inside].all(), what
    # (b) the same map (frame, label) -> (emission, weight): the device's items in the restatement's order pass check_batch
    back = np.empty(len(f), np.int64)
    back[np.lexsort((l, f))] = np.lexsort((gl, got["frame"]))
    check_batch({k: v[back] for k, v in got.items()}, ioff, results, wants, off, what)
    # frames without an exempted item: the restatement's order, element for element
    exempted = br.midpoint_distance(share) <= POSTERIOR_BAR if len(share) else np.zeros(0, bool)
    clean = ~np.isin(f, f[exempted])
    assert np.array_equal(gl[clean], l[clean]) and np.array_equal(got["emission"][clean], e[clean]) and np.array_equal(bits(gw)[clean], bits(w)[clean]), what
    return int(exempted.sum())


@pytest.mark.parametrize("name", wg.BOTH)
def test_viterbi_equals_the_restatement(ctx, name):
    want = viterbi(name)
    got, counters = viterbi_on_device(ctx, name)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        check_segment(g, w, (name, i))
    assert counters[0] == 0 and counters[1] + counters[2] == sum(w["n_iterations"] for w in want)
    assert counters[1] == executed_passes(name), "passes that repeat an outcome are counted, not run"


@pytest.mark.parametrize("name", wg.BOTH)
def test_baum_welch_equals_the_restatement(ctx, name):
    want = baum_welch(name)
    assert exempt_share(want) <= EXEMPT_CAP            # a condition on the inputs, before the device is touched
    got, ioff, res, counters = bw_on_device(ctx, name)
    check_items_wide(got, ioff, res, want, wg.case(name)["off"], name)
    assert counters[0] == 0 and counters[1] + counters[2] == sum(w["n_iterations"] for w in want)
    assert counters[1] == sum(w["passes_run"] for w in want), "passes that repeat an outcome are counted, not run"


def test_the_boundary_pair_differs_in_where_the_arcs_lie_only(ctx):
    """the larger graph of the pair holds the smaller one's arcs and one more; both sides of the decision give the restatement's bits
    (the two tests above), on one handle in either order as well"""
    import rasr_amd
    a = rasr_amd.ViterbiAligner(ctx)
    for name in ("arcs_spill", "arcs_fit", "arcs_spill"):
        got, _ = viterbi_on_device(ctx, name, handle=a)
        check_segment(got[0], viterbi(name)[0], name)
    a.close()


def test_mixed_batch_segments_alone(ctx):
    """the recorded cases give the same bits alone (24 columns, arcs in LDS) and beside the limits (arcs of the whole call in memory,
    every LDS table at its largest)"""
    c = wg.case("mixed_batch")
    small = ar.cases()
    v, _ = viterbi_on_device(ctx, "mixed_batch")
    got, ioff, res, _ = bw_on_device(ctx, "mixed_batch")
    for i, n in zip((0, 1, 3, 4), wg.SMALL):
        g, rows, T = small[n]["graph"], small[n]["scores"], len(small[n]["scores"])
        l, e, s, r, _ = device_align(ctx, [g], [0, T], rows)
        assert same(l, v[i][0]) and same(e, v[i][1]) and same(s, v[i][2]), n
        assert {k: bits(np.asarray(x)).tolist() for k, x in r[0].items()} == {k: bits(np.asarray(x)).tolist() for k, x in v[i][3].items()}, n
        alone, o, ra, _ = device_bw(ctx, [g], [0, T], rows)
        a, b = int(ioff[c["off"][i]]), int(ioff[c["off"][i + 1]])
        assert np.array_equal(o, ioff[c["off"][i]:c["off"][i + 1] + 1] - a), n
        for k in ("label", "emission", "weight", "weight_f64"):
            assert same(alone[k], got[k][a:b]), (n, k)
        assert same(alone["frame"] + int(c["off"][i]), got["frame"][a:b]), n
        assert {k: bits(np.asarray(x)).tolist() for k, x in ra[0].items()} == {k: bits(np.asarray(x)).tolist() for k, x in res[i].items()}, n


def test_4097_emissions_are_refused_and_the_handles_still_work(ctx):
    import rasr_amd
    torch = _torch()
    g = rasr_amd.ViterbiAligner.graphs([wg.refused()])
    scores = torch.zeros((4, NC), dtype=torch.float32, device="cuda")
    a, b = rasr_amd.ViterbiAligner(ctx), rasr_amd.BaumWelchAligner(ctx)
    ctx.use_torch_stream()
    label = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    emission, arc = label.clone(), torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(rasr_amd.AmxError) as err:
        a.align([0, 4], g, scores, NC, label_dev=label, emission_dev=emission, arc_score_dev=arc)
    assert err.value.status == _lib.AMX_ERR_UNSUPPORTED and "4097 emission indices" in str(err.value) and "amx_align_viterbi_dev" in str(err.value)
    ioff = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(rasr_amd.AmxError) as err:
        b.align([0, 4], g, scores, NC, item_offsets_dev=ioff)
    assert err.value.status == _lib.AMX_ERR_UNSUPPORTED and "4097 emission indices" in str(err.value) and "amx_bw_align_dev" in str(err.value)
    torch.cuda.synchronize()
    assert (label == -7).all() and (emission == -7).all() and (arc == -7).all() and (ioff == -7).all() and _lib.lib().amx_bw_n_items(b.h) == 0
    # the handles still work: the widest case that is taken
    got, _ = viterbi_on_device(ctx, "em4096", handle=a)
    check_segment(got[0], viterbi("em4096")[0], "after the refusal")
    got, o, res, _ = bw_on_device(ctx, "em4096", handle=b)
    check_items_wide(got, o, res, baum_welch("em4096"), wg.case("em4096")["off"], "after the refusal")
    a.close(), b.close()


def test_gather_rows_over_the_items_of_the_limits(ctx):
    """thousands of rows of 65 values: the lanes of gather_rows_kernel take a second trip"""
    import rasr_amd
    torch = _torch()
    got, ioff, res, _ = bw_on_device(ctx, "limits")
    n, T = len(got["frame"]), len(wg.case("limits")["scores"])
    assert n == sum(r["n_items"] for r in baum_welch("limits")) > 3 * 4096
    x = np.random.Generator(np.random.PCG64(5)).standard_normal((T, 65)).astype(np.float32)
    ctx.use_torch_stream()
    rows = rasr_amd.gather_rows(ctx, torch.from_numpy(x).cuda(), torch.from_numpy(got["frame"]).cuda())
    torch.cuda.synchronize()
    assert same(rows.cpu().numpy(), x[got["frame"]])
