"""GPU parity: amx_bw_align_dev (bw_search_kernel, bw_forward_kernel, bw_backward_kernel, bw_scan_kernel), amx_bw_items_dev and
amx_gather_rows_dev through the Python class against the device-order restatement of tests/bw_reference.py.

Against the reference's own run (tests/golden/ref_bw.npz): reached flag, iterations, last threshold, survivor sum and average equal, the
score within tests/test_bw.py's derived score bar, `log_total` within 1e-11 (1 + |bw[initial]|), the item keys equal as far as f32 holds
their weights (tests/test_bw.py, "Key sets") and the weights within |d| <= a + r w_ref, (a, r) the bars the generator measured.

Bars.  Discrete results (reached, iterations, last threshold, survivor sum, item keys, order and offsets) equal.  The alignment score
within 2 f32 ulp and log_total within 1e-11 relative: the device's f64 exp and log1p are not the host library's.  f32 weights equal in
bits wherever their f64 share lies further than 1e-11 (relative) from a boundary between two f32 values, within one ulp elsewhere: the
project's bar on posteriors (tests/test_posterior.py).

Shapes.  The kernels give a segment one workgroup of 256 lanes, a lane the states (and labels) lane, lane + 256, ...: graphs of 3, 70 and
130 states sit inside one wave and across waves, 2048 states (the limit) fill every slot of a lane and two survivor words per wave; the
items of a frame are sorted in LDS over the next power of two, from 1 item to 12.  Frames of 13 to 4096 items, equal weights beyond two
items, 4096 labels and emissions, calls of more than 256 rows or segments and a first row above 256 are in tests/test_align_wide_gpu.py."""
import numpy as np
import pytest

from rasr_amd import _lib
from tests import align_reference as ar
from tests import bw_reference as br
from tests.test_align import all_cases, bits, same
from tests.test_bw import POSTERIOR_BAR, check_items_against_reference, check_search_against_fixture, fixture_items, golden, restated  # noqa: F401  (golden is a fixture)

pytestmark = pytest.mark.gpu
N = ar.N_COLUMNS


def _torch():
    import torch
    return torch


def device_bw(ctx, graphs, off, scores, handle=None, ld=None, rows_before=0, n_columns=N, **cfg):
    """one amx_bw_align_dev call; the matrix (n_columns wide) is padded to `ld` columns and shifted down by `rows_before` rows when asked.  Returns the
    item arrays (frame relative to the call's first row), the offsets of the call's rows, the per-segment results and the counters."""
    import rasr_amd
    torch = _torch()
    off = np.asarray(off, np.int64) + rows_before
    ld = ld or n_columns
    rows = int(off[-1])
    host = np.full((max(rows, 1), ld), np.nan, np.float32)
    host[rows_before:rows, :n_columns] = scores
    dev = torch.from_numpy(host).cuda()
    ioff = torch.full((rows + 1,), -7, dtype=torch.int64, device="cuda")
    a = handle or rasr_amd.BaumWelchAligner(ctx, **cfg)
    ctx.use_torch_stream()
    items, _, results, counters = a.align(off, graphs, dev, ld, n_columns=n_columns, item_offsets_dev=ioff)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in items.items()}
    if handle is None:
        a.close()
    o = ioff.cpu().numpy()
    assert (o[:rows_before + 1] == 0).all() and o[-1] == len(got["frame"]) == sum(r["n_items"] for r in results)
    assert np.array_equal(got["weight_f64"], got["weight"].astype(np.float64))
    assert np.array_equal(np.repeat(np.arange(rows), np.diff(o)), got["frame"])
    got["frame"] = got["frame"] - rows_before
    return got, o[rows_before:], results, counters


def check_weights(got, want, share, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    far = br.midpoint_distance(share) > POSTERIOR_BAR
    assert np.array_equal(bits(got)[far], bits(want)[far]), what
    assert (np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64)) <= 1).all(), what


def check_batch(got, ioff, results, wants, off, what):
    """device items and results of a batch against the restatement's results of its segments"""
    f, l, e, w, o, share = br.flat_items(wants, off)
    assert np.array_equal(ioff, o), what
    assert np.array_equal(got["frame"], f) and np.array_equal(got["label"], l) and np.array_equal(got["emission"], e), what
    check_weights(got["weight"], w, share, what)
    for r, want in zip(results, wants):
        assert r["reached"] == bool(want["reached"]) and r["n_iterations"] == want["n_iterations"] and r["state_sum"] == want["state_sum"], what
        assert same(r["last_threshold"], np.float32(want["last_threshold"])) and r["n_items"] == want["n_items"], what
        assert same(np.float64(r["average_states"]), np.float64(want["average_states"])) or (np.isnan(r["average_states"]) and np.isnan(want["average_states"])), what
        if want["reached"]:
            assert abs(float(r["score"]) - float(want["score"])) <= 2 * np.spacing(np.float32(abs(want["score"]))), what
            assert abs(r["log_total"] - want["log_total"]) <= POSTERIOR_BAR * abs(want["log_total"]), what
        else:
            assert same(r["score"], ar.F32_MAX) and r["n_items"] == 0 and r["log_total"] == br.DEAD, what


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_every_case_equals_the_restatement_and_the_references_search(ctx, golden, name):
    c = all_cases()[name]
    T = len(c["scores"])
    got, ioff, res, counters = device_bw(ctx, [c["graph"]], [0, T], c["scores"], **c["cfg"])
    want = restated(name)
    check_batch(got, ioff, res, [want], [0, T], name)
    check_search_against_fixture(golden, name, res[0], exact_score=False)
    check_items_against_reference(golden, {(int(f), int(l)): w for f, l, w in zip(got["frame"], got["label"], got["weight"])}, fixture_items(golden, name), name)
    if want["reached"] and T:
        ref = float(golden["off/%s/bw_initial" % name])
        assert abs(res[0]["log_total"] - ref) <= POSTERIOR_BAR * (1 + abs(ref)), name
    assert counters[0] == 0 and counters[1] + counters[2] == res[0]["n_iterations"]
    assert counters[1] == want["passes_run"], "passes that repeat an outcome are counted, not run"


def batch_results(ctx, handle=None, **kw):
    graphs, off, scores = ar.batch_case(all_cases())
    got, ioff, res, counters = device_bw(ctx, graphs, off, scores, handle=handle, **kw)
    return graphs, off, scores, (got, ioff, res), counters


def same_items(a, b):
    return all(same(a[0][k], b[0][k]) for k in a[0]) and np.array_equal(a[1], b[1]) and \
        [{k: bits(np.asarray(v)).tolist() for k, v in r.items()} for r in a[2]] == [{k: bits(np.asarray(v)).tolist() for k, v in r.items()} for r in b[2]]


def test_batch_of_eight_segments(ctx):
    graphs, off, scores, got, counters = batch_results(ctx)
    assert len(graphs) == 8 and 0 in np.diff(off)
    check_batch(*got, [restated(n) for n in ar.BATCH], off, "batch")
    assert counters[0] == 0 and counters[1] + counters[2] == sum(r["n_iterations"] for r in got[2])


def test_batch_independence_and_call_history(ctx):
    """each segment of the batch aligned alone gives the bits it has inside the batch: on a fresh handle, and on one handle that has
    aligned the whole batch and an unrelated larger graph before (its buffers and its item store are sized and filled by those calls)"""
    import rasr_amd
    graphs, off, scores, got, _ = batch_results(ctx)
    used = rasr_amd.BaumWelchAligner(ctx)
    batch_results(ctx, handle=used)
    big = ar.linear_hmm(300, N, 77)
    device_bw(ctx, [big, big], [0, 150, 190], ar._gauss("history", 190), handle=used)
    for i, name in enumerate(ar.BATCH):
        rows = scores[off[i]:off[i + 1]]
        a, b = int(got[1][off[i]]), int(got[1][off[i + 1]])
        for handle in (None, used):
            g, o, res, _ = device_bw(ctx, [graphs[i]], [0, len(rows)], rows, handle=handle)
            assert np.array_equal(o, got[1][off[i]:off[i + 1] + 1] - a), name
            assert same(g["frame"] + int(off[i]), got[0]["frame"][a:b]), name
            for k in ("label", "emission", "weight", "weight_f64"):
                assert same(g[k], got[0][k][a:b]), (name, k, handle is used)
            assert {k: bits(np.asarray(v)).tolist() for k, v in res[0].items()} == {k: bits(np.asarray(v)).tolist() for k, v in got[2][i].items()}, name
    assert same_items(got, batch_results(ctx, handle=used)[3])
    used.close()


def test_strided_matrix_and_first_row_above_zero(ctx):
    got = batch_results(ctx)[3]
    for kw in (dict(ld=N + 9), dict(rows_before=5), dict(ld=2 * N + 1, rows_before=3)):
        assert same_items(got, batch_results(ctx, **kw)[3]), kw


def test_the_state_limit(ctx):
    """2048 states fill every slot of every lane and 2047 labels the label table; few frames"""
    g = ar.linear_hmm(_lib.AMX_ALIGN_MAX_STATES, N, 99)
    s = ar._gauss("limit5", 5)
    got, ioff, res, _ = device_bw(ctx, [g], [0, 5], s, max_acoustic_pruning=400.0)
    want = br.align_segment(g, s, "device", max_acoustic_pruning=400.0)
    assert not want["reached"]
    check_batch(got, ioff, res, [want], [0, 5], "limit")
    # reached: the same graph entered ten states before its end
    g2 = dict(g, initial=_lib.AMX_ALIGN_MAX_STATES - 10)
    s = ar._gauss("limit_reached", 12)
    got, ioff, res, _ = device_bw(ctx, [g2], [0, 12], s)
    want = br.align_segment(g2, s, "device")
    assert want["reached"] and want["n_items"] > 12
    check_batch(got, ioff, res, [want], [0, 12], "entered late")


def test_parallel_arcs_keep_their_labels_apart(ctx):
    c = all_cases()["parallel_arcs"]
    got, ioff, res, _ = device_bw(ctx, [c["graph"]], [0, len(c["scores"])], c["scores"])
    assert res[0]["reached"] and (np.diff(ioff) == 2).all() and (got["emission"] == got["label"] // 16).all()
    for f in range(len(c["scores"])):
        assert len(set(got["label"][ioff[f]:ioff[f + 1]])) == 2 and got["weight"][ioff[f]] >= got["weight"][ioff[f] + 1]


def test_nan_rule(ctx):
    """a NaN in a column the graph uses marks that segment only and is counted; a NaN in a column no arc reads changes nothing"""
    graphs, off, scores, got, _ = batch_results(ctx)
    i = ar.BATCH.index("variants")
    used = sorted({e for arcs in graphs[i]["arcs"] for _, e, _, _ in arcs})
    unused = [c for c in range(N) if c not in used]
    poisoned = scores.copy()
    poisoned[off[i]:off[i + 1], unused[0]] = np.nan
    g, o, res, counters = device_bw(ctx, graphs, off, poisoned)
    assert counters[0] == 0 and same_items(got, (g, o, res))
    poisoned = scores.copy()
    poisoned[off[i] + 4, used[2]] = np.nan
    g, o, res, counters = device_bw(ctx, graphs, off, poisoned)
    assert counters[0] == 1
    wants = [restated(n) if k != i else br.align_segment(graphs[i], poisoned[off[i]:off[i + 1]], "device") for k, n in enumerate(ar.BATCH)]
    assert wants[i]["nan"] and wants[i]["n_items"] == 0 and not res[i]["reached"]
    check_batch(g, o, res, wants, off, "poisoned")


def test_capacity_too_small(ctx):
    import rasr_amd
    torch = _torch()
    c = all_cases()["finals"]
    a = rasr_amd.BaumWelchAligner(ctx)
    ctx.use_torch_stream()
    items, _, res, _ = a.align([0, len(c["scores"])], [c["graph"]], torch.from_numpy(c["scores"]).cuda(), N)
    n = res[0]["n_items"]
    assert n == restated("finals")["n_items"] and len(items["frame"]) == n
    with pytest.raises(rasr_amd.AmxError, match="capacity %d is too small: the last call left %d items" % (n - 1, n)) as e:
        a.items("cuda", capacity=n - 1)
    assert e.value.status == _lib.AMX_ERR_INVALID
    more = a.items("cuda", weight_f64=False, capacity=n + 3)
    torch.cuda.synchronize()
    assert more["weight_f64"] is None and all(same(more[k][:n].cpu().numpy(), items[k].cpu().numpy()) for k in ("frame", "label", "emission", "weight"))
    a.close()


def test_the_item_store_grows(ctx):
    """the store starts at 4 * frames + 64 items: three frames of twelve items fit into the first store (76), eight such segments (288
    items against 4 * 24 + 64 = 160) make the call write a second time, with the same result"""
    arcs = [(0, 1 + i, i, 16 * i, 1.0) for i in range(12)] + [(1 + i, 1 + j, j, 16 * j, 1.0) for i in range(12) for j in range(12)]
    g = ar.graph(13, 0, {1 + i: 0.0 for i in range(12)}, arcs)
    s = np.full((3, N), 5, np.float32) + ar._gauss("grow", 3) / 100
    got, ioff, res, _ = device_bw(ctx, [g], [0, 3], s)
    want = br.align_segment(g, s, "device")
    assert want["n_items"] == res[0]["n_items"] == 36 <= 4 * 3 + 64
    check_batch(got, ioff, res, [want], [0, 3], "grow")
    wide = [g] * 8
    off = np.arange(9) * 3
    got, ioff, res, _ = device_bw(ctx, wide, off, np.concatenate([s] * 8))
    assert 8 * 36 > 4 * 24 + 64
    check_batch(got, ioff, res, [want] * 8, off, "grow, eight segments")


def test_every_refusal_returns_its_code_and_launches_nothing(ctx):
    import rasr_amd
    torch = _torch()
    small, big = ar.linear_hmm(3, N, 1), ar.linear_hmm(5, N, 2)
    n_small = sum(len(a) for a in small["arcs"])
    scores = torch.from_numpy(ar._gauss("refusals", 9)).cuda()
    a = rasr_amd.BaumWelchAligner(ctx)
    fan = ar.graph(2, 0, {1: 0.0}, [(0, 1, i % N, i % N, 1.0) for i in range(_lib.AMX_ALIGN_MAX_OUT_ARCS + 1)])
    too_many = ar.linear_hmm(_lib.AMX_ALIGN_MAX_STATES + 1, N, 3)
    n = _lib.AMX_BW_MAX_LABELS + 1
    labels = ar.graph(n // 64 + 2, 0, {1: 0.0}, [(1 + i // 64, 1, 3, i, 1.0) for i in range(n)])
    two = ar.graph(2, 0, {1: 0.0}, [(0, 1, 3, 40, 1.0), (1, 1, 4, 40, 1.0)])
    cases = [([small, big], dict(arc_target=(n_small + 2, 5)), _lib.AMX_ERR_INVALID, ("segment 1", "arc_target[%d] = 5" % (n_small + 2))),
             ([small, big], dict(arc_emission=(1, N)), _lib.AMX_ERR_INVALID, ("segment 0", "arc_emission[1] = %d" % N)),
             ([small, big], dict(initial_state=(0, 3)), _lib.AMX_ERR_INVALID, ("segment 0", "initial_state 3")),
             ([small, big], dict(arc_weight=(0, float("nan"))), _lib.AMX_ERR_INVALID, ("segment 0", "arc_weight[0]")),
             ([small, big], dict(final_weight=(2, float("nan"))), _lib.AMX_ERR_INVALID, ("segment 0", "final_weight of state 2")),
             ([small, fan], dict(), _lib.AMX_ERR_UNSUPPORTED, ("segment 1", "state 0 has 65 arcs")),
             ([small, too_many], dict(), _lib.AMX_ERR_UNSUPPORTED, ("segment 1", "2049 states")),
             ([small, labels], dict(), _lib.AMX_ERR_UNSUPPORTED, ("segment 1", "4097 distinct labels")),
             ([small, two], dict(), _lib.AMX_ERR_INVALID, ("segment 1", "label 40", "emission indices 3 and 4"))]
    for graphs, patch, status, words in cases:
        g = rasr_amd.BaumWelchAligner.graphs(graphs)
        for k, (i, v) in patch.items():
            g[k][i] = v
        ioff = torch.full((10,), -7, dtype=torch.int64, device="cuda")
        with pytest.raises(rasr_amd.AmxError) as e:
            a.align([0, 4, 9], g, scores, N, item_offsets_dev=ioff)
        assert e.value.status == status, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert (ioff == -7).all() and _lib.lib().amx_bw_n_items(a.h) == 0
    for kw, status, word in ((dict(use_partial_sums=1), _lib.AMX_ERR_UNSUPPORTED, "use_partial_sums"),
                             (dict(min_weight=0.01), _lib.AMX_ERR_UNSUPPORTED, "min_weight"),
                             (dict(n_best_pruning=10), _lib.AMX_ERR_UNSUPPORTED, "n_best_pruning"),
                             (dict(increment_factor=1.0), _lib.AMX_ERR_INVALID, "increment_factor")):
        with pytest.raises(rasr_amd.AmxError) as e:
            rasr_amd.BaumWelchAligner(ctx, **kw)
        assert e.value.status == status and word in str(e.value)
    # the handle still works
    s = scores.cpu().numpy()
    got, ioff, res, _ = device_bw(ctx, [small], [0, 9], s, handle=a)
    check_batch(got, ioff, res, [br.align_segment(small, s, "device")], [0, 9], "after the refusals")
    a.close()


def test_score_align_gather_accumulate_end_to_end(ctx):
    """amx_gmm_score_dev -> amx_bw_align_dev -> amx_bw_items_dev -> amx_gather_rows_dev -> amx_gmm_accumulate_weighted_dev, the matrix
    never on the host, against the oracle's scores -> the restatement's items -> the oracle's weighted accumulation at
    test_weighted_viterbi_accumulators' bar (f64 sums to rtol 1e-12 / atol 1e-9)"""
    import rasr_amd
    from oracle import OracleGmm
    from tests import synth
    torch = _torch()
    M, dim = 24, 16
    model = synth.gmm_cart(M, 1, 4, dim, seed=70)
    lens = (40, 25, 33)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(off[-1])
    x = np.random.Generator(np.random.PCG64(71)).standard_normal((T, dim)).astype(np.float32)
    graphs = [ar.linear_hmm(n, M, 72 + n) for n in (12, 9, 20)]
    sc = rasr_amd.GmmFeatureScorer(ctx, model)
    al = rasr_amd.BaumWelchAligner(ctx)
    ctx.use_torch_stream()
    xd = torch.from_numpy(x).cuda()
    scores = torch.empty((T, M), dtype=torch.float32, device="cuda")
    best = torch.empty((T, M), dtype=torch.int32, device="cuda")
    sc.score_dev(xd, T, scores, best)
    items, ioff, results, counters = al.align(off, graphs, scores, M)
    n = len(items["frame"])
    rows = rasr_amd.gather_rows(ctx, xd, items["frame"])
    chosen = best[items["frame"].long(), items["emission"].long()].contiguous()
    acc = torch.zeros(sc.accumulator_size(), dtype=torch.float64, device="cuda")
    sc.accumulate_weighted_dev(rasr_amd.AMX_GMM_VITERBI, rows, n, items["emission"], items["weight_f64"], chosen, 0, acc)
    torch.cuda.synchronize()
    o = OracleGmm(model)
    osc, obest = o.score(x)
    wants = [br.align_segment(g, osc[off[i]:off[i + 1]], "device") for i, g in enumerate(graphs)]
    assert all(w["reached"] for w in wants) and counters[0] == 0 and n > T
    f, l, e, w, wo, share = br.flat_items(wants, off)
    got = {k: v.cpu().numpy() for k, v in items.items()}
    check_batch(got, ioff.cpu().numpy(), results, wants, off, "end to end")
    assert np.array_equal(rows.cpu().numpy(), x[f])
    want = o.accumulate_weighted(0, x[f], e.astype(np.uint32), w.astype(np.float64), obest[f, e])
    assert np.allclose(acc.cpu().numpy(), want, rtol=1e-12, atol=1e-9)
    nk = int(model["mix_offsets"][-1])
    assert abs(acc.cpu().numpy()[:nk].sum() - T) <= n * 2.0 ** -24                # the weights of a frame sum to one
    al.close()
