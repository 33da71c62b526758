"""The wide alignment cases of tests/wide_graphs.py without a GPU: on the restatements alone (tests/align_reference.py,
tests/bw_reference.py, held to the reference's recorded results by tests/test_align.py and tests/test_bw.py) the inputs do what
tests/test_align_wide_gpu.py relies on.  One block per GPU case: the active set passes every band of the rank scan, the pruning variants
prune and count passes, ties decide above rank 511 (the arc order reversed: same score, other labels), the item counts pass every sort
size, emissions, labels and arc counts are the named ones, and the share of item weights that the one-ulp exemption of
tests/test_bw_gpu.py covers stays within the project's cap of 1 % (tests/test_posterior_gpu.py).  No kernel runs here."""
import numpy as np
import pytest

from rasr_amd import _lib
from tests import align_reference as ar
from tests import bw_reference as br
from tests import wide_graphs as wg
from tests.test_align import host_call, same
from tests.test_bw import POSTERIOR_BAR

EXEMPT_CAP = 0.01     # tests/test_posterior_gpu.py
_VITERBI, _BW, _EXECUTED = {}, {}, {}


def segments(c):
    return [(g, c["scores"][a:b]) for g, a, b in zip(c["graphs"], c["off"], c["off"][1:])]


def viterbi(name):
    """the Viterbi restatement's results of a case's segments, computed once per session and never changed"""
    if name not in _VITERBI:
        c = wg.case(name)
        _VITERBI[name] = [ar.align_segment(g, rows, **c["cfg"]) for g, rows in segments(c)]
    return _VITERBI[name]


def baum_welch(name):
    """the Baum-Welch restatement's results (device order) of a case's segments, computed once per session and never changed"""
    if name not in _BW:
        c = wg.case(name)
        _BW[name] = [br.align_segment(g, rows, "device", **c["cfg"]) for g, rows in segments(c)]
    return _BW[name]


def executed_passes(name):
    """the passes the device has to run for a case's call (a pass that pruned nothing ends the work), computed once per session"""
    if name not in _EXECUTED:
        c = wg.case(name)
        _EXECUTED[name] = [ar.count_executed_passes(g, rows, **c["cfg"]) for g, rows in segments(c)]
    return sum(_EXECUTED[name])


def exempt_share(results):
    """the share of the live items whose f64 share lies within the bar of a boundary between two f32 values"""
    shares = [np.asarray(f, np.float64) for r in results if "shares" in r for f in r["shares"] if len(f)]
    return float(np.mean(br.midpoint_distance(np.concatenate(shares)) <= POSTERIOR_BAR)) if shares else 0.0


def item_counts(name):
    return [len(f) for r in baum_welch(name) for f in r["items"]]


def new_and_kept(graph, rows, threshold):
    """per frame of one Viterbi pass: the hypotheses before and after pruning"""
    frames, kept, _ = ar.one_pass(graph, rows, threshold)
    new = [len({t for h in hyps for t, _, _, _ in graph["arcs"][h[0]]}) for hyps in frames[:-1]]
    return new, kept


@pytest.mark.parametrize("name", wg.BOTH)
def test_every_case_is_reached_without_nan_and_within_the_exempt_cap(name):
    v, b = viterbi(name), baum_welch(name)
    assert all(r["reached"] and not r["nan"] for r in v) and all(r["reached"] and not r["nan"] for r in b), name
    assert sum(r["n_items"] for r in b) >= len(wg.case(name)["scores"]) > 0
    assert exempt_share(b) <= EXEMPT_CAP, name


def test_active_set_passes_every_band_of_the_rank_scan():
    """8 ranks per lane: wave 0 scans ranks 0 .. 511, the waves behind it need its sum; 2048 is every slot of every lane"""
    S = _lib.AMX_ALIGN_MAX_STATES
    assert [g["n_states"] for g in wg.case("active")["graphs"]] == [S, S] and S == 1 + sum(wg.ACTIVE_WIDTHS)
    for r in viterbi("active") + baum_welch("active"):
        n = r["survivors"]
        assert (n <= 8).any() and ((n > 8) & (n <= 512)).any() and ((n > 512) & (n <= 1024)).any() and (n > 1536).any() and (n == S).any()


def test_pruning_variant_prunes_above_rank_511_in_its_last_pass():
    c = wg.case("active_pruned")
    for (g, rows), v, b in zip(segments(c), viterbi("active_pruned"), baum_welch("active_pruned")):
        assert v["n_iterations"] == b["n_iterations"] == 3 and float(v["last_threshold"]) == float(b["last_threshold"]) == 8.0
        new, kept = new_and_kept(g, rows, v["last_threshold"])
        assert kept == v["survivors"].tolist()
        assert any(k > 512 and k < n for n, k in zip(new, kept))
        frames, counts, pruned = br.one_pass(g, rows, b["last_threshold"], "device")
        assert pruned and counts == b["survivors"].tolist() and max(counts) > 512 and max(counts) < g["n_states"]
        assert b["passes_run"] == 3
    assert executed_passes("active_pruned") == 3 * len(c["graphs"])


def test_counted_variant_counts_passes_it_does_not_run():
    c = wg.case("active_counted")
    for (g, rows), v, b in zip(segments(c), viterbi("active_counted"), baum_welch("active_counted")):
        assert v["n_iterations"] == b["n_iterations"] == 7 and float(v["last_threshold"]) == 64.0
        assert 1 < b["passes_run"] < 7
    assert len(c["graphs"]) < executed_passes("active_counted") < 7 * len(c["graphs"])


def test_ties_decide_above_rank_511():
    """the arc order inside every source state reversed: the alignment score keeps its bits, the labels change on a frame with more
    than 512 active hypotheses.  Only the list positions tell the two orders apart: the GPU test can fail on a wrong rank there."""
    for name in ("active", "active_pruned"):
        c = wg.case(name)
        for (g, rows), want in zip(segments(c), viterbi(name)):
            other = ar.align_segment(wg.reversed_arcs(g), rows, **c["cfg"])
            assert same(np.float32(other["score"]), np.float32(want["score"])) and np.array_equal(other["survivors"], want["survivors"]), name
            differs = other["label"] != want["label"]
            assert (differs & (want["survivors"] > 512)).any(), name


def test_fan64_has_a_state_with_64_arcs_whose_last_one_decides():
    """the entry's 64th arc (ordinal 63, bit 63 of its mask) moved in front of the others: same score, other labels"""
    c = wg.case("fan64")
    for (g, rows), want in zip(segments(c), viterbi("fan64")):
        out = g["arcs"][0]
        assert len(out) == _lib.AMX_ALIGN_MAX_OUT_ARCS == 64 and len({t for t, _, _, _ in out}) == 64 and want["survivors"][0] == 64
        # the 64 targets tie in groups: few distinct scores among them
        first = ar.one_pass(g, rows[:1], 50.0)[0][1]
        assert len(first) == 64 and len({float(h[1]) for h in first}) <= 6
        for other in (dict(g, arcs=[out[-1:] + out[:-1]] + g["arcs"][1:]), wg.reversed_arcs(g, states={0})):
            r = ar.align_segment(other, rows, **c["cfg"])
            assert same(np.float32(r["score"]), np.float32(want["score"])) and (r["label"] != want["label"]).any()


def test_funnel_walks_2047_arcs_of_one_label_into_one_state():
    g = wg.case("funnel")["graphs"][0]
    into = br.by_target(g)[g["n_states"] - 1]
    assert g["n_states"] == 2048 and len(into) == 2047 and len({l for _, _, l, _ in into}) == 1 and len({s for s, _, _, _ in into}) == 2047
    label = into[0][2]
    assert not [1 for s, arcs in enumerate(g["arcs"]) for t, _, l, _ in arcs if l == label and t != g["n_states"] - 1]
    v, b = viterbi("funnel")[0], baum_welch("funnel")[0]
    assert v["survivors"][-2] > 1536 and v["label"][-1] == label
    assert [(l, float(w)) for l, _, w in b["items"][-1]] == [(label, 1.0)]


@pytest.mark.parametrize("name, states, emissions, labels", [("em256", 300, 256, 256), ("em257", 300, 257, 300), ("em4096", 1500, 4096, 4096),
                                                             ("limits", wg.LIMIT_STATES, wg.LIMIT_EMISSIONS, wg.LIMIT_LABELS)])
def test_emissions_and_labels_are_the_named_ones(name, states, emissions, labels):
    g = wg.case(name)["graphs"][0]
    used, labs = wg.used_columns(g), wg.used_labels(g)
    assert g["n_states"] == states and len(used) == emissions and len(labs) == labels
    assert used[0] == 0 and used[-1] == wg.N_COLUMNS - 1
    order = [l for arcs in g["arcs"] for _, _, l, _ in arcs]
    assert order != sorted(order) and all(l // 16 == e for arcs in g["arcs"] for _, e, l, _ in arcs)
    rows = wg.case(name)["scores"]
    assert np.isnan(rows[:, [c for c in range(wg.N_COLUMNS) if c not in set(used)]]).all() and not np.isnan(rows[:, used]).any()


def test_limits_are_the_documented_ones_and_a_frame_has_4096_items():
    g = wg.case("limits")["graphs"][0]
    assert (g["n_states"], len(wg.used_columns(g)), len(wg.used_labels(g))) == (_lib.AMX_ALIGN_MAX_STATES, _lib.AMX_ALIGN_MAX_EMISSIONS, _lib.AMX_BW_MAX_LABELS)
    assert wg.n_arcs(g) >= 4096 and 4 <= len(wg.case("limits")["scores"]) <= 6
    assert _lib.AMX_BW_MAX_LABELS in item_counts("limits")
    assert (viterbi("limits")[0]["survivors"] == _lib.AMX_ALIGN_MAX_STATES).any()


def test_refused_graph_has_one_emission_too_many():
    g = wg.refused()
    assert len(wg.used_columns(g)) == _lib.AMX_ALIGN_MAX_EMISSIONS + 1
    st, msg = host_call([g], [0, 4], n_columns=wg.N_COLUMNS)
    assert st == _lib.AMX_ERR_UNSUPPORTED and "4097 emission indices" in msg and "limit of 4096" in msg


def test_item_counts_pass_every_sort_size():
    """the frame's items are sorted over the next power of two: 64, 512, 1024, 2048 and (limits) 4096 keys, the padding behind 257, 513
    and 1025 items; 60 items of one weight are ordered by label alone"""
    counts = item_counts("items")
    assert counts == [64, 257, 513, 1025, 60, 60, 60]
    every = counts + item_counts("limits") + item_counts("active")
    assert any(13 <= n <= 256 for n in every) and any(257 <= n <= 512 for n in every) and any(513 <= n <= 1024 for n in every) and 4096 in every
    assert any(n > 2 and (n - 1) & (n - 2) == 0 for n in counts)
    for frame in baum_welch("items")[1]["items"]:
        w = np.array([x[2] for x in frame], np.float32)
        assert len(frame) >= 50 and len(set(w.view(np.uint32).tolist())) == 1
        assert [x[0] for x in frame] == sorted(x[0] for x in frame)
    # the integer cases tie as well, where the graph is not symmetric
    assert max(np.unique(np.array([x[2] for x in f], np.float32).view(np.uint32), return_counts=True)[1].max() for f in baum_welch("limits")[0]["items"]) >= 50


def test_boundary_pair_has_the_launch_sites_arc_counts():
    """align.hip, amx_align_viterbi_dev: roundup16(32 S + 4 + 8 E) + 16 n_in <= 128 KB puts the arcs into LDS"""
    fit, spill = wg.case("arcs_fit")["graphs"][0], wg.case("arcs_spill")["graphs"][0]
    n = wg.arcs_that_fit(wg.FIT_STATES, wg.FIT_EMISSIONS)
    assert n == 6131 and (wg.n_arcs(fit), wg.n_arcs(spill)) == (n, n + 1)
    for g in (fit, spill):
        assert g["n_states"] == wg.FIT_STATES and len(wg.used_columns(g)) == wg.FIT_EMISSIONS
    fixed = (32 * wg.FIT_STATES + 4 + 8 * wg.FIT_EMISSIONS + 15) // 16 * 16
    assert fixed + 16 * n <= 128 * 1024 < fixed + 16 * (n + 1)
    # the limits' arcs never fit: at 2048 states and 4096 emissions 2047 arcs would
    assert wg.arcs_that_fit(wg.LIMIT_STATES, wg.LIMIT_EMISSIONS) == 2047 < wg.n_arcs(wg.case("limits")["graphs"][0])


def test_mixed_batch_holds_four_recorded_cases_around_the_limits():
    c = wg.case("mixed_batch")
    small = ar.cases()
    assert len(c["graphs"]) == 5 and c["graphs"][2] is wg.case("limits")["graphs"][0]
    for i, n in zip((0, 1, 3, 4), wg.SMALL):
        assert same(c["scores"][c["off"][i]:c["off"][i + 1], :ar.N_COLUMNS], small[n]["scores"]) and not small[n]["cfg"]
        want = ar.align_segment(small[n]["graph"], small[n]["scores"])
        assert np.array_equal(viterbi("mixed_batch")[i]["label"], want["label"]) and same(np.float32(viterbi("mixed_batch")[i]["score"]), np.float32(want["score"]))


def test_long_call_passes_every_chunk_of_the_scan():
    """bw_scan_kernel takes 256 rows per trip and carries their sum, zeroes the rows below the call 256 at a time and sums the items of
    256 segments at a time"""
    c = wg.case("long_call")
    lens = np.diff(c["off"])
    assert len(lens) == 300 > 256 and c["off"][-1] > 600 > 2 * 256 and set(lens.tolist()) == {0, 1, 2, 3}
    counts = np.array(item_counts("long_call"))
    assert len(counts) == c["off"][-1] and counts[:256].sum() > 0 and counts[512:].sum() > 0
    assert all(r["n_items"] == 0 for r, n in zip(baum_welch("long_call"), lens) if n == 0)
