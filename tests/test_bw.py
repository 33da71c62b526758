"""Baum-Welch alignment without a GPU.  The restatement of tests/bw_reference.py in reference order against the reference's own run
(tests/golden/ref_bw.npz, written by tests/golden/make_bw_golden.py from the reference's text in both of its builds):
  bit for bit   score, reached flag, iterations, last threshold, survivors per frame; LogSemiring::collect on 4096 pairs; bw[initial];
                -log p of every arc as narrowed to f32, in the recorded order; the key sets (time, label); the combined -log p of every
                key with one or two arcs; the item weights (f64) computed from the recorded combined values
  exactly, but  a key with three or more arcs is collected in the order std::sort leaves them in, which the reference does not define
  one of a set  and three collects do not commute: the recorded value must be what ONE order of the restatement's arcs gives
Then the restatement in device order against the same fixture: discrete results and key sets as far as f32 holds them, weights within
the bars the generator MEASURED (bar_a, bar_r: twice the worst deviation of the reference's weights from an all-f64 evaluation), its two
orders against each other, the properties of a soft alignment, the handle's host logic through the library, and the stand-alone host
program under the host sanitizers.  No kernel runs here.

Key sets.  The reference's item weights are f64 (Mm::Weight) and anything above 0 is kept; the library's are f32 (include/amx.h).  An item
whose weight has no f32 value above 0 (below 2^-149) cannot be there: the device order's keys are a subset of the reference's, and
every reference item of at least 2^-149 is among them.  The generator's third condition (no kept weight in (0, 1e-30)) does not hold in
eleven of the cases and is recorded in the fixture, not assumed.

The score bar between the two orders.  Both round a state's score to f32 once per candidate sum; the reference order then rounds once
more per collect (a state with k candidates: k - 1 times), the device order once per state.  The log-sum passes errors of its inputs on
with weights that sum to 1, so a frame adds at most (k + 1) / 2 ulp of the score's magnitude in either order: after T frames and the final
collect the two scores lie within (T + 1) * (k + 1) ulp, k the largest number of arcs into a state."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from rasr_amd import _lib
from tests import align_reference as ar
from tests import bw_reference as br
from tests.test_align import all_cases, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_bw.npz")
INT_MAX = ar.INT_MAX
F32_SMALLEST = 2.0 ** -149      # the smallest f32 above 0
POSTERIOR_BAR = 1e-11            # the project's bar on f64 posterior quantities

_RESTATED = {}


def restated(name, order="device"):
    """the restatement's result of a case, computed once per session and never changed"""
    if (name, order) not in _RESTATED:
        c = all_cases()[name]
        _RESTATED[name, order] = br.align_segment(c["graph"], c["scores"], order, **c["cfg"])
    return _RESTATED[name, order]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def score_bar(name):
    """(T + 1) * (k + 1) ulp of the score's magnitude, see above"""
    c = all_cases()[name]
    k = max(len(a) for a in br.by_target(c["graph"]))
    return (len(c["scores"]) + 1) * (k + 1)


def check_search_against_fixture(golden, name, r, exact_score):
    """the recorded fields of one case: in every bit, or (a result in device order) the score within score_bar"""
    g = {f: golden["off/%s/%s" % (name, f)] for f in ("survivors", "score", "reached", "n_iterations", "last_threshold", "average_states", "state_sum")}
    assert bool(r["reached"]) == bool(g["reached"]) and r["n_iterations"] == int(g["n_iterations"]), name
    assert same(np.float32(r["last_threshold"]), g["last_threshold"]) and r["state_sum"] == int(g["state_sum"]), name
    assert same(np.float64(r["average_states"]), g["average_states"]) or (np.isnan(r["average_states"]) and np.isnan(g["average_states"])), name
    if "survivors" in r:
        assert np.array_equal(r["survivors"], g["survivors"]), name
    if exact_score or not g["reached"]:
        assert same(np.float32(r["score"]), g["score"]), name
    else:
        assert abs(float(r["score"]) - float(g["score"])) <= score_bar(name) * float(np.spacing(np.abs(g["score"]))), name


def fixture_items(golden, name, what="items"):
    """{(time, label): value} of one case"""
    k = "off/%s/%s_" % (name, what)
    return {(int(t), int(l)): v for t, l, v in zip(golden[k + "time"], golden[k + "label"], golden[k + "value"])}


def check_items_against_reference(golden, got, ref, what):
    """got, ref: {(time, label): weight}; ref the reference's f64 weights.  Keys as far as f32 holds them, weights within the measured bars"""
    a, r = float(golden["bar_a"]), float(golden["bar_r"])
    assert set(got) <= set(ref), what
    assert not [q for q, w in ref.items() if w >= F32_SMALLEST and q not in got], what
    for q, w in got.items():
        assert abs(float(w) - float(ref[q])) <= a + r * float(ref[q]), (what, q)


def item_dict(r):
    return {(f, l): w for f, frame in enumerate(r["items"]) for l, _, w in frame}


# ------------------------------------------------------------------ the restatement

def test_fixture_holds_what_the_generator_says(golden):
    """both builds of the reference agree in every bit, the inputs are the cases the tests walk, the compiled collect calls the f64
    library functions, and no case sits near a decision"""
    assert not [k for k in golden if k.startswith("fma/")] and golden["fma_differs"].tolist() == [""] and int(golden["collect_probe_fma_differs"]) == 0
    assert golden["collect_calls/off"].tolist() == ["exp", "log1p"] == golden["collect_calls/fma"].tolist()
    assert golden["restatement_unequal"].tolist() == [""]
    assert float(golden["smallest_margin_ulp"]) >= 32 and float(golden["smallest_almost_equal_ratio"]) >= 64
    names = sorted(k.split("/")[1] for k in golden if k.startswith("off/") and k.endswith("/score"))
    assert names == sorted(all_cases())
    for name, c in all_cases().items():
        assert same(golden["in/%s/scores" % name], np.ascontiguousarray(c["scores"], np.float32)), name
        assert np.array_equal(golden["in/%s/arc_weight" % name], np.array([w for a in c["graph"]["arcs"] for _, _, _, w in a], np.float32)), name
    assert not golden["off/unreachable/reached"] and same(golden["off/unreachable/score"], ar.F32_MAX) and int(golden["off/unreachable/n_iterations"]) == 123


def test_fixture_holds_the_measured_bars_and_the_third_condition(golden):
    """(a, r) are what the generator measured, in the range the issue expected (1.1e-7 absolute, 6.5e-6 relative on six cases); the
    third condition fails in eleven cases and every item that only the reference keeps has no f32 weight"""
    assert 0 < float(golden["bar_a"]) < 2.2e-7 and 0 < float(golden["bar_r"]) < 2 * 1.3e-5
    tiny = {n: int(golden["tiny_items/" + n]) for n in all_cases()}
    assert sum(1 for v in tiny.values() if v) == 11 and tiny["lin130_T80"] == 1291 and tiny["parallel_arcs"] == 0
    assert float(golden["largest_weight_without_f32_value"]) < F32_SMALLEST


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_restatement_posteriors_and_items_equal_the_reference(golden, name):
    r = restated(name, "reference")
    raw_t, raw_l, raw_v = (golden["off/%s/raw_%s" % (name, f)] for f in ("time", "label", "value"))
    if not r["reached"] or not len(all_cases()[name]["scores"]):
        assert len(raw_t) == 0 and not fixture_items(golden, name) and r["n_items"] == 0
        return
    assert same(np.float64(r["log_total"]), golden["off/%s/bw_initial" % name]), name
    assert abs(float(golden["off/%s/fw_final" % name]) - r["log_total"]) <= POSTERIOR_BAR * (1 + abs(r["log_total"])), name
    assert [t for t, _, _ in r["raw"]] == raw_t.tolist() and [l for _, l, _ in r["raw"]] == raw_l.tolist(), name
    assert same(np.array([v for _, _, v in r["raw"]], np.float32), raw_v), name
    arcs = {}
    for t, l, v in r["raw"]:
        arcs.setdefault((t, l), []).append(v)
    mine, ref = {(t, l): v for t, l, v in r["combined"]}, fixture_items(golden, name, "combined")
    assert set(mine) == set(ref) == set(arcs), name
    for q, v in ref.items():
        if len(arcs[q]) <= 2:
            assert same(np.float32(mine[q]), np.float32(v)), (name, q)
        else:
            orders = set()
            for p in itertools.permutations(arcs[q]):
                acc = p[0]
                for x in p[1:]:
                    acc = br.collect32(acc, x)
                orders.add(np.float32(acc).tobytes())
            assert np.float32(v).tobytes() in orders, (name, q)
    # the item arithmetic behind combineItems, on the recorded combined values
    items = fixture_items(golden, name)
    emission = {l: e for a in all_cases()[name]["graph"]["arcs"] for _, e, l, _ in a}
    assert set(item_dict(r)) == set(items), name
    for f in sorted({t for t, _ in ref}):
        frame = br.items_from_combined({l: np.float32(v) for (t, l), v in ref.items() if t == f}, emission)
        assert {(f, l) for l, _, _ in frame} == {q for q in items if q[0] == f}, (name, f)
        for l, _, w in frame:
            assert same(np.float64(w), np.float64(items[f, l])), (name, f, l)


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_device_order_items_against_the_reference(golden, name):
    d = restated(name, "device")
    check_items_against_reference(golden, item_dict(d), fixture_items(golden, name), name)
    if d["reached"] and len(all_cases()[name]["scores"]):
        ref = float(golden["off/%s/bw_initial" % name])
        assert abs(d["log_total"] - ref) <= POSTERIOR_BAR * (1 + abs(ref)), name
        # the all-f64 shares before the rounding to f32, too
        shares = {(f, l): s for f, (its, shs) in enumerate(zip(d["items"], d["shares"])) for (l, _, _), s in zip(its, shs)}
        check_items_against_reference(golden, shares, fixture_items(golden, name), name)


def test_collect_equals_the_references(golden):
    pairs, want = golden["collect_probe_in"], golden["collect_probe_out"]
    got = np.array([br.collect32(a, b) for a, b in pairs], np.float32)
    assert same(got, want)


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_restatement_in_reference_order_equals_the_reference(golden, name):
    check_search_against_fixture(golden, name, restated(name, "reference"), exact_score=True)


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_restatement_in_device_order_against_the_reference(golden, name):
    check_search_against_fixture(golden, name, restated(name, "device"), exact_score=False)


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_the_two_orders_agree(golden, name):
    d, r = restated(name, "device"), restated(name, "reference")
    for k in ("reached", "n_iterations", "state_sum", "nan"):
        assert d[k] == r[k], (name, k)
    assert same(np.float32(d["last_threshold"]), np.float32(r["last_threshold"])) and np.array_equal(d["survivors"], r["survivors"]), name
    if d["reached"]:
        assert abs(float(d["score"]) - float(r["score"])) <= score_bar(name) * float(np.spacing(np.float32(abs(r["score"])))), name
        assert abs(d["log_total"] - r["log_total"]) <= POSTERIOR_BAR * (1 + abs(r["log_total"])), name
    else:
        assert same(np.float32(d["score"]), ar.F32_MAX) and same(np.float32(r["score"]), ar.F32_MAX) and d["n_items"] == r["n_items"] == 0, name
    check_items_against_reference(golden, item_dict(d), {q: float(w) for q, w in item_dict(r).items()}, name)


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_weights_of_a_frame_sum_to_one_and_items_are_ordered(name):
    r = restated(name)
    T = len(all_cases()[name]["scores"])
    assert len(r["items"]) == T and r["n_items"] == sum(len(f) for f in r["items"])
    for f, items in enumerate(r["items"]):
        if not r["reached"]:
            assert not items
            continue
        assert items, (name, f)
        # every weight is one rounding of an exact share: n roundings of at most half an f32 ulp of 1
        assert abs(sum(float(w) for _, _, w in items) - 1.0) <= len(items) * 2.0 ** -24, (name, f)
        keys = [(-float(w), l) for l, _, w in items]
        assert keys == sorted(keys) and len({l for l, _, _ in items}) == len(items), (name, f)
        assert all(w > 0 and w.dtype == np.float32 for _, _, w in items)


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_total_flow_is_not_above_the_best_path(name):
    c = all_cases()[name]
    r, v = restated(name), ar.align_segment(c["graph"], c["scores"], **c["cfg"])
    assert r["reached"] == v["reached"], name
    if r["reached"]:
        assert r["log_total"] <= float(v["score"]) + 1e-3 and float(r["score"]) <= float(v["score"]) + 1e-3, name
        # the f32 score of the search and the f64 total describe the same flow: f32 roundings of a value of this size, one per frame
        T = max(len(c["scores"]), 1)
        assert abs(float(r["score"]) - r["log_total"]) <= (T + 1) * float(np.spacing(np.float32(abs(r["score"])))), name


@pytest.mark.parametrize("name", ["defaults_gauss", "variants", "finals", "parallel_arcs", "lin3_T37"])
def test_one_surviving_path_is_the_viterbi_alignment_with_weight_one(name):
    """a threshold below the gap between the best and the second candidate of every frame leaves one hypothesis per frame; where that
    path ends in a final state its items are the Viterbi alignment's labels, each with weight 1"""
    c = all_cases()[name]
    cfg = dict(c["cfg"], min_acoustic_pruning=1e-3, max_acoustic_pruning=1e-3, increment_factor=1.0)
    for order in ("device", "reference"):
        r = br.align_segment(c["graph"], c["scores"], order, **cfg)
        v = ar.align_segment(c["graph"], c["scores"], **cfg)
        assert r["reached"] == v["reached"] and (r["survivors"] <= 1).all(), (name, order)
        if r["reached"]:
            assert [[(l, e, float(w)) for l, e, w in f] for f in r["items"]] == [[(int(l), int(e), 1.0)] for l, e in zip(v["label"], v["emission"])], (name, order)
            assert same(np.float32(r["score"]), np.float32(v["score"])), (name, order)
    # at least one of these cases keeps its single path to the end
    assert any(br.align_segment(all_cases()[n]["graph"], all_cases()[n]["scores"], "device", **dict(all_cases()[n]["cfg"], min_acoustic_pruning=1e-3,
                                                                                                   max_acoustic_pruning=1e-3, increment_factor=1.0))["reached"]
               for n in ("variants", "finals", "parallel_arcs", "lin3_T37"))


def test_parallel_arcs_keep_their_labels_apart():
    """two arcs between the same states with two labels on two emissions: two items per frame"""
    r = restated("parallel_arcs")
    assert r["reached"] and all(len(f) == 2 for f in r["items"])
    assert all(e == l // 16 for f in r["items"] for l, e, _ in f)


def test_log_semiring_collect():
    assert br.collect32(ar.F32_MAX, 3.0) == np.float32(3) and br.collect32(3.0, ar.F32_MAX) == np.float32(3)
    assert same(br.collect32(2.0, 2.0), np.float32(2 - np.log1p(1.0)))
    assert abs(br.logsum64([2.0, 2.0, 2.0]) - (2 - np.log(3))) < 1e-15 and br.logsum64([5.0]) == 5.0 and br.logsum64([]) is None
    with pytest.raises(br.NanMet):
        br.logsum64([float("inf"), float("inf")])


def test_nan_ends_the_segment():
    c = all_cases()["variants"]
    s = c["scores"].copy()
    s[5, 4] = np.nan
    for order in ("device", "reference"):
        r = br.align_segment(c["graph"], s, order)
        assert r["nan"] and not r["reached"] and r["n_items"] == 0 and r["n_iterations"] == 1 and same(np.float32(r["score"]), ar.F32_MAX)


# ------------------------------------------------------------------ the handle's host logic

def create(**kw):
    L = _lib.lib()
    cfg = _lib.BwCfg()
    L.amx_bw_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    st = L.amx_bw_create(None, C.byref(cfg), C.byref(h))
    return L, h, st, L.amx_last_error().decode()


def test_default_configuration_is_the_aligners():
    L = _lib.lib()
    cfg = _lib.BwCfg()
    L.amx_bw_default_cfg(C.byref(cfg))
    assert (cfg.min_acoustic_pruning, cfg.increment_factor, cfg.min_average_number_of_states, cfg.increase_until_no_score_difference, cfg.n_best_pruning,
            cfg.score_scale, cfg.min_weight, cfg.use_partial_sums) == (50.0, 2.0, 0.0, 1, INT_MAX, 1.0, 0.0, 0)
    assert same(np.float32(cfg.max_acoustic_pruning), ar.F32_MAX)


@pytest.mark.parametrize("kw, status, words", [
    (dict(use_partial_sums=1), _lib.AMX_ERR_UNSUPPORTED, ("amx_bw_create", "use_partial_sums 1")),
    (dict(use_partial_sums=2), _lib.AMX_ERR_INVALID, ("use_partial_sums 2",)),
    (dict(min_weight=1e-3), _lib.AMX_ERR_UNSUPPORTED, ("min_weight 0.001",)),
    (dict(min_weight=-1.0), _lib.AMX_ERR_INVALID, ("min_weight -1",)),
    (dict(min_weight=float("nan")), _lib.AMX_ERR_INVALID, ("min_weight",)),
    (dict(n_best_pruning=100), _lib.AMX_ERR_UNSUPPORTED, ("amx_bw_create", "n_best_pruning 100")),
    (dict(min_acoustic_pruning=200.0, max_acoustic_pruning=100.0), _lib.AMX_ERR_INVALID, ("min_acoustic_pruning=200", "max_acoustic_pruning=100")),
    (dict(increment_factor=1.0), _lib.AMX_ERR_INVALID, ("increment_factor=1", "Inconsistent")),
    (dict(increment_factor=0.5, max_acoustic_pruning=100.0), _lib.AMX_ERR_INVALID, ("increment_factor=0.5",)),
    (dict(min_acoustic_pruning=0.0), _lib.AMX_ERR_INVALID, ("min_acoustic_pruning 0",)),
    (dict(min_acoustic_pruning=float("nan")), _lib.AMX_ERR_INVALID, ("not a number",)),
    (dict(increment_factor=1.00001), _lib.AMX_ERR_UNSUPPORTED, ("increment_factor", "limit of 4096 passes")),
])
def test_every_refused_configuration_names_its_parameter(kw, status, words):
    L, h, st, msg = create(**kw)
    assert st == status and not h.value, msg
    for w in words:
        assert w in msg, msg


def test_accepted_configurations():
    for kw in (dict(), dict(min_acoustic_pruning=80.0, max_acoustic_pruning=80.0, increment_factor=1.0), dict(increment_factor=1.01, max_acoustic_pruning=1e6),
               dict(score_scale=0.37, min_average_number_of_states=6.0, increase_until_no_score_difference=0), dict(min_weight=float(ar.F32_DELTA))):
        L, h, st, msg = create(**kw)
        assert st == 0, (kw, msg)
        L.amx_bw_destroy(h)


def test_the_viterbi_handle_still_refuses_the_mode_and_points_here():
    L = _lib.lib()
    cfg = _lib.AlignCfg()
    L.amx_align_default_cfg(C.byref(cfg))
    cfg.mode = _lib.AMX_ALIGN_BAUM_WELCH
    h = C.c_void_p()
    assert L.amx_align_create(None, C.byref(cfg), C.byref(h)) == _lib.AMX_ERR_UNSUPPORTED and not h.value
    msg = L.amx_last_error().decode()
    assert "mode" in msg and "baum-welch" in msg and "amx_bw_create" in msg


def host_call(graphs, frame_offsets, n_columns=ar.N_COLUMNS, **patch):
    """amx_bw_align_dev on a handle without a context: the checks run, then the call stops with AMX_ERR_STATE before any device work"""
    import rasr_amd
    a = rasr_amd.BaumWelchAligner(None)
    g = rasr_amd.BaumWelchAligner.graphs(graphs)
    for k, (i, v) in patch.items():
        g[k] = g[k].copy()
        g[k][i] = v
    try:
        a.align(frame_offsets, g, None, n_columns)
    except rasr_amd.AmxError as e:
        return e.status, str(e)
    finally:
        a.close()
    return 0, ""


def test_graph_checks_name_segment_and_index_and_launch_nothing():
    small, big = ar.linear_hmm(3, ar.N_COLUMNS, 1), ar.linear_hmm(5, ar.N_COLUMNS, 2)
    assert host_call([small, big], [0, 4, 9])[0] == _lib.AMX_ERR_STATE                       # a valid batch reaches the context check
    n_small = sum(len(a) for a in small["arcs"])
    for patch, status, words in (
            (dict(arc_target=(n_small + 2, 5)), _lib.AMX_ERR_INVALID, ("amx_bw_align_dev", "segment 1", "arc_target[%d] = 5" % (n_small + 2))),
            (dict(arc_emission=(0, ar.N_COLUMNS)), _lib.AMX_ERR_INVALID, ("segment 0", "arc_emission[0] = %d" % ar.N_COLUMNS)),
            (dict(initial_state=(1, 5)), _lib.AMX_ERR_INVALID, ("segment 1", "initial_state 5")),
            (dict(arc_weight=(n_small, float("nan"))), _lib.AMX_ERR_INVALID, ("segment 1", "arc_weight[%d]" % n_small, "not a number")),
            (dict(final_weight=(2, float("nan"))), _lib.AMX_ERR_INVALID, ("segment 0", "final_weight of state 2"))):
        st, msg = host_call([small, big], [0, 4, 9], **patch)
        assert st == status, (patch, msg)
        for w in words:
            assert w in msg, msg
    st, msg = host_call([small, big], [0, 4, 3])
    assert st == _lib.AMX_ERR_INVALID and "frame offsets decrease at segment 1" in msg
    st, msg = host_call([small, ar.linear_hmm(_lib.AMX_ALIGN_MAX_STATES + 1, ar.N_COLUMNS, 3)], [0, 2, 4])
    assert st == _lib.AMX_ERR_UNSUPPORTED and "segment 1" in msg and "limit of 2048 states" in msg
    fan = ar.graph(2, 0, {1: 0.0}, [(0, 1, i % ar.N_COLUMNS, i % ar.N_COLUMNS, 1.0) for i in range(_lib.AMX_ALIGN_MAX_OUT_ARCS + 1)])
    st, msg = host_call([fan], [0, 2])
    assert st == _lib.AMX_ERR_UNSUPPORTED and "state 0 has 65 arcs" in msg
    # the two checks of this entry: labels per segment, and one emission index per label
    n = _lib.AMX_BW_MAX_LABELS + 1
    many = ar.graph(n // 64 + 2, 0, {1: 0.0}, [(1 + i // 64, 1, 3, i, 1.0) for i in range(n)])
    st, msg = host_call([small, many], [0, 2, 4])
    assert st == _lib.AMX_ERR_UNSUPPORTED and "segment 1" in msg and "%d distinct labels" % n in msg and "limit of 4096 labels" in msg
    st, msg = host_call([ar.graph(n // 64 + 2, 0, {1: 0.0}, [(1 + i // 64, 1, 3, i, 1.0) for i in range(n - 1)])], [0, 2])
    assert st == _lib.AMX_ERR_STATE, msg                                                      # the limit itself is taken
    two = ar.graph(2, 0, {1: 0.0}, [(0, 1, 3, 40, 1.0), (1, 1, 4, 40, 1.0)])
    st, msg = host_call([small, two], [0, 2, 4])
    assert st == _lib.AMX_ERR_INVALID and "segment 1" in msg and "label 40" in msg and "emission indices 3 and 4" in msg


def test_the_python_class():
    import rasr_amd
    with pytest.raises(TypeError):
        rasr_amd.BaumWelchAligner(None, beam=3)
    with pytest.raises(TypeError):
        rasr_amd.BaumWelchAligner(None, mode=1)                                               # the mode is the handle
    with pytest.raises(rasr_amd.AmxError, match="use_partial_sums"):
        rasr_amd.BaumWelchAligner(None, use_partial_sums=1)
    g = rasr_amd.BaumWelchAligner.graphs([all_cases()["finals"]["graph"]])
    assert all(np.array_equal(v, rasr_amd.ViterbiAligner.graphs([all_cases()["finals"]["graph"]])[k]) for k, v in g.items())
    a = rasr_amd.BaumWelchAligner(None)
    assert a.align([0], g | dict(state_offsets=g["state_offsets"][:1]), None, 4)[2] == []     # no segment: nothing to do, no items
    assert _lib.lib().amx_bw_n_items(a.h) == 0
    assert _lib.lib().amx_bw_items_dev(a.h, -1, None, None, None, None, None) == _lib.AMX_ERR_INVALID
    assert "capacity -1 is too small" in _lib.lib().amx_last_error().decode()
    a.close()


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_bw_test.cc compiles the handle's host side into a program of its own: configuration refusals, the graph checks, the
    arcs by source and by label and the label tables of a batch; built with -fsanitize=address,undefined on the host side only, run as a
    process of its own (nothing sanitized is loaded into Python).  Sanitizers are for machines without a GPU: where one is present the
    same program is built and run plainly."""
    import torch
    exe = str(tmp_path / "host_bw_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_bw_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_bw_test: ok" in r.stdout, r.stdout + r.stderr
