"""CPU: Viterbi alignment.  The restatement of tests/align_reference.py against the reference's own results (tests/golden/ref_align.npz,
written by tests/golden/make_align_golden.py from the reference's text in both of its builds), bit for bit in every recorded case; the host
logic of the amx_align handle (defaults, refusals, graph checks); and that logic once more from a stand-alone program built with the host
sanitizers.  No kernel runs here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rasr_amd import _lib
from tests import align_reference as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_align.npz")
INT_MAX = ar.INT_MAX


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


_CASES, _RESTATED = None, {}


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = ar.cases()
    return _CASES


def restated(name):
    """the restatement's result of a case, computed once per session and never changed"""
    if name not in _RESTATED:
        c = all_cases()[name]
        _RESTATED[name] = ar.align_segment(c["graph"], c["scores"], **c["cfg"])
    return _RESTATED[name]


def graph_arrays(g):
    """a graph dict as the fixture's in/<case>/ arrays name it"""
    off, tgt, emi, lab, wgt = [0], [], [], [], []
    for arcs in g["arcs"]:
        for t, e, l, w in arcs:
            tgt.append(t), emi.append(e), lab.append(l), wgt.append(w)
        off.append(len(tgt))
    return dict(arc_offsets=np.array(off, np.int32), arc_target=np.array(tgt, np.int32), arc_emission=np.array(emi, np.int32),
                arc_label=np.array(lab, np.int32), arc_weight=np.array(wgt, np.float32), is_final=g["final"].astype(np.uint8),
                final_weight=g["final_weight"].astype(np.float32), initial=np.array(g["initial"], np.int32), n_states=np.array(g["n_states"], np.int32))


def check_against_fixture(golden, name, r):
    """every recorded field of one case, in every bit"""
    g = {f: golden["off/%s/%s" % (name, f)] for f in ("label", "emission", "arc_score", "survivors", "score", "reached", "n_iterations", "last_threshold",
                                                      "average_states", "state_sum")}
    assert np.array_equal(r["label"], g["label"]) and np.array_equal(r["emission"], g["emission"]), name
    assert same(np.asarray(r["arc_score"], np.float32), g["arc_score"]), name
    assert same(np.float32(r["score"]), g["score"]) and bool(r["reached"]) == bool(g["reached"]), name
    assert r["n_iterations"] == int(g["n_iterations"]) and same(np.float32(r["last_threshold"]), g["last_threshold"]), name
    assert r["state_sum"] == int(g["state_sum"]), name
    assert same(np.float64(r["average_states"]), g["average_states"]) or (np.isnan(r["average_states"]) and np.isnan(g["average_states"])), name
    if "survivors" in r:
        assert np.array_equal(r["survivors"], g["survivors"]), name


def test_fixture_holds_what_the_generator_says(golden):
    """both builds of the reference agree in every bit, the inputs are the cases the tests walk, the tie cases tell list order from id
    order, and the recorded outcomes are the ones each case is there for"""
    assert not [k for k in golden if k.startswith("fma/")]
    assert list(golden["fma_differs"]) == [""] and int(golden["fma_arrays_compared"]) == 11 * len(all_cases())
    assert {"tie_labels", "tie_finals"} <= set(golden["ties_where_lowest_id_differs"].tolist())
    for name, c in all_cases().items():
        assert same(golden["in/%s/scores" % name], np.ascontiguousarray(c["scores"], np.float32)), name
        for k, v in graph_arrays(c["graph"]).items():
            assert same(golden["in/%s/%s" % (name, k)], v), (name, k)
    off = lambda k: golden["off/" + k]
    assert int(off("prune_best_first/n_iterations")) == 3 and float(off("prune_best_first/score")) == 22.0       # the first pass pruned the best path
    assert int(off("lin3_T37/n_iterations")) == 2                                                             # the second pass repeats the score
    assert int(off("factor1/n_iterations")) == 1 and int(off("no_increase/n_iterations")) == 1
    assert int(off("min_average/n_iterations")) > 2 and float(off("min_average/average_states")) >= 18.0
    assert not off("unreachable/reached") and float(off("unreachable/score")) == ar.F32_MAX and int(off("unreachable/n_iterations")) == 123
    assert np.all(off("unreachable/label") == -1)
    assert int(off("empty/n_iterations")) == 123 and np.isnan(off("empty/average_states")) and not off("empty/reached")
    assert off("empty_final/reached") and float(off("empty_final/score")) == 2.5
    assert off("fltmax_columns/reached") and off("lin130_T80/reached") and not off("lin130_T37/reached")


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_restatement_equals_the_reference(golden, name):
    check_against_fixture(golden, name, restated(name))


def test_exact_ties_go_to_the_list_order():
    """the last candidate of the minimal score wins a state, the first final hypothesis wins the end: by position in the list, not by id"""
    lab = lambda e, v=0: e * 16 + v
    assert restated("tie_labels")["label"].tolist() == [lab(2), lab(3, 2)]        # candidates arrive from states 1, 2: the later one wins
    assert restated("tie_rank_order")["label"].tolist() == [lab(1), lab(3, 1)]    # the list holds state 2 before state 1: state 1 is the later one
    assert restated("tie_finals")["label"].tolist() == [lab(2)]                    # the list holds final state 2 before final state 1


def test_almost_equal_is_the_f32_one():
    eps = np.float32(ar.F32_EPSILON)
    assert ar.is_almost_equal(np.float32(1), np.float32(1)) and ar.is_almost_equal(np.float32(1), np.float32(1) + eps)   # d = eps < e = 2 eps
    assert not ar.is_almost_equal(np.float32(1), np.float32(1) + np.float32(4) * eps)
    assert ar.is_almost_equal(np.float32(0), np.float32(0)) and ar.is_almost_equal(ar.F32_MAX, ar.F32_MAX)   # |a| + |b| overflows: d = 0 < e = inf
    assert not ar.is_almost_equal(np.float32(np.inf), np.float32(np.inf))


# ------------------------------------------------------------------ the handle's host logic

def create(**kw):
    L = _lib.lib()
    cfg = _lib.AlignCfg()
    L.amx_align_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    st = L.amx_align_create(None, C.byref(cfg), C.byref(h))
    return L, h, st, L.amx_last_error().decode()


def test_default_configuration_is_the_aligners():
    L = _lib.lib()
    cfg = _lib.AlignCfg()
    L.amx_align_default_cfg(C.byref(cfg))
    assert (cfg.min_acoustic_pruning, cfg.increment_factor, cfg.min_average_number_of_states, cfg.increase_until_no_score_difference, cfg.n_best_pruning,
            cfg.mode, cfg.score_scale) == (50.0, 2.0, 0.0, 1, INT_MAX, _lib.AMX_ALIGN_VITERBI, 1.0)
    assert same(np.float32(cfg.max_acoustic_pruning), ar.F32_MAX)


@pytest.mark.parametrize("kw, status, words", [
    (dict(mode=_lib.AMX_ALIGN_BAUM_WELCH), _lib.AMX_ERR_UNSUPPORTED, ("mode", "baum-welch")),
    (dict(mode=7), _lib.AMX_ERR_INVALID, ("mode 7",)),
    (dict(n_best_pruning=100), _lib.AMX_ERR_UNSUPPORTED, ("n_best_pruning 100",)),
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
               dict(score_scale=0.37, min_average_number_of_states=6.0, increase_until_no_score_difference=0)):
        L, h, st, msg = create(**kw)
        assert st == 0, (kw, msg)
        L.amx_align_destroy(h)


def host_call(graphs, frame_offsets, n_columns=ar.N_COLUMNS, **patch):
    """amx_align_viterbi_dev on a handle without a context: the checks run, then the call stops with AMX_ERR_STATE before any device work"""
    import rasr_amd
    a = rasr_amd.ViterbiAligner(None)
    g = rasr_amd.ViterbiAligner.graphs(graphs)
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
            (dict(arc_target=(n_small + 2, 5)), _lib.AMX_ERR_INVALID, ("segment 1", "arc_target[%d] = 5" % (n_small + 2))),
            (dict(arc_target=(1, -1)), _lib.AMX_ERR_INVALID, ("segment 0", "arc_target[1] = -1")),
            (dict(arc_emission=(0, ar.N_COLUMNS)), _lib.AMX_ERR_INVALID, ("segment 0", "arc_emission[0] = %d" % ar.N_COLUMNS, "%d columns" % ar.N_COLUMNS)),
            (dict(initial_state=(1, 5)), _lib.AMX_ERR_INVALID, ("segment 1", "initial_state 5")),
            (dict(arc_weight=(n_small, float("nan"))), _lib.AMX_ERR_INVALID, ("segment 1", "arc_weight[%d]" % n_small, "not a number")),
            (dict(final_weight=(2, float("nan"))), _lib.AMX_ERR_INVALID, ("segment 0", "final_weight of state 2")),
            (dict(final_weight=(0, float("nan"))), _lib.AMX_ERR_STATE, ())):                  # state 0 is not final: its weight is not read
        st, msg = host_call([small, big], [0, 4, 9], **patch)
        assert st == status, (patch, msg)
        for w in words:
            assert w in msg, msg
    st, msg = host_call([small, big], [0, 4, 3])
    assert st == _lib.AMX_ERR_INVALID and "frame offsets decrease at segment 1" in msg
    st, msg = host_call([ar.linear_hmm(_lib.AMX_ALIGN_MAX_STATES, ar.N_COLUMNS, 3)], [0, 2])
    assert st == _lib.AMX_ERR_STATE, msg                                                      # the limit itself is taken
    st, msg = host_call([small, ar.linear_hmm(_lib.AMX_ALIGN_MAX_STATES + 1, ar.N_COLUMNS, 3)], [0, 2, 4])
    assert st == _lib.AMX_ERR_UNSUPPORTED and "segment 1" in msg and "limit of 2048 states" in msg
    fan = ar.graph(2, 0, {1: 0.0}, [(0, 1, i % ar.N_COLUMNS, i, 1.0) for i in range(_lib.AMX_ALIGN_MAX_OUT_ARCS + 1)])
    st, msg = host_call([fan], [0, 2])
    assert st == _lib.AMX_ERR_UNSUPPORTED and "state 0 has 65 arcs" in msg and "limit of 64 arcs" in msg
    wide = ar.graph(2, 0, {1: 0.0}, [(i % 2, 1, i, i, 1.0) for i in range(100)] + [(0, 1, 4500, 4500, 1.0)])
    st, msg = host_call([wide], [0, 2], n_columns=4000)
    assert st == _lib.AMX_ERR_INVALID and "arc_emission[50] = 4500" in msg


def test_the_python_class():
    import rasr_amd
    with pytest.raises(TypeError):
        rasr_amd.ViterbiAligner(None, beam=3)
    with pytest.raises(rasr_amd.AmxError, match="n_best_pruning"):
        rasr_amd.ViterbiAligner(None, n_best_pruning=5)
    g = rasr_amd.ViterbiAligner.graphs([all_cases()["finals"]["graph"], all_cases()["tie_labels"]["graph"]])
    assert g["state_offsets"].tolist() == [0, 5, 9] and g["initial_state"].tolist() == [0, 0]
    assert g["is_final"].tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 1] and g["final_weight"][2:5].tolist() == [7.25, 0.5, 3.0]
    assert g["arc_offsets"].tolist() == [0, 1, 4, 6, 8, 9, 11, 12, 13, 13] and len(g["arc_target"]) == 13
    with pytest.raises(ValueError):
        rasr_amd.ViterbiAligner(None).align([0, 1, 2], g | dict(state_offsets=g["state_offsets"][:2]), None, 4)


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_align_test.cc compiles the handle's host side into a program of its own: configuration and graph refusals, the
    transposition into by-target order, and the arithmetic count of the passes that are not run against a loop that runs them; built with
    -fsanitize=address,undefined on the host side only, run as a process of its own (nothing sanitized is loaded into Python).
    Sanitizers are for machines without a GPU: where one is present the same program is built and run plainly."""
    import torch
    exe = str(tmp_path / "host_align_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_align_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_align_test: ok" in r.stdout, r.stdout + r.stderr
