"""CPU side of the lattice best path and pruning: the host plan (latbest_host.cpp) through the ABI against the restatement of
tests/latbest_reference.py -- both topological orders --, every refusal, amx_latbest_compact against numpy, the symbols and the kernel
shape, and that the constructed cases hold what they are for."""
import numpy as np
import pytest

from tests import latbest_reference as lr


def test_the_cases_hold_what_they_are_for():
    # an exact-min kernel fails: in at least one tie case the ordered chain keeps a value that is not the minimum
    ties = [n for n in lr.CASES if n.startswith("tie")]
    differ = [n for n in ties if lr.best(n)["info"]["best_score"] != 1.0]   # every path's sum is its first arc's weight; the smallest is 1
    assert differ and len(differ) < len(ties), differ
    # one and two ulps apart: the later, smaller arc wins only at two
    assert lr.best("bestarc_1")["best_arc"][0] == 0 and lr.best("bestarc_2")["best_arc"][0] == 1
    assert lr.best("final_below")["best_arc"][0] == 0      # the final weight, one ulp below, does not win
    assert list(lr.best("keep_ulps", 0.5, False)["keep"]) == [1, 0, 1, 1, 1, 1]   # +2 ulps is the one arc dropped
    # pruning leaves a dead arc, the trim clears it
    lat, thr = lr.CASES["dead_arc"]
    assert list(lr.best("dead_arc", thr, False)["keep"]) == [1, 0, 0, 1] and list(lr.best("dead_arc", thr, False, True)["keep"]) == [1, 0, 0, 0]
    assert lr.best("no_final")["info"]["reason"] == lr.NO_FINAL and lr.best("no_final")["info"]["best_score"] == lr.INVALID
    assert lr.best("unreached")["info"]["states_reached"] == 3
    for a, b, c in ((1.0, lr.ulps(1.0, 1), 0), (1.0, lr.ulps(1.0, 2), -1), (0.0, -0.0, 0), (np.inf, lr.ZERO, 0), (-np.inf, np.inf, -1), (lr.ZERO, -lr.ZERO, 1)):
        assert lr.compare(np.float32(a), np.float32(b)) == c      # -0 meets +0, an infinity sits next to f32 max


def test_the_host_plan_equals_the_restatement():
    import rasr_amd
    names = [n for n in lr.CASES if not n.startswith("lds")] + ["lds%d" % (lr.LDS_STATES + 1)]
    lb = rasr_amd.LatticeBest(None)
    plan = lb.plan([lr.CASES[n][0] for n in names])
    lb.close()
    s0 = 0
    for name, info in zip(names, plan["info"]):
        k = lr._walks(name)
        n, want = k["n"], lr.best(name)["info"]
        disc = np.full(n, -1)
        disc[k["discover"]] = np.arange(len(k["discover"]))
        assert np.array_equal(plan["discover_index"][s0:s0 + n], disc), name
        assert np.array_equal(plan["topo_forward"][s0:s0 + n], k["topo_forward"]), name
        assert np.array_equal(plan["topo_backward"][s0:s0 + n], k["topo_backward"]), name
        assert plan["topo_super"][names.index(name)] == k["topo_super"], name
        for f in ("reason", "total_arcs", "states_reached", "states_coreached"):
            assert info[f] == want[f], (name, f)
        s0 += n


def test_the_host_plan_refuses_what_the_reference_would_not_take():
    import rasr_amd
    from rasr_amd import _lib
    good = lr.CASES["tie2_1_0"][0]

    def changed(**kw):
        lat = {k: np.array(v, copy=True) for k, v in good.items()}
        for k, (i, v) in kw.items():
            lat[k][i] = v
        return lat
    bad = [(lr.lattice([(0, 1, 1.0), (1, 2, 1.0), (2, 1, 1.0), (2, 3, 1.0)], 4, {3: 0.0}), "segment 1: state [12] lies on a cycle"),
           (changed(arc_target=(1, 4)), "segment 1: arc 1 of state 0 has target 4"), (dict(good, initial=4), "segment 1: initial state 4"),
           (changed(arc_weight=(3, np.nan)), "segment 1: weight of arc 0 of state 2 is not a number"),
           (changed(final_weight=(3, np.nan)), "final weight of state 3")]
    lb = rasr_amd.LatticeBest(None)
    for lat, text in bad:
        with pytest.raises(rasr_amd.AmxError, match=text) as e:
            lb.plan([good, lat, good])
        assert e.value.status == _lib.AMX_ERR_INVALID
    t = lb.tables([good, good])
    t["arc_offsets"][2] = 1   # tables() would refuse these offsets itself: broken behind it
    with pytest.raises(rasr_amd.AmxError, match="arc_offsets descend at state 1"):
        _lib.check(lb.L.amx_latbest_plan_host(lb.h, 2, *lb._args(t), *([None] * 7)))
    lb.plan([changed(final_weight=(0, np.nan))])   # what is not read may be anything
    with pytest.raises(rasr_amd.AmxError, match="without a context") as e:
        lb.run_dev(lb.tables([good]), None, None, None, None)
    assert e.value.status == _lib.AMX_ERR_STATE
    with pytest.raises(rasr_amd.AmxError, match="threshold"):
        rasr_amd.LatticeBest(None, threshold=np.nan)
    with pytest.raises(ValueError):
        rasr_amd.LatticeBest(None, potentials="lds")


def test_compact_against_numpy():
    import rasr_amd
    names = ["random600", "unreached", "par65"]
    t = rasr_amd.LatticeBest(None).tables([lr.CASES[n][0] for n in names])
    keep = np.random.default_rng(3).integers(0, 2, len(t["arc_target"])).astype(np.uint8)
    out, old_to_new = rasr_amd.LatticeBest.compact(t, keep)
    src = np.repeat(np.arange(len(t["arc_offsets"]) - 1), np.diff(t["arc_offsets"]))
    sel = keep != 0
    assert np.array_equal(out["arc_target"], t["arc_target"][sel]) and np.array_equal(out["arc_weight"].view(np.uint32), t["arc_weight"][sel].view(np.uint32))
    assert np.array_equal(np.diff(out["arc_offsets"]), np.bincount(src[sel], minlength=len(t["arc_offsets"]) - 1))
    assert np.array_equal(old_to_new, np.where(sel, np.cumsum(sel) - 1, -1))
    for k in ("state_offsets", "initial", "final_flag", "final_weight"):
        assert out[k] is t[k]
    with pytest.raises(ValueError):
        rasr_amd.LatticeBest.compact(t, keep[:-1])


def test_symbols_and_kernel_shape():
    import rasr_amd
    from rasr_amd import _lib
    for s in ("cfg_default", "create", "destroy", "kernel_shape", "run_dev", "plan_host", "compact", "last_potentials", "last_timing"):
        assert hasattr(_lib.lib(), "amx_latbest_" + s)
    post = rasr_amd.LatticePosterior.kernel_shape()
    assert rasr_amd.LatticeBest.kernel_shape() == dict(threads=256, lds_states=lr.LDS_STATES, wave_arcs=post["wave_arcs"])
    assert lr.LDS_STATES == 2 * post["lds_states"]
    assert "LatticeBest" in rasr_amd.__all__
