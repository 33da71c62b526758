"""CPU side of the lattice arc posteriors.  The restatement of tests/latpost_reference.py against tests/golden/ref_latpost.npz -- the
reference's own text compiled in both builds -- in every bit; its planted defects; the host plan (latpost_host.cpp) through the ABI against
the restatement: discover order, transposed lists, levels, counts, refusals; tests/host_latpost_test.cc under the host sanitizers."""
import functools
import hashlib
import os

import numpy as np
import pytest

from tests import latpost_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"log": (lr.LOG, True, True), "prob": (lr.PROB, True, True), "expectation": (lr.EXPECTATION, True, True), "log_n0": (lr.LOG, False, True),
            "prob_n0": (lr.PROB, False, True), "expectation_v0": (lr.EXPECTATION, True, False)}
INFO = ("total_inv", "total_inv_f32", "expectation", "forward_flow", "backward_flow", "flows_agree", "vanishing_flow", "reason", "states_reached",
        "arcs_reached", "states_coreached", "undefined_states", "undefined_arcs", "levels_forward", "levels_backward")
POTS = ("forward", "backward", "generalized_forward", "generalized_backward")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_latpost.npz")))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def potentials_of(r, n):
    return np.stack([np.array(r["potentials"][k] + [0.0] * (n + 1 - len(r["potentials"][k]))) for k in POTS])


def test_the_fixture_holds_the_cases_of_this_tree():
    fx = fixture()
    for name, lat in lr.small_cases().items():
        for k in ("arc_offsets", "arc_target", "arc_weight", "arc_risk", "final_flag", "final_weight", "final_risk"):
            stored = fx["case/%s/%s" % (name, k)]
            assert np.asarray(lat[k], dtype=stored.dtype).tobytes() == stored.tobytes(), (name, k)
        assert int(fx["case/%s/initial" % name]) == lat["initial"]
    assert int(fx["overload/expm_double"][0]) == 1 and int(fx["overload/expectation_product_double"][0]) == 1


@pytest.mark.parametrize("build", ["off", "fma"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_restatement_equals_the_reference_in_every_bit(variant, build):
    fx = fixture()
    mode, normalize, v_normalized = VARIANTS[variant]
    for name, lat in lr.small_cases().items():
        r = lr.posterior(lat, mode, normalize, v_normalized, 100, build)
        tag = "case/%s/%s/%s" % (name, variant, build)
        n = lr.n_states(lat)
        assert np.array_equal(bits(r["arc"]), bits(fx[tag + "/arc"])), (tag, r["arc"], fx[tag + "/arc"])
        assert np.array_equal(bits(r["final"]), bits(fx[tag + "/final"])), tag
        pots = potentials_of(r, n)
        if mode != lr.EXPECTATION:
            pots[2:] = 0
        assert np.array_equal(bits(pots), bits(fx[tag + "/potentials"])), tag
        info = np.array([r["info"][k] for k in INFO], np.float64)
        assert np.array_equal(bits(info), bits(fx[tag + "/info"])), (tag, info, fx[tag + "/info"])


@pytest.mark.parametrize("name", ["fan_64", "fan_129", "fan_300", "random_600"])
def test_the_restatement_equals_the_reference_on_the_device_shapes(name):
    """the larger shapes of the device tests: the fixture keeps a digest of what the compiled text gave"""
    fx = fixture()
    lat = lr.shape_cases()[name]
    n = lr.n_states(lat)
    for variant in ("log", "expectation"):
        for build in ("off", "fma"):
            r = lr.posterior(lat, VARIANTS[variant][0], contract=build)
            pots = potentials_of(r, n)
            if variant != "expectation":
                pots[2:] = 0
            h = hashlib.sha256(r["arc"].tobytes() + r["final"].tobytes() + pots.tobytes()).digest()
            assert h == fx["shape/%s/%s/%s/sha256" % (name, variant, build)].tobytes(), (name, variant, build)


def test_the_cases_hold_what_they_are_for():
    c = lr.small_cases()
    # a state with at least three incoming arcs of different magnitude whose sources' discover order differs from their id order
    lat = c["discover_vs_id"]
    order, incoming, _ = lr.transpose(lat)
    src = lr.source_of(lat)
    sources = [int(src[a]) for a in incoming[4]]
    assert len(sources) >= 3 and sources != sorted(sources) and len({float(lat["arc_weight"][a]) for a in incoming[4]}) == len(sources)
    # a tie in the minimum: the first and the last arc of the initial state
    p = lr.potentials(c["tie_min"], lr.LOG)
    scores = [p["backward"][int(c["tie_min"]["arc_target"][a])] + float(c["tie_min"]["arc_weight"][a]) for a in lr.arcs_of(c["tie_min"], 0)]
    assert scores[0] == scores[-1] == min(scores) and len(scores) == 4
    # an arc whose score equals its source's final weight
    p = lr.potentials(c["final_tie"], lr.LOG)
    last = list(lr.arcs_of(c["final_tie"], 1))[-1]
    assert p["backward"][int(c["final_tie"]["arc_target"][last])] + float(c["final_tie"]["arc_weight"][last]) == float(c["final_tie"]["final_weight"][1])
    assert lr.posterior(c["no_final"])["info"]["reason"] == lr.NO_FINAL and lr.posterior(c["dead_end"])["info"]["undefined_arcs"] == 1
    assert lr.posterior(c["unreachable"])["info"]["states_reached"] == 3
    assert np.isposinf(c["inf_weights"]["arc_weight"]).any() and np.isneginf(c["inf_weights"]["arc_weight"]).any()
    fx = fixture()
    assert [n for n in c if fx["builds_differ/" + n][1]], "no case on which the reference's two builds differ"


@pytest.mark.parametrize("defect", [d for d in lr.DEFECTS if d != "expectation-min-nonstrict"])
def test_a_planted_defect_leaves_bit_equality_on_its_case(defect):
    name = lr.CASE_OF_DEFECT[defect]
    mode = lr.MODE_OF_DEFECT.get(defect, lr.LOG)
    fx = fixture()
    variant = {lr.LOG: "log", lr.PROB: "prob", lr.EXPECTATION: "expectation"}[mode]
    for build in ("off", "fma"):
        bad = lr.posterior(lr.small_cases()[name], mode, contract=build, defect=defect)
        tag = "case/%s/%s/%s" % (name, variant, build)
        pots = potentials_of(bad, lr.n_states(lr.small_cases()[name]))
        if mode != lr.EXPECTATION:
            pots[2:] = 0
        same = np.array_equal(bits(bad["arc"]), bits(fx[tag + "/arc"])) and np.array_equal(bits(bad["final"]), bits(fx[tag + "/final"])) and \
            np.array_equal(bits(pots), bits(fx[tag + "/potentials"]))
        assert not same, (defect, name, build)


def test_a_non_strict_minimum_in_the_expectation_pass_cannot_change_a_bit():
    """The issue lists `strict / non-strict swapped in the expectation minimum` among the defects a case must make visible.  No case can:
    the expectation pass uses its minimum as a value only (every arc enters denSum, none is left out), and the value of a minimum does not
    depend on which of two equal candidates supplied it; +0 against -0 does not help, because a tie means at least two terms exp(0) = 1,
    so log1p(denSum - 1) > 0 and the sign of a zero minimum does not reach the potential.  What can be asserted is asserted: with the
    defect the restatement keeps every bit on every case, small and large, in both builds."""
    cases = dict(lr.small_cases())
    cases.update({k: v for k, v in lr.shape_cases().items() if not k.startswith("lds")})
    for name, lat in cases.items():
        for build in ("off", "fma"):
            assert lr.same_bits(lr.posterior(lat, lr.EXPECTATION, contract=build), lr.posterior(lat, lr.EXPECTATION, contract=build, defect="expectation-min-nonstrict")), name


# ---------------------------------------------------------------------------------------------------------------- the host plan through the ABI

def test_the_host_plan_equals_the_restatement():
    import rasr_amd
    cases = dict(lr.small_cases())
    cases.update({k: v for k, v in lr.shape_cases().items() if k in ("fan_129", "fan_300", "random_600")})
    names = list(cases)
    for mode in lr.MODES:
        lp = rasr_amd.LatticePosterior(None, mode)
        plan = lp.plan([cases[n] for n in names])
        s0 = a0 = 0
        for g, name in enumerate(names):
            lat = cases[name]
            n, na = lr.n_states(lat), len(lat["arc_target"])
            r = lr.posterior(lat, mode)
            P = r["potentials"]
            assert list(plan["discover_index"][s0:s0 + n]) == P["discover_index"], name
            assert list(plan["level_backward"][s0:s0 + n]) == P["level_backward"], name
            assert list(plan["level_forward"][s0:s0 + n]) == P["level_forward"], name
            assert int(plan["level_super"][g]) == P["level_super"], name
            finals = [int(v) for v in plan["final_order"][s0:s0 + n] if v >= 0]
            assert finals == P["finals"], name
            for v in range(n):
                got = [int(x) - a0 for x in plan["in_arc"][plan["in_offsets"][s0 + v]:plan["in_offsets"][s0 + v + 1]]]
                assert got == P["incoming"][v], (name, v)
            for k in INFO[7:]:
                assert plan["info"][g][k] == r["info"][k], (name, k)
            s0, a0 = s0 + n, a0 + na
        lp.close()


def test_the_host_plan_refuses_what_the_reference_would_not_take():
    import rasr_amd
    from rasr_amd import _lib
    good = lr.small_cases()["diamond"]

    def changed(**kw):
        lat = {k: np.array(v, copy=True) for k, v in good.items()}
        for k, (i, v) in kw.items():
            lat[k][i] = v
        return lat
    cycle = lr.lattice(4, [(0, 1, 1.0, 0.0), (1, 2, 1.0, 0.0), (2, 1, 1.0, 0.0), (2, 3, 1.0, 0.0)], 0, {3: 0.0})
    loop = lr.lattice(3, [(0, 1, 1.0, 0.0), (2, 2, 1.0, 0.0)], 0, {1: 0.0})      # a cycle the initial state does not reach
    bad = [("log", cycle, "segment 1: state [12] lies on a cycle"), ("log", loop, "segment 1: state 2 lies on a cycle"),
           ("log", changed(arc_target=(1, 4)), "segment 1: arc 1 of state 0 has target 4"), ("log", changed(arc_target=(0, -1)), "target -1"),
           ("log", dict(good, initial=4), "segment 1: initial state 4"), ("log", dict(good, initial=-1), "initial state -1"),
           ("prob", changed(arc_weight=(3, np.nan)), "segment 1: weight of arc 0 of state 2 is not a number"),
           ("log", changed(final_weight=(3, np.nan)), "final weight of state 3"),
           ("expectation", changed(arc_risk=(0, np.nan)), "risk of arc 0 of state 0"), ("expectation", changed(final_risk=(3, np.nan)), "final risk of state 3")]
    for mode, lat, text in bad:
        lp = rasr_amd.LatticePosterior(None, mode)
        with pytest.raises(rasr_amd.AmxError, match=text) as e:
            lp.plan([good, lat, good])
        assert e.value.status == _lib.AMX_ERR_INVALID
        lp.close()
    # what is not read may be anything: a NaN final weight of a state that is not final, a NaN risk outside the expectation mode
    lp = rasr_amd.LatticePosterior(None, "log")
    lp.plan([changed(final_weight=(0, np.nan), arc_risk=(0, np.nan))])
    # +-inf weights are taken
    lp.plan([lr.small_cases()["inf_weights"]])
    with pytest.raises(rasr_amd.AmxError, match="without a context") as e:
        lp.run_dev(lp.tables([good]), None, None)
    assert e.value.status == _lib.AMX_ERR_STATE
    with pytest.raises(ValueError):
        rasr_amd.LatticePosterior(None, "viterbi")
    with pytest.raises(rasr_amd.AmxError, match="tolerance"):
        rasr_amd.LatticePosterior(None, "log", tolerance=0)
    no_risk = {k: v for k, v in good.items() if k not in ("arc_risk", "final_risk")}
    with pytest.raises(ValueError, match="expectation"):
        rasr_amd.LatticePosterior(None, "expectation").plan([no_risk])


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_latpost_test.cc compiles latpost_host.cpp into a program of its own: the plan of a file of lattices against the
    restatement's orders and levels, every refusal, an empty call; built with -fsanitize=address,undefined on the host side only and run as
    a process of its own (nothing sanitized is loaded into Python).  Where a GPU is present the same program is built and run plainly."""
    import subprocess

    import torch
    exe = str(tmp_path / "host_latpost_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_latpost_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    cases = dict(lr.small_cases())
    cases.update({k: v for k, v in lr.shape_cases().items() if k in ("fan_129", "random_600")})
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        np.array([len(cases)], np.int32).tofile(f)
        for lat in cases.values():
            n, na = lr.n_states(lat), len(lat["arc_target"])
            P = lr.posterior(lat, lr.EXPECTATION)
            np.array([n, na, lat["initial"]], np.int32).tofile(f)
            np.asarray(lat["arc_offsets"], np.int64).tofile(f)
            np.asarray(lat["arc_target"], np.int32).tofile(f)
            for k in ("arc_weight", "arc_risk"):
                np.asarray(lat[k], np.float32).tofile(f)
            np.asarray(lat["final_flag"], np.uint8).tofile(f)
            for k in ("final_weight", "final_risk"):
                np.asarray(lat[k], np.float32).tofile(f)
            for k in ("discover_index", "level_backward", "level_forward"):
                np.asarray(P["potentials"][k], np.int32).tofile(f)
            np.array([P["potentials"]["level_super"], P["info"]["reason"], P["info"]["undefined_arcs"], P["info"]["states_coreached"]], np.int32).tofile(f)
            flat = [a for v in range(n) for a in P["potentials"]["incoming"][v]]
            np.array([len(flat)] + flat, np.int32).tofile(f)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "host_latpost_test: ok" in r.stdout, r.stdout + r.stderr
