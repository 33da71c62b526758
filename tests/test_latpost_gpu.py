"""GPU: rasr_amd.LatticePosterior (latpost.hip) against the restatement of tests/latpost_reference.py, which test_latpost.py holds to the
reference's compiled text in every bit.

Discrete results -- reason codes, flags, counts, which outputs are exactly 0, f32 max or not finite -- must equal the restatement; every
other output lies within the bar of its class, measured by tests/golden/make_latpost_golden.py from the reference's arithmetic (exp and
log1p moved by one ulp) and stored in tests/golden/ref_latpost.npz, on the very shapes used here: the fixture's small cases and
latpost_reference.shape_cases() -- fans of 1, 2, 63, 64, 65, 127, 128 (the wave-sharing threshold), 129 and 300 (a level wider than the
workgroup), lattices one state below and above the LDS switch, a random lattice of 600 states.  All three modes, normalize = 0,
v_normalized = 0, both contracts."""
import functools
import os

import numpy as np
import pytest

from tests import latpost_reference as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"log": (lr.LOG, True, True), "prob": (lr.PROB, True, True), "expectation": (lr.EXPECTATION, True, True), "log_n0": (lr.LOG, False, True),
            "prob_n0": (lr.PROB, False, True), "expectation_v0": (lr.EXPECTATION, True, False)}
INTS = ("flows_agree", "vanishing_flow", "reason", "states_reached", "arcs_reached", "states_coreached", "undefined_states", "undefined_arcs",
        "levels_forward", "levels_backward")
F32_MAX = np.float32(3.40282347e+38)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_latpost.npz")))


def bar(name):
    return float(fixture()["bar/" + name][0])


@functools.lru_cache(maxsize=None)
def cases():
    c = dict(lr.small_cases())
    c.update(lr.shape_cases())
    return c


@functools.lru_cache(maxsize=None)
def want(name, variant, contract):
    """the restatement, computed once per (case, variant, contract) and never changed"""
    mode, normalize, v_normalized = VARIANTS[variant]
    return lr.posterior(cases()[name], mode, normalize, v_normalized, 100, contract if mode == lr.EXPECTATION else "off")


@pytest.fixture()
def cctx(ctx):
    ctx.use_torch_stream()
    ctx.set_contract("off")
    yield ctx
    ctx.set_contract("off")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run(cctx, names, variant, contract="off", potentials="auto", lats=None):
    import rasr_amd
    mode, normalize, v_normalized = VARIANTS[variant]
    cctx.set_contract(contract)
    lp = rasr_amd.LatticePosterior(cctx, mode, normalize, v_normalized, 100, potentials)
    lats = [cases()[n] for n in names] if lats is None else lats
    arc, final, info = lp.run(lats)
    n_states = sum(lr.n_states(lat) for lat in lats)
    pots = lp.last_potentials(n_states)
    lp.close()
    arc, final = arc.cpu().numpy(), final.cpu().numpy()
    out, a0, s0 = [], 0, 0
    for lat, i in zip(lats, info):
        n, na = lr.n_states(lat), len(lat["arc_target"])
        out.append(dict(arc=arc[a0:a0 + na], final=final[s0:s0 + n], info=i, potentials={k: v[s0:s0 + n] for k, v in pots.items()}))
        a0, s0 = a0 + na, s0 + n
    return out


def special(v):
    """the discrete part of an output array: 0 exactly zero, 1 f32 max, 2 +inf, 3 -inf, 4 NaN, 5 anything else"""
    v = np.asarray(v, np.float32)
    return np.select([v == 0, v == F32_MAX, np.isposinf(v), np.isneginf(v), np.isnan(v)], [0, 1, 2, 3, 4], 5)


def close(got, ref, limit, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), ok), what
    if ok.any():
        err = np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))
        assert err.max() <= limit, "%s: %.3g above the bar %.3g" % (what, err.max(), limit)


def check(name, variant, contract, got):
    w = want(name, variant, contract)
    cls = variant.split("_")[0]
    what = "%s/%s/%s" % (name, variant, contract)
    for k in INTS:
        assert got["info"][k] == w["info"][k], (what, k, got["info"][k], w["info"][k])
    for k in ("arc", "final"):
        assert np.array_equal(special(got[k]), special(w[k])), (what, k, got[k], w[k])
        close(got[k], w[k], bar(cls), what + " " + k)
    close([got["info"]["total_inv"]], [w["info"]["total_inv"]], bar("total_inv"), what + " total_inv")
    close([got["info"]["expectation"]], [w["info"]["expectation"]], bar("expectation_value"), what + " expectation")
    for k in ("total_inv_f32", "forward_flow", "backward_flow"):
        close([got["info"][k]], [w["info"][k]], bar("potentials") + 2.0 ** -23, what + " " + k)   # an f64 potential narrowed once
    n = len(got["final"])
    for k in ("forward", "backward"):
        close(got["potentials"][k], w["potentials"][k][:n], bar("potentials"), what + " " + k)
        close(got["potentials"]["generalized_" + k], w["potentials"]["generalized_" + k][:n], bar("generalized"), what + " generalized " + k)


def test_the_shapes_stand_where_the_kernel_switches():
    import rasr_amd
    shape = rasr_amd.LatticePosterior.kernel_shape()
    assert shape == dict(threads=256, lds_states=4096, wave_arcs=128), shape
    c = cases()
    assert lr.n_states(c["lds_below"]) + 1 == shape["lds_states"] and lr.n_states(c["lds_above"]) + 1 == shape["lds_states"] + 2
    widths = [int(np.diff(c["fan_%d" % k]["arc_offsets"]).max()) for k in (127, 128, 129)]
    assert widths == [shape["wave_arcs"] - 1, shape["wave_arcs"], shape["wave_arcs"] + 1]
    assert lr.n_states(c["fan_300"]) - 2 > shape["threads"]


# nothing outside the expectation pass is contracted (test_the_contracts_differ_where_the_fixture_says): the other modes run once
@pytest.mark.parametrize("variant,contract", [(v, c) for v in VARIANTS for c in ("off", "fma") if c == "off" or v.startswith("expectation")])
def test_every_case_against_the_restatement(cctx, variant, contract):
    names = [n for n in cases() if "_" not in variant or n in lr.small_cases()]
    for name, got in zip(names, run(cctx, names, variant, contract)):
        check(name, variant, contract, got)


def test_the_device_lies_within_the_bar_of_the_reference_itself(cctx):
    """the same against the arrays the reference's compiled text left in the fixture, not through the restatement"""
    fx = fixture()
    names = list(lr.small_cases())
    for variant in ("log", "prob", "expectation"):
        for contract in ("off", "fma"):
            for name, got in zip(names, run(cctx, names, variant, contract)):
                tag = "case/%s/%s/%s" % (name, variant, contract)
                for k in ("arc", "final"):
                    assert np.array_equal(special(got[k]), special(fx[tag + "/" + k])), (tag, k)
                    close(got[k], fx[tag + "/" + k], bar(variant), tag + " " + k)
                n = len(got["final"])
                close(got["potentials"]["backward"], fx[tag + "/potentials"][1, :n], bar("potentials"), tag + " backward")
                close(got["potentials"]["forward"], fx[tag + "/potentials"][0, :n], bar("potentials"), tag + " forward")


def test_the_contracts_differ_where_the_fixture_says(cctx):
    fx = fixture()
    names = list(lr.small_cases())
    off, fma = (run(cctx, names, "expectation", c) for c in ("off", "fma"))
    differ = []
    for name, a, b in zip(names, off, fma):
        same = all(np.array_equal(bits(a["potentials"][k]), bits(b["potentials"][k])) for k in a["potentials"])
        if fx["builds_differ/" + name][1]:
            differ.append(name)
            assert not same, name
        else:
            assert same, name
    assert differ
    # nothing outside the expectation pass is contracted
    a, b = (run(cctx, names, "log", c) for c in ("off", "fma"))
    assert all(np.array_equal(bits(x["arc"]), bits(y["arc"])) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", ["log", "expectation"])
def test_lds_and_global_potentials_give_the_same_bits(cctx, variant):
    names = list(cases())
    a, b = run(cctx, names, variant, "fma", "auto"), run(cctx, names, variant, "fma", "global")
    for name, x, y in zip(names, a, b):
        for k in ("arc", "final"):
            assert np.array_equal(bits(x[k]), bits(y[k])), (name, k)
        for k in x["potentials"]:
            assert np.array_equal(bits(x["potentials"][k]), bits(y["potentials"][k])), (name, k)


@pytest.mark.parametrize("variant", ["prob", "expectation"])
def test_a_segment_gives_the_same_bits_alone_in_a_batch_and_last(cctx, variant):
    others = [lr.random_dag(20 + k, 60 + 3 * k, 50 + k) for k in range(64)]
    for name in ("random_40", "fan_129", "inf_weights"):
        lat = cases()[name]
        alone = run(cctx, None, variant, "fma", lats=[lat])[0]
        middle = run(cctx, None, variant, "fma", lats=others[:32] + [lat] + others[32:])[32]
        last = run(cctx, None, variant, "fma", lats=others + [lat])[64]
        for other in (middle, last):
            for k in ("arc", "final"):
                assert np.array_equal(bits(alone[k]), bits(other[k])), (name, k)
            for k in alone["potentials"]:
                assert np.array_equal(bits(alone["potentials"][k]), bits(other["potentials"][k])), (name, k)
            for k, v in alone["info"].items():
                assert v == other["info"][k] or (v != v and other["info"][k] != other["info"][k]), (name, k)


def test_refused_inputs_leave_both_outputs_untouched(cctx):
    import torch

    import rasr_amd
    good = cases()["diamond"]
    cycle = lr.lattice(4, [(0, 1, 1.0, 0.0), (1, 2, 1.0, 0.0), (2, 1, 1.0, 0.0), (2, 3, 1.0, 0.0)], 0, {3: 0.0})
    nan = {k: np.array(v, copy=True) for k, v in good.items()}
    nan["arc_weight"][2] = np.nan
    bad_target = {k: np.array(v, copy=True) for k, v in good.items()}
    bad_target["arc_target"][1] = 4
    bad_initial = dict(good, initial=7)
    nan_risk = {k: np.array(v, copy=True) for k, v in good.items()}
    nan_risk["arc_risk"][0] = np.nan
    for mode, bad, word in (("log", cycle, "cycle"), ("prob", nan, "not a number"), ("log", bad_target, "target 4"), ("log", bad_initial, "initial state 7"),
                            ("expectation", nan_risk, "risk")):
        lp = rasr_amd.LatticePosterior(cctx, mode)
        t = lp.tables([good, bad, good])
        arc = torch.full((len(t["arc_target"]),), 7.5, dtype=torch.float32, device="cuda")
        final = torch.full((int(t["state_offsets"][-1]),), -3.25, dtype=torch.float32, device="cuda")
        with pytest.raises(rasr_amd.AmxError, match="segment 1.*" + word) as e:
            lp.run_dev(t, arc, final)
        assert e.value.status == rasr_amd._lib.AMX_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((arc == 7.5).all()) and bool((final == -3.25).all())
        lp.close()
    no_risk = {k: v for k, v in good.items() if k not in ("arc_risk", "final_risk")}
    with pytest.raises(ValueError, match="expectation"):
        rasr_amd.LatticePosterior(cctx, "expectation").run([no_risk])


def test_end_to_end_into_the_ebw_statistics(cctx):
    """LatticePosterior (expectation) -> the arcs in the order of a depth-first walk -> amx_ebw_accumulate_dev: the accumulator is the one the
    restatement's arc weights give.  The pass is linear in the arc weights, so where a device weight differs from the restatement's (by at
    most the expectation bar b, relative to max(1, |w|)) a cell can move by b times the sum of the magnitudes that enter it, which
    n_arcs x the largest cell bounds."""
    import torch

    import rasr_amd
    from tests import synth
    lat = cases()["random_12"]
    cctx.set_contract("fma")
    arc, _, info = rasr_amd.LatticePosterior(cctx, "expectation").run([lat])
    got_w = arc.cpu().numpy()
    ref = want("random_12", "expectation", "fma")
    close(got_w, ref["arc"], bar("expectation"), "arc weights")
    # walk order: the states as the walk discovers them, each with its arcs in its own order; two frames per arc
    order = [a for s in lr.discover_order(lat) for a in lr.arcs_of(lat, s)]
    n_mix, D = 4, 5
    model = synth.gmm_cart(n_mix, 1, 5, D, seed=3, pooled=False, ks=(2, 3, 1, 2))
    T = 2 * len(order)
    feats = np.random.RandomState(4).standard_normal((T, D)).astype(np.float32)
    item_off = np.arange(0, T + 1, 2, dtype=np.int64)
    fr = np.arange(T, dtype=np.int32)
    em = (np.arange(T, dtype=np.int32) // 2) % n_mix
    gmm = rasr_amd.GmmFeatureScorer(cctx, model)
    ebw = rasr_amd.EbwAccumulator(gmm)
    xd = torch.from_numpy(feats).cuda()
    accs = []
    for w in (got_w, ref["arc"]):
        acc = torch.zeros(ebw.accumulator_size(), dtype=torch.float64, device="cuda")
        ebw.accumulate_dev(xd, D, np.array([0, T], np.int64), np.array([0, len(order)], np.int64), np.ascontiguousarray(w[order], np.float32), item_off, fr, em, acc)
        torch.cuda.synchronize()
        accs.append(acc.cpu().numpy())
    assert np.abs(accs[1]).max() > 0 and (ref["arc"] > ebw.weight_threshold).any() and (-ref["arc"] > ebw.weight_threshold).any()
    if np.array_equal(bits(got_w), bits(ref["arc"])):
        assert np.array_equal(bits(accs[0]), bits(accs[1]))
    else:
        assert np.abs(accs[0] - accs[1]).max() <= bar("expectation") * len(order) * np.abs(accs[1]).max()
