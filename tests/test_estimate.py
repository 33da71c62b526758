"""Re-estimation (M-step), splitting and the weighted-accumulation arithmetic: oracle against the reference's own templates
(golden vectors from libref.so, and live when libref.so is present), product (host code of the C ABI) against the oracle."""
import json
import os

import numpy as np
import pytest

from oracle import OracleGmm
from oracle import estimate as oe
from tests import ref_replay, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_estimate.json")


def unhex(h, t):
    return np.frombuffer(bytes.fromhex(h), dtype=t).copy()


def one_density_model(dim):
    return dict(dim=dim, mix_offsets=np.array([0, 1], np.uint32), dens_index=np.array([0], np.uint32), log_weight=np.zeros(1),
                dens_mean=np.array([0], np.uint32), dens_cov=np.array([0], np.uint32), means=np.zeros((1, dim), np.float32),
                variances=np.ones((1, dim), np.float32))


def oracle_accumulate_row(sum_, v, weight, kind):
    """one accumulator row through the oracle's accumulation code (C for kinds 0-3, oracle/estimate.py for kind 4)"""
    dim = len(sum_)
    if kind == 4:
        return oe.plus_normalized_square(sum_, v, weight)
    o = OracleGmm(one_density_model(dim))
    acc = np.zeros(o.accumulator_size())
    lay = dict(ms=slice(2, 2 + dim), cs=slice(3 + dim, 3 + 2 * dim))
    row = lay["ms"] if kind in (0, 1) else lay["cs"]
    acc[row] = sum_
    x = np.asarray(v, np.float32).reshape(1, dim)
    if kind in (0, 2):
        o.accumulate(x, [0], [0], acc)
    else:
        o.accumulate_weighted(0, x, [0], [weight], [0], acc)
    return acc[row]


def test_oracle_matches_reference_functors_golden():
    g = json.load(open(GOLD))
    for c in g["accumulate"]:
        kind = c["kind"]
        got = oracle_accumulate_row(unhex(c["sum"], "<f8"), unhex(c["v"], "<f8" if kind == 4 else "<f4"),
                                    float(unhex(c["weight"], "<f8")[0]), kind)
        assert np.array_equal(np.asarray(got, "<f8").view(np.uint64), unhex(c["out"], "<f8").view(np.uint64)), (c["dim"], kind)
    for c in g["log_exp_norm"]:
        got = oe.log_exp_norm(list(unhex(c["v"], "<f8")))
        assert np.float64(got).tobytes() == bytes.fromhex(c["out"]), (got, unhex(c["out"], "<f8"))
    for c in g["normalized_minus"]:
        got = oe.normalized_minus(unhex(c["x"], "<f8"), unhex(c["y"], "<f8"), float(unhex(c["weight"], "<f8")[0]))
        assert got.tobytes() == bytes.fromhex(c["out"])


def test_oracle_matches_reference_functors_live(monkeypatch):
    """the reference's functors (oracle/_ref, or their recorded answers) on seeded rows"""
    from oracle.binding import ref_accumulate_vector, ref_log_exp_norm, ref_normalized_minus
    R = ref_replay.reference(monkeypatch, "test_estimate.oracle_matches_reference_functors_live")
    rng = np.random.Generator(np.random.PCG64(5))
    for dim in (2, 16, 33):
        for kind in range(5):
            s = rng.standard_normal(dim) * 10
            v = rng.standard_normal(dim) if kind == 4 else rng.standard_normal(dim).astype(np.float32)
            w = float(rng.uniform(0.1, 3))
            assert np.array_equal(oracle_accumulate_row(s, v, w, kind), ref_accumulate_vector(s, v, w, kind))
        v = rng.standard_normal(dim) * 30
        assert oe.log_exp_norm(list(v)) == ref_log_exp_norm(v)
        x, y = np.abs(rng.standard_normal(dim)) * 100, np.abs(rng.standard_normal(dim))
        assert np.array_equal(oe.normalized_minus(x, y, 7.5), ref_normalized_minus(x, y, 7.5))
    ref_replay.finish(R)


def random_statistics(model, seed, frames=4000, zero_some=True):
    """statistics the way accumulation produces them: a weight per (mixture, density) entry and the matching mean / covariance rows"""
    rng = np.random.Generator(np.random.PCG64(seed))
    dim = int(model["dim"])
    off, kd = model["mix_offsets"], model["dens_index"]
    nk, nm, nc = int(off[-1]), model["means"].shape[0], model["variances"].shape[0]
    kw = rng.gamma(0.7, frames / nk, nk)
    if zero_some:
        kw[rng.random(nk) < 0.15] = 0.0
        for m in range(len(off) - 1):                      # keep every mixture observed
            if kw[off[m]:off[m + 1]].sum() == 0:
                kw[off[m]] = 9.0
    mw, cw = np.zeros(nm), np.zeros(nc)
    ms, cs = np.zeros((nm, dim)), np.zeros((nc, dim))
    for k in range(nk):
        d = kd[k]
        mi, ci = model["dens_mean"][d], model["dens_cov"][d]
        mu = rng.standard_normal(dim) * 2
        sd = rng.uniform(0.3, 2.0, dim)
        mw[mi] += kw[k]
        cw[ci] += kw[k]
        ms[mi] += kw[k] * mu
        cs[ci] += kw[k] * (mu * mu + sd * sd)
    return np.concatenate([kw, mw, ms.reshape(-1), cw, cs.reshape(-1)])


def topology(model):
    t = {k: model[k] for k in ("dim", "mix_offsets", "dens_index", "dens_mean", "dens_cov")}
    t["n_mean"], t["n_cov"] = model["means"].shape[0], model["variances"].shape[0]
    return t


def assert_same_model(got, want):
    for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov"):
        assert np.array_equal(got[k], want[k]), k
    assert got["dim"] == want["dim"]
    assert np.array_equal(got["log_weight"].view(np.uint64), np.asarray(want["log_weight"], np.float64).view(np.uint64))
    assert np.array_equal(got["means"].view(np.uint32), want["means"].view(np.uint32))
    assert np.array_equal(got["variances"].view(np.uint32), want["variances"].view(np.uint32))


MODELS = {
    "cart-pooled": lambda: synth.gmm_cart(40, 1, 6, 16, seed=3, pooled=True),
    "cart-private": lambda: synth.gmm_cart(30, 2, 5, 24, seed=4, pooled=False),
    "tied": lambda: synth.gmm_tied(25, 32, 12, seed=5, pooled=True, k_per_mix=9),
    "single": lambda: synth.gmm_cart(12, 1, 1, 8, seed=6, pooled=False),
}


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("cfg", [
    {}, {"min_observation_weight": 0.0}, {"min_observation_weight": 40.0, "min_relative_weight": 0.05, "min_variance": 0.8},
    {"normalize_mixture_weights": 0, "allow_zero_weights": 1},
    {"split": 1}, {"split": 1, "split_min_mean_observation_weight": 60.0, "split_min_covariance_observation_weight": 100.0,
                   "split_perturbation_weight": 3e5, "split_normalize_mixture_weights": 1}])
def test_estimate_matches_oracle(name, cfg):
    """product M-step / splitter (host code behind amx_gmm_estimate) == oracle restatement, bit for bit: topology after density
    removal and renumbering, f64 log weights, f32 means and variances"""
    import rasr_amd
    model = MODELS[name]()
    acc = random_statistics(model, seed=len(name) + len(cfg))
    got = rasr_amd.gmm_estimate(model, acc, **cfg)
    want = oe.estimate(topology(model), acc, **cfg)
    assert_same_model(got, want)
    nk = int(got["mix_offsets"][-1])
    assert nk == len(got["dens_index"]) and got["means"].shape[0] == got["dens_mean"].max() + 1
    if cfg.get("normalize_mixture_weights", 1) and not cfg.get("split"):
        off = got["mix_offsets"]
        for m in range(len(off) - 1):
            assert abs(np.exp(got["log_weight"][off[m]:off[m + 1]]).sum() - 1) < 1e-12


def test_estimate_recovers_moments():
    """size-independent property: with exact sufficient statistics of known Gaussians the estimate returns their moments"""
    import rasr_amd
    model = synth.gmm_cart(10, 4, 4, 6, seed=11, pooled=False)
    rng = np.random.Generator(np.random.PCG64(12))
    nk = 40
    n = rng.integers(50, 500, nk).astype(np.float64)
    mu = rng.standard_normal((nk, 6))
    var = rng.uniform(0.5, 2, (nk, 6))
    acc = np.concatenate([n, n, (n[:, None] * mu).reshape(-1), n, (n[:, None] * (var + mu * mu)).reshape(-1)])
    got = rasr_amd.gmm_estimate(model, acc)
    assert np.allclose(got["means"], mu, rtol=1e-6, atol=1e-6) and np.allclose(got["variances"], var, rtol=1e-5)
    w = n.reshape(10, 4) / n.reshape(10, 4).sum(1, keepdims=True)
    assert np.allclose(np.exp(got["log_weight"]).reshape(10, 4), w, rtol=1e-12)


def test_zero_weight_mixture_is_an_error_unless_allowed():
    import rasr_amd
    model = synth.gmm_cart(6, 3, 3, 8, seed=13, pooled=True)
    acc = random_statistics(model, 14, zero_some=False)
    acc[3:6] = 0.0                                        # mixture 1 unobserved
    with pytest.raises(rasr_amd.AmxError, match="Mixture 1 has zero weight"):
        rasr_amd.gmm_estimate(model, acc)
    with pytest.raises(ValueError, match="Mixture 1 has zero weight"):
        oe.estimate(topology(model), acc)
    got = rasr_amd.gmm_estimate(model, acc, allow_zero_weights=1)
    assert_same_model(got, oe.estimate(topology(model), acc, allow_zero_weights=True))
    assert got["mix_offsets"][2] - got["mix_offsets"][1] == 1          # the heaviest (first) density stays
    with pytest.raises(ValueError):
        rasr_amd.gmm_estimate(model, acc[:-1])
    with pytest.raises(TypeError):
        rasr_amd.gmm_estimate(model, acc, no_such_option=1)


def test_estimate_split_round_trips_through_pms(tmp_path):
    """the estimated set is an ordinary mixture set: .pms write / read returns it, and splitting doubles the observed densities"""
    import rasr_amd
    model = synth.gmm_cart(15, 2, 2, 10, seed=15, pooled=True)
    acc = random_statistics(model, 16, frames=30000, zero_some=False)
    got = rasr_amd.gmm_estimate(model, acc, split=1, split_perturbation_weight=1e5, min_observation_weight=0.0,
                                split_min_mean_observation_weight=0.0)
    assert int(got["mix_offsets"][-1]) == 60 and got["means"].shape[0] == 60 and got["variances"].shape[0] == 1
    off = got["mix_offsets"]
    for m in range(15):                                   # children are appended behind the parents, with the parents' weights
        lw = got["log_weight"][off[m]:off[m + 1]]
        assert np.array_equal(lw[:2], lw[2:])
    d = got["means"][got["dens_mean"][got["dens_index"][2]]] - got["means"][got["dens_mean"][got["dens_index"][0]]]
    assert np.all(d < 0) and np.allclose(-d / 2, np.sqrt(got["variances"][0]) * 1e5 * 1.1920929e-07, rtol=1e-3)
    path = str(tmp_path / "split.pms")
    rasr_amd.write_pms(got, path)
    back = rasr_amd.read_pms(path)
    for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov"):
        assert np.array_equal(back[k], got[k])
    assert np.allclose(back["means"], got["means"], rtol=1e-6) and np.allclose(back["log_weight"], got["log_weight"], rtol=1e-12, atol=1e-12)
