"""The plain training-statistics reference (tests/train_reference.py) against the oracle's sequential accumulation, on the CPU: bit for
bit on exact inputs (and equal to the same sums formed in int64, in any order of the frames), within the project's bar for f64 sums
(rtol=1e-12, atol=1e-9, tests/test_gmm_gpu.py::test_viterbi_accumulators) on Gaussian ones; the skip rules and the input forms."""
import numpy as np
import pytest

from tests import synth
from tests import train_reference as tr

CASES = [(kind, cov, dim) for kind in tr.MODEL_KINDS for cov in tr.COV_KINDS for dim in (7, 65)]


def gaussian(T, dim, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((T, dim)).astype(np.float32)


def oracle_of(model, x, mix, dens, w=None):
    """the oracle has no skip rules: it is given the frames that count"""
    from oracle import OracleGmm
    o = OracleGmm(model)
    t, _ = tr.kept_frames(model, mix, dens)
    assert o.accumulator_size() == tr.layout(model)[4]
    if w is None:
        return o.accumulate(x[t], mix[t].astype(np.uint32), dens[t])
    return o.accumulate_weighted(0, x[t], mix[t].astype(np.uint32), w[t], dens[t])


@pytest.mark.parametrize("kind,cov,dim", CASES)
def test_exact_inputs_equal_the_oracle_bit_for_bit(kind, cov, dim):
    model = tr.model(kind, cov, dim, seed=900)
    T = 3000
    x, kx = tr.exact_features(T, dim, 901)
    w, jw = tr.exact_weights(T, 902)
    mix, dens = tr.alignment(model, T, "bursty", 903)
    tr.add_skips(model, mix, dens, x, np.arange(13, T, 97))
    kx[np.isnan(x)] = 0                                      # skipped frames: never read
    want = tr.accumulate(model, x, mix, dens)
    assert np.isfinite(want).all()
    assert np.array_equal(want, oracle_of(model, x, mix, dens))
    assert np.array_equal(want, tr.accumulate_int(model, kx, mix, dens))
    want_w = tr.accumulate(model, x, mix, dens, w)
    assert np.array_equal(want_w, oracle_of(model, x, mix, dens, w))
    assert np.array_equal(want_w, tr.accumulate_int(model, kx, mix, dens, jw))
    assert np.array_equal(tr.accumulate(model, x, mix, dens, np.ones(T)), want)
    nk = int(model["mix_offsets"][-1])
    kept = len(tr.kept_frames(model, mix, dens)[0])
    assert want[:nk].sum() == kept == T - len(np.arange(13, T, 97))
    off_mw, off_ms, off_cw, off_cs, _ = tr.layout(model)
    assert want[off_mw:off_ms].sum() == kept and want[off_cw:off_cs].sum() == kept
    # accumulating twice doubles; any order of the frames gives the same bits
    assert np.array_equal(tr.accumulate(model, x, mix, dens, w, acc=want_w.copy()), 2 * want_w)
    for order in (np.random.Generator(np.random.PCG64(904)).permutation(T), np.argsort(-dens.astype(np.int64), kind="stable")):
        assert np.array_equal(tr.accumulate(model, x[order], mix[order], dens[order], w[order]), want_w)


@pytest.mark.parametrize("kind,cov,dim", CASES)
def test_gaussian_inputs_equal_the_oracle_within_the_bar(kind, cov, dim):
    model = tr.model(kind, cov, dim, seed=910)
    T = 3000
    x = gaussian(T, dim, 911)
    w = np.random.Generator(np.random.PCG64(912)).uniform(0.0, 2.0, T)
    mix, dens = tr.alignment(model, T, "straddle", 913)
    got, want = tr.accumulate(model, x, mix, dens), oracle_of(model, x, mix, dens)
    nk = int(model["mix_offsets"][-1])
    assert np.array_equal(got[:nk], want[:nk]) and got[:nk].sum() == T
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9)
    assert np.allclose(tr.accumulate(model, x, mix, dens, w), oracle_of(model, x, mix, dens, w), rtol=1e-12, atol=1e-9)


def test_the_full_size_sum_is_exact_in_any_order():
    """63 936 frames of 300 exact features into a handful of rows: the largest partial sums the exact class meets"""
    model = synth.gmm_cart(3, 2, 2, 300, seed=920, pooled=True)
    T = 63936
    x, kx = tr.exact_features(T, 300, 921)
    w, jw = tr.exact_weights(T, 922)
    mix, dens = tr.alignment(model, T, "bursty", 923)
    want = tr.accumulate(model, x, mix, dens, w)
    assert np.array_equal(want, tr.accumulate_int(model, kx, mix, dens, jw))
    for order in (np.random.Generator(np.random.PCG64(924)).permutation(T), np.argsort(-dens.astype(np.int64), kind="stable")):
        assert np.array_equal(tr.accumulate(model, x[order], mix[order], dens[order], w[order]), want)


def test_skip_rules_and_input_forms():
    model = synth.gmm_cart(5, 2, 4, 3, seed=930, pooled=False)
    n_of = np.diff(model["mix_offsets"].astype(np.int64))
    T, M = 40, 5
    x, _ = tr.exact_features(T, 3, 931)
    mix, dens = tr.alignment(model, T, "random", 932)
    base = tr.accumulate(model, x, mix, dens)
    assert base[:int(model["mix_offsets"][-1])].sum() == T
    skipped = np.array([0, 7, 8, 21, 39])
    smix, sdens, sx = mix.copy(), dens.copy(), x.copy()
    nan = tr.add_skips(model, smix, sdens, sx, skipped)
    assert list(nan) == [0] and smix[7] == M and smix[8] == -1 and sdens[21] == n_of[mix[21]] and sdens[39] == tr.NO_DENSITY
    keep = np.setdiff1d(np.arange(T), skipped)
    want = tr.accumulate(model, x[keep], mix[keep], dens[keep])
    assert np.array_equal(tr.accumulate(model, sx, smix, sdens), want) and not np.array_equal(want, base)
    # matrix forms (the column of the aligned mixture counts, the others hold something else) and the byte forms (0xff = none)
    full = np.full((T, M + 2), 1, np.uint32)
    inside = (smix >= 0) & (smix < M)
    full[np.arange(T)[inside], smix[inside]] = sdens[inside]
    assert np.array_equal(tr.accumulate(model, sx, smix, full), want)
    assert np.array_equal(tr.accumulate(model, sx, smix, full.view(np.int32)), want)
    assert np.array_equal(tr.accumulate(model, sx, smix, np.minimum(full, 255).astype(np.uint8)), want)
    assert np.array_equal(tr.accumulate(model, sx, smix, np.minimum(sdens, 255).astype(np.uint8)), want)
    assert np.array_equal(tr.accumulate(model, sx, smix.astype(np.uint32), sdens), want)


def test_retied_models_are_many_to_one():
    cart = synth.gmm_cart(10, 2, 5, 4, seed=940, pooled=False)
    again = synth.gmm_cart(10, 2, 5, 4, seed=940, pooled=False, ks=np.diff(cart["mix_offsets"].astype(np.int64)))
    assert np.array_equal(cart["mix_offsets"], again["mix_offsets"])
    per_mix = synth.gmm_retie(cart, 941, cov="mixture")
    assert per_mix["variances"].shape[0] == 10 and np.array_equal(np.bincount(per_mix["dens_cov"]), np.diff(cart["mix_offsets"].astype(np.int64)))
    shared = synth.gmm_retie(cart, 942, cov=3, n_mean=7)
    assert shared["means"].shape[0] == 7 and set(shared["dens_mean"]) == set(range(7)) and set(shared["dens_cov"]) == {0, 1, 2}
    assert np.array_equal(cart["dens_cov"], np.arange(len(cart["dens_cov"])))   # the source model is left alone
