"""CPU: the f64 restatement of the log-add scorer (tests/sum_reference.py) against the oracle it is built from -- the same best
density, the same bits where a mixture has one density, and the oracle within its own f32 error of the f64 value elsewhere."""
import numpy as np
import pytest

from tests import synth
from tests.sum_reference import NO_DENSITY, line_frames, line_model, own_error_bound, sum_value


def feats(T, dim, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((T, dim)).astype(np.float32)


MODELS = {
    "cart-pooled": lambda: synth.gmm_cart(60, 1, 16, 40, seed=201, pooled=True),
    "cart-private-d7": lambda: synth.gmm_cart(45, 1, 9, 7, seed=202, pooled=False),
    "cart-k1": lambda: synth.gmm_cart(70, 1, 1, 33, seed=203, pooled=False),
    "cart-k200": lambda: synth.gmm_cart(5, 200, 200, 24, seed=204, pooled=True),
    "tied-shared": lambda: synth.gmm_tied(50, 64, 40, seed=205),
    "tied-partial": lambda: synth.gmm_tied(61, 128, 24, seed=206, pooled=False, k_per_mix=40),
    "line-falling": lambda: line_model(4096, 1e-3, value_at=0.0),
    "line-rising": lambda: line_model(256, 1e-5, order="rising", n_mix=3),
    "line-tied": lambda: line_model(256, 3e-4, n_mix=5, tied=True, lists=["falling", "rising"] * 2 + ["falling"]),
    "line-duplicates": lambda: line_model(64, 0.0, n_mix=2),
    "line-underflow": lambda: line_model(16, 110.0, n_mix=2),
}


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_sum_value_pins_the_oracle(name, contract):
    from oracle import OracleGmm
    model = MODELS[name]()
    dim = int(model["dim"])
    x = np.concatenate([feats(9, dim, 207), line_frames(model, n_random=0)]) if name.startswith("line") else feats(11, dim, 207)
    orc = OracleGmm(model, contract=contract)
    osc, obest = orc.score(x, mode=1)
    entries = orc.sum_entries(x)
    assert entries.shape == (x.shape[0], int(model["mix_offsets"][-1])) and entries.dtype == np.float32
    value, best = sum_value(entries, model["mix_offsets"])
    assert np.array_equal(best, obest)
    ks = np.diff(model["mix_offsets"].astype(np.int64))
    one = np.broadcast_to(ks == 1, value.shape)
    assert np.array_equal(value[one].astype(np.float32).view(np.uint32), osc[one].view(np.uint32))   # K = 1: b - log 1 = b, exactly
    err = np.abs(osc.astype(np.float64) - value)
    assert np.all(err <= own_error_bound(value, ks[None, :])), err.max()
    if name == "line-duplicates":   # equal entries: the sum is K exactly, the first density is the best
        assert np.all(best[:, :] == 0) and np.allclose(value[-2:], entries[-2:, ::64] - np.log(64), rtol=0, atol=1e-12)
    if name == "line-underflow":    # (the frame at the origin) steps > 104: every other term underflows, sum = 1, the score is the best entry
        assert np.array_equal(osc[-2].view(np.uint32), entries[-2, [15, 31]].view(np.uint32)) and np.array_equal(best[-2], [15, 15])


def test_sum_value_entries_by_hand():
    """the rule on hand-made entries: first strict minimum, NaN / +inf / FLT_MAX never picked, none -> 0xffffffff"""
    f = np.float32
    big = np.finfo(np.float32).max
    entries = np.array([[3, 1, 1, 2, np.nan, 5, np.inf, np.inf, big, 7]], f)
    off = np.array([0, 4, 6, 8, 10], np.uint32)
    value, best = sum_value(entries, off)
    assert list(best[0]) == [1, 1, NO_DENSITY, 1]
    assert value[0, 0] == pytest.approx(1 - np.log(np.exp(-2) + 1 + 1 + np.exp(-1)), abs=1e-15)
    assert np.isnan(value[0, 1])                 # a NaN term poisons the sum, the best density stays the finite one
    assert value[0, 2] == np.inf                  # all +inf: FLT_MAX - log 0
    assert value[0, 3] == pytest.approx(7.0, abs=1e-15)
