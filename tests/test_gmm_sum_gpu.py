"""GPU: the log-add scorer ("diagonal-sum", AMX_GMM_SUM) on every kernel route that serves it, in both contracts, held to
  (a) the oracle, allclose(rtol=1e-5, atol=1e-5),
  (b) the oracle's best density, bit for bit,
  (c) the f64 value of the reference's own expression on the reference's own f32 entries (tests/sum_reference.py):
      |dev - f64| <= 4 |orc - f64| + 1e-6 max(1, |f64|) -- no worse than the reference it replaces, plus a floor for the ulps by
      which the device's expf / logf differ from glibc's.
Routes: gmm_direct_kernel (CART models) with the dimension in registers or in LDS, gmm_combine_uniform_kernel (tied, one shared list),
gmm_combine_kernel (tied, per-mixture lists), and the tied frame-chunk loop."""
import numpy as np
import pytest

from tests import synth
from tests.sum_reference import NO_DENSITY, check_sum, line_frames, line_model, sum_value

pytestmark = pytest.mark.gpu

CONTRACTS = ["off", "fma"]


def feats(T, dim, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((T, dim)).astype(np.float32)


def scorer(ctx, model, contract, mode="diagonal-sum", **kw):
    import rasr_amd
    return rasr_amd.GmmFeatureScorer(ctx, model, feature_scorer_type=mode, tuning="contract=fma" if contract == "fma" else None, **kw)


def run(ctx, model, x, contract, **kw):
    sc, best = scorer(ctx, model, contract, **kw).score(x)
    check_sum(sc, best, model, x, contract=contract, **kw)
    return sc, best


def assert_bits(a, b):
    assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32)), \
        np.nanmax(np.abs(np.asarray(a, np.float64) - b))


# ---------------------------------------------------------------- 1. every dimension of the direct kernel


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("dim", [16, 24, 32, 33, 39, 40, 45, 48, 64, 1, 3, 7, 50, 80])
def test_direct_every_dimension(ctx, dim, pooled, contract):
    """9 dimensions with the frame in registers, 5 runtime ones with it in LDS; T across the wave (64) and workgroup (256) edges"""
    model = synth.gmm_cart(37, 1, 16, dim, seed=300 + dim, pooled=pooled)
    for T in (1, 63, 65, 257):
        run(ctx, model, feats(T, dim, 301 + T), contract)


# ---------------------------------------------------------------- 2. mixture lengths


def k1_models():
    uni = synth.gmm_tied(77, 1, 40, seed=311)                       # every mixture lists the one density: uniform combine
    return {"direct-d40": synth.gmm_cart(70, 1, 1, 40, seed=310, pooled=False),
            "direct-d50": synth.gmm_cart(70, 1, 1, 50, seed=312, pooled=True),
            "tied-shared": uni,
            "tied-lists": synth.gmm_tied(100, 8, 24, seed=313, k_per_mix=1)}


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("kind", ["direct-d40", "direct-d50", "tied-shared", "tied-lists"])
def test_one_density_bit_exact(ctx, kind, contract):
    """K = 1: the sum is 1, best - logf(1) = best -- the score is the entry itself, bit for bit, on every route"""
    from oracle import OracleGmm
    model = k1_models()[kind]
    dim = int(model["dim"])
    x = feats(67, dim, 314)
    sc, best = run(ctx, model, x, contract)
    orc = OracleGmm(model, contract=contract)
    osc, _ = orc.score(x, mode=1)
    assert_bits(sc, osc)
    assert_bits(sc, sum_value(orc.sum_entries(x), model["mix_offsets"])[0].astype(np.float32))
    assert np.all(best == 0)


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("shape", ["mixed-1-16", "k200", "k4096"])
def test_mixture_lengths(ctx, shape, contract):
    model = {"mixed-1-16": lambda: synth.gmm_cart(200, 1, 16, 40, seed=320, pooled=True),
             "k200": lambda: synth.gmm_cart(6, 200, 200, 40, seed=321, pooled=False),
             "k4096": lambda: synth.gmm_cart(3, 4096, 4096, 33, seed=322, pooled=True)}[shape]()
    run(ctx, model, feats(65, int(model["dim"]), 323), contract)


# ---------------------------------------------------------------- 3. both tied routes


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("lists", ["shared", "partial"])
def test_tied_routes(ctx, lists, pooled, contract):
    """shared list (gmm_combine_uniform_kernel, 8 frames per workgroup) and per-mixture lists (gmm_combine_kernel); mixture counts
    that are no multiple of 64 or 256, frame counts that are no multiple of 8"""
    if lists == "shared":
        model = synth.gmm_tied(300, 64, 40, seed=330, pooled=pooled)
    else:
        model = synth.gmm_tied(301, 128, 24, seed=331, pooled=pooled, k_per_mix=40)
    for T in (1, 9, 77):
        run(ctx, model, feats(T, int(model["dim"]), 332 + T), contract)


# ---------------------------------------------------------------- 4. more than one tied chunk


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("lists", ["shared", "partial"])
def test_tied_chunks(ctx, lists, contract):
    """9000 densities: 7424 frames per internal pass (the distance scratch stays <= 256 MB), T = 7424 + 37 takes two; the frames on
    both sides of the boundary against the oracle, the whole matrix against two separate calls"""
    if lists == "shared":
        model = synth.gmm_tied(5, 9000, 40, seed=340)
    else:
        model = synth.gmm_tied(40, 9000, 16, seed=341, k_per_mix=1000)
    chunk = 7424
    x = feats(chunk + 37, int(model["dim"]), 342)
    s = scorer(ctx, model, contract)
    sc, best = s.score(x)
    check_sum(sc, best, model, x, contract=contract, frames=[0, 1, chunk - 2, chunk - 1, chunk, chunk + 1, chunk + 36])
    a, ab = s.score(x[:chunk])
    b, bb = s.score(x[chunk:])
    assert_bits(sc, np.concatenate([a, b]))
    assert np.array_equal(best, np.concatenate([ab, bb]))


# ---------------------------------------------------------------- 5. adversarial order


LINE_KINDS = ["cart-falling", "cart-rising", "tied-shared", "tied-lists"]


def line(kind, K, gap, value_at=None):
    if kind.startswith("cart"):
        return line_model(K, gap, order=kind[5:], value_at=value_at, n_mix=3)
    lists = ["falling"] * 5 if kind == "tied-shared" else ["falling", "rising", "falling", "rising", "falling"]
    return line_model(K, gap, value_at=value_at, n_mix=5, tied=True, lists=lists)


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("value_at", [None, 0.0])
@pytest.mark.parametrize("gap", [1e-3, 3e-4, 1e-5])
@pytest.mark.parametrize("K", [16, 256, 4096])
@pytest.mark.parametrize("kind", LINE_KINDS)
def test_ordered_lists(ctx, kind, K, gap, value_at, contract):
    """entries that fall (every one a new running minimum) or rise in list order by `gap`, the score at its natural size or near 0:
    the order in which rescaling a running sum at every new minimum piles up the rounding of expf"""
    model = line(kind, K, gap, value_at)
    run(ctx, model, line_frames(model, seed=350), contract)


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("K", [16, 256, 4096])
@pytest.mark.parametrize("kind", ["cart-falling", "tied-shared", "tied-lists"])
def test_duplicate_densities(ctx, kind, K, contract):
    """K equal entries: the sum is K exactly, the first density wins"""
    model = line(kind, K, 0.0)
    x = line_frames(model, seed=351)
    sc, best = run(ctx, model, x, contract)
    assert np.all(best[0] == 0)


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("K", [16, 256])
@pytest.mark.parametrize("kind", LINE_KINDS)
def test_steps_beyond_underflow(ctx, kind, K, contract):
    """steps of 110 between the entries: every term but the best one underflows in f32, the sum is exactly 1 and the score is the
    best entry, bit for bit"""
    from oracle import OracleGmm
    model = line(kind, K, 110.0)
    x = line_frames(model, n_random=2, seed=352)[:1]   # the frame at the origin: the entries step by 110 exactly there
    sc, best = run(ctx, model, x, contract)
    e = OracleGmm(model, contract=contract).sum_entries(x)
    off = model["mix_offsets"][:-1].astype(np.int64)
    assert_bits(sc, np.take_along_axis(e, off[None, :] + best.astype(np.int64), axis=1))


# ---------------------------------------------------------------- 6. non-finite and extreme frames, scales


def extreme_frames(dim, seed):
    """normal frames with, between them, a NaN component, +-inf, +-1e30 (the distance overflows: +inf), a constant frame and zeros"""
    x = feats(24, dim, seed)
    x[1, dim // 2] = np.nan
    x[3, 0] = np.inf
    x[5, dim - 1] = -np.inf
    x[8] = 1e30
    x[9, 0] = -1e30
    x[12] = 3.0
    x[13] = 0.0
    x[17, :] = np.nan
    return x


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("kind", ["direct-d40", "direct-d50", "tied-shared", "tied-lists"])
def test_extreme_frames(ctx, kind, contract):
    model = {"direct-d40": lambda: synth.gmm_cart(37, 1, 16, 40, seed=360, pooled=False),
             "direct-d50": lambda: synth.gmm_cart(37, 1, 16, 50, seed=361, pooled=True),
             "tied-shared": lambda: synth.gmm_tied(70, 32, 40, seed=362),
             "tied-lists": lambda: synth.gmm_tied(70, 64, 40, seed=363, k_per_mix=20)}[kind]()
    dim = int(model["dim"])
    x = extreme_frames(dim, 364)
    sc, best = run(ctx, model, x, contract)
    nan_rows, inf_rows = [1, 17], [3, 5, 8, 9]
    assert np.isnan(sc[nan_rows]).all() and np.all(best[nan_rows] == NO_DENSITY)
    assert np.all(sc[inf_rows] == np.inf) and np.all(best[inf_rows] == NO_DENSITY)
    ok = np.setdiff1d(np.arange(x.shape[0]), nan_rows + inf_rows)
    assert np.isfinite(sc[ok]).all()
    alone, alone_best = scorer(ctx, model, contract).score(x[ok])   # a bad row does not touch its neighbours
    assert_bits(sc[ok], alone)
    assert np.array_equal(best[ok], alone_best)


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("kind", ["direct", "tied-shared", "tied-lists"])
def test_scales(ctx, kind, contract):
    model = {"direct": lambda: synth.gmm_cart(50, 2, 6, 40, seed=9, pooled=False),
             "tied-shared": lambda: synth.gmm_tied(90, 48, 40, seed=370),
             "tied-lists": lambda: synth.gmm_tied(90, 64, 40, seed=371, k_per_mix=24)}[kind]()
    run(ctx, model, feats(100, 40, 10), contract, mixture_weight_scale=0.7, gaussian_scale=1.3)


# ---------------------------------------------------------------- 7. full size


def whole_matrix_properties(ctx, model, x, contract, sc, best):
    """on every frame, with the results on the device: a frame permutation permutes the results bit for bit; score() equals
    score_dev(); the diagonal-maximum scorer brackets the log-add score, max - log K_m - 4 ulp <= sum <= max + 4 ulp"""
    import torch
    T, M = sc.shape
    s = scorer(ctx, model, contract)
    ctx.use_torch_stream()
    xd = torch.from_numpy(x).cuda()
    sd = torch.empty((T, M), dtype=torch.float32, device="cuda")
    bd = torch.empty((T, M), dtype=torch.int32, device="cuda")
    s.score_dev(xd, T, sd, bd)
    torch.cuda.synchronize()
    assert torch.equal(sd.view(torch.int32), torch.from_numpy(sc).cuda().view(torch.int32))
    assert torch.equal(bd, torch.from_numpy(best.view(np.int32)).cuda())
    perm = torch.randperm(T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    s2 = torch.empty_like(sd)
    b2 = torch.empty_like(bd)
    s.score_dev(xd[perm].contiguous(), T, s2, b2)
    torch.cuda.synchronize()
    assert torch.equal(s2.view(torch.int32), sd[perm].view(torch.int32))
    assert torch.equal(b2, bd[perm])
    del s2, b2
    mx = torch.empty_like(sd)
    scorer(ctx, model, contract, mode="diagonal-maximum").score_dev(xd, T, mx, None)
    torch.cuda.synchronize()
    logk = torch.from_numpy(np.log(np.diff(model["mix_offsets"].astype(np.float64)))).cuda()
    for t0 in range(0, T, 8192):
        a, b = mx[t0:t0 + 8192], sd[t0:t0 + 8192]
        mag = torch.maximum(a.abs(), b.abs())
        ulp = (torch.nextafter(mag, torch.full_like(mag, float("inf"))) - mag).double()
        a, b = a.double(), b.double()
        assert torch.isfinite(b).all()
        lo = (b >= a - logk - 4 * ulp).all().item()
        hi = (b <= a + 4 * ulp).all().item()
        assert lo and hi, "frames %d..: sum outside [max - log K - 4 ulp, max + 4 ulp]" % t0


@pytest.mark.parametrize("contract", CONTRACTS)
def test_full_size_tied(ctx, contract):
    """BASELINE config 3 tied: 4096 shared densities x 10 000 mixtures x 256 frames"""
    model = synth.gmm_tied(10000, 4096, 40, seed=380)
    x = feats(256, 40, 381)
    sc, best = scorer(ctx, model, contract).score(x)
    check_sum(sc, best, model, x, contract=contract, frames=[0, 255])
    whole_matrix_properties(ctx, model, x, contract, sc, best)


@pytest.mark.parametrize("contract", CONTRACTS)
def test_full_size_cart(ctx, contract):
    """10 000 mixtures x 16 densities x 70 000 frames: the oracle at the 256-frame and 65536-frame edges, the rest by the properties"""
    model = synth.gmm_cart(10000, 16, 16, 40, seed=390, pooled=False)
    T = 70000
    x = feats(T, 40, 391)
    sc, best = scorer(ctx, model, contract).score(x)
    check_sum(sc, best, model, x, contract=contract, frames=[0, 1, 255, 256, 65535, 65536, 65537, T - 1])
    whole_matrix_properties(ctx, model, x, contract, sc, best)
