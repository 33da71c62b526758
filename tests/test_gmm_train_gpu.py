"""GPU parity: the training-statistics kernels (gmm_accumulate_kernel, gmm_accumulate_weighted_kernel, argmin_accumulate_kernel) on
every branch they have, through the C ABI, against the plain reference of tests/train_reference.py.

Two classes of input.  EXACT: features k/64, weights j/16 -- every product and every partial sum is exact in f64, so the accumulators
have one right value whatever order the device's atomics land in, and the comparison is np.array_equal on every section.  GAUSSIAN:
real rounding in y*y and (w*y)*y, held to the project's bar for f64 sums in an undefined order.  Baum-Welch statistics go through the
device's expf / logf and have no exact class: they are held to the oracle at the bar of the existing Baum-Welch test.
"""
import numpy as np
import pytest

from tests import synth
from tests import train_reference as tr

pytestmark = pytest.mark.gpu

JUNK32, JUNK8 = 0x7FFFFFFF, 0xFF     # what the matrix forms hold off the aligned column: a kernel that reads the wrong column drops the frame


@pytest.fixture()
def cctx(ctx):
    """the session context, handed out in contract=off and restored to it (the pattern of tests/test_contract_gpu.py)"""
    ctx.set_contract("off")
    yield ctx
    ctx.set_contract("off")


def gaussian(T, dim, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((T, dim)).astype(np.float32)


def same(got, want, exact, nk):
    """exact class: the same bits everywhere.  Gaussian class: weights of the mixture entries exactly, sums at the bar below."""
    if exact:
        return np.array_equal(got, want)
    # rtol=1e-12, atol=1e-9: the bar of tests/test_gmm_gpu.py::test_viterbi_accumulators for f64 sums whose order the device picks
    return np.array_equal(got[:nk], want[:nk]) and np.allclose(got, want, rtol=1e-12, atol=1e-9)


def check_all_forms(ctx, model, x, mix, dens, w, exact, nan_frames=(), bytes_too=True):
    """every input form of the Viterbi statistics on one case, each against the reference (and so against each other): the u32
    matrix, the byte matrix, the per-frame list in u32 and in bytes; weighted Viterbi with NULL, unit and the given weights; every
    buffer accumulated into twice.  x may hold NaN frames (nan_frames): their "none" entries are taken from the library itself."""
    import torch

    import rasr_amd
    T, M = len(mix), len(model["mix_offsets"]) - 1
    nk = int(model["mix_offsets"][-1])
    sc = rasr_amd.GmmFeatureScorer(ctx, model)
    assert sc.accumulator_size() == tr.layout(model)[4]
    ctx.use_torch_stream()
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(mix.astype(np.int32)).cuda()
    dens = dens.copy()
    if len(nan_frames):   # what amx_gmm_best_density_dev writes for a frame no density beats FLT_MAX on
        bd = torch.zeros(T, dtype=torch.int32, device="cuda")
        sc.best_density_dev(xd, T, md, bd)
        torch.cuda.synchronize()
        written = bd.cpu().numpy().view(np.uint32)
        assert (written[nan_frames] == tr.NO_DENSITY).all()
        dens[nan_frames] = written[nan_frames]
    want = tr.accumulate(model, x, mix, dens)
    want_w = tr.accumulate(model, x, mix, dens, w)
    kept = len(tr.kept_frames(model, mix, dens)[0])
    assert np.isfinite(want).all() and want[:nk].sum() == kept
    # the forms
    per32 = torch.from_numpy(dens.view(np.int32)).cuda()
    inside = torch.from_numpy((mix >= 0) & (mix < M)).cuda()
    rows, cols = torch.arange(T, device="cuda")[inside], md[inside].long()
    full32 = torch.full((T, M), JUNK32, dtype=torch.int32, device="cuda")
    full32[rows, cols] = per32[inside]
    forms = [("u32 matrix", full32, M), ("u32 list", per32, 0)]
    if bytes_too:
        d8 = np.where(dens == tr.NO_DENSITY, 0xFF, np.minimum(dens, 0xFE)).astype(np.uint8)   # no kept density is above 254 in these cases
        assert np.array_equal(tr.accumulate(model, x, mix, d8), want)
        per8 = torch.from_numpy(d8).cuda()
        full8 = torch.full((T, M), JUNK8, dtype=torch.uint8, device="cuda")
        full8[rows, cols] = per8[inside]
        forms += [("byte matrix", full8, M), ("byte list", per8, 0)]
    acc = torch.zeros(sc.accumulator_size(), dtype=torch.float64, device="cuda")

    def result():
        torch.cuda.synchronize()
        return acc.cpu().numpy()

    for name, best, ld in forms:
        acc.zero_()
        sc.accumulate_dev(xd, T, md, best, ld, acc)
        got = result()
        assert got[:nk].sum() == kept, (name, got[:nk].sum(), kept)
        assert same(got, want, exact, nk), (name, np.abs(got - want).max())
        sc.accumulate_dev(xd, T, md, best, ld, acc)
        assert same(result(), 2 * want, exact, nk), name + ", second call"
    wd = torch.from_numpy(np.ascontiguousarray(w, np.float64)).cuda()
    ones = torch.ones(T, dtype=torch.float64, device="cuda")
    for name, weights, best, ld, expect in (("NULL weights", None, full32, M, want), ("unit weights", ones, per32, 0, want),
                                            ("weights, matrix", wd, full32, M, want_w), ("weights, list", wd, per32, 0, want_w)):
        acc.zero_()
        sc.accumulate_weighted_dev(rasr_amd.AMX_GMM_VITERBI, xd, T, md, weights, best, ld, acc)
        got = result()
        assert same(got, expect, exact, nk if weights is not wd else 0), (name, np.abs(got - expect).max())
        sc.accumulate_weighted_dev(rasr_amd.AMX_GMM_VITERBI, xd, T, md, weights, best, ld, acc)
        assert same(result(), 2 * expect, exact, nk if weights is not wd else 0), name + ", second call"
    return want


def inputs(T, dim, exact, seed):
    """(features, weights) of one class"""
    if exact:
        return tr.exact_features(T, dim, seed)[0], tr.exact_weights(T, seed + 1)[0]
    w = np.random.Generator(np.random.PCG64(seed + 1)).uniform(0.0, 2.0, T)
    w[::17] = 0.0
    return gaussian(T, dim, seed), w


CLASSES = [pytest.param(True, id="exact"), pytest.param(False, id="gaussian")]


@pytest.mark.parametrize("exact", CLASSES)
@pytest.mark.parametrize("cov", ["pooled", "density"])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 300, 1024])
def test_every_register_slot_and_the_tail(ctx, dim, cov, exact):
    """lane + 64 c for c < 4 lives in registers (sx / sxx / pc), dimensions 256..1023 go straight to atomics; the unweighted entry
    points pool a single covariance in registers up to dim 256 only, the weighted one at every dim: both rules at every edge"""
    model = tr.model("cart", cov, dim, seed=1000 + dim)
    T = 1000                                                # three full blocks and a ragged one
    x, w = inputs(T, dim, exact, 2000 + dim)
    mix, dens = tr.alignment(model, T, "bursty", 3000 + dim)
    nan = tr.add_skips(model, mix, dens, x, np.arange(5, T, 83))
    check_all_forms(ctx, model, x, mix, dens, w, exact, nan)


@pytest.mark.parametrize("exact", CLASSES)
@pytest.mark.parametrize("dim", [40, 256, 257])
@pytest.mark.parametrize("cov", tr.COV_KINDS)
@pytest.mark.parametrize("kind", tr.MODEL_KINDS)
def test_every_tying_of_means_and_covariances(ctx, kind, cov, dim, exact):
    """k_dens -> d_mean / d_cov many-to-one: several mixtures add to one mean row (tied lists, shared means), several densities to one
    covariance row without the pooled shortcut (one covariance per mixture; seven spread over a tied model), next to the two extremes;
    at 40, at the last pooled dimension of the unweighted kernel and at the first one behind it"""
    model = tr.model(kind, cov, dim, seed=1100)
    T = 1500
    x, w = inputs(T, dim, exact, 2100 + dim)
    mix, dens = tr.alignment(model, T, "straddle", 3100)
    nan = tr.add_skips(model, mix, dens, x, np.arange(3, T, 101))
    check_all_forms(ctx, model, x, mix, dens, w, exact, nan)


@pytest.mark.parametrize("exact", CLASSES)
@pytest.mark.parametrize("cov", ["pooled", "grouped"])
@pytest.mark.parametrize("align", ["one", "distinct", "straddle", "broken"])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 4097, 63936])
def test_chains_of_every_shape_and_frame_count(ctx, T, align, cov, exact):
    """the chains of one workgroup (s_lead / s_next) at their extremes: one chain through all 256 frames, 256 chains of one frame,
    runs that cross the block edges, one chain whose head, middle and tail frames are skipped -- in one ragged block, at the block
    edges and over many blocks; dim 65 keeps a lone lane busy in the second register slot"""
    dim = 65
    model = tr.model("cart", cov, dim, seed=1200)
    x, w = inputs(T, dim, exact, 2200 + T)
    mix, dens = tr.alignment(model, T, "one" if align == "broken" else align, 3200)
    skipped = tr.chain_breaks(T) if align == "broken" else np.arange(9, T, 211)
    nan = tr.add_skips(model, mix, dens, x, skipped)
    want = check_all_forms(ctx, model, x, mix, dens, w, exact, nan)
    assert want[:int(model["mix_offsets"][-1])].sum() == T - len(skipped)


def test_skipped_frames_as_score_dev_writes_them(ctx):
    """the u32 matrix exactly as amx_gmm_score_dev leaves it: NaN and infinite frames are rows of 0xffffffff, the alignment is the
    best state per frame; 4097 frames, exact features"""
    import torch

    import rasr_amd
    model = synth.gmm_cart(40, 2, 6, 65, seed=1300, pooled=False)
    T, M = 4097, 40
    x, _ = tr.exact_features(T, 65, 1301)
    x *= np.float32(1.0 / 4)                                  # still dyadic, and near enough to the means for a varied alignment
    bad = np.arange(11, T, 173)
    x[bad[::2], 3] = np.nan
    x[bad[1::2]] = np.inf
    sc = rasr_amd.GmmFeatureScorer(ctx, model)
    ctx.use_torch_stream()
    xd = torch.from_numpy(x).cuda()
    scores = torch.empty((T, M), dtype=torch.float32, device="cuda")
    best = torch.empty((T, M), dtype=torch.int32, device="cuda")
    sc.score_dev(xd, T, scores, best)
    mix = scores.argmin(dim=1).to(torch.int32)
    acc = torch.zeros(sc.accumulator_size(), dtype=torch.float64, device="cuda")
    sc.accumulate_dev(xd, T, mix, best, M, acc)
    torch.cuda.synchronize()
    bh = best.cpu().numpy().view(np.uint32)
    assert (bh[bad] == tr.NO_DENSITY).all()
    want = tr.accumulate(model, x, mix.cpu().numpy(), bh)
    got = acc.cpu().numpy()
    nk = int(model["mix_offsets"][-1])
    assert got[:nk].sum() == T - len(bad) and np.array_equal(got, want)
    acc.zero_()
    b8 = torch.where(best < 0, torch.full_like(best, 255), best.clamp(max=255)).to(torch.uint8)   # 0xffffffff -> 0xff, as best_narrow_kernel does
    sc.accumulate_dev(xd, T, mix, b8, M, acc)
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), want)


@pytest.mark.parametrize("exact", CLASSES)
@pytest.mark.parametrize("pooled", [True, False])
def test_full_size_training_shape(ctx, pooled, exact):
    """the shape the benchmark's training workload times: 63 936 frames into 10 000 mixtures of 16 densities, dim 40, a bursty
    alignment with skipped frames mixed in; the reference is np.add.at over the kept frames"""
    model = synth.gmm_cart(10000, 16, 16, 40, seed=1400, pooled=pooled)
    T = 63936
    x, w = inputs(T, 40, exact, 1401)
    mix, dens = tr.alignment(model, T, "bursty", 1402)
    skipped = np.arange(17, T, 389)
    nan = tr.add_skips(model, mix, dens, x, skipped)
    want = check_all_forms(ctx, model, x, mix, dens, w, exact, nan)
    assert want[:160000].sum() == T - len(skipped)


def test_byte_form_on_a_256_density_mixture(ctx):
    """include/amx.h: the byte form holds 0xff where the u32 form holds 0xffffffff, and amx_gmm_score_stats_u8_dev refuses models
    with a mixture of more than 255 densities because a byte cannot name density 255.  amx_gmm_accumulate_u8_dev does not look at the
    model: on a 256-density mixture byte 255 is "none" as documented -- those frames contribute nothing, every other byte is the
    density it names -- and the u32 form of the same alignment counts density 255"""
    import torch

    import rasr_amd
    model = synth.gmm_cart(2, 0, 0, 24, seed=1500, pooled=False, ks=[256, 256])
    T = 2048
    x, _ = tr.exact_features(T, 24, 1501)
    mix = (np.arange(T) // 256 % 2).astype(np.int32)
    dens = ((np.arange(T) * 5) % 256).astype(np.uint32)      # every density 0..255 of both mixtures, 255 among them
    d8 = dens.astype(np.uint8)
    last = dens == 255
    assert last.sum() == 8
    want32, want8 = tr.accumulate(model, x, mix, dens), tr.accumulate(model, x, mix, d8)
    assert np.array_equal(want8, tr.accumulate(model, x[~last], mix[~last], dens[~last]))
    assert want32[:512].sum() == T and want8[:512].sum() == T - 8 and want8[255] == 0 and want32[255] == 4
    sc = rasr_amd.GmmFeatureScorer(ctx, model)
    ctx.use_torch_stream()
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(mix).cuda()
    acc = torch.zeros(sc.accumulator_size(), dtype=torch.float64, device="cuda")
    sc.accumulate_dev(xd, T, md, torch.from_numpy(dens.view(np.int32)).cuda(), 0, acc)
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), want32)
    acc.zero_()
    sc.accumulate_dev(xd, T, md, torch.from_numpy(d8).cuda(), 0, acc)
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), want8)


# ---- Baum-Welch

def bw_model(model):
    """means drawn towards the origin with the dimension, so that the distances of a frame to the densities of its mixture stay a few
    units apart and more than one density keeps a posterior above the threshold at dim 300 as at dim 16"""
    model = dict(model)
    model["means"] = (model["means"] * np.float32(min(1.0, 4.0 / np.sqrt(float(model["dim"]))))).astype(np.float32)
    return model


def check_baum_welch(cctx, contract, model, T, seed):
    import torch

    import rasr_amd
    from oracle import OracleGmm
    cctx.set_contract(contract)
    dim, n_mix = int(model["dim"]), len(model["mix_offsets"]) - 1
    x = (gaussian(T, dim, seed) * 0.6).astype(np.float32)
    w = np.random.Generator(np.random.PCG64(seed + 1)).uniform(0.2, 1.0, T)
    mix = np.repeat(np.random.Generator(np.random.PCG64(seed + 2)).integers(0, n_mix, T // 7 + 1), 7)[:T].astype(np.uint32)
    sc, o = rasr_amd.GmmFeatureScorer(cctx, model), OracleGmm(model, contract=contract)   # no tuning key: the context's arithmetic
    cctx.use_torch_stream()
    xd, md, wd = (torch.from_numpy(a).cuda() for a in (x, mix.astype(np.int32), w))
    acc = torch.zeros(sc.accumulator_size(), dtype=torch.float64, device="cuda")
    sc.accumulate_weighted_dev(rasr_amd.AMX_GMM_BAUM_WELCH, xd, T, md, wd, None, 0, acc)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    want = o.accumulate_weighted(1, x, mix, w)
    nk = int(model["mix_offsets"][-1])
    off_mw, off_ms, off_cw, off_cs, _ = tr.layout(model)
    # the three weight rows each sum to sum(w) within the 1e-3 of tests/test_gmm_gpu.py::test_baum_welch_accumulators
    for lo, hi in ((0, nk), (off_mw, off_ms), (off_cw, off_cs)):
        assert abs(got[lo:hi].sum() - w.sum()) < 1e-3 * w.sum(), (lo, hi, got[lo:hi].sum(), w.sum())
    # rtol=2e-5, atol=2e-6 * max(scale, 1): the bar of tests/test_gmm_gpu.py::test_baum_welch_accumulators (the device's expf / logf are
    # not glibc's; a density at the f32-epsilon threshold may be kept on one side only)
    scale = np.abs(want).max()
    assert np.allclose(got, want, rtol=2e-5, atol=2e-6 * max(scale, 1.0)), np.abs(got - want).max()
    return want, mix


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("cov", tr.COV_KINDS)
@pytest.mark.parametrize("dim", [65, 256, 257, 300])
def test_baum_welch_dimensions_and_tyings(cctx, dim, cov, contract):
    """the weighted kernel's own slot rule (`pooled && c < 4`, pooled at every dimension) with many densities per frame, in both
    arithmetics of the distance"""
    model = bw_model(tr.model("cart", cov, dim, seed=1600))
    want, mix = check_baum_welch(cctx, contract, model, 1500, 1601 + dim)
    nk = int(model["mix_offsets"][-1])
    assert (want[:nk] > 0).sum() > len(np.unique(mix))      # more than one density per frame really takes part


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("pooled", [True, False])
def test_baum_welch_mixture_sizes_up_to_the_lds_buffer(cctx, pooled, contract):
    """mixtures of 1, 64, 65, 1000 and 4096 densities: the lane loop strided by 64 at its edges and the whole LDS score buffer
    (kBwMaxDens).  T = 6000: about 1200 frames meet each mixture, the 4096-density one among them.  The CPU oracle sets the size: it
    takes 0.1 s per 1000 frames of this alignment (measured), 0.6 s per case here, which keeps the four cases a small part of the
    file; the device side is 94 workgroups, and more frames reach no further branch"""
    model = bw_model(synth.gmm_cart(5, 0, 0, 24, seed=1700, pooled=pooled, ks=[1, 64, 65, 1000, 4096]))
    want, _ = check_baum_welch(cctx, contract, model, 6000, 1701)
    off = model["mix_offsets"].astype(np.int64)
    assert all((want[off[m]:off[m + 1]] > 0).sum() > min(k, 32) // 2 for m, k in enumerate(np.diff(off)))


def test_baum_welch_refuses_4097_densities(ctx):
    import torch

    import rasr_amd
    model = synth.gmm_cart(2, 0, 0, 8, seed=1800, pooled=True, ks=[3, 4097])
    sc = rasr_amd.GmmFeatureScorer(ctx, model)
    T = 32
    ctx.use_torch_stream()
    xd = torch.from_numpy(gaussian(T, 8, 1801)).cuda()
    md = torch.zeros(T, dtype=torch.int32, device="cuda")
    acc = torch.zeros(sc.accumulator_size(), dtype=torch.float64, device="cuda")
    with pytest.raises(rasr_amd.AmxError) as e:
        sc.accumulate_weighted_dev(rasr_amd.AMX_GMM_BAUM_WELCH, xd, T, md, None, None, 0, acc)
    assert "Baum-Welch statistics support up to 4096 densities per mixture (model has 4097)" in str(e.value)
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any()                       # refused before anything was written
    # the Viterbi statistics of the same model have no such limit
    x, _ = tr.exact_features(T, 8, 1802)
    dens = np.full(T, 4096, np.uint32)
    mix = np.ones(T, np.int32)
    sc.accumulate_weighted_dev(rasr_amd.AMX_GMM_VITERBI, torch.from_numpy(x).cuda(), T, torch.from_numpy(mix).cuda(), None,
                               torch.from_numpy(dens.view(np.int32)).cuda(), 0, acc)
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), tr.accumulate(model, x, mix, dens))


# ---- amx_stats_accumulate_dev

FLT_MAX = np.finfo(np.float32).max


def stats_base(B, M, seed):
    """B rows of dyadic scores (k/64, |k| <= 2^14: any sum of 140 000 of them is exact in f64) with the cases of the arg-min planted
    in the first rows: ties of the minimum in one lane (e, e + 64), in two lanes, at the two ends of the row; rows without a finite
    minimum (FLT_MAX, NaN, +inf, a blend of the three); a NaN beside the minimum"""
    rng = np.random.Generator(np.random.PCG64(seed))
    s = (rng.integers(-(1 << 14), (1 << 14) + 1, (B, M)) / 64.0).astype(np.float32)
    low = np.float32(-1000.0)
    r = 0
    for a, b in ((5, 69), (3, 4), (0, M - 1), (62, 63), (63, 64), (1, 129), (M - 1, M - 1)):
        if r < B and a < M and b < M:
            s[r, [a, b]] = low
            r += 1
    for fill in (FLT_MAX, np.nan, np.inf, None):
        if r < B:
            s[r] = np.resize(np.array([FLT_MAX, np.nan, np.inf], np.float32), M) if fill is None else fill
            r += 1
    if r < B and M > 2:
        s[r, 0], s[r, M // 2] = np.nan, low
    return s


def stats_reference(base, idx):
    """first minimum among the scores below FLT_MAX (what `v < best` from FLT_MAX keeps), 0xffffffff where there is none"""
    valid = base < FLT_MAX                                   # NaN compares false
    masked = np.where(valid, base, np.inf)
    state = np.where(valid.any(axis=1), masked.argmin(axis=1), 0xFFFFFFFF).astype(np.uint32)
    value = np.where(valid.any(axis=1), masked.min(axis=1), 0.0).astype(np.float64)
    st = state[idx]
    counts = np.bincount(st[st != 0xFFFFFFFF], minlength=base.shape[1]).astype(np.int64)
    return st, counts, float(value[idx].sum())


@pytest.mark.parametrize("pattern", ["random", "runs", "alternating"])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 777, 10000])
@pytest.mark.parametrize("T", [1, 3, 4, 5, 32768, 32769, 70000])
def test_stats_accumulate_every_grid_shape(ctx, T, M, pattern):
    """one wavefront per frame, at most 8192 workgroups of four: above 32 768 frames the grid-stride loop runs again and a wave's
    run-length aggregation spans frames 32 768 apart.  Frames are rows of a small base block in three orders: random, long runs of
    one row (every wave sees one state throughout) and two rows alternating.  score_sum is exact (dyadic scores), the counts and the
    best states equal the first-minimum arg-min; a second call adds the same again"""
    import torch
    B = min(T, 256)
    base = stats_base(B, M, 1900 + M)
    rng = np.random.Generator(np.random.PCG64(1901 + T))
    if pattern == "random":
        idx = rng.permutation(np.arange(T) % B)               # every planted row takes part
    elif pattern == "runs":
        idx = (np.arange(T) // 40000) % B              # frames t and t + 32 768 of one wave: the same row below 7232, another above
    else:
        idx = np.where(np.arange(T) % 2 == 0, 0, B - 1)
    want_state, want_counts, want_sum = stats_reference(base, idx)
    ctx.use_torch_stream()
    scores = torch.from_numpy(base).cuda()[torch.from_numpy(idx).cuda()].contiguous()
    assert scores.shape == (T, M)
    best = torch.full((T,), 7, dtype=torch.int32, device="cuda")
    counts = torch.zeros(M, dtype=torch.int64, device="cuda")
    ssum = torch.zeros(1, dtype=torch.float64, device="cuda")
    for call in (1, 2):
        ctx.stats_accumulate(scores, T, M, best, counts, ssum)
        torch.cuda.synchronize()
        assert np.array_equal(best.cpu().numpy().view(np.uint32), want_state)
        assert np.array_equal(counts.cpu().numpy(), call * want_counts)
        assert counts.sum().item() == call * int((want_state != 0xFFFFFFFF).sum())
        assert ssum.item() == call * want_sum


@pytest.mark.parametrize("n", [1, 4096 * 256 + 5])
def test_counts_round_trip_through_f64(ctx, n):
    """amx_counts_to_f64_dev / amx_f64_to_counts_dev: at most 4096 workgroups of 256, so the second size runs the grid-stride loop
    again; counts above 2^32 (and below 2^53, where f64 still holds every integer)"""
    import torch

    from rasr_amd import _lib
    rng = np.random.Generator(np.random.PCG64(1950 + n % 7))
    c = rng.integers(0, 1 << 52, n, dtype=np.int64)
    c[0] = (1 << 32) + 1
    c[-1] = (1 << 53) - 1 if n > 1 else c[-1]
    ctx.use_torch_stream()
    cd = torch.from_numpy(c).cuda()
    f = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    back = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    _lib.check(ctx.L.amx_counts_to_f64_dev(ctx.h, cd.data_ptr(), f.data_ptr(), n))
    _lib.check(ctx.L.amx_f64_to_counts_dev(ctx.h, f.data_ptr(), back.data_ptr(), n))
    torch.cuda.synchronize()
    assert np.array_equal(f.cpu().numpy(), c.astype(np.float64)) and np.array_equal(back.cpu().numpy(), c)
