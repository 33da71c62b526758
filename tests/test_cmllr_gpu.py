"""GPU parity: amx_cmllr_accumulate_dev and amx_cmllr_apply_dev (cmllr.hip) against the restatement of tests/cmllr_reference.py, which
tests/test_cmllr.py holds to the reference's own text in both of its builds.

Accumulation: every f64 of the flat buffer equals the restatement's bits, in both contracts, in one call and cut into two at a frame
inside a segment.  Apply: every f32 equals amx_matrix_multiply_dev run per segment on the materialised [1, x].  Every test runs on a
handful of frames."""
import numpy as np
import pytest

from tests import cmllr_reference as cr
from tests import synth

pytestmark = pytest.mark.gpu


@pytest.fixture()
def cctx(ctx):
    """the session context on torch's stream, handed out in contract=off and restored to it"""
    ctx.use_torch_stream()
    ctx.set_contract("off")
    yield ctx
    ctx.set_contract("off")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def stage():
    import rasr_amd
    return rasr_amd.AffineFeatureTransformEstimator.kernel_shape()


def problem(F, M, pooled, weighted, lens, keys, seed, matrix):
    """a model, frames, a segment table and an alignment: some frames carry emission -1, some weights are 0; matrix: the best densities
    as the scorer's [T x n_mix] matrix (else one per frame)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    model = synth.gmm_cart(4, 1, 3, M, seed=seed, pooled=pooled)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(off[-1])
    feats = (rng.standard_normal((T, F)) * 1.5 + 0.5).astype(np.float32)
    n_mix = 4
    emission = rng.integers(0, n_mix, T).astype(np.int32)
    if T > 2:
        emission[rng.random(T) < 0.1] = -1
        emission[1] = -1
    ks = (model["mix_offsets"][1:] - model["mix_offsets"][:-1]).astype(np.int64)
    if matrix:
        best = np.stack([rng.integers(0, ks[m], T) for m in range(n_mix)], axis=1).astype(np.uint32)
    else:
        best = np.array([rng.integers(0, ks[e]) if e >= 0 else 0xFFFFFFFF for e in emission], np.uint32)
    weight = None
    if weighted:
        weight = rng.uniform(0.05, 2.0, T)
        weight[rng.random(T) < 0.1] = 0.0
        weight[0] = 0.0
    return dict(model=model, F=F, M=M, n_keys=3, feats=feats, frame_offsets=off, seg_key=np.array(keys, np.int32), emission=emission, best=best,
                weight=weight, best_ld=n_mix if matrix else 0, pooled=pooled)


def device_accumulate(cctx, p, pieces, contract, tile=None):
    """the device's flat buffer after the calls `pieces` (lists of (offsets, keys)); returns (estimator, buffer)"""
    import torch

    import rasr_amd
    cctx.set_contract(contract)
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    est = rasr_amd.AffineFeatureTransformEstimator(gmm, p["F"], p["n_keys"])
    if tile is not None:
        est.set_tile(tile)
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    xd, ed, bd = torch.from_numpy(p["feats"]).cuda(), torch.from_numpy(p["emission"]).cuda(), torch.from_numpy(p["best"].view(np.int32)).cuda()
    wd = torch.from_numpy(p["weight"]).cuda() if p["weight"] is not None else None
    for off, keys in pieces:
        est.accumulate_dev(xd, p["F"], off, keys, ed, bd, acc, p["best_ld"], wd)
    torch.cuda.synchronize()
    return est, acc.cpu().numpy()


def restate(p, contract, off=None):
    return cr.accumulate(p["model"], p["F"], p["n_keys"], p["feats"], p["frame_offsets"] if off is None else off, p["seg_key"], p["emission"], p["best"],
                         p["best_ld"], p["weight"], None, contract)


def two_calls(p):
    """the segment table cut at a frame inside segment 0"""
    off = p["frame_offsets"]
    cut = int(off[0] + (off[1] - off[0] + 1) // 2)
    return [(np.clip(off, 0, cut), p["seg_key"]), (np.clip(off, cut, None), p["seg_key"])]


# key 1 receives no frame; key 0 has two segments around one of key 2; (45, 45) crosses a workgroup's share of the triangle (1081 cells)
# and of the model (three tiles of components); T = stage + 1 crosses the LDS stage
SHAPES = [(5, 5), (13, 9), (45, 45)]


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("F,M", SHAPES)
def test_accumulation_equals_the_restatement_in_every_bit(cctx, F, M, pooled, contract):
    s, cells, comps = stage()
    assert (F, M) != (45, 45) or (46 * 47 // 2 > cells and M > 2 * comps)
    for weighted, matrix in ((True, True), (False, False)):
        p = problem(F, M, pooled, weighted, [s + 1, 3, 4, 2], [0, 2, 0, 2], 31 * F + M + weighted, matrix)
        want = restate(p, contract)
        size = cr.layout(F, M, pooled)["size"]
        assert want[:size].any() and not want[size:2 * size].any() and want[2 * size:].any()
        est, got = device_accumulate(cctx, p, [(p["frame_offsets"], p["seg_key"])], contract)
        assert est.key_size() == size and est.pooled == pooled
        assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
        _, cut = device_accumulate(cctx, p, two_calls(p), contract)
        assert np.array_equal(bits(cut), bits(want))
        if not pooled:   # the wide tile of the G kernel (a lane keeps 48 components): the same bits
            _, wide = device_accumulate(cctx, p, two_calls(p), contract, tile=48)
            assert np.array_equal(bits(wide), bits(want))
    if contract == "fma":   # the two contracts are two arithmetics on these frames (k's m / v * xi is fused in both overloads)
        assert not np.array_equal(bits(want), bits(restate(p, "off")))


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_one_frame_and_skipped_frames(cctx, contract):
    p = problem(13, 9, False, True, [1], [2], 7, False)
    assert p["emission"][0] >= 0 and p["weight"][0] == 0.0   # a weight of 0 adds the reference's zeros: beta stays 0, the call succeeds
    _, got = device_accumulate(cctx, p, [(p["frame_offsets"], p["seg_key"])], contract)
    assert np.array_equal(bits(got), bits(restate(p, contract)))
    p["weight"][0] = 0.75
    _, got = device_accumulate(cctx, p, [(p["frame_offsets"], p["seg_key"])], contract)
    want = restate(p, contract)
    assert np.array_equal(bits(got), bits(want)) and want[2 * cr.layout(13, 9, False)["size"]] == 0.75
    p = problem(5, 5, False, False, [4, 0, 3], [1, 0, 1], 8, True)   # an empty segment; every frame skipped
    p["emission"][:] = -1
    _, got = device_accumulate(cctx, p, [(p["frame_offsets"], p["seg_key"])], contract)
    assert not got.any()


def test_a_wider_stream_and_a_wider_matrix(cctx):
    """F > M with the features a column block of a wider matrix, frames that start past row 0"""
    import torch

    import rasr_amd
    p = problem(13, 9, False, True, [6, 5], [1, 0], 9, True)
    wide = np.full((p["feats"].shape[0], 20), np.nan, np.float32)
    wide[:, 3:16] = p["feats"]
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    est = rasr_amd.AffineFeatureTransformEstimator(gmm, 13, 3)
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    off = p["frame_offsets"][1:]   # the second segment only
    est.accumulate_dev(torch.from_numpy(wide).cuda()[:, 3:], 20, off, p["seg_key"][1:], torch.from_numpy(p["emission"]).cuda(),
                       torch.from_numpy(p["best"].view(np.int32)).cuda(), acc, p["best_ld"], torch.from_numpy(p["weight"]).cuda())
    want = cr.accumulate(p["model"], 13, 3, p["feats"], off, p["seg_key"][1:], p["emission"], p["best"], p["best_ld"], p["weight"])
    assert np.array_equal(bits(acc.cpu().numpy()), bits(want))


def test_refusals_leave_the_buffer_untouched_and_name_the_frame(cctx):
    import torch

    import rasr_amd
    from rasr_amd import _lib
    p = problem(5, 5, False, True, [6, 5], [0, 1], 10, True)
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    est = rasr_amd.AffineFeatureTransformEstimator(gmm, 5, 3)
    mark = 3.25
    acc = torch.full((est.accumulator_size(),), mark, dtype=torch.float64, device="cuda")
    xd, bd, wd = torch.from_numpy(p["feats"]).cuda(), torch.from_numpy(p["best"].view(np.int32)).cuda(), torch.from_numpy(p["weight"]).cuda()

    def refused(match, feats=xd, emission=p["emission"], best=bd, weight=wd, off=p["frame_offsets"], keys=p["seg_key"]):
        with pytest.raises(rasr_amd.AmxError, match=match) as e:
            est.accumulate_dev(feats, 5, off, keys, torch.from_numpy(np.ascontiguousarray(emission)).cuda(), best, acc, p["best_ld"], weight)
        assert e.value.status == _lib.AMX_ERR_INVALID
        assert bool((acc == mark).all())

    for bad in (4, -2, 1 << 20):
        e = p["emission"].copy()
        e[7], e[9] = bad, bad
        refused("frame 7: emission index %d" % bad, emission=e)
    b = p["best"].copy()
    b[8, :] = 3
    em = p["emission"].copy()
    em[8] = 0
    refused("frame 8: the density", emission=em, best=torch.from_numpy(b.view(np.int32)).cuda())
    x = p["feats"].copy()
    x[4, 2] = np.inf
    em = p["emission"].copy()
    em[4] = 1
    refused("frame 4: non-finite feature", feats=torch.from_numpy(x).cuda(), emission=em)
    w = p["weight"].copy()
    w[3] = np.nan
    em = p["emission"].copy()
    em[3] = 1
    refused("frame 3: non-finite weight", weight=torch.from_numpy(w).cuda(), emission=em)
    refused("key 3 is outside", keys=np.array([0, 3], np.int32))
    refused("key -1 is outside", keys=np.array([-1, 0], np.int32))
    refused("frame_offsets decrease", off=np.array([0, 6, 5], np.int64))
    with pytest.raises(rasr_amd.AmxError, match="NULL"):
        est.accumulate_dev(None, 5, p["frame_offsets"], p["seg_key"], torch.from_numpy(p["emission"]).cuda(), bd, acc, p["best_ld"], wd)
    with pytest.raises(rasr_amd.AmxError, match="smaller than the model's dimension"):
        rasr_amd.AffineFeatureTransformEstimator(gmm, 4, 3)
    with pytest.raises(rasr_amd.AmxError):
        rasr_amd.AffineFeatureTransformEstimator(gmm, 256, 3)
    with pytest.raises(rasr_amd.AmxError, match="n_keys 65536") as e:
        rasr_amd.AffineFeatureTransformEstimator(gmm, 5, 65536)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    with pytest.raises(rasr_amd.AmxError, match="instances for 16 and 48"):
        est.set_tile(32)


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("F,M", SHAPES)
def test_apply_equals_matrix_multiply_on_the_extended_features(cctx, F, M, contract):
    import torch

    import rasr_amd
    from rasr_amd import _lib
    cctx.set_contract(contract)
    rng = np.random.Generator(np.random.PCG64(F))
    lens, keys, has = [257, 3, 0, 40], np.array([0, 2, 1, 1], np.int32), np.array([1, 0, 1], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(off[-1])
    x = (rng.standard_normal((T, F)) * 2).astype(np.float32)
    A = (rng.standard_normal((3, M, F + 1))).astype(np.float32)
    xd, Ad = torch.from_numpy(x).cuda(), torch.from_numpy(A).cuda()
    out = torch.full((T, M + 2), -7.0, dtype=torch.float32, device="cuda")
    tr = rasr_amd.AffineFeatureTransform(cctx, M, F, 3)
    assert tr.apply_dev(Ad, has, off, keys, xd, F, out, M + 2) == 2   # the (empty) segment 2 and segment 3 belong to key 1
    got = out.cpu().numpy()
    assert (got[:, M:] == -7.0).all()
    ext = torch.cat([torch.ones((T, 1), dtype=torch.float32, device="cuda"), xd], dim=1).contiguous()
    L = cctx.L
    for s, key in enumerate(keys):
        a, b = int(off[s]), int(off[s + 1])
        if b == a:
            continue
        if not has[key]:
            assert np.array_equal(got[a:b, :M].view(np.uint32), x[a:b, :M].view(np.uint32))
            continue
        want = torch.zeros((b - a, M), dtype=torch.float32, device="cuda")
        _lib.check(L.amx_matrix_multiply_dev(cctx.h, Ad[key].data_ptr(), M, F + 1, ext[a:b].data_ptr(), F + 1, b - a, want.data_ptr(), M))
        torch.cuda.synchronize()
        assert np.array_equal(got[a:b, :M].view(np.uint32), want.cpu().numpy().view(np.uint32)), (s, key)
    mine, n_id = cr.apply(A, has, x, off, keys, M, F, contract)
    assert n_id == 2 and np.array_equal(got[:, :M].view(np.uint32), mine.view(np.uint32))
    with pytest.raises(rasr_amd.AmxError, match="overlap"):
        tr.apply_dev(Ad, has, off, keys, xd, F, xd, F)
    with pytest.raises(rasr_amd.AmxError, match="key 5"):
        tr.apply_dev(Ad, has, off, np.array([0, 5, 1, 1], np.int32), xd, F, out, M + 2)


def test_end_to_end_on_the_device(cctx):
    """amx_gmm_score_dev -> amx_align_viterbi_dev -> amx_cmllr_accumulate_dev -> host estimate -> amx_cmllr_apply_dev -> score again: per
    key, the negative log-likelihood of the aligned path with the transform's Jacobian, sum(score) - n log|det A|, does not get worse.
    The tolerance is the f32 scores' own: n x 2^-23 x the largest |score|, plus the estimate's relative bar on the sum."""
    import torch

    import rasr_amd
    D, n_mix, n_keys = 8, 6, 2
    rng = np.random.Generator(np.random.PCG64(77))
    model = synth.gmm_cart(n_mix, 1, 2, D, seed=77, pooled=False)
    lens, keys = [60, 50, 70, 40], np.array([0, 1, 0, 1], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(off[-1])
    # frames drawn from a left-to-right path through the mixtures' first densities, then distorted per key by an affine map
    feats = np.zeros((T, D), np.float32)
    graphs = []
    distort = [(np.eye(D) * 1.3 + rng.standard_normal((D, D)) * 0.05, rng.standard_normal(D) * 0.5) for _ in range(n_keys)]
    for s, n in enumerate(lens):
        path = np.sort(rng.integers(0, n_mix, n))
        for t in range(n):
            d = int(model["mix_offsets"][path[t]])
            z = model["means"][d] + rng.standard_normal(D) * np.sqrt(model["variances"][d])
            B, c = distort[keys[s]]
            feats[off[s] + t] = (B @ z + c).astype(np.float32)
        arcs = [[(i + 1, i, i, 0.0)] + ([(i, i - 1, i - 1, 0.0)] if i > 0 else []) for i in range(n_mix)] + [[(n_mix, n_mix - 1, n_mix - 1, 0.0)]]
        graphs.append(dict(n_states=n_mix + 1, initial=0, final=[False] * n_mix + [True], final_weight=[0.0] * (n_mix + 1), arcs=arcs))
    gmm = rasr_amd.GmmFeatureScorer(cctx, model)
    xd = torch.from_numpy(feats).cuda()
    scores = torch.zeros((T, n_mix), dtype=torch.float32, device="cuda")
    best = torch.zeros((T, n_mix), dtype=torch.int32, device="cuda")
    gmm.score_dev(xd, T, scores, best)
    aligner = rasr_amd.ViterbiAligner(cctx)
    _, emission, _, results, _ = aligner.align(off, graphs, scores, n_mix)
    assert all(r["reached"] for r in results)
    est = rasr_amd.AffineFeatureTransformEstimator(gmm, D, n_keys)
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    est.accumulate_dev(xd, D, off, keys, emission, best, acc, n_mix)
    torch.cuda.synchronize()
    acc_host = acc.cpu().numpy()
    em = emission.cpu().numpy()
    want = cr.accumulate(model, D, n_keys, feats, off, keys, em, best.cpu().numpy().view(np.uint32), n_mix)
    assert np.array_equal(bits(acc_host), bits(want))
    A = np.stack([est.estimate(acc_host, k, iterations=10, min_observation_weight=20.0) for k in range(n_keys)])
    out = torch.zeros((T, D), dtype=torch.float32, device="cuda")
    assert rasr_amd.AffineFeatureTransform(cctx, D, D, n_keys).apply_dev(torch.from_numpy(A).cuda(), np.ones(n_keys, np.int32), off, keys, xd, D, out, D) == 0
    after = torch.zeros((T, n_mix), dtype=torch.float32, device="cuda")
    gmm.score_dev(out, T, after, None)
    torch.cuda.synchronize()
    s0, s1 = scores.cpu().numpy().astype(np.float64), after.cpu().numpy().astype(np.float64)
    bar_rel = float(cr.fixture()["bar/score_rel"])
    for k in range(n_keys):
        ts = np.concatenate([np.arange(off[s], off[s + 1]) for s in range(len(keys)) if keys[s] == k])
        before, now = s0[ts, em[ts]].sum(), s1[ts, em[ts]].sum() - len(ts) * np.log(abs(np.linalg.det(A[k][:, 1:].astype(np.float64))))
        tol = len(ts) * 2.0 ** -23 * max(np.abs(s0[ts]).max(), np.abs(s1[ts]).max()) + bar_rel * len(ts) * abs(before)
        assert now <= before + tol, (k, before, now)
        assert now < before - 0.1 * len(ts)   # the distortion was large: the gain is, too
