"""GPU parity: amx_mllr_accumulate_dev and amx_mllr_adapt_means_dev (mllr.hip) against the restatement of tests/mllr_reference.py, which
tests/test_mllr.py holds to the reference's own text in both of its builds.

Accumulation: every f64 of the flat buffer equals the restatement's bits, in both modes and both contracts, weighted and not, best
densities in both layouts, in one call and cut into two at a frame inside a segment.  Adapted means: every f32 equals the
restatement's.  Every test runs on a few hundred frames at the most."""
import numpy as np
import pytest

from tests import mllr_reference as mr
from tests import synth

pytestmark = pytest.mark.gpu

N_MIX, N_LEAFS, N_KEYS = 6, 4, 3
LEAF_OF_MIXTURE = np.array([0, 1, 1, 3, 0, 1], np.int32)   # leaf 2 receives no frame
MODES = {"full": mr.FULL, "shift": mr.SHIFT}
# the tree over leaves 0 .. 2 (node ids 0 .. 4), leaf 3 is the silence class of mixture 3
TREE = dict(root=0, left=[1, 3, -1, -1, -1], right=[2, 4, -1, -1, -1], previous=[-1, 0, 0, 1, 1], leaf_number=[-1, -1, 2, 0, 1], leaf_list=[3, 4, 2],
            silence_mixtures=[3])


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
    return rasr_amd.ModelTransformEstimator.kernel_shape()


def problem(D, weighted, lens, keys, seed, matrix, leaf1_frames=None, leaf0_segment=None):
    """a model, frames, a segment table and an alignment: some frames carry emission -1, some weights are exactly 0; matrix: the best
    densities as the scorer's [T x n_mix] matrix (else one per frame).  leaf1_frames: how many frames of segment 0 (key 0) go to leaf 1,
    spread over the segment, the others to leaves 0 and 3 or skipped; leaf0_segment: a segment whose frames all go to leaf 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    model = synth.gmm_cart(N_MIX, 1, 3, D, seed=seed, pooled=False)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(off[-1])
    feats = (rng.standard_normal((T, D)) * 1.5 + 0.5).astype(np.float32)
    emission = rng.integers(0, N_MIX, T).astype(np.int32)
    if T > 2:
        emission[rng.random(T) < 0.1] = -1
        emission[1] = -1
    if leaf0_segment is not None:
        emission[off[leaf0_segment]:off[leaf0_segment + 1]] = 0
    if leaf1_frames is not None:
        seg0 = np.arange(off[0], off[1])
        others = rng.choice(np.array([0, 3, 4, -1]), len(seg0))
        emission[seg0] = others
        emission[rng.choice(seg0, leaf1_frames, replace=False)] = rng.choice(np.array([1, 2, 5]), leaf1_frames)
    ks = (model["mix_offsets"][1:] - model["mix_offsets"][:-1]).astype(np.int64)
    if matrix:
        best = np.stack([rng.integers(0, ks[m], T) for m in range(N_MIX)], axis=1).astype(np.uint32)
    else:
        best = np.array([rng.integers(0, ks[e]) if e >= 0 else 0xFFFFFFFF for e in emission], np.uint32)
    weight = None
    if weighted:
        weight = rng.uniform(0.05, 2.0, T)
        weight[rng.random(T) < 0.1] = 0.0
        weight[0] = 0.0
    return dict(model=model, D=D, n_keys=N_KEYS, feats=feats, frame_offsets=off, seg_key=np.array(keys, np.int32), emission=emission, best=best,
                weight=weight, best_ld=N_MIX if matrix else 0)


def device_accumulate(cctx, p, mode, pieces, contract):
    """the device's flat buffer after the calls `pieces` (lists of (offsets, keys)); returns (scorer, estimator, buffer)"""
    import torch

    import rasr_amd
    cctx.set_contract(contract)
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    est = rasr_amd.ModelTransformEstimator(gmm, mode, N_LEAFS, LEAF_OF_MIXTURE, n_keys=p["n_keys"])
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    xd, ed, bd = torch.from_numpy(p["feats"]).cuda(), torch.from_numpy(p["emission"]).cuda(), torch.from_numpy(p["best"].view(np.int32)).cuda()
    wd = torch.from_numpy(p["weight"]).cuda() if p["weight"] is not None else None
    for off, keys in pieces:
        est.accumulate_dev(xd, p["D"], off, keys, ed, bd, acc, p["best_ld"], wd)
    torch.cuda.synchronize()
    return gmm, est, acc.cpu().numpy()


def restate(p, mode, contract):
    return mr.accumulate(p["model"], MODES[mode], p["n_keys"], N_LEAFS, LEAF_OF_MIXTURE, p["feats"], p["frame_offsets"], p["seg_key"], p["emission"],
                         p["best"], p["weight"], contract)


def two_calls(p):
    """the segment table cut at a frame inside segment 0"""
    off = p["frame_offsets"]
    cut = int(off[0] + (off[1] - off[0] + 1) // 2)
    return [(np.clip(off, 0, cut), p["seg_key"]), (np.clip(off, cut, None), p["seg_key"])]


# key 1 receives no segment, leaf 2 no frame; key 0 has two segments around one of key 2.  D = 16 has 17^2 + 16 * 17 + 2 = 563 cells, more
# than one workgroup's 256; 3 and 5 are multiples of nothing.  Leaf 1 of key 0 gets exactly stage, stage + 1 and 2 stage + 1 frames from
# segment 0 (and none from key 0's other segment): its list ends on, crosses and crosses twice the staging boundary
@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("mode", ["full", "shift"])
@pytest.mark.parametrize("D", [3, 5, 16])
def test_accumulation_equals_the_restatement_in_every_bit(cctx, D, mode, contract):
    s, cells = stage()
    assert D != 16 or mr.leaf_size(mr.FULL, D) > 2 * cells
    ls = mr.leaf_size(MODES[mode], D)
    for n1, (weighted, matrix) in zip((s, s + 1, 2 * s + 1), ((True, True), (False, False), (True, False))):
        p = problem(D, weighted, [3 * s + 5, 3, 4, 2], [0, 2, 0, 2], 31 * D + weighted + n1, matrix, leaf1_frames=n1, leaf0_segment=2)
        want = restate(p, mode, contract).reshape(N_KEYS, N_LEAFS, ls)
        assert want[0].any() and want[2].any()
        assert not want[1].any() and not want[:, 2].any()
        if mode == "full" or not weighted:
            assert want[0, 1, 0] == n1
        if mode == "full":
            assert want[0, 1, 1 + D * (D + 1)] == n1   # the counts count frames, weights of 0 included
        _, est, got = device_accumulate(cctx, p, mode, [(p["frame_offsets"], p["seg_key"])], contract)
        assert est.key_size() == N_LEAFS * ls
        assert np.array_equal(bits(got), bits(want.reshape(-1))), np.argwhere(bits(got) != bits(want.reshape(-1)))[:5]
        _, _, cut = device_accumulate(cctx, p, mode, two_calls(p), contract)
        assert np.array_equal(bits(cut), bits(want.reshape(-1)))
        if weighted and mode == "full":   # Z of the weighted full sums is the one site the two contracts differ in
            other = restate(p, mode, "fma" if contract == "off" else "off").reshape(N_KEYS, N_LEAFS, ls)
            g0 = 1 + D * (D + 1)
            assert not np.array_equal(bits(other[..., 1:g0]), bits(want[..., 1:g0])) and np.array_equal(bits(other[..., g0:]), bits(want[..., g0:]))
        elif contract == "fma":
            assert np.array_equal(bits(restate(p, mode, "off")), bits(want.reshape(-1)))


@pytest.mark.parametrize("mode", ["full", "shift"])
def test_one_frame_and_skipped_frames(cctx, mode):
    p = problem(5, True, [1], [2], 7, False)
    p["emission"][0] = 3
    p["best"][0] = 0
    assert p["weight"][0] == 0.0   # a weight of exactly 0 adds the reference's zeros; the full estimator still counts the frame
    _, _, got = device_accumulate(cctx, p, mode, [(p["frame_offsets"], p["seg_key"])], "off")
    want = restate(p, mode, "off")
    assert np.array_equal(bits(got), bits(want)) and want.reshape(N_KEYS, N_LEAFS, -1)[2, 3, 0] == (1.0 if mode == "full" else 0.0)
    p = problem(5, False, [4, 0, 3], [1, 0, 1], 8, True)   # an empty segment; every frame skipped
    p["emission"][:] = -1
    _, _, got = device_accumulate(cctx, p, mode, [(p["frame_offsets"], p["seg_key"])], "off")
    assert not got.any()


def test_refusals_leave_the_buffer_untouched_and_name_the_frame(cctx):
    import torch

    import rasr_amd
    from rasr_amd import _lib
    p = problem(5, True, [6, 5], [0, 1], 10, True)
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    est = rasr_amd.ModelTransformEstimator(gmm, "full", N_LEAFS, LEAF_OF_MIXTURE, n_keys=3)
    mark = 3.25
    acc = torch.full((est.accumulator_size(),), mark, dtype=torch.float64, device="cuda")
    xd, bd, wd = torch.from_numpy(p["feats"]).cuda(), torch.from_numpy(p["best"].view(np.int32)).cuda(), torch.from_numpy(p["weight"]).cuda()

    def refused(match, feats=xd, emission=p["emission"], best=bd, weight=wd, off=p["frame_offsets"], keys=p["seg_key"]):
        with pytest.raises(rasr_amd.AmxError, match=match) as e:
            est.accumulate_dev(feats, 5, off, keys, torch.from_numpy(np.ascontiguousarray(emission)).cuda(), best, acc, p["best_ld"], weight)
        assert e.value.status == _lib.AMX_ERR_INVALID
        assert bool((acc == mark).all())

    for bad in (N_MIX, -2, 1 << 20):
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
    refused("frame_offsets decrease", off=np.array([0, 6, 5], np.int64))
    with pytest.raises(rasr_amd.AmxError, match="NULL"):
        est.accumulate_dev(None, 5, p["frame_offsets"], p["seg_key"], torch.from_numpy(p["emission"]).cuda(), bd, acc, p["best_ld"], wd)
    with pytest.raises(rasr_amd.AmxError, match="n_keys 65536") as e:
        rasr_amd.ModelTransformEstimator(gmm, "full", N_LEAFS, LEAF_OF_MIXTURE, n_keys=65536)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    with pytest.raises(rasr_amd.AmxError, match="band") as e:
        rasr_amd.ModelTransformEstimator(gmm, "band", N_LEAFS, LEAF_OF_MIXTURE)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    # a model in which two (mixture, density) visits reach one mean
    tied = dict(p["model"])
    tied["dens_mean"] = np.array(tied["dens_mean"])
    tied["dens_mean"][-1] = tied["dens_mean"][0]
    with pytest.raises(rasr_amd.AmxError, match="shared means") as e:
        rasr_amd.ModelTransformEstimator(rasr_amd.GmmFeatureScorer(cctx, tied), "full", N_LEAFS, LEAF_OF_MIXTURE)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("mode", ["full", "shift"])
def test_adapted_means_equal_the_restatement_for_an_estimated_and_a_fallback_key(cctx, mode, contract):
    import torch

    import rasr_amd
    D = 5
    p = problem(D, False, [150, 4, 90, 3], [0, 2, 0, 2], 21, True)
    gmm, est, acc = device_accumulate(cctx, p, mode, [(p["frame_offsets"], p["seg_key"])], contract)
    adaptor = rasr_amd.MixtureSetAdaptor(est)
    n_mean = len(p["model"]["means"])
    seen = []
    for key in (0, 2):   # key 2 has 7 frames: the root-only fallback and the silence fallback
        e = est.estimate(acc, TREE, key, min_observation=30.0, min_silence_observation=5.0)
        seen.append((e["root_fallback"], e["silence_fallback"]))
        out = torch.full((n_mean + 1, D), -7.0, dtype=torch.float32, device="cuda")
        adaptor.adapt_means_dev(e["matrix_ids"], e["matrices"], e["matrix_of_mixture"], out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = mr.adapt_means(p["model"], MODES[mode], e["matrix_ids"], e["matrices"], e["matrix_of_mixture"], contract)
        assert np.array_equal(got[:n_mean].view(np.uint32), want.view(np.uint32)) and (got[n_mean] == -7.0).all()
        if key == 2:   # the unit matrix / the zero shift give the means back
            assert np.array_equal(want, p["model"]["means"])
        else:
            assert not np.array_equal(want, p["model"]["means"])
    assert seen == [(False, False), (True, True)]
    e = est.estimate(acc, TREE, 0, min_observation=30.0, min_silence_observation=5.0)
    with pytest.raises(rasr_amd.AmxError, match="is not among"):
        adaptor.adapt_means_dev(e["matrix_ids"][:-1], e["matrices"][:-1], e["matrix_of_mixture"], torch.zeros((n_mean, D), dtype=torch.float32, device="cuda"))


def test_the_loop_on_the_device_does_not_lose_squared_error(cctx):
    """amx_gmm_score_dev's best densities with given labels -> amx_mllr_accumulate_dev -> host estimate -> amx_mllr_adapt_means_dev ->
    amx_gmm_create on the adapted means -> score.  W = Z pinv(G) is the least-squares solution per regression class: computed on the
    host in f64, the sum over the key's frames of |x - W [1, m]|^2 under the estimated matrices is not larger than under the unit
    matrix (relative margin 1e-9 for rounding)."""
    import torch

    import rasr_amd
    D = 6
    rng = np.random.Generator(np.random.PCG64(5))
    model = synth.gmm_cart(N_MIX, 2, 3, D, seed=5, pooled=False)
    lens, keys = [120, 100, 140], np.array([0, 1, 0], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(off[-1])
    emission = rng.integers(0, N_MIX, T).astype(np.int32)
    key_of = np.repeat(keys, lens)
    distort = [(np.eye(D) * 1.2 + rng.standard_normal((D, D)) * 0.05, rng.standard_normal(D) * 0.5) for _ in range(2)]
    feats = np.zeros((T, D), np.float32)
    for t in range(T):
        d = int(model["mix_offsets"][emission[t]]) + int(rng.integers(0, int(model["mix_offsets"][emission[t] + 1] - model["mix_offsets"][emission[t]])))
        B, c = distort[key_of[t]]
        feats[t] = (B @ (model["means"][d] + rng.standard_normal(D) * 0.3 * np.sqrt(model["variances"][d])) + c).astype(np.float32)
    gmm = rasr_amd.GmmFeatureScorer(cctx, model)
    xd, ed = torch.from_numpy(feats).cuda(), torch.from_numpy(emission).cuda()
    scores = torch.zeros((T, N_MIX), dtype=torch.float32, device="cuda")
    best = torch.zeros((T, N_MIX), dtype=torch.int32, device="cuda")
    gmm.score_dev(xd, T, scores, best)
    est = rasr_amd.ModelTransformEstimator(gmm, "full", N_LEAFS, LEAF_OF_MIXTURE, n_keys=2)
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    est.accumulate_dev(xd, D, off, keys, ed, best, acc, N_MIX)
    torch.cuda.synchronize()
    acc_host, best_host = acc.cpu().numpy(), best.cpu().numpy().view(np.uint32)
    want = mr.accumulate(model, mr.FULL, 2, N_LEAFS, LEAF_OF_MIXTURE, feats, off, keys, emission, best_host)
    assert np.array_equal(bits(acc_host), bits(want))
    adaptor = rasr_amd.MixtureSetAdaptor(est)
    mean_of = np.array([int(model["dens_mean"][mr.frame_density(model, emission[t], best_host[t, emission[t]])]) for t in range(T)])
    x64 = feats.astype(np.float64)
    before = scores.cpu().numpy().astype(np.float64)
    for key in range(2):
        e = est.estimate(acc_host, TREE, key, min_observation=25.0, min_silence_observation=10.0)
        assert not e["root_fallback"] and not e["silence_fallback"]
        where = {int(i): n for n, i in enumerate(e["matrix_ids"])}
        ts = np.flatnonzero(key_of == key)
        ext = np.concatenate([np.ones((len(ts), 1)), model["means"][mean_of[ts]].astype(np.float64)], axis=1)
        W = np.stack([e["matrices"][where[int(e["matrix_of_mixture"][emission[t]])]] for t in ts])
        now = float(((x64[ts] - np.einsum("tij,tj->ti", W, ext)) ** 2).sum())
        unit = float(((x64[ts] - ext[:, 1:]) ** 2).sum())
        assert now <= unit * (1 + 1e-9), (key, unit, now)
        assert now < 0.5 * unit   # the distortion was large: the gain is, too
        out = torch.zeros((len(model["means"]), D), dtype=torch.float32, device="cuda")
        adaptor.adapt_means_dev(e["matrix_ids"], e["matrices"], e["matrix_of_mixture"], out)
        torch.cuda.synchronize()
        adapted = dict(model)
        adapted["means"] = out.cpu().numpy()
        assert np.array_equal(adapted["means"].view(np.uint32),
                              mr.adapt_means(model, mr.FULL, e["matrix_ids"], e["matrices"], e["matrix_of_mixture"], "off").view(np.uint32))
        after = torch.zeros((T, N_MIX), dtype=torch.float32, device="cuda")
        rasr_amd.GmmFeatureScorer(cctx, adapted).score_dev(xd, T, after, None)
        torch.cuda.synchronize()
        a = after.cpu().numpy().astype(np.float64)
        assert a[ts, emission[ts]].sum() < before[ts, emission[ts]].sum()   # the adapted scorer fits the key's frames better
