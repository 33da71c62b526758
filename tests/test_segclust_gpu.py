"""GPU: the segment clustering (segclust.hip) against tests/segclust_reference.py.  The sums equal the reference's frame-order f64 chains
in every bit.  Nothing behind an LU can be pinned to LAPACK's bits, so R, the distances and the tracker scores carry the bars of DESIGN.md
section 6 (4 times the largest deviation measured over these cases, one f32 rounding where none was), and the merge loop is checked by replaying the device's merges through
the reference.  Every test prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import segclust_reference as sr

pytestmark = pytest.mark.gpu

# Measured on an MI355X over the cases below: R and the tracker scores equal the restatement's f32 in every cell (deviation 0), the distances
# deviate by at most 2.98e-8 absolute and 3.39e-7 relative.  Four times zero is no bar: where nothing was measured the bar is ONE rounding of
# the f32 the value is narrowed to, 2^-23 relative to R, and for a score 2^-22 of the largest |likelihood| its three terms can have (the score
# is half a difference of f32 likelihoods; one of them one ulp off moves it by that much).
BAR_R_REL = 2.0 ** -23                                  # relative to |R|; must stay below 2^-20
BAR_DIST_ABS, BAR_DIST_REL = 4 * 2.98e-8, 4 * 3.39e-7   # relative where |distance| >= 1e-3
BAR_SCORE_LIKE = 2.0 ** -22                             # times the largest |likelihood| of the replay


def device(ctx, D, segs, calls=1, debug=True, **params):
    import torch
    ctx.use_torch_stream()
    sc = rasr_amd.SegmentClustering(ctx, D, **params)
    sc.set_debug(debug)
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    xd = torch.from_numpy(np.concatenate(segs)).cuda()
    cuts = np.linspace(0, len(segs), calls + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        sc.accumulate_dev(xd, off[a:b + 1])
    return sc, xd, off


@functools.lru_cache(maxsize=None)
def problem(N, D, seed=0):
    """N segments of >= 4 D frames of full-rank Gaussian data around 3 well-separated means, one of them replaced by a one-frame segment;
    the reference's models, R, automatic alpha and features, computed once"""
    rng = np.random.Generator(np.random.PCG64(1000 * N + D + seed))
    means = rng.standard_normal((3, D)) * 4.0
    segs = [(rng.standard_normal((4 * D + int(rng.integers(0, 20)), D)) * rng.uniform(0.5, 1.5, D) + means[i % 3]).astype(np.float32) for i in range(N)]
    segs[N // 2] = segs[N // 2][:1]
    models = [sr.finalize(s)[0] for s in segs]
    R = sr.relative_likelihoods(models, models)
    alpha, seen = sr.auto_alpha(R)
    return dict(segs=segs, models=models, R=R, alpha=alpha, seen=seen, F=[sr.feature(r, alpha) for r in R])


@pytest.mark.parametrize("D", [1, 3, 17, 45, 64])
def test_sums_equal_the_frame_order_chains_in_every_bit(ctx, D):
    stage = rasr_amd.SegmentClustering.kernel_shape()["stage_frames"]
    rng = np.random.Generator(np.random.PCG64(D))
    segs = [(rng.standard_normal((n, D)) * 3 + 1).astype(np.float32) for n in (1, stage - 1, stage, stage + 1, 3 * stage + 5)]
    want = np.stack([np.concatenate([s, q[np.tril_indices(D)]]) for s, q in map(sr.sums, segs)])
    for calls in (1, 3):
        sc, _, _ = device(ctx, D, segs, calls)
        assert np.array_equal(sc.debug_read("sums").view(np.uint64), want.view(np.uint64)), "%d call(s)" % calls


def test_finalize_uses_the_f32_reciprocal_and_counts_the_regularised_model(ctx):
    rng = np.random.Generator(np.random.PCG64(3))
    segs = [(rng.standard_normal((n, 2)) + 2).astype(np.float32) for n in (3, 1, 9)]
    sc, _, _ = device(ctx, 2, segs, alpha=0.0012)
    out, got = sc.cluster(), sc.debug_read("models")
    assert out["n_regularised"] == 1 and out["alpha"] == np.float32(0.0012) and out["alpha_iterations"] == 0
    for s, g in zip(segs, got):
        m, bumps = sr.finalize(s)
        assert bumps == (len(s) == 1)
        assert np.array_equal(g[:2], m.mean)   # n = 3: sum * f64(1.0F / 3) differs from sum * (1.0 / 3)
        np.testing.assert_allclose(g[2:6].reshape(2, 2), m.var, rtol=0, atol=1e-15 * np.abs(m.var).max())
    s3, _ = sr.sums(segs[0])
    assert not np.array_equal(got[0][:2], s3 * (1.0 / 3))
    assert np.array_equal(got[1][2:6], [0.1, 0, 0, 0.1])


@pytest.mark.parametrize("D", [1, 16, 17, 45, 64])
@pytest.mark.parametrize("N", [2, 15, 16, 17, 33, 70])
def test_relative_likelihoods_and_initial_distances(ctx, N, D):
    p = problem(N, D)
    sc, _, _ = device(ctx, D, p["segs"], alpha=float(p["alpha"]), mincluster=1)
    sc.cluster()
    R, dist, want = sc.debug_read("R"), sc.debug_read("dist"), sr.initial_distances(p["F"])
    r_rel = np.abs(R.astype(np.float64) - p["R"]) / np.abs(p["R"])
    d_abs, big = np.abs(dist.astype(np.float64) - want), np.abs(want) >= 1e-3
    d_rel = (d_abs[big] / np.abs(want[big])).max() if big.any() else 0.0
    print("N %d D %d: R rel %.3g, dist abs %.3g rel %.3g" % (N, D, r_rel.max(), d_abs.max(), d_rel))
    assert r_rel.max() <= BAR_R_REL < 2.0 ** -20
    assert d_abs.max() <= BAR_DIST_ABS and d_rel <= BAR_DIST_REL


@pytest.mark.parametrize("N, D", [(33, 16), (70, 16), (17, 45)])
def test_automatic_alpha_equals_the_reference(ctx, N, D):
    p = problem(N, D)
    lo, hi = np.float32(0.40), np.float32(0.60)
    margin = min(min(abs(a - lo), abs(a - hi)) for a in p["seen"])
    print("alpha %r after %d steps, the averages stay %.3g from the bounds" % (p["alpha"], len(p["seen"]), margin))
    assert margin > BAR_DIST_ABS, "precondition: an average of the reference's bisection lies within the bar of a bound"
    sc, _, _ = device(ctx, D, p["segs"], mincluster=1)
    out = sc.cluster()
    assert lo <= p["seen"][-1] <= hi and out["alpha"] == p["alpha"] and out["alpha_iterations"] == len(p["seen"])


@pytest.mark.parametrize("amalgamation, minframes", [(0, 0), (1, 0), (0, 70), (1, 70)])
def test_merge_loop_by_replay_and_final_class_ids(ctx, amalgamation, minframes):
    N, D = 70, 16
    p = problem(N, D)
    keep = [i for i, s in enumerate(p["segs"]) if len(s) >= minframes]
    models = [p["models"][i] for i in keep]
    R = p["R"][np.ix_(keep, keep)]
    sc, _, _ = device(ctx, D, p["segs"], alpha=float(p["alpha"]), amalgamation=amalgamation, minframes=minframes)
    out = sc.cluster()
    tp, tc, ts = out["tracker"]
    thr = np.float32(out["threshold"])   # the host's own f32 logarithm; the restatement's may round the last bit the other way
    assert out["n_segments"] == len(keep) < N + (minframes == 0) and out["n_filtered"] == N - len(keep)
    assert abs(thr - sr.threshold(0.0, D, 1.0, sum(m.n for m in models))) <= 2.0 ** -22 * thr
    replay, picks, lmax = sr.cluster(models, R, p["alpha"], thr, amalgamation, forced=list(zip(tp, tc)))
    own = sr.cluster(models, R, p["alpha"], thr, amalgamation)[0]
    over = max(float(d) - float(m) for d, m in picks)
    s_abs = max(abs(float(a) - float(b[2])) for a, b in zip(ts, replay))
    s_rel = max(abs(float(a) - float(b[2])) / abs(float(b[2])) for a, b in zip(ts, replay) if abs(b[2]) >= 1)
    print("amalgamation %d minframes %d: pick over the minimum %.3g, score abs %.3g rel %.3g, largest |likelihood| %.3g" %
          (amalgamation, minframes, over, s_abs, s_rel, lmax))
    assert over <= BAR_DIST_ABS and s_abs <= BAR_SCORE_LIKE * lmax
    ids, best, seen = sr.choose(own, len(keep))
    gap = np.sort(np.asarray(seen, np.float64))
    assert gap[1] - gap[0] > len(keep) * BAR_SCORE_LIKE * lmax, "precondition: the reference's BIC minimum is not separated from the runner-up"
    want = np.zeros(N, np.int32)
    want[keep] = ids + (len(keep) < N)
    assert np.array_equal(out["class_ids"], want) and out["best_index"] == best and out["n_clusters"] == len(set(ids))


def test_refusals_leave_the_handle_usable(ctx):
    import torch
    p = problem(15, 3)
    with pytest.raises(rasr_amd.AmxError, match="dim"):
        rasr_amd.SegmentClustering(ctx, 65)
    sc, xd, off = device(ctx, 3, p["segs"], debug=False)
    sc.reset()
    for kw, status in [(dict(), _lib.AMX_ERR_INVALID), (dict(infile="spk.cl"), _lib.AMX_ERR_UNSUPPORTED)]:
        with pytest.raises(rasr_amd.AmxError) as e:
            sc.cluster(**kw)
        assert e.value.status == status
    bad = xd.clone()
    bad[int(off[4]) + 1, 2] = float("nan")
    with pytest.raises(rasr_amd.AmxError, match="not finite"):
        sc.accumulate_dev(bad, off)
    assert sc.segments() == 0
    sc.accumulate_dev(xd, off)
    with pytest.raises(rasr_amd.AmxError, match="mincluster") as e:
        sc.cluster(infile=None, mincluster=16)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    fresh, _, _ = device(ctx, 3, p["segs"], debug=False)
    assert np.array_equal(sc.cluster(mincluster=2)["class_ids"], fresh.cluster()["class_ids"])
    torch.cuda.synchronize()


def test_class_ids_feed_cmllr_as_segment_keys(ctx):
    import torch

    from tests import synth
    p = problem(15, 16)
    sc, xd, off = device(ctx, 16, p["segs"], debug=False)
    keys = sc.cluster()["class_ids"]
    assert keys.min() >= 0 and keys.max() < len(keys) and len(set(keys)) < len(keys)
    est = rasr_amd.AffineFeatureTransformEstimator(rasr_amd.GmmFeatureScorer(ctx, synth.gmm_cart(4, 1, 3, 16, seed=5, pooled=False)), 16, int(keys.max()) + 1)
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    T = int(off[-1])
    est.accumulate_dev(xd, 16, off, keys, torch.zeros(T, dtype=torch.int32, device="cuda"), torch.zeros(T, dtype=torch.int32, device="cuda"), acc)
    beta = acc.cpu().numpy().reshape(int(keys.max()) + 1, -1)[:, 0]
    assert np.array_equal(beta, np.bincount(keys, weights=np.diff(off), minlength=len(beta)))
