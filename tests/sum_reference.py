"""High-precision restatement of the log-add ("diagonal-sum") GMM scorer, built from the reference's own per-density terms.

GaussDiagonalSumFeatureScorer::calculateScoreAndDensity forms, per frame and mixture, the f32 entries
s_k = (f32)(0.5 * ((m2lw_k + logNorm_c) + dist_k)) (OracleGmm.sum_entries), picks the first strict minimum b (`if (best > s_k)`
from FLT_MAX: an entry that is NaN or >= FLT_MAX is never picked, and if none is, the density is "none", 0xffffffff) and returns
b - log sum_k exp(b - s_k) in f32.  `sum_value` evaluates that expression in float64 on the same entries, so the only error left in
it is the f64 rounding; `check_sum` holds a scored matrix to it and to the oracle.  The adversarial models below make every entry a
new running minimum (or none after the first), the order in which a one-pass online log-sum-exp rounds worst.
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
NO_DENSITY = 0xFFFFFFFF


def sum_value(entries, mix_offsets, max_block=1 << 22):
    """entries [T, sum K_m] f32 -> (value [T, n_mix] f64, best density in mixture [T, n_mix] u32), the reference's rule in f64.
    Every mixture needs at least one density."""
    entries = np.asarray(entries, np.float32)
    off = np.asarray(mix_offsets, np.int64)
    T, n_mix = entries.shape[0], len(off) - 1
    ks = np.diff(off)
    assert (ks > 0).all(), "a mixture without densities"
    value = np.empty((T, n_mix), np.float64)
    best = np.empty((T, n_mix), np.uint32)
    m0 = 0
    while m0 < n_mix:   # blocks of whole mixtures, ~max_block entries each (a tied model at full size has 41M entries per frame)
        m1 = max(m0 + 1, int(np.searchsorted(off, off[m0] + max_block, side="right")) - 1)
        m1 = min(m1, n_mix)
        lo, hi = int(off[m0]), int(off[m1])
        seg = np.repeat(np.arange(m1 - m0), ks[m0:m1])
        starts = (off[m0:m1] - lo).astype(np.intp)
        pos = np.arange(hi - lo) - starts[seg]
        for t in range(T):
            s = entries[t, lo:hi].astype(np.float64)
            cand = np.where(s < FLT_MAX, s, np.inf)          # NaN, +inf and FLT_MAX itself never win `best > s`
            b = np.minimum.reduceat(cand, starts)
            has = b < np.inf
            b = np.where(has, b, FLT_MAX)
            bk = b[seg]
            first = np.minimum.reduceat(np.where(has[seg] & (cand == bk), pos, np.iinfo(np.int64).max), starts)
            best[t, m0:m1] = np.where(has, first, NO_DENSITY)
            with np.errstate(all="ignore"):
                value[t, m0:m1] = b - np.log(np.add.reduceat(np.exp(bk - s), starts))
        m0 = m1
    return value, best


def own_error_bound(value, ks):
    """a bound on the f32 rounding of the reference's two-pass evaluation for K entries: every term exp(b - s_k) <= 1 carries
    ~2 ulp (the subtraction and expf), the K-term f32 sum ~K ulp of at most K, logf 1 ulp, the final subtraction half an ulp"""
    return 2.0 ** -21 * (np.asarray(ks, np.float64) + 2) + 2.0 ** -22 * np.abs(value)


def finite_match(got, want):
    """NaN where and only where the f64 value is NaN, +-inf exactly where it is infinite; the mask of finite entries"""
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), "infinite scores differ"
    fin = np.isfinite(want)
    assert np.isfinite(got[fin]).all(), "finite scores became non-finite"
    return fin


def check_sum(sc, best, model, x, contract="off", mixture_weight_scale=1.0, gaussian_scale=1.0, frames=None, oracle=None):
    """hold a device log-add result (sc, best [T, n_mix], or only the given `frames` rows of it) to
      (a) the oracle, allclose(rtol=1e-5, atol=1e-5) -- the bar the scorer has always been held to;
      (b) the oracle's best density, bit for bit;
      (c) the f64 value: |dev - f64| <= 4 |orc - f64| + 1e-6 max(1, |f64|), NaN / +-inf where the f64 value has them.
    Returns (max |dev - f64|, max |orc - f64|) over the finite entries."""
    from oracle import OracleGmm
    if frames is not None:
        x, sc, best = x[frames], sc[frames], best[frames]
    orc = oracle or OracleGmm(model, mixture_weight_scale=mixture_weight_scale, gaussian_scale=gaussian_scale, contract=contract)
    osc, obest = orc.score(x, mode=1)
    ref, rbest = sum_value(orc.sum_entries(x), model["mix_offsets"])
    assert np.allclose(sc, osc, rtol=1e-5, atol=1e-5, equal_nan=True), "(a) max |dev - orc| = %g" % np.nanmax(np.abs(sc - osc))
    bad = np.argwhere(best != obest)
    assert bad.size == 0, "(b) best density differs at (frame, mixture) %s: %d vs %d" % (bad[0], best[tuple(bad[0])], obest[tuple(bad[0])])
    assert np.array_equal(rbest, obest)   # the f64 restatement picks the oracle's density (tests/test_oracle.py pins this on the CPU)
    fin = finite_match(sc, ref)
    assert np.array_equal(np.isnan(osc), np.isnan(ref))
    e_dev = np.abs(sc.astype(np.float64)[fin] - ref[fin])
    e_orc = np.abs(osc.astype(np.float64)[fin] - ref[fin])
    lim = 4 * e_orc + 1e-6 * np.maximum(1.0, np.abs(ref[fin]))
    over = e_dev > lim
    if over.any():
        i = int(np.argmax(e_dev - lim))
        raise AssertionError("(c) %d scores further from the f64 value than 4x the reference's own error: worst |dev - f64| = %.3g "
                             "(f64 %.9g, |orc - f64| = %.3g, limit %.3g); max |dev - f64| %.3g, max |orc - f64| %.3g"
                             % (int(over.sum()), e_dev[i], ref[fin][i], e_orc[i], lim[i], e_dev.max(), e_orc.max()))
    return (float(e_dev.max()) if e_dev.size else 0.0), (float(e_orc.max()) if e_orc.size else 0.0)


def line_model(K, gap, dim=16, order="falling", value_at=None, n_mix=1, tied=False, lists=None):
    """densities on a line through the origin (axis 0), the frame 0 at one end: entry k of every list has distance
    base + 2 gap (K - 1 - k) ("falling": every entry a new minimum) or base + 2 gap k ("rising"), so the entries step by `gap`.
    value_at: the per-density constant moved through the variances of the other axes (the means sit on the frame there) so that
    the frame's score b - log sum exp(b - s_k) lies near this value (0: where an absolute tolerance of 1e-5 is the whole bar).
    Equal weights.  tied=False: CART (every mixture owns its K densities, all on the same K means); tied=True: n_mix mixtures
    over K shared densities, `lists` [n_mix] of "falling" / "rising" (default all `order`)."""
    base = 1.0
    step = 2.0 * gap * np.arange(K, dtype=np.float64)
    d2 = base + (step[::-1] if order == "falling" else step)
    means = np.zeros((K, dim), np.float32)
    means[:, 0] = np.sqrt(d2).astype(np.float32)
    var = np.ones((1, dim), np.float64)
    if value_at is not None:
        assert dim > 1
        b = value_at + np.log(np.exp(-gap * np.arange(K)).sum())      # the smallest entry that puts the score at value_at
        var[0, 1:] = np.exp((2 * b - 2 * np.log(K) - dim * np.log(2 * np.pi) - base) / (dim - 1))
    variances = var.astype(np.float32)
    if tied:
        lists = lists or [order] * n_mix
        perm = {order: np.arange(K, dtype=np.uint32), ("rising" if order == "falling" else "falling"): np.arange(K - 1, -1, -1, dtype=np.uint32)}
        idx = np.concatenate([perm[l] for l in lists])
        n_dens, dens_mean = K, np.arange(K, dtype=np.uint32)
    else:
        idx = np.arange(n_mix * K, dtype=np.uint32)
        n_dens, dens_mean = n_mix * K, np.tile(np.arange(K, dtype=np.uint32), n_mix)
    off = (np.arange(n_mix + 1, dtype=np.uint64) * K).astype(np.uint32)
    return dict(dim=dim, mix_offsets=off, dens_index=idx, log_weight=np.full(n_mix * K, -np.log(K), np.float64),
                dens_mean=dens_mean, dens_cov=np.zeros(n_dens, np.uint32), means=means, variances=variances)


def line_frames(model, n_random=6, seed=0):
    """the frame at the origin (the line's near end), one beyond the far end of the line (the order reversed, uneven steps)
    and a few random ones"""
    dim = int(model["dim"])
    x = np.zeros((2 + n_random, dim), np.float32)
    x[1, 0] = np.float32(model["means"][:, 0].max() + 1.0)
    x[2:] = np.random.Generator(np.random.PCG64(seed)).standard_normal((n_random, dim)).astype(np.float32)
    return x
