"""tests/posterior_reference.py -- Mm::StatePosteriorFeatureScorer (viterbi = true) and Mm::CombinedFeatureScorer restated in numpy: what
the GPU tests compare against.  f64 throughout (f32 for the combination); sums run in increasing index order.  tests/test_posterior.py
holds this file to tests/golden/ref_posterior.npz, which the reference's own text computed.

Line numbers are those of Mm/StatePosteriorFeatureScorer.cc."""
import math

import numpy as np

DBL_MAX = np.finfo(np.float64).max


def fma(a, b, c):
    """a * b + c rounded once, for f64 arrays: formed exactly in rationals, then rounded to nearest even"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    out = np.empty(a.shape, np.float64)
    it = np.nditer([a, b, c, out], op_flags=[["readonly"], ["readonly"], ["readonly"], ["writeonly"]])
    for x, y, z, o in it:
        o[...] = _fma1(float(x), float(y), float(z))
    return out


def _fma1(x, y, z):
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return x * y + z
    from fractions import Fraction
    r = Fraction(x) * Fraction(y) + Fraction(z)
    try:
        return float(r)   # Fraction -> float rounds to nearest even
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def scores_s(scores, scale, prior, contract_fma=False):
    """s = prior + scale * score (:43, :90, :265) for f32 scores; contract_fma: as the reference's -march=native build contracts it"""
    x = np.asarray(scores, np.float32).astype(np.float64)
    if contract_fma:
        return fma(np.float64(scale), x, prior)
    return np.asarray(prior, np.float64) + np.float64(scale) * x


def frame_posteriors(s, in_filter, threshold=DBL_MAX, margin=0.0, margin_mixture=-1, likelihood=False):
    """one frame.  s [n] f64 (un-margined), in_filter [n] bool.  Returns dict(stored, survivors, min, min_index, log_z, post):
    stored / post are [n] with 0 outside the survivors, min_index -1 (min DBL_MAX, log_z 0) where no mixture has s < DBL_MAX or the
    minimum is -inf."""
    n = len(s)
    s = np.asarray(s, np.float64)
    with np.errstate(invalid="ignore"):
        cand = np.where(np.asarray(in_filter, bool) & (s < DBL_MAX), s, np.inf)   # :49-52: strict < from DBL_MAX, so no NaN and no +inf
    mi = int(np.argmin(cand)) if n and np.any(cand < np.inf) else -1                # the first index wins
    mn = float(s[mi]) if mi >= 0 else DBL_MAX
    out = dict(stored=np.zeros(n), survivors=np.zeros(n, bool), min=mn, min_index=mi, log_z=0.0, post=np.zeros(n))
    if mi < 0 or not mn >= -DBL_MAX:
        out["min"], out["min_index"] = DBL_MAX, -1
        return out
    stored = np.array(s, np.float64)
    if margin_mixture >= 0:
        stored[margin_mixture] = stored[margin_mixture] + np.float64(margin)   # :46-48
    surv = np.array(in_filter, bool)
    if threshold < DBL_MAX:   # :105-116
        with np.errstate(over="ignore"):
            limit = np.float64(threshold) + mn
        surv &= stored < limit
    with np.errstate(all="ignore"):
        rest = surv.copy()
        rest[mi] = False
        terms = np.exp(mn - stored[rest])   # :133-138
        total = float(np.cumsum(terms)[-1]) if len(terms) else 0.0   # cumsum adds one after the other, in increasing index order
        log_zs = math.log1p(total)
        if likelihood:
            post = np.where(surv, np.exp(-stored), 0.0)
        else:
            post = np.where(surv, np.exp((mn - stored) - log_zs), 0.0)   # :140-142
    out.update(stored=np.where(surv, stored, 0.0), survivors=surv, log_z=log_zs - mn, post=post)
    return out


def posteriors(scores, scale=1.0, prior=None, in_filter=None, threshold=DBL_MAX, margin=0.0, margin_mixture=None, likelihood=False,
               contract_fma=False):
    """a batch: scores [T, n] f32; prior [n] f64 (None: 0); in_filter [n] bool (None: all); margin_mixture [T] (None: none).
    Returns dict of arrays: s [T, n], stored, survivors, post (f64), post32, min, min_index, log_z, n_survivors."""
    scores = np.asarray(scores, np.float32)
    T, n = scores.shape
    prior = np.zeros(n) if prior is None else np.asarray(prior, np.float64)
    in_filter = np.ones(n, bool) if in_filter is None else np.asarray(in_filter, bool)
    s = scores_s(scores, scale, prior[None, :], contract_fma) if T else np.zeros((0, n))
    r = dict(s=s, stored=np.zeros((T, n)), survivors=np.zeros((T, n), bool), post=np.zeros((T, n)), min=np.zeros(T), min_index=np.zeros(T, np.int32),
             log_z=np.zeros(T), n_survivors=np.zeros(T, np.int32))
    for t in range(T):
        f = frame_posteriors(s[t], in_filter, threshold, margin, -1 if margin_mixture is None else int(margin_mixture[t]), likelihood)
        for k in ("stored", "survivors", "post", "min", "min_index", "log_z"):
            r[k][t] = f[k]
        r["n_survivors"][t] = int(f["survivors"].sum())
    r["post32"] = r["post"].astype(np.float32)
    return r


def sparse_rows(r, keys=None):
    """the survivors' (index, f32 value) per frame in increasing MIXTURE order, as the device emits them; keys [T, n]: density-keyed"""
    rows = []
    for t in range(r["post"].shape[0]):
        m = np.nonzero(r["survivors"][t])[0]
        rows.append(((keys[t, m] if keys is not None else m).astype(np.int32), r["post32"][t, m]))
    return rows


def density_keys(topo_off, topo, best):
    """key[t, m] = topology[m][best[t, m]]"""
    return np.asarray(topo)[np.asarray(topo_off)[:-1][None, :].astype(np.int64) + np.asarray(best).astype(np.int64)].astype(np.int64)


def list_posteriors(scores, scale, offsets, mixture, prior, contract_fma=False):
    """posteriorsAndMixtures(IndicesAndWeights&) (:258-284): one f64 posterior per list entry; the first minimum in list order"""
    scores = np.asarray(scores, np.float32)
    out = np.zeros(len(mixture))
    n = scores.shape[1]
    for t in range(len(offsets) - 1):
        b, e = int(offsets[t]), int(offsets[t + 1])
        if e <= b:
            continue
        mix = np.asarray(mixture[b:e])
        ok = (mix >= 0) & (mix < n)
        x = np.where(ok, scores[t, np.where(ok, mix, 0)].astype(np.float64), np.inf)
        if contract_fma:
            s = fma(np.float64(scale), x, np.asarray(prior[b:e], np.float64))
        else:
            s = np.asarray(prior[b:e], np.float64) + np.float64(scale) * x
        mn, mi = DBL_MAX, -1
        for i in range(e - b):
            if s[i] < mn:
                mn, mi = s[i], i
        if mi < 0 or not mn >= -DBL_MAX:
            continue
        total = 0.0
        for i in range(e - b):
            if i != mi and mn - s[i] > -800:
                total += math.exp(mn - s[i])
        with np.errstate(all="ignore"):
            out[b:e] = np.exp((mn - s) - math.log1p(total))
    return out


def combine(table, scale, mats):
    """CombinedContextScorer::score (CombinedFeatureScorer.cc:42-59): f32, the models' terms in model order, every step rounded"""
    table = np.asarray(table)
    T = mats[0].shape[0]
    out = np.zeros((T, table.shape[0]), np.float32)
    for i, m in enumerate(mats):
        term = np.float32(scale[i]) * np.asarray(m, np.float32)[:, table[:, i]]
        out = (out + term.astype(np.float32)).astype(np.float32)
    return out


def midpoint_distance(x):
    """relative distance of each f64 value to the nearest midpoint between two neighbouring f32 values; 1 for 0 and values outside f32"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        f = x.astype(np.float32)
        lo = np.where(f.astype(np.float64) <= x, f, np.nextafter(f, np.float32(-np.inf)))
        hi = np.nextafter(lo, np.float32(np.inf))
        mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
        d = np.abs(x - mid) / np.abs(x)
    d[~np.isfinite(d) | (x == 0)] = 1.0
    return np.minimum(d, 1.0)


def ulp_distance32(a, b):
    """distance in f32 steps between two non-negative f32 arrays"""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))
