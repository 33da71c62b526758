"""Restatement of Signal::QuantileEqualization in segment mode (Signal/QuantileEqualization.{hh,cc}) in both of the reference's
arithmetics, for tests/test_quanteq.py (against the fixture of tests/golden/make_quanteq_golden.py) and tests/test_quanteq_gpu.py.

f32 stays f32 (numpy float32 arrays), the double expressions are float64.  pow is libm's (ctypes), not numpy's.  The fused operations of
the contract=fma build are vectorised here (a grid search is 121 203 of them per channel, too many for one ctypes call each): fmaf as the
exact f64 product, an error-free sum and rounding to odd before the narrowing; fma as an error-free product and sum of three with
rounding to odd (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums: proved algorithms using rounding to odd", 2008).
Neither rounds twice; tests/test_quanteq.py checks both against libm's fma / fmaf through ctypes.

`variant` switches on one wrong reading at a time, so that the tests can show the fixture tells them apart:
  last_minimum   `<=` instead of `<` in the two searches
  linear_grid    grids lo + k * step instead of the accumulating f32 loop variable
  powf           the f32 power function
  newest_first   the f64 sums from the newest frame to the oldest
"""
import ctypes
import ctypes.util

import numpy as np

F32, F64 = np.float32, np.float64
FLT_MAX = np.finfo(np.float32).max

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3
_libc = ctypes.CDLL(ctypes.util.find_library("c"))
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]

DEFAULTS = dict(quantiles=1, combination=0, estimate=0, mean=1, variance=0, nq=4, of=1.0, delta_alpha=0.005, delta_gamma=0.01, delta_lr=0.005,
                beta=0.05, pool=1)


def libm_fma(a, b, c):
    return _libm.fma(a, b, c)


def libm_fmaf(a, b, c):
    return F32(_libm.fmaf(a, b, c))


def pow_f64(x, y, powf=False):
    """libm's pow on broadcast float64 arrays (powf: the f32 function on the narrowed arguments, widened)"""
    x, y = np.broadcast_arrays(np.asarray(x, F64), np.asarray(y, F64))
    if powf:
        return np.array([_libm.powf(a, b) for a, b in zip(x.ravel().tolist(), y.ravel().tolist())], F64).reshape(x.shape)
    return np.array([_libm.pow(a, b) for a, b in zip(x.ravel().tolist(), y.ravel().tolist())], F64).reshape(x.shape)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _to_odd(s, err):
    """s = RN(exact), err = exact - s: the neighbour of the exact value whose last bit is odd (s itself where exact)"""
    s = np.array(s, F64)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    if fix.any():
        s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    return s


def fmaf(a, b, c):
    """f32 a * b + c with one rounding"""
    with np.errstate(all="ignore"):
        p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)   # exact: 48 bits
        s, err = _two_sum(p, np.asarray(c, F32).astype(F64))
        return _to_odd(s, err).astype(F32)


def _split(x):
    t = 134217729.0 * x
    hi = t - (t - x)
    return hi, x - hi


def fma(a, b, c):
    """f64 a * b + c with one rounding"""
    with np.errstate(all="ignore"):
        a, b, c = np.broadcast_arrays(np.asarray(a, F64), np.asarray(b, F64), np.asarray(c, F64))
        uh = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
        th, tl = _two_sum(c, uh)
        v = _to_odd(*_two_sum(tl, ul))
        z = th + v
        return np.where(np.isfinite(z), z, uh + c)


def mad32(fused, a, b, c):
    with np.errstate(all="ignore"):
        return fmaf(a, b, c) if fused else (np.asarray(a, F32) * np.asarray(b, F32) + np.asarray(c, F32)).astype(F32)


def mad64(fused, a, b, c):
    with np.errstate(all="ignore"):
        return fma(a, b, c) if fused else np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)


def grid(lo, hi, step_f32, linear=False):
    """QuantileEqualization.cc:202-203: `for (f32 a = lo; a <= hi; a += (f64)step)`, the step set through an f32 setter"""
    step = F64(F32(step_f32))
    out, a, k = [], F32(lo), 0
    while a <= F32(hi):
        out.append(a)
        k += 1
        a = F32(F64(lo) + k * step) if linear else F32(F64(a) + step)
    return np.array(out, F32)


def grids(cfg, linear=False):
    return (grid(0.0, 1.0, cfg["delta_alpha"], linear), grid(1.0, 3.0, cfg["delta_gamma"], linear), grid(0.0, 0.5, cfg["delta_lr"], linear))


def std_max(a, b):
    return np.where(a < b, b, a)


def quantiles(x, nq):
    """:163-174 -> [(nq + 1), dim]"""
    T = len(x)
    s = np.sort(x, axis=0)
    return np.stack([s[(i * (T - 1)) // nq] for i in range(nq + 1)]).astype(F32)


def read_quantile_file(text, dim, nq, pool):
    """readTrainingQuantilesFromFile (:70-101) on the file's bytes"""
    tok = bytes(text).split()
    tq = np.zeros((nq + 1, dim), F32)
    k = 0
    for d in range(dim):
        k += 1
        for i in range(nq + 1):
            tq[i, d] = _libc.strtof(tok[k], None)
            k += 1
    if pool:
        for i in range(nq + 1):
            tq[i, :] = np.cumsum(tq[i], dtype=F32)[-1] / F32(dim)   # f32 sum in channel order
    return tq


def write_quantile_file(sums, count):
    """writeEstimatedQuantilesToFile (:103-119) -> bytes"""
    nq1, dim = sums.shape
    return "".join("%i " % d + "".join("%f " % (sums[i, d] / count) for i in range(nq1)) + "\n" for d in range(dim)).encode()


def _first_minimum(dist, last=False):
    """dist [D, n1, n2] -> indices of the winner of `if (distance < minimalDistance)` from FLT_MAX, outer loop first; None where none wins"""
    D = dist.shape[0]
    flat = dist.reshape(D, -1)
    valid = flat < FLT_MAX
    masked = np.where(valid, flat, np.inf)
    if last:
        idx = flat.shape[1] - 1 - np.argmin(masked[:, ::-1], axis=1)
    else:
        idx = np.argmin(masked, axis=1)
    return idx // dist.shape[2], idx % dist.shape[2], valid.any(axis=1)


def _power_function(fused, maxq, alpha, pw, scaled):
    a = np.asarray(alpha, F32).astype(F64)
    return (np.asarray(maxq, F32).astype(F64) * mad64(fused, a, pw, (1.0 - a) * np.asarray(scaled, F32).astype(F64))).astype(F32)


def _combine(fused, l, r, c0, c1, c2):
    """(1. - l - r) * c0 + l * c1 + r * c2 (:249, .hh:120): the first product is f64, the other two are f32 products that are widened"""
    l, r = np.asarray(l, F32), np.asarray(r, F32)
    w = 1.0 - l.astype(F64) - r.astype(F64)
    t = mad64(fused, w, np.asarray(c0, F32).astype(F64), (l * np.asarray(c1, F32)).astype(F32).astype(F64))
    return np.asarray(t + (r * np.asarray(c2, F32)).astype(F32).astype(F64)).astype(F32)


def equalize(x, tq, cfg, fused=False, variant=()):
    """one segment x [T, dim] -> dict(out, params [6, dim], quantiles (as first taken), cq_after)"""
    c = dict(DEFAULTS)
    c.update(cfg)
    x = np.ascontiguousarray(x, F32)
    T, D = x.shape
    nq = int(c["nq"])
    last, powf = "last_minimum" in variant, "powf" in variant
    ga, gg, gl = grids(c, "linear_grid" in variant)
    alpha, gamma = np.zeros(D, F32), np.ones(D, F32)
    lam, rho = np.zeros(D, F32), np.zeros(D, F32)
    cq = np.zeros((nq + 1, D), F32)
    cq_after = cq.copy()
    v = x
    with np.errstate(all="ignore"):
        if c["quantiles"]:
            cq = quantiles(x, nq)
            cq_after = cq.copy()
            of = F32(c["of"])
            maxq = std_max(of * tq[nq], of * cq[nq])                                  # :199
            ni = nq - 1
            scaled = (std_max(tq[1:nq], cq[1:nq]) / maxq).astype(F32)                 # :207  [ni, D]
            dist = np.zeros((D, len(ga), len(gg)), F32)
            for i in range(ni):
                pw = pow_f64(scaled[i][:, None], gg[None, :].astype(F64), powf)       # [D, ng]: pow does not depend on alpha
                tr = _power_function(fused, maxq[:, None, None], ga[None, :, None], pw[:, None, :], scaled[i][:, None, None])
                tmp = tr - tq[i + 1][:, None, None]
                dist = mad32(fused, tmp, tmp, dist)                                  # :210
            ia, ig, won = _first_minimum(dist, last)
            alpha = np.where(won, ga[ia], F32(0)).astype(F32)
            gamma = np.where(won, gg[ig], F32(1)).astype(F32)
            for i in range(ni):                                                       # :221-224
                cq_after[i + 1] = _power_function(fused, maxq, alpha, pow_f64(scaled[i], gamma, powf), scaled[i])
            if c["combination"]:
                lo, hi = np.maximum(np.arange(D) - 1, 0), np.minimum(np.arange(D) + 1, D - 1)
                L, R = gl[None, :, None], gl[None, None, :]
                dist = np.zeros((D, len(gl), len(gl)), F32)
                for i in range(1, nq):
                    tr = _combine(fused, L, R, cq_after[i][:, None, None], cq_after[i][lo][:, None, None], cq_after[i][hi][:, None, None])
                    tmp = tr - tq[i][:, None, None]
                    dist = mad32(fused, tmp, tmp, dist)
                pen = mad32(fused, L, L, (R * R).astype(F32))
                dist = mad32(fused, np.broadcast_to(pen, dist.shape), F32(c["beta"]), dist)          # :254
                il, ir, won = _first_minimum(dist, last)
                lam = np.where(won, gl[il], F32(0)).astype(F32)
                rho = np.where(won, gl[ir], F32(0)).astype(F32)
            sv = (x / maxq[None, :]).astype(F32)                                                     # .hh:108
            v = _power_function(fused, maxq[None, :], alpha[None, :], pow_f64(sv, gamma[None, :], powf), sv)
        if c["combination"]:                                                                         # .hh:114-123
            lo, hi = np.maximum(np.arange(D) - 1, 0), np.minimum(np.arange(D) + 1, D - 1)
            v = _combine(fused, lam[None, :], rho[None, :], v, v[:, lo], v[:, hi])
        mean, dev = np.zeros(D, F32), np.zeros(D, F32)
        out = v
        if c["mean"]:
            w = v[::-1] if "newest_first" in variant else v
            w64 = w.astype(F64)
            s = np.add.accumulate(w64, axis=0)[-1]                                                   # :295, one chain per channel
            mean = (s / F64(T)).astype(F32)                                                          # :302
            out = (v - mean[None, :]).astype(F32)                                                    # .hh:126
            if c["variance"]:
                if fused:
                    sq = np.zeros(D, F64)
                    for t in range(T):
                        sq = fma(w64[t], w64[t], sq)                                                 # :298
                else:
                    sq = np.add.accumulate(w64 * w64, axis=0)[-1]
                dev = np.sqrt((sq - s * s / F64(T)) / F64(T)).astype(F32)                            # :305
                out = (out / dev[None, :]).astype(F32)                                               # .hh:130
    return {"out": np.ascontiguousarray(out, F32), "params": np.stack([alpha, gamma, lam, rho, mean, dev]).astype(F32), "quantiles": cq,
            "cq_after": cq_after}


def estimate(segments, nq):
    """estimate = true: (sums f64 [(nq + 1), dim], count) over the non-empty segments in order (:172, :316)"""
    sums, count = None, 0
    for x in segments:
        if len(x) == 0:
            continue
        q = quantiles(np.asarray(x, F32), nq).astype(F64)
        sums = (np.zeros_like(q) if sums is None else sums) + q
        count += 1
    return sums, count
