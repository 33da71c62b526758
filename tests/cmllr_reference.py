"""Plain restatement of constrained MLLR (Mm::AffineFeatureTransformAccumulator: accumulate, finalize, combine, estimate, score, the
binary accumulator file) in Python / numpy f64: neither the oracle nor the library is called.

One key's accumulator is a flat f64 vector [beta | k: M x R | mean: R | cov: tri | G: M x tri] with R = F + 1 and tri the row-major UPPER
triangle (j <= k) of an R x R matrix; G is absent for a pooled model (one covariance).  A frame x (f32; xi = [1, x] widened) aligned to
a density with mean m and variance v (f32, widened) and weight w (f64; None: the unweighted overload) adds, in frame order,
    beta += 1 | w;  k[i][j] += m_i / v_i * xi_j [* w];  mean[j] += xi_j [* w];  cov[j][k] += xi_j * xi_k [* w];
    G[i][j][k] += xi_j * xi_k / v_i [* w]
evaluated from the left.  contract "fma": the last multiplication of a `+= a * b` and the addition are one fused multiply-add, what
the reference's -march=native build compiles (tests/golden/ref_cmllr.npz holds both builds' bits).  xi_j * xi_k is exact in f64 (two
24-bit significands), so fusing the unweighted cov changes nothing.

estimate and score follow the reference's text operation by operation with Math::Matrix / Math::Vector's loop orders; the inverse is
an LU with partial pivoting and a triangular solve per unit vector (the reference calls LAPACK), and no product is fused: these two are
what the fixture's bar measures.

DEFECTS names what a wrong implementation would do; tests show that each leaves the checks on at least one case."""
import math
import struct
from fractions import Fraction

import numpy as np

TAG = b"affine-feature-transform-accumulator"
NAIVE, MMI_PRIME, HLDA = 0, 1, 2
DEFECTS = ("reciprocal", "weight_first", "lower", "restart", "pooled_g", "half", "wrong_root", "segment_sorted")


# ---------------------------------------------------------------------------------------------------------------- fused multiply-add

def fma_exact(a, b, c):
    """a * b + c rounded once (scalars), through rationals"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c
    return float(r)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = a * 134217729.0, b * 134217729.0   # Veltkamp split, 2^27 + 1
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """a * b + c rounded once, for f64 arrays (Boldo and Melquiond: the low parts added with rounding to odd, then one rounding to
    nearest).  Valid away from overflow and underflow, where the tests' values are; test_cmllr.py checks it against fma_exact."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    v, err = _two_sum(tl, ul)
    bits = v.view(np.int64) if v.ndim else np.array(v).view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)
    if np.any(fix):
        v = np.where(fix, np.nextafter(v, np.where(err > 0, np.inf, -np.inf)), v)
    return th + v


def mad(a, b, c, fused):
    return fma(a, b, c) if fused else a * b + c


# ---------------------------------------------------------------------------------------------------------------- layout

def layout(F, M, pooled):
    """dict(R, tri, off_k, off_mean, off_cov, off_g, size) of one key"""
    R = F + 1
    tri = R * (R + 1) // 2
    off_mean = 1 + M * R
    off_cov = off_mean + R
    off_g = off_cov + tri
    return dict(R=R, tri=tri, off_k=1, off_mean=off_mean, off_cov=off_cov, off_g=off_g, size=off_g + (0 if pooled else M * tri))


def is_pooled(model):
    return model["variances"].shape[0] == 1


def frame_densities(model, emission, best, best_ld=0):
    """(mean index, covariance index) per frame, -1 where emission is -1; best as the scorers leave it (matrix or one per frame)"""
    emission = np.asarray(emission, np.int64)
    mi, ci = np.full(len(emission), -1, np.int64), np.full(len(emission), -1, np.int64)
    best = np.asarray(best)
    for t, e in enumerate(emission):
        if e == -1:
            continue
        assert 0 <= e < len(model["mix_offsets"]) - 1, (t, e)
        kk = int(best[t, e] if best_ld else best[t])
        lo, hi = int(model["mix_offsets"][e]), int(model["mix_offsets"][e + 1])
        assert kk < hi - lo, (t, e, kk)
        d = int(model["dens_index"][lo + kk])
        mi[t], ci[t] = int(model["dens_mean"][d]), int(model["dens_cov"][d])
    return mi, ci


def key_frames(frame_offsets, seg_key, key, defects=()):
    """the frames of `key` in ascending order: its segments in table order"""
    segs = [(int(frame_offsets[s]), int(frame_offsets[s + 1])) for s in range(len(seg_key)) if seg_key[s] == key]
    if "segment_sorted" in defects:
        segs.sort(key=lambda be: (be[1] - be[0], be[0]))   # defect: by length
    return [t for b, e in segs for t in range(b, e)]


# ---------------------------------------------------------------------------------------------------------------- accumulate

def accumulate(model, F, n_keys, feats, frame_offsets, seg_key, emission, best, best_ld=0, weight=None, acc=None, contract="off", defects=()):
    """add the segments' frames into the flat accumulator of all keys (a new zero vector if acc is None) and return it"""
    feats = np.asarray(feats, np.float32)
    M, pooled, fused = int(model["dim"]), is_pooled(model), contract == "fma"
    assert F >= M and feats.shape[1] >= F
    lay = layout(F, M, pooled and "pooled_g" not in defects)
    R, tri = lay["R"], lay["tri"]
    if acc is None:
        acc = np.zeros(n_keys * lay["size"], np.float64)
    assert acc.dtype == np.float64 and acc.shape == (n_keys * lay["size"],)
    start = acc.copy()
    if "restart" in defects:
        acc[:] = 0
    mi, ci = frame_densities(model, emission, best, best_ld)
    means, variances = model["means"].astype(np.float64), model["variances"].astype(np.float64)
    ju, ku = np.triu_indices(R)
    if "lower" in defects:
        ju, ku = np.tril_indices(R)   # defect: the cells in the order of the lower triangle
    w_all = None if weight is None else np.asarray(weight, np.float64)
    for key in range(n_keys):
        a = acc[key * lay["size"]:(key + 1) * lay["size"]]
        k = a[1:lay["off_mean"]].reshape(M, R)
        mean, cov = a[lay["off_mean"]:lay["off_cov"]], a[lay["off_cov"]:lay["off_g"]]
        G = a[lay["off_g"]:].reshape(M, tri) if lay["size"] > lay["off_g"] else None
        for t in key_frames(frame_offsets, seg_key, key, defects):
            if mi[t] < 0:
                continue
            xi = np.concatenate([[1.0], feats[t, :F].astype(np.float64)])
            m, v = means[mi[t]], variances[ci[t]]
            r = m * (1.0 / v) if "reciprocal" in defects else m / v
            P = xi[ju] * xi[ku]
            if w_all is None:
                a[0] += 1
                k[:] = mad(r[:, None], xi[None, :], k, fused)                    # :63 / :68
                mean += xi                                                        # :76
                cov += P                                                          # :78 (the product is exact)
                if G is not None:
                    G += P[None, :] * (1.0 / v)[:, None] if "reciprocal" in defects else P[None, :] / v[:, None]   # :70
            else:
                w = w_all[t]
                a[0] += w
                k[:] = mad(r[:, None] * xi[None, :], w, k, fused)                 # :104 / :109
                mean[:] = mad(xi, w, mean, fused)                                 # :117
                cov[:] = mad(P, w, cov, fused)                                    # :119
                if G is not None:
                    if "weight_first" in defects:
                        G += (P[None, :] * w) / v[:, None]
                    elif "reciprocal" in defects:
                        G[:] = mad(P[None, :] * (1.0 / v)[:, None], w, G, fused)
                    else:
                        G[:] = mad(P[None, :] / v[:, None], w, G, fused)          # :111
    if "restart" in defects:
        acc += start
    return acc


def members(acc, F, M, pooled, key=0):
    """dict(beta, k, mean, cov [R, R] upper, G [M, R, R] upper or None) of one key of a flat accumulator"""
    lay = layout(F, M, pooled)
    R = lay["R"]
    a = np.asarray(acc, np.float64).reshape(-1)[key * lay["size"]:(key + 1) * lay["size"]]
    iu = np.triu_indices(R)
    cov = np.zeros((R, R))
    cov[iu] = a[lay["off_cov"]:lay["off_g"]]
    G = None
    if not pooled:
        G = np.zeros((M, R, R))
        for i in range(M):
            G[i][iu] = a[lay["off_g"] + i * lay["tri"]:lay["off_g"] + (i + 1) * lay["tri"]]
    return dict(beta=float(a[0]), k=a[1:lay["off_mean"]].reshape(M, R).copy(), mean=a[lay["off_mean"]:lay["off_cov"]].copy(), cov=cov, G=G)


def flat(mem, pooled):
    """members -> one key's flat accumulator"""
    R = len(mem["mean"])
    iu = np.triu_indices(R)
    parts = [[mem["beta"]], mem["k"].ravel(), mem["mean"], mem["cov"][iu]]
    if not pooled:
        parts += [g[iu] for g in mem["G"]]
    return np.concatenate([np.asarray(p, np.float64) for p in parts])


# ---------------------------------------------------------------------------------------------------------------- files

def file_bytes(acc, F, M, pooled_variance=None, key=0):
    """the reference's binary accumulator behind Core::IoRef's tag, as the accumulating pass leaves it (lower triangles zero; a pooled
    model's G matrices 0 x 0)"""
    pooled = pooled_variance is not None
    mem = members(acc, F, M, pooled, key)
    R = F + 1

    def vector(v):
        return struct.pack("<I", len(v)) + np.asarray(v, "<f8").tobytes()

    def matrix(m):
        if m is None:
            return struct.pack("<III", 0, 0, 0)
        return struct.pack("<III", R, R, R) + b"".join(vector(row) for row in m)

    out = struct.pack("<I", len(TAG)) + TAG + struct.pack("<IId", F, M, mem["beta"])
    out += struct.pack("<I", M) + b"".join(matrix(None if pooled else mem["G"][i]) for i in range(M))
    out += struct.pack("<I", M) + b"".join(vector(mem["k"][i]) for i in range(M))
    out += vector(mem["mean"]) + matrix(mem["cov"])
    var = np.zeros(0, "<f4") if not pooled else np.asarray(pooled_variance, "<f4")
    out += struct.pack("<I", len(var)) + var.tobytes() + (b"\xff" if pooled else b"\x00")
    return out


def transform_file_bytes(transform):
    """the XML file of `os << transform` on a Core::XmlOutputStream (Math/Matrix.hh:641-647): declaration, element, print_raw's rows in
    std::scientific with six digits and a space behind every value"""
    t = np.asarray(transform, np.float32)
    rows = "".join("".join("%e " % float(v) for v in row) + "\n" for row in t)
    return ('<?xml version="1.0" encoding="ISO-8859-1"?>\n<matrix-f32 nRows="%d" nColumns="%d">\n' % t.shape + rows + "</matrix-f32>\n").encode()


def combine(acc, other, weight):
    """combine (:345-365): every member += other * weight, the product stored first"""
    return np.asarray(acc, np.float64) + np.asarray(other, np.float64) * np.float64(weight)


# ---------------------------------------------------------------------------------------------------------------- estimate, score

def finalize(acc, F, M, pooled_variance=None, key=0):
    """members with G and cov mirrored; a pooled model's G from cov (:124-133)"""
    pooled = pooled_variance is not None
    mem = members(acc, F, M, pooled, key)
    R = F + 1
    if pooled:
        v = np.asarray(pooled_variance, np.float32).astype(np.float64)
        mem["G"] = np.stack([np.triu(mem["cov"]) / v[i] for i in range(M)])
    il = np.tril_indices(R, -1)
    for g in list(mem["G"]) + [mem["cov"]]:
        g[il] = g.T[il]
    return mem


def _dot_rows(m, v):
    """Matrix * Vector: every row's sum starts at 0 and adds m[n][i] * v[i] with i ascending"""
    s = np.zeros(m.shape[0])
    for i in range(m.shape[1]):
        s = s + m[:, i] * v[i]
    return s


def _mat_mat(l, r):
    out = np.zeros((l.shape[0], r.shape[1]))
    for k in range(l.shape[1]):
        out = out + l[:, k][:, None] * r[k, :][None, :]
    return out


def lu_factor(a):
    a = np.array(a, np.float64)
    n = len(a)
    piv = np.zeros(n, np.int64)
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))   # the first largest
        piv[c] = p
        if not (abs(a[p, c]) > 0 and math.isfinite(a[p, c])):
            raise ZeroDivisionError("singular matrix")
        if p != c:
            a[[c, p]] = a[[p, c]]
        a[c + 1:, c] = a[c + 1:, c] / a[c, c]
        a[c + 1:, c + 1:] -= a[c + 1:, c][:, None] * a[c, c + 1:][None, :]
    return a, piv


def invert(m):
    lu, piv = lu_factor(m)
    n = len(lu)
    x = np.eye(n)
    for i in range(n):
        if piv[i] != i:
            x[[i, piv[i]]] = x[[piv[i], i]]
    for i in range(1, n):
        for j in range(i):
            x[i] = x[i] - lu[i, j] * x[j]
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            x[i] = x[i] - lu[i, j] * x[j]
        x[i] = x[i] / lu[i, i]
    return x


def log_determinant(m):
    lu, _ = lu_factor(m)
    d = 0.0
    for i in range(len(lu)):
        d += math.log(abs(lu[i, i]))
    return d


def global_covariance(mem):
    a = mem["mean"] / mem["beta"]
    return (mem["cov"] / mem["beta"] - a[:, None] * a[None, :])[1:, 1:]


def estimate(acc, F, M, iterations, min_obs_weight, criterion, initial=None, pooled_variance=None, key=0, defects=(), inverse=invert):
    """dict(transform f32 [M, R], transform64, iterations [it, M, R], estimated, choices [(l1 > l2) per row update])"""
    assert criterion in (NAIVE, MMI_PRIME)
    R = F + 1
    T = np.zeros((M, R))
    if initial is None:
        T[np.arange(M), np.arange(M) + 1] = 1.0
    else:
        ini = np.asarray(initial, np.float32).astype(np.float64)
        assert ini.shape in ((M, F), (M, R))
        T[:, R - ini.shape[1]:] = ini
    mem = finalize(acc, F, M, pooled_variance, key)
    beta = mem["beta"]
    its, choices = [], []

    def give(est):
        return dict(transform=T.astype(np.float32), transform64=T.copy(), iterations=np.array(its).reshape(len(its), M, R), estimated=est, choices=choices)

    if criterion != NAIVE and beta < min_obs_weight:
        return give(False)
    g_inv = [inverse(g) for g in mem["G"]]
    if criterion == NAIVE:
        for i in range(M):
            T[i] = _dot_rows(g_inv[i], mem["k"][i])
        return give(True)
    gc = global_covariance(mem)
    hct = _mat_mat(T[:, 1:], gc)
    tc = _mat_mat(T[:, 1:], hct.T)
    half = 0.5 if "half" in defects else 1 // 2
    for _ in range(iterations):
        for row in range(M):
            lt = T[:, 1:].copy()
            pinv = inverse(tc if M < F else lt)
            col = pinv[:, row]
            cof = np.zeros(R)
            cof[1:] = _dot_rows(hct.T, col) if M < F else col
            gi, kr = g_inv[row], mem["k"][row]
            e1 = e2 = 0.0
            for j in range(R):
                cj = float(cof[j])
                grow = gi[j]
                for k in range(R):
                    g = float(grow[k])
                    e1 += cj * g * float(cof[k])
                    e2 += cj * g * float(kr[k])
            root = math.sqrt(e2 * e2 + 4 * e1 * beta)
            a1 = (-e2 + root) / (2 * e1)
            a2 = (-e2 - root) / (2 * e1)
            l1 = beta * math.log(abs(a1 * e1 + e2)) - half * a1 * a1 * e1
            l2 = beta * math.log(abs(a2 * e1 + e2)) - half * a2 * a2 * e1
            first = l1 > l2
            choices.append((first, l1, l2))
            if "wrong_root" in defects:
                first = not first
            alpha = a1 if first else a2
            new_row = _dot_rows(gi, cof * alpha + kr)
            T[row] = new_row
            nrl = new_row[1:]
            lt[row] = nrl
            nrhc = _dot_rows(gc, nrl)
            hct[row] = nrhc
            tc[row] = _dot_rows(hct, nrl)
            tc[:, row] = _dot_rows(lt, nrhc)
        its.append(T.copy())
    return give(True)


def score(acc, F, M, transform, criterion, pooled_variance=None, key=0):
    assert criterion in (NAIVE, MMI_PRIME)
    mem = finalize(acc, F, M, pooled_variance, key)
    A = np.asarray(transform, np.float32).astype(np.float64)
    jacobian = 0.0
    if criterion == MMI_PRIME:
        lt = A[:, 1:]
        jacobian = log_determinant(_mat_mat(_mat_mat(lt, global_covariance(mem)), lt.T)) / 2
    distance = 0.0
    for i in range(M):
        gr = _dot_rows(mem["G"][i], A[i])
        distance += float(_dot_rows(gr[None, :], A[i])[0]) / 2 - float(_dot_rows(mem["k"][i][None, :], A[i])[0])
    return jacobian - distance / mem["beta"]


def apply(transforms, has_transform, feats, frame_offsets, seg_key, M, F, contract="off"):
    """y = A_key [1, x] per frame in f32: the chain starts at 0, adds A[r][0] * 1, then A[r][k] * x[k - 1] with k ascending; a key without a
    transform passes x[:M] through.  Returns (y [T, M] with rows outside the segments zero, identity segments)"""
    feats = np.asarray(feats, np.float32)
    out = np.zeros((feats.shape[0], M), np.float32)
    n_identity = 0
    for s, key in enumerate(seg_key):
        b, e = int(frame_offsets[s]), int(frame_offsets[s + 1])
        if not has_transform[key]:
            n_identity += 1
            out[b:e] = feats[b:e, :M]
            continue
        A = np.asarray(transforms[key], np.float32)
        xi = np.concatenate([np.ones((e - b, 1), np.float32), feats[b:e, :F]], axis=1)
        y = np.zeros((e - b, M), np.float32)
        for k in range(F + 1):
            if contract == "fma":
                y = fma32(A[None, :, k], xi[:, k][:, None], y)
            else:
                y = (A[None, :, k] * xi[:, k][:, None]).astype(np.float32) + y
        out[b:e] = y
    return out, n_identity


def fma32(a, b, c):
    """the f32 fused multiply-add of f32 arrays: a * b is exact in f64, its sum with c is formed exactly as a pair (two_sum), rounded to
    odd in f64 and then once to f32 (53 >= 2 * 24 + 2 bits: the double rounding through an odd-rounded f64 is the single one)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    v, err = _two_sum(c, a * b)
    fix = (err != 0) & ((v.view(np.int64) & 1) == 0)
    v = np.where(fix, np.nextafter(v, np.where(err > 0, np.inf, -np.inf)), v)
    return v.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the fixture's cases

def fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cmllr.npz"))


def case_names(z):
    return sorted({k[:-len("/feats")] for k in z.files if k.endswith("/feats")})


def load_case(z, name):
    """dict(model, F, M, pooled, pooled_variance, n_keys, feats, frame_offsets, seg_key, emission, best, weight, cut, iterations, initial)"""
    model = {k: z["%s/model/%s" % (name, k)] for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov", "means", "variances", "log_weight")}
    model["dim"] = int(model["means"].shape[1])
    c = dict(model=model, M=model["dim"], pooled=is_pooled(model), n_keys=3, cut=int(z[name + "/cut"]), iterations=int(z[name + "/iterations"]))
    for k in ("feats", "frame_offsets", "seg_key", "emission", "best"):
        c[k] = z["%s/%s" % (name, k)]
    c["F"] = int(c["feats"].shape[1])
    c["weight"] = z[name + "/weight"] if name + "/weight" in z.files else None
    c["initial"] = z[name + "/initial"] if name + "/initial" in z.files else None
    c["pooled_variance"] = model["variances"][0] if c["pooled"] else None
    return c


def recorded(z, name, build, what):
    """(kind, value) of a recorded result: ("bits", array) or ("sha256", digest); the fma build's is off's where the generator found them equal"""
    if build == "fma" and "%s/fma/%s_same_as_off" % (name, what) in z.files:
        build = "off"
    for suffix, kind in (("", "bits"), ("_sha256", "sha256")):
        key = "%s/%s/%s%s" % (name, build, what, suffix)
        if key in z.files:
            return kind, z[key]
    raise KeyError((name, build, what))


def matches(rec, value):
    """whether `value` has the recorded bits"""
    import hashlib
    kind, want = rec
    value = np.ascontiguousarray(value)
    if kind == "sha256":
        return hashlib.sha256(value.tobytes()).digest() == want.tobytes()
    return value.dtype == want.dtype and value.shape == want.shape and np.array_equal(value.view(np.uint8), want.view(np.uint8))


def accumulate_case(c, contract, calls=1, defects=(), upto=None):
    """the restatement on a case: in one call, or cut into two at c["cut"] (a frame inside a segment); upto: only the frames before it"""
    off, keys = np.asarray(c["frame_offsets"]), np.asarray(c["seg_key"])

    def part(lo, hi, acc):
        o = np.clip(off, lo, hi)
        return accumulate(c["model"], c["F"], c["n_keys"], c["feats"], o, keys, c["emission"], c["best"], 0, c["weight"], acc, contract, defects)

    end = int(off[-1]) if upto is None else upto
    if calls == 1:
        return part(0, end, None)
    return part(c["cut"], end, part(0, min(c["cut"], end), None))
