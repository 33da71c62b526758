"""Plain restatement of the LDA scatter-matrix estimation (Signal::ScatterMatricesEstimator: accumulate, the accumulator file,
finalize) in numpy: neither the oracle nor the library is called.  The counterpart of tests/train_reference.py.

The accumulator is one flat f64 vector [dim (dim + 1) / 2 | n_classes * dim | n_classes]: the lower triangle of the square sum,
row-major, the vector sum of every class, the count of every class.  Frame x (f32) of class c with weight w (f32, None: 1) adds
    (f64)((x_i * x_j) * w)  to square[i][j], j <= i     both products are f32 operations, rounded in that order, then widened
    (f64)(x_i * w)          to sums[c][i]
    (f64)w                  to counts[c]
in frame order.  A frame whose class is >= n_classes (NO_LABEL among them) is skipped.

Exact inputs.  With features k/64 (integer |k| <= 512) and weights j/16 (f32, integer 0 <= j <= 32), (x_i x_j) w = k_i k_j j / 2^16
with |k_i k_j j| <= 2^23: exact in f32, and so is x w.  Every partial sum of up to 65 536 frames is an integer multiple of 2^-16
below 2^23: no f64 addition ever rounds, so every accumulator has ONE right value whatever the order of addition.  `exact_features`
/ `exact_weights` draw such inputs, `accumulate_int` forms the same sums in int64 (the proof that `accumulate` itself rounds
nowhere on them).
"""
import struct

import numpy as np

NO_LABEL = 0xFFFFFFFF
FEATURE_SCALE, WEIGHT_SCALE = 64, 16


def layout(dim, n_classes):
    """(length of the triangle = offset of the class sums, offset of the counts, total length)"""
    tri = dim * (dim + 1) // 2
    return tri, tri + n_classes * dim, tri + n_classes * dim + n_classes


def kept_frames(cls, n_classes):
    c = np.asarray(cls).astype(np.int64) & 0xFFFFFFFF
    t = np.nonzero(c < n_classes)[0]
    return t, c[t]


def tril(dim):
    """(i, j) of the triangle's entries in their order"""
    i, j = np.tril_indices(dim)
    return i, j


def accumulate(feats, cls, n_classes, weight=None, acc=None):
    """add the frames feats [T, dim] (f32) of classes cls [T] with weights weight [T] (f32; None: 1) into acc (a new zero vector if
    None), in frame order"""
    feats = np.asarray(feats, np.float32)
    T, dim = feats.shape
    tri, off_counts, size = layout(dim, n_classes)
    if acc is None:
        acc = np.zeros(size, np.float64)
    assert acc.dtype == np.float64 and acc.shape == (size,)
    i, j = tril(dim)
    sums = acc[tri:off_counts].reshape(n_classes, dim)
    w = None if weight is None else np.asarray(weight, np.float32)
    for t, c in zip(*kept_frames(cls, n_classes)):
        x = feats[t]
        p = x[i] * x[j]                       # f32
        assert p.dtype == np.float32
        if w is not None:
            p = p * w[t]                      # f32
            assert p.dtype == np.float32
        acc[:tri] += p.astype(np.float64)
        y = x if w is None else x * w[t]      # f32
        assert y.dtype == np.float32
        sums[c] += y.astype(np.float64)
        acc[off_counts + c] += np.float64(1.0 if w is None else w[t])
    return acc


def single_frame_products(x, weight=None):
    """the widened f32 products of ONE frame: (triangle, x * w)"""
    x = np.asarray(x, np.float32)
    i, j = tril(len(x))
    p = x[i] * x[j]
    y = x
    if weight is not None:
        p = p * np.float32(weight)
        y = x * np.float32(weight)
    assert p.dtype == np.float32 and y.dtype == np.float32
    return p.astype(np.float64), y.astype(np.float64)


def exact_features(T, dim, seed):
    """(f32 features [T, dim] = k / 64, the integers k) with |k| <= 512"""
    k = np.random.Generator(np.random.PCG64(seed)).integers(-512, 513, (T, dim))
    return (k / FEATURE_SCALE).astype(np.float32), k.astype(np.int64)


def exact_weights(T, seed):
    """(f32 weights [T] = j / 16, the integers j) with 0 <= j <= 32"""
    j = np.random.Generator(np.random.PCG64(seed)).integers(0, 33, T)
    return (j / WEIGHT_SCALE).astype(np.float32), j.astype(np.int64)


def accumulate_int(k_feats, cls, n_classes, j_weight=None):
    """the accumulator of exact inputs from their integers, summed in int64 and scaled once: features k_feats / 64, weights
    j_weight / 16 (None: 1).  Every scaled value is an integer below 2^53 over a power of two, so the division is exact."""
    kf = np.asarray(k_feats, np.int64)
    T, dim = kf.shape
    tri, off_counts, size = layout(dim, n_classes)
    t, c = kept_frames(cls, n_classes)
    kf = kf[t]
    j = np.full(len(t), WEIGHT_SCALE, np.int64) if j_weight is None else np.asarray(j_weight, np.int64)[t]
    acc = np.zeros(size, np.int64)
    ii, jj = tril(dim)
    acc[:tri] = np.einsum("t,ti,tj->ij", j, kf, kf)[ii, jj]
    np.add.at(acc[tri:off_counts].reshape(n_classes, dim), c, j[:, None] * kf)
    np.add.at(acc[off_counts:], c, j)
    assert np.abs(acc).max(initial=0) < 1 << 53
    scale = np.full(size, float(WEIGHT_SCALE))
    scale[:tri] *= FEATURE_SCALE * FEATURE_SCALE
    scale[tri:off_counts] *= FEATURE_SCALE
    return acc.astype(np.float64) / scale


def finalize(acc, dim, n_classes, normalize=False):
    """(between, within, total), each f64 [dim, dim], in the reference's order of f64 operations: total-mean part (s_i s_j) / N,
    class-mean part the sum over classes with n_c > 0, in class order, of (s_ci s_cj) / n_c; between = class-mean - total-mean,
    within = square - class-mean, total = square - total-mean; normalisation multiplies by 1 / N; the square sum's upper triangle
    mirrors its lower.  N == 0 raises ValueError."""
    acc = np.asarray(acc, np.float64)
    tri, off_counts, size = layout(dim, n_classes)
    assert acc.shape == (size,)
    sums = acc[tri:off_counts].reshape(n_classes, dim)
    counts = acc[off_counts:]
    s = np.zeros(dim, np.float64)
    N = np.float64(0.0)
    for c in range(n_classes):
        s += sums[c]
    for c in range(n_classes):
        N = N + counts[c]
    if N == 0:
        raise ValueError("No observation has been seen.")
    class_mean = np.zeros((dim, dim), np.float64)
    for c in range(n_classes):
        if counts[c] > 0:
            class_mean += np.outer(sums[c], sums[c]) / counts[c]
    i, j = tril(dim)
    square = np.zeros((dim, dim), np.float64)
    square[i, j] = acc[:tri]
    square[j, i] = acc[:tri]
    with np.errstate(all="ignore"):
        total_mean = np.outer(s, s) / N
        out = [class_mean - total_mean, square - class_mean, square - total_mean]
        if normalize:
            inv = np.float64(1.0) / N
            out = [m * inv for m in out]
    return tuple(out)


def file_bytes(acc, dim, n_classes):
    """the accumulator file: u32 dim, the triangle, u32 n_classes, the class sums, the counts; little endian"""
    acc = np.asarray(acc, "<f8")
    tri, off_counts, size = layout(dim, n_classes)
    assert acc.shape == (size,)
    return struct.pack("<I", dim) + acc[:tri].tobytes() + struct.pack("<I", n_classes) + acc[tri:].tobytes()


def matrix_bytes(m):
    """a binary Math::Matrix<T> file: u32 rows, u32 cols, u32 rows, then per row u32 cols + the values; little endian"""
    m = np.asarray(m)
    r, c = m.shape
    out = struct.pack("<III", r, c, r)
    for row in m:
        out += struct.pack("<I", c) + np.ascontiguousarray(row).astype(m.dtype.newbyteorder("<")).tobytes()
    return out


# ---- the cases both test files build

ALIGNMENTS = ("random", "runs", "alternating")


def alignment(T, n_classes, kind, seed, skip_every=10):
    """classes u32 [T]: "random", "runs" (long runs of one class, like an aligned utterance), "alternating" (two classes in turn: every
    frame ends a run).  Every skip_every-th frame (0: none) carries a class outside the model: n_classes, n_classes + 7, NO_LABEL in turn."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "random":
        c = rng.integers(0, n_classes, T)
    elif kind == "runs":
        c = np.repeat(rng.integers(0, n_classes, T // 11 + 1), 11)[:T]
    else:
        assert kind == "alternating"
        a, b = rng.integers(0, n_classes, 2)
        c = np.where(np.arange(T) % 2 == 0, a, b)
    c = c.astype(np.int64)
    if skip_every:
        t = np.arange(skip_every // 2, T, skip_every)
        c[t] = np.array([n_classes, n_classes + 7, NO_LABEL], np.int64)[np.arange(len(t)) % 3]
    return c.astype(np.uint32)
