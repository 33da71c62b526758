"""Histogram normalisation restated in numpy, every operation in f32 and in the reference's order: estimation
(Signal/Histogram.hh:46-48, Signal/LookupTable.hh:69-72, 178-202), CDF / percentile (Histogram.hh:56-80), getInverse and
proposeBucketSizeForInverse (LookupTable.hh:239-271), the interpolation of several training histograms
(Signal/HistogramNormalization.cc:36-60, 77-93), the file (LookupTable.hh:298-319, Histogram.hh:122-135) and apply (:68-75) with the
library's rule for a bucket outside its table: the nearest end bucket, counted.  tests/test_histogram.py holds it to
tests/golden/ref_histogram.npz bit for bit."""
import struct

import numpy as np

F = np.float32
SATURATION = 1 << 24          # the f32 value at which a + 1.0f == a
MAX_QUOTIENT = float(1 << 30)  # |x / bucket_size| from here on is refused by the estimator


class Table:
    """Signal::LookupTable<f32, f32>: bucketSize_, offset_, grow_, f_"""

    def __init__(self, bucket_size, offset=0, values=(), grow=True):
        self.bucket_size, self.offset, self.grow = F(bucket_size), int(offset), bool(grow)
        self.f = np.array(values, F)

    def copy(self):
        return Table(self.bucket_size, self.offset, self.f.copy(), self.grow)

    def index(self, b):
        """LookupTable::index: (f32)(b - offset) * bucketSize"""
        return F(F(int(b) - self.offset) * self.bucket_size)


def round_half_away(q):
    """round() of f32 values, as whole f64 numbers (exact: an f32 plus 0.5 needs no more than f64 holds)"""
    q = np.asarray(q, np.float64)
    return np.sign(q) * np.floor(np.abs(q) + 0.5)


def quotient(x, bucket_size):
    """x / bucket_size, the correctly rounded f32 division"""
    with np.errstate(all="ignore"):
        return np.asarray(x, F) / F(bucket_size)


def bucket_numbers(x, bucket_size):
    """k = (s32)round(x / bucket_size) as int64; the caller has checked the range"""
    return round_half_away(quotient(x, bucket_size)).astype(np.int64)


def acceptable(x, bucket_size):
    """the estimator's rule: every value finite and fewer than 2^30 buckets from zero"""
    with np.errstate(all="ignore"):
        return bool((np.abs(quotient(x, bucket_size)) < MAX_QUOTIENT).all())


def estimate(x, bucket_size, start=None):
    """frames [T, dim] -> one Table per dimension; start: tables (whole counts) to go on from.  Counts are kept exactly and cut at 2^24
    on the way out, like the library; the reference reaches the same value by adding 1.0f."""
    x = np.asarray(x, F)
    assert acceptable(x, bucket_size)
    k = bucket_numbers(x, bucket_size)
    out = []
    for d in range(x.shape[1]):
        lo, hi = int(k[:, d].min()), int(k[:, d].max())
        old = None if start is None or len(start[d].f) == 0 else start[d]
        if old is not None:
            lo, hi = min(lo, -old.offset), max(hi, len(old.f) - 1 - old.offset)
        c = np.bincount(k[:, d] - lo, minlength=hi - lo + 1).astype(np.int64)
        if old is not None:
            at = -old.offset - lo
            c[at:at + len(old.f)] += old.f.astype(np.int64)
        out.append(Table(bucket_size, -lo, np.minimum(c, SATURATION).astype(F)))
    return out


def file_bytes(tables):
    b = struct.pack("<I", len(tables))
    for t in tables:
        # Core::BinaryOutputStream writes true as 0xff
        b += struct.pack("<fiBI", t.bucket_size, t.offset, 0xff if t.grow else 0, len(t.f)) + t.f.astype("<f4").tobytes()
    return b


def parse_file(b):
    (n,), at, out = struct.unpack_from("<I", b, 0), 4, []
    for _ in range(n):
        bs, off, grow, size = struct.unpack_from("<fiBI", b, at)
        at += 13
        out.append(Table(bs, off, np.frombuffer(b, "<f4", size, at), grow != 0))
        at += 4 * size
    assert at == len(b)
    return out


def seq_sum(f):
    """std::accumulate(begin, end, (f32)0)"""
    return F(np.cumsum(np.asarray(f, F), dtype=F)[-1]) if len(f) else F(0)


def cdf(t):
    """Histogram::getCdf"""
    s = seq_sum(t.f)
    assert s != 0
    return Table(t.bucket_size, t.offset, np.cumsum(t.f, dtype=F) / s, t.grow)


def percentile(t, percent):
    """Histogram::percentile"""
    p, b = F(F(percent) * seq_sum(t.f)), 0
    while b < len(t.f) and p > 0:
        p = F(p - t.f[b])
        b += 1
    return t.index(b)


def insert(t, index, init=0.0):
    """LookupTable::insert: the position of `index`, the table grown where it may"""
    b = int(bucket_numbers(index, t.bucket_size)) + t.offset
    if len(t.f):
        if b < 0:
            if t.grow:
                t.f = np.concatenate([np.full(-b, init, F), t.f])
                t.offset -= b
            b = 0
        elif b >= len(t.f):
            if t.grow:
                t.f = np.concatenate([t.f, np.full(b - len(t.f) + 1, init, F)])
            b = len(t.f) - 1
    else:
        t.f = np.full(1, init, F)
        t.offset -= b
        b = 0
    return b


def propose_bucket_size(t):
    """LookupTable::proposeBucketSizeForInverse"""
    return F(F(t.f.max() - t.f.min()) / F(F(len(t.f)) * F(2)))


def inverse(t, bucket_size=0.0):
    """LookupTable::getInverse into a table of `bucket_size` (0: the proposal)"""
    inv = Table(propose_bucket_size(t) if bucket_size == 0 else bucket_size)
    assert inv.bucket_size > 0
    previous = 0
    for b in range(len(t.f)):
        current = insert(inv, t.f[b])
        v = t.index(b)
        inv.f[current] = v
        if previous < current:
            inv.f[previous + 1:current] = v
        elif current < previous:
            inv.f[current + 1:previous] = v
        previous = current
    return inv


def normalize_scales(scales):
    """HistogramNormalization::normalizeScales: the first scale is 1 - sum of the others, the sum taken in f64"""
    s = [F(v) for v in scales]
    return [F(np.float64(F(1.0)) - sum((np.float64(v) for v in s), np.float64(0.0)))] + s


def scales_well_defined(scales):
    return not any(s < 0 or s > 1 for s in scales)


def interpolate(train, all_scales):
    """the several-histograms form of setTrainingHistograms: train [n][dim] Tables -> [dim] Tables of the minimal bucket size"""
    minimal = min(t.bucket_size for tv in train for t in tv)
    out = [Table(minimal) for _ in train[0]]
    for tv, s in zip(train, all_scales):
        for d, t in enumerate(tv):
            surface = F(seq_sum(t.f) * t.bucket_size)
            assert surface != 0
            add = (t.f / surface) * F(s)
            for b in range(len(t.f)):
                at = insert(out[d], t.index(b))
                out[d].f[at] = F(out[d].f[at] + add[b])
    return out


def training_inverses(train, scales=(), probability_bucket_size=0.0):
    """train [n][dim] -> the inverse training CDFs [dim]"""
    if len(train) == 1:
        hist = train[0]
    else:
        s = normalize_scales(scales)
        assert scales_well_defined(s)
        hist = interpolate(train, s)
    return [inverse(cdf(t), F(probability_bucket_size)) for t in hist]


def lookup(t, x):
    """values of table t at x [..]: (values, clamped mask).  A bucket outside the table is the nearest end bucket; NaN: bucket 0, clamped."""
    with np.errstate(all="ignore"):
        r = round_half_away(quotient(x, t.bucket_size))
    nan = np.isnan(r)
    b = np.where(nan, -1.0, np.clip(r, -2147483648.0, 2147483520.0)).astype(np.int64) + t.offset
    b = np.where(nan, -1, b)
    clamped = (b < 0) | (b >= len(t.f))
    return t.f[np.clip(b, 0, len(t.f) - 1)], clamped


def apply(x, test_cdfs, inverses):
    """out = inverse[cdf[x]] per component for frames x [T, dim] of one key -> (out, clamped at the test CDF, clamped at the inverse)"""
    x = np.asarray(x, F)
    out, n_test, n_inv = np.empty_like(x), 0, 0
    for d in range(x.shape[1]):
        p, c1 = lookup(test_cdfs[d], x[:, d])
        y, c2 = lookup(inverses[d], p)
        out[:, d] = np.where(np.isnan(x[:, d]), x[:, d], y)
        n_test += int(c1.sum())
        n_inv += int(c2.sum())
    return out, n_test, n_inv


def apply_segments(x, frame_offsets, key_of_segment, keys, inverses):
    """the batched form: rows [frame_offsets[s], frame_offsets[s + 1]) of x with the test CDFs keys[key_of_segment[s]]"""
    out, n_test, n_inv = np.array(x, F), 0, 0
    for s, k in enumerate(key_of_segment):
        a, b = frame_offsets[s], frame_offsets[s + 1]
        if b > a:
            out[a:b], c1, c2 = apply(x[a:b], keys[k], inverses)
            n_test, n_inv = n_test + c1, n_inv + c2
    return out, n_test, n_inv
