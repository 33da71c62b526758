"""GPU parity: amx_histogram_accumulate_dev (hist_range_kernel, hist_count_kernel) and amx_histnorm_apply_dev (histnorm_apply_kernel)
through the C ABI against the plain restatement of tests/histogram_reference.py and the reference's own results in
tests/golden/ref_histogram.npz.  Every comparison is equality of bits: a finished histogram depends only on the multiset of bucket
numbers, and the two look-ups of apply are pure f32.

Shapes.  Both kernels run 256 lanes over the elements of a chunk of frames, consecutive lanes on consecutive components: dim 1, 3, 40
and 65 (one more than a wave) give steps of 256, 85 + 1, 6 + 16 and 3 + 61 elements; T = 1, 63, 64, 65, 1000 are one frame, the wave
edges and several workgroups.  Which count path a dimension takes is read from amx_histogram_describe, not assumed.
"""
import os

import numpy as np
import pytest

from tests import histogram_reference as hr
from tests.test_histogram import GOLDEN, NORMALIZERS, bits, golden_table, same_table

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 40, 65)
FRAMES = (1, 63, 64, 65, 1000)
PAD_LEFT, PAD_RIGHT = 3, 2      # the features are columns [3, 3 + dim) of a [T, dim + 5] matrix whose other columns hold NaN


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def padded(x, fill=np.nan):
    import torch
    wide = np.full((len(x), PAD_LEFT + x.shape[1] + PAD_RIGHT), fill, np.float32)
    wide[:, PAD_LEFT:PAD_LEFT + x.shape[1]] = x
    wd = torch.from_numpy(wide).cuda()
    return wd, wd[:, PAD_LEFT:PAD_LEFT + x.shape[1]], wide.shape[1]


def estimator(ctx, dim, bucket_size):
    import rasr_amd
    ctx.use_torch_stream()
    return rasr_amd.HistogramEstimator(ctx, dim, bucket_size)


def add(e, x):
    """one device call with the frames x [T, dim]; returns the (dimension, call) pairs that went (LDS, global) in it"""
    before = e.describe()
    wd, view, ld = padded(np.ascontiguousarray(x, np.float32))
    e.accumulate_dev(view, ld, len(x))
    after = e.describe()
    assert after["n_device_calls"] == before["n_device_calls"] + (1 if len(x) else 0)
    return after["n_lds"] - before["n_lds"], after["n_global"] - before["n_global"]


def expected_paths(tables, info):
    """the rule amx_histogram_describe documents: windows of at most lds_max_buckets, dimensions in order, while lds_capacity lasts"""
    used = lds = 0
    for t in tables:
        if len(t.f) <= info["lds_max_buckets"] and used + len(t.f) <= info["lds_capacity"]:
            used, lds = used + len(t.f), lds + 1
    return lds, len(tables) - lds


def equal(e, tables):
    return all(same_table(e.table(d), t) for d, t in enumerate(tables))


def gaussian(T, dim, seed, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal((T, dim)) * scale + rng.standard_normal(dim)).astype(np.float32)


@pytest.mark.parametrize("dim", DIMS)
def test_accumulation_every_shape_and_both_paths(ctx, dim):
    for T in FRAMES:
        x = gaussian(T, dim, 100 * dim + T)
        mixed = x.copy()
        mixed[:, ::2] *= 64.0                                 # even dimensions: windows 64 times as wide
        for what, data, bs in (("lds", x, 0.25), ("global", x, 0.0005), ("mixed", mixed, 0.125)):
            e = estimator(ctx, dim, bs)
            want = hr.estimate(data, bs)
            paths = add(e, data)
            assert paths == expected_paths(want, e.describe()), (what, T)
            if what == "lds":
                assert paths == (dim, 0), T
            elif T >= 63:
                assert paths == (0, dim) if what == "global" else paths == (dim // 2, dim - dim // 2), (what, T, paths)
            assert equal(e, want) and e.describe()["frames"] == T, (what, T)
            e.close()


def test_the_threshold_between_the_two_count_paths(ctx):
    info = estimator(ctx, 1, 1.0).describe()
    n, cap = info["lds_max_buckets"], info["lds_capacity"]
    assert 1 < n <= cap
    for size, want_paths in ((n, (1, 0)), (n + 1, (0, 1))):
        x = np.repeat(np.arange(size, dtype=np.float32), 2)[:, None]
        e = estimator(ctx, 1, 1.0)
        assert add(e, x) == want_paths, size
        t = e.table(0)
        assert t[1] == 0 and bits(t[2], np.full(size, 2.0, np.float32))
    # dimensions of a full window each: those that fit the table together count in LDS, the next one does not
    dim = cap // n + 1
    x = np.tile(np.arange(n, dtype=np.float32)[:, None], (1, dim))
    e = estimator(ctx, dim, 1.0)
    assert add(e, x) == (cap // n, 1)
    assert equal(e, hr.estimate(x, 1.0))


def one_ulp_around_the_ties(bucket_size):
    """values whose f32 quotient by bucket_size lies one ulp below / above k + 0.5, confirmed by the restatement's own quotient"""
    bs, below, above, k_below, k_above = np.float32(bucket_size), [], [], [], []
    for k in list(range(1000, 9000, 13)) + list(range(-9000, -1000, 17)):
        tie = np.float32(k + 0.5)
        x0 = np.float32(np.float64(tie) * np.float64(bs))
        for step in range(-3, 4):
            x = x0
            for _ in range(abs(step)):
                x = np.nextafter(x, np.float32(np.inf if step > 0 else -np.inf), dtype=np.float32)
            q = hr.quotient(x, bs)
            if q == np.nextafter(tie, np.float32(-np.inf), dtype=np.float32):
                below.append(x)
                k_below.append(k)
            elif q == np.nextafter(tie, np.float32(np.inf), dtype=np.float32):
                above.append(x)
                k_above.append(k + 1)
    return np.array(below, np.float32), np.array(above, np.float32), np.array(k_below), np.array(k_above)


def test_accumulation_rounds_like_the_reference(ctx):
    # exact ties of both signs and -0.0 at a power-of-two bucket size: round() is half away from zero
    k = np.arange(-20, 21)
    ties = np.concatenate([k * 0.25 + 0.125, k * 0.25 - 0.125, [-0.0, 0.0]]).astype(np.float32)
    x = np.stack([ties, ties[::-1]], 1)
    e = estimator(ctx, 2, 0.25)
    add(e, x)
    want = hr.estimate(x, 0.25)
    assert equal(e, want)
    t = hr.Table(*e.table(0))
    assert t.f[t.offset + 1] == 2 and t.f[t.offset - 1] == 2 and t.f[t.offset] == 2   # +-0.125 go to k = +-1; only the two zeros stay at 0
    # one ulp either side of a tie at a bucket size that is no power of two: the quotient must be the correctly rounded one
    bs = np.float32(0.0002)
    below, above, k_below, k_above = one_ulp_around_the_ties(bs)
    assert len(below) > 200 and len(above) > 200 and (below < 0).any() and (below > 0).any() and (above < 0).any() and (above > 0).any()
    # a quotient just below k + 0.5 belongs to bucket k, one just above to k + 1, for either sign of k
    assert np.array_equal(hr.bucket_numbers(below, bs), k_below) and np.array_equal(hr.bucket_numbers(above, bs), k_above)
    n = min(len(below), len(above)) // 2 * 2
    x = np.stack([below[:n], above[:n]], 1)
    e = estimator(ctx, 2, bs)
    paths = add(e, x)
    want = hr.estimate(x, bs)
    assert paths == (0, 2) and equal(e, want)


def test_a_call_that_grows_the_window_equals_one_call(ctx, golden):
    dim = 5
    x1 = gaussian(300, dim, 1)
    x2 = np.concatenate([gaussian(200, dim, 2), np.full((1, dim), -9.0, np.float32), np.full((1, dim), 11.0, np.float32)])
    x3 = gaussian(50, dim, 3, 0.1)                            # inside the window: no growth
    for bs in (0.25, 0.002):
        e = estimator(ctx, dim, bs)
        add(e, x1)
        assert equal(e, hr.estimate(x1, bs))
        add(e, x2)
        add(e, x3)
        whole = hr.estimate(np.concatenate([x1, x2, x3]), bs)
        assert equal(e, whole) and e.describe()["frames"] == 552
        assert whole[0].offset > hr.estimate(x1, bs)[0].offset and len(whole[0].f) > len(hr.estimate(x1, bs)[0].f)
        once = estimator(ctx, dim, bs)
        add(once, np.concatenate([x1, x2, x3]))
        assert equal(once, whole)
        # host calls and device calls mix: the handle carries its counts to where the next call runs
        e.accumulate(x2)
        add(e, x1)
        assert equal(e, hr.estimate(np.concatenate([x1, x2, x3, x2, x1]), bs))
    # the fixture's frames through the device equal the reference's tables and file
    for name in ("ties2", "ties5", "gauss_a", "speaker"):
        x = golden["h/%s/feats" % name]
        e = estimator(ctx, x.shape[1], float(golden["h/%s/bucket_size" % name]))
        add(e, x[:len(x) // 3])
        add(e, x[len(x) // 3:])
        for d in range(x.shape[1]):
            assert same_table(e.table(d), golden_table(golden, "off/h/%s/table/%d" % (name, d))), (name, d)


def test_values_the_cast_is_undefined_for_are_refused_and_add_nothing(ctx):
    import rasr_amd
    dim, bs = 3, 0.5
    x = gaussian(200, dim, 5)
    e = estimator(ctx, dim, bs)
    add(e, x)
    want = hr.estimate(x, bs)
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 29, -2.0 ** 29):
        y = gaussian(130, dim, 6)
        y[77, 1] = bad
        assert not hr.acceptable(y, bs)
        wd, view, ld = padded(y)
        with pytest.raises(rasr_amd.AmxError, match="nothing was added") as err:
            e.accumulate_dev(view, ld, len(y))
        assert err.value.status == rasr_amd._lib.AMX_ERR_INVALID
        assert equal(e, want) and e.describe()["frames"] == 200, bad
    y = gaussian(130, dim, 6)
    y[77, 1] = np.float32(2.0 ** 29 - 64)                     # the largest quotient below 2^30 at this bucket size is taken
    add(e, y)
    assert equal(e, hr.estimate(y, bs, start=want))
    fresh = estimator(ctx, dim, bs)                            # an empty handle stays empty
    wd, view, ld = padded(np.full((4, dim), np.nan, np.float32))
    with pytest.raises(rasr_amd.AmxError):
        fresh.accumulate_dev(view, ld, 4)
    assert fresh.table(0)[2].size == 0 and fresh.describe()["frames"] == 0


def test_a_count_stops_at_two_to_the_24_on_the_device(ctx, tmp_path):
    import rasr_amd
    start = [hr.Table(0.25, 1, [5.0, 16777215.0, 7.0])]
    path = str(tmp_path / "full.hist")
    with open(path, "wb") as f:
        f.write(hr.file_bytes(start))
    ctx.use_torch_stream()
    h = rasr_amd.HistogramEstimator.read(path, ctx)
    add(h, np.zeros((3, 1), np.float32))
    assert same_table(h.table(0), hr.Table(0.25, 1, [5.0, 16777216.0, 7.0]))
    add(h, np.array([[0.25], [-0.5]], np.float32))
    assert same_table(h.table(0), hr.Table(0.25, 2, [1.0, 5.0, 16777216.0, 8.0]))


class Normalizer:
    """a training histogram and n_keys speakers of `dim` components: the library's handle and the restatement's tables"""

    def __init__(self, ctx, dim, n_keys, seed, bucket_size=0.05, train_frames=400, key_frames=300):
        import rasr_amd
        ctx.use_torch_stream()
        self.dim = dim
        self.frames = [gaussian(key_frames, dim, seed + 10 * k, 0.8 + 0.2 * k) for k in range(n_keys)]
        train_x = gaussian(train_frames, dim, seed + 7)
        train = rasr_amd.HistogramEstimator(None, dim, bucket_size)
        train.accumulate(train_x)
        self.norm = rasr_amd.HistogramNormalization(ctx, [train])
        self.inverses = hr.training_inverses([hr.estimate(train_x, bucket_size)])
        self.keys = []
        for k, x in enumerate(self.frames):
            h = rasr_amd.HistogramEstimator(None, dim, bucket_size)
            h.accumulate(x)
            assert self.norm.add_key(h) == k
            self.keys.append([hr.cdf(t) for t in hr.estimate(x, bucket_size)])

    def check(self, x, offsets, seg_keys, what):
        """out of place into a NaN-filled matrix with its own leading dimension, then in place: both equal the restatement"""
        import torch
        want, n_test, n_inv = hr.apply_segments(x, offsets, seg_keys, self.keys, self.inverses)
        wd, view, ld = padded(x)
        out = torch.full((len(x), self.dim + 7), -7.0, dtype=torch.float32, device="cuda")
        clamped = self.norm.apply_dev(offsets, seg_keys, view, ld, out, self.dim + 7)
        got = out.cpu().numpy()
        inside = slice(offsets[0], offsets[-1])               # rows outside keep what the output buffer held (checked below)
        assert bits(got[inside, :self.dim], want[inside]), what
        assert (got[:, self.dim:] == -7.0).all(), what
        assert clamped == (n_test, n_inv), what
        before = wd.cpu().numpy()
        assert self.norm.apply_dev(offsets, seg_keys, view, ld, view, ld) == clamped, what
        after = wd.cpu().numpy()
        assert bits(after[:, PAD_LEFT:PAD_LEFT + self.dim], want), what
        pad = np.ones(after.shape[1], bool)
        pad[PAD_LEFT:PAD_LEFT + self.dim] = False
        assert bits(after[:, pad], before[:, pad]), what
        if offsets[0] > 0 or offsets[-1] < len(x):            # rows outside [offsets[0], offsets[-1]) are not touched
            outside = np.ones(len(x), bool)
            outside[offsets[0]:offsets[-1]] = False
            assert (got[outside] == -7.0).all() and bits(after[outside], before[outside]), what
        return clamped


def segmentations(T):
    """(frame offsets, n_seg) forms: one segment; two; five with an empty segment and segments of one frame where T allows"""
    out = [[0, T], [0, T // 2, T]]
    if T >= 4:
        out.append([0, 1, 1, 2, T - 1, T])
    else:
        out.append([0, 0, T, T, T, T])
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_application_every_shape(ctx, dim):
    one, three = Normalizer(ctx, dim, 1, 50 * dim), Normalizer(ctx, dim, 3, 50 * dim + 1)
    rng = np.random.Generator(np.random.PCG64(dim))
    for T in FRAMES:
        for nz in (one, three):
            n_keys = len(nz.keys)
            for offsets in segmentations(T):
                n_seg = len(offsets) - 1
                seg_keys = [(s * 2 + 1) % n_keys for s in range(n_seg)]
                # every segment's frames come from what its key has seen: inside both tables
                x = np.zeros((T, dim), np.float32)
                for s in range(n_seg):
                    n = offsets[s + 1] - offsets[s]
                    x[offsets[s]:offsets[s + 1]] = nz.frames[seg_keys[s]][rng.integers(0, len(nz.frames[seg_keys[s]]), n)]
                nz.check(x, offsets, seg_keys, (T, n_keys, offsets))
    # a range of frames in the middle of the buffer
    x = three.frames[1][:200].copy()
    three.check(x, [40, 41, 100, 100, 163], [1, 1, 1, 1], "middle")


def test_application_outside_the_tables_clamps_and_counts(ctx):
    dim = 3
    # the second speaker has many frames and the training histogram few: the speaker's CDF starts below the inverse table's first bucket
    nz = Normalizer(ctx, dim, 2, 900, train_frames=20, key_frames=2000)
    assert hr.lookup(nz.inverses[0], nz.keys[1][0].f[:1])[1][0]
    x = nz.frames[1][:400].copy()
    assert nz.check(x, [0, 400], [1], "below the inverse")[1] > 0
    x = gaussian(500, dim, 901, 6.0)                          # far beyond both ends of every test table
    x[5, 0], x[6, 1], x[7, 2], x[8, 0] = 1e30, -1e30, np.inf, -np.inf
    c_test, c_inv = nz.check(x, [0, 250, 500], [0, 1], "beyond the ends")
    assert c_test > 100
    x[100, 1] = x[300, 2] = np.nan
    want, n_test, n_inv = hr.apply_segments(x, [0, 250, 500], [0, 1], nz.keys, nz.inverses)
    assert np.isnan(want[100, 1]) and np.isnan(want[300, 2]) and np.isnan(want).sum() == 2
    assert nz.check(x, [0, 250, 500], [0, 1], "NaN") == (n_test, n_inv)


def test_application_equals_the_reference(ctx, golden):
    import rasr_amd
    import torch
    ctx.use_torch_stream()

    def handle(name):
        x = golden["h/%s/feats" % name]
        e = rasr_amd.HistogramEstimator(ctx, x.shape[1], float(golden["h/%s/bucket_size" % name]))
        add(e, x)
        return e
    for name in NORMALIZERS:
        n = rasr_amd.HistogramNormalization(ctx, [handle(t) for t in golden["n/%s/train" % name]], float(golden["n/%s/probability_bucket_size" % name]))
        if len(golden["n/%s/train" % name]) > 1:
            n.set_scales(golden["n/%s/scales" % name])
        for d in range(n.dim):
            assert same_table(n.inverse_cdf(d), golden_table(golden, "off/n/%s/inverse/%d" % (name, d))), (name, d)
        tests = list(golden["n/%s/tests" % name])
        for key in tests:
            n.add_key(handle(key))
        x = np.concatenate([golden["h/%s/feats" % key] for key in tests])
        offsets = np.cumsum([0] + [len(golden["h/%s/feats" % key]) for key in tests])
        xd = torch.from_numpy(x).cuda()
        out = torch.empty_like(xd)
        # inputs drawn only from values the key's histograms saw: the condition under which the reference itself is defined
        assert n.apply_dev(offsets, list(range(len(tests))), xd, n.dim, out, n.dim) == (0, 0), name
        want = np.concatenate([golden["off/n/%s/test/%s/out" % (name, key)] for key in tests])
        assert bits(out.cpu().numpy(), want), name


def test_the_full_loop(ctx, tmp_path):
    """frames -> HistogramEstimator per key on the device -> file -> read -> HistogramNormalization with a training histogram estimated
    from all keys -> apply: equal to the restatement run on the same host buffers"""
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    dim, bs = 40, np.float32(0.01)
    speakers = [gaussian(700 + 100 * k, dim, 2000 + k, 0.7 + 0.3 * k) for k in range(3)]
    train = rasr_amd.HistogramEstimator(ctx, dim, bs)
    paths = []
    for k, x in enumerate(speakers):
        e = rasr_amd.HistogramEstimator(ctx, dim, bs)
        for part in np.array_split(x, 3):                    # three segments of the key
            add(e, part)
            add(train, part)
        paths.append(str(tmp_path / ("speaker%d.hist" % k)))
        e.write(paths[-1])
        with open(paths[-1], "rb") as f:
            assert f.read() == hr.file_bytes(hr.estimate(x, bs)), k
    train_path = str(tmp_path / "train.hist")
    train.write(train_path)
    norm = rasr_amd.HistogramNormalization(ctx, [rasr_amd.HistogramEstimator.read(train_path)])
    for p in paths:
        norm.add_key(rasr_amd.HistogramEstimator.read(p))
    inverses = hr.training_inverses([hr.estimate(np.concatenate(speakers), bs)])
    keys = [[hr.cdf(t) for t in hr.estimate(x, bs)] for x in speakers]
    order = [2, 0, 1, 0]
    x = np.concatenate([speakers[k][:300] for k in order])
    offsets = [0, 300, 600, 900, 1200]
    want, n_test, n_inv = hr.apply_segments(x, offsets, order, keys, inverses)
    xd = torch.from_numpy(x).cuda()
    assert norm.apply_dev(offsets, order, xd, dim, xd, dim) == (n_test, n_inv) == (0, 0)
    assert bits(xd.cpu().numpy(), want)
