"""GPU parity: amx_scatter_accumulate_dev (scatter_square_kernel, scatter_class_kernel) through the C ABI against the plain
restatement of tests/scatter_reference.py.

Two classes of input.  EXACT: features k/64, weights j/16 -- every f32 product is exact and no f64 sum rounds, so the flat buffer has
one right value whatever order the device's atomics land in: np.array_equal on the whole buffer.  GAUSSIAN: the f32 products round
(a single frame into a zero buffer shows each of them bit for bit, no order being involved), and sums of several frames are held to
the project's bar for f64 sums in device order, rtol=1e-12, atol=1e-9 (tests/test_gmm_train_gpu.py); counts are exact.

Shapes.  The square sum is tiled in 64 x 64 blocks of components and in frame chunks of whole 64-frame stages; at the frame counts
used here a chunk is one stage.  dim 1, 3, 63, 64, 65 are one block and its edges, 130 is three block rows with off-diagonal and
partial blocks; T = 1, 63, 65, 257 are the stage edges, T = 145 two chunks and a remainder.  The class kernel gives every wave 32
frames and 256 components a pass.  One case at dim 440 and 2500 frames runs chunks of several stages, seven block rows and the
class kernel's second pass.
"""
import os

import numpy as np
import pytest

from tests import scatter_reference as sr

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 63, 64, 65, 130)
FRAMES = (1, 63, 65, 257, 145)
CLASSES = (1, 7, 1000)
PAD_LEFT, PAD_RIGHT = 3, 2      # the features are columns [3, 3 + dim) of a [T, dim + 5] matrix whose other columns hold NaN
RTOL, ATOL = 1e-12, 1e-9


def gaussian(T, dim, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal((T, dim)) * 2 + 0.5).astype(np.float32), rng.uniform(0.05, 2.0, T).astype(np.float32)


class Device:
    """one estimator's device buffers; run() accumulates into a zeroed buffer (or the one left by the last call) and returns it"""

    def __init__(self, ctx, dim, n_classes):
        import torch

        import rasr_amd
        self.torch, self.ctx = torch, ctx
        self.est = rasr_amd.ScatterMatricesEstimator(ctx, dim, n_classes)
        self.dim = dim
        assert self.est.accumulator_size() == sr.layout(dim, n_classes)[2]
        self.acc = torch.zeros(self.est.accumulator_size(), dtype=torch.float64, device="cuda")
        ctx.use_torch_stream()

    def run(self, x, cls, w=None, keep=False):
        torch = self.torch
        T = len(x)
        wide = np.full((T, PAD_LEFT + self.dim + PAD_RIGHT), np.nan, np.float32)
        wide[:, PAD_LEFT:PAD_LEFT + self.dim] = x
        wd = torch.from_numpy(wide).cuda()
        view = wd[:, PAD_LEFT:PAD_LEFT + self.dim]
        cd = torch.from_numpy(np.ascontiguousarray(cls, np.uint32).view(np.int32)).cuda()
        weights = None if w is None else torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda()
        if not keep:
            self.acc.zero_()
        self.est.accumulate_dev(view, wide.shape[1], T, cd, self.acc, weights)
        torch.cuda.synchronize()
        return self.acc.cpu().numpy()


def close(got, want, n_classes):
    """the Gaussian class: counts exactly, sums at the bar"""
    return np.array_equal(got[-n_classes:], want[-n_classes:]) and np.allclose(got, want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("dim", DIMS)
def test_exact_class_every_shape(ctx, dim):
    seed = 1000 * dim
    for n_classes in CLASSES:
        dev = Device(ctx, dim, n_classes)
        for T in FRAMES:
            x, _ = sr.exact_features(T, dim, seed + T)
            w, _ = sr.exact_weights(T, seed + T + 1)
            for kind in sr.ALIGNMENTS:
                cls = sr.alignment(T, n_classes, kind, seed + T + 2)
                for weights in (None, w):
                    want = sr.accumulate(x, cls, n_classes, weights)
                    got = dev.run(x, cls, weights)
                    assert np.array_equal(got, want), (n_classes, T, kind, weights is not None, int((got != want).sum()))


def test_exact_class_at_a_production_width_with_chunks_of_several_stages(ctx):
    """dim 440 (11 x 40) is 28 blocks in 7 block rows and two 256-component passes of the class kernel; on the 256 CUs of an MI355X
    2500 frames are 20 chunks of two 64-frame stages, the last chunk ending 4 frames into its second stage: the stage loop runs again,
    re-stages, and meets a chunk end inside a later stage.  (On a part with another CU count the chunking differs, the sums do not.)"""
    dim, n_classes, T = 440, 1000, 2500
    x, kx = sr.exact_features(T, dim, 440)
    w, jw = sr.exact_weights(T, 441)
    cls = sr.alignment(T, n_classes, "runs", 442)
    dev = Device(ctx, dim, n_classes)
    # the int64 twin of the restatement (equal to it on exact inputs, tests/test_scatter.py) forms these sums in a fraction of the time
    want = sr.accumulate_int(kx, cls, n_classes, jw)
    got = dev.run(x, cls, w)
    assert np.array_equal(got, want), int((got != want).sum())
    got = dev.run(x, cls, None)
    want = sr.accumulate_int(kx, cls, n_classes)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("dim", (3, 65, 130))
def test_f32_rounding_of_one_frame_bit_for_bit(ctx, dim):
    """T = 1 into a zero buffer: every entry is ONE widened f32 product -- (x_i * x_j) * w rounded twice in f32.  A product formed in
    f64, or a fused one, is another number."""
    n_classes = 7
    tri, off_counts, _ = sr.layout(dim, n_classes)
    dev = Device(ctx, dim, n_classes)
    for seed in (1, 2):
        x, w = gaussian(2, dim, 50 * dim + seed)
        for weights in (None, w):
            got = dev.run(x[:1], np.array([4], np.uint32), None if weights is None else weights[:1])
            p, y = sr.single_frame_products(x[0], None if weights is None else weights[0])
            assert np.array_equal(got[:tri], p), int((got[:tri] != p).sum())
            sums = got[tri:off_counts].reshape(n_classes, dim)
            assert np.array_equal(sums[4], y) and not np.delete(sums, 4, axis=0).any()
            assert got[off_counts + 4] == (1.0 if weights is None else np.float64(weights[0])) and got[off_counts:].sum() == got[off_counts + 4]
            if weights is not None and dim > 3:   # the test has teeth: the f64 product differs somewhere
                i, j = sr.tril(dim)
                assert (p != x[0][i].astype(np.float64) * x[0][j].astype(np.float64) * np.float64(weights[0])).any()
            # T = 2, two classes: each class sum is one widened product x * w
            got = dev.run(x, np.array([2, 5], np.uint32), weights)
            sums = got[tri:off_counts].reshape(n_classes, dim)
            for t, c in ((0, 2), (1, 5)):
                assert np.array_equal(sums[c], sr.single_frame_products(x[t], None if weights is None else weights[t])[1])
            assert np.array_equal(got, sr.accumulate(x, np.array([2, 5]), n_classes, weights))   # two addends: no order either


@pytest.mark.parametrize("dim", DIMS)
def test_gaussian_class_every_shape(ctx, dim):
    seed = 2000 * dim
    for n_classes in CLASSES:
        dev = Device(ctx, dim, n_classes)
        for T in FRAMES:
            x, w = gaussian(T, dim, seed + T)
            kind = sr.ALIGNMENTS[(T + n_classes) % 3]
            cls = sr.alignment(T, n_classes, kind, seed + T + 2)
            for weights in (None, w):
                want = sr.accumulate(x, cls, n_classes, weights)
                got = dev.run(x, cls, weights)
                assert close(got, want, n_classes), (n_classes, T, kind, weights is not None, np.abs(got - want).max())


def test_nan_reaches_the_sums_it_touches_and_a_skipped_frame_touches_none(ctx):
    dim, n_classes, T = 65, 7, 70
    x, _ = sr.exact_features(T, dim, 71)
    w, _ = sr.exact_weights(T, 72)
    cls = sr.alignment(T, n_classes, "runs", 73)
    skipped = np.nonzero(cls >= n_classes)[0]
    x[skipped[0], :] = np.nan            # a skipped frame may hold anything, its weight too
    w[skipped[1]] = np.inf
    want = sr.accumulate(x, cls, n_classes, w)
    dev = Device(ctx, dim, n_classes)
    assert np.isfinite(want).all() and np.array_equal(dev.run(x, cls, w), want)
    t = int(np.nonzero(cls < n_classes)[0][3])
    x[t, 64] = np.nan                    # row 64 of the triangle and one class sum
    with np.errstate(invalid="ignore"):
        want = sr.accumulate(x, cls, n_classes, w)
    got = dev.run(x, cls, w)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 65 + 1
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


def test_second_call_adds_and_both_contracts_give_the_same_bits(ctx):
    dim, n_classes, T = 130, 7, 145
    x, _ = sr.exact_features(T, dim, 81)
    w, _ = sr.exact_weights(T, 82)
    cls = sr.alignment(T, n_classes, "runs", 83)
    want = sr.accumulate(x, cls, n_classes, w)
    dev = Device(ctx, dim, n_classes)
    try:
        ctx.set_contract("off")
        assert np.array_equal(dev.run(x, cls, w), want)
        assert np.array_equal(dev.run(x, cls, w, keep=True), 2 * want)
        assert np.array_equal(dev.run(x, cls, None, keep=True), 2 * want + sr.accumulate(x, cls, n_classes))
        gx, gw = gaussian(1, dim, 84)
        one_off = dev.run(gx, np.array([3], np.uint32), gw)
        ctx.set_contract("fma")
        assert np.array_equal(dev.run(x, cls, w), want)
        assert np.array_equal(dev.run(gx, np.array([3], np.uint32), gw), one_off)
    finally:
        ctx.set_contract("off")


def test_the_fixtures_frames_through_the_device(ctx):
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_scatter.npz")) as z:
        g = {k: z[k] for k in z.files}
    n_classes = int(g["n_classes"])
    names = sorted({k[:-len("/feats")] for k in g if k.endswith("/feats")})
    assert len(names) == 8
    for name in names:
        x, cls, w = g[name + "/feats"], g[name + "/classes"], g.get(name + "/weights")
        want = g[name + "/off/acc"]
        got = Device(ctx, x.shape[1], n_classes).run(x, cls, w)
        if "/exact/" in name:
            assert np.array_equal(got, want), name
        else:
            assert close(got, want, n_classes), (name, np.abs(got - want).max())


def test_argument_errors(ctx):
    import torch

    from rasr_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    f, c, a = buf.data_ptr(), buf.data_ptr(), buf.data_ptr()
    for args, word in (((f, 3, 1, 0, c, 2, None, a), "dim 0"), ((f, 2000, 1, 1025, c, 2, None, a), "dim 1025"), ((f, 3, 1, 3, c, 0, None, a), "n_classes 0"),
                       ((f, 2, 1, 3, c, 2, None, a), "in_ld 2"), ((f, 3, -1, 3, c, 2, None, a), "negative frame count"),
                       ((None, 3, 1, 3, c, 2, None, a), "NULL buffer"), ((f, 3, 1, 3, None, 2, None, a), "NULL buffer"),
                       ((f, 3, 1, 3, c, 2, None, None), "NULL buffer")):
        assert L.amx_scatter_accumulate_dev(ctx.h, *args) == _lib.AMX_ERR_INVALID
        msg = L.amx_last_error().decode()
        assert msg.startswith("amx_scatter_accumulate_dev:") and word in msg, msg
    assert L.amx_scatter_accumulate_dev(ctx.h, None, 3, 0, 3, None, 2, None, None) == 0     # no frames: nothing to do
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()


def test_full_loop_context_window_to_scatter_matrices(ctx):
    """amx_context_window_dev at 9 x 16 = 144 -> accumulate -> copy back -> finalize: between + within == total, within symmetric"""
    import torch

    import rasr_amd
    fe = rasr_amd.MfccExtractor(ctx, nr_cepstrum_coefficients=16)
    off = np.concatenate([[0], np.cumsum([16000, 9000, 12000])])
    plan = fe.plan(off)
    F = plan.total_frames
    n_classes, dim = 50, 144
    ctx.use_torch_stream()
    x = (np.random.Generator(np.random.PCG64(91)).standard_normal((F, 16)) * 3).astype(np.float32)
    win = torch.zeros((F, dim), dtype=torch.float32, device="cuda")
    ctx.context_window(plan, torch.from_numpy(x).cuda(), 16, 4, 4, win, dim)
    cls = sr.alignment(F, n_classes, "runs", 92)
    est = rasr_amd.ScatterMatricesEstimator(ctx, dim, n_classes)
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    est.accumulate_dev(win, dim, F, torch.from_numpy(cls.view(np.int32)).cuda(), acc)
    torch.cuda.synchronize()
    host = acc.cpu().numpy()
    assert close(host, sr.accumulate(win.cpu().numpy(), cls, n_classes), n_classes)
    for normalize in (False, True):
        between, within, total = est.finalize(host, normalize)
        scale = np.abs(total).max()
        assert np.abs(between + within - total).max() <= 1e-12 * scale
        assert np.array_equal(within, within.T) and np.array_equal(between, between.T)
        assert np.all(np.diag(within) > 0) and np.all(np.diag(between) >= 0)
