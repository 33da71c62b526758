"""GPU: amx_nntrain_accumulate_dev (forward on gemm_f32_kernel, nntrain_error_kernel, nntrain_gemm_bwd_kernel, nntrain_gemm_tn_kernel,
the column sums and the tail) through rasr_amd.FeedForwardTrainer against the plain restatement of tests/nntrain_reference.py.

Shapes.  Networks 24-40-33-50 and 7-130-129: no dimension is a multiple of the 128 tile, 130 and 129 are two tiles with a nearly empty
second one.  T = 1, 31, 127, 128, 129, 300: the tile edge from both sides and, at 300, two frame chunks (AMX_NNTRAIN_CHUNK = 256) with a
padded tail.  Every hidden activation set runs plain at every T and with one option per T (frame weights, class weights, disregarded
classes, preprocessing layers, the clip) and all of them at T = 300.
What these shapes do not reach: with at most 130 outputs and 24 features every 256-strided loop (softmax, arg-max, error signal, column
sums) takes one trip, so waves 2 and 3 of the arg-max hold no candidate and its cross-wave tie rule is never decided; the tile grids are
1 x 1, 1 x 2 and 2 x 2, never with more k-tiles than n-tiles and never three to a side; a call has two frame chunks at most and stays far
below AMX_NNTRAIN_MAX_FRAMES; every network has hidden layers; the labels are random, so nearly every frame is a classification error
whatever the arg-max says.  tests/test_nn_wide_gpu.py (cases: tests/nn_wide_cases.py) runs the same pass on 300-40-260-700 and
1030-1100 with 513 to 4096 frames and labels of which half are right.

Bars.  Counts, observations, classification errors and the total weight are exact.  Gradients, bias gradients, feature sums and the
objective are held to the bars tests/golden/make_nntrain_golden.py measured and stored in tests/golden/ref_nntrain.npz (4 x the
distance between an sgemm and an f64 evaluation, relative to the block's largest magnitude); none is written here.
"""
import functools
import os

import numpy as np
import pytest

from tests import nntrain_reference as nr

pytestmark = pytest.mark.gpu

ALL = nr.CLASS_COUNTS | nr.MEAN_AND_VARIANCE | nr.BASE | nr.GRADIENT
PAD_LEFT, PAD_RIGHT = 3, 2   # the features are columns [3, 3 + dim) of a wider matrix whose other columns hold NaN
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_nntrain.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(key):
    kw = nr.gpu_cases()[key]
    net, x, e, w = nr.variant(**kw)
    want = nr.accumulate(net, x, e, w, mask=ALL, products="f64")
    for v in (x, e) + ((w,) if w is not None else ()):
        v.setflags(write=False)
    return kw["name"], net, x, e, w, want


def trainer(ctx, net, mask=ALL):
    import rasr_amd
    pre = None
    if net.pre:
        pre = [p if isinstance(p, str) else (p[0], p[1], p[2]) for p in net.pre]
    ctx.use_torch_stream()
    return rasr_amd.FeedForwardTrainer(ctx, net.Ws, net.bs, net.acts, statistics=mask, error_signal_clip=net.clip, class_weights=net.class_weights,
                                       class_to_output=net.class_to_output, preprocessing=pre)


def run(tr, x, e, w, acc=None):
    """one accumulate_dev call on a strided feature view; returns the host copy of the buffer"""
    import torch
    T, dim = x.shape
    wide = np.full((T, PAD_LEFT + dim + PAD_RIGHT), np.nan, np.float32)
    wide[:, PAD_LEFT:PAD_LEFT + dim] = x
    xd = torch.from_numpy(wide).cuda()
    ed = torch.from_numpy(np.array(e, np.uint32).view(np.int32)).cuda()
    wd = None if w is None else torch.from_numpy(np.array(w, np.float64)).cuda()
    if acc is None:
        acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    tr.accumulate_dev(xd[:, PAD_LEFT:], wide.shape[1], T, ed, acc, wd)
    torch.cuda.synchronize()
    return acc.cpu().numpy()


def check(tr, got, want, name, what):
    fx, s = fixture(), tr.statistics(got)
    assert s["n_observations"] == want["n_observations"], what
    assert np.array_equal(s["class_counts"], want["class_counts"]), what
    assert s["n_classification_errors"] == want["n_classification_errors"], what
    assert s["total_weight"] == want["total_weight"], what
    bar = fx["bar_objective/" + name][0]
    print("%s objective %.9g want %.9g bar %.3g" % (what, s["objective"], want["objective"], bar))
    assert abs(s["objective"] - want["objective"]) <= bar * abs(want["objective"]), what
    for block in ("feature_sum", "feature_square_sum"):
        bar, ref = fx["bar_%s/%s" % (block, name)][0], want[block]
        dev = np.abs(s[block] - ref).max()
        print("%s %s dev %.3g of %.3g" % (what, block, dev, bar * np.abs(ref).max()))
        assert dev <= bar * np.abs(ref).max(), (what, block)
    for l in range(tr.n_layers):
        for block in ("gradient_weights", "gradient_bias"):
            bar, ref = fx["bar_%s/%s/%d" % (block, name, l)][0], want[block][l]
            assert s[block][l].shape == ref.shape
            dev = np.abs(s[block][l] - ref).max()
            print("%s %s[%d] dev %.3g of %.3g" % (what, block, l, dev, bar * np.abs(ref).max()))
            assert dev <= bar * np.abs(ref).max(), (what, block, l)


ACT_SETS = sorted({k.split("-T")[0] for k in nr.gpu_cases()})


@pytest.mark.parametrize("prefix", ACT_SETS)
def test_every_shape_and_option_against_the_restatement(ctx, prefix):
    keys = [k for k in nr.gpu_cases() if k.split("-T")[0] == prefix]
    assert len(keys) == 2 * len(nr.FRAMES)
    for key in keys:
        name, net, x, e, w, want = case(key)
        tr = trainer(ctx, net)
        assert tr.accumulator_size() == nr.layout(net.dims, net.dims[0], net.dims[-1], ALL)["size"]
        check(tr, run(tr, x, e, w), want, name, key)
        tr.close()


def test_two_calls_into_one_buffer_equal_the_sum_of_two_buffers(ctx):
    import torch
    _, net, x, e, w, _ = case("a-32-T300-class_weights+clip+disregard+frame_weights+pre")
    tr = trainer(ctx, net)
    first, second = run(tr, x[:170], e[:170], w[:170]), run(tr, x[170:], e[170:], w[170:])
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    run(tr, x[:170], e[:170], w[:170], acc)
    both = run(tr, x[170:], e[170:], w[170:], acc)
    assert np.array_equal(both, first + second)
    assert tr.statistics(both)["n_observations"] == tr.statistics(first)["n_observations"] + tr.statistics(second)["n_observations"]


def test_the_same_call_gives_the_same_bits(ctx):
    _, net, x, e, w, _ = case("b-3-T300-class_weights+clip+disregard+frame_weights+pre")
    _, other, ox, oe, ow, _ = case("a-21-T129")
    tr = trainer(ctx, net)
    first = run(tr, x, e, w)
    assert np.array_equal(run(tr, x, e, w), first)                    # repeated
    run(tr, x[:31], e[:31], w[:31])                                    # after a call of another length (the workspaces hold its traces)
    assert np.array_equal(run(tr, x, e, w), first)
    tr2 = trainer(ctx, other)                                          # after another handle's work
    run(tr2, ox, oe, ow)
    assert np.array_equal(run(tr, x, e, w), first)
    assert np.array_equal(run(trainer(ctx, net), x, e, w), first)      # a fresh handle


def test_a_bad_label_is_refused_with_the_frame_named_and_the_buffer_untouched(ctx):
    import torch

    import rasr_amd
    _, net, x, e, w, _ = case("a-21-T129")
    tr = trainer(ctx, net)
    acc = torch.arange(tr.accumulator_size(), dtype=torch.float64, device="cuda") * 0.5 + 1.0
    before = acc.cpu().numpy()
    bad = e.copy()
    bad[77] = net.dims[-1]           # the first class that does not exist
    bad[100] = 0xFFFFFFFF
    with pytest.raises(rasr_amd.AmxError) as err:
        run(tr, x, bad, w, acc)
    assert err.value.status == rasr_amd._lib.AMX_ERR_INVALID and "frame 77" in str(err.value)
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), before)
    # the handle goes on working
    assert np.array_equal(run(tr, x, e, w), run(trainer(ctx, net), x, e, w))


def test_planted_ties_and_a_vanished_probability(ctx):
    """a top layer of zeros: every softmax value of a frame is the same, argMax answers 0 (the first), so every frame whose label is not
    0 is an error; a top layer that leaves p[label] = 0 makes the objective +inf, and it is kept"""
    rng = np.random.Generator(np.random.PCG64(5))
    dims, T = [7, 130, 129], 200
    Ws = [rng.standard_normal((130, 7)).astype(np.float32), np.zeros((129, 130), np.float32)]
    bs = [np.zeros(130, np.float32), np.zeros(129, np.float32)]
    net = nr.Net(Ws, bs, [nr.TANH, nr.NONE])
    x, e, _ = nr.frames(dims, T, 6)
    tr = trainer(ctx, net)
    s = tr.statistics(run(tr, x, e, None))
    want = nr.accumulate(net, x, e, None, mask=ALL)
    assert s["n_classification_errors"] == int((e != 0).sum()) == want["n_classification_errors"]
    assert s["n_observations"] == T and s["total_weight"] == float(T)
    assert abs(s["objective"] - want["objective"]) <= fixture()["bar_objective/b"][0] * want["objective"]
    bs[1][:] = [-200.0 * (i == 5) for i in range(129)]     # exp(-200) is 0 in f32: p[5] = 0
    net = nr.Net(Ws, bs, [nr.TANH, nr.NONE])
    e[:] = 5
    tr = trainer(ctx, net, mask=nr.BASE)
    s = tr.statistics(run(tr, x, e, None))
    assert s["objective"] == np.inf and s["n_classification_errors"] == T


def test_mean_and_variance_and_class_counts_need_no_network(ctx):
    import torch

    import rasr_amd
    rng = np.random.Generator(np.random.PCG64(9))
    T, dim, n_out = 300, 45, 17
    x = (rng.standard_normal((T, dim)) * 2 + 1).astype(np.float32)
    e = rng.integers(0, n_out, T).astype(np.uint32)
    w = rng.uniform(0.25, 2.0, T)
    ctx.use_torch_stream()
    tr = rasr_amd.FeedForwardTrainer(ctx, statistics=("mean-and-variance", "class-counts"), feature_dim=dim, n_outputs=n_out)
    s = tr.statistics(run(tr, x, e, w))
    want = nr.accumulate(nr.Net([np.zeros((n_out, dim), np.float32)], [np.zeros(n_out, np.float32)], [nr.NONE]), x, e, w,
                         mask=nr.MEAN_AND_VARIANCE | nr.CLASS_COUNTS)
    assert s["n_observations"] == T and np.array_equal(s["class_counts"], want["class_counts"]) and s["total_weight"] == want["total_weight"]
    fx = fixture()
    for block in ("feature_sum", "feature_square_sum"):
        bar = max(fx["bar_%s/a" % block][0], fx["bar_%s/b" % block][0])
        assert np.abs(s[block] - want[block]).max() <= bar * np.abs(want[block]).max(), block
    # mean and variance alone: no labels at all
    tr = rasr_amd.FeedForwardTrainer(ctx, statistics=("mean-and-variance",), feature_dim=dim)
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    tr.accumulate(x, None, acc)
    mean, dev = rasr_amd.mean_and_deviation(tr, acc)
    assert np.allclose(mean, x.astype(np.float64).mean(0), rtol=1e-5, atol=1e-6) and np.allclose(dev, x.astype(np.float64).std(0), rtol=1e-4)


def test_a_buffer_written_read_and_combined_round_trips(ctx, tmp_path):
    import rasr_amd
    _, net, x, e, w, _ = case("a-32-T300-class_weights+clip+disregard+frame_weights+pre")
    tr = trainer(ctx, net)
    a, b = run(tr, x[:170], e[:170], w[:170]), run(tr, x[170:], e[170:], w[170:])
    pa, pb = str(tmp_path / "a.stat"), str(tmp_path / "b.stat")
    tr.write(a, pa)
    tr.write(b, pb)
    dims = net.dims
    assert open(pa, "rb").read() == nr.statistics_bytes(a, dims, dims[0], dims[-1], ALL)
    ra, rb = tr.read(pa), tr.read(pb)
    assert np.array_equal(ra, nr.narrowed(a, dims, dims[0], dims[-1], ALL))
    both = rasr_amd.combine_nn_statistics(tr, [pa, pb])
    y = tr.layout
    want = (ra.astype(np.float32) + rb.astype(np.float32)).astype(np.float64)      # Statistics<f32>::add
    want[y.tail], want[y.tail + 1] = ra[y.tail] + rb[y.tail], ra[y.tail + 1] + rb[y.tail + 1]
    want[y.class_counts:y.class_counts + dims[-1]] = (ra + rb)[y.class_counts:y.class_counts + dims[-1]]
    assert np.array_equal(both, want)
    prior = rasr_amd.prior_from_class_counts(tr, both, back_off_count=1)
    assert np.array_equal(prior, nr.prior_from_class_counts(tr.statistics(both)["class_counts"], net.class_weights, 1))
