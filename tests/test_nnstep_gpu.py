"""GPU: NN mini-batch training (nnstep.hip's update, bias, norm and bookkeeping kernels, nntrain_reduce_step_kernel) through
rasr_amd.MiniBatchTrainer against the plain restatement of tests/nnstep_reference.py.

Shapes.  Networks 24-40-33-50 and 7-130-129: no dimension is a multiple of the 128 padding or of the update kernel's 32 x 32 tile, 130
and 129 leave a nearly empty last tile in both directions of the transpose.  T = 1, 129, 300: below a tile, past one, and two frame
chunks with a padded tail.
What these shapes do not reach: a layer has at most 64 update tiles and 16 norm segments of 4096, so nnstep_stepsize_kernel and
nnstep_sum_kernel take one trip over their partial sums; nnstep_bias_kernel runs one block; the bias term with activation statistics
adds the column partials of at most eight tile rows; the activation sums and the chunk partials of a gradient never see a third frame
chunk; no network has one layer only.  tests/test_nn_wide_gpu.py (cases: tests/nn_wide_cases.py) runs the step on 300-40-260-700 and on
1030-1100 (1296 update tiles, 324 norm segments, five bias blocks) with 513 frames per mini-batch.

Bars.  Element-wise results are exact given identical inputs read back from the device: the finalized gradient, the new weights in both
images, the biases, the clipped weights, the regularised gradient, the outer product with an activation mean, and the activation
statistics themselves (on the layer inputs read back, in both contract modes).  What lies behind a sum (the regulariser's objective,
step sizes, the bias update term with statistics, gradients of a group against the restatement's, whole trajectories) is held to the bars tests/golden/make_nnstep_golden.py measured and
stored in tests/golden/ref_nnstep.npz (4 x the distance between an evaluation with f32 sums and one with f64 sums); none is written here.
"""
import functools
import os

import numpy as np
import pytest

from tests import nnstep_reference as ns
from tests import nntrain_reference as nr

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD_LEFT, PAD_RIGHT = 3, 2   # the features are columns [3, 3 + dim) of a wider matrix whose other columns hold NaN
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_nnstep.npz")
REG_NAMES = {ns.NONE: "none", ns.L1: "l1", ns.L2: "l2", ns.CENTERED_L2: "centered-l2"}
STAT_NAMES = {ns.NO_STATISTICS: None, ns.STAT_NONE: "none", ns.EXPONENTIAL_TRACE: "exponential-trace"}
EST_NAMES = {ns.SGD: "mean-normalized-sgd", ns.SGD_L1_CLIPPING: "mean-normalized-sgd-l1-clipping"}


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def trainer(ctx, net, cfg=None, log_step_size=True):
    """a MiniBatchTrainer on a copy of the restatement's network, with the restatement's configuration"""
    import rasr_amd
    pre = None
    if net.pre:
        pre = [p if isinstance(p, str) else (p[0], p[1], p[2]) for p in net.pre]
    ctx.use_torch_stream()
    tr = rasr_amd.MiniBatchTrainer(ctx, net.Ws, net.bs, net.acts, error_signal_clip=net.clip, class_weights=net.class_weights,
                                   class_to_output=net.class_to_output, preprocessing=pre)
    if cfg is not None:
        tr.set_estimator(learning_rate=float(cfg.eta), bias_learning_rate=float(cfg.eta_bias), layer_learning_rate=cfg.eta_l, regularization_constant=cfg.c,
                         trainable=[int(t) for t in cfg.trainable], regularizer=REG_NAMES[cfg.regularizer], center=cfg.center, estimator=EST_NAMES[cfg.estimator],
                         accumulate_multiple_batches=cfg.A, normalize_by_observations=cfg.normalize, log_step_size=log_step_size,
                         update_input_layer_weights=cfg.update_input, statistics_smoothing=[STAT_NAMES[m] for m in cfg.stat_mode[1:]] + [None],
                         trace_factor=[float(f) for f in cfg.stat_f[1:]] + [0.5], initial_activations=list(cfg.stat_initial[1:]) + [None],
                         input_smoothing=STAT_NAMES[cfg.stat_mode[0]], input_trace_factor=float(cfg.stat_f[0]), input_initial_activations=cfg.stat_initial[0])
    return tr


def upload(x, e, w):
    import torch
    T, dim = x.shape
    wide = np.full((T, PAD_LEFT + dim + PAD_RIGHT), np.nan, np.float32)
    wide[:, PAD_LEFT:PAD_LEFT + dim] = x
    xd = torch.from_numpy(wide).cuda()
    ed = torch.from_numpy(np.array(e, np.uint32).view(np.int32)).cuda()
    wd = None if w is None else torch.from_numpy(np.array(w, np.float64)).cuda()
    torch.cuda.synchronize()
    return xd[:, PAD_LEFT:], wide.shape[1], T, ed, wd


def images_agree(tr):
    a, b = tr.parameters(0), tr.parameters(1)
    return all(same(Wa, Wb) and same(ba, bb) for (Wa, ba), (Wb, bb) in zip(a, b))


def read(tr):
    """(Ws, bs, Gs, gs) as the device holds them"""
    p, s = tr.parameters(0), tr.step_statistics()
    return [W for W, _ in p], [b for _, b in p], [G for G, _ in s], [g for _, g in s]


# ------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("name,acts", [("a", (nr.SIGMOID, nr.RELU)), ("b", (nr.TANH,))])
def test_accumulate_equals_the_existing_pass(ctx, name, acts):
    import torch
    for T in (1, 129, 300):
        net, x, e, w = nr.variant(name, acts, T, 40 + T, frame_weights=True, class_weights=True, disregard=True, clip=0.02)
        tr = trainer(ctx, net, ns.Cfg(len(net.Ws)))
        args = upload(x, e, w)
        acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
        tr.accumulate_dev(args[0], args[1], args[2], args[3], acc, args[4])
        torch.cuda.synchronize()
        want = tr.statistics(acc)
        tr.step_accumulate_dev(*args)
        info = tr.step_info()
        for l, (G, g) in enumerate(tr.step_statistics()):
            assert np.array_equal(G.astype(np.float64), want["gradient_weights"][l]), (T, l)      # the call's f32 total, widened: every bit
            assert np.array_equal(g.astype(np.float64), want["gradient_bias"][l]), (T, l)
        assert info["n_observations"] == want["n_observations"] and info["n_classification_errors"] == want["n_classification_errors"]
        assert info["total_weight"] == F32(want["total_weight"]) and info["criterion_objective"] == F32(want["objective"])
        assert info["objective"] == info["criterion_objective"] and info["minibatch"] == 1 and not info["updated"]
        assert not info["step_size"].any()
        tr.close()


# ------------------------------------------------------------------------------------ the update
@pytest.mark.parametrize("key", sorted(ns.update_cases()))
def test_the_update_is_exact(ctx, key):
    fx = fixture()
    ref, x, e, w = ns.update_case(key)
    name, cfg = key.split("-")[0], ref.cfg
    tr = trainer(ctx, ref.net, cfg)
    tr.step_accumulate_dev(*upload(x, e, w))
    Ws, bs, Gs, gs = read(tr)
    before = tr.step_info()
    assert all(same(W, W0) and same(b, b0) for W, W0, b, b0 in zip(Ws, ref.net.Ws, bs, ref.net.bs))      # accumulate changes no parameter
    tr.step_estimate_dev()
    Ws1, bs1, Gs1, gs1 = read(tr)
    after = tr.step_info()
    # the restatement on the read-back inputs
    n = before["n_observations"]
    Gf, gf, (of, cf) = ns.finalize(cfg, Gs, gs, [before["objective"], before["criterion_objective"]], n)
    Wr, br, steps = ns.estimate(cfg, Ws, bs, Gf, gf)
    for l in range(ref.L):
        assert same(Gs1[l], Gf[l]) and same(gs1[l], gf[l]), (key, l)          # the finalized gradient replaces the gradient
        assert same(Ws1[l], Wr[l]) and same(bs1[l], br[l]), (key, l)
        assert not same(Ws1[l], Ws[l]) and not same(bs1[l], bs[l]), (key, l)
        bar = fx["bar_step_size/%s/%d" % (name, l)][0]
        print("%s step_size[%d] %.9g want %.9g bar %.3g" % (key, l, after["step_size"][l], steps[l], bar))
        assert abs(float(after["step_size"][l]) - float(steps[l])) <= bar * abs(float(steps[l])), (key, l)
    assert images_agree(tr)
    assert after["updated"] and bits(F32(after["objective"])) == bits(of) and bits(F32(after["criterion_objective"])) == bits(cf)
    # the regulariser's objective, against the restatement's on the same parameters
    if cfg.regularizer != ns.NONE:
        reg = ns.regularizer_objective(cfg, Ws, bs, n, "f64")
        bar = fx["bar_regularizer_objective/" + name][0]
        got = float(before["objective"]) - float(before["criterion_objective"])
        print("%s regulariser objective %.9g want %.9g bar %.3g" % (key, got, reg, bar))
        assert abs(got - float(reg)) <= bar * abs(float(reg)), key
    else:
        assert before["objective"] == before["criterion_objective"]
    # a second estimate on the finalized group scales nothing again (isFinalized_) and steps once more
    tr.step_estimate_dev()
    Ws2, bs2, Gs2, _ = read(tr)
    Wr2, br2, _ = ns.estimate(cfg, Ws1, bs1, Gs1, gs1)
    assert all(same(a, b) for a, b in zip(Gs2, Gs1)) and all(same(a, b) for a, b in zip(Ws2, Wr2)) and all(same(a, b) for a, b in zip(bs2, br2))
    tr.close()


@pytest.mark.parametrize("name", ["a", "b"])
def test_the_regulariser_is_exact(ctx, name):
    """two identically created handles, one without a regulariser: G_reg == axpy(c * factor, ., G_none) in every bit"""
    plain, x, e, w = ns.update_case("%s-none-sgd" % name)
    args = upload(x, e, w)
    t0 = trainer(ctx, plain.net, plain.cfg)
    t0.step_accumulate_dev(*args)
    Ws, bs, G0, g0 = read(t0)
    n = t0.step_info()["n_observations"]
    assert n == len(e)
    for reg in ("l1", "l2", "centered"):
        ref, _, _, _ = ns.update_case("%s-%s-sgd" % (name, reg))
        ref.cfg.c[-1] = 0           # one layer without a constant: it takes no regulariser
        t1 = trainer(ctx, plain.net, ref.cfg)
        t1.step_accumulate_dev(*args)
        _, _, G1, g1 = read(t1)
        Gr, gr = ns.add_gradient(ref.cfg, Ws, bs, G0, g0, n)
        for l in range(ref.L):
            assert same(G1[l], Gr[l]) and same(g1[l], gr[l]), (reg, l)
        assert same(G1[-1], G0[-1]) and not same(G1[0], G0[0])
        t1.close()
    t0.close()


def test_padding_survives_ten_steps(ctx):
    """the sigmoid 7-130-129 network with an exponential trace on the hidden layer (a padded sigmoid unit outputs 0.5: an unguarded outer
    product would write 0.5 * g into the padding rows of the output layer's weights) under the clipping estimator: after ten steps a plain accumulate_dev on the read-back parameters
    through a FRESH handle gives the same gradient bits as the stepped handle's next step_accumulate_dev.  Anything written into the
    padding of either weight image would enter the stepped handle's GEMMs and not the fresh handle's."""
    import rasr_amd
    import torch
    Ws, bs, acts = nr.network("b", (nr.SIGMOID,), 61)
    net = nr.Net(Ws, bs, acts)
    cfg = ns.Cfg(2, learning_rate=0.5, regularization_constant=[2e-4, 1e-4], estimator=ns.SGD_L1_CLIPPING,
                 statistics_smoothing=[ns.EXPONENTIAL_TRACE, ns.NO_STATISTICS], trace_factor=[0.75, 0.5])
    tr = trainer(ctx, net, cfg)
    for i in range(10):
        x, e, w = ns.teacher_frames(net.dims, 129, 7000 + i)
        info = tr.step_dev(*upload(x, e, w))
        assert info["updated"] and info["minibatch"] == i + 1
        assert images_agree(tr)
    p = tr.parameters(0)
    assert not same(p[0][0], Ws[0])
    x, e, w = ns.teacher_frames(net.dims, 300, 7777)
    args = upload(x, e, w)
    fresh = rasr_amd.FeedForwardTrainer(ctx, [W for W, _ in p], [b for _, b in p], acts)
    acc = torch.zeros(fresh.accumulator_size(), dtype=torch.float64, device="cuda")
    fresh.accumulate_dev(args[0], args[1], args[2], args[3], acc, args[4])
    torch.cuda.synchronize()
    want = fresh.statistics(acc)
    tr.set_estimator()      # no regulariser; the parameters stay
    tr.step_accumulate_dev(*args)
    for l, (G, g) in enumerate(tr.step_statistics()):
        assert np.array_equal(G.astype(np.float64), want["gradient_weights"][l]), l
        assert np.array_equal(g.astype(np.float64), want["gradient_bias"][l]), l
    fresh.close()
    tr.close()


# ------------------------------------------------------------------------------------ grouping, the counter, the quirk
def test_groups_of_two_and_the_running_factor(ctx):
    fx = fixture()
    ref, x, e, w = ns.update_case("a-l2-clip")
    ref.cfg.A = 2
    batches = [(x, e, w), (x[::-1].copy(), e[::-1].copy(), w[::-1].copy()), (x[:100], e[:100], w[:100]), (x[50:], e[50:], w[50:])]
    tr = trainer(ctx, ref.net, ref.cfg)
    two = trainer(ctx, ref.net, ref.cfg)                # the same calls in two phases
    W0 = [W.copy() for W in ref.net.Ws]
    for i, (bx, be, bw) in enumerate(batches):
        args = upload(bx, be, bw)
        before = read(tr)
        info = tr.step_dev(*args)
        assert info["minibatch"] == i + 1 and info["updated"] == (i % 2 == 1)
        assert info["n_observations"] == (len(be) if i % 2 == 0 else len(batches[i - 1][1]) + len(be))
        after = read(tr)
        # the regulariser's factor is the group's running count: G = fmaf(c * n_running, W, G_before + call)
        single = trainer(ctx, nr.Net(before[0], before[1], ref.net.acts), ns.Cfg(ref.L))      # one call's gradient bits: a group of one, no regulariser
        single.step_accumulate_dev(*args)
        _, _, Gc, gc = read(single)
        single.close()
        if not info["updated"]:
            assert all(same(a, b) for a, b in zip(after[0], before[0])) and all(same(a, b) for a, b in zip(after[1], before[1]))      # no parameter bit changes
            start = [np.zeros_like(G) for G in Gc] if i % 2 == 0 else before[2]
            startb = [np.zeros_like(g) for g in gc] if i % 2 == 0 else before[3]
            Gr, gr = ns.add_gradient(ref.cfg, before[0], before[1], [(a + b).astype(F32) for a, b in zip(start, Gc)], [(a + b).astype(F32) for a, b in zip(startb, gc)],
                                     info["n_observations"])
            assert all(same(a, b) for a, b in zip(after[2], Gr)) and all(same(a, b) for a, b in zip(after[3], gr)), i
        else:
            Gr, gr = ns.add_gradient(ref.cfg, before[0], before[1], [(a + b).astype(F32) for a, b in zip(before[2], Gc)],
                                     [(a + b).astype(F32) for a, b in zip(before[3], gc)], info["n_observations"])
            Gf, gf, _ = ns.finalize(ref.cfg, Gr, gr, [0.0], info["n_observations"])
            Wr, br, _ = ns.estimate(ref.cfg, before[0], before[1], Gf, gf)
            assert all(same(a, b) for a, b in zip(after[0], Wr)) and all(same(a, b) for a, b in zip(after[1], br)), i
            assert all(same(a, b) for a, b in zip(after[2], Gf)), i
        # two phases give the same bits
        two.step_accumulate_dev(*args)
        if i % 2 == 1:
            two.step_estimate_dev()
        assert all(same(a, b) for ra, rb in zip(read(tr), read(two)) for a, b in zip(ra, rb)), i
        i2 = two.step_info()
        assert (i2["objective"], i2["criterion_objective"], i2["total_weight"]) == (info["objective"], info["criterion_objective"], info["total_weight"])
    assert not same(read(tr)[0][0], W0[0])
    # the group's gradient against the restatement's own (its gradient is another sum): the fixture's bar
    r2 = ns.Trainer(nr.Net(W0, ref.net.bs, ref.net.acts), ref.cfg)
    t2 = trainer(ctx, r2.net, ref.cfg)
    for bx, be, bw in batches[:2]:
        r2.step_accumulate(bx, be, bw)
        t2.step_accumulate_dev(*upload(bx, be, bw))
    for l, (G, g) in enumerate(t2.step_statistics()):
        for block, got, want in (("gradient_weights", G, r2.G[l]), ("gradient_bias", g, r2.g[l])):
            bar = fx["bar_group_%s/a/%d" % (block, l)][0]
            dev = np.abs(got.astype(np.float64) - want).max()
            print("group %s[%d] dev %.3g of %.3g" % (block, l, dev, bar * np.abs(want).max()))
            assert dev <= bar * np.abs(want).max(), (block, l)
    for t in (tr, two, t2):
        t.close()


def test_the_input_layer_quirk_and_frozen_layers(ctx):
    ref, x, e, w = ns.update_case("b-l2-sgd")
    args = upload(x, e, w)
    ref.cfg.update_input = False
    tr = trainer(ctx, ref.net, ref.cfg)
    info = tr.step_dev(*args)
    Ws, bs, Gs, gs = read(tr)
    assert same(Ws[0], ref.net.Ws[0]) and not same(bs[0], ref.net.bs[0]) and not same(Ws[1], ref.net.Ws[1])     # the text as it stands
    _, _, steps = ns.estimate(ref.cfg, ref.net.Ws, ref.net.bs, Gs, gs)
    bar = fixture()["bar_step_size/b/0"][0]
    assert abs(float(info["step_size"][0]) - float(steps[0])) <= bar * float(steps[0])        # the bias's part alone
    assert images_agree(tr)
    tr.close()
    # with a preprocessing layer in front, layer 0 has a predecessor and its weights move
    net, x2, e2, w2 = nr.variant("b", (nr.TANH,), 129, 88, pre=True)
    tr = trainer(ctx, net, ref.cfg)
    tr.step_dev(*upload(x2, e2, w2))
    assert not same(tr.parameters(0)[0][0], net.Ws[0])
    tr.close()
    # a layer that is not trainable keeps its parameters; its gradient is still finalized
    ref, x, e, w = ns.update_case("a-l2-clip")
    ref.cfg.trainable[1] = False
    tr = trainer(ctx, ref.net, ref.cfg)
    tr.step_accumulate_dev(*upload(x, e, w))
    Ws, bs, Gs, gs = read(tr)
    tr.step_estimate_dev()
    Ws1, bs1, Gs1, gs1 = read(tr)
    Gf, gf, _ = ns.finalize(ref.cfg, Gs, gs, [0.0], len(e))
    Wr, br, steps = ns.estimate(ref.cfg, Ws, bs, Gf, gf)
    assert same(Ws1[1], Ws[1]) and same(bs1[1], bs[1]) and same(Gs1[1], Gf[1]) and tr.step_info()["step_size"][1] == 0
    assert all(same(a, b) for a, b in zip(Ws1, Wr)) and all(same(a, b) for a, b in zip(bs1, br)) and images_agree(tr)
    tr.close()


def test_without_normalisation_and_without_step_sizes(ctx):
    ref, x, e, w = ns.update_case("b-l1-clip")
    ref.cfg.normalize = False
    tr = trainer(ctx, ref.net, ref.cfg, log_step_size=False)
    tr.step_accumulate_dev(*upload(x, e, w))
    Ws, bs, Gs, gs = read(tr)
    before = tr.step_info()
    tr.step_estimate_dev()
    Ws1, bs1, Gs1, _ = read(tr)
    Wr, br, _ = ns.estimate(ref.cfg, Ws, bs, Gs, gs)
    assert all(same(a, b) for a, b in zip(Gs1, Gs)) and all(same(a, b) for a, b in zip(Ws1, Wr)) and all(same(a, b) for a, b in zip(bs1, br))
    after = tr.step_info()
    assert after["objective"] == before["objective"] and not after["step_size"].any()
    tr.close()


# ------------------------------------------------------------------------------------ trajectories, the batch estimator, refusals
@pytest.mark.parametrize("key", sorted(ns.TRAJECTORIES))
def test_whole_trajectories(ctx, key):
    fx = fixture()
    ref, batches = ns.trajectory(key)
    tr = trainer(ctx, ref.net, ref.cfg)
    objective = []
    for i, (x, e, w) in enumerate(batches):
        info = tr.step_dev(*upload(x, e, w))
        if not info["updated"]:
            continue
        objective.append(info["objective"])
        step = (i + 1) // ref.cfg.A
        if step in ns.TRAJECTORY_STEPS:
            for l, (W, b) in enumerate(tr.parameters(0)):
                for p, got in (("W", W), ("b", b)):
                    want, bar = fx["traj/%s/%d/%s%d" % (key, step, p, l)], fx["bar_traj/%s/%d/%s%d" % (key, step, p, l)][0]
                    dev = np.abs(got.astype(np.float64) - want).max()
                    print("%s step %d %s%d dev %.3g of %.3g" % (key, step, p, l, dev, bar * np.abs(want).max()))
                    assert dev <= bar * np.abs(want).max(), (key, step, p, l)
            assert images_agree(tr)
    assert len(objective) == max(ns.TRAJECTORY_STEPS) and objective[-1] < objective[0]
    tr.close()


def test_the_batch_estimator_on_a_combined_buffer(ctx, tmp_path):
    import rasr_amd
    import torch
    for key in ("a-centered-clip", "b-l1-sgd"):
        ref, x, e, w = ns.update_case(key)
        tr = trainer(ctx, ref.net, ref.cfg)
        acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
        for bx, be, bw in ((x, e, w), (x[::-1].copy(), e[::-1].copy(), w[::-1].copy())):
            a = upload(bx, be, bw)
            tr.accumulate_dev(a[0], a[1], a[2], a[3], acc, a[4])
        torch.cuda.synchronize()
        host = acc.cpu().numpy()
        # through two files and combine, as acoustic-model-trainer's ranks leave them
        tr.write(host, str(tmp_path / "s1"))
        combined = rasr_amd.combine_nn_statistics(tr, [str(tmp_path / "s1")])
        info = tr.estimate(combined)
        want = ref.batch_estimate(host)
        Ws, bs, Gs, gs = read(tr)
        for l in range(ref.L):
            assert same(Gs[l], ref.G[l]) and same(gs[l], ref.g[l]), (key, l)        # narrowed, regularised with factor nObservations, finalized
            assert same(Ws[l], ref.net.Ws[l]) and same(bs[l], ref.net.bs[l]), (key, l)
        assert images_agree(tr)
        assert info["updated"] and info["n_observations"] == want["n_observations"] == 2 * len(e)
        assert info["n_classification_errors"] == want["n_classification_errors"] and info["total_weight"] == F32(want["total_weight"])
        assert info["criterion_objective"] == F32(want["criterion_objective"])
        bar = fixture()["bar_regularizer_objective/" + key[0]][0]
        reg = float(want["objective"]) - float(want["criterion_objective"])
        assert abs((info["objective"] - info["criterion_objective"]) - reg) <= bar * abs(reg)
        tr.close()


def test_refusals_on_the_device(ctx):
    import rasr_amd
    from rasr_amd import _lib
    ref, x, e, w = ns.update_case("b-none-sgd")
    tr = trainer(ctx, ref.net)
    args = upload(x, e, w)
    for call in (lambda: tr.step_dev(*args), tr.step_estimate_dev, tr.step_info, tr.step_statistics):
        with pytest.raises(rasr_amd.AmxError) as err:
            call()
        assert err.value.status == _lib.AMX_ERR_STATE and "no estimator is set" in str(err.value)
    ref.cfg.A = 2
    tr = trainer(ctx, ref.net, ref.cfg)
    tr.step_accumulate_dev(*args)
    before, info = read(tr), tr.step_info()
    bad = e.copy()
    bad[5] = 129        # one past the last class
    with pytest.raises(rasr_amd.AmxError) as err:
        tr.step_dev(*upload(x, bad, w))
    assert err.value.status == _lib.AMX_ERR_INVALID and "frame 5" in str(err.value)
    with pytest.raises(rasr_amd.AmxError, match="T = 0"):
        tr.step_accumulate_dev(args[0], args[1], 0, args[3], args[4])
    after = tr.step_info()
    assert after["minibatch"] == 1 and after["n_observations"] == info["n_observations"] and after["objective"] == info["objective"]
    assert all(same(a, b) for ra, rb in zip(before, read(tr)) for a, b in zip(ra, rb))       # a refused call in the middle of a group changes nothing
    tr.close()


# ------------------------------------------------------------------------------------ activation statistics
def device_statistics(tr, ref, x, e, w, contract):
    """one step_accumulate_dev; the restatement's statistics updated from the layer inputs READ BACK from the device"""
    T = len(e)
    tr.step_accumulate_dev(*upload(x, e, w))
    keep, _, _ = nr.labels(e, ref.net.class_to_output, ref.net.class_weights, None)
    idx = np.nonzero(keep)[0]
    inputs = {p: tr.layer_input(p, T)[keep] for p, st in enumerate(ref.stats) if st is not None}
    return inputs, idx


@pytest.mark.parametrize("contract", ["fma", "off"])
def test_activation_statistics_in_both_contract_modes(ctx, contract):
    fx = fixture()
    c = ns.CONTRACT_FMA if contract == "fma" else ns.CONTRACT_OFF
    before = ctx.contract()      # the session's context is shared: it goes back to what it was
    ctx.set_contract(contract)
    try:
        for key in ("a-none-sgd", "a-trace-sgd", "b-none-sgd", "b-trace-sgd"):
            for T in (129, 300):
                ref, x, e, w = ns.stat_case(key, T=T)
                tr = trainer(ctx, ref.net, ref.cfg)
                one = [None if st is None else ns.ActStat(st.mode, st.f, st.n) for st in ref.stats]
                for batch in range(2):      # the second batch continues the sums (and, for the trace, is no first batch)
                    bx = x if batch == 0 else x[::-1].copy()
                    inputs, idx = device_statistics(tr, ref, bx, e, w, c)
                    for p, X in inputs.items():
                        ref.stats[p].update(X, idx, c)
                        one[p].update(X, idx, c, single_chain=True)
                    got = tr.activation_statistics()
                    assert sorted(got) == [p - 1 for p in sorted(inputs)]
                    for p in inputs:
                        mean, var = got[p - 1]
                        assert same(mean, ref.stats[p].mean()) and same(var, ref.stats[p].variance()), (key, T, batch, p)      # the library's order: exact
                        bar = fx["bar_activation_sums/" + key[0]][0]      # the reference's one chain: within the bar when two chunks were cut
                        dev = np.abs(mean.astype(np.float64) - one[p].mean()).max()
                        print("%s T=%d batch %d layer %d mean dev %.3g of %.3g" % (key, T, batch, p - 1, dev, bar * np.abs(one[p].mean()).max()))
                        assert dev <= bar * np.abs(one[p].mean()).max() and (T > 256 or same(mean, one[p].mean())), (key, T, batch, p)
                tr.close()
    finally:
        ctx.set_contract(before)


def test_initial_activation_mean_and_deviation_are_honoured(ctx, tmp_path):
    import rasr_amd
    for mode in (ns.STAT_NONE, ns.EXPONENTIAL_TRACE):
        ref, x, e, w = ns.stat_case("b-none-sgd")
        rng = np.random.Generator(np.random.PCG64(3))
        initial = (rng.uniform(-0.5, 0.5, 130).astype(F32), rng.uniform(0.5, 1.5, 130).astype(F32))
        cfg = ns.Cfg(2, statistics_smoothing=[mode, ns.NO_STATISTICS], trace_factor=[0.75, 0.5], initial_activations=[initial, None])
        ref = ns.Trainer(ref.net, cfg)
        tr = trainer(ctx, ref.net, cfg)
        with pytest.raises(rasr_amd.AmxError, match="no mini-batch"):
            tr.activation_statistics()
        c = ns.CONTRACT_FMA if ctx.contract() == "fma" else ns.CONTRACT_OFF      # whichever the session's context follows
        inputs, idx = device_statistics(tr, ref, x, e, w, c)
        plain = ns.ActStat(mode, 0.75, 130)
        for p, X in inputs.items():
            ref.stats[p].update(X, idx, c)
            plain.update(X, idx, c)
        mean, var = tr.activation_statistics()[0]
        assert same(mean, ref.stats[1].mean()) and same(var, ref.stats[1].variance()) and not same(mean, plain.mean())
        # save writes the mean and the square root of the variance as the scorers' vector files
        tr.save(str(tmp_path / "net"))
        back = rasr_amd._read_vector("amx_nn_vector_read_f32", str(tmp_path / "net-layer-1-activation-mean.xml"), __import__("ctypes").c_float, np.float32)
        assert np.allclose(back, mean, rtol=1e-6) and os.path.exists(str(tmp_path / "net-layer-1-activation-standard-deviation.xml"))
        tr.close()


@pytest.mark.parametrize("key", sorted(ns.stat_cases()))
def test_the_update_with_activation_statistics(ctx, key):
    """the outer product, the weights in both images and the update term of the weights are exact given the read-back gradient, parameters
    and means; the update term of the bias lies behind a gemv and is held to the fixture's bar, the bias is exact given that term"""
    fx = fixture()
    ref, x, e, w = ns.stat_case(key)
    name, cfg = key.split("-")[0], ref.cfg
    tr = trainer(ctx, ref.net, cfg)
    tr.step_accumulate_dev(*upload(x, e, w))
    Ws, bs, Gs, gs = read(tr)
    stats = tr.activation_statistics()
    means = [None] + [stats[l][0] for l in range(ref.L - 1)]
    n = tr.step_info()["n_observations"]
    tr.step_estimate_dev()
    Ws1, bs1, Gs1, gs1 = read(tr)
    Gf, gf, _ = ns.finalize(cfg, Gs, gs, [0.0], n)
    Wr, br, _ = ns.estimate(cfg, Ws, bs, Gf, gf, means=means)       # Gf, gf become the update terms
    plain_W, _, _ = ns.estimate(cfg, Ws, bs, *ns.finalize(cfg, Gs, gs, [0.0], n)[:2])
    for l in range(ref.L):
        assert same(Gs1[l], Gf[l]) and same(Ws1[l], Wr[l]), (key, l)
        if means[l] is None:
            assert same(gs1[l], gf[l]) and same(bs1[l], br[l]), (key, l)
            continue
        assert not same(Ws1[l], plain_W[l]), (key, l)           # the mean did enter
        bar = fx["bar_delta_bias/%s/%d" % (name, l)][0]
        dev = np.abs(gs1[l].astype(np.float64) - gf[l]).max()
        print("%s bias update term[%d] dev %.3g of %.3g" % (key, l, dev, bar * np.abs(gf[l]).max()))
        assert dev <= bar * np.abs(gf[l]).max(), (key, l)
        rate = F32(F32(cfg.eta * cfg.eta_bias) * cfg.eta_l[l])
        b = ns.axpy(-rate, gs1[l], bs[l])
        if cfg.estimator == ns.SGD_L1_CLIPPING:
            b = ns.l1_clip(b, F32(F32(cfg.c[l] * cfg.eta) * cfg.eta_l[l]))
        assert same(bs1[l], b), (key, l)
    assert images_agree(tr)
    tr.close()
