"""amx_nntrain_cfg.gemm = AMX_NNTRAIN_GEMM_BF16X3 (rasr_amd/csrc/nntrain_x3.hpp): the three GEMM kinds of NN training on split bf16.

Reference: the all-f64 evaluation nntrain_reference.accumulate(products="f64").  Bar per block (gradient and bias gradient per layer,
objective), relative to the block's largest magnitude: 4 x (d_split + d_f32), both measured on the CPU from the reference alone --
d_split: the distance of split_pass() below (every GEMM operand replaced by its split_bf16x3 planes, hi hi + hi lo + lo hi summed in
f64) from the f64 evaluation, d_f32: that of products="f32".  4: the project's margin (the order inside a matrix instruction is not
ours to know; the activations' slope is at most 1).  test_the_bar_is_sharp: a pass without one cross term, or without the lo planes,
leaves the bar on every case.  Cases: T = 1, 257, 300 (the 256-frame chunk crossed, a short last one), 513 on 1030-1100 (three chunks, 9 x 9
tiles); 130 units, K = 97; every hidden activation, three layers once; frame weights, a disregarded class, a finite clip."""
import functools

import numpy as np
import pytest

from tests import nnstep_reference as ns
from tests import nntrain_reference as nr
from tests.split_gemm_reference import split_bf16x3

F32, F64 = np.float32, np.float64
ALL = nr.CLASS_COUNTS | nr.MEAN_AND_VARIANCE | nr.BASE | nr.GRADIENT
OPT = dict(frame_weights=True, disregard=True)
CASES = {"sigmoid-relu-T300": dict(name=(97, 130, 40, 50), acts=(nr.SIGMOID, nr.RELU), T=300, seed=11, clip=0.02, **OPT),
         "tanh-T257": dict(name=(97, 130, 129), acts=(nr.TANH,), T=257, seed=12, **OPT),
         "linear-T1": dict(name=(7, 130, 129), acts=(nr.NONE,), T=1, seed=13),
         "wide-T513": dict(name=(1030, 1100), acts=(), T=513, seed=14, **OPT)}
GAP_ULP = 4096   # 2^-12 of the larger softmax value: the split's error of a logit is about 2^-17 |z|


def x3_matmul(a, b, drop=None):
    """a [m x k] . b [k x n], both split along k; drop: "cross" (no lo hi) or "lo" (hi hi alone)"""
    (ah, al), (bh, bl) = (tuple(p.astype(F64) for p in split_bf16x3(v)) for v in (a, b.T))
    s = ah @ bh.T
    if drop != "lo":
        s = s + ah @ bl.T + (0 if drop == "cross" else al @ bh.T)
    return s


def split_pass(net, feats, emission, weights, drop=None):
    """nntrain_reference.accumulate's BASE | GRADIENT blocks with x3_matmul for every matrix product"""
    keep, o, w = nr.labels(emission, net.class_to_output, net.class_weights, weights)
    X, L = [nr.preprocess(np.asarray(feats, F32)[keep], net.pre)], len(net.Ws)
    for l in range(L):
        z = (x3_matmul(X[l], net.Ws[l].T, drop).astype(F32) + net.bs[l][None, :]).astype(F32)
        if l < L - 1:
            X.append(nr.activate(z, net.acts[l]))
    p = nr.softmax(z)
    do_clip = net.clip is not None and net.clip < nr.FLT_MAX
    E = [None] * L
    E[L - 1] = (nr.kronecker(p, o) * w[:, None]).astype(F32)
    if do_clip and L > 1:
        E[L - 1] = nr.clip(E[L - 1], net.clip)
    for l in range(L - 1, 0, -1):
        d, y, act = x3_matmul(E[l], net.Ws[l], drop).astype(F32), X[l], net.acts[l - 1]
        d = nr.sigmoid_derivative(d, y) if act == nr.SIGMOID else nr.tanh_derivative(d, y) if act == nr.TANH else nr.rectified_derivative(d, y) if act == nr.RELU else d
        E[l - 1] = nr.clip(d, net.clip) if do_clip and l - 1 > 0 else d
    return {"objective": float(nr.objective_terms(p, o, w).astype(F64).sum()), "gradient_weights": [x3_matmul(X[l].T, E[l], drop) for l in range(L)],
            "gradient_bias": [E[l].astype(F64).sum(0) for l in range(L)]}


def blocks(s):
    d = {"objective": np.array([s["objective"]], F64)}
    for l, (G, g) in enumerate(zip(s["gradient_weights"], s["gradient_bias"])):
        d["gradient_weights/%d" % l], d["gradient_bias/%d" % l] = np.asarray(G, F64), np.asarray(g, F64)
    return d


def fractions(got, want, bars):
    """per block: distance from the reference, relative to its largest magnitude, as a fraction of the bar"""
    return {k: float(np.abs(blocks(got)[k] - v).max() / np.abs(v).max() / bars[k]) for k, v in blocks(want).items()}


def bars_of(net, x, e, w):
    want = nr.accumulate(net, x, e, w, mask=nr.BASE | nr.GRADIENT, products="f64")
    one = dict.fromkeys(blocks(want), 1.0)
    d_split, d_f32 = fractions(split_pass(net, x, e, w), want, one), fractions(nr.accumulate(net, x, e, w, mask=nr.BASE | nr.GRADIENT, products="f32"), want, one)
    return want, {k: 4.0 * (d_split[k] + d_f32[k]) for k in one}


@functools.lru_cache(maxsize=None)
def case(key):
    net, x, e, w = nr.variant(**CASES[key])
    return (net, x, e, w) + bars_of(net, x, e, w)


@pytest.mark.parametrize("key", sorted(CASES))
def test_the_bar_is_sharp(key):
    net, x, e, w, want, bars = case(key)
    for drop in ("cross", "lo"):
        worst = max(fractions(split_pass(net, x, e, w, drop), want, bars).values())
        print("%s without %s: %.3g of the bar" % (key, drop, worst))
        assert worst > 3.0, (key, drop)


def test_the_switch_through_the_interface():
    import ctypes as C
    import rasr_amd
    from rasr_amd import _lib
    cfg = _lib.NnTrainCfg()
    _lib.lib().amx_nntrain_default_cfg(C.byref(cfg))
    assert cfg.gemm == 0 == _lib.AMX_NNTRAIN_GEMM_F32
    net = case("linear-T1")[0]
    tr = rasr_amd.FeedForwardTrainer(None, net.Ws, net.bs, net.acts, gemm="bf16x3")    # a host-only handle
    assert tr.accumulator_size() == nr.layout(net.dims, 7, 129, nr.BASE | nr.GRADIENT)["size"]
    with pytest.raises(Exception, match="gemm = 7"):
        rasr_amd.FeedForwardTrainer(None, net.Ws, net.bs, net.acts, gemm=7)


def run(ctx, net, x, e, w, gemm, mask=ALL):
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    tr = rasr_amd.FeedForwardTrainer(ctx, net.Ws, net.bs, net.acts, statistics=mask, error_signal_clip=net.clip, class_weights=net.class_weights,
                                     class_to_output=net.class_to_output, gemm=gemm)
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    tr.accumulate(x, e, acc, w)
    return acc.cpu().numpy(), tr


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(CASES))
def test_against_the_f64_evaluation(ctx, key):
    net, x, e, w, want, bars = case(key)
    got, tr = run(ctx, net, x, e, w, "bf16x3")
    assert np.array_equal(run(ctx, net, x, e, w, "bf16x3")[0].view(np.uint64), got.view(np.uint64))     # the same call, a fresh handle: the same bits
    s, f = tr.statistics(got), tr.statistics(run(ctx, net, x, e, w, "f32")[0])
    for k in ("n_observations", "total_weight", "class_counts", "feature_sum", "feature_square_sum"):       # no GEMM in their way: every bit
        assert np.array_equal(s[k], f[k]), (key, k)
    frac = fractions(s, want, bars)
    for k in sorted(frac):
        print("%s %s bar %.3g device %.3g of it" % (key, k, bars[k], frac[k]))
    assert max(frac.values()) <= 1.0, (key, frac)
    if nr.min_top2_gap_ulp(want["softmax"]) > GAP_ULP:
        assert s["n_classification_errors"] == want["n_classification_errors"], key


@pytest.mark.gpu
def test_a_chunk_is_one_chain_from_zero(ctx):
    """the whole call's gradient is the f32 sum, in ascending order, of what its 256-frame slices give alone"""
    net, x, e, w, *_ = case("wide-T513")
    whole, tr = run(ctx, net, x, e, w, "bf16x3", nr.GRADIENT)
    parts = [tr.statistics(run(ctx, net, x[t:t + 256], e[t:t + 256], w[t:t + 256], "bf16x3", nr.GRADIENT)[0]) for t in (0, 256, 512)]
    for k in ("gradient_weights", "gradient_bias"):
        total = functools.reduce(lambda a, b: (a + b).astype(F32), [p[k][0].astype(F32) for p in parts], np.zeros_like(parts[0][k][0], F32))
        assert np.array_equal(tr.statistics(whole)[k][0], total.astype(F64)), k


@pytest.mark.gpu
def test_a_segment_alone_and_in_a_batch(ctx):
    import rasr_amd
    import torch
    from tests import test_nnseq_gpu as sq
    net, off, feats, emission, *_ = sq.batch()
    tr, seq = sq.trainers(ctx, net, cls=functools.partial(rasr_amd.FeedForwardTrainer, gemm="bf16x3"))
    whole, _ = sq.run(seq, feats, off, emission, sq.flows()["mmi"])
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    for s in range(len(off) - 1):
        single, _ = sq.run(seq, feats, off, emission, sq.flows()["mmi"], objective=[F32(0.375) * (s + 1)], acc=acc, segments=[s])
    assert np.array_equal(single.view(np.uint64), whole.view(np.uint64)) and np.any(whole)
    assert not np.array_equal(whole, sq.run(sq.trainers(ctx, net)[1], feats, off, emission, sq.flows()["mmi"])[0])    # not the f32 kernels


@pytest.mark.gpu
def test_the_step_resplits_the_weight_images(ctx):
    import rasr_amd
    from tests.test_nnstep_gpu import read, upload
    net, x, e, w, _, bars = case("sigmoid-relu-T300")
    ctx.use_torch_stream()
    tr = rasr_amd.MiniBatchTrainer(ctx, net.Ws, net.bs, net.acts, error_signal_clip=net.clip, class_to_output=net.class_to_output, gemm="bf16x3")
    tr.set_estimator(learning_rate=2.0)
    cfg = ns.Cfg(len(net.Ws))
    cfg.eta = F32(2.0)
    for step in range(2):       # the second call's forward and backward read the planes of the stepped images
        tr.step_accumulate_dev(*upload(x, e, w))
        Ws, bs, Gs, gs = read(tr)
        here = nr.Net(Ws, bs, net.acts, class_to_output=net.class_to_output, clip=net.clip)
        want, bars = bars_of(here, x, e, w)
        frac = fractions({"objective": want["objective"], "gradient_weights": Gs, "gradient_bias": gs}, want, bars)
        print("step %d: worst %.3g of the bar" % (step, max(frac.values())))
        assert max(frac.values()) <= 1.0, (step, frac)
        stale = fractions(nr.accumulate(net, x, e, w, mask=nr.BASE | nr.GRADIENT), want, bars)
        assert step == 0 or max(stale.values()) > 3.0       # the unstepped weights' gradient is far outside: a stale plane would show
        tr.step_estimate_dev()
        W1, b1, _, _ = read(tr)
        Gf, gf, _ = ns.finalize(cfg, Gs, gs, [F32(0), F32(0)], int(tr.step_info()["n_observations"]))
        Wr, br, _ = ns.estimate(cfg, Ws, bs, Gf, gf)
        assert all(np.array_equal(a, b) for a, b in zip(W1 + b1, Wr + br))      # the update itself is the f32 step on the device's statistic
    tr.close()
