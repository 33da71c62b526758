"""The wide networks and long calls that tests/test_nn_wide.py (CPU) and tests/test_nn_wide_gpu.py (GPU) share: NN training statistics
(nntrain.hip) and the mini-batch step (nnstep.hip) on shapes where every 256-strided loop takes more than one trip, the 128-tile grids
are not square, a call holds three and more frame chunks and the network has one layer only.

Networks, kept out of nr.NETWORKS so that nr.gpu_cases(), ns.update_cases() and the two .npz fixtures stay what they are:
  W = 300-40-260-700   feature dimension above 256; 128-tile grids 3x1, 1x3 and 3x6; 700 outputs = three trips of the strided loops, the
                       last partly filled; layer 2 has 12 x 24 = 288 update tiles of 32 x 32 (those past the first 256 hold padding
                       alone: its 260 inputs end in tile row 8)
  D = 1030-1100        one layer (no backward GEMM, no clip), padded to 1152 x 1152: 324 norm segments of 4096, 1296 update tiles, five
                       trips over the outputs
  a = 24-40-33-50      nr.NETWORKS["a"], for one call of the documented cap alone
Frame counts: 513 (three chunks of 256, the third holding one frame), 768 (three full chunks), 1000 on D, 4096 = AMX_NNTRAIN_MAX_FRAMES
(sixteen chunks).

Labels.  On the plain cases every even frame's label is the f64 restatement's own arg-max, odd frames keep their random label: about
half the frames are correct, and one wrong arg-max moves the error count.  The option case keeps nr.variant's labels.

Conditions on the inputs, asserted by tests/test_nn_wide.py (conditions()): in every case the two largest softmax values of every frame
differ by at least 64 ulp (the bound tests/golden/make_nntrain_golden.py asserts), every pre-activation of a rectified unit keeps
4 x the largest distance between the two evaluations' pre-activations away from zero (a derivative that flips between two orders of a
sum moves a gradient by a whole frame's term, not by a rounding), and the f32 and f64 evaluations agree in error count and class counts.

Bars.  The rule of tests/golden/make_nntrain_golden.py and make_nnstep_golden.py, evaluated here instead of stored: per network and
block 4 x the distance between the restatement with f32 sums and with f64 sums, relative to the block's largest magnitude (objective,
step sizes: to the value), the worst over the network's cases.  Both evaluations run on the CPU; nothing comes from the device.
"""
import functools

import numpy as np

from tests import nnstep_reference as ns
from tests import nntrain_reference as nr

F32, F64 = np.float32, np.float64
ALL = nr.CLASS_COUNTS | nr.MEAN_AND_VARIANCE | nr.BASE | nr.GRADIENT
MAX_FRAMES = 4096     # AMX_NNTRAIN_MAX_FRAMES
FACTOR = 4.0

NETS = {"W": ([300, 40, 260, 700], (nr.SIGMOID, nr.RELU)), "D": ([1030, 1100], ()), "a": (nr.NETWORKS["a"], (nr.SIGMOID, nr.RELU))}
OPTIONS = dict(frame_weights=True, class_weights=True, disregard=True, pre=True, clip=0.02)
CASES = {
    "W-T513": dict(net="W", T=513, seed=88),
    "W-T768": dict(net="W", T=768, seed=88),
    "W-T4096": dict(net="W", T=4096, seed=77, acts=(nr.SIGMOID, nr.TANH)),     # a million rectified units would not all keep the margin below
    "D-T513": dict(net="D", T=513, seed=77),
    "D-T1000": dict(net="D", T=1000, seed=77),
    "a-T4096": dict(net="a", T=4096, seed=77),
    "W-T768-options": dict(net="W", T=768, seed=79, options=True),
}


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(key):
    """-> (Net, feats, emission, weights or None); the arrays are shared and read-only"""
    c = CASES[key]
    dims, acts = NETS[c["net"]]
    net, x, e, w = nr.variant(dims, c.get("acts", acts), c["T"], c["seed"], **(OPTIONS if c.get("options") else {}))
    if not c.get("options"):
        p = nr.accumulate(net, x, e, None, mask=nr.BASE, products="f64")["softmax"]
        e = e.copy()
        e[::2] = nr.arg_max(p)[::2].astype(e.dtype)
    frozen(x, e, w)
    return net, x, e, w


@functools.lru_cache(maxsize=None)
def evaluation(key, products="f64"):
    """the restatement's pass over a case, every block; shared, not to be written to"""
    net, x, e, w = case(key)
    return nr.accumulate(net, x, e, w, mask=ALL, products=products)


def rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    m = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / m) if m > 0 else 0.0


def blocks(stats, n_layers):
    """name -> array of every block that is held to a bar"""
    out = {"feature_sum": stats["feature_sum"], "feature_square_sum": stats["feature_square_sum"]}
    for l in range(n_layers):
        out["gradient_weights/%d" % l] = stats["gradient_weights"][l]
        out["gradient_bias/%d" % l] = stats["gradient_bias"][l]
    return out


def bars_between(a, b, n_layers):
    """block -> 4 x the distance of evaluation b (f32 sums) from evaluation a (f64 sums), relative to a's largest magnitude"""
    ba, bb = blocks(a, n_layers), blocks(b, n_layers)
    out = {k: FACTOR * rel(bb[k], ba[k]) for k in ba}
    out["objective"] = FACTOR * abs(b["objective"] - a["objective"]) / abs(a["objective"])
    assert all(v > 0 for v in out.values()), out
    return out


@functools.lru_cache(maxsize=None)
def network_bars(name):
    """make_nntrain_golden.py's rule: per network and block, the worst over the network's cases"""
    worst = {}
    for key in sorted(CASES):
        if CASES[key]["net"] == name:
            for block, v in bars_between(evaluation(key, "f64"), evaluation(key, "f32"), len(case(key)[0].Ws)).items():
                worst[block] = max(worst.get(block, 0.0), v)
    return worst


def bars(key):
    """block -> bar of a case: its network's"""
    return network_bars(CASES[key]["net"])


def leaves(got, want, bar):
    """does a block lie outside its bar"""
    want = np.asarray(want, F64)
    return bool(np.abs(np.asarray(got, F64) - want).max() > bar * np.abs(want).max())


def pre_activations(net, x, e, products):
    """[z of layer l for the kept frames], l below the top layer, as nr.accumulate forms them"""
    keep, _, _ = nr.labels(e, net.class_to_output, net.class_weights, None)
    h, out = nr.preprocess(np.asarray(x, F32)[keep], net.pre), []
    for l in range(len(net.Ws) - 1):
        z = (nr.matmul(h, net.Ws[l].T, products) + net.bs[l][None, :]).astype(F32)
        out.append(z)
        h = nr.activate(z, net.acts[l])
    return out


def layer_inputs(net, x, e, products="f64"):
    """[the input of layer l for the kept frames], every layer, as nr.accumulate forms them"""
    keep, _, _ = nr.labels(e, net.class_to_output, net.class_weights, None)
    out = [nr.preprocess(np.asarray(x, F32)[keep], net.pre)]
    for z, act in zip(pre_activations(net, x, e, products), net.acts):
        out.append(nr.activate(z, act))
    return out


def rectified_margin(net, x, e):
    """-> (the smallest |z| of a rectified unit / (4 x the largest |z_f32 - z_f64| of its layer), inf without such a unit; do the two
    evaluations open the same units)"""
    margin, same_gates = np.inf, True
    za, zb = pre_activations(net, x, e, "f64"), pre_activations(net, x, e, "f32")
    for l, act in enumerate(net.acts[:-1]):
        if act != nr.RELU:
            continue
        dist = float(np.abs(za[l].astype(F64) - zb[l]).max())
        margin = min(margin, float(np.abs(za[l]).min()) / (FACTOR * dist) if dist > 0 else np.inf)
        same_gates = same_gates and bool(np.array_equal(za[l] <= 0, zb[l] <= 0))
    return margin, same_gates


def conditions(key):
    """-> dict: min_top2_gap_ulp, rectified_margin, same_gates, same_counts (the module's docstring)"""
    net, x, e, w = case(key)
    a, b = evaluation(key, "f64"), evaluation(key, "f32")
    margin, same_gates = rectified_margin(net, x, e)
    return {"min_top2_gap_ulp": nr.min_top2_gap_ulp(a["softmax"]), "rectified_margin": margin, "same_gates": same_gates,
            "same_counts": a["n_classification_errors"] == b["n_classification_errors"] and np.array_equal(a["class_counts"], b["class_counts"])}


# ------------------------------------------------------------------------------------ ties on 700 outputs
TIE_PAIRS = ((300, 556), (600, 650), (5, 517))    # one thread on two trips; two waves of the third trip; trips 0 and 2
TIE_T = 130


def tie_network(carrier, vanish=None):
    """W with a top layer whose rows and biases are identical within every pair of TIE_PAIRS; the pair `carrier` holds every frame's
    maximum (a bias of +40).  vanish: an output whose bias is -200, so that exp() of it is 0 in f32"""
    dims, acts = NETS["W"]
    Ws, bs, a = nr.network(dims, acts, 5)
    for i, j in TIE_PAIRS:
        Ws[-1][j] = Ws[-1][i]
        bs[-1][j] = bs[-1][i]
    if carrier is not None:
        bs[-1][list(TIE_PAIRS[carrier])] = 40.0
    if vanish is not None:
        bs[-1][vanish] = -200.0
    x, _, _ = nr.frames(dims, TIE_T, 6)
    return nr.Net(Ws, bs, a), x


# ------------------------------------------------------------------------------------ the step
STEP_T = 513
STEP_CASES = {
    "W-l2-sgd": dict(net="W", seed=97, cfg=dict(learning_rate=0.125, bias_learning_rate=0.75, layer_learning_rate=[1.0, 0.5, 2.0], regularizer=ns.L2,
                                                estimator=ns.SGD, regularization_constant=[3e-3, 1e-3, 2e-3],
                                                statistics_smoothing=[ns.EXPONENTIAL_TRACE, ns.STAT_NONE, ns.NO_STATISTICS], trace_factor=[0.75, 0.5, 0.5])),
    "W-centered-clip": dict(net="W", seed=96, centered=True,
                            cfg=dict(learning_rate=0.125, bias_learning_rate=0.75, layer_learning_rate=[1.0, 0.5, 2.0], regularizer=ns.CENTERED_L2,
                                     estimator=ns.SGD_L1_CLIPPING, regularization_constant=[3e-3, 1e-3, 2e-3],
                                     statistics_smoothing=[ns.STAT_NONE, ns.EXPONENTIAL_TRACE, ns.NO_STATISTICS], trace_factor=[0.5, 0.75, 0.5])),
    "D-l1-clip": dict(net="D", seed=80, cfg=dict(learning_rate=0.125, bias_learning_rate=0.75, regularizer=ns.L1, estimator=ns.SGD_L1_CLIPPING,
                                                 regularization_constant=[2e-4])),
}


def step_case(key, sums="f64", T=STEP_T):
    """-> (ns.Trainer, feats, emission, weights) of one step case: a fresh restated trainer on the case's network"""
    c = STEP_CASES[key]
    dims, acts = NETS[c["net"]]
    net, x, e, w = nr.variant(dims, acts, T, c["seed"], frame_weights=True)
    kw = dict(c["cfg"])
    if c.get("centered"):
        Ws, bs, _ = nr.network(dims, acts, 7)
        kw["center"] = ([(m * F32(0.5)).astype(F32) for m in Ws], [(m * F32(0.5)).astype(F32) for m in bs])
    return ns.Trainer(net, ns.Cfg(len(net.Ws), **kw), sums), x, e, w


def regularizer_bar(cfg, Ws, bs, n, criterion, objective):
    """make_nnstep_golden.py's bar of the regulariser's objective as the tests form it (the group's objective minus its criterion part,
    both f32: half an ulp of the objective belongs to the figure)"""
    oa, ob = ns.regularizer_objective(cfg, Ws, bs, n, "f64"), ns.regularizer_objective(cfg, Ws, bs, n, "f32")
    formed = float(F32(F32(criterion) + ob)) - float(F32(criterion))
    return float(oa), FACTOR * (abs(formed - float(oa)) + 0.5 * float(np.spacing(F32(objective)))) / abs(float(oa))


def step_size_parts(cfg, l, G, g, sums):
    """stepSizes[l] of ns.estimate from the update terms G, g of a layer whose weights and bias are both updated"""
    rate = F32(cfg.eta * cfg.eta_l[l])
    bias_rate = F32(F32(cfg.eta * cfg.eta_bias) * cfg.eta_l[l])
    step = F32(F32(0) + F32(ns.asum(G, sums) * rate))
    return F32(step + F32(ns.asum(g, sums) * bias_rate))


def step_size_bar(cfg, l, G, g):
    s64, s32 = step_size_parts(cfg, l, G, g, "f64"), step_size_parts(cfg, l, G, g, "f32")
    return float(s64), FACTOR * abs(float(s32) - float(s64)) / abs(float(s64))


@functools.lru_cache(maxsize=None)
def step_bars(name):
    """make_nnstep_golden.py's rule: per network (and layer) the worst over the network's step cases of 4 x the distance between f32
    and f64 sums on the restatement's own f64 statistics -> {"regulariser objective", "step size/<l>", "bias term/<l>"}"""
    worst = {}

    def note(k, v):
        assert v > 0, k
        worst[k] = max(worst.get(k, 0.0), v)
    for key in sorted(STEP_CASES):
        if STEP_CASES[key]["net"] != name:
            continue
        a, x, e, w = step_case(key, "f64")
        a.step_accumulate(x, e, w)
        note("regulariser objective", regularizer_bar(a.cfg, a.net.Ws, a.net.bs, a.n_obs, a.criterion, a.objective)[1])
        G, g, _ = ns.finalize(a.cfg, a.G, a.g, [0.0], a.n_obs)
        finalized, means = [m.copy() for m in g], a.means()
        ns.estimate(a.cfg, a.net.Ws, a.net.bs, G, g, "f64", means=means)      # G, g become the update terms
        for l in range(a.L):
            note("step size/%d" % l, step_size_bar(a.cfg, l, G[l], g[l])[1])
            if means[l] is not None:
                note("bias term/%d" % l, FACTOR * rel(ns.delta_bias(G[l], finalized[l], means[l], "f32"), g[l]))
    return worst


def padded_transposed_image(W):
    """a layer's weights as the device holds them for the backward GEMM, the update and the norms: [Pin x Pout], zero padded to 128"""
    n, k = W.shape
    img = np.zeros(((k + 127) // 128 * 128, (n + 127) // 128 * 128), F32)
    img[:k, :n] = W.T
    return img
