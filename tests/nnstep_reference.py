"""Plain-numpy restatement of NN mini-batch training (include/amx.h, "NN mini-batch training"): Nn::FeedForwardTrainer with batch-mode =
false -- the regulariser on the objective and on the gradient, Statistics::finalize, the estimator's step, accumulate-multiple-batches --
and Nn::BatchEstimator, on top of the statistics pass of tests/nntrain_reference.py.

Element-wise steps follow the reference's BLAS calls: saxpy is one fused multiply-add per element, sscal one product.  The fused
multiply-add is libm's fmaf through ctypes (exact; a route through f64 rounds twice).  Sums whose order BLAS leaves open (asum, dot, the
matrix products of the pass) are taken in f64 (sums="f64", what the tests compare the device with) or sequentially in f32 / by numpy's
sgemm (sums="f32"); tests/golden/make_nnstep_golden.py measures the tests' bars as the distance between the two.
"""
import ctypes
import ctypes.util

import numpy as np

from tests import nntrain_reference as nr

F32, F64 = np.float32, np.float64
NONE, L1, L2, CENTERED_L2 = 0, 1, 2, 3
SGD, SGD_L1_CLIPPING = 0, 1
NO_STATISTICS, STAT_NONE, EXPONENTIAL_TRACE = 0, 1, 2
CONTRACT_OFF, CONTRACT_FMA = 0, 1

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
_fmaf = np.frompyfunc(_libm.fmaf, 3, 1)


def fma(a, x, y):
    """fmaf(a, x, y) element-wise with broadcasting, f32"""
    a, x, y = np.broadcast_arrays(np.asarray(a, F32), np.asarray(x, F32), np.asarray(y, F32))
    if a.size == 0:
        return np.zeros(a.shape, F32)
    return np.asarray(_fmaf(a, x, y), dtype=object).astype(F32).reshape(a.shape)


def axpy(alpha, x, y):
    """y + alpha * x as saxpy computes it: one fused multiply-add per element"""
    return fma(F32(alpha), x, y)


def scal(alpha, x):
    """sscal: one product per element"""
    return (np.asarray(x, F32) * F32(alpha)).astype(F32)


def sign(w):
    """Math/CudaMatrixKernels.cu:897-902: in == 0 ? 0 : copysignf(1.0, in)"""
    w = np.asarray(w, F32)
    return np.where(w == 0, F32(0), np.copysign(F32(1), w)).astype(F32)


def l1_clip(w, v):
    """FastMatrix::l1clipping (Math/FastMatrix.hh:1291-1303): > 0: max(0, w - v); < 0: min(0, w + v); a zero of either sign stays"""
    w, v = np.asarray(w, F32), F32(v)
    down, up = (w - v).astype(F32), (w + v).astype(F32)
    pos = np.where(F32(0) < down, down, F32(0))       # std::max((T)0.0, t) = (0 < t) ? t : 0
    neg = np.where(up < F32(0), up, F32(0))           # std::min((T)0.0, t) = (t < 0) ? t : 0
    return np.where(w > 0, pos, np.where(w < 0, neg, w)).astype(F32)


def asum(x, sums):
    a = np.abs(np.asarray(x, F32)).reshape(-1)
    return F32(a.astype(F64).sum()) if sums == "f64" else F32(nr.seq_sum_f32(a, 0))


def dot(x, sums):
    x = np.asarray(x, F32).reshape(-1)
    return F32((x.astype(F64) * x.astype(F64)).sum()) if sums == "f64" else F32(nr.seq_sum_f32((x * x).astype(F32), 0))


class Cfg:
    """amx_nnstep_cfg"""

    def __init__(self, n_layers, learning_rate=1.0, bias_learning_rate=1.0, layer_learning_rate=None, regularization_constant=None, trainable=None,
                 regularizer=NONE, center=None, estimator=SGD, accumulate_multiple_batches=1, normalize_by_observations=True, log_step_size=True,
                 update_input_layer_weights=True, statistics_smoothing=None, trace_factor=None, initial_activations=None, input_smoothing=NO_STATISTICS,
                 input_trace_factor=0.5, input_initial_activations=None):
        # activation statistics by the layer they feed: index 0 the last preprocessing layer, index l the output of layer l - 1
        smoothing = [NO_STATISTICS] * n_layers if statistics_smoothing is None else list(statistics_smoothing)
        factors = [0.5] * n_layers if trace_factor is None else list(trace_factor)
        initial = [None] * n_layers if initial_activations is None else list(initial_activations)
        self.stat_mode = [input_smoothing] + smoothing[:-1]
        self.stat_f = [F32(input_trace_factor)] + [F32(f) for f in factors[:-1]]
        self.stat_initial = [input_initial_activations] + initial[:-1]
        self.eta, self.eta_bias = F32(learning_rate), F32(bias_learning_rate)
        self.eta_l = np.ones(n_layers, F32) if layer_learning_rate is None else np.asarray(layer_learning_rate, F32)
        self.c = np.zeros(n_layers, F32) if regularization_constant is None else np.asarray(regularization_constant, F32)
        self.trainable = [True] * n_layers if trainable is None else [bool(t) for t in trainable]
        self.regularizer, self.estimator, self.A = regularizer, estimator, int(accumulate_multiple_batches)
        self.center = None if center is None else ([np.asarray(w, F32) for w in center[0]], [np.asarray(b, F32) for b in center[1]])
        self.normalize, self.log_step_size, self.update_input = bool(normalize_by_observations), bool(log_step_size), bool(update_input_layer_weights)

    def regularized(self, l):
        return self.regularizer != NONE and self.trainable[l] and self.c[l] > 0


def regularizer_objective(cfg, Ws, bs, T, sums):
    """regularizer.objectiveFunction(network, (f32)T) (Nn/Regularizer.cc:74-94,129-149,182-212), every step in f32"""
    obj = F32(0)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        if not cfg.regularized(l):
            continue
        if cfg.regularizer == L1:
            tmp = asum(b, sums)
            tmp = F32(tmp + asum(W, sums))
            tmp = F32(tmp * cfg.c[l])
        else:
            if cfg.regularizer == CENTERED_L2:
                b, W = axpy(-1.0, cfg.center[1][l], b), axpy(-1.0, cfg.center[0][l], W)
            tmp = dot(b, sums)
            tmp = F32(tmp + dot(W, sums))
            tmp = F32(F64(tmp) * (F64(cfg.c[l]) / 2.0))
        obj = F32(obj + tmp)
    return F32(F32(T) * obj)


def add_gradient(cfg, Ws, bs, Gs, gs, n_observations):
    """regularizer.addGradient(network, statistics, (f32)nObservations) (:97-119,152-165,215-234); Gs[l] is [in, out]"""
    Gs, gs = [G.copy() for G in Gs], [g.copy() for g in gs]
    for l in range(len(Ws)):
        if not cfg.regularized(l):
            continue
        cf = F32(cfg.c[l] * F32(n_observations))
        if cfg.regularizer == L1:
            Gs[l], gs[l] = axpy(cf, sign(Ws[l]).T, Gs[l]), axpy(cf, sign(bs[l]), gs[l])
        else:
            Gs[l], gs[l] = axpy(cf, Ws[l].T, Gs[l]), axpy(cf, bs[l], gs[l])
            if cfg.regularizer == CENTERED_L2:
                Gs[l], gs[l] = axpy(-cf, cfg.center[0][l].T, Gs[l]), axpy(-cf, cfg.center[1][l], gs[l])
    return Gs, gs


def finalize(cfg, Gs, gs, objective, n_observations, normalize=None):
    """Statistics::finalize (Nn/Statistics.cc:146-161)"""
    weight = F32(n_observations) if (cfg.normalize if normalize is None else normalize) else F32(1)
    if weight == 1 or weight == 0:
        return [G.copy() for G in Gs], [g.copy() for g in gs], [F32(o) for o in objective]
    s = F32(1.0 / F64(weight))
    return [scal(s, G) for G in Gs], [scal(s, g) for g in gs], [F32(F64(F32(o)) * (1.0 / F64(weight))) for o in objective]


class ActStat:
    """a layer's activation statistics (Nn/NeuralNetworkLayer.cc:189-334)"""

    def __init__(self, mode, f, n, initial=None):
        self.mode, self.f, self.n = mode, F32(f), n
        self.initial = None if initial is None else (np.asarray(initial[0], F32), np.asarray(initial[1], F32))
        self.sum, self.sumsq, self.nobs, self.need_init = np.zeros(n, F32), np.zeros(n, F32), 0, True

    @staticmethod
    def chain(acc, Y, frame_index, scale, square, contract, single_chain=False):
        """at(row) += scale * m [* m] over the frames ascending (Math/FastVector.hh:461-478): the chain over the call's first 256 frames
        starts from acc, every further chunk's from zero, chunk totals added ascending (single_chain: the reference's one chain)"""
        scale, total, part, chunk = F32(scale), acc.astype(F32), acc.astype(F32), 0
        for y, t in zip(Y, frame_index):
            c = 0 if single_chain else int(t) // nr.CHUNK
            if c != chunk:
                total = part if chunk == 0 else (total + part).astype(F32)
                part, chunk = np.zeros_like(acc), c
            a = (scale * y).astype(F32) if square else np.full_like(y, scale)
            part = fma(a, y, part) if contract == CONTRACT_FMA else (part + (a * y).astype(F32)).astype(F32)
        return part if chunk == 0 else (total + part).astype(F32)

    def update(self, Y, frame_index, contract=CONTRACT_FMA, single_chain=False):
        """finalizeForwarding on the output Y [T, n] of the frames that entered the batch (frame_index: their positions in the call)"""
        T = len(Y)
        if T == 0:
            return
        ch = lambda acc, scale, square: self.chain(acc, Y, frame_index, scale, square, contract, single_chain)   # noqa: E731
        trace = self.mode == EXPONENTIAL_TRACE
        if self.need_init:
            self.need_init = False
            if self.initial is not None:
                n0 = 1 if trace else T
                m, d = self.initial
                self.sum = (m * F32(n0)).astype(F32)
                self.sumsq = (((d * d).astype(F32) + (m * m).astype(F32)).astype(F32) * F32(n0)).astype(F32)
                self.nobs = n0
            elif trace:
                self.sum = ch(self.sum, F32(1.0) / F32(T), False)
                self.sumsq = ch(self.sumsq, F32(1.0 / F64(T)), True)
        if trace:
            scale = (F32(1.0) - self.f) / F32(T)
            self.sum = ch((self.f * self.sum).astype(F32), scale, False)
            self.sumsq = ch((self.f * self.sumsq).astype(F32), scale, True)
        else:
            self.sum, self.sumsq = ch(self.sum, 1.0, False), ch(self.sumsq, 1.0, True)
            self.nobs += T

    def _a(self):
        return F32(1.0 / F64(1 if self.mode == EXPONENTIAL_TRACE else self.nobs))

    def mean(self):
        return fma(self._a(), self.sum, np.zeros(self.n, F32))

    def variance(self):
        v = self.mean()
        v = (v * v).astype(F32)
        v = (F32(-1.0) * v).astype(F32)
        v = fma(self._a(), self.sumsq, v)
        return ((F32(1.0) * v).astype(F32) + F32(0.0)).astype(F32)


def delta_bias(G, g, m, sums):
    """gradientWeights.multiply(mean, gradientBias, transposed, -1, 1): g - G^T m (sgemv; the order of the sum is the BLAS's)"""
    if sums == "f64":
        return (g.astype(F64) - G.T.astype(F64) @ m.astype(F64)).astype(F32)
    return (g - nr.seq_sum_f32((G * m[:, None]).astype(F32), 0)).astype(F32)


def estimate(cfg, Ws, bs, Gs, gs, sums="f64", has_preprocessing=False, means=None):
    """MeanNormalizedSgd::estimate and MeanNormalizedSgdL1Clipping::estimate (Nn/MeanNormalizedSgdEstimator.cc:51-126,136-153)
    -> (Ws, bs, step sizes); Gs and gs are replaced IN PLACE by the update terms, as the reference replaces the gradient.  means[l]:
    the activation mean of what feeds layer l, None where that keeps no statistics"""
    Ws, bs, steps = [W.copy() for W in Ws], [b.copy() for b in bs], np.zeros(len(Ws), F32)
    means = [None] * len(Ws) if means is None else means
    for l in range(len(Ws)):
        if not cfg.trainable[l]:
            continue
        rate = F32(cfg.eta * cfg.eta_l[l])
        bias_rate = F32(F32(cfg.eta * cfg.eta_bias) * cfg.eta_l[l])
        step = F32(0)
        if l > 0 or has_preprocessing or cfg.update_input:      # the loop over input streams runs to nPredecessors()
            if means[l] is not None:    # addOuterProduct(mean, gradientBias, -1): sger, A[i][j] = fmaf(x[i], round(alpha * y[j]), A[i][j])
                Gs[l] = fma(means[l][:, None], (-gs[l])[None, :], Gs[l])
            Ws[l] = axpy(-rate, Gs[l].T, Ws[l])
            step = F32(step + F32(asum(Gs[l], sums) * rate))
            if means[l] is not None:
                gs[l] = delta_bias(Gs[l], gs[l], means[l], sums)
        bs[l] = axpy(-bias_rate, gs[l], bs[l])
        step = F32(step + F32(asum(gs[l], sums) * bias_rate))
        if cfg.log_step_size:
            steps[l] = step
    if cfg.estimator == SGD_L1_CLIPPING:
        for l in range(len(Ws)):
            if cfg.trainable[l]:
                v = F32(F32(cfg.c[l] * cfg.eta) * cfg.eta_l[l])
                Ws[l], bs[l] = l1_clip(Ws[l], v), l1_clip(bs[l], v)
    return Ws, bs, steps


class Trainer:
    """the handle's state: the network, the group's f32 statistics, the mini-batch counter"""

    def __init__(self, net, cfg, sums="f64"):
        self.net, self.cfg, self.sums, self.n = net, cfg, sums, 0
        self.L = len(net.Ws)
        self._reset()
        self.steps, self.updated = np.zeros(self.L, F32), False
        self.contract = CONTRACT_FMA
        self.stats = [None if m == NO_STATISTICS else ActStat(m, f, net.dims[p], ini)
                      for p, (m, f, ini) in enumerate(zip(cfg.stat_mode, cfg.stat_f, cfg.stat_initial))]

    def _reset(self):
        d = self.net.dims
        self.G = [np.zeros((i, o), F32) for i, o in zip(d[:-1], d[1:])]
        self.g = [np.zeros(o, F32) for o in d[1:]]
        self.n_obs = self.n_err = 0
        self.total_weight = self.objective = self.criterion = F32(0)
        self.finalized = False

    def step_accumulate(self, feats, emission, weights=None):
        cfg = self.cfg
        if self.n % cfg.A == 0:
            self._reset()
        self.n += 1
        s = nr.accumulate(self.net, feats, emission, weights, mask=nr.BASE | nr.GRADIENT, products=self.sums)
        T = s["n_observations"]
        self.n_obs += T
        self.n_err += s["n_classification_errors"]
        self.total_weight = F32(self.total_weight + F32(s["total_weight"]))
        crit = F32(s["objective"])
        reg = regularizer_objective(cfg, self.net.Ws, self.net.bs, T, self.sums)
        self.objective = F32(F32(self.objective + crit) + reg)
        self.criterion = F32(self.criterion + crit)
        self.G = [(G + gw.astype(F32)).astype(F32) for G, gw in zip(self.G, s["gradient_weights"])]
        self.g = [(g + gb.astype(F32)).astype(F32) for g, gb in zip(self.g, s["gradient_bias"])]
        self.G, self.g = add_gradient(cfg, self.net.Ws, self.net.bs, self.G, self.g, self.n_obs)
        self.updated = False
        if any(st is not None for st in self.stats):
            keep, frame_index = self.layer_inputs(feats, emission)
            for st, X in zip(self.stats, keep):
                if st is not None:
                    st.update(X, frame_index, self.contract)
        return s

    def layer_inputs(self, feats, emission):
        """(the input of every layer for the frames that entered the batch, their positions in the call): the forward pass of
        tests/nntrain_reference.py's accumulate, step by step the same"""
        net = self.net
        keep, _, _ = nr.labels(emission, net.class_to_output, net.class_weights, None)
        X = [nr.preprocess(np.asarray(feats, F32)[keep], net.pre)]
        for l in range(self.L - 1):
            z = (nr.matmul(X[l], net.Ws[l].T, self.sums) + net.bs[l][None, :]).astype(F32)
            X.append(nr.activate(z, net.acts[l]))
        return X, np.nonzero(keep)[0]

    def means(self):
        return [None if st is None else st.mean() for st in self.stats]

    def step_estimate(self, normalize=None):
        if not self.finalized:
            self.G, self.g, (self.objective, self.criterion) = finalize(self.cfg, self.G, self.g, [self.objective, self.criterion], self.n_obs, normalize)
            self.finalized = True
        self.net.Ws, self.net.bs, self.steps = estimate(self.cfg, self.net.Ws, self.net.bs, self.G, self.g, self.sums, bool(self.net.pre), self.means())
        self.updated = True

    def step(self, feats, emission, weights=None):
        self.step_accumulate(feats, emission, weights)
        if self.n % self.cfg.A == 0:
            self.step_estimate()
        return self.info()

    def batch_estimate(self, a):
        """Nn::BatchEstimator (Nn/BatchEstimator.cc:50-101) on a flat f64 buffer of the BASE | GRADIENT layout"""
        d, mask = self.net.dims, nr.BASE | nr.GRADIENT
        y = nr.layout(d, d[0], d[-1], mask)
        r = nr.narrowed(a, d, d[0], d[-1], mask)
        self._reset()
        for l, (i, o) in enumerate(zip(d[:-1], d[1:])):
            self.G[l] = r[y["gradient_weights"][l]:y["gradient_weights"][l] + i * o].reshape(i, o).astype(F32)
            self.g[l] = r[y["gradient_bias"][l]:y["gradient_bias"][l] + o].astype(F32)
        t = y["tail"]
        self.n_obs, self.n_err, self.total_weight = int(r[t]), int(r[t + 1]), F32(r[t + 2])
        self.criterion = F32(r[t + 3])
        self.objective = F32(self.criterion + regularizer_objective(self.cfg, self.net.Ws, self.net.bs, self.n_obs, self.sums))
        self.G, self.g = add_gradient(self.cfg, self.net.Ws, self.net.bs, self.G, self.g, self.n_obs)
        self.step_estimate(normalize=True)
        return self.info()

    def info(self):
        return {"minibatch": self.n, "updated": self.updated, "n_observations": self.n_obs, "n_classification_errors": self.n_err,
                "total_weight": float(self.total_weight), "objective": float(self.objective), "criterion_objective": float(self.criterion),
                "step_size": self.steps.copy()}


# ------------------------------------------------------------------------------------ the cases the tests and the fixture share
def teacher_frames(dims, T, seed):
    """frames whose class is a fixed random linear function of the features: an objective that ten steps can lower"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal((T, dims[0])) * 1.2 + 0.1).astype(F32)
    R = np.random.Generator(np.random.PCG64(4242 + dims[0])).standard_normal((dims[0], dims[-1]))
    e = np.argmax(x.astype(F64) @ R, axis=1).astype(np.uint32)
    w = rng.uniform(0.5, 1.5, T)
    return x, e, w


def center_of(name, acts):
    Ws, bs, _ = nr.network(name, acts, 7)
    return [(w * F32(0.5)).astype(F32) for w in Ws], [(b * F32(0.5)).astype(F32) for b in bs]


TRAJECTORY_STEPS = (1, 2, 10)
TRAJECTORIES = {
    "a-rectified-l2": dict(name="a", acts=(nr.RELU, nr.RELU), seed=31, T=129, weights=False,
                           cfg=dict(learning_rate=0.25, bias_learning_rate=0.5, regularizer=L2, regularization_constant=[1e-3, 2e-3, 1e-3])),
    "b-sigmoid-l1clip-A2": dict(name="b", acts=(nr.SIGMOID,), seed=32, T=129, weights=True,
                                cfg=dict(learning_rate=0.5, layer_learning_rate=[1.0, 0.5], regularizer=L1, regularization_constant=[2e-4, 1e-4],
                                         estimator=SGD_L1_CLIPPING, accumulate_multiple_batches=2,
                                         statistics_smoothing=[EXPONENTIAL_TRACE, NO_STATISTICS], trace_factor=[0.75, 0.5])),
    "a-tanh-centered": dict(name="a", acts=(nr.TANH, nr.TANH), seed=33, T=300, weights=True,
                            cfg=dict(learning_rate=0.25, regularizer=CENTERED_L2, regularization_constant=[1e-3, 0.0, 1e-3], trainable=[1, 1, 1],
                                     normalize_by_observations=True, statistics_smoothing=[STAT_NONE, STAT_NONE, NO_STATISTICS]), centered=True),
}


def trajectory(key, sums="f64"):
    """-> (Trainer, batches): the case's fresh trainer and the batches of its update steps (A mini-batches each)"""
    k = TRAJECTORIES[key]
    Ws, bs, acts = nr.network(k["name"], k["acts"], k["seed"])
    net = nr.Net(Ws, bs, acts)
    kw = dict(k["cfg"])
    if k.get("centered"):
        kw["center"] = center_of(k["name"], k["acts"])
    cfg = Cfg(len(Ws), **kw)
    n = max(TRAJECTORY_STEPS) * cfg.A
    batches = []
    for i in range(n):
        x, e, w = teacher_frames(net.dims, k["T"], 1000 * k["seed"] + i)
        batches.append((x, e, w if k["weights"] else None))
    return Trainer(net, cfg, sums), batches


UPDATE_NETS = {"a": (nr.SIGMOID, nr.RELU), "b": (nr.TANH,)}
UPDATE_T = 129


def update_cases():
    """name -> (network name, Cfg keyword arguments): every estimator x regulariser on both networks, one mini-batch of UPDATE_T frames"""
    cases = {}
    for name in UPDATE_NETS:
        L = len(nr.NETWORKS[name]) - 1
        for reg, rname in ((NONE, "none"), (L1, "l1"), (L2, "l2"), (CENTERED_L2, "centered")):
            for est, ename in ((SGD, "sgd"), (SGD_L1_CLIPPING, "clip")):
                kw = dict(learning_rate=0.125, bias_learning_rate=0.75, layer_learning_rate=[1.0, 0.5, 2.0][:L], regularizer=reg, estimator=est,
                          regularization_constant=[3e-3, 1e-3, 2e-3][:L])
                cases["%s-%s-%s" % (name, rname, ename)] = (name, kw)
    return cases


def update_case(key, sums="f64"):
    """-> (Trainer, feats, emission, weights) of one update case"""
    name, kw = update_cases()[key]
    net, x, e, w = nr.variant(name, UPDATE_NETS[name], UPDATE_T, 500 + sorted(update_cases()).index(key), frame_weights=True)
    kw = dict(kw)
    if kw["regularizer"] == CENTERED_L2:
        kw["center"] = center_of(name, UPDATE_NETS[name])
    return Trainer(net, Cfg(len(net.Ws), **kw), sums), x, e, w


def stat_cases():
    """name -> (network name, Cfg keyword arguments): both estimators with each smoothing method on every hidden layer (L2, one mini-batch)"""
    cases = {}
    for name in UPDATE_NETS:
        L = len(nr.NETWORKS[name]) - 1
        for mode, mname in ((STAT_NONE, "none"), (EXPONENTIAL_TRACE, "trace")):
            for est, ename in ((SGD, "sgd"), (SGD_L1_CLIPPING, "clip")):
                kw = dict(learning_rate=0.125, bias_learning_rate=0.75, layer_learning_rate=[1.0, 0.5, 2.0][:L], regularizer=L2, estimator=est,
                          regularization_constant=[3e-3, 1e-3, 2e-3][:L], statistics_smoothing=[mode] * (L - 1) + [NO_STATISTICS], trace_factor=[0.75] * L)
                cases["%s-%s-%s" % (name, mname, ename)] = (name, kw)
    return cases


def stat_case(key, sums="f64", T=UPDATE_T):
    name, kw = stat_cases()[key]
    net, x, e, w = nr.variant(name, UPDATE_NETS[name], T, 900 + sorted(stat_cases()).index(key), frame_weights=True)
    return Trainer(net, Cfg(len(net.Ws), **kw), sums), x, e, w
