"""Plain-numpy restatement of the NN training statistics pass (include/amx.h, "NN training statistics"): Nn::FeedForwardTrainer in batch
mode, Nn::MeanAndVarianceTrainer, Nn::Prior::setFromClassCounts and the Nn::Statistics<f32> file.

Element-wise steps follow the reference's roundings (file:line in include/amx.h); matrix products are taken in f64 (products="f64",
what the tests compare the device with) or in f32 through numpy's BLAS sgemm (products="f32", the arithmetic of the reference's own
Math::gemm<f32>; tests/golden/make_nntrain_golden.py measures the tests' bars as the distance between the two).  Frames of a disregarded
class are removed before anything else, as Nn/BufferedAlignedFeatureProcessor.cc:133-145 never buffers them.
"""
import struct

import numpy as np

F32 = np.float32
F64 = np.float64
FLT_MAX = np.finfo(np.float32).max
NONE, RELU, SIGMOID, TANH = 0, 1, 2, 3
CLASS_COUNTS, MEAN_AND_VARIANCE, BASE, GRADIENT = 1, 2, 4, 8
CHUNK = 256


# ------------------------------------------------------------------------------------ element-wise functions
def sigmoid_derivative(e, y):
    """elem *= X * (1.0 - X) (Math/FastMatrix.hh:1019-1025): a double product narrowed once"""
    return (e.astype(F64) * (y.astype(F64) * (1.0 - y.astype(F64)))).astype(F32)


def tanh_derivative(e, y):
    """elem *= 1.0 - X * X (:1027-1034): the square is an f32 product"""
    return (e.astype(F64) * (1.0 - (y * y).astype(F64))).astype(F32)


def rectified_derivative(e, y):
    """elem = 0 where X <= 0 (:1050-1057)"""
    return np.where(y <= 0, F32(0), e).astype(F32)


def clip(e, c):
    """elem > 0 ? std::min(elem, c) : std::max(elem, -c) (:1306-1311); a NaN stays"""
    c = F32(c)
    with np.errstate(invalid="ignore"):
        return np.where(e > 0, np.where(c < e, c, e), np.where(e < -c, -c, e)).astype(F32)


def arg_max(p):
    """FastMatrix::argMax per row (:899-909): the first strictly greater value from Core::Type<f32>::min; a NaN never wins"""
    with np.errstate(invalid="ignore"):
        masked = np.where(p > -FLT_MAX, p, -np.inf)
    return np.argmax(masked, axis=1)


def kronecker(p, label):
    """errorSignal = p, at(label) += -1.0 (:1061-1070)"""
    e = p.copy()
    e[np.arange(len(label)), label] = e[np.arange(len(label)), label] + F32(-1.0)
    return e


def objective_terms(p, label, w):
    """-(std::log(p[label])) * w per frame in f32 (:1105-1130)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (-logf(p[np.arange(len(label)), label]) * w.astype(F32)).astype(F32)


def logf(x):
    """std::log on a float: the f64 logarithm narrowed (numpy's own f32 logarithm is a vector routine of a few ulp)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(x, F32).astype(F64)).astype(F32)


def seq_sum_f32(a, axis):
    """the sequential f32 sum along axis (Math::FastVector::addSummedRows / addSummedColumns)"""
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), F32)
    return np.take(np.cumsum(a, axis=axis, dtype=F32), -1, axis=axis)


def activate(v, act):
    if act == RELU:
        return np.where(v < 0, F32(0), v).astype(F32)
    if act == SIGMOID:
        return (F32(1) / (F32(1) + np.exp(-v, dtype=F32))).astype(F32)
    if act == TANH:
        return np.tanh(v, dtype=F32)
    return v


def softmax(z):
    """Math::FastMatrix<f32>::softmax per frame (Math/FastMatrix.hh:818-834), as amx_ffnn_forward_dev(AMX_NN_TOP_SOFTMAX) states it"""
    m = z.max(axis=1)
    a = z + (F32(-1.0) * m)[:, None]
    e = np.exp(a.astype(F64)).astype(F32)
    r = F32(1.0) / seq_sum_f32(e, 1)
    return (e * r[:, None]).astype(F32)


def preprocess(x, pre):
    for p in pre or ():
        if p == "logarithm" or p[0] == "logarithm":
            with np.errstate(divide="ignore", invalid="ignore"):
                x = np.log(x.astype(F64)).astype(F32)
        else:
            mean, dev = np.asarray(p[1], F32), np.asarray(p[2], F32)
            x = ((x - mean[None, :]).astype(F32) * (F32(1.0) / dev)[None, :]).astype(F32)
    return x


def matmul(a, b, products):
    if products == "f64":
        return (a.astype(F64) @ b.astype(F64)).astype(F32)
    return np.matmul(a.astype(F32), b.astype(F32))


# ------------------------------------------------------------------------------------ the pass
class Net:
    def __init__(self, Ws, bs, acts, pre=None, class_to_output=None, class_weights=None, clip=None):
        self.Ws, self.bs, self.acts = [np.asarray(w, F32) for w in Ws], [np.asarray(b, F32) for b in bs], list(acts)
        self.pre, self.clip = pre, clip
        self.class_to_output = None if class_to_output is None else np.asarray(class_to_output, np.int64)
        self.n_outputs = self.Ws[-1].shape[0]
        self.class_weights = np.ones(self.n_outputs, F32) if class_weights is None else np.asarray(class_weights, F32)
        self.dims = [self.Ws[0].shape[1]] + [w.shape[0] for w in self.Ws]


def labels(emission, class_to_output, class_weights, weights):
    """(kept frames mask, output index of the kept frames, f32 weight of the kept frames)"""
    e = np.asarray(emission, np.int64)
    o = e if class_to_output is None else np.asarray(class_to_output, np.int64)[e]
    keep = o >= 0
    o = o[keep]
    w = np.asarray(class_weights, F32)[o]
    if weights is not None:
        w = (w.astype(F64) * np.asarray(weights, F64)[keep]).astype(F32)   # weights.at(i) *= alignment weight (f64), narrowed
    return keep, o, w


def accumulate(net, feats, emission, weights=None, mask=BASE | GRADIENT, products="f64"):
    """one call of amx_nntrain_accumulate_dev into zeros: a dict of the blocks (f64; gradients [in, out])"""
    feats = np.asarray(feats, F32)
    keep, o, w = labels(emission, net.class_to_output, net.class_weights, weights)
    x_raw = feats[keep]
    T, L = len(o), len(net.Ws)
    out = {"n_observations": int(T), "total_weight": float(np.abs(w).astype(F64).sum()), "n_classification_errors": 0, "objective": 0.0}
    if mask & CLASS_COUNTS:
        out["class_counts"] = np.bincount(o, minlength=net.n_outputs).astype(np.int64)
    if mask & MEAN_AND_VARIANCE:
        p1 = (x_raw * w[:, None]).astype(F32)
        p2 = ((x_raw * x_raw).astype(F32) * w[:, None]).astype(F32)
        if products == "f64":
            out["feature_sum"], out["feature_square_sum"] = p1.astype(F64).sum(0), p2.astype(F64).sum(0)
        else:
            out["feature_sum"], out["feature_square_sum"] = seq_sum_f32(p1, 0).astype(F64), seq_sum_f32(p2, 0).astype(F64)
    if not mask & (BASE | GRADIENT):
        return out
    X = [preprocess(x_raw, net.pre)]
    for l in range(L):
        z = (matmul(X[l], net.Ws[l].T, products) + net.bs[l][None, :]).astype(F32)
        if l < L - 1:
            X.append(activate(z, net.acts[l]))
    p = softmax(z)
    out["softmax"] = p
    if mask & BASE:
        out["n_classification_errors"] = int((arg_max(p) != o).sum())
        terms = objective_terms(p, o, w)
        out["objective"] = float(terms.astype(F64).sum()) if products == "f64" else float(seq_sum_f32(terms, 0))
    if not mask & GRADIENT:
        return out
    do_clip = net.clip is not None and net.clip < FLT_MAX
    E = [None] * L
    E[L - 1] = (kronecker(p, o) * w[:, None]).astype(F32)
    if do_clip and L > 1:
        E[L - 1] = clip(E[L - 1], net.clip)
    for l in range(L - 1, 0, -1):
        d = matmul(E[l], net.Ws[l], products)
        y, act = X[l], net.acts[l - 1]
        d = sigmoid_derivative(d, y) if act == SIGMOID else tanh_derivative(d, y) if act == TANH else rectified_derivative(d, y) if act == RELU else d
        if do_clip and l - 1 > 0:
            d = clip(d, net.clip)
        E[l - 1] = d
    out["error_signals"] = E
    if products == "f64":
        out["gradient_weights"] = [X[l].astype(F64).T @ E[l].astype(F64) for l in range(L)]
        out["gradient_bias"] = [E[l].astype(F64).sum(0) for l in range(L)]
    else:
        out["gradient_weights"] = [np.matmul(X[l].T, E[l]).astype(F64) for l in range(L)]
        out["gradient_bias"] = [seq_sum_f32(E[l], 0).astype(F64) for l in range(L)]
    return out


def objective_f64(Ws, bs, acts, x, o, w):
    """the cross-entropy objective of a network in f64 throughout (finite differences of it check accumulate's gradient)"""
    h = np.asarray(x, F64)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        h = h @ np.asarray(W, F64).T + np.asarray(b, F64)
        if l < len(Ws) - 1:
            a = acts[l]
            h = np.maximum(h, 0) if a == RELU else 1 / (1 + np.exp(-h)) if a == SIGMOID else np.tanh(h) if a == TANH else h
    h = h - h.max(axis=1, keepdims=True)
    logp = h - np.log(np.exp(h).sum(axis=1, keepdims=True))
    return float(-(logp[np.arange(len(o)), o] * np.asarray(w, F64)).sum())


# ------------------------------------------------------------------------------------ flat buffer, files, prior, mean and deviation
def layout(dims, feature_dim, n_outputs, mask):
    """offsets of amx_nntrain_layout: dict with gradient_weights / gradient_bias lists, feature_sum, feature_square_sum, class_counts, tail, size"""
    off, y = 0, {"gradient_weights": [], "gradient_bias": [], "feature_sum": -1, "feature_square_sum": -1, "class_counts": -1}
    if mask & GRADIENT:
        for i, n in zip(dims[:-1], dims[1:]):
            y["gradient_weights"].append(off)
            off += i * n
            y["gradient_bias"].append(off)
            off += n
    if mask & MEAN_AND_VARIANCE:
        y["feature_sum"], y["feature_square_sum"] = off, off + feature_dim
        off += 2 * feature_dim
    if mask & CLASS_COUNTS:
        y["class_counts"] = off
        off += n_outputs
    y["tail"], y["size"] = off, off + 4
    return y


def flat(stats, dims, feature_dim, n_outputs, mask):
    y = layout(dims, feature_dim, n_outputs, mask)
    a = np.zeros(y["size"], F64)
    if mask & GRADIENT:
        for l, (gw, gb) in enumerate(zip(stats["gradient_weights"], stats["gradient_bias"])):
            a[y["gradient_weights"][l]:y["gradient_weights"][l] + gw.size] = gw.reshape(-1)
            a[y["gradient_bias"][l]:y["gradient_bias"][l] + gb.size] = gb
    if mask & MEAN_AND_VARIANCE:
        a[y["feature_sum"]:y["feature_sum"] + feature_dim] = stats["feature_sum"]
        a[y["feature_square_sum"]:y["feature_square_sum"] + feature_dim] = stats["feature_square_sum"]
    if mask & CLASS_COUNTS:
        a[y["class_counts"]:y["class_counts"] + n_outputs] = stats["class_counts"]
    a[y["tail"]:] = [stats["n_observations"], stats["n_classification_errors"] if mask & BASE else 0, stats["total_weight"],
                     stats["objective"] if mask & BASE else 0.0]
    return a


def magic(mask, precision="S"):
    return ("NNSTAT" + ("C" if mask & CLASS_COUNTS else "#") + ("M" if mask & MEAN_AND_VARIANCE else "#") + ("B" if mask & BASE else "#") +
            ("G" if mask & GRADIENT else "#") + precision + "#####").encode()


def _vector(v):
    v = np.asarray(v, F64).astype("<f4")
    return struct.pack("<I", len(v)) + v.tobytes()


def statistics_bytes(a, dims, feature_dim, n_outputs, mask, version=2, precision="S"):
    """the Nn::Statistics<f32> file of a flat buffer (Nn/Statistics.cc:345-389,584-604)"""
    y = layout(dims, feature_dim, n_outputs, mask)
    t = y["tail"]
    b = magic(mask, precision) + struct.pack("<IIf", version, int(a[t]), F32(a[t + 2]))
    if mask & BASE:
        b += struct.pack("<If", int(a[t + 1]), F32(a[t + 3]))
    if mask & CLASS_COUNTS:
        c = a[y["class_counts"]:y["class_counts"] + n_outputs]
        seen = [(i, int(v)) for i, v in enumerate(c) if v > 0]
        b += struct.pack("<I", len(seen)) + b"".join(struct.pack("<II", i, v) for i, v in seen)
    if mask & MEAN_AND_VARIANCE:
        b += _vector(a[y["feature_sum"]:y["feature_sum"] + feature_dim]) + _vector(a[y["feature_square_sum"]:y["feature_square_sum"] + feature_dim])
    if mask & GRADIENT:
        b += struct.pack("<I", len(dims) - 1)
        for l, (i, n) in enumerate(zip(dims[:-1], dims[1:])):
            g = a[y["gradient_weights"][l]:y["gradient_weights"][l] + i * n].reshape(i, n)
            b += struct.pack("<IIII", 1, i, n, i) + b"".join(_vector(row) for row in g)
            b += _vector(a[y["gradient_bias"][l]:y["gradient_bias"][l] + n])
    return b


def narrowed(a, dims, feature_dim, n_outputs, mask):
    """the buffer as a file holds it and amx_nnstat_read gives it back: sums as f32, integers as u32"""
    y, r = layout(dims, feature_dim, n_outputs, mask), np.asarray(a, F64).astype(F32).astype(F64)
    t = y["tail"]
    r[t], r[t + 1] = int(a[t]), int(a[t + 1])
    if mask & CLASS_COUNTS:
        r[y["class_counts"]:y["class_counts"] + n_outputs] = a[y["class_counts"]:y["class_counts"] + n_outputs]
    if not mask & BASE:
        r[t + 1] = r[t + 3] = 0
    return r


def prior_from_class_counts(counts, class_weights, back_off_count):
    """Nn::Prior::setFromClassCounts (Nn/Prior.cc:128-156)"""
    v = np.maximum(np.asarray(counts, np.uint32), np.uint32(back_off_count)).astype(F32) * np.asarray(class_weights, F32)
    total = seq_sum_f32(v, 0)
    with np.errstate(divide="ignore"):
        return np.where(v == 0, -FLT_MAX, logf((v / total).astype(F32))).astype(F32)


def mean_and_deviation(feature_sum, feature_square_sum, total_weight):
    """Statistics<f32>::finalize + writeMeanAndStandardDeviation (Nn/Statistics.cc:146-173, Nn/NeuralNetworkTrainer.cc:447-462)"""
    a = F32(1.0 / F64(F32(total_weight)))
    mean = (np.asarray(feature_sum, F64).astype(F32) * a).astype(F32)
    sq = (np.asarray(feature_square_sum, F64).astype(F32) * a).astype(F32)
    with np.errstate(invalid="ignore"):
        return mean, np.sqrt((sq + (F32(-1.0) * (mean * mean).astype(F32))).astype(F32), dtype=F32)


# ------------------------------------------------------------------------------------ the cases the tests and the fixture share
NETWORKS = {"a": [24, 40, 33, 50], "b": [7, 130, 129]}
FRAMES = (1, 31, 127, 128, 129, 300)


def dims_of(name):
    """a key of NETWORKS, or the dimensions themselves (tests/nn_wide_cases.py keeps its networks out of NETWORKS)"""
    return NETWORKS[name] if isinstance(name, str) else [int(d) for d in name]


def network(name, acts, seed):
    """weights N(0, 1 / in) and small biases; acts: the hidden activations"""
    dims = dims_of(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    Ws = [(rng.standard_normal((n, i)) / np.sqrt(i) * 1.5).astype(F32) for i, n in zip(dims[:-1], dims[1:])]
    bs = [(rng.standard_normal(n) * 0.1).astype(F32) for n in dims[1:]]
    return Ws, bs, list(acts) + [NONE]


def frames(dims, T, seed, n_classes=None, positive=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal((T, dims[0])) * 1.2 + 0.1).astype(F32)
    if positive:
        x = (np.abs(x) + F32(0.05)).astype(F32)
    e = rng.integers(0, n_classes or dims[-1], T).astype(np.uint32)
    w = rng.uniform(0.25, 2.0, T)
    return x, e, w


def variant(name, acts, T, seed, frame_weights=False, class_weights=False, disregard=False, pre=False, clip=None):
    """(Net, feats, emission, weights): one configuration of the GPU tests"""
    dims = dims_of(name)
    Ws, bs, a = network(name, acts, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    c2o, n_classes = None, dims[-1]
    if disregard:   # two extra classes, dropped, in the middle of the class numbering (Nn::ClassLabelWrapper with disregard-classes)
        n_classes = dims[-1] + 2
        c2o = np.full(n_classes, -1, np.int64)
        c2o[[c for c in range(n_classes) if c not in (3, 11)]] = np.arange(dims[-1])
    cw = rng.uniform(0.5, 1.5, dims[-1]).astype(F32) if class_weights else None
    p = None
    if pre:
        p = ["logarithm", ("mean-and-variance-normalization", rng.uniform(-0.5, 0.5, dims[0]).astype(F32), rng.uniform(0.5, 2.0, dims[0]).astype(F32))]
    x, e, w = frames(dims, T, seed + 1, n_classes, positive=pre)
    if disregard and T > 2:
        e[T // 2] = 3
    return Net(Ws, bs, a, pre=p, class_to_output=c2o, class_weights=cw, clip=clip), x, e, (w if frame_weights else None)


def gpu_cases():
    """name -> keyword arguments of variant(): every hidden activation, with and without each option, at every frame count"""
    cases = {}
    acts_of = {"a": [(SIGMOID, RELU), (TANH, SIGMOID), (RELU, NONE)], "b": [(TANH,), (SIGMOID,), (RELU,), (NONE,)]}
    i = 0
    for name in ("a", "b"):
        for acts in acts_of[name]:
            for k, T in enumerate(FRAMES):
                plain = dict(name=name, acts=acts, T=T, seed=1000 + i)
                cases["%s-%s-T%d" % (name, "".join(str(c) for c in acts), T)] = plain
                # the options rotate over the frame counts, and one case per activation set carries them all
                opt = [dict(frame_weights=True), dict(class_weights=True), dict(disregard=True), dict(pre=True), dict(clip=0.01),
                       dict(frame_weights=True, class_weights=True, disregard=True, pre=True, clip=0.02)][k]
                cases["%s-%s-T%d-%s" % (name, "".join(str(c) for c in acts), T, "+".join(sorted(opt)))] = dict(plain, **opt)
                i += 1
    return cases


def min_top2_gap_ulp(p):
    """the smallest distance, in ulp of the larger value, between a frame's two largest softmax values"""
    if p.shape[1] < 2 or len(p) == 0:
        return np.inf
    s = np.sort(p, axis=1)
    return float(((s[:, -1] - s[:, -2]) / np.spacing(s[:, -1])).min())
