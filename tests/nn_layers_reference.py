"""numpy f32 restatement of the NN layer types behind amx_ffnn_create_ex (include/amx.h), for the tests.

Every function reproduces the reference's f32 arithmetic element by element:
  * logarithm:  Nn/PreprocessingLayer.cc:40-74 -> Math::FastMatrix::log (Math/FastMatrix.hh:790-792) -> Math::vr_log
                (Math/FastVectorOperations.hh:86-90), the unqualified log on a float: ::log(double), narrowed to f32.
  * mean-and-variance-normalization: Nn/PreprocessingLayer.cc:86-177: addToAllColumns(mean, -1) (Math/FastMatrix.hh:1356-1361, axpy:
                x + (-1 * m), the product is exact) then divideRowsByScalars(stddev) (Math/FastMatrix.hh:1439-1444: scal by (f32)1 / s).
  * elu:        Nn/ActivationLayer.cc:331-396 -> Math::FastMatrix::elu (Math/FastMatrix.hh:1658-1667), alpha 1: x < 0 ? exp(x) - 1 : x
                with std::exp on a float (here the f64 exponential narrowed to f32: the correctly rounded expf).
  * maxoutvar:  Nn/ActivationLayer.cc:404-520 -> Math::FastMatrix::maxoutvar (Math/FastMatrix.hh:840-860): per group the first element,
                replaced only by a strictly greater later one.
The linear part of each layer comes from the oracle, one layer at a time (oracle_ffnn_forward(..., top=0)).
"""
import numpy as np

F32 = np.float32
LOGARITHM, MEAN_AND_VARIANCE = 1, 2   # AMX_NN_PRE_*
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_ELU = 0, 1, 2, 3, 4


def logarithm(x):
    """Math::vr_log: (float)::log((double)x)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(x, F32).astype(np.float64)).astype(F32)


def mean_and_variance(x, mean, stddev):
    """addToAllColumns(mean, -1), divideRowsByScalars(stddev): (x - m) * ((f32)1 / s)"""
    x = np.asarray(x, F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = (F32(1) / np.asarray(stddev, F32)).astype(F32)
        return ((x - np.asarray(mean, F32)).astype(F32) * r).astype(F32)


def preprocess(x, layers):
    """layers: [("logarithm",) | ("mean-and-variance-normalization", mean, stddev)] in order (the rasr_amd argument)"""
    for p in layers:
        p = (p,) if isinstance(p, str) else tuple(p)
        x = logarithm(x) if p[0] == "logarithm" else mean_and_variance(x, p[1], p[2])
    return x


def elu(x):
    """x < 0 ? expf(x) - 1 : x (a NaN stays NaN)"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = (np.exp(x.astype(np.float64)).astype(F32) - F32(1)).astype(F32)
    return np.where(x < 0, e, x).astype(F32)


def activate(x, act):
    """the chain's hidden activations; sigmoid / tanh only where the tests need them in f64 (bars, not bits)"""
    x = np.asarray(x, F32)
    if act == ACT_RELU:
        return np.where(x < 0, F32(0), x).astype(F32)
    if act == ACT_ELU:
        return elu(x)
    if act == ACT_SIGMOID:
        return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(F32)
    if act == ACT_TANH:
        return np.tanh(x.astype(np.float64)).astype(F32)
    return x


def group_sizes(n_out, spec):
    """maxout spec (G, or a list of group sizes) -> list of sizes"""
    if np.isscalar(spec):
        return [n_out // int(spec)] * int(spec)
    return [int(s) for s in spec]


def maxoutvar(x, sizes):
    """x [T, sum(sizes)] -> [T, len(sizes)]: the first element of each group, replaced only by a strictly greater later one"""
    x = np.asarray(x, F32)
    out = np.empty((x.shape[0], len(sizes)), F32)
    o = 0
    for g, s in enumerate(sizes):
        m = x[:, o].copy()
        for j in range(1, s):
            c = x[:, o + j]
            m = np.where(c > m, c, m)
        out[:, g] = m
        o += s
    return out


def compose(Ws, bs, acts, x, preprocessing=(), maxout=None, log_prior=None, prior_scale=1.0, acc64=2, hidden=False):
    """the scores -(W x + b - alpha log prior) of a network with preprocessing, ELU and maxout, layer by layer through the oracle
    (acc64: 2 = k-ordered fmaf chain, True = f64 accumulation).  hidden=True: the last hidden activation (forwardHiddenLayers)."""
    from oracle.binding import oracle_ffnn_forward
    maxout = dict(maxout or {})
    a = preprocess(np.asarray(x, F32), preprocessing)
    L = len(Ws)
    for l in range(L - 1):
        z = oracle_ffnn_forward([Ws[l]], [bs[l]], [0], a, top=0, acc64=acc64)
        a = activate(z, acts[l])
        if l in maxout:
            a = maxoutvar(a, group_sizes(Ws[l].shape[0], maxout[l]))
    if hidden:
        return a
    return -oracle_ffnn_forward([Ws[-1]], [bs[-1]], [0], a, top=0, log_prior=log_prior, prior_scale=prior_scale, acc64=acc64)
