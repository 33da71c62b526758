"""GPU tests of the NN layer types behind amx_ffnn_create_ex (include/amx.h): preprocessing layers fused into the input pack kernels,
the ELU activation in every GEMM epilogue, and maxoutvar behind hidden layers, in every precision, against compositions of the
oracle's linear layers with the numpy restatement of tests/nn_layers_reference.py."""
import json
import os

import numpy as np
import pytest

from tests import nn_layers_reference as ref
from tests import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PRECISIONS = ("fp32", "bf16", "bf16x3", "f16mx")
TILES = {"bf16": ("0", "3", "6", "4", "2"), "bf16x3": ("0", "3", "6", "4", "2"),
         "f16mx": ("0", "3", "6", "2", "4", "5", "7", "8", "9", "11", "12", "14")}
MVN = "mean-and-variance-normalization"


def feats(T, dim, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((T, dim)).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def meets_bar(precision, got, want):
    """the bar of the existing tests: 1e-4 |ref| + 1e-4 with the same arg-min (fp32, bf16x3, f16mx); bf16: max error below 5e-2 of
    the mean score magnitude (tests/test_ffnn_gpu.py::test_bf16_path_accuracy)"""
    if precision == "bf16":
        return np.abs(got - want).max() < 5e-2 * np.abs(want).mean()
    return bool(np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-4)) and np.array_equal(got.argmin(axis=1), want.argmin(axis=1))


def scorer(ctx, net, precision, pre=None, maxout=None, tuning=None):
    import rasr_amd
    Ws, bs, acts, logp = net
    return rasr_amd.NnBatchFeatureScorer(ctx, Ws, bs, acts, log_prior=logp, precision=precision, tuning=tuning,
                                         preprocessing=pre, maxout=maxout)


def forward_hidden(ctx, nn, x):
    import torch
    ctx.use_torch_stream()
    T = x.shape[0]
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    act = torch.full((T, nn.hidden_dim), float("nan"), dtype=torch.float32, device="cuda")
    nn.forward_hidden_dev(xd, x.shape[1], T, act)
    torch.cuda.synchronize()
    return act.cpu().numpy()


def net(dims, seed, act=ref.ACT_RELU, widen=None):
    """synth.ffnn with hidden activation `act`; widen = {layer: width}: that hidden layer gets `width` outputs (its next layer keeps
    the in-dimension of dims, the maxout's G)"""
    Ws, bs, acts, logp = synth.ffnn(dims, seed=seed, act=act)
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    for l, w in (widen or {}).items():
        Ws[l] = (rng.standard_normal((w, dims[l])) / np.sqrt(dims[l])).astype(np.float32)
        bs[l] = (0.1 * rng.standard_normal(w)).astype(np.float32)
    return Ws, bs, acts, logp


def raw_features(x, seed, positive=False):
    """features a normalisation layer brings back to x: mean m, standard deviation s (one negative, as the reference's test has)"""
    D = x.shape[1]
    rng = np.random.Generator(np.random.PCG64(seed))
    m = (3.0 * rng.standard_normal(D)).astype(np.float32)
    s = (0.5 + 2.0 * rng.random(D)).astype(np.float32)
    s[1] = -s[1]
    raw = (x * s + m).astype(np.float32)
    if positive:
        raw = np.exp(raw / 8).astype(np.float32)
    return raw, m, s


# ------------------------------------------------------------------------------------------------------- 1. preprocessing


@pytest.mark.parametrize("precision", ["fp32", "f16mx"])
def test_preprocessing_kat_on_the_device(ctx, precision):
    """Test/Nn_PreprocessingLayer.cc through forward_hidden of a network without hidden layers (it exports the preprocessed input)"""
    kat = json.load(open(os.path.join(GOLD, "nn_preprocessing_kat.json")))
    x = np.array(kat["input"], np.float32)
    W, b = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    for case in kat["cases"]:
        layers = [tuple(l) for l in case["layers"]]
        nn = scorer(ctx, ([W], [b], [0], None), precision, pre=layers)
        assert nn.hidden_dim == 3
        got = forward_hidden(ctx, nn, x)
        assert np.allclose(got.astype(np.float64), np.array(case["expected"]), rtol=0, atol=kat["tol"]), (case["name"], got)
        assert same_bits(got, ref.preprocess(x, layers)), case["name"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_preprocessing_is_the_host_normalisation(ctx, precision):
    """MVN, log, and log followed by MVN on raw features give the bits of a plain handle fed the host-normalised features; fp32
    scores are the oracle's fmaf chain on them"""
    from oracle import oracle_ffnn_score
    nw = net([40, 300, 260, 333], seed=3)
    x = feats(300, 40, 4)
    raw, m, s = raw_features(x, 5)
    rawp, mp, sp = raw_features(x, 6, positive=True)
    plain = scorer(ctx, nw, precision)
    for name, xin, layers in (("mvn", raw, [(MVN, m, s)]), ("log", rawp, ["logarithm"]),
                              ("log+mvn", rawp, ["logarithm", (MVN, mp / 8, sp / 8)])):
        got = scorer(ctx, nw, precision, pre=layers).score(xin)
        xn = ref.preprocess(xin, layers)
        assert np.isfinite(xn).all()
        assert same_bits(got, plain.score(xn)), name
        if precision == "fp32":
            Ws, bs, acts, logp = nw
            assert same_bits(got, oracle_ffnn_score(Ws, bs, acts, xn, log_prior=logp, acc64=2)), name


def test_f16mx_mvn_brings_large_features_into_range(ctx):
    """features of magnitude 1e6 fail an f16mx pass (AMX_ERR_STATE) unless an MVN layer normalises them before the pack"""
    import rasr_amd
    from oracle import oracle_ffnn_score
    nw = net([64, 256, 300], seed=8)
    x = feats(200, 64, 9)
    m = np.full(64, 2.0e6, np.float32)
    s = np.full(64, 1.0e6, np.float32)
    raw = (x * s + m).astype(np.float32)
    got = scorer(ctx, nw, "f16mx", pre=[(MVN, m, s)]).score(raw)
    Ws, bs, acts, logp = nw
    want = oracle_ffnn_score(Ws, bs, acts, ref.preprocess(raw, [(MVN, m, s)]), log_prior=logp, acc64=True)
    assert meets_bar("f16mx", got, want)
    with pytest.raises(rasr_amd.AmxError) as e:
        scorer(ctx, nw, "f16mx").score(raw)
    assert e.value.status == rasr_amd._lib.AMX_ERR_STATE


# ------------------------------------------------------------------------------------------------------------- 2. ELU


def test_elu_hidden_activations_fp32(ctx):
    """fp32 forward_hidden = elu of the oracle's fmaf-chain linear output, within one ulp (the device expf against the correctly rounded
    one: one ulp of exp(x), which the subtraction of 1 may round to one ulp of the result); non-negative inputs are bit-exact"""
    nw = net([64, 130, 90, 77], seed=17)
    nw[2][1] = ref.ACT_ELU   # ReLU in front (bit-exact), so that the ELU layer's linear output is the oracle's
    x = feats(150, 64, 18)
    got = forward_hidden(ctx, scorer(ctx, nw, "fp32"), x)
    Ws, bs, acts, _ = nw
    from oracle.binding import oracle_ffnn_forward
    want = ref.compose(Ws, bs, acts, x, acc64=2, hidden=True)
    a0 = ref.compose(Ws[:2], bs[:2], acts[:2], x, acc64=2, hidden=True)   # the first hidden layer's activation
    z = oracle_ffnn_forward([Ws[1]], [bs[1]], [0], a0, top=0, acc64=2)   # the last hidden layer's linear output
    neg = z < 0
    assert neg.mean() > 0.2 and same_bits(got[~neg], want[~neg])
    ulp = np.maximum(np.spacing(np.exp(z[neg].astype(np.float64)).astype(np.float32)), np.spacing(np.abs(want[neg])))
    assert np.all(np.abs(got[neg] - want[neg]) <= ulp), np.abs(got[neg] - want[neg]).max()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_elu_scores_meet_the_bar(ctx, precision):
    nw = net([100, 256, 300, 500], seed=19, act=ref.ACT_ELU)
    x = feats(257, 100, 20)
    Ws, bs, acts, logp = nw
    got = scorer(ctx, nw, precision).score(x)
    assert meets_bar(precision, got, ref.compose(Ws, bs, acts, x, log_prior=logp, acc64=True))


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "f16mx"])
def test_elu_tile_configurations_agree(ctx, precision):
    """every tile configuration of a precision gives the same bits with ELU hidden layers (and a maxout, through the score epilogue)"""
    nw = net([64, 300, 150, 700], seed=21, act=ref.ACT_ELU, widen={1: 300})
    x = feats(2100, 64, 22)
    res = {cfg: scorer(ctx, nw, precision, maxout={1: 150}, tuning="tile=" + cfg).score(x) for cfg in TILES[precision]}
    first = res[TILES[precision][0]]
    assert np.isfinite(first).all()
    for cfg, r in res.items():
        assert same_bits(r, first), cfg


# ----------------------------------------------------------------------------------------------------------- 3. maxout


def _var_sizes():
    """520 units in 200 groups: sizes 1 and 2 mostly, one group over units 120..135 (the 128-row tile edge) and one over 250..261
    (the 256-row edge)"""
    sizes = [1] * 40 + [2] * 40 + [16] + [1] * 50 + [2] * 32 + [12] + [3] * 40 + [2] * 22
    sizes.append(520 - sum(sizes))
    assert sizes[-1] >= 1 and 120 == sum(sizes[:80]) and 250 == sum(sizes[:163])
    return sizes


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["fixed", "var"])
def test_maxout_scores(ctx, precision, kind):
    sizes = _var_sizes()
    G = 260 if kind == "fixed" else len(sizes)
    spec = G if kind == "fixed" else sizes
    nw = net([48, G, 300], seed=31, widen={0: 520})
    x = feats(300, 48, 32)
    Ws, bs, acts, logp = nw
    nn = scorer(ctx, nw, precision, maxout={0: spec})
    assert nn.hidden_dim == G
    got = nn.score(x)
    assert meets_bar(precision, got, ref.compose(Ws, bs, acts, x, maxout={0: spec}, log_prior=logp, acc64=True))
    if precision == "fp32":
        assert same_bits(got, ref.compose(Ws, bs, acts, x, maxout={0: spec}, log_prior=logp, acc64=2))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_maxout_on_the_last_hidden_layer(ctx, precision):
    """hidden_dim is G; forward_hidden exports the maxout (bit-exact in fp32 and f16mx, which leave it as f32 rows) and the on-demand
    scorer reads it"""
    import torch
    sizes = _var_sizes()
    nw = net([48, 200, len(sizes), 400], seed=41, widen={1: 520})
    x = feats(260, 48, 42)
    Ws, bs, acts, logp = nw
    nn = scorer(ctx, nw, precision, maxout={1: sizes})
    assert nn.hidden_dim == len(sizes)
    hid = forward_hidden(ctx, nn, x)
    want = ref.compose(Ws, bs, acts, x, maxout={1: sizes}, acc64=2 if precision == "fp32" else True, hidden=True)
    if precision == "fp32":
        assert same_bits(hid, want)
    else:
        assert np.abs(hid - want).max() <= (2e-2 if precision == "bf16" else 1e-4) * (1 + np.abs(want).max())
    rng = np.random.Generator(np.random.PCG64(43))
    n = 1000
    fr, em = rng.integers(0, 260, n).astype(np.int32), rng.integers(0, 400, n).astype(np.int32)
    act = torch.from_numpy(hid).cuda()
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    nn.score_on_demand_dev(act, n, torch.from_numpy(fr).cuda(), torch.from_numpy(em).cuda(), out)
    torch.cuda.synchronize()
    full = -(hid.astype(np.float64) @ Ws[2].T.astype(np.float64) + (bs[2] - logp).astype(np.float64))
    assert np.allclose(out.cpu().numpy(), full[fr, em], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_maxout_nan_selection(ctx, precision):
    """a NaN unit in first position of its group makes the group NaN, a NaN unit in a later position never wins (the bias of a
    unit set to NaN makes it NaN on every frame)"""
    nw = net([32, 40, 10, 50], seed=51, widen={1: 40})
    nw[1][1][0] = np.nan    # group 0, first position
    nw[1][1][6] = np.nan    # group 1, third position
    Ws, bs, acts, logp = nw
    x = feats(70, 32, 52)
    hid = forward_hidden(ctx, scorer(ctx, nw, precision, maxout={1: 10}), x)
    want = ref.compose(Ws, bs, acts, x, maxout={1: 10}, acc64=2, hidden=True)
    assert np.isnan(hid[:, 0]).all() and np.isfinite(hid[:, 1:]).all()
    if precision == "fp32":
        assert np.array_equal(hid, want, equal_nan=True)
    else:
        assert np.allclose(hid[:, 1:], want[:, 1:], rtol=2e-2, atol=2e-2)


# ------------------------------------------------------------------------------------------------ 4. entry points and history


@pytest.mark.parametrize("precision", ["fp32", "f16mx", "bf16x3"])
@pytest.mark.parametrize("tuning", ["chunk=256", "graph=1"])
def test_entry_points_match_fresh_handles(ctx, precision, tuning):
    """one network with MVN, ELU and a maxout through every entry point on one handle, each call against the same call on a fresh
    handle (1000 frames: four internal passes with chunk=256)"""
    import torch
    dims = [40, 300, 150, 256, 333]
    nw = net(dims, seed=61, act=ref.ACT_ELU, widen={1: 300})
    x = feats(1000, 40, 62)
    raw, m, s = raw_features(x, 63)
    Ws, bs, acts, logp = nw
    kw = dict(pre=[(MVN, m, s)], maxout={1: 150}, tuning=tuning)
    ctx.use_torch_stream()
    T, D, M = 1000, 40, 333
    xd = torch.from_numpy(raw).cuda()
    rng = np.random.Generator(np.random.PCG64(64))
    fr = torch.from_numpy(rng.integers(0, T, 3000).astype(np.int32)).cuda()
    em = torch.from_numpy(rng.integers(0, M, 3000).astype(np.int32)).cuda()

    def call(h, what):
        if what == "host":
            return [h.score(raw)]
        if what == "dev":
            sd = torch.full((T, M), float("nan"), dtype=torch.float32, device="cuda")
            for _ in range(3):    # graph=1: the third call replays the captured pass
                h.score_dev(xd, D, T, sd)
            return [sd]
        if what == "stats":
            sd = torch.empty((T, M), dtype=torch.float32, device="cuda")
            st = torch.empty(T, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(M, dtype=torch.int64, device="cuda")
            ssum = torch.zeros(1, dtype=torch.float64, device="cuda")
            h.score_stats_dev(xd, D, T, sd, st, cnt, ssum)
            return [sd, st, cnt, ssum]
        if what in ("linear", "softmax"):
            out = torch.empty((T, M), dtype=torch.float32, device="cuda")
            h.forward_dev(xd, D, T, out, what)
            return [out]
        act = torch.empty((T, h.hidden_dim), dtype=torch.float32, device="cuda")
        h.forward_hidden_dev(xd, D, T, act)
        od = torch.empty(3000, dtype=torch.float32, device="cuda")
        h.score_on_demand_dev(act, 3000, fr, em, od)
        return [act, od]

    def host(vals):
        torch.cuda.synchronize()
        return [v if isinstance(v, np.ndarray) else v.cpu().numpy() for v in vals]

    seq = ["dev", "host", "stats", "linear", "softmax", "hidden", "dev", "stats"]
    h = scorer(ctx, nw, precision, **kw)
    got = [host(call(h, w)) for w in seq]
    h.wait_dev()
    for w, g in zip(seq, got):
        fresh = host(call(scorer(ctx, nw, precision, **kw), w))
        for a, b in zip(g, fresh):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (w, tuning)
    want = ref.compose(Ws, bs, acts, raw, preprocessing=[(MVN, m, s)], maxout={1: 150}, log_prior=logp, acc64=True)
    assert meets_bar(precision, got[0][0], want)
    assert np.array_equal(got[2][1], want.argmin(axis=1))


# ---------------------------------------------------------------------------------------------------------- 5. full size


def test_f16mx_config4_with_mvn_elu_maxout(ctx):
    """BASELINE config 4 (440 -> 6 x 2048 -> 10000) with an MVN input layer, ELU hidden layers and hidden layer 2 widened to 4096
    with a maxout of k = 2, in f16mx at 63 936 frames; checked on a frame sample against the f64-accumulating composition"""
    import torch
    dims = [440] + [2048] * 6 + [10000]
    nw = net(dims, seed=71, act=ref.ACT_ELU, widen={2: 4096})
    Ws, bs, acts, logp = nw
    T = 63936
    x = feats(T, 440, 72)
    raw, m, s = raw_features(x, 73)
    kw = dict(pre=[(MVN, m, s)], maxout={2: 2048})
    nn = scorer(ctx, nw, "f16mx", **kw)
    assert nn.effective_precision()[0] == "f16mx"
    ctx.use_torch_stream()
    xd = torch.from_numpy(raw).cuda()
    sd = torch.empty((T, 10000), dtype=torch.float32, device="cuda")
    nn.score_dev(xd, 440, T, sd)
    nn.wait_dev()
    rows = np.sort(np.random.Generator(np.random.PCG64(74)).choice(T, 192, replace=False))
    got = sd[torch.from_numpy(rows).cuda()].cpu().numpy()
    want = ref.compose(Ws, bs, acts, raw[rows], preprocessing=[(MVN, m, s)], maxout={2: 2048}, log_prior=logp, acc64=True)
    assert meets_bar("f16mx", got, want), np.abs(got - want).max()


# ------------------------------------------------------------------------------------------------------ 6. invalid descriptors


def test_invalid_descriptors_are_refused(ctx):
    import rasr_amd
    nw = net([16, 40, 20, 30], seed=81, widen={1: 40})
    m, s = np.zeros(16, np.float32), np.ones(16, np.float32)
    cases = [
        (dict(maxout={1: [10, 10, 0, 20]}), "layer 1: maxout group 2 has size 0"),
        (dict(maxout={1: [10, 10, 10]}), "layer 1: maxout group sizes add up to 30"),
        (dict(maxout={1: 30}), "layer 1: 40 outputs do not split into 30"),
        (dict(maxout={2: 10}), "layer 2 is the output layer"),
        (dict(maxout={0: 20}), "layer 1 input dimension 40 != 20 outputs of the maxout behind layer 0"),
        (dict(maxout={1: 20}, pre=[(MVN, None, s)]), "preprocessing layer 0 (mean-and-variance-normalization) has no mean vector"),
        (dict(maxout={1: 20}, pre=["logarithm", (MVN, m, None)]), "preprocessing layer 1 (mean-and-variance-normalization) has no standard"),
        (dict(maxout={1: 20}, pre=["logarithm"] * 5), "5 preprocessing layers"),
    ]
    for kw, msg in cases:
        with pytest.raises(rasr_amd.AmxError) as e:
            scorer(ctx, nw, "fp32", **kw)
        assert e.value.status == rasr_amd._lib.AMX_ERR_INVALID and msg in str(e.value), (kw, str(e.value))
    scorer(ctx, nw, "fp32", maxout={1: 20}, pre=["logarithm"] * 4)   # four is the limit
