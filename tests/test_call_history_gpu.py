"""Call history as an input: one handle, a scripted sequence of calls, every result checked three ways.

A handle keeps state that depends on the calls made so far: workspaces sized to the largest pass so far, HIP graphs keyed by buffer
pointers and frame count (and switched off for good after 64 signatures), the tied scorer's near keys and its dense / pruned
decision, the split-K workspace of f16mx ksplit=4.  include/amx.h promises results that do not depend on any of it.  So every call
of a sequence is checked
  (a) bit for bit against the same call on a FRESH handle of the same model and tuning,
  (b) against the oracle at the route's existing bar (GMM and gammatone bit-exact, the log-add scorer and the cepstral front ends at
      their tolerance, NN at nn_parity_report's 1e-4 bar and arg-min rules),
  (c) for device accumulators (counts, score sums, Viterbi statistics): equal to the sum of the fresh handles' contributions,
      counts exactly, f64 atomic sums to 1e-9 relative.
Sequences (each applied to every handle kind it fits):
  S1 large then small (1024, 256, 1, 255, 100, 256); S2 small then large (1, 256, 1024, 256, 6000, host and device entry points);
  S3 replays on unchanged buffers with new contents, a larger pass that moves the workspaces, the recorded signature again, then
     70 signatures that switch graphs off mid-life; S4 entry points interleaved, statistics passes between replays of plain ones;
  S5 tuning chunk=256 and 600 frames (internal passes of 256 + 256 + 88); S6 the context's own stream and torch's, alternating."""
import numpy as np
import pytest

from tests import synth
from tests.parity import nn_parity_report

pytestmark = pytest.mark.gpu

POOL = 6400  # frames every sequence draws its inputs from (the oracle runs once per model over all of them)


def feats(T, dim, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((T, dim)).astype(np.float32)


def _torch():
    import torch
    return torch


def step(call, T, off=None, buf=None, pos=0, stream="torch", **kw):
    """one call of a sequence: entry point, frames [off, off + T) of the pool, device buffer slot (None: new tensors), row offset of
    the input inside the slot (slides the pointer), stream ("torch" | "own")"""
    return dict(call=call, T=T, off=off, buf=buf, pos=pos, stream=stream, **kw)


def _offsets(steps, n_pool):
    out = []
    for i, s in enumerate(steps):
        s = dict(s)
        if s["off"] is None:
            s["off"] = (i * 331 + 17) % max(1, n_pool - s["T"] + 1)
        out.append(s)
    return out


def sequences(kind, graph_call="dev"):
    """the scripted sequences; kind "nn" | "gmm" | "gmm-plain" (scorers with host / device scores only)"""
    dev = graph_call
    S = {}
    S["S1"] = [step(dev, T) for T in (1024, 256, 1, 255, 100, 256)]
    if kind == "nn":
        S["S2"] = [step("host", 1), step("stats", 256), step("dev", 1024), step("stats", 256), step("dev", 6000)]
    elif kind == "gmm":
        S["S2"] = [step("host", 1), step("stats32", 256), step("dev", 1024), step("stats8", 256), step("dev", 6000)]
    else:
        S["S2"] = [step("host", 1), step("dev", 256), step("host", 1024), step("dev", 256), step("dev", 6000)]
    s3 = [step(dev, 256, off=o, buf="A") for o in (0, 300, 600)]              # plain, recorded, replayed: new contents every time
    s3 += [step(dev, 2048, off=1000, buf="B")]                                # moves the workspaces the recorded graph points to
    s3 += [step(dev, 256, off=o, buf="A") for o in (900, 1200, 1500)]         # the recorded signature again
    s3 += [step(dev, 64, off=(37 * i) % 4000, buf="S", pos=i) for i in range(70)]   # 70 signatures: graphs off for good
    s3 += [step(dev, 256, off=o, buf="A") for o in (1800, 2100)]
    S["S3"] = s3
    if kind == "nn":
        S["S4"] = ([step("host", 256, off=0)] + [step("dev", 256, off=o, buf="A") for o in (10, 20, 30)] +
                   [step("stats", 256, off=40, buf="B"), step("dev", 256, off=50, buf="A"), step("hidden", 256, off=60, buf="C"),
                    step("forward", 256, off=70, buf="D"), step("dev", 256, off=80, buf="A"), step("stats", 256, off=90, buf="B"),
                    step("dev", 256, off=100, buf="A"), step("host", 300, off=110), step("dev", 256, off=120, buf="A")])
    elif kind == "gmm":
        S["S4"] = ([step("host", 256, off=0)] + [step("dev", 256, off=o, buf="A") for o in (10, 20, 30)] +
                   [step("stats32", 256, off=40, buf="B"), step("dev", 256, off=50, buf="A"), step("stats8", 256, off=60, buf="C"),
                    step("dev", 256, off=70, buf="A"), step("stats32", 256, off=80, buf="B"), step("acc", 256, off=80),
                    step("bestd", 256, off=90), step("accw", 256, off=90), step("dev", 256, off=100, buf="A"), step("host", 256, off=110),
                    step("acc", 256, off=110), step("stats8", 256, off=120, buf="C"), step("dev", 256, off=130, buf="A")])
    else:
        S["S4"] = ([step("host", 256, off=0)] + [step("dev", 256, off=o, buf="A") for o in (10, 20, 30)] +
                   [step("host", 256, off=40), step("dev", 256, off=50, buf="A"), step("dev", 300, off=60), step("dev", 256, off=70, buf="A")])
    S["S6"] = [step(dev, T, off=o, buf="A" if T == 256 else None, stream=st)
               for T, o, st in ((256, 0, "own"), (256, 100, "torch"), (256, 200, "own"), (1024, 300, "torch"), (256, 400, "own"),
                                (100, 500, "torch"), (256, 600, "own"))]
    return S


S5 = [step("dev", 600, off=0), step("dev", 100, off=700), step("host", 600, off=1000), step("dev", 256, off=2000), step("dev", 600, off=3000, buf="A"),
      step("dev", 600, off=3300, buf="A"), step("dev", 600, off=3600, buf="A")]


class Bufs:
    """device buffers of one handle's sequence: a named slot keeps its tensors (same pointers) for the whole sequence"""

    def __init__(self):
        self.slots = {}

    def get(self, s, name, shape, dtype):
        torch = _torch()
        if s["buf"] is None:
            return torch.empty(shape, dtype=dtype, device="cuda")
        key = (s["buf"], name)
        rows = shape[0] + (s["pos"] if name == "x" else 0)
        t = self.slots.get(key)
        if t is None or t.shape[0] < rows or t.shape[1:] != tuple(shape[1:]) or t.dtype != dtype:
            assert t is None, "slot %s reused with another shape" % (key,)
            cap = max(rows, 4096 if name == "x" else shape[0])
            t = torch.empty((cap,) + tuple(shape[1:]), dtype=dtype, device="cuda")
            self.slots[key] = t
        if name == "x":
            return t[s["pos"]:s["pos"] + shape[0]]
        return t[:shape[0]]


def _np(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    if a.dtype in (np.float32,):
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


def _set_stream(ctx, which):
    if which == "own":
        ctx.L.amx_set_stream(ctx.h, None)
    else:
        ctx.use_torch_stream()


def play(ctx, route, seq, label):
    """run `seq` on ONE handle of `route`; check (a) fresh-handle bits, (b) the oracle, (c) the accumulators after every step"""
    torch = _torch()
    steps = _offsets(seq, route.n_pool)
    h = route.make()
    bufs, acc = Bufs(), route.new_acc()
    want_acc = {k: np.zeros(v.shape, np.float64 if v.dtype == torch.float64 else np.int64) for k, v in acc.items()}
    fresh_cache = {}
    prev = {}
    ctx.use_torch_stream()
    try:
        for i, s in enumerate(steps):
            where = "%s %s step %d %s" % (route.name, label, i, {k: v for k, v in s.items() if v is not None})
            if s["call"] in route.controls:     # a control call on the history handle only (screen counting, preselection parameters)
                route.control(h, s)
                continue
            torch.cuda.synchronize()
            _set_stream(ctx, s["stream"])
            got = route.run(h, s, bufs, acc, prev)
            ctx.synchronize()
            torch.cuda.synchronize()
            ctx.use_torch_stream()
            got = {k: _np(v) if hasattr(v, "cpu") else v for k, v in got.items()}
            key = route.fresh_key(s, prev)
            if key not in fresh_cache:
                f_acc = route.new_acc()
                fh = route.make()
                fres = route.run(fh, s, Bufs(), f_acc, prev)
                torch.cuda.synchronize()
                fresh_cache[key] = ({k: _np(v) if hasattr(v, "cpu") else v for k, v in fres.items()}, {k: _np(v) for k, v in f_acc.items()})
                del fh
            fres, facc = fresh_cache[key]
            for k in fres:                                                   # (a)
                assert got[k].shape == fres[k].shape, (where, k)
                assert _same_bits(got[k], fres[k]), (where, k, "differs from a fresh handle")
            route.check_oracle(s, got, where)                                # (b)
            for k in acc:                                                    # (c)
                want_acc[k] += facc[k]
                have = _np(acc[k])
                if np.issubdtype(have.dtype, np.integer):
                    assert np.array_equal(have, want_acc[k]), (where, k)
                else:
                    assert np.allclose(have, want_acc[k], rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(want_acc[k]).max()))), (where, k)
            route.after(h, s, got)
            prev.update(got)
            prev["_T"] = s["T"]
    finally:
        ctx.use_torch_stream()
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
# NN scorers

_NN_CACHE = {}


def _nn_model(dims, seed):
    key = (tuple(dims), seed)
    if key not in _NN_CACHE:
        _NN_CACHE[key] = synth.ffnn(dims, seed=seed)
    return _NN_CACHE[key]


def _nn_oracle(dims, seed, pool, rows):
    from oracle import oracle_ffnn_score
    key = ("oracle", tuple(dims), seed, rows)
    if key not in _NN_CACHE:
        Ws, bs, acts, logp = _nn_model(dims, seed)
        _NN_CACHE[key] = oracle_ffnn_score(Ws, bs, acts, pool[:rows], log_prior=logp, prior_scale=1.0, acc64=True)
    return _NN_CACHE[key]


class NnRoute:
    controls = ()

    def __init__(self, ctx, dims, precision, tuning, seed=7, oracle_rows=POOL, n_pool=POOL):
        self.ctx, self.dims, self.precision, self.tuning, self.seed = ctx, dims, precision, tuning, seed
        self.name = "nn-%s-%s%s" % ("x".join(map(str, (dims[0], len(dims) - 2, max(dims[1:-1]) if len(dims) > 2 else 0, dims[-1]))), precision,
                                    ("[" + tuning + "]") if tuning else "")
        self.n_pool = n_pool
        self.pool = feats(n_pool, dims[0], 1000 + seed)
        self.oracle_rows = oracle_rows
        self.M = dims[-1]

    def make(self, tuning="same"):
        import rasr_amd
        Ws, bs, acts, logp = _nn_model(self.dims, self.seed)
        return rasr_amd.NnBatchFeatureScorer(self.ctx, Ws, bs, acts, log_prior=logp, priori_scale=1.0, precision=self.precision,
                                             tuning=self.tuning if tuning == "same" else tuning)

    def new_acc(self):
        torch = _torch()
        return dict(counts=torch.zeros((self.M,), dtype=torch.int64, device="cuda"), ssum=torch.zeros((1,), dtype=torch.float64, device="cuda"))

    def fresh_key(self, s, prev):
        return (s["call"], s["T"], s["off"])

    def run(self, h, s, bufs, acc, prev):
        torch = _torch()
        T, D, x = s["T"], self.dims[0], self.pool[s["off"]:s["off"] + s["T"]]
        if s["call"] == "host":
            return dict(scores=h.score(x))
        xd = bufs.get(s, "x", (T, D), torch.float32)
        xd.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()     # inputs are written on torch's stream; the call may run on the context's own
        if s["call"] == "dev":
            sd = bufs.get(s, "scores", (T, self.M), torch.float32)
            h.score_dev(xd, D, T, sd)
            return dict(scores=sd)
        if s["call"] == "stats":
            sd = bufs.get(s, "scores", (T, self.M), torch.float32)
            st = bufs.get(s, "state", (T,), torch.int32)
            h.score_stats_dev(xd, D, T, sd, st, acc["counts"], acc["ssum"])
            return dict(scores=sd, state=st)
        if s["call"] == "hidden":
            H = h.hidden_dim
            act = bufs.get(s, "act", (T, H), torch.float32)
            h.forward_hidden_dev(xd, D, T, act)
            rng = np.random.Generator(np.random.PCG64(s["off"]))
            n = 2 * T
            fr = torch.from_numpy(rng.integers(0, T, n).astype(np.int32)).cuda()
            em = torch.from_numpy(rng.integers(0, self.M, n).astype(np.int32)).cuda()
            od = torch.empty((n,), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            h.score_on_demand_dev(act, n, fr, em, od)
            return dict(hidden=act, on_demand=od)
        if s["call"] == "forward":
            out = bufs.get(s, "forward", (T, self.M), torch.float32)
            h.forward_dev(xd, D, T, out, "softmax")
            return dict(forward=out)
        raise AssertionError(s["call"])

    def check_oracle(self, s, got, where):
        if "scores" not in got:
            return      # hidden / on-demand / forward outputs: (a) only here, their bars live in test_ffnn_*
        lo, hi = s["off"], min(s["off"] + s["T"], self.oracle_rows)
        if hi <= lo:
            return
        want = _nn_oracle(self.dims, self.seed, self.pool, self.oracle_rows)[lo:hi]
        sc = got["scores"][:hi - lo]
        if self.precision == "bf16":     # not a 1e-4 path: test_bf16_path_accuracy's bar, relative to the score scale
            assert np.abs(sc - want).max() < 5e-2 * np.abs(want).mean(), (where, np.abs(sc - want).max())
            return
        rep = nn_parity_report(sc, want, gap=1e-5)
        assert rep["bar_violations"] == 0 and rep["worst_pure_relative"] <= 1e-4, (where, rep)
        assert rep["argmin_mismatches_outside_gap_rule"] == 0, (where, rep)
        if "state" in got:
            assert np.array_equal(got["state"], got["scores"].argmin(axis=1)), where

    def after(self, h, s, got):
        pass


NN_SMALL = [64, 256, 256, 300]
NN_CASES = [(p, g) for p in ("fp32", "bf16", "bf16x3", "f16mx") for g in ("", "graph=1")]


@pytest.mark.parametrize("seq", ["S1", "S2", "S3", "S4", "S6"])
@pytest.mark.parametrize("precision,tuning", NN_CASES, ids=["%s%s" % (p, "-graph" if g else "") for p, g in NN_CASES])
def test_nn_call_history(ctx, precision, tuning, seq):
    route = NnRoute(ctx, NN_SMALL, precision, tuning or None)
    play(ctx, route, sequences("nn")[seq], seq)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3", "f16mx"])
@pytest.mark.parametrize("graph", ["", ",graph=1"])
def test_nn_call_history_chunked_passes(ctx, precision, graph):
    """S5: tuning chunk=256, so 600 frames are three internal passes of different Tpad (256 + 256 + 88)"""
    route = NnRoute(ctx, NN_SMALL, precision, "chunk=256" + graph)
    play(ctx, route, S5, "S5")


class KsplitRoute(NnRoute):
    """f16mx ksplit=4: besides (a) - (c), every fill that can run split must still differ from the default order's bits (the
    split is on), whatever the handle scored first"""

    def __init__(self, ctx, dims, split_fills, **kw):
        super().__init__(ctx, dims, "f16mx", "ksplit=4", **kw)
        self.split_fills = split_fills

    def after(self, h, s, got):
        if s["T"] in self.split_fills and s["call"] == "dev":
            dflt = self.make(tuning=None)
            torch = _torch()
            x = torch.from_numpy(self.pool[s["off"]:s["off"] + s["T"]]).cuda()
            out = torch.empty((s["T"], self.M), dtype=torch.float32, device="cuda")
            dflt.score_dev(x, self.dims[0], s["T"], out)
            torch.cuda.synchronize()
            d = _np(out)
            assert np.count_nonzero(got["scores"].view(np.uint32) != d.view(np.uint32)) > 0, \
                (self.name, s, "the split-K fill gives the default order's bits: the split is off")
            assert np.max(np.abs(got["scores"] - d) / (np.abs(d) + 1.0)) < 2e-5, (self.name, s)


def test_f16mx_ksplit_config4_large_pass_first(ctx):
    """BASELINE config 4's network (440-6x2048-10000) with ksplit=4 and S1: the handle's first pass has 1024 frames, which nothing
    can split (16 x 16 tiles x 4 > 256 CUs); the 256-frame fills after it must still run split -- the bits of a fresh ksplit=4
    handle, not the default order's.  The oracle checks the frames of the first 256 of the pool."""
    route = KsplitRoute(ctx, [440] + [2048] * 6 + [10000], split_fills=(256,), oracle_rows=256, n_pool=1024)
    seq = [step("dev", 1024, off=0)] + [step("dev", T, off=o) for T, o in ((256, 0), (1, 5), (255, 1), (100, 37), (256, 0))]
    play(ctx, route, seq, "S1")


def test_f16mx_ksplit_narrow_layers_split_at_512_frames(ctx):
    """1024-wide hidden layers split at 512 frames too (8 x 8 tiles x 4 = 256): the workspace must cover the worst pass that can
    ever split, not the split layers of the pass that first grew the buffers"""
    route = KsplitRoute(ctx, [440, 1024, 1024, 1024, 2000], split_fills=(256, 512), oracle_rows=1024, n_pool=2048)
    seq = [step("dev", 1024, off=0), step("dev", 512, off=0), step("dev", 256, off=100), step("dev", 512, off=512, buf="A"),
           step("dev", 512, off=300, buf="A"), step("dev", 1, off=7), step("dev", 512, off=200, buf="A")]
    play(ctx, route, seq, "S1")


# ---------------------------------------------------------------------------------------------------------------------------------
# GMM scorers

_GMM_CACHE = {}

GMM_MODELS = {
    "cart": lambda: synth.gmm_cart(64, 1, 16, 40, seed=160, pooled=True),
    "cart-private": lambda: synth.gmm_cart(48, 1, 8, 40, seed=161, pooled=False),
    "tied": lambda: synth.gmm_tied(120, 192, 40, seed=162, pooled=True, alpha=0.1),
}


def _gmm_model(name):
    if name not in _GMM_CACHE:
        _GMM_CACHE[name] = GMM_MODELS[name]()
    return _GMM_CACHE[name]


class GmmRoute:
    def __init__(self, ctx, model, kind="diagonal-maximum", tuning=None, presel=None):
        self.ctx, self.model_name, self.kind, self.tuning = ctx, model, kind, tuning
        self.name = "gmm-%s-%s%s" % (model, kind, ("[" + tuning + "]") if tuning else "")
        self.n_pool = POOL
        self.pool = feats(POOL, 40, 2000)
        self.pool_tag = "standard"    # names the pool in the oracle cache (a test may replace frames)
        self.M = len(_gmm_model(model)["mix_offsets"]) - 1
        self.presel = presel          # current preselection parameters (clusters, select, iterations, backoff)
        self.max_mode = kind == "diagonal-maximum"
        self.controls = ("screen_on", "screen_off", "presel", "count")
        self.counts = []              # screen_counts() read by "count" steps

    def make(self):
        import rasr_amd
        sc = rasr_amd.GmmFeatureScorer(self.ctx, _gmm_model(self.model_name), feature_scorer_type=self.kind, tuning=self.tuning)
        if self.presel is not None:
            sc.set_preselection(*self.presel)
        return sc

    def control(self, h, s):
        if s["call"] == "presel":
            self.presel = s["params"]
            h.set_preselection(*self.presel)
        elif s["call"] == "count":
            self.counts.append(h.screen_counts(True))
        else:
            h.screen_counts(s["call"] == "screen_on")

    def new_acc(self):
        torch = _torch()
        if not self.max_mode:
            return {}
        n = _torch_acc_size(self)
        return dict(counts=torch.zeros((self.M,), dtype=torch.int64, device="cuda"), ssum=torch.zeros((1,), dtype=torch.float64, device="cuda"),
                    acc=torch.zeros((n,), dtype=torch.float64, device="cuda"))

    def fresh_key(self, s, prev):
        return (s["call"], s["T"], s["off"], self.presel, s["call"] in ("acc", "bestd", "accw") and prev.get("_T"))

    def _want_best(self):
        return self.kind in ("diagonal-maximum", "diagonal-sum", "SIMD-diagonal-maximum")

    def run(self, h, s, bufs, acc, prev):
        torch = _torch()
        T, x = s["T"], self.pool[s["off"]:s["off"] + s["T"]]
        c = s["call"]
        if c == "host":
            r = h.score(x, want_best=self._want_best())
            return dict(scores=r[0], best=r[1]) if self._want_best() else dict(scores=r)
        xd = bufs.get(s, "x", (T, 40), torch.float32)
        xd.copy_(torch.from_numpy(x))
        torch.cuda.synchronize()     # inputs are written on torch's stream; the call may run on the context's own
        if c == "dev":
            sd = bufs.get(s, "scores", (T, self.M), torch.float32)
            bd = bufs.get(s, "best", (T, self.M), torch.int32) if self._want_best() else None
            h.score_dev(xd, T, sd, bd)
            return dict(scores=sd, best=bd) if bd is not None else dict(scores=sd)
        if c in ("stats32", "stats8"):
            sd = bufs.get(s, "scores", (T, self.M), torch.float32)
            bd = bufs.get(s, "best" + c, (T, self.M), torch.int32 if c == "stats32" else torch.uint8)
            st = bufs.get(s, "state", (T,), torch.int32)
            h.score_stats_dev(xd, T, sd, bd, st, acc["counts"], acc["ssum"])
            return dict(scores=sd, best=bd, state=st) if c == "stats32" else dict(scores=sd, best8=bd, state=st)
        mix = prev["scores"].argmin(axis=1).astype(np.int32) if prev.get("_T") == T else \
            np.random.Generator(np.random.PCG64(s["off"])).integers(0, self.M, T).astype(np.int32)
        md = torch.from_numpy(mix).cuda()
        torch.cuda.synchronize()
        if c == "acc":       # Viterbi statistics from the previous call's best-density matrix
            bm = torch.from_numpy(prev["best"].astype(np.int32)).cuda()
            torch.cuda.synchronize()
            h.accumulate_dev(xd, T, md, bm, self.M, acc["acc"])
            return {}
        if c == "bestd":
            bdv = torch.empty((T,), dtype=torch.int32, device="cuda")
            sdv = torch.empty((T,), dtype=torch.float32, device="cuda")
            h.best_density_dev(xd, T, md, bdv, sdv)
            return dict(bd=bdv, sd=sdv, mix=mix)
        if c == "accw":      # weighted Viterbi statistics of the previous call's aligned densities
            import rasr_amd
            mix = prev["mix"]
            md = torch.from_numpy(mix).cuda()
            w = torch.from_numpy(np.random.Generator(np.random.PCG64(s["off"] + 1)).uniform(0.0, 2.0, T)).cuda()
            cd = torch.from_numpy(prev["bd"].astype(np.int32)).cuda()
            torch.cuda.synchronize()
            h.accumulate_weighted_dev(rasr_amd.AMX_GMM_VITERBI, xd, T, md, w, cd, 0, acc["acc"])
            return {}
        raise AssertionError(c)

    def _oracle(self):
        from oracle import OracleGmm
        key = ("oracle", self.model_name, self.kind, self.presel, self.pool_tag)
        if key not in _GMM_CACHE:
            o = OracleGmm(_gmm_model(self.model_name))
            if self.kind == "diagonal-maximum":
                r = o.score(self.pool, mode=0)
            elif self.kind == "diagonal-sum":
                r = o.score(self.pool, mode=1)
            elif self.kind == "batch-diagonal-maximum-float":
                r = (o.score_batch_float(self.pool), None)
            elif self.kind == "SIMD-diagonal-maximum":
                r = o.score_simd(self.pool)[:2]
            elif self.kind == "batch-diagonal-maximum-int":
                r = (o.score_batch_int(self.pool), None)
            elif self.kind == "preselection-batch-float":
                r = (o.score_preselection_float(self.pool, *self.presel)[0], None)
            else:
                r = (o.score_preselection_int(self.pool, *self.presel[:3])[0], None)
            _GMM_CACHE[key] = r
        return _GMM_CACHE[key]

    def check_oracle(self, s, got, where):
        if "scores" not in got and "bd" not in got:
            return
        osc, obest = self._oracle()
        rows = slice(s["off"], s["off"] + s["T"])
        if "bd" in got:
            t = np.arange(s["T"])
            assert np.array_equal(got["bd"].astype(np.uint32), obest[rows][t, got["mix"]]), where
            assert _same_bits(got["sd"], osc[rows][t, got["mix"]]), where
            return
        if self.kind == "diagonal-sum":
            assert np.allclose(got["scores"], osc[rows], rtol=1e-5, atol=1e-5), (where, np.abs(got["scores"] - osc[rows]).max())
        else:
            assert _same_bits(got["scores"], osc[rows]), (where, np.abs(got["scores"] - osc[rows]).max())
        if "best" in got and obest is not None:
            assert np.array_equal(got["best"].astype(np.uint32), obest[rows]), where
        if "best8" in got:
            assert np.array_equal(got["best8"], np.where(obest[rows] == 0xFFFFFFFF, 0xFF, obest[rows]).astype(np.uint8)), where
        if "state" in got:
            assert np.array_equal(got["state"], osc[rows].argmin(axis=1)), where

    def after(self, h, s, got):
        pass


def _torch_acc_size(route):
    import rasr_amd
    return rasr_amd.GmmFeatureScorer(None, _gmm_model(route.model_name)).accumulator_size()


GMM_MAX_CASES = [("cart", None), ("cart", "graph=1"), ("cart", "fused_pack=0"), ("cart", "fused_pack=0,graph=1"), ("cart", "fused=0"),
                 ("cart", "fused=0,graph=1"), ("tied", "tied_prune=1"), ("tied", "tied_prune=1,graph=1"), ("tied", "tied_prune=0"),
                 ("tied", "near_fused=0,tied_prune=1"), ("tied", "near_fused=0,tied_prune=1,graph=1"), ("tied", None), ("tied", "graph=1")]


@pytest.mark.parametrize("seq", ["S1", "S2", "S3", "S4", "S6"])
@pytest.mark.parametrize("model,tuning", GMM_MAX_CASES, ids=["%s-%s" % (m, t or "default") for m, t in GMM_MAX_CASES])
def test_gmm_max_call_history(ctx, model, tuning, seq):
    route = GmmRoute(ctx, model, tuning=tuning)
    s = sequences("gmm")[seq]
    if seq == "S3":          # screen counting switched on and off mid-sequence: recorded passes carry the counter argument
        s = s[:2] + [step("screen_on", 0)] + s[2:5] + [step("screen_off", 0)] + s[5:]
    play(ctx, route, s, seq)


@pytest.mark.parametrize("model,tuning", [("cart", "chunk=256"), ("cart", "chunk=256,fused=0,graph=1"), ("tied", "chunk=256,tied_prune=1,graph=1"),
                                          ("tied", "chunk=256,tied_prune=0")])
def test_gmm_call_history_chunked_passes(ctx, model, tuning):
    """S5: tuning chunk=256, 600 frames = internal passes of 256 + 256 + 88 frames"""
    play(ctx, GmmRoute(ctx, model, tuning=tuning), S5, "S5")


GMM_OTHER_CASES = [("cart-private", "diagonal-sum", None), ("tied", "diagonal-sum", None), ("cart", "batch-diagonal-maximum-float", None),
                   ("cart", "SIMD-diagonal-maximum", None), ("cart", "batch-diagonal-maximum-int", None),
                   ("cart", "preselection-batch-float", (16, 4, 5, 40000.0)), ("cart", "preselection-batch-int", (16, 4, 5, 0.0))]


@pytest.mark.parametrize("seq", ["S1", "S2", "S3", "S4", "S6"])
@pytest.mark.parametrize("model,kind,presel", GMM_OTHER_CASES, ids=["%s-%s" % (m, k) for m, k, _ in GMM_OTHER_CASES])
def test_gmm_other_scorers_call_history(ctx, model, kind, presel, seq):
    """the direct log-add scorer and the batch / SIMD / preselection scorers (never recorded as graphs)"""
    play(ctx, GmmRoute(ctx, model, kind=kind, presel=presel), sequences("gmm-plain")[seq], seq)


@pytest.mark.parametrize("kind,params", [("preselection-batch-float", [(16, 4, 5, 40000.0), (8, 2, 3, 123.0), (16, 16, 5, 40000.0)]),
                                         ("preselection-batch-int", [(16, 4, 5, 0.0), (8, 2, 3, 0.0), (16, 16, 5, 0.0)])])
def test_gmm_preselection_changed_mid_life(ctx, kind, params):
    """set_preselection between calls of one handle: every call equals a fresh handle given the same parameters, and the oracle"""
    seq = []
    for j, p in enumerate(params):
        seq += [step("presel", 0, params=p)] + [step("dev" if k % 2 else "host", T, off=300 * j + 50 * k) for k, T in enumerate((1024, 256, 1, 256))]
    play(ctx, GmmRoute(ctx, "cart", kind=kind, presel=params[0]), seq, "presel")


@pytest.mark.parametrize("tuning", [None, "graph=1"])
def test_gmm_tied_dense_pruned_decision_flips(ctx, tuning):
    """the adaptive tied scorer decides dense or pruned from survivor statistics of EARLIER calls (more than 10 % of the examined
    triples standing: 64 calls on the dense kernel): frames next to one density each (prunable), then frames drawn like the means
    (more than a tenth survives), then prunable frames again -- every call bit-exact whichever kernel ran, and the triples the
    pruned path examined show that the decision did flip both ways"""
    route = GmmRoute(ctx, "tied", tuning=tuning)
    model = _gmm_model("tied")
    rng = np.random.Generator(np.random.PCG64(2002))
    route.pool = route.pool.copy()
    near = model["means"][rng.integers(0, len(model["means"]), 1024)] + 0.05 * rng.standard_normal((1024, 40))
    route.pool[:1024] = near.astype(np.float32)
    route.pool_tag = "near"
    seq = [step("count", 0)] + [step("dev", 256, off=(k % 3) * 256, buf="A") for k in range(24)] + [step("count", 0)]
    seq += [step("dev", 256, off=4096 + (k % 3) * 256, buf="A") for k in range(40)] + [step("count", 0)]
    seq += [step("dev", 256, off=(k % 3) * 256 + 7, buf="A") for k in range(64)] + [step("count", 0)]
    seq += [step("dev", 256, off=(k % 3) * 256 + 9, buf="A") for k in range(32)] + [step("count", 0)]
    play(ctx, route, seq, "flip")
    per_call = 192 * 256 * 2       # densities x frames x 64-mixture tiles
    t = [c[1] // per_call for c in route.counts[1:]]
    frac = [c[0] / max(1, c[1]) for c in route.counts[1:]]
    assert t[0] == 24, (t, frac)              # prunable frames: every call pruned
    assert t[1] < 40, (t, frac)               # frames that defeat pruning: the dense kernel takes over
    assert t[2] < 64 and t[3] > 0, (t, frac)  # prunable again: dense for the rest of its window, then pruned once more


# ---------------------------------------------------------------------------------------------------------------------------------
# front ends: workspaces sized to the largest batch so far (mfcc.hip d_ac, gammatone.hip d_off / d_ti: DevBuf capacities)

FE_BATCHES = [(48000, 16000, 0, 7777, 32000), (401,), (0, 160), (64000, 400, 12345, 0, 2000), (1,), (5281, 48077)]


class FrontEnd:
    def __init__(self, ctx, kind):
        self.ctx, self.kind = ctx, kind
        self.wave = synth.waveform(200000, seed=3000)
        self._oracle = {}

    def make(self):
        import rasr_amd
        if self.kind == "mfcc":
            return rasr_amd.MfccExtractor(self.ctx, nr_cepstrum_coefficients=16)
        if self.kind == "mfplp":
            return rasr_amd.MfccExtractor(self.ctx, nr_cepstrum_coefficients=12, front_end="mfplp", nr_autocorrelation_coefficients=16, normalize=True)
        if self.kind == "plp":
            return rasr_amd.MfccExtractor.plp(self.ctx)
        return rasr_amd.GammatoneExtractor(self.ctx, channels=68, max_freq=7500.0, si_length=9, si_shift=4, power=0.1, n_ceps=12)

    def oracle(self, off, n):
        if (off, n) not in self._oracle:
            from oracle import OracleMfcc
            from oracle.binding import GammatoneCfg, MfccCfg, OracleGammatone
            pcm = self.wave[off:off + n]
            if self.kind == "mfcc":
                o = OracleMfcc(n_ceps=16)
            elif self.kind == "mfplp":
                o = OracleMfcc(MfccCfg.mfplp(n_ceps=12, n_autocorrelation=16))
            elif self.kind == "plp":
                o = OracleMfcc(MfccCfg.plp())
            else:
                o = OracleGammatone(GammatoneCfg.default(channels=68, max_freq=7500.0, si_length=9, si_shift=4, power=0.1, n_ceps=12))
            self._oracle[(off, n)] = o.run(pcm)
        return self._oracle[(off, n)]

    def run(self, h, call, segs):
        torch = _torch()
        pcms = [self.wave[o:o + n] for o, n in segs]
        if call == "host":
            return h.run_batch(pcms)
        off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
        pcm = torch.from_numpy(np.concatenate(pcms) if off[-1] else np.zeros(1, np.float32)).cuda()
        if self.kind == "gammatone":
            nf = [h.n_frames(len(p)) for p in pcms]
            out = torch.empty((max(1, sum(nf)), h.n_out), dtype=torch.float32, device="cuda")
            h.run_batch_dev(off, pcm, out)
            fo = np.concatenate([[0], np.cumsum(nf)])
        else:
            plan = h.plan(off)
            out = torch.empty((max(1, plan.total_frames), h.n_ceps), dtype=torch.float32, device="cuda")
            h.run_plan(plan, pcm, out)
            fo = plan.frame_offsets
        torch.cuda.synchronize()
        o = _np(out)
        return [o[fo[u]:fo[u + 1]] for u in range(len(pcms))]

    def check_oracle(self, got, want, where):
        from tests.test_mfcc_gpu import PLP_ATOL, PLP_RTOL, close
        assert got.shape == want.shape, where
        if self.kind == "gammatone":
            assert _same_bits(got, want), (where, np.abs(got - want).max())
            return
        fin = np.isfinite(want)          # log10(0) = -inf (a one-sample segment) and NaN (a failed recursion) as the reference has them
        assert np.array_equal(got[~fin], want[~fin], equal_nan=True), where
        assert np.array_equal(np.isfinite(got), fin), where
        if self.kind == "mfcc":
            assert close(got[fin], want[fin]), (where, np.abs(got[fin] - want[fin]).max())
        else:
            assert np.all(np.abs(got[fin] - want[fin]) <= PLP_RTOL * np.abs(want[fin]) + PLP_ATOL), where


@pytest.mark.parametrize("call", ["host", "dev"])
@pytest.mark.parametrize("kind", ["mfcc", "mfplp", "plp", "gammatone"])
def test_front_end_call_history(ctx, kind, call):
    """ragged batches large -> small -> large (with empty segments) on one extractor: every segment bit-identical to a fresh
    extractor's and at the oracle's bar (bit-exact for gammatone)"""
    if kind == "gammatone" and call == "host":
        call = "dev-again"      # gammatone has no host batch entry point: the device sequence twice on the same handle
    fe = FrontEnd(ctx, kind)
    h = fe.make()
    ctx.use_torch_stream()
    rounds = 2 if call == "dev-again" else 1
    for r in range(rounds):
        for b, lens in enumerate(FE_BATCHES):
            segs = [((7919 * (b + 1) * (u + 1)) % (len(fe.wave) - n + 1), n) for u, n in enumerate(lens)]
            where = (kind, call, r, b, lens)
            got = fe.run(h, "dev" if call == "dev-again" else call, segs)
            fresh = fe.run(fe.make(), "dev" if call == "dev-again" else call, segs)
            for u, (o, n) in enumerate(segs):
                assert _same_bits(got[u], fresh[u]), (where, u, "differs from a fresh extractor")
                fe.check_oracle(got[u], fe.oracle(o, n), (where, u))
