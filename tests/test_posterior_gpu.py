"""GPU parity: amx_posterior_dev, amx_posterior_lists_dev and amx_posterior_gmm_dev (posterior_kernel, posterior_list_kernel) through
rasr_amd.StatePosteriorScorer against the restatement of tests/posterior_reference.py, which tests/test_posterior.py holds against the
reference's own results.

Bars.  s, the minimum, its index, the survivor sets, counts and sparse indices: bits.  f64 posteriors and logZ: 1e-11 relative (derived
in tests/test_posterior.py: the order of the f64 sum is the only freedom), and 0 where the restatement has 0.  f32 posteriors: equal in
bits wherever the restatement's f64 value is further than 1e-11 relative from a midpoint between two f32 values, one ulp elsewhere; the
exempted share is asserted <= 1 % on the CPU before the device is touched.  Whatever the batch, a frame's results are the same bits.

Shapes.  posterior_kernel takes one wave for rows up to 256 mixtures and four waves above, four elements per lane and pass: 1, 2, 63,
64, 65 mixtures are below / at / above a wave's lanes, 257 is the first row of the four-wave kernel, 1000 fills one pass of it raggedly,
4099 takes five passes with a ragged tail.  The score matrix has ld = n + 3 with NaN in the padding (so rows start unaligned and the
scalar path loads them), and once ld = n rounded up to 4 (the dwordx4 path)."""
import numpy as np
import pytest

from tests import posterior_reference as pr
from tests.test_posterior import REL, close, refused, same

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 1000, 4099)
T_ALL = 300
BATCHES = (0, 1, 2, 65, 300)
DBL_MAX = pr.DBL_MAX
S_F32, S_F64, S_I32 = np.float32(-12345.5), -54321.25, -77


def inputs(n, T=T_ALL, seed=0):
    """scores N(50, 30) with a few near 1e4 (exp underflows there), priors in [0, 5]"""
    rng = np.random.Generator(np.random.PCG64(1009 * n + seed))
    s = rng.normal(50.0, 30.0, (T, n)).astype(np.float32)
    hit = rng.random((T, n)) < 0.03
    s[hit] = (1e4 + rng.normal(0.0, 50.0, (T, n))).astype(np.float32)[hit]
    return s, rng.random(n) * 5.0


def cancelling_inputs(n, T, seed):
    """inputs on which the reference's two arithmetics differ by more than the tests' tolerance: scores near 1e7 (whole numbers, exact in
    f32) and priors near -0.37e7, so that s = prior + 0.37 * score is of order 10 while the product is of order 4e6.  The product's
    rounding, up to 2.3e-10, which the fused form does not make, then moves a posterior by up to that much relative: 20 times the
    1e-11 bar.  Returns scores, priors [n] and the offset -0.37e7 for per-entry priors."""
    rng = np.random.Generator(np.random.PCG64(2003 * n + seed))
    s = (1e7 + rng.integers(0, 80, (T, n))).astype(np.float32)
    return s, -0.37e7 + rng.random(n) * 5.0, -0.37e7


def exempt_share(post):
    live = post > 0
    return float(np.mean(pr.midpoint_distance(post[live]) <= REL)) if live.any() else 0.0


class Run:
    """one call with every output pre-filled with sentinels; results on the host"""

    def __init__(self, h, scores, pad=3, capacity=None, mode="mixture", best=None, margin_mixture=None, rows=None):
        import torch
        T, n = scores.shape
        ld = n + pad if pad >= 0 else (n + 3) // 4 * 4
        wide = np.full((T, ld), np.nan, np.float32)
        wide[:, :n] = scores
        cap = n if capacity is None else capacity
        dev = torch.from_numpy(wide).cuda()
        # pad < 0: the rows of the dense outputs start on 16-byte boundaries too (the 16-byte stores); still wider than n
        ld32 = n + 2 if pad >= 0 else (n + 2 + 3) // 4 * 4
        ld64 = n + 1 if pad >= 0 else (n + 1 + 1) // 2 * 2
        o32 = torch.full((T, ld32), float(S_F32), dtype=torch.float32, device="cuda")
        o64 = torch.full((T, ld64), S_F64, dtype=torch.float64, device="cuda")
        lz = torch.full((T,), S_F64, dtype=torch.float64, device="cuda")
        mn = torch.full((T,), S_F64, dtype=torch.float64, device="cuda")
        mi = torch.full((T,), S_I32, dtype=torch.int32, device="cuda")
        ns = torch.full((T,), S_I32, dtype=torch.int32, device="cuda")
        si = torch.full((T, cap + 1), S_I32, dtype=torch.int32, device="cuda")   # one guard cell behind the last row's capacity
        sv = torch.full((T, cap + 1), float(S_F32), dtype=torch.float32, device="cuda")
        sc = torch.full((T,), S_I32, dtype=torch.int32, device="cuda")
        # the sparse arrays are [T x capacity] for the library; the guard column is the tail of a flat buffer of T * cap + T cells
        si_flat, sv_flat = si.reshape(-1), sv.reshape(-1)
        bd = torch.from_numpy(np.ascontiguousarray(best)).cuda() if best is not None else None
        mm = torch.from_numpy(np.ascontiguousarray(margin_mixture, dtype=np.int32)).cuda() if margin_mixture is not None else None
        torch.cuda.synchronize()
        sel = range(T) if rows is None else rows
        self.no_min = 0
        if rows is None:
            self.no_min = h.posteriors(dev, ld, T, mode=mode, best_density_dev=bd, margin_mixture_dev=mm, posterior_f32_dev=o32, posterior_f32_ld=ld32,
                                       posterior_f64_dev=o64, posterior_f64_ld=ld64, log_z_dev=lz, min_dev=mn, min_index_dev=mi, n_survivors_dev=ns,
                                       sparse_index_dev=si_flat, sparse_value_dev=sv_flat, sparse_count_dev=sc, sparse_capacity=cap)
        else:   # the given rows, one call each, in the given order
            for t in sel:
                self.no_min += h.posteriors(dev[t:], ld, 1, mode=mode, best_density_dev=bd[t:] if bd is not None else None,
                                            margin_mixture_dev=mm[t:] if mm is not None else None, posterior_f32_dev=o32[t:], posterior_f32_ld=ld32,
                                            posterior_f64_dev=o64[t:], posterior_f64_ld=ld64, log_z_dev=lz[t:], min_dev=mn[t:], min_index_dev=mi[t:],
                                            n_survivors_dev=ns[t:], sparse_index_dev=si_flat[t * cap:], sparse_value_dev=sv_flat[t * cap:],
                                            sparse_count_dev=sc[t:], sparse_capacity=cap)
        torch.cuda.synchronize()
        self.T, self.n, self.cap = T, n, cap
        self.o32, self.o64 = o32.cpu().numpy(), o64.cpu().numpy()
        self.lz, self.mn, self.mi, self.ns, self.sc = (x.cpu().numpy() for x in (lz, mn, mi, ns, sc))
        flat_i, flat_v = si_flat.cpu().numpy(), sv_flat.cpu().numpy()
        self.si, self.sv = flat_i[:T * cap].reshape(T, cap), flat_v[:T * cap].reshape(T, cap)
        self.guard_i, self.guard_v = flat_i[T * cap:], flat_v[T * cap:]

    def arrays(self):
        return (self.o32, self.o64, self.lz, self.mn, self.mi, self.ns, self.sc, self.si, self.sv)


def check(run, want, keys=None, likelihood=False):
    """a Run against the restatement's dict"""
    T, n, cap = run.T, run.n, run.cap
    assert same(run.mn, want["min"]) and np.array_equal(run.mi, want["min_index"])
    assert np.array_equal(run.ns, want["n_survivors"]) and np.array_equal(run.sc, want["n_survivors"])
    if not likelihood:
        assert close(run.lz, want["log_z"])
    else:
        assert np.all(run.lz == S_F64)
    assert close(run.o64[:, :n], want["post"]) and not np.any(run.o64[:, :n][want["post"] == 0])
    far = pr.midpoint_distance(want["post"]) > REL
    d = pr.ulp_distance32(run.o32[:, :n], want["post32"])
    assert not np.any(d[far]) and np.all(d <= 1)
    assert np.all(run.o32[:, n:] == S_F32) and np.all(run.o64[:, n:] == S_F64)   # nothing outside the rows
    assert np.all(run.guard_i == S_I32) and np.all(run.guard_v == S_F32)
    for t, (idx, val) in enumerate(pr.sparse_rows(want, keys)):
        k = min(len(idx), cap)
        assert same(run.si[t, :k], idx[:k]), t
        assert np.all(pr.ulp_distance32(run.sv[t, :k], val[:k]) <= 1) and same(run.sv[t, :k], run.o32[t, np.nonzero(want["survivors"][t])[0][:k]]), t
        assert np.all(run.si[t, k:] == S_I32) and np.all(run.sv[t, k:] == S_F32), t


@pytest.fixture(scope="module")
def wanted():
    """the restatement per size, computed once: scale 0.37, random priors, threshold 30"""
    cache = {}

    def get(n):
        if n not in cache:
            s, prior = inputs(n)
            cache[n] = (s, prior, pr.posteriors(s, 0.37, prior, None, 30.0))
        return cache[n]
    return get


@pytest.mark.parametrize("n", SIZES)
def test_mixture_posteriors_and_batch_independence(ctx, wanted, n):
    import rasr_amd
    ctx.use_torch_stream()
    s, prior, want = wanted(n)
    assert exempt_share(want["post"]) <= 0.01
    if n > 2:
        assert len(set(want["n_survivors"].tolist())) > 1 and want["n_survivors"].max() < n   # the threshold keeps a few, not all
    h = rasr_amd.StatePosteriorScorer(ctx, n, scale=0.37, pruning_threshold=30.0)
    h.set_filter(np.arange(n), prior)
    full = Run(h, s)
    assert full.no_min == 0
    check(full, want)
    for T in BATCHES[:-1]:   # 0, 1, 2 and 65 frames in one call: the same bits as in the call of 300
        part = Run(h, s[:T])
        for a, b in zip(part.arrays(), full.arrays()):
            assert same(a, b[:T]), T
    back = Run(h, s[::-1].copy())   # another batch order
    for a, b in zip(back.arrays(), full.arrays()):
        assert same(a, b[::-1]), "reversed"
    single = Run(h, s[:65], rows=list(range(64, -1, -1)))   # single-frame calls
    for a, b in zip(single.arrays(), full.arrays()):
        assert same(a, b[:65]), "single"
    aligned = Run(h, s[:65], pad=-1)   # rows of the scores and of the dense outputs on 16-byte boundaries: the 16-byte loads and stores
    check(aligned, {k: v[:65] for k, v in want.items()})
    for a, b in zip(aligned.arrays()[2:], full.arrays()[2:]):
        assert same(a, b[:65]), "aligned"
    assert same(aligned.o32[:, :n], full.o32[:65, :n]) and same(aligned.o64[:, :n], full.o64[:65, :n])
    one = Run(h, s[:65], pad=-1, rows=[64, 0, 33])   # ... and as single-frame calls
    for t in (64, 0, 33):
        assert same(one.o32[t, :n], full.o32[t, :n]) and same(one.o64[t, :n], full.o64[t, :n]) and np.all(one.o32[t, n:] == S_F32), t
    h.close()


@pytest.mark.parametrize("n", (65, 257, 1000))
@pytest.mark.parametrize("threshold", (DBL_MAX, 30.0, 1e-3))
def test_thresholds_and_sparse_capacity(ctx, n, threshold):
    import rasr_amd
    ctx.use_torch_stream()
    s, prior = inputs(n, 40, seed=5)
    want = pr.posteriors(s, 1.0, prior, None, threshold)
    assert exempt_share(want["post"]) <= 0.01
    most = int(want["n_survivors"].max())
    if threshold == DBL_MAX:
        assert np.all(want["n_survivors"] == n)    # keeps all
    elif threshold == 1e-3:
        assert np.all(want["n_survivors"] == 1)    # keeps the minimum only
    else:
        assert 1 < most < n                        # keeps a few
    h = rasr_amd.StatePosteriorScorer(ctx, n, pruning_threshold=threshold)
    h.set_filter(np.arange(n), prior)
    for cap in sorted({max(most - 1, 0), most, most + 5, 0}):   # smaller than, equal to and larger than the survivors' count; none
        check(Run(h, s, capacity=cap), want)
    h.close()


@pytest.mark.parametrize("n", (2, 65, 257, 4099))
def test_tie_and_rows_without_a_minimum(ctx, n):
    import rasr_amd
    ctx.use_torch_stream()
    s, _ = inputs(n, 6, seed=9)
    a, b = (0, 1) if n == 2 else (7, n - 2)   # the tie's two indices: different lanes; different waves above a wave
    s[1, :] += np.float32(100.0)
    s[1, a] = s[1, b] = np.float32(3.25)      # an exact two-way tie for the minimum
    s[2, :] = np.inf                          # no minimum
    s[4, :] = np.inf
    s[4, n - 1] = np.float32(1.5)             # one finite value, last
    s[5, 0] = -np.inf                         # the minimum is -inf: no minimum either
    want = pr.posteriors(s, 1.0)
    assert exempt_share(want["post"]) <= 0.01
    assert want["min_index"].tolist()[1:3] == [a, -1] and want["min_index"][4] == n - 1 and want["min_index"][5] == -1
    assert want["post"][1, a] == want["post"][1, b] > 0 and not want["post"][2].any()
    h = rasr_amd.StatePosteriorScorer(ctx, n)
    run = Run(h, s)
    assert run.no_min == 2
    check(run, want)
    h.close()


def test_filter_with_holes_and_disregard(ctx):
    import rasr_amd
    ctx.use_torch_stream()
    n = 257
    s, prior = inputs(n, 20, seed=3)
    rng = np.random.Generator(np.random.PCG64(4))
    keep = np.sort(rng.choice(n, 180, replace=False))
    h = rasr_amd.StatePosteriorScorer(ctx, n, scale=0.5, pruning_threshold=30.0)
    h.set_filter(keep, prior[keep])
    h.set_disregard([int(keep[0]), int(keep[77]), n + 9])
    in_filter = np.zeros(n, bool)
    in_filter[keep] = True
    in_filter[[keep[0], keep[77]]] = False
    assert np.array_equal(h.filter()[0], np.nonzero(in_filter)[0])
    want = pr.posteriors(s, 0.5, prior, in_filter, 30.0)
    default = pr.posteriors(s, 0.5, None, None, 30.0)
    assert exempt_share(want["post"]) <= 0.01 and exempt_share(default["post"]) <= 0.01
    # the frames' minima over ALL mixtures lie outside the filter somewhere: the filter acts
    assert np.any(pr.posteriors(s, 0.5, prior, None, 30.0)["min_index"] != want["min_index"])
    check(Run(h, s), want)
    h.set_disregard([])
    h.set_default_filter()   # back to every mixture with prior 0: the table-free path
    check(Run(h, s), default)
    h.close()


def test_likelihoods(ctx):
    import rasr_amd
    ctx.use_torch_stream()
    n = 257
    s, prior = inputs(n, 20, seed=6)
    s = (s * np.float32(0.1)).astype(np.float32)   # exp(-s) stays inside f64 and f32
    for threshold in (DBL_MAX, 3.0):
        want = pr.posteriors(s, 1.0, prior, None, threshold, likelihood=True)
        assert exempt_share(want["post"]) <= 0.01 and want["post"].max() > 0
        h = rasr_amd.StatePosteriorScorer(ctx, n, pruning_threshold=threshold)
        h.set_filter(np.arange(n), prior)
        check(Run(h, s, mode="likelihood"), want, likelihood=True)
        h.close()


@pytest.mark.parametrize("n", (65, 257))
def test_density_keyed_posteriors_with_margin(ctx, n):
    import rasr_amd
    ctx.use_torch_stream()
    T = 24
    s, prior = inputs(n, T, seed=11)
    rng = np.random.Generator(np.random.PCG64(12 + n))
    sizes = rng.integers(1, 4, n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    topo = rng.permutation(int(off[-1])).astype(np.uint32)
    best = (rng.integers(0, 1 << 20, (T, n)) % sizes[None, :]).astype(np.uint32)
    keys = pr.density_keys(off, topo, best)
    plain = pr.posteriors(s, 0.37, prior, None, 30.0)
    mm = np.full(T, -1, np.int32)
    for t in range(T):   # on the minimum, on another survivor, none
        if t % 3 == 0:
            mm[t] = plain["min_index"][t]
        elif t % 3 == 1:
            others = [m for m in np.nonzero(plain["survivors"][t])[0] if m != plain["min_index"][t]]
            mm[t] = others[0] if others else (plain["min_index"][t] + 1) % n
    want = pr.posteriors(s, 0.37, prior, None, 30.0, margin=2.5, margin_mixture=mm)
    assert not same(want["post"], plain["post"]) and same(want["min"], plain["min"])   # the margin acts, and not on the minimum
    assert exempt_share(want["post"]) <= 0.01 and exempt_share(plain["post"]) <= 0.01
    h = rasr_amd.StatePosteriorScorer(ctx, n, scale=0.37, pruning_threshold=30.0, margin=2.5)
    h.set_filter(np.arange(n), prior)
    h.set_topology(off, topo)
    assert h.topology_info() == (False, -1)
    run = Run(h, s, mode="density", best=best, margin_mixture=mm)
    check(run, want, keys=keys)
    # the adapter's sort gives the node's vector: keys in increasing order with their values
    rows = h.sort_sparse(run.si, run.sv, run.sc)
    for t, (idx, val) in enumerate(rows):
        m = np.nonzero(want["survivors"][t])[0]
        order = np.argsort(keys[t, m])
        assert np.array_equal(idx, keys[t, m][order]) and np.all(np.diff(idx) > 0) and same(val, run.o32[t, m[order]]), t
    # the mixture modes refuse a margin mixture; a shared density is refused in density-keyed mode only
    refused(-1, "margin_mixture_dev", Run, h, s, margin_mixture=mm)
    shared = topo.copy()
    shared[off[3]] = shared[off[1]]
    h.set_topology(off, shared)
    assert h.topology_info()[1] == int(shared[off[1]])
    refused(-2, "density %d" % shared[off[1]], Run, h, s, mode="density", best=best)
    check(Run(h, s), plain)
    h.close()


@pytest.mark.parametrize("contract", ("off", "fma"))
def test_candidate_lists(ctx, contract):
    """in both arithmetics: the fixture records that the reference's two builds differ on the lists wherever scale != 1"""
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    n = 257
    lengths = [0, 1, 64, 65, 300, 0, 2, 300, 64]
    T = len(lengths)
    s, _, shift = cancelling_inputs(n, T, seed=13)
    s[6, :] = np.inf   # a list without a minimum
    rng = np.random.Generator(np.random.PCG64(14))
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    mix = rng.integers(0, n, int(off[-1])).astype(np.int32)
    pri = shift + rng.random(int(off[-1])) * 5.0
    mix[off[4] + 5] = mix[off[4] + 200]   # a repeated mixture with one prior and the row's lowest score: an exact tie for the minimum;
    pri[off[4] + 5] = pri[off[4] + 200]   # the first in list order is the minimum's own entry, the second adds exp(0) to the sum
    s[4, mix[off[4] + 5]] = np.float32(1e7 - 100.0)
    want = pr.list_posteriors(s, 0.37, off, mix, pri, contract_fma=contract == "fma")
    other = pr.list_posteriors(s, 0.37, off, mix, pri, contract_fma=contract != "fma")
    assert not close(want, other, 10 * REL) and not close(other, want, 10 * REL)   # the other arithmetic is 10 bars away: the test can fail
    assert exempt_share(want) <= 0.01 and not want[off[6]:off[7]].any() and want[off[4]:off[5]].max() > 0
    h = rasr_amd.StatePosteriorScorer(ctx, n, scale=0.37)
    sd = torch.from_numpy(np.pad(s, ((0, 0), (0, 3)), constant_values=np.nan)).cuda()
    md, pd = torch.from_numpy(mix).cuda(), torch.from_numpy(pri).cuda()
    o64 = torch.full((len(mix) + 1,), S_F64, dtype=torch.float64, device="cuda")
    o32 = torch.full((len(mix) + 1,), float(S_F32), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = ctx.contract()
    ctx.set_contract(contract)
    try:
        assert h.list_posteriors(sd, n + 3, off, md, pd, o64, o32) == 1
        torch.cuda.synchronize()
        singles = []   # every list alone, in the same arithmetic
        for t in range(T):
            one = torch.full((max(lengths[t], 1),), S_F64, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            if lengths[t]:
                h.list_posteriors(sd[t:], n + 3, np.array([0, lengths[t]]), md[off[t]:], pd[off[t]:], one, None)
            torch.cuda.synchronize()
            singles.append(one.cpu().numpy()[:lengths[t]])
    finally:
        ctx.set_contract(before)
    g64, g32 = o64.cpu().numpy(), o32.cpu().numpy()
    assert g64[-1] == S_F64 and g32[-1] == S_F32
    assert close(g64[:-1], want) and not np.any(g64[:-1][want == 0])
    far = pr.midpoint_distance(want) > REL
    d = pr.ulp_distance32(g32[:-1], want.astype(np.float32))
    assert not np.any(d[far]) and np.all(d <= 1)
    # every list alone gives the bits it gave in the batch
    for t in range(T):
        assert same(singles[t], g64[off[t]:off[t + 1]]), t
    h.close()


@pytest.mark.parametrize("n", (13, 200))
def test_contract_modes(ctx, n):
    """where the reference's two builds differ (the fixture: scale != 1 with priors that are not 0), the device follows amx_set_contract:
    mixture posteriors, density-keyed posteriors with a margin, likelihoods"""
    import rasr_amd
    ctx.use_torch_stream()
    T = 12
    s, prior, _ = cancelling_inputs(n, T, seed=21)
    rng = np.random.Generator(np.random.PCG64(22 + n))
    sizes = rng.integers(1, 4, n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    topo = rng.permutation(int(off[-1])).astype(np.uint32)
    best = (rng.integers(0, 1 << 20, (T, n)) % sizes[None, :]).astype(np.uint32)
    keys = pr.density_keys(off, topo, best)
    want = {}
    for c in ("off", "fma"):
        f = c == "fma"
        mix = pr.posteriors(s, 0.37, prior, None, 30.0, contract_fma=f)
        mm = np.where(np.arange(T) % 2 == 0, mix["min_index"], (mix["min_index"] + 1) % n).astype(np.int32)   # on and off the minimum
        want[c] = dict(mixture=mix, mm=mm, density=pr.posteriors(s, 0.37, prior, None, 30.0, margin=2.5, margin_mixture=mm, contract_fma=f),
                       likelihood=pr.posteriors(s, 0.37, prior, None, 3.0, likelihood=True, contract_fma=f))
        for k in ("mixture", "density", "likelihood"):
            assert exempt_share(want[c][k]["post"]) <= 0.01, (c, k)
    for k in ("mixture", "density", "likelihood"):   # the other arithmetic is 10 bars away and has another minimum: the test can fail
        assert not same(want["off"][k]["min"], want["fma"][k]["min"]), k
        assert np.array_equal(want["off"][k]["survivors"], want["fma"][k]["survivors"]), k
        assert not close(want["off"][k]["post"], want["fma"][k]["post"], 10 * REL), k
    h = rasr_amd.StatePosteriorScorer(ctx, n, scale=0.37, pruning_threshold=30.0, margin=2.5)
    h.set_filter(np.arange(n), prior)
    h.set_topology(off, topo)
    hl = rasr_amd.StatePosteriorScorer(ctx, n, scale=0.37, pruning_threshold=3.0)
    hl.set_filter(np.arange(n), prior)
    before = ctx.contract()
    try:
        for c in ("fma", "off"):
            ctx.set_contract(c)
            check(Run(h, s), want[c]["mixture"])
            check(Run(h, s, mode="density", best=best, margin_mixture=want[c]["mm"]), want[c]["density"], keys=keys)
            check(Run(hl, s, mode="likelihood"), want[c]["likelihood"], likelihood=True)
    finally:
        ctx.set_contract(before)
    h.close()
    hl.close()


def test_posteriors_gmm_is_score_then_posteriors(ctx):
    import rasr_amd
    import torch
    from tests import synth
    ctx.use_torch_stream()
    dim, n, T = 16, 65, 33
    model = synth.gmm_cart(n, 1, 3, dim, seed=5, pooled=False)
    gmm = rasr_amd.GmmFeatureScorer(ctx, model, "diagonal-maximum")
    rng = np.random.Generator(np.random.PCG64(32))
    feats = torch.from_numpy(rng.standard_normal((T, dim)).astype(np.float32)).cuda()
    sc = torch.zeros((T, n), dtype=torch.float32, device="cuda")
    bd = torch.zeros((T, n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gmm.score_dev(feats, T, sc, bd)
    torch.cuda.synchronize()
    h = rasr_amd.StatePosteriorScorer(ctx, n, pruning_threshold=20.0)
    h.set_topology(gmm=gmm)
    assert h.topology_info() == (True, -1)
    outs = []
    for composed in (False, True):
        o64 = torch.full((T, n), S_F64, dtype=torch.float64, device="cuda")
        si = torch.full((T, n), S_I32, dtype=torch.int32, device="cuda")
        sv = torch.full((T, n), float(S_F32), dtype=torch.float32, device="cuda")
        cnt = torch.full((T,), S_I32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        kw = dict(mode="density", posterior_f64_dev=o64, sparse_index_dev=si, sparse_value_dev=sv, sparse_count_dev=cnt, sparse_capacity=n)
        if composed:
            assert h.posteriors_gmm(gmm, feats, T, **kw) == 0
        else:
            assert h.posteriors(sc, n, T, best_density_dev=bd, **kw) == 0
        torch.cuda.synchronize()
        outs.append([x.cpu().numpy() for x in (o64, si, sv, cnt)])
    for a, b in zip(*outs):
        assert same(a, b)
    scores, best = sc.cpu().numpy(), bd.cpu().numpy().astype(np.int64)
    want = pr.posteriors(scores, 1.0, None, None, 20.0)
    keys = pr.density_keys(model["mix_offsets"], model["dens_index"], best)
    assert close(outs[1][0], want["post"]) and np.array_equal(outs[1][3], want["n_survivors"])
    for t, (idx, _) in enumerate(pr.sparse_rows(want, keys)):
        assert np.array_equal(outs[1][1][t, :len(idx)], idx) and np.all(np.diff(idx) > 0), t   # monotone: already in key order
    twelve = rasr_amd.GmmFeatureScorer(ctx, synth.gmm_cart(12, 1, 1, dim, seed=6, pooled=False), "diagonal-maximum")
    refused(-1, "12 mixtures", h.posteriors_gmm, twelve, feats, T)
    h.close()
