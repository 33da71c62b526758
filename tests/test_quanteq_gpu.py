"""GPU parity: amx_quanteq_apply_dev and amx_quanteq_estimate_dev (quanteq_quantile_kernel, quanteq_search_kernel,
quanteq_combine_search_kernel, quanteq_apply_kernel, quanteq_sum_kernel, quanteq_normalize_kernel) through the Python classes against the
fixture that the reference's own text produced in both of its builds; tests/test_quanteq.py holds the restatement against the same fixture.

The bar.  Quantiles, alpha, gamma, lambda and rho are equal in every bit, with no exception.  Outputs, means and deviations are equal in
bits, NaNs compare by position.  The device's double pow is not glibc's, but every pow result is narrowed to f32 inside a double
expression, so a one-ulp error of the double survives only within about 2^-29 of a rounding boundary.  One exception, for the outputs
only: per contract at most 1e-5 of the output elements of the whole fixture may differ, each by at most 2 f32 ulps of
max(|reference|, |mean|).  The count is printed.

Shapes.  Every configuration of the fixture goes through ONE call: its segments one after the other with an empty segment first, in the
middle and last, the first frame at row 2, in_ld = dim + 3 with NaN in the spare columns, out_ld = dim + 1 with a sentinel in the spare
column; then once more in place.  Lengths 1, 2, 3, 5, 63, 64, 65, 300 lie around the sort's power-of-two network sizes and the sum kernel's
block of 8 frames; 1024 | 1025 and 16383 | 16384 are the network's largest step and the end of LDS (16385 is refused).
"""
import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import quanteq_reference as R
from tests.test_quanteq import config, config_names, differing, fixture, recorded, same, segments, training

pytestmark = pytest.mark.gpu

CONTRACTS = ("off", "fma")
FIRST_ROW, PAD_IN, PAD_OUT = 2, 3, 1
SENTINEL = np.float32(-12345.5)
ALLOWED_FRACTION, ALLOWED_ULPS = 1e-5, 2
off_budget = {c: 0 for c in CONTRACTS}      # output elements that used the exception, per contract, over the whole module


@pytest.fixture()
def cctx(ctx):
    """the session context, handed out in contract=off and restored to it (other tests expect the default)"""
    ctx.set_contract("off")
    ctx.use_torch_stream()
    yield ctx
    ctx.set_contract("off")


def total_outputs():
    return sum(recorded("off", n + "/out").size for n in config_names())


def handle(cctx, name, **more):
    dim, c = config(name)
    kw = dict(quantiles=c["quantiles"], combination=c["combination"], mean=c["mean"], variance=c["variance"], number_of_quantiles=c["nq"],
              overestimation_factor=c["of"], delta_alpha=c["delta_alpha"], delta_gamma=c["delta_gamma"], delta_lambda_and_rho=c["delta_lr"],
              beta=c["beta"], pool_quantiles=c["pool"])
    kw.update(more)
    return rasr_amd.QuantileEqualization(cctx, dim, training(name) if c["quantiles"] else None, **kw)


def batch(name):
    """(segment lengths with the empty ones, index of each fixture segment in that list, offsets from FIRST_ROW, the wide input matrix)"""
    dim, _ = config(name)
    xs, _ = segments(name)
    lens, where = [0], []
    for i, x in enumerate(xs):
        where.append(len(lens))
        lens.append(len(x))
        if i == len(xs) // 2:
            lens.append(0)
    lens.append(0)
    off = np.concatenate([[FIRST_ROW], FIRST_ROW + np.cumsum(lens)]).astype(np.int64)
    wide = np.full((off[-1], dim + PAD_IN), np.nan, np.float32)
    wide[:FIRST_ROW, :dim] = 7.0
    wide[FIRST_ROW:, :dim] = np.concatenate(xs)
    return lens, where, off, wide


def ulps_apart(got, ref, mean):
    """|got - ref| in f32 ulps of max(|ref|, |mean|)"""
    scale = np.maximum(np.abs(ref), np.abs(mean)).astype(np.float32)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(scale).astype(np.float64)


def check_outputs(got, name, contract):
    """the bar of the module's docstring for one configuration's outputs; returns the elements that used the exception"""
    ref = recorded(contract, name + "/out")
    assert got.shape == ref.shape
    _, off = segments(name)
    u = got.view(np.uint32) != ref.view(np.uint32)
    u &= ~(np.isnan(got) & np.isnan(ref))
    n = int(u.sum())
    if n:
        mean = np.concatenate([np.broadcast_to(recorded(contract, name + "/params")[s, 4], (off[s + 1] - off[s], got.shape[1])) for s in range(len(off) - 1)])
        worst = ulps_apart(got[u], ref[u], mean[u]).max()
        print("quanteq %s/%s: %d of %d output elements differ, at most %.2f ulps" % (name, contract, n, got.size, worst))
        assert worst <= ALLOWED_ULPS, (name, contract, n, worst)
        off_budget[contract] += n
        assert off_budget[contract] <= int(ALLOWED_FRACTION * total_outputs()), (name, contract, off_budget)
    return n


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("name", config_names())
def test_apply_equals_the_reference(cctx, name, contract):
    import torch
    dim, c = config(name)
    cctx.set_contract(contract)
    lens, where, off, wide = batch(name)
    xs, foff = segments(name)
    h = handle(cctx, name)
    xd = torch.from_numpy(wide).cuda()
    out = torch.full((int(off[-1]), dim + PAD_OUT), float(SENTINEL), dtype=torch.float32, device="cuda")
    par = h.apply_dev(off, xd, dim + PAD_IN, out, dim + PAD_OUT, want_params=True)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[:FIRST_ROW] == SENTINEL) and np.all(got[:, dim:] == SENTINEL)       # rows before the call's first frame, spare column
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), wide.view(np.uint32))          # the input is read only
    want = recorded(contract, name + "/params")
    for i, s in enumerate(where):
        tag = (name, contract, i, lens[s])
        for k, field in enumerate(("alpha", "gamma", "lambda", "rho")):
            assert np.array_equal(par[field][s].view(np.uint32), want[i, k].view(np.uint32)), tag + (field,)
        if c["quantiles"]:
            assert np.array_equal(par["quantiles"][s].view(np.uint32), R.quantiles(xs[i], c["nq"]).view(np.uint32)), tag + ("quantiles",)
        assert same(par["mean"][s], want[i, 4]), tag + ("mean",)
        assert same(par["deviation"][s], want[i, 5]), tag + ("deviation",)
    for s, n in enumerate(lens):
        if n == 0:
            assert not any(par[k][s].any() for k in par), (name, s)
    n_exc = check_outputs(got[FIRST_ROW:, :dim], name, contract)
    # in place, on the identical view, without asking for the parameters
    h.apply_dev(off, xd, dim + PAD_IN, xd, dim + PAD_IN)
    torch.cuda.synchronize()
    again = xd.cpu().numpy()
    assert np.array_equal(again[FIRST_ROW:, :dim].view(np.uint32), got[FIRST_ROW:, :dim].view(np.uint32)), (name, contract, "in place")
    assert np.all(np.isnan(again[:, dim:])) and np.all(again[:FIRST_ROW, :dim] == 7.0)
    print("quanteq %s/%s: %d segments, %d output elements, %d used the exception" % (name, contract, len(where), got[FIRST_ROW:, :dim].size, n_exc))


def test_the_two_contracts_differ_on_the_device(cctx):
    """the one-frame segment on which the reference's builds choose different (alpha, gamma): so does the device"""
    import torch
    fx = fixture()
    xs, _ = segments("d20")
    x = xs[-1]
    assert len(x) == 1 and differing(fx["fma/d20/params"][-1, :2], fx["off/d20/params"][-1, :2]) > 0
    got = {}
    for contract in CONTRACTS:
        cctx.set_contract(contract)
        h = handle(cctx, "d20")
        xd = torch.from_numpy(x).cuda()
        got[contract] = h.apply_dev([0, 1], xd, 20, xd, 20, want_params=True)
        for k, field in enumerate(("alpha", "gamma")):
            assert np.array_equal(got[contract][field][0].view(np.uint32), recorded(contract, "d20/params")[-1, k].view(np.uint32)), (contract, field)
    assert differing(got["off"]["alpha"], got["fma"]["alpha"]) + differing(got["off"]["gamma"], got["fma"]["gamma"]) > 0


def test_refusals_write_nothing(cctx):
    import torch
    dim = 20
    lens, where, off, wide = batch("d20_cv")
    h = handle(cctx, "d20_cv")
    out = torch.full((int(off[-1]), dim), float(SENTINEL), dtype=torch.float32, device="cuda")
    for value, seg, ch in ((np.nan, where[3], 7), (np.inf, where[4], 0), (-np.inf, where[0], 19)):
        bad = wide.copy()
        bad[off[seg] + lens[seg] // 2, ch] = value
        bad[off[where[5]] + 1, 11] = np.nan                 # a later one as well: the first is named
        xd = torch.from_numpy(bad).cuda()
        with pytest.raises(rasr_amd.AmxError, match="segment %d, channel %d " % (seg, ch)) as e:
            h.apply_dev(off, xd, dim + PAD_IN, out, dim, want_params=True)
        assert e.value.status == _lib.AMX_ERR_INVALID and "not finite" in str(e.value)
        torch.cuda.synchronize()
        assert bool((out == float(SENTINEL)).all()), "a refused call wrote"
    xd = torch.from_numpy(wide).cuda()
    # the handle still works, and gives what it gives when fresh
    h.apply_dev(off, xd, dim + PAD_IN, out, dim)
    torch.cuda.synchronize()
    assert check_outputs(out.cpu().numpy()[FIRST_ROW:], "d20_cv", "off") >= 0
    # a segment longer than the sort takes: named, nothing written
    out.fill_(float(SENTINEL))
    long_off = np.array([0, 5, 5 + _lib.AMX_QUANTEQ_MAX_SEGMENT_FRAMES + 1], np.int64)
    with pytest.raises(rasr_amd.AmxError, match="segment 1 has 16385 frames") as e:
        h.apply_dev(long_off, xd, dim + PAD_IN, out, dim)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    for bad_off, word in (([0, 5, 3], "decrease"), ([-1, 3], "negative")):
        with pytest.raises(rasr_amd.AmxError, match=word):
            h.apply_dev(np.array(bad_off, np.int64), xd, dim + PAD_IN, out, dim)
    with pytest.raises(rasr_amd.AmxError, match="in_ld"):
        h.apply_dev(off, xd, dim - 1, out, dim)
    with pytest.raises(rasr_amd.AmxError, match="overlap"):
        h.apply_dev(off, xd, dim + PAD_IN, xd[1:], dim + PAD_IN)
    torch.cuda.synchronize()
    assert bool((out == float(SENTINEL)).all())
    # nothing to do
    h.apply_dev(np.array([4], np.int64), xd, dim + PAD_IN, out, dim)
    h.apply_dev(np.array([4, 4, 4], np.int64), None, dim + PAD_IN, None, dim)


def test_reused_handles_give_the_same_bits_whatever_ran_before(cctx):
    """a handle's workspaces are sized by the calls before: a small call after a large one, and the large one again"""
    import torch
    dim = 20
    h = handle(cctx, "d20_cv")
    lens, where, off, wide = batch("d20_cv")
    xd = torch.from_numpy(wide).cuda()

    def run(o, handle_):
        out = torch.full((int(off[-1]), dim), float(SENTINEL), dtype=torch.float32, device="cuda")
        par = handle_.apply_dev(o, xd, dim + PAD_IN, out, dim, want_params=True)
        torch.cuda.synchronize()
        return out.cpu().numpy(), par

    small = off[where[1]:where[1] + 2]
    first_small, p_small = run(small, h)
    large, p_large = run(off, h)
    again_small, p_again = run(small, h)
    again_large, p_again_large = run(off, h)
    fresh_large, p_fresh = run(off, handle(cctx, "d20_cv"))
    for a, b in ((first_small, again_small), (large, again_large), (large, fresh_large)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in ((p_small, p_again), (p_large, p_again_large), (p_large, p_fresh)):
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    # the small call alone is what the large call gives for that segment
    a, e = int(small[0]), int(small[1])
    assert np.array_equal(first_small[a:e].view(np.uint32), large[a:e].view(np.uint32))
    assert bool(np.all(first_small[:a] == SENTINEL)) and bool(np.all(first_small[e:] == SENTINEL))


@pytest.mark.parametrize("name", config_names(estimate=True))
def test_estimation_equals_the_reference(cctx, name, tmp_path):
    """sums in f64 on the host in segment order, one count per non-empty segment, in any split; the file's bytes"""
    import torch
    fx = fixture()
    dim, c = config(name)
    lens, where, off, wide = batch(name)
    xd = torch.from_numpy(wide).cuda()
    want, count = fx["off/" + name + "/sums"], int(fx["off/" + name + "/count"])
    xs, _ = segments(name)
    rs, rc = R.estimate(xs, c["nq"])
    assert same(rs, want) and rc == count
    for cuts in ([0, len(off) - 1], [0, 1, 2, len(off) - 1], list(range(len(off)))):
        est = rasr_amd.QuantileEstimator(cctx, dim, number_of_quantiles=c["nq"])
        for a, e in zip(cuts[:-1], cuts[1:]):
            est.accumulate_dev(off[a:e + 1], xd, dim + PAD_IN)
        sums, n = est.result()
        assert n == count and np.array_equal(sums.view(np.uint64), want.view(np.uint64)), (name, cuts)
    p = str(tmp_path / "quantiles.txt")
    est.write(p)
    with open(p, "rb") as f:
        assert f.read() == fx["off/" + name + "/file"].tobytes()
    with pytest.raises(TypeError):
        est.apply_dev(off, xd, dim + PAD_IN, xd, dim + PAD_IN)
    bad = wide.copy()
    bad[off[where[0]], 1] = np.nan
    with pytest.raises(rasr_amd.AmxError, match="not finite"):
        est.accumulate_dev(off, torch.from_numpy(bad).cuda(), dim + PAD_IN)
    assert est.result()[1] == count                        # a refused call adds nothing


def test_negative_zero_sorts_before_positive_zero(cctx):
    """the added rule where std::sort leaves the order open: of equal zeros the negative ones come first, so the lowest quantile of a
    column of both is -0 and the highest +0, whatever their order in the segment"""
    import torch
    for T in (2, 7, 64, 65):
        x = np.zeros((T, 3), np.float32)
        x[::2, 0] = -0.0                    # -0 first
        x[1::2, 1] = -0.0                   # +0 first
        x[:, 2] = np.linspace(-1.0, 1.0, T, dtype=np.float32)
        x[T // 2, 2] = -0.0
        nq = T - 1 if T <= 7 else 4         # T - 1: every order statistic is a quantile
        h = rasr_amd.QuantileEqualization(cctx, 3, np.ones((nq + 1, 3), np.float32), mean=0, number_of_quantiles=nq)
        xd = torch.from_numpy(x).cuda()
        out = torch.empty_like(xd)
        q = h.apply_dev([0, T], xd, 3, out, 3, want_params=True)["quantiles"][0]
        for d in (0, 1):
            assert q[0, d].view(np.uint32) == 0x80000000 and q[-1, d].view(np.uint32) == 0, (T, d, q[:, d])
            if nq == T - 1:                 # the negative zeros, then the positive ones
                assert np.array_equal(np.signbit(q[:, d]), np.arange(T) < int(np.signbit(x[:, d]).sum())), (T, d, q[:, d])
        assert np.array_equal(q[:, 2], R.quantiles(x, nq)[:, 2])
