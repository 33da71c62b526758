"""GPU parity: amx_linseg_align_dev (linseg_kernel) against the restatement of tests/linseg_reference.py, which tests/test_linseg.py holds
to the reference's own results in both of its builds.

The device's double logarithm need not agree with glibc's in the last bit and the delimitation is discrete, so the restatement says per
case whether it is DECIDED (no comparison between two different candidates closer than 2^-48 S, S the larger |s * log(.)| term;
DESIGN.md section 6).  Decided cases must agree exactly in everything discrete and within 2^-47 S in the score; the fixture's generator
asserts that only the tie_* cases are undecided, and those are held to the weaker check: the device's choice is as good as the
restatement's within the margin, and everything after the choice is exact."""
import numpy as np
import pytest

from tests import linseg_reference as lr
from tests import synth
from tests import train_reference as tr

pytestmark = pytest.mark.gpu

SENTINEL = -77
CFG_KEYS = tuple(lr.DEFAULTS)


@pytest.fixture()
def cctx(ctx):
    """the session context on torch's stream, handed out in contract=off and restored to it"""
    ctx.use_torch_stream()
    ctx.set_contract("off")
    yield ctx
    ctx.set_contract("off")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


_RESTATED = {}


def restated(name, contract):
    """the restatement's result of a fixture case, computed once per session and never changed"""
    if (name, contract) not in _RESTATED:
        c = lr.cases()[name]
        _RESTATED[name, contract] = lr.segment(c["energy"], c["labels"], c["emissions"], contract=contract, **c["cfg"])
    return _RESTATED[name, contract]


def call(ctx, segments, front=0, column=None, seg=None, **cfg):
    """one amx_linseg_align_dev call.  segments: (energy, labels, emissions) per segment; front: rows in front of the first segment;
    column: (ld, c) puts the energies into column c of a [rows x ld] matrix of other values.  Returns a dict: label, emission (numpy,
    every row, SENTINEL where nothing was written), results, counters, off, and chains(s) reading the handle's workspace."""
    import torch

    import rasr_amd
    off = np.cumsum([front] + [len(s[0]) for s in segments])
    e = np.full(int(off[-1]), 123.0, np.float32)
    for o, s in zip(off, segments):
        e[o:o + len(s[0])] = s[0]
    if column is None:
        buf, ld = torch.from_numpy(e).cuda(), 1
        energy = buf
    else:
        ld, c = column
        m = np.random.Generator(np.random.PCG64(9)).standard_normal((len(e), ld)).astype(np.float32)
        m[:, c] = e
        buf = torch.from_numpy(m).cuda()
        energy = buf[:, c]
    lab = torch.full((int(off[-1]),), SENTINEL, dtype=torch.int32, device="cuda")
    emi = torch.full((int(off[-1]),), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    own = seg is None
    seg = rasr_amd.LinearSegmenter(ctx, **cfg) if own else seg
    models = rasr_amd.LinearSegmenter.models([(s[1], s[2]) for s in segments], lr.SILENCE_LABEL, lr.SILENCE_EMISSION)
    _, _, results, counters = seg.align(off, models, energy, ld, lab, emi)
    torch.cuda.synchronize()
    out = dict(label=lab.cpu().numpy(), emission=emi.cpu().numpy(), results=results, counters=counters, off=off, seg=seg,
               chains=lambda s: seg.chains(s, len(segments[s][0])))
    return out


def rows(out, s):
    a, b = int(out["off"][s]), int(out["off"][s + 1])
    return out["label"][a:b], out["emission"][a:b]


def check_case(out, s, name, contract, energy, labels, emissions, cfg):
    """segment s of a call against the restatement of (energy, labels, emissions, cfg)"""
    r = restated(name, contract) if name else lr.segment(energy, labels, emissions, contract=contract, **cfg)
    got, (lab, emi) = out["results"][s], rows(out, s)
    if r["M"] is not None:   # the handle's debug read: the chains' bits are the sequential chain's
        m, q = out["chains"](s)
        assert np.array_equal(bits(m), bits(r["M"])) and np.array_equal(bits(q), bits(r["Q"])), name
    if r["decided"]:
        assert got["reason"] == r["reason"], (name, got, lr.REASONS[r["reason"]])
        assert (got["speech_begin"], got["speech_end"]) == (r["begin"], r["end"]), (name, got, r["begin"], r["end"])
        assert np.array_equal(lab, r["label"]) and np.array_equal(emi, r["emission"]), name
        if r["score"] == lr.DBL_MAX or got["score"] == lr.DBL_MAX:
            assert got["score"] == r["score"], (name, got["score"], r["score"])
        else:
            S = lr.score_of(energy, r["begin"], r["end"], contract=contract, **cfg)[1]
            print("%s %s: score %r, restated %r, |d| / S = %.3g" % (name, contract, got["score"], r["score"], abs(got["score"] - r["score"]) / S))
            assert abs(got["score"] - r["score"]) <= lr.SCORE_MARGIN * S, (name, got["score"], r["score"], S)
        return
    # undecided (tie_* only): the device's delimitation is as good as the restatement's, and everything behind it is exact
    assert lr.is_tie(name), name
    b, e = got["speech_begin"], got["speech_end"]
    assert 0 <= b <= e < len(energy)
    x, S = lr.score_of(energy, b, e, contract=contract, **cfg)
    S = max(S, lr.score_of(energy, r["begin"], r["end"], contract=contract, **cfg)[1])
    print("%s %s: device (%d, %d) restated (%d, %d), restated scores %r %r, device score %r" % (name, contract, b, e, r["begin"], r["end"], x, r["score"],
                                                                                              got["score"]))
    assert x == r["score"] or abs(x - r["score"]) <= lr.MARGIN * S, (name, x, r["score"], S)
    assert got["score"] == x or abs(got["score"] - x) <= lr.SCORE_MARGIN * S, (name, got["score"], x)
    reason, want_lab, want_emi = lr.spread(len(energy), b, e, labels, emissions)
    assert got["reason"] == reason and np.array_equal(lab, want_lab) and np.array_equal(emi, want_emi), name


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", sorted(lr.cases()))
def test_every_fixture_case(cctx, name, contract):
    c = lr.cases()[name]
    cctx.set_contract(contract)
    out = call(cctx, [(c["energy"], c["labels"], c["emissions"])], **c["cfg"])
    check_case(out, 0, name, contract, c["energy"], c["labels"], c["emissions"], c["cfg"])
    r = out["results"][0]
    assert out["counters"] == tuple(int(i == r["reason"]) for i in range(lr.N_REASONS))
    assert not (out["label"] == SENTINEL).any() and not (out["emission"] == SENTINEL).any()


MIXED = ("d_n1", "d_n2", "d_n64", "d_n65", "d_n4097", "d_n129", "d_n5", "d_n63")


def everything(out, s):
    r = out["results"][s]
    m, q = out["chains"](s)
    return (r["reason"], r["speech_begin"], r["speech_end"], bits(np.float64(r["score"])).tolist(), rows(out, s)[0].tolist(), rows(out, s)[1].tolist(),
            bits(m).tolist(), bits(q).tolist())


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_batching_and_history_change_no_bit(cctx, contract):
    """a segment alone, in a batch of eight mixed lengths, and after an unrelated call on the same handle"""
    import rasr_amd
    cctx.set_contract(contract)
    cs = lr.cases()
    segs = [(cs[n]["energy"], cs[n]["labels"], cs[n]["emissions"]) for n in MIXED]
    batch = call(cctx, segs, front=3)
    assert batch["counters"][lr.OK] + batch["counters"][lr.MISMATCH] == len(MIXED)
    assert (batch["label"][:3] == SENTINEL).all() and (batch["emission"][:3] == SENTINEL).all()
    seg = rasr_amd.LinearSegmenter(cctx)
    for s, n in enumerate(MIXED):
        alone = call(cctx, [segs[s]])
        assert everything(alone, 0) == everything(batch, s), n
        check_case(batch, s, n, contract, *segs[s], cs[n]["cfg"])
        if n in ("d_n65", "d_n4097", "d_n1"):
            call(cctx, [segs[(s + 3) % len(segs)], (lr.track(300, 77), *lr.states(9))], seg=seg)      # an unrelated call
            assert everything(call(cctx, [segs[s]], seg=seg), 0) == everything(batch, s), n
    back = call(cctx, segs[::-1], front=0)
    for s, n in enumerate(MIXED):
        assert everything(back, len(MIXED) - 1 - s) == everything(batch, s), n


def test_strided_energy_column(cctx):
    """the energy as column 5 of a [rows x 40] feature matrix whose first segment starts at row 4 equals the packed call"""
    cs = lr.cases()
    segs = [(cs[n]["energy"], cs[n]["labels"], cs[n]["emissions"]) for n in ("d_n65", "d_n3", "d_n129")]
    packed = call(cctx, segs)
    strided = call(cctx, segs, front=4, column=(40, 5))
    assert (strided["label"][:4] == SENTINEL).all()
    for s in range(3):
        assert everything(strided, s) == everything(packed, s)
    assert strided["results"][0]["reason"] == lr.OK and strided["results"][0]["speech_begin"] > 0


def test_every_reason_once_at_its_smallest_shape(cctx):
    e = lr.track(8, 41)
    lab, emi = lr.states(4)
    nan = e[:2].copy()
    nan[1] = np.nan
    segs = [(e[:3], lab[:3], emi[:3]),        # OK: (0, 1), indices 0, 2, then silence
            (e[:1], lab[:1], emi[:1]),        # TOO_SHORT
            (e[:5], lab[:1], emi[:1]),        # TOO_LONG
            (e[:2], lab[:0], emi[:0]),        # NO_STATES: no states
            (e[:0], lab[:2], emi[:2]),        # NO_STATES: no frames
            (e[:3], lab[:4], emi[:4]),        # JUMP: one step from index 0 to 3
            (e[:2], lab[:2], emi[:2]),        # MISMATCH: (0, 0), the only frame takes index 0 of 2 states
            (nan, lab[:1], emi[:1])]          # NONFINITE
    cfg = dict(minimum_segment_length=2, maximum_segment_length=4)
    out = call(cctx, segs, front=2, **cfg)
    want = [lr.OK, lr.TOO_SHORT, lr.TOO_LONG, lr.NO_STATES, lr.NO_STATES, lr.JUMP, lr.MISMATCH, lr.NONFINITE]
    assert [r["reason"] for r in out["results"]] == want
    assert out["counters"] == tuple(want.count(r) for r in range(lr.N_REASONS)) and sum(out["counters"]) == len(segs)
    for s, (seg, reason) in enumerate(zip(segs, want)):
        r = lr.segment(*seg, **cfg)
        assert r["reason"] == reason and r["decided"]
        l, m = rows(out, s)
        assert np.array_equal(l, r["label"]) and np.array_equal(m, r["emission"])
        assert (l == -1).all() and (m == -1).all() if reason != lr.OK else (l >= 0).all() and (m >= 0).all()
        assert (out["results"][s]["speech_begin"], out["results"][s]["speech_end"]) == (r["begin"], r["end"])
    assert rows(out, 0)[0].tolist() == [int(lab[0]), int(lab[2]), lr.SILENCE_LABEL]
    assert (out["label"][:2] == SENTINEL).all() and (out["emission"][:2] == SENTINEL).all()


def test_values_that_are_not_finite(cctx):
    """NaN, +inf, -inf and a Q_ that leaves the finite range give NONFINITE; the other segments of the batch are untouched.  Energies are
    f32, so with penalty 0 no Q_ can overflow (x * x <= 1.2e77); a penalty of 1e-290 divides it out of range."""
    cs = lr.cases()
    good = [(cs[n]["energy"], cs[n]["labels"], cs[n]["emissions"]) for n in ("d_n65", "d_n129")]
    lab, emi = lr.states(3)
    for cfg, bad in ((dict(), np.nan), (dict(), np.inf), (dict(), -np.inf), (dict(penalty=1e-290), 3e38)):
        x = lr.track(300, 43)
        x[257] = bad                                  # not a frame of the lane that runs the chain
        if cfg:
            x[:] = bad
        segs = [good[0], (x, lab, emi), good[1]]
        out = call(cctx, segs, **cfg)
        assert [r["reason"] for r in out["results"]] == [lr.OK, lr.NONFINITE, lr.OK], (bad, out["results"])
        assert out["counters"][lr.NONFINITE] == 1 and out["counters"][lr.OK] == 2
        assert (rows(out, 1)[0] == -1).all() and (rows(out, 1)[1] == -1).all()
        assert lr.segment(x, lab, emi, **cfg)["reason"] == lr.NONFINITE
        for s in (0, 2):
            alone = call(cctx, [segs[s]], **cfg)
            assert everything(alone, 0) == everything(out, s)
    # the largest finite energies stay finite with the default penalty
    out = call(cctx, [(np.full(40, 3.4e38, np.float32), lab, emi)])
    assert out["results"][0]["reason"] == lr.OK


def test_refusals_launch_nothing(cctx):
    import torch

    import rasr_amd
    from rasr_amd import _lib
    with pytest.raises(rasr_amd.AmxError, match="minimum_speech_proportion"):
        rasr_amd.LinearSegmenter(cctx, minimum_speech_proportion=2.0)
    seg = rasr_amd.LinearSegmenter(cctx)
    e = torch.from_numpy(lr.track(40, 44)).cuda()
    lab = torch.full((40,), SENTINEL, dtype=torch.int32, device="cuda")
    emi = torch.full((40,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = rasr_amd.LinearSegmenter.models([lr.states(3), lr.states(2)], lr.SILENCE_LABEL, lr.SILENCE_EMISSION)
    for off, models, ld, word in (([0, 25, 20], good, 1, "frame offsets decrease at segment 1"),
                                  ([-1, 20, 40], good, 1, "negative frame offset"),
                                  ([0, 20, 40], dict(good, state_label=np.array([1, 2, -5, 4, 5], np.int32)), 1, "state_label[2] = -5"),
                                  ([0, 20, 40], dict(good, state_emission=np.array([1, 2, 3, -4, 5], np.int32)), 1, "state_emission[3] = -4"),
                                  ([0, 20, 40], dict(good, silence_label=-1), 1, "silence_label -1"),
                                  ([0, 20, 40], good, 0, "energy_ld 0")):
        with pytest.raises(rasr_amd.AmxError, match=word.replace("[", r"\[").replace("]", r"\]")) as err:
            seg.align(off, models, e, ld, lab, emi)
        assert err.value.status == _lib.AMX_ERR_INVALID
        torch.cuda.synchronize()
        assert (lab == SENTINEL).all().item() and (emi == SENTINEL).all().item()
    _, _, results, counters = seg.align([0, 20, 40], good, e, 1, lab, emi)      # the handle still works
    assert sum(counters) == 2 and not (lab == SENTINEL).any().item()


def test_flat_start_end_to_end(cctx):
    """synthetic features whose column 0 is the energy -> amx_linseg_align_dev -> amx_gmm_accumulate_dev on a one-density-per-mixture model
    (a zero best-density vector, best_density_ld = 0) -> amx_gmm_estimate: the first model of a training.  The labels never leave the
    device.  The statistics equal the reference's over the restatement's labels at the bar of tests/test_gmm_train_gpu.py for Viterbi
    statistics (counts exactly; rtol=1e-12, atol=1e-9 for f64 sums whose order the device picks), the means and variances numpy's at the
    bar of tests/test_estimate.py::test_estimate_recovers_moments."""
    import torch

    import rasr_amd
    dim, n_mix, per_segment = 8, 7, (150, 131, 200)
    rng = np.random.Generator(np.random.PCG64(51))
    model = synth.gmm_cart(n_mix, 1, 1, dim, seed=52, pooled=False)
    state_mean = rng.standard_normal((n_mix, dim)) * 3
    segs, feats, flat = [], [], []
    for s, n in enumerate(per_segment):
        emi = np.array([1 + (s + i) % (n_mix - 1) for i in range(5 + s)], np.int32)   # emission 0 is silence
        lab = 100 + 10 * s + np.arange(len(emi), dtype=np.int32)
        a, b = int(0.15 * n), int(0.85 * n)
        x = rng.standard_normal((n, dim))
        x[:, 0] = rng.normal(2.0, 0.5, n)
        x[a:b, 0] = rng.normal(8.0, 1.5, b - a)
        # the other columns are drawn per state of the speech part, silence around it
        st = np.zeros(n, np.int64)
        st[a:b] = emi[np.minimum((np.arange(b - a) * len(emi)) // (b - a), len(emi) - 1)]
        x[:, 1:] += state_mean[st, 1:]
        x = x.astype(np.float32)
        feats.append(x)
        segs.append((x[:, 0].copy(), lab, emi))
    x = np.concatenate(feats)
    T = len(x)
    off = np.cumsum([0] + list(per_segment))
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    seg = rasr_amd.LinearSegmenter(cctx)
    models = rasr_amd.LinearSegmenter.models([(s[1], s[2]) for s in segs], lr.SILENCE_LABEL, lr.SILENCE_EMISSION)
    label_dev, emission_dev, results, counters = seg.align(off, models, xd[:, 0], dim)
    assert counters[lr.OK] == len(segs)
    want_emission = []
    for (e, lab, emi), r in zip(segs, results):
        w = lr.segment(e, lab, emi)
        assert w["decided"] and w["reason"] == lr.OK and (r["speech_begin"], r["speech_end"]) == (w["begin"], w["end"])
        want_emission.append(w["emission"])
    want_emission = np.concatenate(want_emission)
    sc = rasr_amd.GmmFeatureScorer(cctx, model)
    acc = torch.zeros(sc.accumulator_size(), dtype=torch.float64, device="cuda")
    zero = torch.zeros(T, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sc.accumulate_dev(xd, T, emission_dev, zero, 0, acc)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    assert np.array_equal(emission_dev.cpu().numpy(), want_emission)
    want = tr.accumulate(model, x, want_emission, np.zeros(T, np.uint32))
    assert np.array_equal(got[:n_mix], want[:n_mix]) and got[:n_mix].sum() == T and got[:n_mix].min() >= 10
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9), np.abs(got - want).max()
    new = rasr_amd.gmm_estimate(model, got)
    x64 = x.astype(np.float64)
    mu = np.stack([x64[want_emission == m].mean(0) for m in range(n_mix)])
    var = np.stack([(x64[want_emission == m] ** 2).mean(0) - mu[m] ** 2 for m in range(n_mix)])
    assert np.allclose(new["means"], mu, rtol=1e-6, atol=1e-6) and np.allclose(new["variances"], var, rtol=1e-5)
