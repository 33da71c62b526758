"""GPU parity: amx_ebw_accumulate_dev (ebw.hip) against the restatement of tests/ebw_reference.py in the library's key order, in every bit of
the flat buffer, in both contracts.

The problem is the smallest on which the kernels can go wrong: segments of 7, 5 (no arcs), 40 and 300 frames, 600 arcs whose weights are
spread over 20 binary exponents (any other order of addition changes bits), keys fed by three and more arcs, the same (frame, mixture) on
both sides, a frame with more than 256 items (a sort chunk), a density with more than 256 keys (several stages of a chain and a last one that is not full), arcs exactly at the
threshold, arcs without items.  Dimensions 1, 39 and 65; one covariance per density and one pooled covariance."""
import numpy as np
import pytest

from tests import ebw_reference as er
from tests import synth

pytestmark = pytest.mark.gpu

LENS = (7, 5, 40, 300)          # segment 1 has no arcs
ARCS = (30, 0, 120, 450)
KS = (1, 5, 3, 2, 4, 5)         # densities per mixture: mixture 0 has one, so every key of mixture 0 lands in one list
N_MIX = len(KS)
BUSY = 17                       # the frame of segment 3 that more than 256 items name


@pytest.fixture()
def cctx(ctx):
    """the session context on torch's stream, handed out in contract=off and restored to it"""
    ctx.use_torch_stream()
    ctx.set_contract("off")
    yield ctx
    ctx.set_contract("off")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def lattice(seed, lens=LENS, n_arcs=ARCS):
    """(arc_offsets, arc_weight, item_offsets, item_frame, item_emission) for segments of the given lengths"""
    rng = np.random.Generator(np.random.PCG64(seed))
    arc_off, w, item_off, fr, em = [0], [], [0], [], []
    for s, (n, a) in enumerate(zip(lens, n_arcs)):
        for i in range(a):
            length = int(rng.integers(0, min(n, 12) + 1)) if i % 9 else 0          # every ninth arc has no items
            start = int(rng.integers(0, n - length + 1))
            if n == 300 and i < 340 and length:                                      # most of 340 arcs over the busy frame
                start = BUSY - int(rng.integers(0, length))
            if n == 300 and 340 <= i < 370:                                          # numerator arcs of mixture 0 that tile the segment
                length, start = 10, (i - 340) * 10
            e = rng.integers(0, N_MIX, 2)
            frames = np.arange(start, start + length)
            emis = np.where(frames < start + length // 2, e[0], e[1])
            mag = float(rng.uniform(1.0, 2.0)) * 2.0 ** -int(rng.integers(0, 20))
            sign = 1.0 if rng.random() < 0.5 else -1.0
            if n == 300 and 340 <= i < 370:
                emis[:], sign = 0, 1.0
            if i % 50 == 3:
                mag = float(er.EPSILON)                                              # exactly at the threshold: neither side
            if i % 50 == 4:
                mag = float(np.nextafter(er.EPSILON, np.float32(1)))                 # the first weight that counts
            if n == 7 and i >= 27:
                # three numerator arcs on one key, 33 binary exponents apart: a + b and (a + b) + c are ties that round to even, b + c is
                # exact and one ulp of a.  The widened f32 weights of the other keys add without rounding in any order; these do not
                frames, emis, sign = np.array([2]), np.array([3]), 1.0
                mag = 1024.0 * (1 + 2.0 ** -23) if i == 27 else 2.0 ** -22 * (1 + 2.0 ** -21)
            w.append(sign * mag)
            fr.extend(frames)
            em.extend(emis)
            item_off.append(len(fr))
        arc_off.append(len(w))
    return (np.array(arc_off, np.int64), np.array(w, np.float32), np.array(item_off, np.int64), np.array(fr, np.int32), np.array(em, np.int32))


def problem(D, pooled, seed=5):
    rng = np.random.Generator(np.random.PCG64(seed + D))
    model = synth.gmm_cart(N_MIX, 1, 5, D, seed=seed, pooled=pooled, ks=KS)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64) + 3               # three rows in front of the first segment
    feats = (rng.standard_normal((int(off[-1]) + 2, D + 3)) * 1.5 + 0.5).astype(np.float32)   # a leading dimension above D
    lat = lattice(seed)
    return dict(model=model, D=D, feats=feats, frame_offsets=off, lattice=lat)


def device(cctx, p, contract, calls=None, feats=None, acc0=None, threshold=None):
    """accumulate `calls` (lists of (frame_offsets, lattice)); returns (accumulator, buffer, best densities [rows, n_mix])"""
    import torch

    import rasr_amd
    cctx.set_contract(contract)
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    ebw = rasr_amd.EbwAccumulator(gmm, weight_threshold=threshold)
    feats = p["feats"] if feats is None else feats
    xd = torch.from_numpy(feats).cuda()
    acc = torch.zeros(ebw.accumulator_size(), dtype=torch.float64, device="cuda") if acc0 is None else torch.from_numpy(acc0).cuda()
    for off, lat in ([(p["frame_offsets"], p["lattice"])] if calls is None else calls):
        ebw.accumulate_dev(xd, feats.shape[1], off, *lat, acc)
    torch.cuda.synchronize()
    dense = torch.from_numpy(np.ascontiguousarray(feats[:, :p["D"]])).cuda()
    T = dense.shape[0]
    scores = torch.zeros((T, N_MIX), dtype=torch.float32, device="cuda")
    best = torch.zeros((T, N_MIX), dtype=torch.int32, device="cuda")
    gmm.score_dev(dense, T, scores, best)
    torch.cuda.synchronize()
    return ebw, acc.cpu().numpy(), best.cpu().numpy().view(np.uint32), gmm


def restate(p, best, contract, off=None, lat=None, acc=None, order="device", defect=None, feats=None):
    off = p["frame_offsets"] if off is None else off
    keys = er.collect(off, *(p["lattice"] if lat is None else lat), defect=defect)
    feats = p["feats"] if feats is None else feats
    t0 = int(off[0])
    return er.accumulate(p["model"], feats[t0:, :p["D"]], best[t0:], keys, order, contract, acc, defect), keys


def segment_call(p, s, lat=None, off=None):
    """segment s alone: its offsets and its arcs"""
    a_off, w, i_off, fr, em = p["lattice"] if lat is None else lat
    off = p["frame_offsets"] if off is None else off
    a0, a1 = int(a_off[s]), int(a_off[s + 1])
    i0, i1 = int(i_off[a0]), int(i_off[a1])
    return off[s:s + 2], (np.array([0, a1 - a0], np.int64), w[a0:a1], i_off[a0:a1 + 1] - i0, fr[i0:i1], em[i0:i1])


def test_the_problem_holds_what_it_is_for():
    p = problem(1, False)
    a_off, w, i_off, fr, em = p["lattice"]
    keys = er.collect(p["frame_offsets"], *p["lattice"])
    fed = {}
    for s in range(len(LENS)):
        for a in range(a_off[s], a_off[s + 1]):
            if er.side_of(w[a]) >= 0:
                for i in range(i_off[a], i_off[a + 1]):
                    k = (er.side_of(w[a]), s, fr[i], em[i])
                    fed[k] = fed.get(k, 0) + 1
    assert len(w) == 600 and max(fed.values()) >= 3
    assert any((1 - side, s, f, m) in fed for (side, s, f, m) in fed)                    # both sides of one (frame, mixture)
    busy = int(np.sum((fr == BUSY) & (np.repeat(np.arange(len(w)), np.diff(i_off)) >= a_off[3])))
    assert busy > 256
    assert sum(1 for k in keys if k["mixture"] == 0 and k["side"] == er.NUM) > 256      # mixture 0 has one density: one list
    assert np.any(np.abs(w) == er.EPSILON) and np.any(np.diff(i_off) == 0) and a_off[1] == a_off[2]
    fwd = {(k["side"], k["frame"], k["mixture"]): k["weight"] for k in keys}
    rev = {(k["side"], k["frame"], k["mixture"]): k["weight"] for k in er.collect(p["frame_offsets"], *p["lattice"], defect="reversed-arcs")}
    assert fwd.keys() == rev.keys() and [k for k in fwd if fwd[k] != rev[k]] == [(er.NUM, 2, 3)]   # the one key whose collection rounds
    exps = np.unique(np.frexp(np.abs(w[np.abs(w) > 1e-6]))[1])
    assert len(exps) >= 20


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("D", [1, 39, 65])
def test_accumulation_equals_the_restatement_in_every_bit(cctx, D, pooled, contract):
    p = problem(D, pooled)
    ebw, got, best, _ = device(cctx, p, contract)
    want, keys = restate(p, best, contract)
    o = er.layout(p["model"])
    assert ebw.accumulator_size() == o["size"] and all(getattr(ebw.layout, k) == v for k, v in o.items())
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
    assert want[o["den_density_weights"]:o["objective"]].any() and want[:o["den_density_weights"]].any()
    # the collected weights have one right value: the device's keys are the restatement's, in ascending (frame, mixture, side)
    lk = ebw.last_keys()
    ordered = [keys[i] for i in er.key_order(keys, "device")]
    assert len(lk["frame"]) == len(ordered)
    assert np.array_equal(lk["frame"], [k["frame"] for k in ordered]) and np.array_equal(lk["mixture"], [k["mixture"] for k in ordered])
    assert np.array_equal(lk["side"], [k["side"] for k in ordered])
    assert np.array_equal(bits(lk["weight"]), bits([k["weight"] for k in ordered]))
    # the other order of addition and the other arithmetic are other bits: the comparison above can tell them apart
    assert not np.array_equal(bits(restate(p, best, contract, order=er.key_order(keys, "device")[::-1])[0]), bits(want))
    if D > 1:
        assert not np.array_equal(bits(restate(p, best, "fma" if contract == "off" else "off")[0]), bits(want))
    # the views by name
    assert np.array_equal(ebw.view(got, "den_mean_sums").reshape(-1), got[o["den_mean_sums"]:o["den_cov_weights"]])
    assert ebw.view(got, "num_cov_sums").shape == (p["model"]["variances"].shape[0], D)


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_calls_and_batches_give_the_same_bits(cctx, contract):
    p = problem(39, False)
    _, whole, best, _ = device(cctx, p, contract)
    # the corpus cut into calls between segments, and every segment in a call of its own
    off, (a_off, w, i_off, fr, em) = p["frame_offsets"], p["lattice"]
    a2, i2 = int(a_off[2]), int(i_off[a_off[2]])
    first = (off[:3], (a_off[:3], w[:a2], i_off[:a2 + 1], fr[:i2], em[:i2]))
    second = (off[2:], (a_off[2:] - a2, w[a2:], i_off[a2:] - i2, fr[i2:], em[i2:]))
    _, cut, _, _ = device(cctx, p, contract, calls=[first, second])
    assert np.array_equal(bits(cut), bits(whole))
    _, single, _, _ = device(cctx, p, contract, calls=[segment_call(p, s) for s in range(len(LENS))])
    assert np.array_equal(bits(single), bits(whole))
    # a segment alone gives the bits it gives in another slot of another batch: the segments' rows and arcs moved to other slots
    perm = [3, 0, 2, 1]
    lens = [LENS[s] for s in perm]
    poff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pfeats = np.concatenate([p["feats"][off[s]:off[s + 1]] for s in perm])
    parts = [segment_call(p, s)[1] for s in perm]
    plat = (np.concatenate([[0], np.cumsum([len(q[1]) for q in parts])]).astype(np.int64), np.concatenate([q[1] for q in parts]),
            np.concatenate([[0], np.cumsum(np.concatenate([np.diff(q[2]) for q in parts]))]).astype(np.int64),
            np.concatenate([q[3] for q in parts]), np.concatenate([q[4] for q in parts]))
    _, moved, pbest, _ = device(cctx, p, contract, calls=[(poff, plat)], feats=pfeats)
    want, _ = restate(p, pbest, contract, off=poff, lat=plat, feats=pfeats)
    assert np.array_equal(bits(moved), bits(want))
    for slot, s in enumerate(perm):
        _, alone, _, _ = device(cctx, p, contract, calls=[segment_call(p, s)])
        _, alone_moved, _, _ = device(cctx, p, contract, calls=[segment_call(p, slot, plat, poff)], feats=pfeats)
        assert np.array_equal(bits(alone), bits(alone_moved))
        assert alone.any() == (ARCS[s] > 0)


def test_every_planted_defect_leaves_the_device_bits(cctx):
    p = problem(39, False)
    _, got, best, _ = device(cctx, p, "off")
    for defect in er.DEFECTS:
        bad, _ = restate(p, best, "off", defect=defect)
        assert not np.array_equal(bits(bad), bits(got)), defect
    # at the threshold itself: an arc of exactly epsilon counts for neither side, the next f32 counts
    one = (np.array([0, 2], np.int64), np.array([er.EPSILON, -er.EPSILON], np.float32), np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32),
           np.array([1, 1], np.int32))
    _, at, _, _ = device(cctx, p, "off", calls=[(p["frame_offsets"][:2], one)])
    assert not at.any()
    up = np.nextafter(er.EPSILON, np.float32(1))
    _, above, _, _ = device(cctx, p, "off", calls=[(p["frame_offsets"][:2], (one[0], np.array([up, -up], np.float32)) + one[2:])])
    o = er.layout(p["model"])
    assert above[o["num_mean_weights"]:o["num_mean_sums"]].sum() == float(up) and above[o["den_mean_weights"]:o["den_mean_sums"]].sum() == float(up)
    assert above[:o["num_mean_weights"]].sum() == float(up) and above[o["den_density_weights"]:o["den_mean_weights"]].sum() == float(up)
    _, low, _, _ = device(cctx, p, "off", calls=[(p["frame_offsets"][:2], one)], threshold=1e-8)
    assert low[o["num_mean_weights"]:o["num_mean_sums"]].sum() == float(er.EPSILON)


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_fixture_cases_collected_weights_and_bar(cctx, contract):
    """tests/golden/ref_ebw.npz (the reference's own text, both builds): the device's collected weights are the fixture's in every bit;
    the buffer, with the scorer's densities in place of the fixture's, is the restatement's in the library's order"""
    from tests import test_ebw as te
    for name in te.CASES:
        c = te.load_case(name)
        p = dict(model=c["model"], D=c["model"]["dim"], feats=c["feats"], frame_offsets=c["frame_offsets"], lattice=c["lat"])
        ebw, got, best, _ = device(cctx, p, contract)
        keys = er.collect(c["frame_offsets"], *c["lat"])
        order = te.Z["%s/%s/order" % (name, contract)]
        want = {(keys[i]["side"], keys[i]["frame"], keys[i]["mixture"]): w for i, w in zip(order, te.Z["%s/%s/weights" % (name, contract)])}
        lk = ebw.last_keys()
        assert len(lk["frame"]) == len(want)
        assert np.array_equal(bits(lk["weight"]), bits([want[(s, f, m)] for s, f, m in zip(lk["side"], lk["frame"], lk["mixture"])]))
        assert np.array_equal(bits(got), bits(er.accumulate(c["model"], c["feats"], best, keys, "device", contract)))


def test_refused_inputs_leave_the_buffer_untouched(cctx):
    import torch

    import rasr_amd
    from rasr_amd import _lib
    p = problem(39, False)
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    ebw = rasr_amd.EbwAccumulator(gmm)
    mark = np.arange(ebw.accumulator_size(), dtype=np.float64) * 0.5 + 1.0
    acc = torch.from_numpy(mark.copy()).cuda()
    off, (a_off, w, i_off, fr, em) = p["frame_offsets"], p["lattice"]
    ld = p["feats"].shape[1]
    items_of_sided = np.repeat(np.array([er.side_of(v) >= 0 for v in w]), np.diff(i_off))
    seg_of_item = np.searchsorted(a_off, np.repeat(np.arange(len(w)), np.diff(i_off)), side="right") - 1

    def refused(match, feats=p["feats"], w=w, fr=fr, em=em):
        with pytest.raises(rasr_amd.AmxError, match=match) as e:
            ebw.accumulate_dev(torch.from_numpy(feats).cuda(), ld, off, a_off, w, i_off, fr, em, acc)
        assert e.value.status == _lib.AMX_ERR_INVALID
        torch.cuda.synchronize()
        assert np.array_equal(bits(acc.cpu().numpy()), bits(mark))

    last = len(fr) - 1                                           # an item of the last segment
    for f in (LENS[3], -1):
        bad = fr.copy()
        bad[last] = f
        refused("item %d: frame %d is outside its segment" % (last, f), fr=bad)
    first0 = int(np.nonzero(seg_of_item == 0)[0][0])
    bad = fr.copy()
    bad[first0] = LENS[0]                                        # a frame of the next segment
    refused("item %d: frame %d is outside its segment" % (first0, LENS[0]), fr=bad)
    for e_bad in (N_MIX, -1):
        bad = em.copy()
        bad[5] = e_bad
        refused("item 5: emission index %d is outside" % e_bad, em=bad)
    empty = int(np.nonzero(np.diff(i_off) == 0)[0][0])
    for v in (np.nan, np.inf):
        bad = w.copy()
        bad[empty] = v                                           # an arc without items
        refused("arc %d: non-finite weight" % empty, w=bad)
    touched = np.zeros(p["feats"].shape[0], bool)
    touched[off[seg_of_item[items_of_sided]] + fr[items_of_sided]] = True
    t_bad = int(np.nonzero(touched)[0][-1])
    x = p["feats"].copy()
    x[t_bad, p["D"] - 1] = np.nan
    refused("frame %d: non-finite feature" % t_bad, feats=x)
    # a NaN where no item of an arc with a side looks: the rows in front of the first segment, the segment without arcs, the padding
    x = p["feats"].copy()
    x[0, 0] = x[off[1] + 2, 3] = x[5, p["D"]] = np.nan
    assert not touched[0] and not touched[off[1] + 2]
    ebw.accumulate_dev(torch.from_numpy(x).cuda(), ld, off, a_off, w, i_off, fr, em, acc)
    torch.cuda.synchronize()
    assert not np.array_equal(bits(acc.cpu().numpy()), bits(mark)) and np.isfinite(acc.cpu().numpy()).all()
    with pytest.raises(rasr_amd.AmxError, match="viterbi") as e:
        rasr_amd.EbwAccumulator(gmm, viterbi=False)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED


def test_the_objective_is_widened_and_added_to_the_last_cell(cctx):
    import torch

    import rasr_amd
    p = problem(1, True)
    ebw = rasr_amd.EbwAccumulator(rasr_amd.GmmFeatureScorer(cctx, p["model"]))
    acc = torch.zeros(ebw.accumulator_size(), dtype=torch.float64, device="cuda")
    want = np.zeros(ebw.accumulator_size())
    for v in (0.1, -3.25e-3, 7.0):
        ebw.accumulate_objective(v, acc)
        er.accumulate_objective(p["model"], want, v)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and got[-1] != 0.1 - 3.25e-3 + 7.0 and ebw.view(got, "objective")[0] == got[-1]


def test_the_loop_on_the_device_ends_in_a_scorer_and_the_zero_denominator_is_the_ml_estimate(cctx):
    """amx_gmm_score_dev -> the best-scoring mixture of every frame (the Viterbi path of an ergodic graph) as numerator arcs, one per run,
    plus competitor arcs on perturbed labels as denominator -> amx_ebw_accumulate_dev -> amx_ebw_estimate -> amx_gmm_create -> score.
    With no denominator arc and the iteration constants at their floor the EBW means are amx_gmm_estimate's within one f32 rounding:
    (sum + D * previous) / (weight + D) with D of the order 1e-30 is sum / weight in f64, and both are narrowed once"""
    import torch

    import rasr_amd
    D = 5
    rng = np.random.Generator(np.random.PCG64(3))
    model = synth.gmm_cart(N_MIX, 1, 5, D, seed=11, pooled=False, ks=KS)
    owner = np.repeat(np.arange(N_MIX), KS)
    rows = np.repeat(np.arange(sum(KS)), 12)                                    # twelve frames from every density, in runs
    feats = (model["means"][rows] + rng.standard_normal((len(rows), D)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    T = len(rows)
    gmm = rasr_amd.GmmFeatureScorer(cctx, model)
    xd = torch.from_numpy(feats).cuda()
    scores = torch.zeros((T, N_MIX), dtype=torch.float32, device="cuda")
    gmm.score_dev(xd, T, scores, None)
    torch.cuda.synchronize()
    label = scores.cpu().numpy().argmin(axis=1)
    assert (label == owner[rows]).mean() > 0.5                                  # most frames go where they were drawn from
    starts = np.concatenate([[0], np.nonzero(np.diff(label))[0] + 1, [T]])
    num = [(int(a), int(b), int(label[a]), 1.0) for a, b in zip(starts[:-1], starts[1:])]
    den = [(a, b, int((m + 1 + i) % N_MIX), -0.4) for i, (a, b, m, _) in enumerate(num)]

    def lattice_of(arcs):
        w = np.array([a[3] for a in arcs], np.float32)
        i_off = np.concatenate([[0], np.cumsum([a[1] - a[0] for a in arcs])]).astype(np.int64)
        fr = np.concatenate([np.arange(a[0], a[1]) for a in arcs]).astype(np.int32)
        em = np.concatenate([np.full(a[1] - a[0], a[2]) for a in arcs]).astype(np.int32)
        return np.array([0, len(arcs)], np.int64), w, i_off, fr, em

    ebw = rasr_amd.EbwAccumulator(gmm)
    o = er.layout(model)
    out = {}
    for name, arcs in (("both", num + den), ("numerator", num)):
        acc = torch.zeros(ebw.accumulator_size(), dtype=torch.float64, device="cuda")
        ebw.accumulate_dev(xd, D, np.array([0, T], np.int64), *lattice_of(arcs), acc)
        ebw.accumulate_objective(-1.5, acc)
        torch.cuda.synchronize()
        out[name] = acc.cpu().numpy()
    assert out["both"][o["den_density_weights"]:o["objective"]].any() and not out["numerator"][o["den_density_weights"]:o["objective"]].any()
    new, info = rasr_amd.EbwEstimator(minimum_observation_weight=0.0).estimate(model, out["both"], model)
    want = er.estimate(model, out["both"], model, None, dict(min_observation_weight=0.0))
    assert new["means"].tobytes() == want["model"]["means"].tobytes() and new["variances"].tobytes() == want["model"]["variances"].tobytes()
    assert np.array_equal(bits(new["log_weight"]), bits(want["model"]["log_weight"]))
    nxt = rasr_amd.GmmFeatureScorer(cctx, new)                                   # the next iteration's scorer
    nxt.score_dev(xd, T, scores, None)
    torch.cuda.synchronize()
    assert np.isfinite(scores.cpu().numpy()).all()
    # the zero denominator
    floor, _ = rasr_amd.EbwEstimator(minimum_observation_weight=0.0, step_size=1e-30, minimum_icd=1e-30).estimate(model, out["numerator"], model)
    ml = rasr_amd.gmm_estimate(model, out["numerator"][:o["den_density_weights"]], min_observation_weight=0.0, allow_zero_weights=1)
    assert np.array_equal(floor["dens_mean"], ml["dens_mean"]) and floor["means"].shape == ml["means"].shape
    seen = out["numerator"][o["num_mean_weights"]:o["num_mean_sums"]] > 0         # a mean without a frame: EBW keeps the previous one, ML writes zeros
    assert seen.sum() >= 10
    a, b = floor["means"][seen].astype(np.float64), ml["means"][seen].astype(np.float64)
    assert (np.abs(a - b) <= 2.0 ** -23 * np.abs(b)).all()
