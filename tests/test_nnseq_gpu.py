"""GPU: amx_nnseq_* (rasr_amd.SegmentwiseNnTrainer: nnseq_score_kernel, the key sort and nnseq_collect_kernel, nnseq_reject_kernel,
nnseq_smooth_kernel, nnseq_reduce_kernel, nnseq_tail_kernel, and nntrain.hip's GEMMs on a batch of segments) against the plain
restatement of tests/nnseq_reference.py.

Shapes.  Network 20-33-17-50, sigmoid then rectified, 60 classes of which ten have no output; segments of 1, 255, 256, 257 and 300
frames (the frame chunk AMX_NNTRAIN_CHUNK from both sides, and two chunks), the features from row 2 of a wider matrix whose other cells
hold NaN.  Arc tables: 13 arcs per segment (65: no multiple of the score kernel's 4 arcs per workgroup), every fifth without items, one
of up to 200 items (more than the 64 a wave stages); item counts one below, at and one above the sort's workgroup (kernel_shape), keys
of 17 bits (three digit passes).

Bars.  Arc scores, the error signal before and after smoothing, the frame weights, the rejected counts, classification errors,
observations and the total weight are compared in every bit (the smoothing on the device's own softmax: its exp is the device
library's).  Gradients and bias gradients are held to the bars tests/golden/make_nnseq_golden.py measured and stored in
tests/golden/ref_nnseq.npz; none is written here."""
import functools
import os

import numpy as np
import pytest

from tests import nnseq_reference as sr
from tests import nntrain_reference as nr

pytestmark = pytest.mark.gpu

F32 = np.float32
LENGTHS, LEAD = sr.GPU_LENGTHS, sr.GPU_LEAD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_nnseq.npz")


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


def batch():
    return sr.gpu_batch()


def flows():
    return sr.gpu_flows()


def trainers(ctx, net, cls=None, **kw):
    import rasr_amd
    ctx.use_torch_stream()
    cls = cls or rasr_amd.FeedForwardTrainer
    tr = cls(ctx, net.Ws, net.bs, net.acts, statistics=("base", "gradient"), class_weights=net.class_weights, class_to_output=net.class_to_output)
    return tr, rasr_amd.SegmentwiseNnTrainer(tr, keep_lattice_error=True, **kw)


def dev(a, view=None):
    import torch
    a = np.array(a)   # a copy: the cached inputs are read-only
    return torch.from_numpy(a if view is None else a.view(view)).cuda()


def run(seq, feats, off, emission, passes, objective=None, skip=None, acc=None, segments=None):
    """forward + accumulate of the segments `segments` (default all) of the batch; -> (host copy of acc, info)"""
    import torch
    segments = list(range(len(off) - 1)) if segments is None else list(segments)
    sub_off = np.array([off[s] for s in segments] + [off[segments[-1] + 1]], np.int64)
    assert all(off[s + 1] == off[t] for s, t in zip(segments, segments[1:])), "consecutive segments only"
    xd = dev(feats)
    seq.forward_dev(xd, feats.shape[1], sub_off)
    sub = []
    for p in passes:
        t = p["tables"]
        a0, a1 = int(t["arc_offsets"][segments[0]]), int(t["arc_offsets"][segments[-1] + 1])
        i0, i1 = int(t["item_offsets"][a0]), int(t["item_offsets"][a1])
        tt = dict(arc_offsets=t["arc_offsets"][segments[0]:segments[-1] + 2] - a0, item_offsets=t["item_offsets"][a0:a1 + 1] - i0,
                  item_frame=t["item_frame"][i0:i1], item_emission=t["item_emission"][i0:i1])
        sub.append(dict(p, tables=tt, arc_weight_dev=dev(np.asarray(p["arc_weight"])[a0:a1] if a1 > a0 else np.zeros(1, F32))))
    ed = dev(np.asarray(emission)[sub_off[0] - off[0]:sub_off[-1] - off[0]], np.int32)
    if acc is None:
        acc = torch.zeros(seq.trainer.accumulator_size(), dtype=torch.float64, device="cuda")
    obj = np.arange(1, len(segments) + 1, dtype=F32) * F32(0.375) if objective is None else np.asarray(objective, F32)
    torch.cuda.synchronize()
    info = seq.accumulate_dev(sub, ed, obj, acc, None if skip is None else [skip[s] for s in segments])
    torch.cuda.synchronize()
    return acc.cpu().numpy(), info


def test_arc_scores_equal_the_chain_on_the_devices_own_output(ctx):
    net, off, feats, emission, den, _, _, _, _ = batch()
    tr, seq = trainers(ctx, net)
    shape = seq.kernel_shape()
    n_arcs = int(den["arc_offsets"][-1])
    assert n_arcs % shape["score_block_arcs"] != 0
    assert np.diff(den["item_offsets"]).max() > shape["score_stage_items"] and (np.diff(den["item_offsets"]) == 0).any()
    seq.forward_dev(dev(feats), feats.shape[1], off)
    got = seq.arc_scores(den).cpu().numpy()
    for s in range(len(LENGTHS)):
        top = seq.top(s)
        want = sr.arc_scores(net, top, den, s)
        a0, a1 = int(den["arc_offsets"][s]), int(den["arc_offsets"][s + 1])
        assert np.array_equal(bits(got[a0:a1]), bits(want)), s
        assert (got[a0:a1][np.diff(den["item_offsets"])[a0:a1] == 0] == 0).all()
        assert seq.workspace_row(s) % 256 == 0
    # the forward pass is the one of the frame-wise trainer: the restatement's output within the GEMM's bar
    _, z = sr.forward(net, feats[off[4]:off[5]])
    assert np.abs(seq.top(4) - z).max() <= 1e-4 * np.abs(z).max()
    seq.close(), tr.close()


@pytest.mark.parametrize("flow", ["mmi", "me", "me-rejection"])
def test_error_signal_weights_and_rejections_in_every_bit(ctx, flow):
    net, off, feats, emission, *_ = batch()
    passes = flows()[flow]
    tr, seq = trainers(ctx, net, frame_rejection_threshold=0.3)
    _, info = run(seq, feats, off, emission, passes)
    want = sr.process(net, feats, off, emission, passes, np.zeros(5, F32), rejection=0.3)
    assert seq.last_shape()["sort_passes"] >= 2
    for s, seg in enumerate(want["segments"]):
        assert np.array_equal(bits(seq.error_signal(s, "lattice")), bits(seg["E_lattice"])), (flow, s)
        assert np.array_equal(bits(seq.weights(s)), bits(seg["w"])), (flow, s)
        assert info["seg_rejected"][s] == seg["rejected"], (flow, s)
        assert np.array_equal(bits(seq.error_signal(s)), bits(seg["E"])), (flow, s)   # lambda = 0: E times w
    assert info["rejected_observations"] == want["info"]["rejected_observations"]
    if flow != "me":
        assert 0 < info["rejected_observations"] < sum(LENGTHS)
    seq.close(), tr.close()


def items_table(net, n_items, T, rng, lead=None):
    """one segment of T frames: arcs of 37 items over consecutive frames (wrapping), n_items in all; lead: (tables, weights) in front"""
    valid = sr.valid_classes(net)[:5]
    io, fr, em = [0], [], []
    while len(fr) < n_items:
        n = min(37, n_items - len(fr))
        b = int(rng.integers(0, T))
        fr.extend((b + np.arange(n)) % T)
        em.extend(rng.choice(valid, n))
        io.append(len(fr))
    io, fr, em = np.array(io, np.int64), np.array(fr, np.int32), np.array(em, np.int32)
    w = (rng.random(len(io) - 1) * 0.5 + 0.25).astype(F32)
    if lead is not None:
        lt, lw = lead
        k = len(lt["item_frame"])
        io = np.concatenate([lt["item_offsets"], io[1:] + k])
        fr, em, w = np.concatenate([lt["item_frame"], fr]), np.concatenate([lt["item_emission"], em]), np.concatenate([lw, w])
    return dict(arc_offsets=np.array([0, len(io) - 1], np.int64), item_offsets=io, item_frame=fr, item_emission=em), w


def test_collection_around_the_sorts_workgroup_and_the_order_sensitive_key(ctx):
    net = sr.network()
    block = __import__("rasr_amd").SegmentwiseNnTrainer.kernel_shape()["sort_block_items"]
    rng = np.random.Generator(np.random.PCG64(12))
    T = 300
    feats = rng.standard_normal((T, 20)).astype(F32)
    off = np.array([0, T], np.int64)
    emission = rng.choice(sr.valid_classes(net), T).astype(np.uint32)
    e0 = int(sr.valid_classes(net)[7])
    lead_t, lead_w, thr = sr.order_case(e0)
    tr, seq = trainers(ctx, net, weight_threshold=thr)
    for n_items in (block - 1, block, block + 1, 2 * block + 5):
        tables, w = items_table(net, n_items - 4, T, rng, lead=(lead_t, lead_w))
        assert len(tables["item_frame"]) == n_items
        passes = [dict(tables=tables, arc_weight=w, factor=1.0)]
        run(seq, feats, off, emission, passes)
        shape = seq.last_shape()
        assert shape["sort_blocks"] == -(-n_items // block) and shape["sort_passes"] >= 2
        want = sr.process(net, feats, off, emission, passes, np.zeros(1, F32), threshold=thr)["segments"][0]
        got = seq.error_signal(0, "lattice")
        assert np.array_equal(bits(got), bits(want["E_lattice"])), n_items
        o = sr.class_to_output(net, e0)
        assert got[0, o] == F32(1.0) and want["E_lattice"][0, o] == F32(1.0)   # arc order; the other order gives 1 + 2^-23
    seq.close(), tr.close()


@pytest.mark.parametrize("prior", [False, True])
def test_smoothing_on_the_devices_softmax_in_every_bit(ctx, prior):
    net, off, feats, emission, *_ = batch()
    passes = flows()["mmi"]
    lam = 0.3
    rng = np.random.Generator(np.random.PCG64(13))
    log_prior = np.log(rng.dirichlet(np.ones(50))).astype(F32) if prior else None
    tr, seq = trainers(ctx, net, ce_smoothing_weight=lam, frame_rejection_threshold=0.3, log_prior=log_prior, prior_scale=0.7 if prior else 0.0)
    xd = dev(feats)
    seq.forward_dev(xd, feats.shape[1], off)
    tops = [seq.top(s) for s in range(5)]
    _, info = run(seq, feats, off, emission, passes)
    ps = [seq.top(s, softmax=True) for s in range(5)]
    want = sr.process(net, feats, off, emission, passes, np.zeros(5, F32), lam=lam, rejection=0.3, log_prior=log_prior, prior_scale=0.7 if prior else 0.0,
                      top=tops, p=ps)
    for s, seg in enumerate(want["segments"]):
        assert np.array_equal(bits(seq.error_signal(s)), bits(seg["E"])), s
        assert info["seg_errors"][s] == seg["errors"], s
        # the CE objective: one logf per frame (1 ulp class on the device) and an f32 chain of T terms
        terms = np.abs(nr.logf(ps[s][np.arange(len(ps[s])), sr.alignment(net, emission[off[s] - LEAD:off[s + 1] - LEAD])]) * seg["w"])
        assert abs(float(info["seg_ce_objective"][s]) - float(seg["ce"])) <= (len(terms) + 4) * float(np.finfo(F32).eps) * float(terms.sum()) + 1e-30, s
        # the device's softmax is the restatement's within the exp's ulp class
        assert np.abs(ps[s] - sr.softmax_of(net, tops[s], log_prior, 0.7 if prior else 0.0)).max() <= 4 * np.finfo(F32).eps
    seq.close(), tr.close()


def test_lambda_one_is_the_frame_wise_trainer_in_every_bit(ctx):
    import torch
    net, off, feats, emission, *_ = batch()
    tr, seq = trainers(ctx, net, ce_smoothing_weight=1.0)
    s = 4
    got, _ = run(seq, feats, off, emission, flows()["mmi"], objective=[1.25], segments=[s])
    tr2, _seq2 = trainers(ctx, net)
    acc = torch.zeros(tr2.accumulator_size(), dtype=torch.float64, device="cuda")
    xd = dev(feats[off[s]:off[s + 1]])
    tr2.accumulate_dev(xd, feats.shape[1], LENGTHS[s], dev(emission[off[s] - LEAD:off[s + 1] - LEAD], np.int32), acc)
    torch.cuda.synchronize()
    want = acc.cpu().numpy()
    tail = tr.layout.tail
    assert got[tail + 3] == 1.25
    want[tail + 3] = 1.25
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert got[tail] == LENGTHS[s] and np.abs(got[:tail]).max() > 0
    _seq2.close(), tr2.close(), seq.close(), tr.close()


@pytest.mark.parametrize("flow,lam", [("mmi", 0.0), ("me-rejection", 0.25)])
def test_gradients_meet_the_measured_bars(ctx, flow, lam):
    net, off, feats, emission, *_ = batch()
    passes, fx = flows()[flow], fixture()
    tr, seq = trainers(ctx, net, ce_smoothing_weight=lam, frame_rejection_threshold=0.3)
    objective = np.linspace(-3, 5, 5).astype(F32)
    got, info = run(seq, feats, off, emission, passes, objective=objective)
    want = sr.process(net, feats, off, emission, passes, objective, lam=lam, rejection=0.3)
    s, ws = tr.statistics(got), want["stats"]
    assert s["n_observations"] == ws["n_observations"] == sum(LENGTHS)
    assert s["objective"] == float(objective.astype(np.float64).sum())
    # the classification errors, exactly, from the device's own top output as it then stands (linear with lambda = 0, else the softmax)
    errors = 0
    for k in range(5):
        top = seq.top(k, softmax=lam > 0)
        wrong = int((nr.arg_max(top) != sr.alignment(net, emission[off[k] - LEAD:off[k + 1] - LEAD])).sum())
        assert info["seg_errors"][k] == wrong, (flow, k)
        errors += wrong
    assert s["n_classification_errors"] == errors and 0 < errors < sum(LENGTHS)
    assert abs(s["total_weight"] - ws["total_weight"]) <= 1e-12 * ws["total_weight"]
    for l in range(tr.n_layers):
        for block in ("gradient_weights", "gradient_bias"):
            bar, ref = float(fx["bar_%s/%s/%d" % (block, flow, l)][0]), ws[block][l]
            devn = np.abs(s[block][l] - ref).max()
            print("%s %s[%d] dev %.3g of %.3g" % (flow, block, l, devn, bar * np.abs(ref).max()))
            assert devn <= bar * np.abs(ref).max(), (flow, block, l)
    seq.close(), tr.close()


def test_batches_single_segments_and_a_skipped_segment_give_the_same_bits(ctx):
    import torch
    net, off, feats, emission, *_ = batch()
    passes = flows()["mmi"]
    tr, seq = trainers(ctx, net, ce_smoothing_weight=0.2, frame_rejection_threshold=0.3)
    objective = np.linspace(-3, 5, 5).astype(F32)
    whole, _ = run(seq, feats, off, emission, passes, objective=objective)
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    for s in range(5):
        single, _ = run(seq, feats, off, emission, passes, objective=objective[s:s + 1], acc=acc, segments=[s])
    assert np.array_equal(single.view(np.uint64), whole.view(np.uint64))
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    run(seq, feats, off, emission, passes, objective=objective[:2], acc=acc, segments=[0, 1])
    other, _ = run(seq, feats, off, emission, passes, objective=objective[2:], acc=acc, segments=[2, 3, 4])
    assert np.array_equal(other.view(np.uint64), whole.view(np.uint64))
    # a skipped segment and one without an alignment add nothing: the batch equals the other segments' calls
    em = np.array(emission)
    em[off[3] - LEAD + 5] = sr.NO_ALIGNMENT
    em[off[3] - LEAD + 9] = 60            # nothing of a segment without an alignment is checked, a label out of range included
    em[off[1] - LEAD + 3] = 0x7fffffff    # nor of a skipped one
    bad_w = [dict(p, arc_weight=np.array(p["arc_weight"])) for p in passes]
    a0, a1 = int(passes[0]["tables"]["arc_offsets"][1]), int(passes[0]["tables"]["arc_offsets"][2])
    bad_w[0]["arc_weight"][a0:a1] = np.nan   # a skipped segment's weights are not read
    skipped, info = run(seq, feats, off, em, bad_w, objective=objective, skip=[0, 1, 0, 0, 0])
    assert list(info["seg_reason"]) == [0, 1, 0, 2, 0]
    assert (info["segments_processed"], info["segments_skipped"], info["segments_without_alignment"]) == (3, 1, 1)
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    for s in (0, 2, 4):
        rest, _ = run(seq, feats, off, emission, passes, objective=objective[s:s + 1], acc=acc, segments=[s])
    assert np.array_equal(skipped.view(np.uint64), rest.view(np.uint64))
    seq.close(), tr.close()


def test_every_refusal_leaves_the_accumulator_untouched(ctx):
    import rasr_amd
    import torch
    net, off, feats, emission, den, num, w_den, w_num, _ = batch()
    tr, seq = trainers(ctx, net, frame_rejection_threshold=0.3)
    pattern = np.arange(tr.accumulator_size(), dtype=np.float64) * 0.5 - 7

    def refused(match, emission=emission, passes=None):
        acc = torch.from_numpy(pattern.copy()).cuda()
        with pytest.raises(rasr_amd.AmxError, match=match) as e:
            run(seq, feats, off, emission, flows()["mmi"] if passes is None else passes, acc=acc)
        assert e.value.status == rasr_amd._lib.AMX_ERR_INVALID
        torch.cuda.synchronize()
        assert np.array_equal(acc.cpu().numpy(), pattern)

    def den_with(**kw):
        t = {k: np.array(v) for k, v in den.items()}
        for k, (i, v) in kw.items():
            t[k][i] = v
        return [dict(tables=t, arc_weight=w_den, factor=1.0, role=sr.REJECT), dict(tables=num, arc_weight=w_num, factor=-1.0)]

    first = int(den["item_offsets"][int(den["arc_offsets"][2])])   # an item of segment 2 (256 frames)
    refused("pass 0: item %d: the frame" % first, passes=den_with(item_frame=(first, 256)))
    refused("pass 0: item %d: the emission" % first, passes=den_with(item_emission=(first, 60)))
    disregarded = int(np.nonzero(net.class_to_output < 0)[0][0])
    refused("pass 0: item %d: the emission" % first, passes=den_with(item_emission=(first, disregarded)))
    w = np.array(w_den)
    w[5] = np.inf
    refused("pass 0: arc 5: the arc weight", passes=[dict(tables=den, arc_weight=w, factor=1.0)])
    em = np.array(emission)
    em[300] = 60
    refused("frame 300: the label", emission=em)
    em[300] = disregarded
    refused("frame 300: the label", emission=em)
    refused("pass 0: workspace row .*negative", passes=[dict(tables=den, arc_weight=w_den, factor=-1.0, role=sr.REJECT)])
    # the scores check their items too
    seq.forward_dev(dev(feats), feats.shape[1], off)
    with pytest.raises(rasr_amd.AmxError, match="item %d: the frame" % first):
        seq.arc_scores(den_with(item_frame=(first, 256))[0]["tables"])
    # a batch over the cap
    with pytest.raises(rasr_amd.AmxError, match="cap of 4096 frames"):
        seq.forward_dev(dev(feats), feats.shape[1], np.arange(0, 18, dtype=np.int64))
    seq.close(), tr.close()


def sausage(net, T, rng, slots=6, width=3):
    """a lattice of `slots` consecutive frame spans with `width` parallel arcs each, one item per frame; arc 0 of a slot is the numerator"""
    valid = sr.valid_classes(net)
    cuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, T), slots - 1, replace=False)), [T]])
    io, fr, em, lm = [0], [], [], []
    for k in range(slots):
        for a in range(width):
            fr.extend(range(cuts[k], cuts[k + 1]))
            em.extend(rng.choice(valid, cuts[k + 1] - cuts[k]))
            io.append(len(fr))
            lm.append(float(rng.random() * 3))
    tables = dict(arc_offsets=np.array([0, slots * width], np.int64), item_offsets=np.array(io, np.int64), item_frame=np.array(fr, np.int32),
                  item_emission=np.array(em, np.int32))
    lat = dict(arc_offsets=np.concatenate([np.arange(slots + 1) * width, [slots * width]]).astype(np.int64),
               arc_target=np.repeat(np.arange(1, slots + 1), width).astype(np.int32), initial=0,
               final_flag=np.array([0] * slots + [1], np.uint8), final_weight=np.zeros(slots + 1, F32))
    return tables, lat, np.array(lm, F32), cuts


def numerator_of(tables, lat, lm, slots, width):
    keep = np.arange(slots) * width
    io = tables["item_offsets"]
    fr = np.concatenate([tables["item_frame"][io[a]:io[a + 1]] for a in keep])
    em = np.concatenate([tables["item_emission"][io[a]:io[a + 1]] for a in keep])
    nio = np.concatenate([[0], np.cumsum([io[a + 1] - io[a] for a in keep])]).astype(np.int64)
    t = dict(arc_offsets=np.array([0, slots], np.int64), item_offsets=nio, item_frame=fr, item_emission=em)
    nl = dict(arc_offsets=np.concatenate([np.arange(slots + 1), [slots]]).astype(np.int64), arc_target=np.arange(1, slots + 1).astype(np.int32), initial=0,
              final_flag=lat["final_flag"], final_weight=lat["final_weight"])
    return t, nl, lm[keep], keep


def test_end_to_end_mmi_on_the_device_and_the_statistics_file(ctx, tmp_path):
    import rasr_amd
    import torch
    net = sr.network()
    rng = np.random.Generator(np.random.PCG64(14))
    T, slots, width = 120, 6, 3
    feats = rng.standard_normal((T, 20)).astype(F32)
    off = np.array([0, T], np.int64)
    den_t, den_l, den_lm, _ = sausage(net, T, rng, slots, width)
    num_t, num_l, num_lm, keep = numerator_of(den_t, den_l, den_lm, slots, width)
    emission = num_t["item_emission"].astype(np.uint32)   # the numerator is one path: its items are the alignment
    tr, seq = trainers(ctx, net, cls=rasr_amd.MiniBatchTrainer)
    tr.set_estimator(learning_rate=0.01)
    seq.forward_dev(dev(feats), 20, off)
    post = rasr_amd.LatticePosterior(ctx, mode="prob")
    passes, total_inv = [], []
    for t, lat, lm, factor in ((den_t, den_l, den_lm, 1.0), (num_t, num_l, num_lm, -1.0)):
        scores = seq.arc_scores(t).cpu().numpy()
        arcs, _, info = post.run([dict(lat, arc_weight=(scores + lm).astype(F32))])
        assert info[0]["reason"] == 0 and not info[0]["vanishing_flow"]
        total_inv.append(F32(info[0]["total_inv_f32"]))
        passes.append(dict(tables=t, arc_weight_dev=arcs, factor=factor))
    objective = np.array([F32(total_inv[0] - total_inv[1])])   # MmiSegmentwiseNnTrainer: f32(den totalInv) - f32(num totalInv)
    assert objective[0] > 0   # the numerator's paths are among the denominator's
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    info = seq.accumulate_dev(passes, dev(emission, np.int32), objective, acc)
    torch.cuda.synchronize()
    assert info["segments_processed"] == 1 and info["observations"] == T
    # posteriors of one frame sum to one on both sides: every column of the MMI error signal sums to zero
    E = seq.error_signal(0, "lattice")
    keys = np.zeros(T, np.int64)   # distinct (frame, output) keys of a column over both lattices
    for t in range(T):
        keys[t] = len({sr.class_to_output(net, e) for tab in (den_t, num_t) for f, e in zip(tab["item_frame"], tab["item_emission"]) if f == t})
    eps = float(np.finfo(F32).eps)
    sums = np.abs(E.astype(np.float64).sum(axis=1))
    print("column sums: max %.3g, keys %d..%d" % (sums.max(), keys.min(), keys.max()))
    assert (sums <= keys * eps).all()
    assert np.abs(E).max() > 0.01
    # the file round-trips and the estimator takes the statistics
    path = str(tmp_path / "seq.stat")
    host = acc.cpu().numpy()
    tr.write(host, path)
    back = tr.read(path)
    s = tr.statistics(host)
    assert tr.statistics(back)["n_observations"] == T and tr.statistics(back)["objective"] == float(F32(s["objective"]))
    for l in range(tr.n_layers):
        assert np.array_equal(tr.statistics(back)["gradient_weights"][l], s["gradient_weights"][l].astype(F32).astype(np.float64))
    tr.write(back, path + "2")
    assert open(path, "rb").read() == open(path + "2", "rb").read()
    before = [w.copy() for w, _ in tr.parameters()]
    tr.estimate(back)
    assert any(not np.array_equal(b, w) for b, (w, _) in zip(before, tr.parameters()))
    post.close(), seq.close(), tr.close()


def test_the_workspace_is_guarded_against_a_call_in_between(ctx):
    import rasr_amd
    import torch
    net, off, feats, emission, den, *_ = batch()
    tr, seq = trainers(ctx, net)
    seq.forward_dev(dev(feats), feats.shape[1], off)
    seq.arc_scores(den)
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    tr.accumulate_dev(dev(feats[off[1]:off[2]]), feats.shape[1], 8, dev(emission[:8], np.int32), acc)   # the frame-wise trainer takes the workspace
    torch.cuda.synchronize()
    with pytest.raises(rasr_amd.AmxError, match="forward pass") as e:
        seq.arc_scores(den)
    assert e.value.status == rasr_amd._lib.AMX_ERR_STATE
    before = acc.cpu().numpy()
    with pytest.raises(rasr_amd.AmxError, match="forward pass"):
        seq.accumulate_dev([], dev(emission, np.int32), np.zeros(5, F32), acc)
    assert np.array_equal(acc.cpu().numpy(), before)
    seq.forward_dev(dev(feats), feats.shape[1], off)
    seq.arc_scores(den)
    seq.close(), tr.close()
