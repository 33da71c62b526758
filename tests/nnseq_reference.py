"""Plain-numpy restatement of the sequence-discriminative NN training pass (include/amx.h, "NN sequence-discriminative training"):
Nn::SegmentwiseNnTrainer with the criteria MMI and ME -- arc scores (EmissionLatticeRescorerAutomaton::_score), the collection of the
arcs' posteriors into the error signal (Lattice::AcousticAccumulator::discoverState, Nn::CachedAcousticAccumulator,
ErrorSignalAccumulator), frame rejection, cross-entropy smoothing, weighting, backpropagation and the per-segment sums.

The forward pass, the derivatives and the buffer layout are tests/nntrain_reference.py's.  `f64=True` computes everything in double
precision with no narrowing (the derivative test).  `defect=` plants one mistake (DEFECTS) that tests/test_nnseq.py must see.

Tables of a batch are the ABI's: arc_offsets [n_seg + 1], item_offsets [n_arcs + 1], item_frame (relative to the segment),
item_emission; a pass is dict(tables, arc_weight f32 [n_arcs], factor, negate, role)."""
import functools

import numpy as np

from tests import nntrain_reference as nr

F32, F64 = np.float32, np.float64
ADD, REJECT, REJECT_CLEAR = "add", "reject", "reject-clear"
NO_ALIGNMENT = 0xFFFFFFFF
EPSILON = float(np.finfo(np.float32).eps)   # Core::Type<f32>::epsilon, the default weight threshold

DEFECTS = ("collection-order", "non-strict-threshold", "factor-after-narrowing", "rejection-wrong-row", "smoothing-order",
           "weights-before-smoothing", "chunks-across-segments", "zero-item-arc-nonzero")


class Refused(Exception):
    """what the device refuses with AMX_ERR_INVALID"""


def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays, correctly rounded: the product is exact in f64, the sum is rounded to odd there, then narrowed"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64), np.asarray(c, F32).astype(F64))
    s = a * b
    t = s + c
    bb = t - s
    err = (s - (t - bb)) + (c - bb)
    even = (t.view(np.int64) & 1) == 0
    nudge = (err != 0) & even & np.isfinite(t)
    toward = np.where(err > 0, np.inf, -np.inf)
    t = np.where(nudge, np.nextafter(t, toward), t)
    return t.astype(F32)


def forward(net, x, products="f64"):
    """every layer's input and the linear top output of the frames x"""
    X = [nr.preprocess(np.asarray(x, F32), net.pre)]
    L = len(net.Ws)
    for l in range(L):
        z = (nr.matmul(X[l], net.Ws[l].T, products) + net.bs[l][None, :]).astype(F32)
        if l < L - 1:
            X.append(nr.activate(z, net.acts[l]))
    return X, z


def row_plan(frame_offsets):
    """(rows, row0 [n_seg + 1], row_src [rows]) of amx_nnseq_forward_dev: a segment starts at a multiple of nr.CHUNK; row_src is the
    feature row a workspace row holds, -1 between two segments"""
    off = np.asarray(frame_offsets, np.int64)
    row0, src = [0], []
    for s in range(len(off) - 1):
        n = int(off[s + 1] - off[s])
        padded = -(-n // nr.CHUNK) * nr.CHUNK
        src.extend(list(range(int(off[s]), int(off[s + 1]))) + [-1] * (padded - n))
        row0.append(row0[-1] + padded)
    return row0[-1], np.array(row0, np.int32), np.array(src, np.int64)


def class_to_output(net, e):
    return int(e) if net.class_to_output is None else int(net.class_to_output[int(e)])


def segment_arcs(tables, s):
    """the arcs of segment s as (arc index, frames, emissions)"""
    ao, io = np.asarray(tables["arc_offsets"]), np.asarray(tables["item_offsets"])
    for a in range(int(ao[s]), int(ao[s + 1])):
        b, e = int(io[a]), int(io[a + 1])
        yield a, np.asarray(tables["item_frame"])[b:e], np.asarray(tables["item_emission"])[b:e]


def check_item(net, T, f, e):
    if f < 0 or f >= T:
        raise Refused("frame")
    if e < 0 or e >= n_classes(net) or class_to_output(net, e) < 0:
        raise Refused("emission")


def n_classes(net):
    return net.n_outputs if net.class_to_output is None else len(net.class_to_output)


def arc_scores(net, top, tables, s, defect=None):
    """_score per arc of segment s on the segment's linear top output [T x n_out]: one f32 chain from 0 in item order"""
    out = []
    for _, frames, ems in segment_arcs(tables, s):
        score = F32(0)
        if len(frames) == 0 and defect == "zero-item-arc-nonzero":
            score = F32(1)
        for f, e in zip(frames, ems):
            check_item(net, len(top), int(f), int(e))
            score = F32(score - top[int(f), class_to_output(net, e)])
        out.append(score)
    return np.array(out, F32)


def alignment(net, emission):
    """AlignmentAccumulator: outputs of the best path; None = the alignment vector failed"""
    em = np.asarray(emission, np.uint32)
    if (em == NO_ALIGNMENT).any():
        return None
    if (em >= n_classes(net)).any():
        raise Refused("label")
    a = np.array([class_to_output(net, e) for e in em], np.int64)
    if (a < 0).any():
        raise Refused("label")
    return a


def lattice_error(net, T, s, passes, align, w, threshold=EPSILON, rejection=0.0, defect=None, f64=False):
    """the passes of one segment: (E [T x n_out], rejected); w is updated in place"""
    E = np.zeros((T, net.n_outputs), F64 if f64 else F32)
    rejected = 0
    for ps in passes:
        lists = {}
        for a, frames, ems in segment_arcs(ps["tables"], s):
            wa = F32(ps["arc_weight"][a])
            if not np.isfinite(wa):
                raise Refused("weight")
            if ps.get("negate"):
                wa = F32(wa * F32(-1.0))
            counts = F64(wa) >= threshold if defect == "non-strict-threshold" else F64(wa) > threshold
            for f, e in zip(frames, ems):
                check_item(net, T, int(f), int(e))
                if counts:
                    lists.setdefault((int(f), class_to_output(net, e)), []).append(wa)
        factor = float(ps.get("factor", 1.0))
        for (t, o), ws in lists.items():
            if defect == "collection-order":
                ws = ws[::-1]
            c = 0.0
            for x in ws:
                c += float(x)
            if defect == "factor-after-narrowing":
                c = float(F32(c))
            v = float(E[t, o]) + factor * c
            E[t, o] = v if f64 else F32(v)
        role = ps.get("role", ADD)
        if role != ADD and rejection > 0:
            for t in range(T):
                row = align[(t + 1) % T] if defect == "rejection-wrong-row" else align[t]
                cell = E[t, row]
                if not cell >= 0:
                    raise Refused("cell")
                if cell < F32(rejection):
                    w[t] = 0
                    rejected += 1
        if role == REJECT_CLEAR:
            E[:] = 0
    return E, rejected


def softmax_of(net, top, log_prior=None, prior_scale=0.0, f64=False):
    """the smoothing's p from the linear top output"""
    if f64:
        z = np.asarray(top, F64)
        if prior_scale > 0 and log_prior is not None:
            z = z + float(prior_scale) * np.asarray(log_prior, F64)[None, :]
        z = z - z.max(axis=1, keepdims=True)
        e = np.exp(z)
        return e / e.sum(axis=1, keepdims=True)
    z = np.asarray(top, F32)
    if prior_scale > 0 and log_prior is not None:
        z = fma32(F32(prior_scale), np.asarray(log_prior, F32)[None, :], z)
    return nr.softmax(z)


def smooth(E, p, align, w, lam, defect=None, f64=False):
    """smoothErrorSignalWithCE on E with the softmax p, then multiplyColumnsByScalars(w): (E, CE objective of the segment)"""
    T = len(align)
    idx = np.arange(T)
    if f64:
        E = np.asarray(E, F64).copy()
        if lam > 0:
            E = E * (1.0 - lam) + lam * p
            E[idx, align] += -lam
        ce = float(-(np.log(p[idx, align]) * w).sum()) if lam > 0 else 0.0
        return E * np.asarray(w, F64)[:, None], ce
    E = np.asarray(E, F32).copy()
    lam32 = F32(lam)
    if defect == "weights-before-smoothing":
        E = (E * w[:, None]).astype(F32)
    if lam > 0:
        keep = F32(1.0 - float(lam32))
        if defect == "smoothing-order":
            E[idx, align] = E[idx, align] + -lam32
            E = fma32(lam32, p, E)
            E = (E * keep).astype(F32)
        else:
            E = (E * keep).astype(F32)
            E = fma32(lam32, p, E)
            E[idx, align] = E[idx, align] + -lam32
    if defect != "weights-before-smoothing":
        E = (E * w[:, None]).astype(F32)
    ce = F32(0)
    if lam > 0:
        terms = (nr.logf(p[idx, align]) * w).astype(F32)
        for t in range(T):
            ce = F32(ce - terms[t])
    return E, ce


def backpropagate(net, X, Etop, products="f64"):
    """error signals of every layer, no clip"""
    L = len(net.Ws)
    E = [None] * L
    E[L - 1] = Etop
    for l in range(L - 1, 0, -1):
        d = nr.matmul(E[l], net.Ws[l], products)
        y, act = X[l], net.acts[l - 1]
        E[l - 1] = nr.sigmoid_derivative(d, y) if act == nr.SIGMOID else nr.tanh_derivative(d, y) if act == nr.TANH else \
            nr.rectified_derivative(d, y) if act == nr.RELU else d
    return E


def chunk_sums(X, E, bounds):
    """X^T E and the column sums of E as the device orders them: an f32 product per chunk of nr.CHUNK frames, the partials added in f32
    in ascending order; bounds: the (begin, end) frame ranges whose chunks start afresh"""
    gw, gb = np.zeros((X.shape[1], E.shape[1]), F32), np.zeros(E.shape[1], F32)
    for b, e in bounds:
        for c in range(b, e, nr.CHUNK):
            gw = gw + np.matmul(X[c:min(e, c + nr.CHUNK)].T, E[c:min(e, c + nr.CHUNK)])
            gb = gb + nr.seq_sum_f32(E[c:min(e, c + nr.CHUNK)], 0)
    return gw.astype(F64), gb.astype(F64)


def process(net, feats, frame_offsets, emission, passes, objective, skip=None, threshold=EPSILON, lam=0.0, rejection=0.0, log_prior=None,
            prior_scale=0.0, products="f64", defect=None, f64=False, top=None, p=None, gradient=True):
    """amx_nnseq_forward_dev + amx_nnseq_accumulate_dev into zeros.  top / p: per segment, the device's own linear output / softmax to
    apply the restatement to (None: the restatement's forward pass).  -> dict(stats: nr.accumulate's blocks, segments: per segment dict
    (reason, E_lattice, E, w, rejected, errors, ce, p, error_signals), info)"""
    off = np.asarray(frame_offsets, np.int64)
    n_seg, L = len(off) - 1, len(net.Ws)
    dims = net.dims
    stats = {"n_observations": 0, "n_classification_errors": 0, "total_weight": 0.0, "objective": 0.0,
             "gradient_weights": [np.zeros((dims[l], dims[l + 1]), F64) for l in range(L)], "gradient_bias": [np.zeros(dims[l + 1], F64) for l in range(L)]}
    segs, info = [], dict(segments_processed=0, segments_skipped=0, segments_without_alignment=0, observations=0, rejected_observations=0, ce_objective=F32(0))
    pending = []   # the defect that chunks across segment boundaries sums these at the end
    for s in range(n_seg):
        T = int(off[s + 1] - off[s])
        em = np.asarray(emission)[off[s] - off[0]:off[s + 1] - off[0]]
        if skip is not None and skip[s]:
            info["segments_skipped"] += 1
            segs.append(dict(reason="skipped"))
            continue
        align = alignment(net, em)
        if align is None:
            info["segments_without_alignment"] += 1
            segs.append(dict(reason="no-alignment"))
            continue
        if T == 0:
            segs.append(dict(reason="ok"))
            continue
        X, z = forward(net, feats[off[s]:off[s + 1]], products)
        if top is not None and top[s] is not None:
            z = top[s]
        w = net.class_weights[align].astype(F64 if f64 else F32)
        if gradient and lam < 1:
            E, rejected = lattice_error(net, T, s, passes, align, w, threshold, rejection, defect, f64)
        else:
            E, rejected = np.zeros((T, net.n_outputs), F64 if f64 else F32), 0
        seg = dict(reason="ok", E_lattice=E.copy(), rejected=rejected)
        if lam > 0:
            ps = p[s] if p is not None and p[s] is not None else softmax_of(net, z, log_prior, prior_scale, f64)
            seg["p"] = ps
        else:
            ps = None
        E, ce = smooth(E, ps, align, w, lam, defect, f64)
        seg.update(E=E, w=w.copy(), ce=ce, errors=int((nr.arg_max(ps if lam > 0 else z) != align).sum()))
        if gradient and not f64:
            Es = backpropagate(net, X, E, "f64" if products == "f64" else "f32")
            seg["error_signals"] = Es
            for l in range(L):
                if products == "f64":
                    stats["gradient_weights"][l] += X[l].astype(F64).T @ Es[l].astype(F64)
                    stats["gradient_bias"][l] += Es[l].astype(F64).sum(0)
                elif defect == "chunks-across-segments":
                    pending.append((l, X[l], Es[l]))
                else:
                    gw, gb = chunk_sums(X[l], Es[l], [(0, T)])
                    stats["gradient_weights"][l] += gw
                    stats["gradient_bias"][l] += gb
        stats["n_observations"] += T
        stats["n_classification_errors"] += seg["errors"]
        stats["total_weight"] += float(np.abs(w).astype(F64).sum())
        stats["objective"] += float(F32(objective[s])) if not f64 else float(objective[s])
        info["segments_processed"] += 1
        info["observations"] += T
        info["rejected_observations"] += rejected
        info["ce_objective"] = F32(info["ce_objective"] + F32(ce))
        segs.append(seg)
    for l in range(L):
        parts = [(x, e) for ll, x, e in pending if ll == l]
        if parts:
            gw, gb = chunk_sums(np.concatenate([x for x, _ in parts]), np.concatenate([e for _, e in parts]), [(0, sum(len(x) for x, _ in parts))])
            stats["gradient_weights"][l] += gw
            stats["gradient_bias"][l] += gb
    return dict(stats=stats, segments=segs, info=info)


# ------------------------------------------------------------------------------------ small lattices in f64 (the derivative test)
def paths(lat):
    """every path of a small acyclic lattice dict(n_states, initial, finals {state: weight}, arcs [(source, target, lm)]) as arc lists"""
    out = []

    def walk(state, taken):
        if state in lat["finals"]:
            out.append(list(taken))
        for k, (src, tgt, _) in enumerate(lat["arcs"]):
            if src == state:
                walk(tgt, taken + [k])
    walk(lat["initial"], [])
    return out


def posteriors_f64(lat, acoustic):
    """(arc posteriors, log of the total flow) of the lattice with arc costs acoustic[k] + lm[k], by enumeration in f64"""
    ps = paths(lat)
    cost = np.array([sum(acoustic[k] + lat["arcs"][k][2] for k in path) + lat["finals"][lat["arcs"][path[-1]][1] if path else lat["initial"]] for path in ps], F64)
    m = cost.min()
    z = np.exp(-(cost - m))
    total = z.sum()
    post = np.zeros(len(lat["arcs"]), F64)
    for path, q in zip(ps, z):
        for k in path:
            post[k] += q / total
    return post, float(np.log(total) - m)


def acoustic_f64(net, top, items):
    """_score in f64: per arc -sum of out[o, t]"""
    return np.array([-sum(float(top[f, class_to_output(net, e)]) for f, e in arc) for arc in items], F64)


def derivative_case():
    """a lattice of a few arcs over 6 frames on a 5-4-6 network, and its numerator (the arcs 0 and 3)"""
    rng = np.random.Generator(np.random.PCG64(21))
    Ws = [(rng.standard_normal((4, 5)) * 0.5).astype(F32), (rng.standard_normal((6, 4)) * 0.5).astype(F32)]
    bs = [(rng.standard_normal(4) * 0.1).astype(F32), (rng.standard_normal(6) * 0.1).astype(F32)]
    net = nr.Net(Ws, bs, [nr.TANH, nr.NONE])
    x = rng.standard_normal((6, 5)).astype(F32)
    lat = dict(initial=0, finals={2: 0.25}, arcs=[(0, 1, 0.5), (0, 1, 1.0), (0, 1, 0.2), (1, 2, 0.7), (1, 2, 0.1)])
    items = [[(0, 1), (1, 1), (2, 3)], [(0, 2), (1, 2), (2, 2)], [(0, 1), (1, 5), (2, 0)], [(3, 4), (4, 4), (5, 0)], [(3, 3), (4, 4), (5, 5)]]
    return net, x, lat, items, [0, 3]



def mmi_objective_f64(net, top, lat, items, numerator):
    """f(den totalInv) - f(num totalInv) of MmiSegmentwiseNnTrainer in f64: the logarithms of the two total flows"""
    ac = acoustic_f64(net, top, items)
    num = dict(lat, arcs=[lat["arcs"][k] for k in numerator])
    return posteriors_f64(lat, ac)[1] - posteriors_f64(num, ac[numerator])[1]


def mmi_derivative_deviation(net, x, lat, items, numerator, step):
    """max over the cells of the top output of |MMI error signal (all f64, threshold 0, no smoothing) - central difference of the
    objective at `step`|: pins the signs of factor, score and objective"""
    _, z = forward(net, x)
    top = z.astype(F64)
    ac = acoustic_f64(net, top, items)
    num_lat = dict(lat, arcs=[lat["arcs"][k] for k in numerator])
    den_post, num_post = posteriors_f64(lat, ac)[0], posteriors_f64(num_lat, ac[numerator])[0]

    def tables(arcs):
        io = np.concatenate([[0], np.cumsum([len(items[k]) for k in arcs])]).astype(np.int64)
        return dict(arc_offsets=np.array([0, len(arcs)], np.int64), item_offsets=io, item_frame=np.array([f for k in arcs for f, _ in items[k]], np.int32),
                    item_emission=np.array([e for k in arcs for _, e in items[k]], np.int32))
    passes = [dict(tables=tables(range(len(items))), arc_weight=den_post, factor=1.0), dict(tables=tables(numerator), arc_weight=num_post, factor=-1.0)]
    T = len(x)
    E = np.zeros((T, net.n_outputs), F64)
    for ps in passes:   # lattice_error in f64, the weights kept in f64 as well
        for a, frames, ems in segment_arcs(ps["tables"], 0):
            if ps["arc_weight"][a] > 0:
                for f, e in zip(frames, ems):
                    E[int(f), class_to_output(net, e)] += ps["factor"] * ps["arc_weight"][a]
    worst = 0.0
    for t in range(T):
        for o in range(net.n_outputs):
            up, down = top.copy(), top.copy()
            up[t, o] += step
            down[t, o] -= step
            d = (mmi_objective_f64(net, up, lat, items, numerator) - mmi_objective_f64(net, down, lat, items, numerator)) / (2 * step)
            worst = max(worst, abs(d - E[t, o]))
    assert np.abs(E).max() > 0.1
    return worst


# ------------------------------------------------------------------------------------ cases
def network(seed=5):
    """20-33-17-50, sigmoid then rectified, 60 classes of which ten, drawn at random, have no output (they map to -1); the other fifty map
    one-to-one onto the outputs in a random order"""
    rng = np.random.Generator(np.random.PCG64(seed))
    dims = [20, 33, 17, 50]
    Ws = [(rng.standard_normal((dims[l + 1], dims[l])) * (1.2 / np.sqrt(dims[l]))).astype(F32) for l in range(3)]
    bs = [(rng.standard_normal(dims[l + 1]) * 0.2).astype(F32) for l in range(3)]
    c2o = np.full(60, -1, np.int64)
    keep = np.sort(rng.permutation(60)[:50])
    c2o[keep] = rng.permutation(50)
    cw = (0.5 + rng.random(50)).astype(F32)
    return nr.Net(Ws, bs, [nr.SIGMOID, nr.RELU, nr.NONE], class_to_output=c2o, class_weights=cw)


def valid_classes(net):
    return np.nonzero(net.class_to_output >= 0)[0]


def random_lattice_tables(net, lengths, rng, arcs_per_segment=12, empty_arcs=True, long_arc=0):
    """arc tables of a batch: per segment arcs_per_segment arcs over random frame spans with one item per frame, some arcs empty"""
    valid = valid_classes(net)
    ao, io, fr, em = [0], [0], [], []
    for s, T in enumerate(lengths):
        n = arcs_per_segment if T > 0 else 0
        for a in range(n):
            if empty_arcs and a % 5 == 4:
                b = e = 0
            elif long_arc and a == 0:
                b, e = 0, min(T, long_arc)
            else:
                b = int(rng.integers(0, T))
                e = int(min(T, b + 1 + rng.integers(0, 40)))
            fr.extend(range(b, e))
            em.extend(rng.choice(valid[:6] if a % 2 else valid, e - b))   # a small emission set: keys repeat across arcs
            io.append(len(fr))
        ao.append(ao[-1] + n)
    return dict(arc_offsets=np.array(ao, np.int64), item_offsets=np.array(io, np.int64), item_frame=np.array(fr, np.int32),
                item_emission=np.array(em, np.int32))


def order_case(e=0):
    """one key with the f32 weights 1, 2^-24, 2^-53, 2^-53 in arc order (threshold below 2^-53): summed in this order in f64 the
    two small terms vanish one by one, 1 + 2^-24, which narrows to 1.0 (a tie, to even); summed in the other order they first join to
    2^-52 and survive, 1 + 2^-24 + 2^-52, which narrows to 1 + 2^-23"""
    tables = dict(arc_offsets=np.array([0, 4], np.int64), item_offsets=np.array([0, 1, 2, 3, 4], np.int64), item_frame=np.zeros(4, np.int32),
                  item_emission=np.full(4, e, np.int32))
    return tables, np.array([1.0, 2.0 ** -24, 2.0 ** -53, 2.0 ** -53], F32), 2.0 ** -60


def narrowing_case(e=0):
    """a cell that holds 1 takes the weights 2^-24 and 2^-50 from a second pass: 1 + (2^-24 + 2^-50) narrows to 1 + 2^-23; with the
    collected sum narrowed first (2^-24) the result is the tie 1 + 2^-24, which narrows to 1"""
    one = dict(arc_offsets=np.array([0, 1], np.int64), item_offsets=np.array([0, 1], np.int64), item_frame=np.zeros(1, np.int32), item_emission=np.full(1, e, np.int32))
    two = dict(arc_offsets=np.array([0, 2], np.int64), item_offsets=np.array([0, 1, 2], np.int64), item_frame=np.zeros(2, np.int32),
               item_emission=np.full(2, e, np.int32))
    return [dict(tables=one, arc_weight=np.array([1.0], F32), factor=1.0), dict(tables=two, arc_weight=np.array([2.0 ** -24, 2.0 ** -50], F32), factor=1.0)], 2.0 ** -60


GPU_LENGTHS = (1, 255, 256, 257, 300)
GPU_LEAD = 2   # rows of the feature matrix in front of the first segment


@functools.lru_cache(maxsize=None)
def gpu_batch():
    """the batch of tests/test_nnseq_gpu.py (and of the bars in tests/golden/ref_nnseq.npz): (net, frame offsets, features, emission,
    denominator tables, numerator tables, denominator weights, numerator weights, signed weights of the ME flow)"""
    net = network()
    rng = np.random.Generator(np.random.PCG64(11))
    off = GPU_LEAD + np.concatenate([[0], np.cumsum(GPU_LENGTHS)]).astype(np.int64)
    feats = np.full((int(off[-1]) + 1, 20), np.nan, F32)
    feats[GPU_LEAD:off[-1]] = rng.standard_normal((int(off[-1]) - GPU_LEAD, 20)).astype(F32)
    emission = rng.choice(valid_classes(net), int(off[-1]) - GPU_LEAD).astype(np.uint32)
    den = random_lattice_tables(net, GPU_LENGTHS, rng, arcs_per_segment=13, long_arc=200)
    num = random_lattice_tables(net, GPU_LENGTHS, rng, arcs_per_segment=3, empty_arcs=False)
    emission = emission.copy()   # where the denominator has an item, the alignment takes one of its emissions: the rejection test reads cells that hold something
    for s in range(len(GPU_LENGTHS)):
        for _, frames, ems in segment_arcs(den, s):
            emission[off[s] - GPU_LEAD + frames] = ems
    n_den, n_num = int(den["arc_offsets"][-1]), int(num["arc_offsets"][-1])
    w_den = rng.random(n_den).astype(F32)
    w_den[::7] = 0                    # arcs below the threshold
    w_den[3] = F32(EPSILON)           # exactly at it: strict, does not count
    w_num = rng.random(n_num).astype(F32)
    w_me = (rng.random(n_den) - 0.5).astype(F32)
    for v in (feats, emission, w_den, w_num, w_me):
        v.setflags(write=False)
    return net, off, feats, emission, den, num, w_den, w_num, w_me


def gpu_flows():
    """the three flows of include/amx.h on gpu_batch()"""
    net, off, feats, emission, den, num, w_den, w_num, w_me = gpu_batch()
    mmi = [dict(tables=den, arc_weight=w_den, factor=1.0, role=REJECT), dict(tables=num, arc_weight=w_num, factor=-1.0)]
    me = [dict(tables=den, arc_weight=w_me, factor=-1.0), dict(tables=den, arc_weight=w_me, factor=1.0, negate=True)]
    me_rej = [dict(tables=den, arc_weight=w_den, factor=1.0, role=REJECT_CLEAR)] + me
    return {"mmi": mmi, "me": me, "me-rejection": me_rej}
