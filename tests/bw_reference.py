"""Plain restatement of the reference's Baum-Welch alignment (Search/Aligner.cc: SearchSpace::expand,
activateOrUpdateStateHypothesisBaumWelch, prune, finalStatePotential, getAlignmentFsaBaumWelch, Aligner::feed, getAlignment,
getAlignmentPosteriorFsa; Fsa/Sssp.cc: StatePotentials64DfsState::finishState, Posterior64Automaton; Fsa/tRealSemiring.cc: LogSemiring::collect;
Speech/Alignment.cc: the item functions), in two orders:

  order="reference"   the f32 sequential collect in list order during the search, f64 potentials in the arc orders of the fixture's
                      transposition, -log p narrowed to f32 per arc, the f32 collect per (frame, label), and the item arithmetic (clip,
                      shift, exp, normalise) on f64 weights, as the reference has it (Mm::Weight is f64)
  order="device"      the sums as the kernels of rasr_amd/csrc/align_bw.hip take them: a state's candidates in the static by-target order,
                      their log-sum in f64 rounded to f32 once; exp(-(fw + w + bw - total)) summed per (frame, label) in f64 in (target,
                      source, ordinal) order, `total` being the forward sweep's; the frame's sum over 256 lanes' partial sums by the
                      kernel's tree; one rounding to f32 at the end

Graphs, cases and the pass loop's helpers are tests/align_reference.py's.  Plain Python loops; f64 exp and log1p are the C library's."""
import math

import numpy as np

from tests import align_reference as ar

F32, F32_MAX = ar.F32, ar.F32_MAX
DEAD = float(np.finfo(np.float64).max)            # Fsa/Sssp.cc:67
DEFAULTS = dict(ar.DEFAULTS, min_weight=0.0, use_partial_sums=0)
THREADS = 256


class NanMet(Exception):
    """the library's added rule: a NaN candidate, or inf - inf in a log-sum, ends the search of the segment"""


def collect32(a, b):
    """LogSemiring<f32>::collect (Fsa/tRealSemiring.cc:130-146)"""
    a, b = F32(a), F32(b)
    if b == F32_MAX:
        return a
    if a == F32_MAX:
        return b
    lo, hi = (a, b) if a <= b else (b, a)
    with np.errstate(all="ignore"):
        d = F32(lo - hi)                                   # the difference is f32; `::exp` and `::log1p` name the f64 functions there
        if np.isnan(d):
            raise NanMet()
        r = F32(float(lo) - math.log1p(math.exp(float(d))))   # one rounding back to f32 (tests/golden/ref_bw.npz: collect_calls, collect_probe_*)
    return r


def logsum64(xs):
    """min - log1p(sum over the others of exp(min - x)), the first minimal one left out, in the order given; None for no candidate"""
    if not xs:
        return None
    first = min(range(len(xs)), key=lambda i: (xs[i], i))
    m = xs[first]
    if len(xs) == 1:
        return m
    acc = 0.0
    for i, x in enumerate(xs):
        if i != first:
            d = m - x
            if d != d:
                raise NanMet()
            acc += math.exp(d)
    return m - math.log1p(acc)


def by_target(graph):
    """incoming arcs per state in (source, ordinal) order: (source, emission, label, weight)"""
    inc = [[] for _ in range(graph["n_states"])]
    for s, arcs in enumerate(graph["arcs"]):
        for t, e, l, w in arcs:
            inc[t].append((s, e, l, F32(w)))
    return inc


def one_pass(graph, rows, threshold, order):
    """all frames at one threshold.  Returns per frame the survivors as an ordered dict state -> f32 score (list order in reference order,
    state order in device order), the survivor counts and whether anything was pruned."""
    t = F32(threshold)
    cur = {graph["initial"]: F32(0)}
    frames, counts, pruned = [cur], [], False
    inc = by_target(graph) if order == "device" else None
    with np.errstate(all="ignore"):
        for row in rows:
            new = {}
            if order == "reference":
                for state, score in cur.items():                                  # expand (:215-252)
                    for target, emission, _, weight in graph["arcs"][state]:
                        arc = F32(F32(weight) + row[emission])                    # :238
                        cand = F32(score + arc)                                   # :239
                        if np.isnan(cand):
                            raise NanMet()
                        new[target] = cand if target not in new else collect32(new[target], cand)   # :178-193
            else:
                for s in range(graph["n_states"]):
                    cands = []
                    for src, emission, _, weight in inc[s]:
                        if src in cur:
                            c = F32(cur[src] + F32(weight + row[emission]))
                            if np.isnan(c):
                                raise NanMet()
                            cands.append(c)
                    if cands:
                        v = F32(logsum64([float(c) for c in cands])) if len(cands) > 1 else cands[0]
                        if np.isnan(v):
                            raise NanMet()
                        new[s] = v
            m = F32_MAX
            for v in new.values():
                if m > v:
                    m = v
            limit = F32(m + t)
            kept = {s: v for s, v in new.items() if v <= limit}
            pruned = pruned or len(kept) < len(new)
            cur = kept
            frames.append(cur)
            counts.append(len(kept))
    return frames, counts, pruned


def final_potential(graph, hyps, order):
    """finalStatePotential (:385-405) in Baum-Welch mode"""
    with np.errstate(all="ignore"):
        vals = []
        for s in (hyps if order == "reference" else sorted(hyps)):
            if graph["final"][s]:
                v = F32(F32(graph["final_weight"][s]) + hyps[s])
                if np.isnan(v):
                    raise NanMet()
                vals.append(v)
        if order == "reference":
            result = F32_MAX
            for v in vals:
                result = v if result == F32_MAX else collect32(result, v)
            return result
        vals = [v for v in vals if v < F32_MAX]
        if not vals:
            return F32_MAX
        r = F32(logsum64([float(v) for v in vals])) if len(vals) > 1 else vals[0]
        if np.isnan(r):
            raise NanMet()
        return r


def search(graph, scores, order, **cfg):
    """Aligner::feed(vector) (:603-630).  Returns the result dict (without items) and the last pass's survivors per frame."""
    c = dict(DEFAULTS)
    c.update(cfg)
    T = len(scores)
    scale = F32(c["score_scale"])
    with np.errstate(all="ignore"):
        rows = np.asarray(scores, F32) if scale == 1 else (scale * np.asarray(scores, F32)).astype(F32)
    lo, hi, factor = F32(c["min_acoustic_pruning"]), F32(c["max_acoustic_pruning"]), F32(c["increment_factor"])
    min_avg = float(c["min_average_number_of_states"])
    out = dict(score=F32_MAX, reached=False, n_iterations=0, last_threshold=F32(0), average_states=0.0, state_sum=0, survivors=np.zeros(T, np.int32),
               nan=False, passes_run=0)
    previous, t, frames, stop_running = F32_MAX, lo, None, False
    with np.errstate(all="ignore"):
        while t <= hi:
            out["n_iterations"] += 1
            out["last_threshold"] = t
            try:
                frames, counts, pruned = one_pass(graph, rows, t, order)
                score = final_potential(graph, frames[-1], order)
            except NanMet:
                out.update(nan=True, score=F32_MAX, reached=False, state_sum=0, average_states=0.0, survivors=np.zeros(T, np.int32))
                out["passes_run"] += 1
                return out, None, rows
            if not stop_running:
                out["passes_run"] += 1
            stop_running = stop_running or not pruned
            out["score"], out["reached"] = score, bool(score != F32_MAX)
            out["state_sum"] = int(sum(counts))
            out["average_states"] = float(np.float64(out["state_sum"]) / np.float64(T)) if T else float("nan")
            out["survivors"] = np.array(counts, np.int32).reshape(T)
            if factor <= 1:
                break
            if out["reached"] and out["average_states"] >= min_avg:
                if not c["increase_until_no_score_difference"]:
                    break
                if t > lo and ar.is_almost_equal(score, previous):
                    break
            previous = score
            t = F32(t * factor)
    return out, frames, rows


def potentials(graph, frames, rows):
    """f64 forward and backward potentials over the survivors (posterior64): fw[f][s] for f = 0 .. T (f = 0: the initial state), bw alike.
    A state's sum runs over its arcs in (source, ordinal) order forward and in the graph's arc order backward."""
    T = len(rows)
    inc = by_target(graph)
    fw = [{graph["initial"]: 0.0}]
    for f in range(T):
        cur, row = {}, rows[f]
        for s in sorted(frames[f + 1]):
            xs = []
            for src, e, _, w in inc[s]:
                if src in fw[f]:
                    x = fw[f][src] + float(F32(w + row[e]))
                    if x < DEAD:
                        xs.append(x)
            v = logsum64(xs)
            if v is not None and v < DEAD:
                cur[s] = v
        fw.append(cur)
    bw = [None] * (T + 1)
    bw[T] = {s: float(graph["final_weight"][s]) for s in fw[T] if graph["final"][s] and graph["final_weight"][s] < F32_MAX}
    for f in range(T - 1, -1, -1):
        cur, row = {}, rows[f]
        for s in fw[f]:
            xs = []
            for tgt, e, _, w in graph["arcs"][s]:
                if tgt in bw[f + 1]:
                    x = bw[f + 1][tgt] + float(F32(F32(w) + row[e]))
                    if x < DEAD:
                        xs.append(x)
            v = logsum64(xs)
            if v is not None and v < DEAD:
                cur[s] = v
        bw[f] = cur
    fw_total = logsum64([fw[T][s] + float(graph["final_weight"][s]) for s in sorted(fw[T])
                         if graph["final"][s] and graph["final_weight"][s] < F32_MAX and fw[T][s] + float(graph["final_weight"][s]) < DEAD])
    return fw, bw, fw_total


def _tree_sum(parts):
    """the kernel's sum of 256 lanes' partial sums: a shuffle-down tree within each wave of 64, the four waves in order"""
    p = np.array(parts, np.float64).reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        q = p.copy()
        q[:, :64 - o] = p[:, :64 - o] + p[:, o:]
        p = q
    return float(((p[0, 0] + p[1, 0]) + p[2, 0]) + p[3, 0])


def items_device(graph, frames, rows, fw, bw, total):
    """per frame [(label, emission, f32 weight)] ordered by decreasing weight, then label; and in the same order the f64 shares the
    weights are rounded from"""
    T = len(rows)
    inc = by_target(graph)
    labels = sorted({l for arcs in graph["arcs"] for _, _, l, _ in arcs})
    index = {l: i for i, l in enumerate(labels)}
    emission = {l: e for arcs in graph["arcs"] for _, e, l, _ in arcs}
    out, shares = [], []
    for f in range(T):
        P, row = [0.0] * len(labels), rows[f]
        for tgt in range(graph["n_states"]):                                   # (target, source, ordinal): the by-label arc lists' order
            if tgt not in bw[f + 1]:
                continue
            for src, e, l, w in inc[tgt]:
                if src in fw[f]:
                    lp = ((fw[f][src] + float(F32(w + row[e]))) + bw[f + 1][tgt]) - total
                    if lp < float(F32_MAX):
                        P[index[l]] += math.exp(-lp)
        parts = [0.0] * THREADS
        for i, v in enumerate(P):
            parts[i % THREADS] += v
        Z = _tree_sum(parts)
        frame = []
        with np.errstate(all="ignore"):
            for i, v in enumerate(P):
                w = F32(np.float64(v) / np.float64(Z))
                if w > 0:
                    frame.append((labels[i], emission[labels[i]], w, float(np.float64(v) / np.float64(Z))))
        frame.sort(key=lambda it: (-float(it[2]), it[0]))
        out.append([it[:3] for it in frame])
        shares.append([it[3] for it in frame])
    return out, shares


def logsum_reference(xs):
    """StatePotentials64DfsState::finishState (Sssp.cc:112-133) for a state that is not final: the LAST minimal arc is left out of the
    sum (`score <= minimumScore`), infinite scores and the result are clipped at Zero"""
    xs = [DEAD if math.isinf(x) else x for x in xs]
    m, at = DEAD, None
    for i, x in enumerate(xs):
        if x <= m:
            m, at = x, i
    acc = 0.0
    for i, x in enumerate(xs):
        if i != at:
            acc += math.exp(m - x)
    v = m - math.log1p(acc)
    return v if v < DEAD else DEAD


def potentials_reference(graph, frames, rows):
    """posterior64 over the automaton getAlignmentFsaBaumWelch returns, in the arc orders of tests/golden/make_bw_golden.py's transposition:
    a hypothesis sums its incoming arcs by (position of the source in its frame's list, arc order of the source) and its outgoing arcs by
    (position of the target in its frame's list, arc order).  frames: the hypothesis lists of the last pass, in list order.  Hypotheses
    that collectGarbage removes have no path to a final state; they get Zero here, which adds exp(-inf) = 0 to a sum."""
    T = len(rows)
    fw = [{graph["initial"]: 0.0}]
    for f in range(T):
        cand = {s: [] for s in frames[f + 1]}
        for src in frames[f]:
            for tgt, e, _, w in graph["arcs"][src]:
                if tgt in cand:
                    cand[tgt].append(fw[f][src] + float(F32(F32(w) + rows[f][e])))
        fw.append({s: logsum_reference(xs) for s, xs in cand.items()})
    bw = [None] * (T + 1)
    bw[T] = {s: (0.0 + float(F32(graph["final_weight"][s])) if graph["final"][s] else DEAD) for s in frames[T]}
    for f in range(T - 1, -1, -1):
        pos = {s: i for i, s in enumerate(frames[f + 1])}
        cur = {}
        for src in frames[f]:
            out = sorted(((pos[tgt], k, bw[f + 1][tgt] + float(F32(F32(w) + rows[f][e]))) for k, (tgt, e, _, w) in enumerate(graph["arcs"][src]) if tgt in pos))
            cur[src] = logsum_reference([x for _, _, x in out])
        bw[f] = cur
    return fw, bw


def items_from_combined(per, emission):
    """one frame of getAlignment's Baum-Welch branch behind combineItems (Aligner.cc:713-720) on {label: f32 -log p}: clipWeights,
    shiftMinToZeroWeights, expm, normalizeWeights (summed by increasing -log p) and filterWeightsGT(0) on f64 weights"""
    vals = {l: min(max(float(v), 0.0), DEAD) for l, v in per.items()}
    if not vals:
        return []
    lo = min(vals.values())
    ws = {l: (0.0 if math.isinf(v - lo) else math.exp(-(v - lo))) for l, v in vals.items()}
    order = sorted(ws, key=lambda l: (vals[l], l))
    total = 0.0
    for l in order:
        total += ws[l]
    inv = 1 / total if total != 0 else 1.0
    return [(l, emission[l], np.float64(ws[l] * inv)) for l in order if ws[l] * inv > 0]


def items_reference(graph, frames, rows, fw, bw):
    """Posterior64Automaton::logPosterior per arc, narrowed to f32 (Sssp.cc:156-159), on the trimmed automaton; then getAlignment's
    Baum-Welch branch (Aligner.cc:711-721): combineItems with the f32 collect, clipWeights, shiftMinToZeroWeights, expm, normalizeWeights
    and filterWeightsGT(0) on f64 item weights (Mm::Weight is f64).  Returns the items per frame as (label, emission, f64 weight) by
    increasing -log p, the arcs' (frame, label, f32 -log p) before the combination and the (frame, label, f32 -log p) after it."""
    T = len(rows)
    emission = {l: e for arcs in graph["arcs"] for _, e, l, _ in arcs}
    total_inv = -bw[0][graph["initial"]]
    out, raw, combined = [], [], []
    with np.errstate(all="ignore"):
        for f in range(T):
            pos = {s: i for i, s in enumerate(frames[f + 1])}
            per = {}
            for src in frames[f]:
                if not (fw[f][src] < DEAD and bw[f][src] < DEAD):
                    continue                                                   # Fsa::trim: no path to a final state
                arcs = sorted((pos[tgt], k) for k, (tgt, _, _, _) in enumerate(graph["arcs"][src]) if tgt in pos)
                for _, k in arcs:
                    tgt, e, l, w = graph["arcs"][src][k]
                    if not bw[f + 1][tgt] < DEAD:
                        continue
                    tmp = ((fw[f][src] + float(F32(F32(w) + rows[f][e]))) + bw[f + 1][tgt]) + total_inv
                    lp = F32(tmp) if tmp < float(F32_MAX) else F32_MAX
                    raw.append((f, l, lp))
                    per[l] = lp if l not in per else collect32(per[l], lp)
            combined.extend((f, l, per[l]) for l in sorted(per))
            out.append(items_from_combined(per, emission))
    return out, raw, combined


def align_segment(graph, scores, order="device", **cfg):
    """Aligner::feed(vector) and getAlignment in mode baum-welch over one segment.  Returns the search's dict plus items (a list per frame
    of (label, emission, weight): f32 in device order, f64 in reference order), n_items and log_total (bw[initial] in f64; DEAD without items)."""
    out, frames, rows = search(graph, scores, order, **cfg)
    T = len(scores)
    out.update(items=[[] for _ in range(T)], n_items=0, log_total=DEAD)
    if not out["reached"] or frames is None:
        return out
    if order == "device":
        fw, bw, fw_total = potentials(graph, frames, rows)
        if fw_total is None or graph["initial"] not in bw[0]:
            return out
        out["log_total"] = bw[0][graph["initial"]]
        out["items"], out["shares"] = items_device(graph, frames, rows, fw, bw, fw_total)
    else:
        fw, bw = potentials_reference(graph, frames, rows)
        out["log_total"] = bw[0][graph["initial"]]
        out["items"], out["raw"], out["combined"] = items_reference(graph, frames, rows, fw, bw)
    out["n_items"] = sum(len(f) for f in out["items"])
    return out


def flat_items(results, frame_offsets):
    """the item arrays amx_bw_items_dev copies out for a batch of align_segment results: frame, label, emission, weight, the offsets per
    matrix row and (device order) the f64 shares behind the weights"""
    rows = int(frame_offsets[-1])
    frame, label, emission, weight, share, offsets = [], [], [], [], [], np.zeros(rows + 1, np.int64)
    for s, r in enumerate(results):
        for f, its in enumerate(r["items"]):
            t = int(frame_offsets[s]) + f
            offsets[t + 1] = len(its)
            for l, e, w in its:
                frame.append(t), label.append(l), emission.append(e), weight.append(w)
            if "shares" in r:
                share.extend(r["shares"][f])
    return (np.array(frame, np.int32), np.array(label, np.int32), np.array(emission, np.int32), np.array(weight, np.float32), np.cumsum(offsets),
            np.array(share, np.float64))


def midpoint_distance(share):
    """relative distance of f64 values to the nearest boundary between two f32 roundings"""
    v = np.asarray(share, np.float64)
    w = v.astype(np.float32)
    up = (w.astype(np.float64) + np.nextafter(w, np.float32(np.inf)).astype(np.float64)) / 2
    dn = (w.astype(np.float64) + np.nextafter(w, np.float32(-np.inf)).astype(np.float64)) / 2
    return np.minimum(np.abs(v - up), np.abs(v - dn)) / v
