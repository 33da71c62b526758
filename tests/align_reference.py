"""Plain restatement of the reference's Viterbi alignment (Search/Aligner.cc: SearchSpace::expand, activateOrUpdateStateHypothesisViterbi,
prune, minimumScore, finalStatePotential, getAlignmentFsaViterbi; Aligner::feed): an explicit hypothesis list per frame, f32 arithmetic,
plain Python loops.  tests/test_align.py holds it against the reference's own results (tests/golden/ref_align.npz) bit for bit; the GPU
tests hold the library against it.

A graph is a dict: n_states, initial, final (bool [n_states]), final_weight (f32 [n_states]) and arcs, a list per source state of
(target, emission, label, weight) in the reference's arc order.
"""
import numpy as np

F32 = np.float32
F32_MAX = np.finfo(np.float32).max
F32_EPSILON = np.finfo(np.float32).eps      # Core::Type<f32>::epsilon
F32_DELTA = np.finfo(np.float32).tiny       # Core::Type<f32>::delta (FLT_MIN)
INT_MAX = 2 ** 31 - 1
DEFAULTS = dict(min_acoustic_pruning=50.0, max_acoustic_pruning=float(F32_MAX), increment_factor=2.0, min_average_number_of_states=0.0,
                increase_until_no_score_difference=1, score_scale=1.0)


def is_almost_equal(a, b):
    """Core::isAlmostEqual(f32, f32) with tolerance 1 (Core/Utility.hh:316-321)"""
    with np.errstate(all="ignore"):
        d = np.abs(F32(a) - F32(b))
        e = F32(F32(F32(np.abs(F32(a)) + np.abs(F32(b))) + F32_DELTA) * F32_EPSILON) * F32(1)
    return bool(d < e)


class NanMet(Exception):
    """the library's added rule: a NaN candidate score ends the search of the segment"""


def one_pass(graph, rows, threshold):
    """restart() and feed() of every frame at one threshold.  rows: f32 [T, n_columns], already scaled.  Returns the hypothesis lists per
    frame (lists of [state, score, trace, label, emission]; trace indexes the previous frame's list after pruning), the survivor count per
    frame and whether anything was pruned."""
    arcs = graph["arcs"]
    hyps = [[graph["initial"], F32(0), -1, -1, -1]]
    frames, counts, pruned = [hyps], [], False
    t = F32(threshold)
    with np.errstate(all="ignore"):
        for row in rows:
            new, where = [], {}
            for shi, (state, score, _, _, _) in enumerate(hyps):             # expand (:215-252)
                for target, emission, label, weight in arcs[state]:
                    sco = F32(F32(score + F32(weight)) + row[emission])
                    if np.isnan(sco):
                        raise NanMet()
                    at = where.get(target)
                    if at is None:                                            # :150-155: the first candidate fixes the position
                        where[target] = len(new)
                        new.append([target, sco, shi, label, emission])
                    elif new[at][1] >= sco:                                   # :159-165: a later candidate that is not worse replaces
                        new[at][1:] = [sco, shi, label, emission]
            m = F32_MAX                                                       # minimumScore (:254-261)
            for h in new:
                if m > h[1]:
                    m = h[1]
            limit = F32(m + t)                                                # feed (:597)
            kept = [h for h in new if h[1] <= limit]                          # prune (:294-301), the order is kept
            pruned = pruned or len(kept) < len(new)
            # traces index the pruned list of the previous frame already (nothing of it is removed later: collectGarbage changes no result)
            hyps = kept
            frames.append(hyps)
            counts.append(len(kept))
    return frames, counts, pruned


def final_potential(graph, hyps):
    """finalStatePotential (:385-405) and the best final hypothesis of getAlignmentFsaViterbi (:408-419)"""
    result, best, best_score = F32_MAX, -1, F32_MAX
    with np.errstate(all="ignore"):
        for shi, h in enumerate(hyps):
            if graph["final"][h[0]]:
                score = F32(F32(graph["final_weight"][h[0]]) + h[1])
                if score < result:          # std::min(result, score)
                    result = score
                if score < best_score:
                    best_score, best = score, shi
    return result, best


def align_segment(graph, scores, **cfg):
    """Aligner::feed(vector) (:603-630) and getAlignmentFsa over one segment.  scores: f32 [T, n_columns].  Returns a dict: label, emission
    (int32 [T], -1 where no final state was reached), arc_score (f32 [T], 0 there), score, reached, n_iterations, last_threshold,
    average_states (f64), state_sum, survivors (int32 [T] of the last pass), nan."""
    c = dict(DEFAULTS)
    c.update(cfg)
    T = len(scores)
    scale = F32(c["score_scale"])
    with np.errstate(all="ignore"):
        rows = np.asarray(scores, F32) if scale == 1 else (scale * np.asarray(scores, F32)).astype(F32)   # ScaledContextScorer::score
    lo, hi, factor = F32(c["min_acoustic_pruning"]), F32(c["max_acoustic_pruning"]), F32(c["increment_factor"])
    min_avg = float(c["min_average_number_of_states"])                      # an f64 member (Aligner.hh:110)
    out = dict(label=np.full(T, -1, np.int32), emission=np.full(T, -1, np.int32), arc_score=np.zeros(T, F32), score=F32_MAX, reached=False,
               n_iterations=0, last_threshold=F32(0), average_states=0.0, state_sum=0, survivors=np.zeros(T, np.int32), nan=False)
    previous, t, frames = F32_MAX, lo, None
    with np.errstate(all="ignore"):
        while t <= hi:
            out["n_iterations"] += 1
            out["last_threshold"] = t
            try:
                frames, counts, _ = one_pass(graph, rows, t)
            except NanMet:
                out["nan"] = True
                return out
            score, best = final_potential(graph, frames[-1])
            out["score"], out["reached"] = score, bool(score != F32_MAX)
            out["state_sum"] = int(sum(counts))
            out["average_states"] = float(np.float64(out["state_sum"]) / np.float64(T)) if T else float("nan")
            out["survivors"] = np.array(counts, np.int32).reshape(T)
            if factor <= 1:
                break
            if out["reached"] and out["average_states"] >= min_avg:
                if not c["increase_until_no_score_difference"]:
                    break
                if t > lo and is_almost_equal(score, previous):
                    break
            previous = score
            t = F32(t * factor)
        if frames is None or not out["reached"] or best < 0:
            return out
        shi = best                                                             # getAlignmentFsaViterbi (:430-442)
        for time in range(T, 0, -1):
            h = frames[time][shi]
            out["label"][time - 1], out["emission"][time - 1] = h[3], h[4]
            out["arc_score"][time - 1] = F32(h[1] - frames[time - 1][h[2]][1])
            shi = h[2]
    return out


def count_executed_passes(graph, scores, **cfg):
    """how many passes have to be run when a pass that pruned nothing ends the work: what the device does"""
    c = dict(DEFAULTS)
    c.update(cfg)
    scale = F32(c["score_scale"])
    rows = np.asarray(scores, F32) if scale == 1 else (scale * np.asarray(scores, F32)).astype(F32)
    t, hi, factor, n = F32(c["min_acoustic_pruning"]), F32(c["max_acoustic_pruning"]), F32(c["increment_factor"]), 0
    r = align_segment(graph, scores, **cfg)
    with np.errstate(all="ignore"):
        while t <= hi and n < r["n_iterations"]:
            n += 1
            try:
                _, _, pruned = one_pass(graph, rows, t)
            except NanMet:
                break
            if not pruned or factor <= 1:
                break
            t = F32(t * factor)
    return n


def align_batch(graphs, frame_offsets, scores, **cfg):
    """what amx_align_viterbi_dev leaves for a batch: label, emission, arc_score over all rows of `scores` (rows outside the segments keep
    -1 / 0) and the list of per-segment results"""
    T_all = len(scores)
    label, emission, arc = np.full(T_all, -1, np.int32), np.full(T_all, -1, np.int32), np.zeros(T_all, F32)
    results = []
    for s, g in enumerate(graphs):
        a, b = int(frame_offsets[s]), int(frame_offsets[s + 1])
        r = align_segment(g, scores[a:b], **cfg)
        label[a:b], emission[a:b], arc[a:b] = r["label"], r["emission"], r["arc_score"]
        results.append(r)
    return label, emission, arc, results


# ------------------------------------------------------------------ graphs of the recorded cases

def graph(n_states, initial, finals, arcs):
    """finals: {state: weight}; arcs: list of (source, target, emission, label, weight) in the order they are added to their source"""
    g = dict(n_states=n_states, initial=initial, final=np.zeros(n_states, bool), final_weight=np.zeros(n_states, F32), arcs=[[] for _ in range(n_states)])
    for s, w in finals.items():
        g["final"][s], g["final_weight"][s] = True, F32(w)
    for s, t, e, l, w in arcs:
        g["arcs"][s].append((t, e, l, F32(w)))
    return g


def linear_hmm(n, n_columns, seed, loop=3.0, forward=1.0, skip=5.0, integer=False):
    """left to right: state 0 is the entry, state i > 0 emits column col[i]; loop, forward and skip arcs into the emitting states; the
    last state is final.  Label = 1000 + target state."""
    rng = np.random.Generator(np.random.PCG64(seed))
    col = rng.integers(0, n_columns, n + 1)
    arcs = []
    for s in range(n):
        if s > 0:
            arcs.append((s, s, col[s], 1000 + s, loop))
        if s + 1 < n:
            arcs.append((s, s + 1, col[s + 1], 1000 + s + 1, forward))
        if s + 2 < n:
            arcs.append((s, s + 2, col[s + 2], 1000 + s + 2, skip))
    if n == 1:
        arcs.append((0, 0, col[0], 1000, loop))
    return graph(n, 0, {n - 1: 0.0}, arcs)


# ------------------------------------------------------------------ the recorded cases (tests/golden/make_align_golden.py, the tests)

N_COLUMNS = 24
BATCH = ("defaults_gauss", "unreachable", "empty", "tie_labels", "variants", "finals", "lin130_T80", "lin3_T1")


def _seed(name):
    import hashlib
    return int(hashlib.sha256(name.encode()).hexdigest()[:12], 16)


def _gauss(name, T):
    rng = np.random.Generator(np.random.PCG64(_seed(name)))
    return rng.normal(60.0, 15.0, (T, N_COLUMNS)).astype(F32)


def _random_tie_graph(seed):
    """12 states, up to 4 arcs out of each in a shuffled target order, weights in {0, 1, 2}, three final states with weights in {0, 1}"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n, arcs = 12, []
    for s in range(n):
        for t in rng.permutation(n)[:int(rng.integers(1, 5))]:
            e = int(rng.integers(0, N_COLUMNS))
            arcs.append((s, int(t), e, e * 16 + int(rng.integers(0, 16)), float(rng.integers(0, 3))))
    finals = {int(s): float(rng.integers(0, 2)) for s in rng.permutation(n)[:3]}
    return graph(n, 0, finals, arcs)


def cases():
    """name -> dict(graph, scores f32 [T, N_COLUMNS], cfg).  Labels determine the emission index (label // 16 or the linear HMM's table),
    as an acoustic model's emissionIndex() does."""
    out = {}
    for n in (3, 70, 130):
        for T in (1, 2, 3, 37):
            name = "lin%d_T%d" % (n, T)
            out[name] = dict(graph=linear_hmm(n, N_COLUMNS, _seed(name) + 1), scores=_gauss(name, T),
                             cfg=dict(max_acoustic_pruning=400.0) if (n, T) == (130, 37) else {})
    out["lin130_T80"] = dict(graph=linear_hmm(130, N_COLUMNS, 5), scores=_gauss("lin130_T80", 80), cfg={})
    lab = lambda e, v=0: e * 16 + v
    # two pronunciation variants that rejoin: 0 -> (1 -> 2) | (3 -> 4 -> 5) -> 6 -> 7, loops everywhere
    arcs = [(0, 1, 1, lab(1), 1.0), (0, 3, 3, lab(3), 1.5), (1, 1, 1, lab(1), 3.0), (1, 2, 2, lab(2), 1.0), (2, 2, 2, lab(2), 3.0), (2, 6, 6, lab(6), 1.0),
            (3, 3, 3, lab(3), 3.0), (3, 4, 4, lab(4), 1.0), (4, 4, 4, lab(4), 3.0), (4, 5, 5, lab(5), 1.0), (5, 5, 5, lab(5), 3.0), (5, 6, 6, lab(6, 1), 1.0),
            (6, 6, 6, lab(6), 3.0), (6, 7, 7, lab(7), 1.0), (7, 7, 7, lab(7), 3.0)]
    out["variants"] = dict(graph=graph(8, 0, {7: 0.0}, arcs), scores=_gauss("variants", 14), cfg={})
    arcs = [(0, 1, 1, lab(1), 1.0), (1, 1, 1, lab(1), 2.0), (1, 2, 2, lab(2), 1.0), (1, 3, 3, lab(3), 1.0), (2, 2, 2, lab(2), 2.0), (3, 3, 3, lab(3), 2.0),
            (2, 4, 4, lab(4), 1.0), (3, 4, 4, lab(4, 1), 1.0), (4, 4, 4, lab(4), 2.0)]
    out["finals"] = dict(graph=graph(5, 0, {2: 7.25, 3: 0.5, 4: 3.0}, arcs), scores=_gauss("finals", 9), cfg={})
    arcs = [(0, 1, 1, lab(1), 1.0), (0, 1, 2, lab(2), 1.0), (1, 1, 1, lab(1, 1), 2.0), (1, 1, 2, lab(2, 1), 2.0), (1, 2, 3, lab(3), 1.0), (1, 2, 4, lab(4), 1.0)]
    out["parallel_arcs"] = dict(graph=graph(3, 0, {2: 0.0}, arcs), scores=_gauss("parallel_arcs", 7), cfg={})
    # exact ties: integer scores and weights
    twos = np.full((2, N_COLUMNS), 2, F32)
    out["tie_labels"] = dict(graph=graph(4, 0, {3: 0.0}, [(0, 1, 1, lab(1), 1.0), (0, 2, 2, lab(2), 1.0), (1, 3, 3, lab(3, 1), 1.0), (2, 3, 3, lab(3, 2), 1.0)]),
                             scores=twos, cfg={})
    out["tie_rank_order"] = dict(graph=graph(4, 0, {3: 0.0}, [(0, 2, 2, lab(2), 1.0), (0, 1, 1, lab(1), 1.0), (1, 3, 3, lab(3, 1), 1.0), (2, 3, 3, lab(3, 2), 1.0)]),
                                 scores=twos, cfg={})
    out["tie_finals"] = dict(graph=graph(3, 0, {1: 0.0, 2: 0.0}, [(0, 2, 2, lab(2), 1.0), (0, 1, 1, lab(1), 1.0)]), scores=twos[:1], cfg={})
    for i in range(3):
        rng = np.random.Generator(np.random.PCG64(900 + i))
        out["tie_random%d" % i] = dict(graph=_random_tie_graph(700 + i), scores=rng.integers(0, 4, (12, N_COLUMNS)).astype(F32), cfg={})
    # pruning
    chains = [(0, 1, 0, lab(0), 0.0), (1, 2, 1, lab(1), 0.0), (2, 3, 2, lab(2), 0.0), (0, 4, 3, lab(3), 0.0), (4, 5, 4, lab(4), 0.0), (5, 6, 5, lab(5), 0.0)]
    s = np.full((3, N_COLUMNS), 9, F32)
    s[:, 0:3] = np.array([[1, 9, 9], [9, 50, 9], [9, 9, 50]], F32)
    s[:, 3:6] = np.array([[20, 9, 9], [9, 1, 9], [9, 9, 1]], F32)
    out["prune_best_first"] = dict(graph=graph(7, 0, {3: 0.0, 6: 0.0}, chains), scores=s, cfg=dict(min_acoustic_pruning=10.0))
    out["defaults_gauss"] = dict(graph=linear_hmm(40, N_COLUMNS, 11), scores=_gauss("defaults_gauss", 60), cfg={})
    out["factor1"] = dict(graph=linear_hmm(40, N_COLUMNS, 12), scores=_gauss("factor1", 60),
                          cfg=dict(min_acoustic_pruning=80.0, max_acoustic_pruning=80.0, increment_factor=1.0))
    out["min_average"] = dict(graph=linear_hmm(40, N_COLUMNS, 13), scores=_gauss("min_average", 60), cfg=dict(min_average_number_of_states=18.0))
    out["no_increase"] = dict(graph=linear_hmm(40, N_COLUMNS, 14), scores=_gauss("no_increase", 60), cfg=dict(increase_until_no_score_difference=0))
    out["unreachable"] = dict(graph=graph(6, 0, {5: 0.0}, [(i, i + 1, i + 1, lab(i + 1), 1.0) for i in range(5)] + [(i, i, i, lab(i, 1), 2.0) for i in range(1, 6)]),
                              scores=_gauss("unreachable", 3), cfg={})
    out["empty"] = dict(graph=linear_hmm(3, N_COLUMNS, 15), scores=np.zeros((0, N_COLUMNS), F32), cfg={})
    out["empty_final"] = dict(graph=graph(2, 0, {0: 2.5, 1: 0.0}, [(0, 1, 1, lab(1), 1.0)]), scores=np.zeros((0, N_COLUMNS), F32), cfg={})
    g = linear_hmm(20, N_COLUMNS, 16)
    s = _gauss("fltmax_columns", 30)
    used = sorted({e for a in g["arcs"] for _, e, _, _ in a})
    s[:, used[1]] = F32_MAX
    s[:, used[4]] = F32_MAX
    s[::3, used[7]] = F32_MAX
    out["fltmax_columns"] = dict(graph=g, scores=s, cfg={})
    out["scale"] = dict(graph=linear_hmm(40, N_COLUMNS, 17), scores=_gauss("scale", 50), cfg=dict(score_scale=0.37))
    return out


def batch_case(all_cases):
    """the eight segments of BATCH in one call: (graphs, frame_offsets, scores)"""
    graphs = [all_cases[n]["graph"] for n in BATCH]
    lens = [len(all_cases[n]["scores"]) for n in BATCH]
    return graphs, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate([all_cases[n]["scores"] for n in BATCH])
