"""Lattice/TimeframeError.cc:86-395, Lattice/Accuracy.cc:361-473 and the LogCollector of Fsa/tRealSemiring.cc:168-194 restated in plain
Python and numpy.float32, operation by operation, with the reference's own containers (a dict per frame).  In the f32 instantiation
`min - *it` is an f32 difference, ::exp and ::log1p are the f64 overloads and `sum +=` adds in f64 and narrows; TimeframeError.cc's
unqualified exp(-p) is the f64 one too (found by compiling the text's calls with its system headers).  Checked by reading
against the cited lines; there is no golden file.  A lattice is a LatticeWordMeasures dict."""
import numpy as np

from tests.quanteq_reference import mad32

F32, F64 = np.float32, np.float64
F32_MIN = F32(-3.40282347e+38)


def discover(lat):
    """DfsState::dfs (Fsa/tDfs.cc:21-68): the states in discover order"""
    off, tgt = lat["arc_offsets"], lat["arc_target"]
    color, stack, order = {}, [int(lat["initial"])], []
    while stack:
        s = stack[-1]
        if s not in color:
            color[s] = 1
            order.append(s)
            stack.extend(int(t) for t in tgt[off[s]:off[s + 1]] if int(t) not in color)
        else:
            stack.pop()
    return order


def arcs(lat):
    """the reached arcs in feed order: (arc, label, start, end)"""
    off, tgt, tm, lab = lat["arc_offsets"], lat["arc_target"], lat["state_time"], lat["arc_label"]
    return [(a, int(lab[a]), int(tm[s]), int(tm[tgt[a]])) for s in discover(lat) for a in range(off[s], off[s + 1])]


def collect(feeds, exact=False):
    """LogCollector: constructor, feed ..., get -> p.  exact: the same cell all in f64 (the bars' yardstick)"""
    T = F64 if exact else F32
    m, values = T(feeds[0]), []
    for a in feeds[1:]:
        a = T(a)
        if a < m:
            values.append(m)
            m = a
        else:
            values.append(a)
    if not values:
        return m
    total = T(np.exp(F64(T(m - values[0]))))
    for v in values[1:]:
        total = T(F64(total) + np.exp(F64(T(m - v))))
    return T(F64(m) - np.log1p(F64(total)))


def cell_score(p, exact=False):
    return (F64 if exact else F32)(1.0 - np.exp(-F64(p)))


def cells(lat, weight):
    """TimeframeErrorDfsState: {(frame, label): the feeds in order}"""
    acc = {}
    for a, label, s, e in arcs(lat):
        for t in range(s, e):
            acc.setdefault((t, label), []).append(F32(weight[a]))
    return acc


def den(normalization, s, e, fma):
    return F32(mad32(fma, F32(normalization), F32(np.uint32((e - s - 1) & 0xFFFFFFFF)), F32(1)))


def timeframe_errors(lat, weight, maximum=False, normalization=0.0, fma=False):
    """-> (f32 per arc, None | (frame, label) of the first cell that fails verify(p > -0.001), {cell: (score, exact score, feeds)})"""
    table, bad = {}, None
    for key, feeds in cells(lat, weight).items():
        p = collect(feeds)
        if not p > F32(-0.001):
            bad = min(bad, key[::-1]) if bad else key[::-1]
        table[key] = (cell_score(p), cell_score(collect(feeds, True), True), len(feeds))
    out = np.zeros(len(lat["arc_target"]), F32)
    for a, label, s, e in arcs(lat):
        v = F32_MIN if maximum else F32(0)
        for t in range(s, e):
            v = max(v, table[(t, label)][0]) if maximum else F32(v + table[(t, label)][0])
        with np.errstate(all="ignore"):
            out[a] = v if maximum else F32(v / den(normalization, s, e, fma))
    return out, bad and bad[::-1], table


def frame_word_accuracy(lat, correct, normalization=0.0, fma=False):
    marks = {(t, label) for _, label, s, e in arcs(correct) for t in range(s, e)}
    out = np.zeros(len(lat["arc_target"]), F32)
    for a, label, s, e in arcs(lat):
        total = F32(0)
        for t in range(s, e):
            total = F32(total + F32((t, label) in marks))
        with np.errstate(all="ignore"):
            out[a] = F32(total / den(normalization, s, e, fma))
    return out


def approximate_word(lat, correct, short_pauses=()):
    active = {}
    for _, label, s, e in arcs(correct):
        for t in range(s, e):
            active.setdefault(t, {}).setdefault(label, set()).add((s, e))
    out = np.zeros(len(lat["arc_target"]), F32)
    for a, label, hs, he in arcs(lat):
        if label in short_pauses:
            continue
        refs = {}
        for t in range(hs, he):
            for rl, ivs in active.get(t, {}).items():
                refs.setdefault(rl, set()).update(ivs)
        acc = F32_MIN if refs else F32(0)
        for rl, ivs in refs.items():
            for rs, re in ivs:
                o = F32(min(he, re) - max(hs, rs)) / F32(re - rs)
                acc = max(F32(-1) + (F32(2) * o if rl == label else o), acc)
        out[a] = acc
    return out


def lattice(times, arc_list, initial=0):
    """a lattice dict from state times and (source, target, label) triples; a state's arcs keep the order of the list"""
    by = sorted(range(len(arc_list)), key=lambda i: arc_list[i][0])
    off = np.zeros(len(times) + 1, np.int64)
    for s, _, _ in arc_list:
        off[s + 1] += 1
    n = len(times)
    return dict(arc_offsets=np.cumsum(off), arc_target=np.array([arc_list[i][1] for i in by], np.int32), arc_label=np.array([arc_list[i][2] for i in by], np.int32),
                state_time=np.array(times, np.int32), initial=initial, arc_weight=np.zeros(len(by), np.float32), final_flag=np.isin(np.arange(n), (1, 3)),
                final_weight=np.zeros(n, np.float32))
