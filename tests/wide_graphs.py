"""Deterministic wide alignment graphs and score matrices for tests/test_align_wide.py (CPU: the inputs do what is claimed) and
tests/test_align_wide_gpu.py (the device against the restatements): shapes taken from the kernels' own constants (256 lanes, 8 ranks and
16 row words per lane, 64 arcs out of a state, 2048 states, 4096 emissions and labels per segment, 256 rows per scan chunk), where the
cases of tests/align_reference.py are toys.  numpy only, every draw from a PCG64 seed.

Every generator returns the graph dict of align_reference.graph().  A label has exactly one emission (label = 16 * emission + v, as the
recorded cases have it); arc weights are 0, 1 or 2 and final weights 0 or 1, so with an integer score matrix every Viterbi sum is exact
and ties are everywhere.  scores() fills every column no arc reads with NaN: a wrong column read flags the segment (both libraries' NaN
rule) and cannot pass as a plausible number."""
import numpy as np

from tests import align_reference as ar

F32 = np.float32
N_COLUMNS, LD = 10000, 10003      # every wide case's matrix: 10000 emissions, rows 10003 words apart
MAX_OUT = 64                      # AMX_ALIGN_MAX_OUT_ARCS


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _pool(rng, n, n_columns):
    """n distinct columns in increasing order, the first and the last column among them"""
    assert 2 <= n <= n_columns
    inner = rng.choice(n_columns - 2, n - 2, replace=False) + 1
    return np.sort(np.concatenate([[0], inner, [n_columns - 1]])).astype(np.int64)


def _weight(rng):
    return float(rng.integers(0, 3))


def layered(widths, fan, n_columns, seed, n_emissions=24, entry_loop=False, label_by_target=False):
    """State 0 is the entry, then layers of the given widths; the last layer is final.  Every state of a layer has a self-loop and
    `fan` arcs (an int, or one per pair of layers) into the next layer in a shuffled target order, dealt from shuffled decks of the next
    layer so that EVERY state of it is a target.  The entry has arcs into min(64, widths[0]) states of the first layer (with entry_loop:
    a self-loop and at most 63).  label_by_target: all arcs into a state carry that state's own label, distinct from every other
    state's; otherwise every arc draws its emission from the pool of n_emissions columns and its v from 0 .. 15."""
    rng = _rng(seed)
    widths = [int(w) for w in widths]
    fans = [int(fan)] * (len(widths) - 1) if np.isscalar(fan) else [int(f) for f in fan]
    assert len(fans) == len(widths) - 1
    first = np.concatenate([[1], 1 + np.cumsum(widths)]).astype(int)
    n = int(first[-1])
    pool = _pool(rng, n_emissions, n_columns)
    own = None
    if label_by_target:
        assert n <= 16 * n_emissions
        own = [(int(pool[p // 16]), int(16 * pool[p // 16] + p % 16)) for p in rng.permutation(16 * n_emissions)[:n]]

    def arc(s, t):
        if own is not None:
            e, l = own[t]
        else:
            e = int(pool[rng.integers(n_emissions)])
            l = 16 * e + int(rng.integers(16))
        return (s, int(t), e, l, _weight(rng))

    arcs = [arc(0, 0)] if entry_loop else []
    arcs += [arc(0, first[0] + t) for t in rng.permutation(widths[0])[:min(MAX_OUT - bool(entry_loop), widths[0])]]
    for k, W in enumerate(widths):
        if k + 1 == len(widths):
            arcs += [arc(first[k] + i, first[k] + i) for i in range(W)]
            break
        V, f = widths[k + 1], fans[k]
        assert W * f >= V and f <= V and f + 1 <= MAX_OUT, (W, f, V)
        deck = np.concatenate([rng.permutation(V) for _ in range((W * f + V - 1) // V)])[:W * f]   # its first V cards are all of the layer
        for i in range(W):
            hand, seen = [], set()
            for t in deck[i * f:(i + 1) * f]:
                while int(t) in seen:   # the other copy stays in this hand: the layer stays covered
                    t = rng.integers(V)
                seen.add(int(t)), hand.append(int(t))
            s = first[k] + i
            arcs.append(arc(s, s))
            arcs += [arc(s, first[k + 1] + hand[j]) for j in rng.permutation(f)]
    finals = {int(first[-2] + i): float(rng.integers(0, 2)) for i in range(widths[-1])}
    return ar.graph(n, 0, finals, arcs)


def funnel(n, n_columns, seed, n_emissions=24):
    """n - 1 states that all go into one final sink (state n - 1, in-degree n - 1), all arcs into the sink under ONE label on a column of
    its own.  The entry reaches up to 63 states, those the rest; every state between entry and sink has a self-loop."""
    rng = _rng(seed)
    assert n >= 4
    pool = _pool(rng, n_emissions, n_columns)
    sink, e_sink = n - 1, int(pool[-1])
    l_sink = 16 * e_sink + 5
    k1 = min(MAX_OUT - 1, n - 2)
    children = [[] for _ in range(n)]
    children[0] = list(range(1, 1 + k1))
    for j in range(1 + k1, n - 1):
        children[1 + (j - 1 - k1) % k1].append(j)

    def arc(s, t):
        e = int(pool[rng.integers(n_emissions - 1)])
        return (s, int(t), e, 16 * e + int(rng.integers(16)), _weight(rng))

    arcs = []
    for s in range(n - 1):
        out = [arc(s, t) for t in ([s] if s else []) + children[s]] + [(s, sink, e_sink, l_sink, _weight(rng))]
        assert len(out) <= MAX_OUT
        arcs += [out[j] for j in rng.permutation(len(out))]
    return ar.graph(n, 0, {sink: 0.0}, arcs)


def emission_wide(n_states, n_emissions, n_labels, n_columns, seed, n_arcs=None):
    """exactly n_emissions distinct emission indices out of range(n_columns), 0 and n_columns - 1 among them, and exactly n_labels
    distinct labels, given to the arcs in a shuffled (not the sorted) order.  A tree from the entry reaches every state in few frames,
    every state has a self-loop and is final; further arcs between random states bring the count to n_arcs (default: one per state
    but the entry).  The arcs of a state are in a shuffled order."""
    rng = _rng(seed)
    n = int(n_states)
    assert n >= 2 and n_emissions <= n_labels <= 16 * n_emissions
    pool = _pool(rng, n_emissions, n_columns)
    base = 16 * np.arange(n_emissions) + rng.integers(0, 16, n_emissions)          # every emission has a label
    rest = np.setdiff1d(np.arange(16 * n_emissions), base)
    ids = rng.permutation(np.concatenate([base, rng.choice(rest, n_labels - n_emissions, replace=False)]))
    labels = [(int(pool[i // 16]), int(16 * pool[i // 16] + i % 16)) for i in ids]
    k = min(60, max(2, int(np.ceil(np.sqrt(n)))))
    out = [[] for _ in range(n)]
    for i in range(1, n):
        out[(i - 1) // k].append(i)
    for i in range(n):
        out[i].append(i)
    total = sum(len(o) for o in out)
    n_arcs = total + n - 1 if n_arcs is None else int(n_arcs)
    assert n_arcs >= max(total, n_labels) and n_arcs <= MAX_OUT * n
    while total < n_arcs:
        s = int(rng.integers(1, n))
        if len(out[s]) < MAX_OUT:
            out[s].append(int(rng.integers(n)))
            total += 1
    which = np.empty(n_arcs, np.int64)
    order = rng.permutation(n_arcs)
    which[order[:n_labels]] = np.arange(n_labels)                                   # every label is on an arc
    which[order[n_labels:]] = rng.integers(0, n_labels, n_arcs - n_labels)
    arcs, a = [], 0
    for s in range(n):
        for j in rng.permutation(len(out[s])):
            e, l = labels[which[a]]
            arcs.append((s, out[s][j], e, l, _weight(rng)))
            a += 1
    return ar.graph(n, 0, {s: float(rng.integers(0, 2)) for s in range(n)}, arcs)


def symmetric(n, n_columns, seed):
    """the entry goes into n states that only loop, every arc of weight 1, every state final with weight 0, a label and an emission
    per state: with scores(.., same_columns=True) the n items of a frame have one weight, bit for bit"""
    rng = _rng(seed)
    pool = _pool(rng, n, n_columns)
    arcs = [(0, 1 + i, int(pool[i]), 16 * int(pool[i]) + 3, 1.0) for i in rng.permutation(n)]
    arcs += [(1 + i, 1 + i, int(pool[i]), 16 * int(pool[i]) + 3, 1.0) for i in range(n)]
    return ar.graph(n + 1, 0, {1 + i: 0.0 for i in range(n)}, arcs)


def used_columns(graph):
    return sorted({e for arcs in graph["arcs"] for _, e, _, _ in arcs})


def used_labels(graph):
    return sorted({l for arcs in graph["arcs"] for _, _, l, _ in arcs})


def n_arcs(graph):
    return sum(len(a) for a in graph["arcs"])


def reversed_arcs(graph, states=None):
    """the same graph with the arc order reversed inside every source state (or inside the given ones)"""
    return dict(graph, arcs=[list(reversed(a)) if states is None or s in states else list(a) for s, a in enumerate(graph["arcs"])])


def scores(T, n_columns, used, seed, integer=True, same_columns=False):
    """f32 [T, n_columns]: NaN in every column that is not in `used`; there integers 0 .. 3 (or uniform values below 4), with
    same_columns one value per frame in all of them"""
    rng = _rng(seed)
    used = np.asarray(used, np.int64)
    out = np.full((T, n_columns), np.nan, F32)
    shape = (T, 1) if same_columns else (T, len(used))
    v = rng.integers(0, 4, shape).astype(F32) if integer else (4 * rng.random(shape)).astype(F32)
    out[:, used] = np.broadcast_to(v, (T, len(used)))
    return out


# ------------------------------------------------------------------ the named cases

ACTIVE_WIDTHS = (6, 36, 200, 500, 1305)     # with the entry 2048 states; the active set grows 7, 43, 243, 743, 2048
LIMIT_STATES, LIMIT_EMISSIONS, LIMIT_LABELS = 2048, 4096, 4096
FIT_STATES, FIT_EMISSIONS = 1024, 24
SMALL = ("variants", "finals", "tie_labels", "lin3_T1")     # the recorded cases that share a call with `limits`


def arcs_that_fit(n_states, n_emissions, lds_bytes=128 * 1024):
    """the largest arc count that align.hip's launch site (amx_align_viterbi_dev, `a.lds_arcs = ...`) still puts into LDS:
    roundup16(32 S + 4 + 8 E) + 16 n_in <= kAlignLdsBytes"""
    fixed = (32 * n_states + 4 + 8 * max(n_emissions, 1) + 15) // 16 * 16
    return (lds_bytes - fixed) // 16


def batch(graphs, lens, seed, cfg=None, **kw):
    """a call: the graphs, their frame offsets, one matrix whose rows are NaN outside their own segment's columns, the configuration"""
    lens = [int(t) for t in lens]
    seeds = [seed + 1000 * s for s in range(len(lens))] if np.isscalar(seed) else list(seed)
    rows = [scores(t, N_COLUMNS, used_columns(g), sd, **kw) for g, t, sd in zip(graphs, lens, seeds)]
    return dict(graphs=list(graphs), off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                scores=np.concatenate(rows) if rows else np.zeros((0, N_COLUMNS), F32), cfg=dict(cfg or {}))


_BUILD = {}
_CASES = {}


def _case(name):
    def add(f):
        _BUILD[name] = f
        return f
    return add


@_case("active")
def _active():
    # two graphs: a second workgroup, and seeds at which the best path runs through tied candidates (tests/test_align_wide.py shows it)
    return batch([layered(ACTIVE_WIDTHS, 6, N_COLUMNS, seed, entry_loop=True) for seed in (15, 17)], [8, 8], (16, 18))


@_case("active_pruned")
def _active_pruned():
    # three passes (2, 4, 8): the average is reached in the last one only, which still prunes
    return dict(case("active"), cfg=dict(min_acoustic_pruning=2.0, max_acoustic_pruning=8.0, min_average_number_of_states=500.0))


@_case("active_counted")
def _active_counted():
    # no pass satisfies the average, so the loop runs to the last threshold: the passes behind the first that prunes nothing are counted
    return dict(case("active"), cfg=dict(min_acoustic_pruning=1.0, max_acoustic_pruning=64.0, min_average_number_of_states=1e9))


@_case("fan64")
def _fan64():
    # seeds at which the position of the entry's 64th arc decides the labels (tests/test_align_wide.py shows it)
    return batch([layered((64, 32, 8), (8, 4), N_COLUMNS, seed) for seed in (31, 47)], [5, 5], (32, 48))


@_case("funnel")
def _funnel():
    return batch([funnel(2048, N_COLUMNS, 31)], [4], 32)


@_case("em256")
def _em256():
    return batch([emission_wide(300, 256, 256, N_COLUMNS, 41)], [4], 42)


@_case("em257")
def _em257():
    return batch([emission_wide(300, 257, 300, N_COLUMNS, 43)], [4], 44)


@_case("em4096")
def _em4096():
    return batch([emission_wide(1500, 4096, 4096, N_COLUMNS, 45)], [4], 46)


@_case("limits")
def _limits():
    return batch([emission_wide(LIMIT_STATES, LIMIT_EMISSIONS, LIMIT_LABELS, N_COLUMNS, 51)], [5], 52)


@_case("items")
def _items():
    # a path has to advance in every frame to end in the last layer: frame f's items are the labels of layer f, one per state
    sym = symmetric(60, N_COLUMNS, 62)
    c = batch([layered((64, 257, 513, 1025), (5, 3, 3), N_COLUMNS, 61, n_emissions=128, label_by_target=True), sym], [4, 3], 63)
    c["scores"][4:] = scores(3, N_COLUMNS, used_columns(sym), 64, same_columns=True)
    return c


@_case("arcs_fit")
def _arcs_fit():
    return batch([emission_wide(FIT_STATES, FIT_EMISSIONS, 200, N_COLUMNS, 71, n_arcs=arcs_that_fit(FIT_STATES, FIT_EMISSIONS))], [4], 72)


@_case("arcs_spill")
def _arcs_spill():
    return batch([emission_wide(FIT_STATES, FIT_EMISSIONS, 200, N_COLUMNS, 71, n_arcs=arcs_that_fit(FIT_STATES, FIT_EMISSIONS) + 1)], [4], 72)


@_case("mixed_batch")
def _mixed_batch():
    small = ar.cases()
    lim = case("limits")
    graphs = [small[n]["graph"] for n in SMALL[:2]] + lim["graphs"] + [small[n]["graph"] for n in SMALL[2:]]
    rows = []
    for n in SMALL:
        m = np.full((len(small[n]["scores"]), N_COLUMNS), np.nan, F32)
        m[:, :ar.N_COLUMNS] = small[n]["scores"]
        rows.append(m)
    rows = rows[:2] + [lim["scores"]] + rows[2:]
    return dict(graphs=graphs, off=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), scores=np.concatenate(rows), cfg={})


@_case("long_call")
def _long_call():
    rng = _rng(81)
    lens = rng.choice(4, 300, p=[0.1, 0.1, 0.3, 0.5])
    graphs = [emission_wide(4 + i % 9, 3, 5, N_COLUMNS, 900 + i) for i in range(300)]
    return batch(graphs, lens, 82)


def case(name):
    """a named case, built once: dict(graphs, off, scores f32 [rows, N_COLUMNS], cfg)"""
    if name not in _CASES:
        _CASES[name] = _BUILD[name]()
    return _CASES[name]


BOTH = ("active", "active_pruned", "active_counted", "fan64", "funnel", "em256", "em257", "em4096", "limits", "items", "arcs_fit", "arcs_spill",
        "mixed_batch", "long_call")


def refused():
    """4097 distinct emissions: one more than a segment may use"""
    return emission_wide(LIMIT_STATES, LIMIT_EMISSIONS + 1, LIMIT_EMISSIONS + 1, N_COLUMNS, 91)
