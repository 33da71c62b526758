"""Plain restatement of the lattice best path and forward-backward pruning (rasr_amd.LatticeBest, include/amx.h): Fsa::bestscore, Fsa::best
and Fsa::prunePosterior in the tropical semiring of tolerance 1, operation by operation in f32 (np.float32 scalars), and the named cases
of tests/test_latbest.py and tests/test_latbest_gpu.py.  A lattice is LatticePosterior's dict: arc_offsets, arc_target, arc_weight,
initial, final_flag, final_weight.  The loops are the reference's own (the stack walk, the topological queue with d and r, getState's
searches), not the level plan of the library."""
import functools
import heapq
import itertools

import numpy as np

F32 = np.float32
ZERO = F32(3.40282347e+38)      # zero() and max()
INVALID = F32(-3.40282347e+38)  # invalid() = Core::Type<f32>::min
OK, NO_FINAL = 0, 1
LDS_STATES = 8192   # amx_latbest_kernel_shape (tests/test_latbest.py holds it to the library's)


def _wrap(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def difference_ulp(a, b):
    """Core::differenceUlp(f32, f32), the s32 arithmetic wrapping"""
    a, b = (int(np.array(x, np.float32).view(np.int32)) for x in (a, b))
    if a < 0:
        a = _wrap(0x80000000 - a)
    if b < 0:
        b = _wrap(0x80000000 - b)
    d = _wrap(a - b)
    return _wrap(-d) if d < 0 else d


def compare(a, b):
    """LogSemiring::compare with tolerance 1"""
    if a == b or difference_ulp(a, b) <= 1:
        return 0
    return -1 if a < b else 1


def ulps(x, k):
    """x moved by k units in the last place"""
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def n_states(lat):
    return len(lat["arc_offsets"]) - 1


def dfs(n, start, targets):
    """DfsState::dfs -> (discover order, topologicallySort's numbers: descending finishing time, -1 not reached)"""
    color, stack, discover, finish = [0] * n, [start], [], []
    while stack:
        s = stack[-1]
        if color[s] == 0:
            color[s] = 1
            discover.append(s)
            stack.extend(t for t in targets(s) if color[t] == 0)
        else:
            if color[s] == 1:
                color[s] = 2
                finish.append(s)
            stack.pop()
    number = [-1] * n
    for i, s in enumerate(finish):
        number[s] = len(finish) - 1 - i
    return discover, number


def sssp(n, start, arcs, s2t):
    """ssspLoop with the TopologicalSsspQueue: d, r, collect = min, the tolerant test"""
    d, r = [ZERO] * n, [ZERO] * n
    d[start] = r[start] = F32(0)
    queue, queued = [(s2t[start], start)], {start}
    while queue:
        _, s = heapq.heappop(queue)
        queued.discard(s)
        R, r[s] = r[s], ZERO
        for t, w in arcs(s):
            ext = R + w
            m = ext if ext < d[t] else d[t]
            if compare(d[t], m) != 0:
                d[t] = m
                r[t] = ext if ext < r[t] else r[t]
                if t not in queued:
                    heapq.heappush(queue, (s2t[t], t))
                    queued.add(t)
    return d


@functools.lru_cache(maxsize=None)
def _walks(name):
    """what does not depend on the pruning options: orders, potentials, best arcs, path"""
    lat = CASES[name][0]
    n, ini = n_states(lat), int(lat["initial"])
    off, tgt = [int(x) for x in lat["arc_offsets"]], [int(x) for x in lat["arc_target"]]
    w, fw_ = np.asarray(lat["arc_weight"], np.float32), np.asarray(lat["final_weight"], np.float32)
    final = [bool(x) for x in lat["final_flag"]]
    arcs_of = lambda s: range(off[s], off[s + 1])   # noqa: E731
    with np.errstate(all="ignore"):
        discover, topo_f = dfs(n, ini, lambda s: [tgt[a] for a in arcs_of(s)])
        fw = sssp(n, ini, lambda s: [(tgt[a], w[a]) for a in arcs_of(s)], topo_f)
        # transpose: arcs appended in discover order of their sources; node n is the new initial state
        tr = [[] for _ in range(n + 1)]
        for u in discover:
            for a in arcs_of(u):
                tr[tgt[a]].append((u, w[a]))
            if final[u]:
                tr[n].append((u, fw_[u]))
        dead = not tr[n]
        topo_b, topo_super, bw, coreached = [-1] * n, -1, [ZERO] * n, 0
        if not dead:
            found, m = dfs(n + 1, n, lambda s: [t for t, _ in tr[s]])
            topo_b, topo_super, coreached = m[:n], m[n], len(found) - 1
            bw = sssp(n + 1, n, lambda s: tr[s], m)[:n]
        best_arc = [-1] * n
        if not dead:
            for s in discover:
                mn = ZERO
                for a in arcs_of(s):
                    c = w[a] + bw[tgt[a]]
                    if compare(c, mn) < 0:
                        mn, best_arc[s] = c, a
                if final[s] and compare(fw_[s], mn) < 0:
                    best_arc[s] = -1
        path, s = [], ini
        while best_arc[s] >= 0:
            path.append(best_arc[s])
            s = tgt[best_arc[s]]
    return dict(n=n, ini=ini, off=off, tgt=tgt, w=w, final=final, discover=discover, topo_forward=topo_f, topo_backward=topo_b, topo_super=topo_super,
                fw=np.array(fw, np.float32), bw=np.array(bw, np.float32), dead=dead, best_arc=best_arc, path=path, coreached=coreached,
                best_score=INVALID if dead else bw[ini])


@functools.lru_cache(maxsize=None)
def best(name, threshold=None, relative=True, trim=False):
    """every output of LatticeBest.run for the named case (arc numbers within the lattice)"""
    k = _walks(name)
    n, off, tgt, w, fw, bw = k["n"], k["off"], k["tgt"], k["w"], k["fw"], k["bw"]
    n_arcs, prune = len(tgt), threshold is not None and F32(threshold) < ZERO
    keep, mn, after = [1] * n_arcs, ZERO, ZERO
    with np.errstate(all="ignore"):
        score = lambda s, a: fw[s] + (w[a] + bw[tgt[a]])   # noqa: E731
        if prune:
            keep = [0] * n_arcs
        if prune and not k["dead"]:
            if relative:
                for s in k["discover"]:
                    for a in range(off[s], off[s + 1]):
                        if compare(score(s, a), mn) < 0:
                            mn = score(s, a)
            else:
                mn = bw[k["ini"]]
            after = mn + F32(threshold)
            for s in k["discover"]:
                for a in range(off[s], off[s + 1]):
                    keep[a] = int(compare(score(s, a), after) <= 0)
    if trim:
        src = [s for s in range(n) for _ in range(off[s], off[s + 1])]
        back = [[] for _ in range(n)]
        for a in range(n_arcs):
            if keep[a]:
                back[tgt[a]].append(src[a])
        reach = set(dfs(n, k["ini"], lambda s: [tgt[a] for a in range(off[s], off[s + 1]) if keep[a]])[0])
        co = set()
        for f in k["discover"]:
            if k["final"][f] and f not in co:
                co.update(dfs(n, f, lambda s: [u for u in back[s] if u not in co])[0])
        keep = [int(keep[a] and src[a] in reach and tgt[a] in co) for a in range(n_arcs)]
    kept_index = (np.cumsum(keep) - 1).astype(np.int32) if n_arcs else np.zeros(0, np.int32)
    kept_index[np.asarray(keep, bool) == 0] = -1
    info = dict(best_score=F32(k["best_score"]), min_weight=F32(mn), min_weight_threshold=F32(after), reason=NO_FINAL if k["dead"] else OK,
                path_length=len(k["path"]), kept_arcs=int(sum(keep)), total_arcs=n_arcs, states_reached=len(k["discover"]),
                states_coreached=k["coreached"])
    return dict(forward=fw, backward=bw, best_arc=np.array(k["best_arc"], np.int32), path=np.array(k["path"] + [-1] * (n - len(k["path"])), np.int32),
                keep=np.array(keep, np.uint8), kept_index=kept_index, info=info)


# ---- the cases: name -> (lattice, threshold)

def lattice(arcs, n, finals, initial=0):
    """arcs: (source, target, weight) in the automaton's order per source; finals: {state: weight}"""
    by = [[] for _ in range(n)]
    for a in arcs:
        by[a[0]].append(a)
    off = np.cumsum([0] + [len(b) for b in by]).astype(np.int64)
    flat = [a for b in by for a in b]
    fw = np.zeros(n, np.float32)
    for s, v in finals.items():
        fw[s] = v
    return dict(arc_offsets=off, arc_target=np.array([a[1] for a in flat], np.int32), arc_weight=np.array([a[2] for a in flat], np.float32),
                initial=initial, final_flag=np.array([s in finals for s in range(n)], np.uint8), final_weight=fw)


def _near(rng, k):
    """k values within a few ulps of each other, in random order"""
    return [ulps(3.0, int(j)) for j in rng.integers(-4, 5, k)]


def _cases():
    c, rng = {}, np.random.default_rng(26)
    for k in (1, 2, 63, 64, 65, 127, 128, 129, 300):
        # k parallel arcs 0 -> 1: an out-fan and an in-fan of k in the source's arc order
        c["par%d" % k] = (lattice([(0, 1, v) for v in _near(rng, k)], 2, {1: 0.25}), 1e-6)
        # 0 -> k middle states -> T: the chains' order is the topological order of the middle states; a level of k states
        first = [F32(rng.uniform(1, 2)) for _ in range(k)]
        arcs = [(0, 1 + i, first[i]) for i in range(k)] + [(1 + i, k + 1, F32(t - first[i])) for i, t in enumerate(_near(rng, k))]
        c["fan%d" % k] = (lattice(arcs, k + 2, {k + 1: 0.5}), 1e-6)
    x = F32(1.0)
    for order in itertools.permutations((0, 1, 2)):
        vals = [ulps(x, j) for j in order]
        c["tie3_%d%d%d" % order] = (lattice([(0, 1 + i, v) for i, v in enumerate(vals)] + [(1 + i, 4, 0.0) for i in range(3)], 5, {4: 0.0}), 0.5)
    for j in (0, 1, 2):
        for swap in (0, 1):
            vals = [ulps(x, j), x][::-1 if swap else 1]
            c["tie2_%d_%d" % (j, swap)] = (lattice([(0, 1, vals[0]), (0, 2, vals[1]), (1, 3, 0.0), (2, 3, 0.0)], 4, {3: 0.0}), 0.5)
        if j:
            c["bestarc_%d" % j] = (lattice([(0, 1, ulps(x, j)), (0, 1, x)], 2, {1: 0.0}), 0.5)
    c["final_below"] = (lattice([(0, 1, x)], 2, {0: ulps(x, -1), 1: 0.0}), 0.5)
    # minWeight = f32(1 + 0.5): arcs at -2 ... +2 ulps of it
    c["keep_ulps"] = (lattice([(0, 1, x)] + [(0, 1, ulps(1.5, j)) for j in (2, -2, 1, 0, -1)], 2, {1: 0.0}), 0.5)
    # 0 -> 3 (0.5) is the best path; along 0 -> 1 -> 2 -> 3 the arc scores round differently: 1 + 1 ulp, 1 + 1 ulp, 1.  With
    # minWeight = 1 - 2^-24 (absolute) the last arc is kept one ulp above it and the two before it, two ulps above, are not
    h = F32(2.0 ** -24)
    c["dead_arc"] = (lattice([(0, 3, 0.5), (0, 1, 1.0), (1, 2, h), (2, 3, h)], 4, {3: 0.0}), F32(0.5) - h)
    c["no_final"] = (lattice([(0, 1, 1.0), (0, 2, 2.0), (1, 2, 0.5)], 3, {}), 0.5)
    c["unreached"] = (lattice([(0, 1, 1.0), (0, 2, 0.25), (1, 3, 1.0), (1, 2, 2.0), (2, 3, 0.5), (4, 1, 0.125), (4, 3, 0.125)], 5, {3: 0.0, 0: 0.0}, initial=1), 1.0)

    def random_dag(n, fan, seed):
        r = np.random.default_rng(seed)
        ident = r.permutation(n)   # state ids do not follow the topological order
        arcs = []
        for i in range(n - 1):
            for j in r.integers(i + 1, min(n, i + 1 + 40), r.integers(1, fan + 1)):
                arcs.append((int(ident[i]), int(ident[j]), ulps(F32(r.integers(1, 12)) * F32(0.25), int(r.integers(-1, 2)))))
        finals = {int(ident[i]): float(r.integers(0, 4)) * 0.25 for i in list(r.integers(n // 2, n, 5)) + [n - 1]}
        return lattice(arcs, n, finals, initial=int(ident[3]))
    c["random600"] = (random_dag(600, 4, 7), 1.0)
    for n in (LDS_STATES - 1, LDS_STATES + 1):   # a ladder i -> i + 1, i -> i + 2 one state below and one above the LDS limit
        r = np.random.default_rng(n)
        arcs = [(i, i + d, F32(r.integers(1, 9)) * F32(0.125)) for i in range(n - 1) for d in (1, 2) if i + d < n]
        c["lds%d" % n] = (lattice(arcs, n, {n - 1: 0.0}), 0.25)
    return c


CASES = _cases()
