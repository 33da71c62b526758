"""Plain-Python restatement of the lattice arc posteriors (amx_latpost_*): Fsa::posterior64 and Fsa::posteriorE (Fsa/Sssp.cc:95-375), the
stack walk of Fsa/tDfs.cc:21-68, the transposition of Fsa/tRational.cc:594-689 and Fsa::expm (Fsa/Arithmetic.cc:47-61), operation by
operation in the reference's order; f64 is Python's float, f32 a float holding an f32 value, exp and log1p are the host libm's (the functions
the reference's build calls).  tests/golden/ref_latpost.npz holds what the reference's own text computes; test_latpost.py holds this file
to it in every bit, in both builds.

A lattice is a dict: arc_offsets [n + 1], arc_target, arc_weight, arc_risk, initial, final_flag [n], final_weight, final_risk.

contract "fma": numSum += p * (risk + generalized[target]) is one fused multiply-add (the reference's default build), "off": two roundings.
DEFECTS are planted mistakes; each is visible in the bits of a named case (CASE_OF_DEFECT) except "expectation-min-nonstrict", which
cannot be: the expectation pass uses its minimum as a VALUE only (no arc is left out of denSum), and the value of a minimum does not
depend on which of two equal candidates supplied it -- not even for +0 against -0, since a tie means two terms exp(0) = 1, so
log1p(denSum - 1) is not 0 and the sign of a zero minimum does not reach the result.  test_latpost.py asserts exactly that.
The library's choices where the reference defines nothing (Zero potentials where a walk does not come, dead outputs) are restated too."""
import math
import sys

import numpy as np

from tests.cmllr_reference import fma_exact

ZERO = sys.float_info.max                       # Core::Type<f64>::max
F32_MAX = float(np.float32(3.40282347e+38))
F32_MIN = -F32_MAX
F32_EPSILON = np.float32(1.19209290e-07)
F32_DELTA = np.float32(1.17549435e-38)
LOG, PROB, EXPECTATION = "log", "prob", "expectation"
MODES = (LOG, PROB, EXPECTATION)
OK, NO_FINAL = 0, 1
DEFECTS = ("first-minimal", "strict-minimum", "final-dropped", "incoming-by-id", "no-cap", "expm-no-isinf", "expectation-min-nonstrict",
           "contract-swapped")


def f32(x):
    """narrowing to f32, as a float"""
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def host_exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def host_log1p(x):
    if x == -1.0:
        return -math.inf
    if x < -1.0 or x != x:
        return math.nan
    return math.log1p(x)


HOST = (host_exp, host_log1p)


def arcs_of(lat, s):
    return range(int(lat["arc_offsets"][s]), int(lat["arc_offsets"][s + 1]))


def n_states(lat):
    return len(lat["arc_offsets"]) - 1


def discover_order(lat):
    """Ftl::DfsState::dfs: the states in the order they are discovered"""
    n = n_states(lat)
    color, order, stack = [0] * n, [], [int(lat["initial"])]
    while stack:
        s = stack[-1]
        if color[s] == 0:
            color[s] = 1
            order.append(s)
            for a in arcs_of(lat, s):
                t = int(lat["arc_target"][a])
                if color[t] == 0:
                    stack.append(t)
        else:
            if color[s] == 1:
                color[s] = 2
            stack.pop()
    return order


def has_cycle(lat):
    n = n_states(lat)
    indeg = [0] * n
    for t in lat["arc_target"]:
        indeg[int(t)] += 1
    todo, placed = [s for s in range(n) if not indeg[s]], 0
    while todo:
        s = todo.pop()
        placed += 1
        for a in arcs_of(lat, s):
            t = int(lat["arc_target"][a])
            indeg[t] -= 1
            if not indeg[t]:
                todo.append(t)
    return placed != n


def transpose(lat, defect=None):
    """node lists of the transposed automaton: incoming[v] = input arc indices in the reference's order, finals in discover order"""
    n = n_states(lat)
    order = discover_order(lat)
    incoming = [[] for _ in range(n)]
    for u in (sorted(order) if defect == "incoming-by-id" else order):
        for a in arcs_of(lat, u):
            incoming[int(lat["arc_target"][a])].append(a)
    finals = [s for s in order if lat["final_flag"][s]]
    return order, incoming, finals


def source_of(lat):
    src = np.zeros(len(lat["arc_target"]), np.int64)
    for s in range(n_states(lat)):
        src[int(lat["arc_offsets"][s]):int(lat["arc_offsets"][s + 1])] = s
    return src


def finish64(arcs, fin, fw, pot, defect, fn):
    """StatePotentials64DfsState::finishState: arcs = [(target, f32 weight)]"""
    exp, log1p = fn
    start_final = fin and defect != "final-dropped"
    mn, mi = (float(fw) if start_final else ZERO), -1
    for k, (t, w) in enumerate(arcs):
        score = pot[t] + float(w)
        if math.isinf(score):
            score = ZERO
        if defect == "strict-minimum":
            take = score < mn
        elif defect == "first-minimal":
            take = score < mn or (score == mn and mi < 0)
        else:
            take = score <= mn
        if take:
            mn, mi = score, k
    total = exp(mn - float(fw)) if (fin and mi >= 0) else 0.0
    for k, (t, w) in enumerate(arcs):
        if k != mi:
            score = pot[t] + float(w)
            if math.isinf(score):
                score = ZERO
            total += exp(mn - score)
    r = mn - log1p(total)
    return r if r < ZERO else ZERO


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def finish_e(arcs, fin, fw, fr, pot, gen, old, contract, defect, fn):
    """StatePotentialsEDfsState::finishState: arcs = [(target, f32 weight, f32 risk)]; old = (potential, generalized) before"""
    exp, log1p = fn
    mn = float(fw) if fin else ZERO
    for t, w, _ in arcs:
        weight = pot[t] + float(w)
        if math.isinf(weight):
            weight = ZERO
        if (mn >= weight) if defect == "expectation-min-nonstrict" else (mn > weight):
            mn = weight
    den = exp(mn - float(fw)) if fin else 0.0
    num = float(fr) * den if fin else 0.0
    fused = (contract == "fma") != (defect == "contract-swapped")
    for t, w, r in arcs:
        weight = pot[t] + float(w)
        if math.isinf(weight):
            weight = ZERO
        p = exp(mn - weight)
        x = float(r) + gen[t]
        num = fma_exact(p, x, num) if fused else num + p * x
        den += p
    if den > 0:
        return std_min(mn - log1p(den - 1), ZERO), std_max(std_min(num / den, ZERO), -ZERO)
    return old


def topological(n, arcs_out):
    indeg = [0] * n
    for s in range(n):
        for t in arcs_out[s]:
            indeg[t] += 1
    order, todo = [], [s for s in range(n) if not indeg[s]]
    while todo:
        s = todo.pop()
        order.append(s)
        for t in arcs_out[s]:
            indeg[t] -= 1
            if not indeg[t]:
                todo.append(t)
    return order


def potentials(lat, mode, contract="off", defect=None, fn=HOST):
    """-> dict(forward [n + 1] (the last: the new initial state), backward [n], generalized_forward, generalized_backward, plan fields)"""
    n, e = n_states(lat), mode == EXPECTATION
    order, incoming, finals = transpose(lat, defect)
    reached = [False] * n
    for s in order:
        reached[s] = True
    src = source_of(lat)
    tgt, w, rk = lat["arc_target"], lat["arc_weight"], lat.get("arc_risk")
    risk = (lambda a: rk[a]) if e else (lambda a: 0.0)
    topo = topological(n, [[int(tgt[a]) for a in arcs_of(lat, s)] for s in range(n)])
    bw, gbw = [ZERO] * n, [0.0] * n
    level_b, level_f, co = [-1] * n, [-1] * n, [False] * n
    for s in reversed(topo):
        if not reached[s]:
            continue
        arcs = [(int(tgt[a]), w[a], risk(a)) for a in arcs_of(lat, s)]
        fin = bool(lat["final_flag"][s])
        if e:
            bw[s], gbw[s] = finish_e(arcs, fin, lat["final_weight"][s], lat["final_risk"][s], bw, gbw, (bw[s], gbw[s]), contract, defect, fn)
        else:
            bw[s] = finish64([(t, ww) for t, ww, _ in arcs], fin, lat["final_weight"][s], bw, defect, fn)
        level_b[s] = max([level_b[t] + 1 for t, _, _ in arcs] + [0])
        co[s] = fin or any(co[t] for t, _, _ in arcs)
    fwd, gfw = [ZERO] * (n + 1), [0.0] * (n + 1)
    dead = not finals
    level_super = -1
    if not dead:
        ini = int(lat["initial"])
        for v in topo:
            if not co[v]:
                continue
            arcs = [(int(src[a]), w[a], risk(a)) for a in incoming[v]]
            fin = v == ini
            if e:
                fwd[v], gfw[v] = finish_e(arcs, fin, 0.0, 0.0, fwd, gfw, (fwd[v], gfw[v]), contract, defect, fn)
            else:
                fwd[v] = finish64([(t, ww) for t, ww, _ in arcs], fin, 0.0, fwd, defect, fn)
            level_f[v] = max([level_f[u] + 1 for u, _, _ in arcs] + [0])
        arcs = [(f, lat["final_weight"][f], lat["final_risk"][f] if e else 0.0) for f in finals]
        if e:
            fwd[n], gfw[n] = finish_e(arcs, False, 0.0, 0.0, fwd, gfw, (fwd[n], gfw[n]), contract, defect, fn)
        else:
            fwd[n] = finish64([(t, ww) for t, ww, _ in arcs], False, 0.0, fwd, defect, fn)
        level_super = max(level_f[f] for f in finals) + 1
    disc = [-1] * n
    for i, s in enumerate(order):
        disc[s] = i
    return dict(forward=fwd, backward=bw, generalized_forward=gfw, generalized_backward=gbw, dead=dead, discover_index=disc, level_backward=level_b,
                level_forward=level_f, level_super=level_super, incoming=incoming, finals=finals, coreached=co, reached=reached)


def cap(v):
    """tmp < Core::Type<f32>::max ? tmp : Core::Type<f32>::max, narrowed"""
    return f32(v) if v < F32_MAX else F32_MAX


def expm(wt, defect=None, fn=HOST):
    """Fsa::expm's ApplyExp: the f64 overload of exp, narrowed by Weight(double)"""
    if math.isinf(wt) and defect != "expm-no-isinf":
        return 0.0
    return f32(fn[0](-float(wt)))


def difference_ulp(a, b):
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    wrap = lambda v: (v + 2**31) % 2**32 - 2**31   # noqa: E731
    if ia < 0:
        ia = wrap(-2**31 - ia)
    if ib < 0:
        ib = wrap(-2**31 - ib)
    d = wrap(ia - ib)
    return wrap(-d) if d < 0 else d


def almost_equal(a, b, tolerance):
    a, b, t = np.float32(a), np.float32(b), np.float32(tolerance)
    with np.errstate(all="ignore"):
        d = np.abs(a - b)
        e = (np.abs(a) + np.abs(b) + F32_DELTA) * F32_EPSILON * t
    return bool(d < e)


def posterior(lat, mode=LOG, normalize=True, v_normalized=True, tolerance=100, contract="off", defect=None, fn=HOST):
    """-> dict(arc [n_arcs] f32, final [n] f32, info, potentials)"""
    n, e = n_states(lat), mode == EXPECTATION
    P = potentials(lat, mode, contract, defect, fn)
    fw, bw, gfw, gbw = P["forward"], P["backward"], P["generalized_forward"], P["generalized_backward"]
    ini = int(lat["initial"])
    total_inv = -bw[ini] if (e or normalize) else 0.0
    normalization = gbw[ini] if (e and v_normalized) else 0.0
    dead_value = F32_MAX if mode == LOG else 0.0
    n_arcs = len(lat["arc_target"])
    arc, final = np.full(n_arcs, dead_value, np.float32), np.full(n, dead_value, np.float32)
    src = source_of(lat)
    uncapped = defect == "no-cap"
    narrow = f32 if uncapped else cap
    if not P["dead"]:
        for a in range(n_arcs):
            s, t = int(src[a]), int(lat["arc_target"][a])
            lp = narrow(fw[s] + float(lat["arc_weight"][a]) + bw[t] + total_inv)
            if mode == LOG:
                arc[a] = lp
            elif mode == PROB:
                arc[a] = expm(lp, defect, fn)
            else:
                risk = narrow(gfw[s] + float(lat["arc_risk"][a]) + gbw[t] - normalization)
                with np.errstate(all="ignore"):
                    arc[a] = f32(np.float64(fn[0](-lp)) * np.float64(risk))
        for s in range(n):
            if not lat["final_flag"][s]:
                continue
            no_arcs = lat["arc_offsets"][s + 1] == lat["arc_offsets"][s]
            lp = 0.0 if no_arcs else narrow(fw[s] + float(lat["final_weight"][s]) + total_inv)
            if mode == LOG:
                final[s] = lp
            elif mode == PROB:
                final[s] = expm(lp, defect, fn)
            else:
                risk = 0.0 if no_arcs else narrow(float(lat["final_risk"][s]) - normalization)
                with np.errstate(all="ignore"):
                    final[s] = f32(np.float64(fn[0](-lp)) * np.float64(risk))
    inv = -bw[ini]
    inv32 = f32(inv) if e else (f32(inv) if inv > F32_MIN else F32_MIN)
    fwd_flow, bwd_flow = f32(fw[n]), f32(bw[ini])
    co = P["coreached"]
    counts = dict(reason=NO_FINAL if P["dead"] else OK, states_reached=sum(P["reached"]),
                  arcs_reached=sum(len(arcs_of(lat, s)) for s in range(n) if P["reached"][s]), states_coreached=sum(co),
                  undefined_states=n - sum(co), undefined_arcs=sum(len(arcs_of(lat, s)) for s in range(n) if not co[s]),
                  levels_forward=0 if P["dead"] else P["level_super"] + 1, levels_backward=max(P["level_backward"]) + 1)
    info = dict(total_inv=inv, total_inv_f32=inv32, expectation=f32(gbw[ini]) if e else 0.0, forward_flow=fwd_flow, backward_flow=bwd_flow,
                flows_agree=int(difference_ulp(fwd_flow, bwd_flow) <= tolerance if e else almost_equal(fwd_flow, bwd_flow, tolerance)),
                vanishing_flow=int(difference_ulp(inv32, F32_MIN) <= tolerance), **counts)
    return dict(arc=arc, final=final, info=info, potentials=P)


def same_bits(x, y):
    """two results of posterior(): the outputs and all four potentials in every bit"""
    def b(v):
        v = np.ascontiguousarray(v)
        return v.view({4: np.uint32, 8: np.uint64}[v.dtype.itemsize])
    return all(np.array_equal(b(x[k]), b(y[k])) for k in ("arc", "final")) and \
        all(np.array_equal(b(np.array(x["potentials"][k], np.float64)), b(np.array(y["potentials"][k], np.float64)))
            for k in ("forward", "backward", "generalized_forward", "generalized_backward"))


# ---------------------------------------------------------------------------------------------------------------- cases

def lattice(n, arcs, initial, finals, final_risk=None):
    """arcs: [(source, target, weight, risk)] in the automaton's order per source; finals: {state: weight}"""
    by = [[] for _ in range(n)]
    for s, t, w, r in arcs:
        by[s].append((t, w, r))
    off = np.zeros(n + 1, np.int64)
    for s in range(n):
        off[s + 1] = off[s] + len(by[s])
    flat = [x for s in range(n) for x in by[s]]
    ff, fw, fr = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for s, wt in finals.items():
        ff[s], fw[s] = 1, wt
        fr[s] = (final_risk or {}).get(s, 0.0)
    return dict(arc_offsets=off, arc_target=np.array([x[0] for x in flat], np.int32), arc_weight=np.array([x[1] for x in flat], np.float32),
                arc_risk=np.array([x[2] for x in flat], np.float32), initial=initial, final_flag=ff, final_weight=fw, final_risk=fr)


def random_dag(n, n_arcs, seed, n_final=2, shuffle=True):
    """a connected random lattice: a backbone 0 -> ... and random forward arcs; state ids shuffled so that discover order != id order"""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(n) if shuffle else np.arange(n)
    pairs = [(i, i + 1) for i in range(n - 1)]
    while len(pairs) < n_arcs:
        i = rng.randint(0, n - 1)
        pairs.append((i, rng.randint(i + 1, min(n, i + 12))))
    idx = rng.permutation(len(pairs))
    arcs = [(int(perm[pairs[k][0]]), int(perm[pairs[k][1]]), float(np.float32(rng.uniform(0.1, 30.0))), float(np.float32(rng.uniform(0, 1)))) for k in idx]
    finals = {int(perm[n - 1 - k]): float(np.float32(rng.uniform(0, 3))) for k in range(n_final)}
    return lattice(n, arcs, int(perm[0]), finals, {s: float(np.float32(rng.uniform(0, 1))) for s in finals})


def fan(width, seed):
    """initial -> `width` middle states -> one final state: fan-out and fan-in of `width`"""
    rng = np.random.RandomState(seed)
    n = width + 2
    arcs = [(0, 1 + k, float(np.float32(rng.uniform(0.5, 20))), float(np.float32(rng.uniform(0, 1)))) for k in range(width)]
    arcs += [(1 + k, n - 1, float(np.float32(rng.uniform(0.5, 20))), float(np.float32(rng.uniform(0, 1)))) for k in rng.permutation(width)]
    return lattice(n, arcs, 0, {n - 1: 0.5}, {n - 1: 0.25})


def small_cases():
    """the named small cases of the fixture; every one carries risks"""
    inf = math.inf
    c = {}
    c["one_arc"] = lattice(2, [(0, 1, 1.5, 0.5)], 0, {1: 0.0})
    c["chain"] = lattice(5, [(i, i + 1, 0.75 * (i + 1), 0.1 * i) for i in range(4)], 0, {4: 0.25}, {4: 0.5})
    c["diamond"] = lattice(4, [(0, 1, 1.0, 0.0), (0, 2, 1.25, 1.0), (1, 3, 2.0, 0.5), (2, 3, 1.5, 0.25)], 0, {3: 0.0})
    # a tie in the minimum at the first and the last of four arcs, different terms between them
    # (the two weights between them were searched for: with them the two orders of the sum round differently)
    c["tie_min"] = lattice(6, [(0, 1, 1.0, 0.1), (0, 2, 1.6578320264816284, 0.2), (0, 3, 2.0435683727264404, 0.3), (0, 4, 1.0, 0.4), (1, 5, 2.0, 0.0), (2, 5, 2.0, 0.5), (3, 5, 2.0, 0.7),
                               (4, 5, 2.0, 0.9)], 0, {5: 0.0})
    # the LAST arc of state 1 has a score equal to the state's final weight, two more arcs stand in front of it (weights searched for likewise)
    c["final_tie"] = lattice(5, [(0, 1, 0.5, 0.2), (1, 2, 2.1612658500671387, 0.3), (1, 3, 2.446044683456421, 0.6), (1, 4, 2.0, 0.1), (2, 4, 1.25, 0.5),
                                 (3, 4, 1.125, 0.2)], 0, {1: 2.0, 4: 0.0}, {1: 0.75})
    # state 4 has four incoming arcs of different magnitude; their sources 0, 1, 2, 3 are discovered in the order 0, 3, 2, 1 (three weights
    # searched for: the two orders of the forward sum round differently)
    c["discover_vs_id"] = lattice(6, [(0, 1, 0.3, 0.1), (0, 2, 2.5, 0.2), (0, 3, 7.0, 0.3), (0, 4, 9.5, 0.9), (1, 4, 1.5429561138153076, 0.4), (2, 4, 0.6955212950706482, 0.5),
                                      (3, 4, 0.06375738978385925, 0.6),
                                      (4, 5, 1.0, 0.7)], 0, {5: 0.125}, {5: 0.5})
    c["multi_final"] = lattice(5, [(0, 1, 1.0, 0.3), (0, 2, 2.0, 0.1), (1, 3, 0.5, 0.2), (2, 4, 0.25, 0.8), (1, 4, 3.0, 0.4)], 0, {3: 0.5, 4: 1.5, 2: 4.0},
                               {3: 0.1, 4: 0.2, 2: 0.3})
    # a final state with outgoing arcs whose final weight is the minimum (state 1) and one whose final weight is not (state 2)
    c["final_with_arcs"] = lattice(5, [(0, 1, 1.0, 0.3), (0, 2, 1.5, 0.6), (1, 3, 4.0, 0.2), (2, 3, 0.5, 0.1), (3, 4, 0.5, 0.9)], 0, {1: 0.25, 2: 6.0, 4: 0.0},
                                   {1: 0.5, 2: 0.75, 4: 0.25})
    c["inf_weights"] = lattice(5, [(0, 1, 1.0, 0.3), (0, 2, inf, 0.6), (0, 3, -inf, 0.1), (1, 4, 2.0, 0.2), (2, 4, 0.5, 0.1), (3, 4, 0.5, 0.9)], 0, {4: 0.0})
    c["dead_end"] = lattice(5, [(0, 1, 1.0, 0.3), (0, 2, 0.5, 0.6), (2, 3, 0.25, 0.2), (1, 4, 2.0, 0.2)], 0, {4: 0.0})
    c["unreachable"] = lattice(5, [(0, 1, 1.0, 0.3), (2, 1, 0.5, 0.6), (2, 3, 0.25, 0.2), (1, 4, 2.0, 0.2), (3, 4, 1.0, 0.1)], 0, {4: 0.5, 3: 0.1}, {4: 0.3})
    c["no_final"] = lattice(4, [(0, 1, 1.0, 0.3), (1, 2, 0.5, 0.6), (3, 2, 0.5, 0.1)], 0, {3: 0.0})
    c["initial_final"] = lattice(3, [(0, 1, 1.0, 0.3), (1, 2, 0.5, 0.6)], 0, {0: 3.0, 2: 0.0}, {0: 0.9, 2: 0.1})
    c["single_state"] = lattice(1, [], 0, {0: 0.5}, {0: 0.25})
    c["random_12"] = random_dag(12, 30, 3)
    c["random_40"] = random_dag(40, 130, 5, n_final=3)
    return c


def shape_cases():
    """the larger shapes of the device tests, placed around amx_latpost_kernel_shape()'s numbers (threads 256, LDS 4096 states, a wave
    from 128 arcs): fans of 1, 2, 63, 64, 65, 127, 128, 129 and 300 (a level wider than the workgroup), and fans whose state count is one
    below and one above the LDS switch (4096 nodes with the forward walk's new initial state: 4095 states fit, 4096 do not)"""
    c = {"fan_%d" % k: fan(k, 100 + k) for k in (1, 2, 63, 64, 65, 127, 128, 129, 300)}
    c["lds_below"] = fan(4093, 7)    # 4095 states
    c["lds_above"] = fan(4095, 8)    # 4097 states
    c["random_600"] = random_dag(600, 2400, 11, n_final=4)
    return c


CASE_OF_DEFECT = {"first-minimal": "tie_min", "strict-minimum": "final_tie", "final-dropped": "final_with_arcs", "incoming-by-id": "discover_vs_id",
                  "no-cap": "dead_end", "expm-no-isinf": "inf_weights", "contract-swapped": "random_40"}
MODE_OF_DEFECT = {"no-cap": LOG, "expm-no-isinf": PROB, "contract-swapped": EXPECTATION}
