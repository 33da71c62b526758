"""tests/cart_reference.py -- plain Python / numpy restatement of decision-tree state tying, in both of the reference's arithmetics:
  * accumulate(): Speech::FeatureAccumulator::processAlignedFeature (Speech/DecisionTreeTrainer.cc:58-90)
  * train():      Cart::Training (Cart/DecisionTreeTrainer.cc:353-801) with Core::PriorityQueue's heap (Core/PriorityQueue.hh:55-108) and
                  StateTyingDecisionTreeTrainer::LogLikelihoodGain (Speech/DecisionTreeTrainer.cc:134-250) as the scorer
tests/golden/make_cart_golden.py holds it to the reference's own text in every bit, where that is mounted; tests/test_cart.py holds it to
the fixture that generator wrote; tests/test_cart_gpu.py holds the library to it.

The logarithm is math.log: this machine's libm.  Everything else is IEEE f64 arithmetic written operation by operation; contract="fma"
fuses the sites FMA_SITES names, which the generator finds in the -march=native build.
"""
import ctypes
import math

import numpy as np

from tests.linseg_reference import div, fma as _fma_slow

SPLIT, PARTITION, CLUSTER = 0, 1, 2
ACTIONS = {"split": SPLIT, "partition": PARTITION, "cluster": CLUSTER}
LOG_2PI = math.log(3.141592653589793238462643383279502884197169399375105820975E+0000 + 3.141592653589793238462643383279502884197169399375105820975E+0000)
EPS = 2.0 ** -52
# sites of the reference's text that a contracting build may fuse; the generator asserts that this is what -march=native does
FMA_SITES = dict(sum=True, sum_sq=True, variance=True, constant=True)

try:
    _libm = ctypes.CDLL("libm.so.6")
    _libm.fma.restype = ctypes.c_double
    _libm.fma.argtypes = [ctypes.c_double] * 3
    fma = _libm.fma
except OSError:   # no libm to call: exact rational arithmetic
    fma = _fma_slow
_vfma = np.frompyfunc(fma, 3, 1)


def vfma(a, b, c):
    return _vfma(a, b, c).astype(np.float64)


def clog(x):
    """::log for every double"""
    if x != x:
        return math.nan
    if x == 0.0:
        return -math.inf
    if x < 0.0:
        return math.nan
    if x == math.inf:
        return math.inf
    return math.log(x)


def u32_add(c, w):
    """u32 += f64: the sum is formed in f64 and truncated"""
    return int(float(c) + float(w)) & 0xffffffff


# ------------------------------------------------------------------------------------------------------------------ accumulation

def accumulator(n_labels, dim):
    return np.zeros((n_labels, 1 + 2 * dim), np.float64)


def accumulate(acc, feats, labels, weights=None, contract="off", sites=None):
    """adds the frames in order into acc [n_labels x (1 + 2 dim)] = rows [nObs, sum, sumSq]; returns acc"""
    sites = FMA_SITES if sites is None else sites
    feats = np.ascontiguousarray(feats, np.float32)
    dim = feats.shape[1]
    fuse = contract == "fma"
    for t in range(len(labels)):
        i = int(labels[t])
        if i == -1:
            continue
        if not 0 <= i < len(acc):
            raise ValueError("frame %d: label %d" % (t, i))
        w = 1.0 if weights is None else float(weights[t])
        if w == 0.0:
            continue
        x = feats[t]
        xd, sq = x.astype(np.float64), (x * x).astype(np.float64)   # the square is an f32 product
        acc[i, 0] += w
        acc[i, 1:1 + dim] = vfma(xd, w, acc[i, 1:1 + dim]) if fuse and sites["sum"] else acc[i, 1:1 + dim] + xd * w
        acc[i, 1 + dim:] = vfma(sq, w, acc[i, 1 + dim:]) if fuse and sites["sum_sq"] else acc[i, 1 + dim:] + sq * w
    return acc


# ------------------------------------------------------------------------------------------------------------------ the scorer

def chain_sum(rows):
    """plain f64 chains down the rows, from +0.0"""
    if len(rows) == 0:
        return np.zeros(rows.shape[1])
    return np.add.accumulate(np.vstack([np.zeros((1, rows.shape[1])), rows]), axis=0)[-1]


def likelihood_of_sums(s, n_examples, dim, clip, contract, sites=None, detail=None):
    """LogLikelihoodGain::logLikelihood from a side's sums s = [count, sum[dim], sumSq[dim]]"""
    sites = FMA_SITES if sites is None else sites
    if n_examples == 0:
        return 0.0
    fuse = contract == "fma"
    n = float(s[0])
    ll, abs_log = 0.0, 0.0
    for d in range(dim):
        mu = div(float(s[1 + d]), n)
        var = div(float(s[1 + dim + d]), n)
        var = fma(-mu, mu, var) if fuse and sites["variance"] else var - mu * mu
        if var < clip:
            var = clip
        lg = clog(var)
        ll += lg
        abs_log += abs(lg)
    D = float(dim)
    const = fma(D, LOG_2PI, D) if fuse and sites["constant"] else D + D * LOG_2PI
    value = (0.5 * n) * (const + ll)
    if detail is not None:
        detail["abs_log"], detail["n"] = abs_log, n
    return value


def score_bar(n, dim, abs_log, value, ulps=2.0):
    """how far two evaluations of a side may lie apart when each logarithm is within one ulp of the exact value (glibc documents 1 ulp for
    log; two libms are then within `ulps` = 2 of each other): per component the logs differ by ulps * eps * |log|, the two ll chains
    round alike except where their inputs differ, by at most one ulp of the running sum per step (<= eps * abs_log each, dim steps), the
    constant is added once more (dim (1 + log 2 pi) bounds it), and the closing product and the sum in front of it round once each."""
    if not (math.isfinite(abs_log) and math.isfinite(value)):
        return math.inf
    D = float(dim)
    return 0.5 * abs(n) * (ulps + D + 4.0) * EPS * (abs_log + D * (1.0 + LOG_2PI)) + 4.0 * EPS * abs(value)


def almost_zero(gain):
    """Core::isAlmostEqualUlp(f32(gain), f32(0.0), 20) (Core/Utility.cc:61-73)"""
    i = int(np.array(gain, np.float64).astype(np.float32).view(np.int32))
    if i < 0:
        i = ((0x80000000 - (i & 0xffffffff)) & 0xffffffff)
        i = i - (1 << 32) if i >= (1 << 31) else i
    return abs(i) <= 20


# ------------------------------------------------------------------------------------------------------------------ the tree

class _Node:
    __slots__ = ("depth", "score", "n_obs", "ex", "question", "order", "left", "right", "bar")

    def __init__(self, depth, score, n_obs, ex, bar=0.0):
        self.depth, self.score, self.n_obs, self.ex, self.bar = depth, score, n_obs, ex, bar
        self.question, self.order, self.left, self.right = -1, None, None, None


class _Split:
    __slots__ = ("node", "qids", "qidid", "gain")

    def __init__(self, node, qids, qidid, gain):
        self.node, self.qids, self.qidid, self.gain = node, qids, qidid, gain


class _Queue:
    """Core::PriorityQueue<Split*, SplitPtrGreaterThan>, move by move"""

    def __init__(self, note):
        self.heap, self.note = [None], note

    def precedes(self, a, b):
        self.note(a.gain, b.gain)
        return a.gain > b.gain

    def size(self):
        return len(self.heap) - 1

    def insert(self, e):
        self.heap.append(e)
        i = self.size()
        while i > 1 and not self.precedes(self.heap[i // 2], e):
            self.heap[i] = self.heap[i // 2]
            i //= 2
        self.heap[i] = e

    def pop(self):
        top = self.heap[1]
        self.heap[1] = self.heap[self.size()]
        self.heap.pop()
        if self.size() > 0:
            i, e = 1, self.heap[1]
            while i <= self.size() // 2:
                j = 2 * i
                if j < self.size() and self.precedes(self.heap[j + 1], self.heap[j]):
                    j += 1
                if not self.precedes(self.heap[j], e):
                    break
                self.heap[i] = self.heap[j]
                i = j
            self.heap[i] = e
        return top


DEFECTS = ("unstable_partition", "no_swap_with_back", "obs_not_truncated", "no_strict", "last_of_equal_gains", "heap_is_sorted_list",
           "leaf_limit_off_by_one", "left_first_classes", "variance_unclipped")


def train(n_obs, values, answers, steps, max_leaves=0xffffffff, variance_clipping=0.0, contract="off", sites=None, defect=None):
    """n_obs [E], values [E x 2 dim] (sum, sumSq), answers bool [Q x E], steps: dicts (action, questions, min_obs, min_gain).
    defect: one of DEFECTS, a planted deviation from the reference (tests show that each one leaves the case it is planted in).
    Returns a dict: nodes (list of dicts in `order`), classes, log, question_stats, n_obs, initial_score, total_gain, errors,
    decided_gap (the smallest |a - b| / bar over all comparisons of two gains or a gain and a threshold that did not compare equal
    operands, inf if none), score_bar per node."""
    assert defect is None or defect in DEFECTS, defect
    n_obs = np.ascontiguousarray(n_obs, np.float64)
    values = np.ascontiguousarray(values, np.float64)
    answers = np.asarray(answers, bool)
    E, dim = len(n_obs), values.shape[1] // 2
    rows = np.hstack([n_obs[:, None], values])
    clip = -math.inf if defect == "variance_unclipped" else variance_clipping
    integral = bool(np.all(n_obs == np.floor(n_obs)))
    st = dict(gap=math.inf, errors=0)

    def side(ex):
        d = {}
        s = chain_sum(rows[ex]) if len(ex) else np.zeros(rows.shape[1])
        v = likelihood_of_sums(s, len(ex), dim, clip, contract, sites, d)
        return v, (score_bar(d["n"], dim, d["abs_log"], v) if len(ex) else 0.0)

    def obs_chain(ex):
        if defect == "obs_not_truncated":
            return int(round(float(n_obs[ex].sum()))) if len(ex) else 0
        if integral:
            return int(n_obs[ex].sum()) if len(ex) else 0
        c = 0
        for w in n_obs[ex]:
            c = u32_add(c, w)
        return c

    cur = dict(bar=0.0)

    def note(a, b):
        """a comparison of two gains (or a gain and a threshold)"""
        if a == b or not (math.isfinite(a) and math.isfinite(b)):
            return
        bar = cur["bar"] if cur["bar"] > 0 else EPS * max(abs(a), abs(b))
        st["gap"] = min(st["gap"], abs(a - b) / bar)

    question_of, qstats, log = [], [], []
    nodes_, splits_ = [], _Queue(note)
    counters = dict(number=0, leaf=0, gain=0.0)

    def split_node(node, qids, step):
        min_obs, min_gain = step.get("min_obs", 0), step.get("min_gain", 0.0)
        if node.n_obs < ((2 * min_obs) & 0xffffffff):
            return None
        ex = np.asarray(node.ex, np.int64)
        best = None
        for qidid, qid in enumerate(qids):
            a = answers[question_of[qid][1], ex]
            left, right = ex[a], ex[~a]
            l_obs, r_obs = obs_chain(left), obs_chain(right)
            if l_obs < min_obs or r_obs < min_obs:
                continue
            if defect != "no_strict" and (l_obs == 0 or r_obs == 0):
                continue
            (l, lb), (r, rb) = side(left), side(right)
            gain = node.score - (l + r)
            cur["bar"] = lb + rb + node.bar + 4 * EPS * (abs(l) + abs(r) + abs(node.score))
            note(gain, 0.0)
            if gain < 0.0:
                if not almost_zero(gain):
                    st["errors"] += 1
                continue
            note(gain, min_gain)
            if gain < min_gain:
                continue
            if defect != "no_strict" and gain == 0.0:
                continue
            if best is not None:
                note(gain, best[1])
                if (gain < best[1]) if defect == "last_of_equal_gains" else (gain <= best[1]):
                    continue
            best = (qidid, gain, l, r, l_obs, r_obs, left, right, lb, rb)
        if best is None:
            return None
        qidid, gain, l, r, l_obs, r_obs, left, right, lb, rb = best
        if defect == "unstable_partition":
            left, right = left[::-1], right[::-1]
        node.left = _Node(node.depth + 1, l, l_obs, [int(e) for e in left], lb)
        node.right = _Node(node.depth + 1, r, r_obs, [int(e) for e in right], rb)
        node.ex = None
        return _Split(node, qids, qidid, gain)

    def suggest(node, qids, step):
        sp = split_node(node, qids, step)
        if sp is not None:
            if defect == "heap_is_sorted_list":
                splits_.heap.append(sp)
                splits_.heap[1:] = sorted(splits_.heap[1:], key=lambda s: -s.gain)
            else:
                splits_.insert(sp)
        else:
            nodes_.append(node)

    def insert_split(sp):
        counters["gain"] += sp.gain
        node = sp.node
        node.question = sp.qids[sp.qidid]
        node.left.order = counters["number"]
        node.right.order = counters["number"] + 1
        counters["number"] += 2
        stp, row = question_of[node.question]
        log.append(dict(node=node.order, step=stp, row=row, depth=node.depth, gain=sp.gain, total_gain=counters["gain"]))
        q = qstats[node.question]
        q["count"] += 1
        q["sum_gain"] += sp.gain
        q["min_gain"], q["max_gain"] = min(q["min_gain"], sp.gain), max(q["max_gain"], sp.gain)
        q["sum_depth"] += node.depth
        q["min_depth"], q["max_depth"] = min(q["min_depth"], node.depth), max(q["max_depth"], node.depth)

    def take_question(sp):
        if defect == "no_swap_with_back":
            del sp.qids[sp.qidid]
        else:
            sp.qids[sp.qidid] = sp.qids[-1]
            sp.qids.pop()

    def pop_split():
        if defect == "heap_is_sorted_list":
            return splits_.heap.pop(1)
        return splits_.pop()

    def run_step(i, step):
        action = ACTIONS.get(step["action"], step["action"])
        base = len(question_of)
        ids = []
        for k, row in enumerate(step["questions"]):
            question_of.append((i, int(row)))
            qstats.append(dict(step=i, row=int(row), count=0, min_gain=1.7976931348623157e+308, sum_gain=0.0, max_gain=-1.7976931348623157e+308,
                               min_depth=0xffffffff, sum_depth=0, max_depth=0))
            ids.append(base + k)
        for _ in range(len(nodes_)):
            suggest(nodes_.pop(0), list(ids), step)
        limit = max_leaves + 1 if defect == "leaf_limit_off_by_one" else max_leaves
        while splits_.size() > 0 and counters["leaf"] + len(nodes_) + splits_.size() < limit:
            sp = pop_split()
            insert_split(sp)
            take_question(sp)
            node = sp.node
            if action == SPLIT:
                suggest(node.left, list(sp.qids), step)
                suggest(node.right, sp.qids, step)
            else:
                suggest(node.right, sp.qids, step)
                if action == CLUSTER:
                    counters["leaf"] += 1
                else:
                    nodes_.append(node.left)
        while splits_.size() > 0:
            sp = pop_split()
            node = sp.node
            node.ex = node.left.ex + node.right.ex
            node.left = node.right = None
            nodes_.append(node)

    # init
    total_obs = 0
    for w in n_obs:
        total_obs = u32_add(total_obs, w)
    score, bar = side(np.arange(E))
    root = _Node(0, score, total_obs, list(range(E)), bar)
    root.order = 0
    counters["number"] = 1
    nodes_.append(root)
    for i, step in enumerate(steps):
        if not counters["leaf"] + len(nodes_) < max_leaves:
            break
        run_step(i, step)
    counters["leaf"] += len(nodes_)
    # finish
    out_nodes = [None] * counters["number"]
    classes = np.full(E, -1, np.int32)
    n_cluster = [0]

    def commit(node):
        o = dict(step=-1, row=-1, left=-1, right=-1, depth=node.depth, n_obs=node.n_obs, score=node.score, class_id=-1, bar=node.bar)
        out_nodes[node.order] = o
        if node.left is not None:
            o["step"], o["row"] = question_of[node.question]
            o["left"], o["right"] = node.left.order, node.right.order
            # setChilds(commitNode(left), commitNode(right)): the order of the two calls is the compiler's; the reference's (GCC) build
            # evaluates the arguments from the right, which the generator finds in the class ids
            if defect == "left_first_classes":
                commit(node.left)
                commit(node.right)
            else:
                commit(node.right)
                commit(node.left)
        else:
            o["class_id"] = n_cluster[0]
            n_cluster[0] += 1
            classes[node.ex] = o["class_id"]

    commit(root)
    assert n_cluster[0] == counters["leaf"], (n_cluster[0], counters["leaf"])
    return dict(nodes=out_nodes, classes=classes, log=log, question_stats=qstats, n_obs=total_obs, initial_score=score, total_gain=counters["gain"],
                errors=st["errors"], decided_gap=st["gap"], n_leaves=counters["leaf"])


# ------------------------------------------------------------------------------------------------------------------ cases

def make_examples(rng, E, dim, frames=(1, 40), weights=False, spread=1.0):
    """E examples as an accumulation would leave them: per example a centre, some frames around it; weights: fractional nObs"""
    n_obs, values = np.zeros(E), np.zeros((E, 2 * dim))
    acc = accumulator(E, dim)
    for e in range(E):
        n = int(rng.integers(frames[0], frames[1] + 1))
        x = (rng.standard_normal(dim) * 2.0 + rng.standard_normal((n, dim)) * spread).astype(np.float32)
        w = rng.uniform(0.05, 1.5, n) if weights else None
        accumulate(acc, x, np.full(n, e), w)
    n_obs[:], values[:] = acc[:, 0], acc[:, 1:]
    return n_obs, values


def _case(seed, E, Q, dim, steps, max_leaves=0xffffffff, clip=0.0, weights=False, frames=(1, 40), all_left=False, duplicate=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_obs, values = make_examples(rng, E, dim, frames, weights)
    answers = rng.random((Q, E)) < rng.uniform(0.2, 0.8, (Q, 1))
    if all_left:
        answers[Q // 2] = True
    half = E // 2
    if duplicate == "copy":   # examples in pairs with equal statistics and questions in pairs with equal answers: equal gains within a node
        n_obs[half:2 * half], values[half:2 * half] = n_obs[:half], values[:half]
        answers[:, half:2 * half] = answers[:, :half]
        answers[1::2] = answers[0:2 * (Q // 2):2][:len(answers[1::2])]
    elif duplicate == "negate":   # the second half mirrors the first (sum -> -sum: every later sum is the exact negative, every gain equal),
        n_obs[half:2 * half] = n_obs[:half]   # and question 0 tells the halves apart: twin nodes wait in the queue with equal gains
        values[:half, dim:] += 6.0 * values[:half, :dim] + 9.0 * n_obs[:half, None]   # every frame moved by 3: the first half lies off the origin
        values[:half, :dim] += 3.0 * n_obs[:half, None]
        values[half:2 * half, :dim], values[half:2 * half, dim:] = -values[:half, :dim], values[:half, dim:]
        answers[:, half:2 * half] = answers[:, :half]
        answers[0, :half], answers[0, half:] = True, False
    return dict(n_obs=n_obs, values=values, answers=answers, steps=steps, max_leaves=max_leaves, variance_clipping=clip)


def _all(Q):
    return list(range(Q))


def kernel_shape(dim):
    """(examples per LDS stage, questions per workgroup) of the library's split search as it was written: 32 KiB of rows of 1 + 2 dim doubles,
    64 at most; 256 lanes over the rows' components.  The GPU test hands cases() the library's own amx_cart_kernel_shape instead."""
    R = 1 + 2 * dim
    return max(1, min(64, 32768 // (8 * R))), max(1, 256 // R)


def cases(shape=kernel_shape):
    """name -> arguments of train().  shape(dim): the split search's LDS stage and question tile; the sizes around them are part of the
    cases."""
    (stage, tile), (stage32, tile32), (stage1, tile1) = shape(40), shape(32), shape(1)
    c = {}
    c["e1"] = _case(1, 1, 3, 4, [dict(action="split", questions=_all(3))])
    c["e33_q1_d1"] = _case(2, 33, 1, 1, [dict(action="split", questions=[0])])
    c["stage_plus_1"] = _case(3, stage + 1, tile + 1, 40, [dict(action="split", questions=_all(tile + 1))])
    c["tile_plus_1_d32"] = _case(4, stage32 + 1, tile32 + 1, 32, [dict(action="split", questions=_all(tile32 + 1))])
    c["d1_tile_plus_1"] = _case(5, stage1 + 26, tile1 + 1, 1, [dict(action="split", questions=_all(tile1 + 1))], frames=(2, 30))
    c["big"] = _case(6, 700, 70, 40, [dict(action="split", questions=_all(70), min_obs=200, min_gain=50.0)], max_leaves=60)
    c["three_actions"] = _case(7, 120, 24, 23, [dict(action="partition", questions=_all(8), min_obs=20),
                                                dict(action="cluster", questions=list(range(8, 16)), min_obs=30),
                                                dict(action="split", questions=list(range(4, 24)), min_obs=10)], max_leaves=40, weights=True,
                               frames=(1, 12))
    c["rollback"] = _case(8, 150, 20, 8, [dict(action="split", questions=_all(10), min_obs=15),
                                          dict(action="split", questions=list(range(10, 20)), min_obs=5)], max_leaves=9, weights=True, frames=(1, 12))
    c["max_leaves_mid_step"] = _case(9, 200, 16, 8, [dict(action="split", questions=_all(16), min_obs=5)], max_leaves=7)
    c["min_obs_excludes_best"] = _case(10, 80, 12, 6, [dict(action="split", questions=_all(12), min_obs=700)])
    c["min_gain_excludes_best"] = _case(11, 80, 12, 6, [dict(action="split", questions=_all(12), min_gain=200.0)])
    c["all_left"] = _case(12, 20, 6, 5, [dict(action="split", questions=_all(6))], all_left=True, clip=1e-3)
    c["weights"] = _case(13, 70, 10, 7, [dict(action="split", questions=_all(10), min_obs=8)], weights=True, frames=(1, 12))
    c["clipping"] = _case(14, 90, 10, 6, [dict(action="split", questions=_all(10), min_obs=6)], clip=1.5)
    c["tie_duplicates"] = _case(15, 64, 12, 4, [dict(action="split", questions=_all(12), min_obs=4)], duplicate="copy")
    c["tie_twins"] = _case(16, 64, 10, 4, [dict(action="split", questions=_all(10), min_obs=4)], duplicate="negate", max_leaves=21)
    return c


def is_tie(name):
    return name.startswith("tie_")


# a planted defect and the case it must leave
PLANTED = {
    "unstable_partition": "rollback", "no_swap_with_back": "tie_duplicates", "obs_not_truncated": "weights", "no_strict": "all_left",
    "last_of_equal_gains": "tie_duplicates", "heap_is_sorted_list": "tie_twins", "leaf_limit_off_by_one": "max_leaves_mid_step",
    "left_first_classes": "three_actions", "variance_unclipped": "clipping",
}


def discrete(r):
    """everything of a result that is not a floating-point value"""
    return dict(nodes=[(n["step"], n["row"], n["left"], n["right"], n["depth"], n["n_obs"], n["class_id"]) for n in r["nodes"]],
                classes=[int(v) for v in r["classes"]], log=[(l["node"], l["step"], l["row"], l["depth"]) for l in r["log"]],
                stats=[(q["step"], q["row"], q["count"], q["min_depth"], q["sum_depth"], q["max_depth"]) for q in r["question_stats"]],
                n_obs=r["n_obs"], errors=r["errors"])


def floats(r):
    """every floating-point value of a result, flat"""
    return np.array([n["score"] for n in r["nodes"]] + [v for l in r["log"] for v in (l["gain"], l["total_gain"])] +
                    [v for q in r["question_stats"] for v in (q["min_gain"], q["sum_gain"], q["max_gain"])] + [r["initial_score"], r["total_gain"]], np.float64)
