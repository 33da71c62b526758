"""tests/linseg_reference.py -- plain-Python restatement of Speech::LinearSegmenter (Speech/AlignmentWithLinearSegmentation.cc:30-350): the
two-Gaussian silence / speech / silence delimiter over one energy value per frame and the linear spread of a flat state sequence over the
speech part.  The checker of amx_linseg_align_dev (include/amx.h, section "Linear-segmentation alignment"); tests/golden/ref_linseg.npz holds
what the reference's own text computes for cases() in both of its builds, and tests/test_linseg.py holds this file to it bit for bit.

f64 arithmetic is Python's float (IEEE double, one rounding per operation), f32 arithmetic numpy.float32.  contract="fma" follows the
reference's -march=native build.  Of its fused multiply-adds one can change a bit (tests/golden/make_linseg_golden.py finds it):
logLikelihood's xsil + xspe, where the product s2 * log(.) is fused into the sum.  feed's xx * xx + f / 2 is fused there too, but xx is a
widened f32 whose square is exact in f64, so both forms round the same sum once.  A fused multiply-add is math.fma where Python has it, else the exact rational a * b + c rounded once (fractions.Fraction).

Every comparison of the searches is also judged: the delimitation is DECIDED when no comparison between two different candidates comes
closer than 2^-48 of the larger |s * log(.)| term: then an implementation whose double logarithm is within one ulp
of the exact value takes the same decisions."""
import math
from fractions import Fraction

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
INT_MAX = 2**31 - 1
F32 = np.float32
OK, TOO_SHORT, TOO_LONG, NO_STATES, JUMP, MISMATCH, NONFINITE, N_REASONS = range(8)
REASONS = ("ok", "too_short", "too_long", "no_states", "jump", "mismatch", "nonfinite")
DEFAULTS = dict(number_of_iterations=3, penalty=100.0, minimum_speech_proportion=0.7, should_use_sietill=0, minimum_segment_length=1,
                maximum_segment_length=INT_MAX)
MARGIN = 2.0 ** -48        # of S, between two candidates: decided
SCORE_MARGIN = 2.0 ** -47  # of S: how far a device score may be from the restatement's
SILENCE_LABEL, SILENCE_EMISSION = 9000, 0


def fma(a, b, c):
    """a * b + c rounded once"""
    if hasattr(math, "fma"):
        try:
            return math.fma(a, b, c)
        except (OverflowError, ValueError):
            return a * b + c
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c
    try:
        return r.numerator / r.denominator   # int / int is correctly rounded
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def div(a, b):
    """IEEE a / b"""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def log_ieee(x):
    if x != x:
        return x
    if x == 0.0:
        return -math.inf
    if x < 0.0:
        return math.nan
    return math.log(x)


# the site of the -march=native build that matters: which product of xsil + xspe is fused into the sum ("xsil", "xspe" or None)
FMA_SITES = dict(sum="xspe")


def sites_of(contract, sites=None):
    if contract not in ("off", "fma"):
        raise ValueError("contract is %r, neither 'off' nor 'fma'" % (contract,))
    return dict(sum=None) if contract == "off" else dict(sites or FMA_SITES)


def chains(energy, penalty):
    """Delimiter::feed (:61-71) over the segment: M_, Q_ [N + 1]; the same bits in both builds (x * x is exact)"""
    f = float(penalty)
    M, Q = [0.0], [0.0]
    half = f / 2.0
    for v in np.asarray(energy, np.float32):
        x = float(v)
        M.append(M[-1] + x)
        if f > 0:
            Q.append(Q[-1] + div(x * x + half, f))
        else:
            Q.append(Q[-1] + x * x)
    return np.array(M, np.float64), np.array(Q, np.float64)


class Delimiter:
    """logLikelihood (:103-120) and the two getDelimitation (:145-182, :200-245) over finished chains"""

    def __init__(self, M, Q, penalty, proportion, iterations, contract="off", log=log_ieee, sites=None):
        self.M, self.Q = [float(v) for v in M], [float(v) for v in Q]
        self.N = len(self.M) - 1
        self.f = float(penalty)
        self.prop = F32(proportion)
        self.iterations = int(iterations)
        self.fused = sites_of(contract, sites)["sum"]
        self.log = log
        self.gate = self.prop * F32(np.uint32(self.N))   # f32 product
        self.decided = True
        self.evaluations = 0

    def likelihood(self, ib, ie):
        """-> (yy, S): S the larger |s * log(.)| term"""
        M, Q, N = self.M, self.Q, self.N
        self.evaluations += 1
        u = lambda v: v & 0xffffffff
        d = self.f if self.f > 0 else 1.0
        s1 = float(u(ib - 1 + N - ie))
        m1 = M[ib - 1] + M[N] - M[ie]
        qq = Q[ib - 1] + Q[N] - Q[ie]
        a1 = div(m1, s1)
        xx = div(qq, s1) - div(a1 * a1, d)
        l1 = self.log(0.5 if xx < 0.5 else xx)   # std::max(xx, e): (xx < e) ? e : xx
        xsil = s1 * l1
        s2 = float(u(ie - ib + 1))
        m2 = M[ie] - M[ib - 1]
        qq = Q[ie] - Q[ib - 1]
        a2 = div(m2, s2)
        xx = div(qq, s2) - div(a2 * a2, d)
        l2 = self.log(0.5 if xx < 0.5 else xx)
        xspe = s2 * l2
        S = max(abs(xsil), abs(xspe)) if xsil == xsil and xspe == xspe else math.inf
        if a1 < a2 and F32(np.uint32(u(ie - ib))) >= self.gate:
            if self.fused == "xspe":
                return fma(s2, l2, xsil), S
            if self.fused == "xsil":
                return fma(s1, l1, xspe), S
            return xsil + xspe, S
        return DBL_MAX, S

    def _less(self, x, S, cand, best):
        """x < best's value, and whether that comparison is safe from a one-ulp logarithm"""
        bx, bS, bc = best
        if cand != bc and not (x == DBL_MAX or bx == DBL_MAX):
            if not abs(x - bx) > MARGIN * max(S, bS):
                self.decided = False
        return x < bx

    def delimitation(self):
        """Delimiter::getDelimitation -> (begin, end, x_min)"""
        N = self.N
        if self.prop == F32(1.0):
            return 0, N - 1, DBL_MAX
        if N == 1:
            return 0, 0, DBL_MAX
        best = (DBL_MAX, 0.0, None)
        i_end, i_beg = N - 1, 1
        for _ in range(self.iterations):
            for ib in range(2, i_end - 1):
                x, S = self.likelihood(ib, i_end)
                if self._less(x, S, (ib, i_end), best):
                    best, i_beg = (x, S, (ib, i_end)), ib
            for ie in range(i_beg + 1, N - 1):
                x, S = self.likelihood(i_beg, ie)
                if self._less(x, S, (i_beg, ie), best):
                    best, i_end = (x, S, (i_beg, ie)), ie
        return i_beg - 1, i_end - 1, best[0]

    def sietill(self):
        """SietillDelimiter::getDelimitation -> (begin, end, x_min)"""
        N = self.N
        if self.prop == F32(1.0):
            return 0, N - 1, DBL_MAX
        best = (DBL_MAX, 0.0, None)
        i_end, i_beg = N, 1
        for _ in range(self.iterations):
            best = (DBL_MAX, 0.0, None)
            for ib in range(2, N):
                if ib != i_end:
                    c = (min(i_end, ib), max(ib, i_end))
                    x, S = self.likelihood(*c)
                    if self._less(x, S, c, best):
                        best, i_beg = (x, S, c), ib
            for ie in range(2, N):
                if ie != i_beg:
                    c = (min(i_beg, ie), max(ie, i_beg))
                    x, S = self.likelihood(*c)
                    if self._less(x, S, c, best):
                        best, i_end = (x, S, c), ie
            if i_end < i_beg:
                i_beg, i_end = i_end, i_beg
        return i_beg - 1, i_end - 1, best[0]


def spread(N, begin, end, labels, emissions, silence=(SILENCE_LABEL, SILENCE_EMISSION)):
    """LinearSegmenter::getAlignment's loops (:325-347) -> (reason, label [N], emission [N]); -1 everywhere unless OK"""
    n = len(labels)
    lab, emi = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    lab[:begin], emi[:begin] = silence
    slope = F32(n - 1) / F32(np.uint32(max(end - begin, 1)))
    previous = 0
    for t in range(begin, end + 1):
        v = float(slope * F32(np.uint32(t - begin)))
        index = int(math.floor(v + 0.5))   # round() of a value >= 0
        if index - previous > 2:
            return JUMP, np.full(N, -1, np.int32), np.full(N, -1, np.int32)
        lab[t], emi[t] = labels[index], emissions[index]
        previous = index
    if previous != n - 1:
        return MISMATCH, np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    lab[end + 1:], emi[end + 1:] = silence
    return OK, lab, emi


def segment(energy, labels, emissions, silence=(SILENCE_LABEL, SILENCE_EMISSION), contract="off", log=log_ieee, table=False, sites=None, **cfg):
    """one segment as AlignmentWithLinearSegmentationNode::work treats it.  Returns a dict: reason, begin, end (-1 when not computed), score,
    label, emission [N], M, Q [N + 1] (None when not computed), decided, and with table=True table [N + 1, N + 1] of logLikelihood(ib, ie) for
    1 <= ib <= ie <= N (0 elsewhere)."""
    c = dict(DEFAULTS)
    for k in cfg:
        if k not in c:
            raise TypeError("linseg_reference.segment: unknown parameter %r" % k)
    c.update(cfg)
    energy = np.asarray(energy, np.float32)
    N = len(energy)
    r = dict(reason=OK, begin=-1, end=-1, score=DBL_MAX, label=np.full(N, -1, np.int32), emission=np.full(N, -1, np.int32), M=None, Q=None,
             decided=True, table=None)
    if len(labels) == 0 or N == 0:
        r["reason"] = NO_STATES
    elif N < c["minimum_segment_length"]:
        r["reason"] = TOO_SHORT
    elif N > c["maximum_segment_length"]:
        r["reason"] = TOO_LONG
    if r["reason"] != OK:
        return r
    M, Q = chains(energy, c["penalty"])
    r["M"], r["Q"] = M, Q
    if not (np.all(np.isfinite(energy)) and np.all(np.isfinite(M)) and np.all(np.isfinite(Q))):
        r["reason"] = NONFINITE
        return r
    d = Delimiter(M, Q, c["penalty"], c["minimum_speech_proportion"], c["number_of_iterations"], contract, log, sites)
    r["begin"], r["end"], r["score"] = d.sietill() if c["should_use_sietill"] else d.delimitation()
    r["decided"] = d.decided
    r["reason"], r["label"], r["emission"] = spread(N, r["begin"], r["end"], labels, emissions, silence)
    if table:
        t = np.zeros((N + 1, N + 1), np.float64)
        for ib in range(1, N + 1):
            for ie in range(ib, N + 1):
                t[ib, ie] = d.likelihood(ib, ie)[0]
        r["table"] = t
    return r


def score_of(energy, begin, end, contract="off", log=log_ieee, **cfg):
    """logLikelihood of a given 0-based delimitation and its S: what the tie cases are judged with"""
    c = dict(DEFAULTS)
    c.update(cfg)
    M, Q = chains(energy, c["penalty"])
    return Delimiter(M, Q, c["penalty"], c["minimum_speech_proportion"], c["number_of_iterations"], contract, log).likelihood(begin + 1, end + 1)


# ------------------------------------------------------------------ the cases of the fixture

def track(n, seed, lead=0.15, trail=0.12, silence=(2.0, 0.5), speech=(8.0, 1.5)):
    """silence / speech / silence energies, f32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    a, b = int(round(lead * n)), n - int(round(trail * n))
    x = rng.normal(silence[0], silence[1], n)
    x[a:b] = rng.normal(speech[0], speech[1], max(b - a, 0))
    return x.astype(np.float32)


def states(n, first=100):
    """n allophone-state ids in path order and their emission indices"""
    return np.arange(first, first + 3 * n, 3, dtype=np.int32), (np.arange(n, dtype=np.int32) * 7 + 1) % 50


_CASES = None


def cases():
    """name -> dict(energy, labels, emissions, cfg): the cases of tests/golden/ref_linseg.npz, the same for everyone who asks"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}

    def add(name, energy, n_states, **cfg):
        lab, emi = states(n_states)
        out[name] = dict(energy=np.asarray(energy, np.float32), labels=lab, emissions=emi, cfg=cfg)

    for tag, s in (("d", 0), ("s", 1)):
        for n in (1, 2, 3, 4, 5, 63, 64, 65, 129, 4097):
            add("%s_n%d" % (tag, n), track(n, 10 + n) if n > 5 else track(8, 20 + n)[1:1 + n], 3, should_use_sietill=s)
        for pen, word in ((0.0, "0"), (1e-3, "1em3")):
            add("%s_penalty_%s" % (tag, word), track(65, 31), 3, should_use_sietill=s, penalty=pen)
        for prop, word in ((0.0, "0"), (0.3, "03"), (1.0, "1")):
            add("%s_proportion_%s" % (tag, word), track(64, 32, lead=0.3, trail=0.3), 3, should_use_sietill=s, minimum_speech_proportion=prop)
        # loud edges, a quiet middle: every window of 0.7 N frames is quieter than what is left, no candidate passes the gate
        add("%s_gate_none" % tag, track(64, 33, lead=0.1, trail=0.1, silence=(9.0, 0.5), speech=(2.0, 0.5)), 3, should_use_sietill=s)
        for it in (0, 1):
            add("%s_iterations_%d" % (tag, it), track(129, 34), 3, should_use_sietill=s, number_of_iterations=it)
        add("tie_digital_silence_%s" % tag, np.zeros(40, np.float32), 3, should_use_sietill=s)
        # two exact levels so close that every variance is floored at 0.5 (penalty 0): all candidates that pass the gate are N log 0.5 up to rounding
        two = np.full(40, 1.0, np.float32)
        two[8:34] = 1.5
        add("tie_constant_%s" % tag, two, 3, should_use_sietill=s, penalty=0.0)
    e = track(63, 35)
    r = segment(e, *states(3))
    speech = r["end"] - r["begin"] + 1
    for n, word in ((1, "1"), (2, "2"), (speech, "speech"), (2 * speech + 2, "jump")):
        add("d_states_%s" % word, e, n)
    add("d_mismatch_n1", track(8, 36)[:1], 2)
    add("d_quiet_speech", track(65, 37, silence=(8.0, 1.5), speech=(2.0, 0.5)), 3)
    for n, word in ((9, "below"), (10, "at")):
        add("d_minimum_%s" % word, track(n, 38), 3, minimum_segment_length=10)
    for n, word in ((10, "at"), (11, "above")):
        add("d_maximum_%s" % word, track(n, 39), 3, maximum_segment_length=10)
    _CASES = out
    return out


def is_tie(name):
    return name.startswith("tie_")
