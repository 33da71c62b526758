#!/usr/bin/env python3
"""Writes tests/golden/ref_latpost.npz: lattice arc posteriors as the reference's own text computes them, in both of its arithmetics.

What it compiles (the flag sets of oracle/ref/Makefile: -msse3 = contract "off", -msse3 -march=native = contract "fma"), taken by line
range + SHA-256 into a temporary directory that is deleted afterwards, behind stand-ins of this file's own for Automaton, State, Arc,
Weight, Semiring, StaticAutomaton, ModifyAutomaton, Stack, Vector and Ref.  This file holds none of the reference's program text:
  dfs_class     Fsa/tDfs.hh:42-166        Ftl::DfsState (colours, info_, the callbacks)
  dfs_walk      Fsa/tDfs.cc:20-68         DfsState::dfs, the stack walk
  transpose     Fsa/tRational.cc:594-689  TransposeDfsState and transpose()
  zero          Fsa/Sssp.cc:67            Zero
  posterior64   Fsa/Sssp.cc:69-225        StatePotentials64DfsState (finishState :95-138), sssp64, Posterior64Automaton, posterior64()
  posteriorE    Fsa/Sssp.cc:231-375       StatePotentialsEDfsState (finishState :254-288), ssspE, PosteriorEAutomaton, posteriorE()
  expm          Fsa/Arithmetic.cc:47-54   ApplyExp
  almost_equal, almost_equal_ulp, difference_ulp   Core/Utility.hh:316-321, :384-388, Core/Utility.cc:61-73
The stand-in Weight has the reference's two floating-point constructors (f32, double) and records which one a call took: that is how
the fixture knows whether exp(-f32) in ApplyExp and in PosteriorEAutomaton::modifyState resolved to the float or the double overload
(`overload/*`; the translation units include <cmath>, not <math.h>, and so does the generated source).

The driver builds the automaton in the input's arc order, constructs the Posterior64Automaton / PosteriorEAutomaton and calls modifyState on
a copy of every state that both walks reach.  Where the reference defines nothing (states a walk does not reach, a lattice without a
reached final state: its transpose() returns an empty automaton and the constructor would index a vector with InvalidStateId) the fixture
holds the library's documented choice, computed by tests/latpost_reference.py; `defined/<case>` marks the states the reference computed.
tests/latpost_reference.py must equal the compiled text in every bit on every case, small and large, or this script stops.

THE BARS.  The device library's f64 exp and log1p are in the 1 ulp class.  Every case (the small ones and the shapes of the device
tests, tests/latpost_reference.py:shape_cases) is recomputed by the restatement -- equal to the reference in every bit -- with every exp
and log1p result moved by one ulp, the sign drawn per call, for SEEDS seeds, in every variant and both builds.  Per output class the largest
|changed - unchanged| / max(1, |unchanged|) times 4 (the project's usual margin) is the measured part.  The f32 outputs add what their
number format can do to a value that moved at all: every f32 rounding on the way to the output may fall to the other neighbour, one f32
ulp (2^-23, relative) each --
  log          1 rounding (the cap):                                                    + 1 x 2^-23
  prob         the cap's ulp moves exp(-lp) by |lp| e^-lp 2^-23 <= 0.37 x 2^-23, plus the narrowing: + 2 x 2^-23
  expectation  the same for exp(-lp) (times the risk factor), the risk factor's cap, the narrowing: + 3 x 2^-23 x max(1, largest |risk factor|)
total_inv, expectation value and the potentials are f64 / narrowed once: the measured part (+ 2^-23 for the f32 expectation).
The bars come from the reference's arithmetic alone, never from the library.

    python3 tests/golden/make_latpost_golden.py [reference source tree] [--accept: take the text whatever its hash]
"""
import ctypes as C
import hashlib
import io
import math
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = next((a for a in sys.argv[1:] if not a.startswith("--")), "/root/reference/src")

from tests import latpost_reference as lr   # noqa: E402

PIECES = {
    "dfs_class": [("Fsa/tDfs.hh", 42, 166)],
    "dfs_walk": [("Fsa/tDfs.cc", 20, 68)],
    "transpose": [("Fsa/tRational.cc", 594, 689)],
    "zero": [("Fsa/Sssp.cc", 67, 67)],
    "posterior64": [("Fsa/Sssp.cc", 69, 225)],
    "posteriorE": [("Fsa/Sssp.cc", 231, 375)],
    "expm": [("Fsa/Arithmetic.cc", 47, 54)],
    "almost_equal": [("Core/Utility.hh", 316, 321)],
    "almost_equal_ulp": [("Core/Utility.hh", 384, 388)],
    "difference_ulp": [("Core/Utility.cc", 61, 73)],
}
TEXT_SHA256 = "969029ae5034e4f5e943907e346a139f80063caeae51e5124031df0a42812adb"
SEEDS = 6
F32_ULP = 2.0 ** -23
VARIANTS = {"log": (lr.LOG, 1, 1), "prob": (lr.PROB, 1, 1), "expectation": (lr.EXPECTATION, 1, 1), "log_n0": (lr.LOG, 0, 1), "prob_n0": (lr.PROB, 0, 1),
            "expectation_v0": (lr.EXPECTATION, 1, 0)}
MODE_ID = {lr.LOG: 0, lr.PROB: 1, lr.EXPECTATION: 2}

SOURCE = r'''
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
typedef float    f32;
typedef double   f64;
typedef int32_t  s32;
typedef uint32_t u32;
typedef int64_t  s64;
#define require(x)
#define require_(x)
#define verify(x)
static int lp_ctor_f32 = 0, lp_ctor_f64 = 0;
namespace Core {
template<class T> struct Type;
template<> struct Type<f32> { static constexpr f32 max = FLT_MAX, min = -FLT_MAX, epsilon = FLT_EPSILON, delta = FLT_MIN; };
template<> struct Type<f64> { static constexpr f64 max = DBL_MAX, min = -DBL_MAX, epsilon = DBL_EPSILON, delta = DBL_MIN; };
template<class T> struct Vector : public std::vector<T> {
    void grow(size_t id, const T& def = T()) { if (id >= this->size()) this->insert(this->end(), id - this->size() + 1, def); }
};
struct ProgressIndicator {
    ProgressIndicator(const char*, const char*) {}
    void start(size_t) {} void setTotal(size_t) {} void notify() {} void finish() {}
};
inline std::string form(const char* s, ...) { return s; }
inline f32 abs(f32 v) { return std::fabs(v); }
inline s32 abs(s32 v) { return v < 0 ? -v : v; }
s32 differenceUlp(f32 a, f32 b);
%(almost_equal)s
%(almost_equal_ulp)s
template<class T> struct Ref {
    T* p;
    Ref() : p(0) {}
    explicit Ref(T* q) : p(q) {}
    template<class U> Ref(const Ref<U>& o) : p(o.p) {}
    T* operator->() const { return p; }
    T& operator*() const { return *p; }
    T* get() const { return p; }
    operator bool() const { return p != 0; }
    template<class U> bool operator==(const Ref<U>& o) const { return p == o.p; }
    template<class U> bool operator!=(const Ref<U>& o) const { return p != o.p; }
};
}  // namespace Core
%(difference_ulp)s
namespace Fsa {
typedef u32 StateId;
typedef u32 StateTag;
typedef s32 LabelId;
typedef u32 Property;
typedef int Type;
static const StateTag StateTagFinal  = 0x80000000;
static const StateTag StateIdMask    = 0x3fffffff;
static const StateId  InvalidStateId = StateIdMask;
static const LabelId  Epsilon        = -1;
static const Type     TypeTransducer = 2;
static const Property PropertyAcyclic = 0x20;
class Weight {
    f32 f_;
public:
    Weight() : f_(0) {}
    explicit Weight(f32 v) : f_(v) { ++lp_ctor_f32; }
    explicit Weight(double v) : f_(v) { ++lp_ctor_f64; }
    operator float() const { return f_; }
};
struct Semiring {
    Weight one_;
    Weight one() const { return one_; }
};
typedef Core::Ref<const Semiring> ConstSemiringRef;
static Semiring        lp_log_semiring;
static ConstSemiringRef LogSemiring(&lp_log_semiring), TropicalSemiring;
struct Arc {
    StateId target_;
    Weight  weight_;
    LabelId input_;
    StateId target() const { return target_; }
    Weight  weight() const { return weight_; }
};
class State {
    StateId          id_;
    StateTag         tags_;
    std::vector<Arc> arcs_;
public:
    typedef std::vector<Arc>::iterator       iterator;
    typedef std::vector<Arc>::const_iterator const_iterator;
    Weight weight_;
    State(StateId id = 0) : id_(id), tags_(0) {}
    StateId  id() const { return id_; }
    StateTag tags() const { return tags_; }
    void     setTags(StateTag t) { tags_ = t; }
    bool     hasTags(StateTag t) const { return tags_ & t; }
    bool     isFinal() const { return tags_ & StateTagFinal; }
    iterator begin() { return arcs_.begin(); }
    iterator end() { return arcs_.end(); }
    const_iterator begin() const { return arcs_.begin(); }
    const_iterator end() const { return arcs_.end(); }
    size_t   nArcs() const { return arcs_.size(); }
    Arc*     newArc() { arcs_.push_back(Arc()); return &arcs_.back(); }
    Arc*     newArc(StateId t, Weight w, LabelId l) { Arc a; a.target_ = t, a.weight_ = w, a.input_ = l; arcs_.push_back(a); return &arcs_.back(); }
};
typedef Core::Ref<State>       StateRef;
typedef Core::Ref<const State> ConstStateRef;
class Automaton {
public:
    typedef Fsa::Arc                   Arc;
    typedef Fsa::State                 State;
    typedef Fsa::Weight                Weight;
    typedef Fsa::StateRef              StateRef;
    typedef Fsa::ConstStateRef         ConstStateRef;
    typedef Core::Ref<const Automaton> ConstRef;
    ConstSemiringRef semiring_;
    Automaton() : semiring_(LogSemiring) {}
    virtual ~Automaton() {}
    virtual ConstStateRef getState(StateId) const { return ConstStateRef(); }
    virtual StateId       initialStateId() const { return InvalidStateId; }
    virtual std::string   describe() const { return ""; }
    ConstSemiringRef semiring() const { return semiring_; }
    Type     type() const { return 1; }
    Property knownProperties() const { return 0; }
    Property properties() const { return 0; }
    int      getInputAlphabet() const { return 0; }
    int      getOutputAlphabet() const { return 0; }
};
typedef Automaton::ConstRef ConstAutomatonRef;
inline bool hasProperties(ConstAutomatonRef, Property) { return true; }
template<class T> struct Stack : public std::vector<T> {
    void push(const T& t) { this->push_back(t); }
    T    top() const { return this->back(); }
    void pop() { this->pop_back(); }
    bool isEmpty() const { return this->empty(); }
};
}  // namespace Fsa
namespace Ftl {
template<class _Automaton> class StaticAutomaton : public _Automaton {
    std::vector<Fsa::State*> states_;
    Fsa::StateId             initial_;
public:
    StaticAutomaton() : initial_(Fsa::InvalidStateId) {}
    void setType(Fsa::Type) {} void setProperties(Fsa::Property, Fsa::Property) {} void setInputAlphabet(int) {} void setOutputAlphabet(int) {}
    void setSemiring(Fsa::ConstSemiringRef s) { this->semiring_ = s; }
    Fsa::StateRef state(Fsa::StateId s) { return Fsa::StateRef(s < states_.size() ? states_[s] : 0); }
    void setState(Fsa::State* sp) { if (sp->id() >= states_.size()) states_.resize(sp->id() + 1, 0); states_[sp->id()] = sp; }
    Fsa::State* newState() { Fsa::State* sp = new Fsa::State(states_.size()); states_.push_back(sp); return sp; }
    void setInitialStateId(Fsa::StateId s) { initial_ = s; }
    void clear() { states_.clear(); }
    size_t size() const { return states_.size(); }
    virtual Fsa::ConstStateRef getState(Fsa::StateId s) const { return Fsa::ConstStateRef(s < states_.size() ? states_[s] : 0); }
    virtual Fsa::StateId       initialStateId() const { return initial_; }
};
%(dfs_class)s
%(dfs_walk)s
%(transpose)s
}  // namespace Ftl
namespace Fsa {
typedef Ftl::DfsState<Automaton>  DfsState;
typedef Core::Vector<f64>         StatePotentials64;
inline ConstAutomatonRef transpose(ConstAutomatonRef f) { return Ftl::transpose<Automaton>(f, false); }
class ModifyAutomaton : public Automaton {
public:
    ConstAutomatonRef fsa_;
    ModifyAutomaton(ConstAutomatonRef f) : fsa_(f) {}
    virtual void modifyState(State* sp) const = 0;
};
#define private public
#define protected public
%(zero)s
%(posterior64)s
%(posteriorE)s
#undef private
#undef protected
%(expm)s
}  // namespace Fsa

extern "C" {
// the transposed automaton's arc lists: for every state its arcs' targets (the sources of the input's arcs) in the reference's order, the new
// initial state last; returns the number of transposed states (0: the empty automaton)
int lp_transpose(int n, const long* off, const int* tgt, const float* w, int initial, const uint8_t* ff, const float* fw, long* t_off, int* t_tgt,
                 float* t_w) {
    Ftl::StaticAutomaton<Fsa::Automaton>* f = new Ftl::StaticAutomaton<Fsa::Automaton>;
    for (int s = 0; s < n; ++s) {
        Fsa::State* sp = new Fsa::State(s);
        if (ff[s]) sp->setTags(Fsa::StateTagFinal), sp->weight_ = Fsa::Weight(fw[s]);
        for (long a = off[s]; a < off[s + 1]; ++a) sp->newArc(tgt[a], Fsa::Weight(w[a]), 0);
        f->setState(sp);
    }
    f->setInitialStateId(initial);
    Fsa::ConstAutomatonRef t = Fsa::transpose(Fsa::ConstAutomatonRef(f));
    long k = 0;
    t_off[0] = 0;
    if (t->initialStateId() == Fsa::InvalidStateId) return 0;
    for (int s = 0; s <= n; ++s) {
        Fsa::ConstStateRef sp = t->getState(s);
        if (sp)
            for (Fsa::State::const_iterator a = sp->begin(); a != sp->end(); ++a, ++k) t_tgt[k] = a->target(), t_w[k] = f32(a->weight());
        t_off[s + 1] = k;
    }
    return (int)t->initialStateId() == n ? n + 1 : -1;
}
// pots: forward [n + 1], backward [n + 1], generalized forward, generalized backward (entries past a vector's size keep what the caller put);
// sizes [4]; scalars: totalInv(f64 overload), totalInv as Weight, expectation, forward flow, backward flow, flows agree, vanishing flow,
// the Weight constructor (1: f32, 2: double) taken by expm and by the expectation's arc product
int lp_run(int mode, int normalize, int v_normalized, int tol, int n, const long* off, const int* tgt, const float* w, const float* r, int initial,
           const uint8_t* ff, const float* fw, const float* fr, const uint8_t* defined, float* arc_out, float* final_out, double* pots, int* sizes,
           double* scalars) {
    std::cerr.setstate(std::ios_base::failbit);
    Ftl::StaticAutomaton<Fsa::Automaton>*f = new Ftl::StaticAutomaton<Fsa::Automaton>, *rf = new Ftl::StaticAutomaton<Fsa::Automaton>;
    for (int s = 0; s < n; ++s) {
        Fsa::State *sp = new Fsa::State(s), *rp = new Fsa::State(s);
        if (ff[s]) {
            sp->setTags(Fsa::StateTagFinal), sp->weight_ = Fsa::Weight(fw[s]);
            rp->setTags(Fsa::StateTagFinal), rp->weight_ = Fsa::Weight(fr[s]);
        }
        for (long a = off[s]; a < off[s + 1]; ++a) sp->newArc(tgt[a], Fsa::Weight(w[a]), 0), rp->newArc(tgt[a], Fsa::Weight(r[a]), 0);
        f->setState(sp), rf->setState(rp);
    }
    f->setInitialStateId(initial), rf->setInitialStateId(initial);
    Fsa::ConstAutomatonRef fa(f), ra(rf);
    Fsa::Posterior64Automaton* p;
    Fsa::PosteriorEAutomaton*  pe = 0;
    if (mode == 2) {
        p = pe = new Fsa::PosteriorEAutomaton(fa, ra, v_normalized != 0, tol);
        Fsa::Weight e = pe->expectation(), ti = pe->totalInv();
        scalars[0] = p->Posterior64Automaton::totalInv(), scalars[1] = f32(ti), scalars[2] = f32(e);
    }
    else {
        p = new Fsa::Posterior64Automaton(fa, normalize != 0, tol);
        const f64  t64 = p->totalInv();
        Fsa::Weight ti  = Fsa::Weight(t64 > Core::Type<f32>::min ? t64 : Core::Type<f32>::min);   // the Weight& overload's line
        scalars[0] = t64, scalars[1] = f32(ti), scalars[2] = 0;
    }
    const Core::Vector<f64>* v[4] = {&p->forwardPotentials_, &p->backwardPotentials_, pe ? &pe->generalizedForwardPotentials_ : 0,
                                     pe ? &pe->generalizedBackwardPotentials_ : 0};
    for (int k = 0; k < 4; ++k) {
        sizes[k] = v[k] ? (int)v[k]->size() : 0;
        for (int s = 0; s < sizes[k] && s <= n; ++s) pots[(size_t)k * (n + 1) + s] = (*v[k])[s];
    }
    if (sizes[0] <= n || sizes[1] <= initial) return -1;
    const f32 fwd = (f32)p->forwardPotentials_[n], bwd = (f32)p->backwardPotentials_[initial];
    scalars[3] = fwd, scalars[4] = bwd;
    scalars[5] = mode == 2 ? Core::isAlmostEqualUlp(fwd, bwd, tol) : Core::isAlmostEqual(fwd, bwd, tol);
    scalars[6] = Core::isAlmostEqualUlp(f32(scalars[1]), Core::Type<f32>::min, tol);
    scalars[7] = scalars[8] = 0;
    Fsa::ApplyExp apply;
    for (int s = 0; s < n; ++s) {
        if (!defined[s]) continue;
        if ((int)p->forwardPotentials_.size() <= s || (int)p->backwardPotentials_.size() <= s) return -2;
        Fsa::State copy(*f->getState(s));
        lp_ctor_f32 = lp_ctor_f64 = 0;
        p->modifyState(&copy);
        if (mode == 2 && copy.nArcs()) scalars[8] = lp_ctor_f64 ? 2 : 1;
        long a = off[s];
        for (Fsa::State::iterator it = copy.begin(); it != copy.end(); ++it, ++a) {
            if (mode == 1) {
                const bool through_exp = !std::isinf(f32(it->weight_));   // the other branch constructs from a literal
                lp_ctor_f32 = lp_ctor_f64 = 0;
                it->weight_ = apply(it->weight_);
                if (through_exp) scalars[7] = lp_ctor_f64 ? 2 : 1;
            }
            arc_out[a] = f32(it->weight_);
        }
        if (copy.isFinal()) final_out[s] = f32(mode == 1 ? apply(copy.weight_) : copy.weight_);
    }
    return 0;
}
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-D_GNU_SOURCE", "-DSPRINT_RELEASE_BUILD", "-w"]


def reference_text():
    cache, parts, h = {}, {}, hashlib.sha256()
    for key, ranges in PIECES.items():
        out = []
        for fn, first, last in ranges:
            if fn not in cache:
                with open(os.path.join(REF, fn), encoding="utf-8", errors="replace") as f:
                    cache[fn] = f.readlines()
            out.append("".join(cache[fn][first - 1:last]))
        parts[key] = "\n".join(out)
        h.update(parts[key].encode())
    return parts, h.hexdigest()


def build(tmp, flavour, parts):
    gen, so = os.path.join(tmp, "latpost_%s.cc" % flavour), os.path.join(tmp, "latpost_%s.so" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    subprocess.check_call(["g++"] + FLAGS + ([] if flavour == "off" else ["-march=native"]) + ["-shared", "-o", so, gen])
    os.remove(gen)
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    i64, i32, f32p, f64p, u8 = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.int64, np.int32, np.float32, np.float64, np.uint8))
    L.lp_transpose.argtypes = [C.c_int, i64, i32, f32p, C.c_int, u8, f32p, i64, i32, f32p]
    L.lp_run.argtypes = [C.c_int] * 5 + [i64, i32, f32p, f32p, C.c_int, u8, f32p, f32p, u8, f32p, f32p, f64p, i32, f64p]
    return L, int(fma or 0)


def arrays(lat):
    return (np.ascontiguousarray(lat["arc_offsets"], np.int64), np.ascontiguousarray(lat["arc_target"], np.int32), np.ascontiguousarray(lat["arc_weight"], np.float32),
            np.ascontiguousarray(lat["arc_risk"], np.float32), int(lat["initial"]), np.ascontiguousarray(lat["final_flag"], np.uint8),
            np.ascontiguousarray(lat["final_weight"], np.float32), np.ascontiguousarray(lat["final_risk"], np.float32))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def reference_transpose(L, lat):
    off, tgt, w, _, ini, ff, fw, _ = arrays(lat)
    n = len(off) - 1
    cap = len(tgt) + n + 1
    t_off, t_tgt, t_w = np.zeros(n + 2, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
    k = L.lp_transpose(n, off, tgt, w, ini, ff, fw, t_off, t_tgt, t_w)
    assert k in (0, n + 1), k
    return k, t_off, t_tgt, t_w


def run_reference(L, lat, variant, want):
    """the compiled text on one lattice; `want` (the restatement) supplies the library's choices where the reference defines nothing and is
    compared everywhere else"""
    mode, normalize, v_normalized = VARIANTS[variant]
    off, tgt, w, r, ini, ff, fw, fr = arrays(lat)
    n = len(off) - 1
    P = want["potentials"]
    defined = np.array([P["coreached"][s] for s in range(n)], np.uint8)
    arc, final = want["arc"].copy(), want["final"].copy()
    pots = np.stack([np.array(P[k] + [0.0] * (n + 1 - len(P[k]))) for k in ("forward", "backward", "generalized_forward", "generalized_backward")])
    if P["dead"]:
        return dict(arc=arc, final=final, pots=pots, scalars=None, defined=defined * 0)
    ref_arc, ref_final, ref_pots = np.full_like(arc, np.nan), np.full_like(final, np.nan), np.full_like(pots, np.nan)
    sizes, scalars = np.zeros(4, np.int32), np.zeros(9)
    rc = L.lp_run(MODE_ID[mode], normalize, v_normalized, 100, n, off, tgt, w, r, ini, ff, fw, fr, defined, ref_arc, ref_final, ref_pots, sizes, scalars)
    assert rc == 0, rc
    src = lr.source_of(lat)
    for a in range(len(tgt)):
        if defined[src[a]]:
            arc[a] = ref_arc[a]
    for s in range(n):
        if defined[s] and ff[s]:
            final[s] = ref_final[s]
        # a potential is the reference's where its walk finished the state
        if P["coreached"][s]:
            pots[0, s], pots[2, s] = ref_pots[0, s], ref_pots[2, s]
        if P["reached"][s]:
            pots[1, s], pots[3, s] = ref_pots[1, s], ref_pots[3, s]
    pots[0, n], pots[2, n] = ref_pots[0, n], ref_pots[2, n]
    if mode != lr.EXPECTATION:
        pots[2:] = 0
    return dict(arc=arc, final=final, pots=pots, scalars=scalars, defined=defined)


INFO_SCALARS = ("total_inv", "total_inv_f32", "expectation", "forward_flow", "backward_flow", "flows_agree", "vanishing_flow")


def compare(name, got, want):
    """the restatement against the compiled text, in every bit"""
    P = want["potentials"]
    n = len(want["final"])
    mine = np.stack([np.array(P[k] + [0.0] * (n + 1 - len(P[k]))) for k in ("forward", "backward", "generalized_forward", "generalized_backward")])
    assert np.array_equal(bits(got["arc"]), bits(want["arc"])), (name, "arc", got["arc"], want["arc"])
    assert np.array_equal(bits(got["final"]), bits(want["final"])), (name, "final", got["final"], want["final"])
    assert np.array_equal(bits(got["pots"]), bits(mine)), (name, "potentials", got["pots"], mine)
    if got["scalars"] is not None:
        s = np.array([want["info"][k] for k in INFO_SCALARS], np.float64)
        assert np.array_equal(bits(got["scalars"][:7]), bits(s)), (name, "info", got["scalars"], s)


def perturbed(seed):
    rng = np.random.RandomState(seed)

    def move(v):
        return float(np.nextafter(v, math.inf if rng.randint(2) else -math.inf)) if math.isfinite(v) else v
    return (lambda x: move(lr.host_exp(x))), (lambda x: move(lr.host_log1p(x)))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok])))) if ok.any() else 0.0


def main():
    parts, sha = reference_text()
    if "--accept" not in sys.argv:
        assert sha == TEXT_SHA256, "the reference's text changed: %s" % sha
    out = {}
    small, shapes = lr.small_cases(), lr.shape_cases()
    measured = {k: 0.0 for k in ("log", "prob", "expectation", "total_inv", "expectation_value", "potentials", "generalized")}
    risk_factor = 1.0
    with tempfile.TemporaryDirectory() as tmp:
        libs = {fl: build(tmp, fl, parts) for fl in ("off", "fma")}
    assert libs["off"][1] == 0 and libs["fma"][1] > 0, "the two builds are not the two arithmetics: %r" % ({k: v[1] for k, v in libs.items()},)
    overloads = set()
    for group, cases in (("case", small), ("shape", shapes)):
        for name, lat in cases.items():
            assert not lr.has_cycle(lat)
            if group == "case":
                for k, v in zip(("arc_offsets", "arc_target", "arc_weight", "arc_risk", "initial", "final_flag", "final_weight", "final_risk"), arrays(lat)):
                    out["case/%s/%s" % (name, k)] = np.asarray(v)
            # the transposed order, from the compiled text, against the restatement's
            k, t_off, t_tgt, t_w = reference_transpose(libs["off"][0], lat)
            order, incoming, finals = lr.transpose(lat)
            n, src = lr.n_states(lat), lr.source_of(lat)
            if k:
                for v in range(n):
                    assert [int(x) for x in t_tgt[t_off[v]:t_off[v + 1]]] == [int(src[a]) for a in incoming[v]] or not t_off[v + 1] - t_off[v], (name, v)
                assert [int(x) for x in t_tgt[t_off[n]:t_off[n + 1]]] == finals, name
            else:
                assert not finals, name
            for variant, (mode, normalize, v_normalized) in VARIANTS.items():
                if group == "shape" and variant not in ("log", "prob", "expectation"):
                    continue
                for fl in ("off", "fma"):
                    want = lr.posterior(lat, mode, bool(normalize), bool(v_normalized), 100, fl)
                    got = run_reference(libs[fl][0], lat, variant, want)
                    tag = "%s/%s/%s/%s" % (group, name, variant, fl)
                    compare(tag, got, want)
                    if got["scalars"] is not None:
                        overloads.add((int(got["scalars"][7]), int(got["scalars"][8]), variant.split("_")[0]))
                    if group == "case":
                        out[tag + "/arc"], out[tag + "/final"], out[tag + "/potentials"] = got["arc"], got["final"], got["pots"]
                        out[tag + "/info"] = np.array([want["info"][k] for k in lr_info_keys()], np.float64)
                        out["defined/%s" % name] = got["defined"]
                    else:
                        h = hashlib.sha256(got["arc"].tobytes() + got["final"].tobytes() + got["pots"].tobytes()).digest()
                        out[tag + "/sha256"] = np.frombuffer(h, np.uint8)
                    if mode == lr.EXPECTATION and not want["potentials"]["dead"]:
                        P = want["potentials"]
                        ini = int(lat["initial"])
                        norm = P["generalized_backward"][ini] if v_normalized else 0.0
                        for a in range(len(src)):
                            v = P["generalized_forward"][int(src[a])] + float(lat["arc_risk"][a]) + P["generalized_backward"][int(lat["arc_target"][a])] - norm
                            if math.isfinite(v) and abs(v) < 1e30:
                                risk_factor = max(risk_factor, abs(v))
                    for seed in range(SEEDS):
                        moved = lr.posterior(lat, mode, bool(normalize), bool(v_normalized), 100, fl, fn=perturbed(1000 * seed + 17))
                        cls = variant.split("_")[0]
                        measured[cls] = max(measured[cls], rel(moved["arc"], want["arc"]), rel(moved["final"], want["final"]))
                        measured["total_inv"] = max(measured["total_inv"], rel(moved["info"]["total_inv"], want["info"]["total_inv"]))
                        measured["expectation_value"] = max(measured["expectation_value"], rel(moved["info"]["expectation"], want["info"]["expectation"]))
                        for k in ("forward", "backward"):
                            measured["potentials"] = max(measured["potentials"], rel(moved["potentials"][k], want["potentials"][k]))
                            measured["generalized"] = max(measured["generalized"], rel(moved["potentials"]["generalized_" + k], want["potentials"]["generalized_" + k]))
                if group == "case" and variant == "expectation":
                    a, b = (out["case/%s/expectation/%s/arc" % (name, fl)] for fl in ("off", "fma"))
                    pa, pb = (out["case/%s/expectation/%s/potentials" % (name, fl)] for fl in ("off", "fma"))
                    out["builds_differ/%s" % name] = np.array([int(not np.array_equal(bits(a), bits(b))), int(not np.array_equal(bits(pa), bits(pb)))], np.int32)
    # the overloads: 2 = Weight(double), 1 = Weight(f32)
    expm_ctor = {o[0] for o in overloads if o[2] == "prob" and o[0]}
    prod_ctor = {o[1] for o in overloads if o[2] == "expectation" and o[1]}
    assert expm_ctor == {2} and prod_ctor == {2}, (expm_ctor, prod_ctor)   # what latpost.hip and the restatement compute; a change here is a change there
    out["overload/expm_double"], out["overload/expectation_product_double"] = np.array([1], np.int32), np.array([1], np.int32)
    # every planted defect is visible in its case
    for defect, name in lr.CASE_OF_DEFECT.items():
        mode = lr.MODE_OF_DEFECT.get(defect, lr.LOG)
        fl = "fma"
        good, bad = lr.posterior(small[name], mode, contract=fl), lr.posterior(small[name], mode, contract=fl, defect=defect)
        assert not lr.same_bits(good, bad), "defect %s does not show on %s" % (defect, name)
    assert any(out["builds_differ/%s" % n][1] for n in small), "no case on which the two builds differ"
    format_part = {"log": F32_ULP, "prob": 2 * F32_ULP, "expectation": 3 * F32_ULP * risk_factor, "total_inv": 0.0, "expectation_value": F32_ULP,
                   "potentials": 0.0, "generalized": 0.0}
    for k, v in measured.items():
        out["measured/" + k] = np.array([v])
        out["bar/" + k] = np.array([4 * v + format_part[k]])
    out["risk_factor"] = np.array([risk_factor])
    out["seeds"] = np.array([SEEDS], np.int32)
    path = os.path.join(ROOT, "tests", "golden", "ref_latpost.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:   # np.savez_compressed's layout with a fixed time stamp: the same bytes every run
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print("wrote %s: %d arrays, %d bytes; fma instructions %r; text %s" % (path, len(out), os.path.getsize(path), {k: v[1] for k, v in libs.items()}, sha))
    print("measured:", {k: "%.3g" % v for k, v in measured.items()}, "risk factor %.3g" % risk_factor)
    print("bars:", {k[4:]: "%.3g" % float(out[k][0]) for k in sorted(out) if k.startswith("bar/")})
    print("builds differ on:", [n for n in small if out["builds_differ/%s" % n][1]])


def lr_info_keys():
    return INFO_SCALARS + ("reason", "states_reached", "arcs_reached", "states_coreached", "undefined_states", "undefined_arcs", "levels_forward", "levels_backward")


if __name__ == "__main__":
    main()
