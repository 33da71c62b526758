#!/usr/bin/env python3
"""tests/golden/make_align_golden.py -- writes tests/golden/ref_align.npz: Viterbi alignments as Search::Aligner computes them (what
Speech::AlignmentNode runs), from the reference's own text.

Run it where the reference tree is mounted; tests read only the fixture.  What it compiles, in both of the reference's arithmetics (the
flag sets of oracle/ref/Makefile: -msse3 = contract=off, -msse3 -march=native = contract=fma), taken by line range + SHA-256 into a
temporary directory that is deleted afterwards:
  * Search/Aligner.cc:41-106 (class Aligner::SearchSpace), 108-167 (constructor, setViterbi, setModel, clear,
    activateOrUpdateStateHypothesisViterbi), 198-324 (addStartupHypothesis, expand, minimumScore, prune, deleteStateHypothesisViterbi),
    341-445 (collectGarbage, finalStatePotential, getAlignmentFsaViterbi), 463-469 (getAlignmentFsa) and 587-634 (Aligner::restart, feed,
    feed(vector), alignmentScore)
  * Search/Aligner.hh:173-175 (reachedFinalState), Core/Utility.hh:316-321 (isAlmostEqual), Mm/ScaledFeatureScorer.hh:47-76
    (ScaledContextScorer, used when score_scale != 1)
behind a shell of this file's own that holds no reference text: stand-ins for Fsa::StaticAutomaton / State / Arc / Weight / Semiring,
Core::Component / Configuration / Ref / Statistics, Am::AcousticModel (label -> emission index), the frame of class Search::Aligner, and a
row scorer that returns column e of the frame's row out of line.  The Baum-Welch members (activateOrUpdateStateHypothesisBaumWelch,
deleteStateHypothesisBaumWelch, getAlignmentFsaBaumWelch, Semiring::collect) are stubs that abort.  Virtual calls are kept out of line
(-fno-devirtualize): in the reference the scorers live in other translation units, so neither build fuses a scorer's product into
expand()'s additions.

The cases are tests/align_reference.py's cases().  Findings (printed by every run, kept in the fixture):
  * fma_differs: which recorded arrays the -march=native build computes differently (expected: none; the search only adds and compares).
  * ties: for the cases with exact ties, a dense Viterbi in which the lowest state id wins every tie reaches the SAME score (the cases
    really tie) and, in at least one of them, other labels than the reference (so the cases tell list order from id order).
  * empty segments: whatever the reference's text gives for zero frames is recorded (cases empty, empty_final).

    python3 tests/golden/make_align_golden.py [out.npz]
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import align_reference as ar  # noqa: E402

REF = "/root/reference/src"

PIECES = {
    "ss_class": [("Search/Aligner.cc", 41, 106)],
    "ss_first": [("Search/Aligner.cc", 108, 167)],
    "ss_search": [("Search/Aligner.cc", 198, 324)],
    "ss_result": [("Search/Aligner.cc", 341, 445)],
    "ss_fsa": [("Search/Aligner.cc", 463, 469)],
    "aligner": [("Search/Aligner.cc", 587, 634)],
    "reached": [("Search/Aligner.hh", 173, 175)],
    "almost_equal": [("Core/Utility.hh", 316, 321)],
    "scaled_hh": [("Mm/ScaledFeatureScorer.hh", 47, 76)],
}
SHA = "185c9ee4567a76959538ab5fe00335ba78e9a942246209b6d97bc4bcb3df4eec"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/Types.hh>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <string>
#include <unordered_map>
#include <vector>
// ---- shell: stand-ins (no reference text) ----
namespace Core {
struct Configuration {};
struct NullLog {
    template<class T> NullLog& operator<<(const T&) { return *this; }
};
class Component {
public:
    Configuration config;
    Component(const Configuration&) {}
    virtual ~Component() {}
    NullLog       log() const { return NullLog(); }
    NullLog       log(const char*) const { return NullLog(); }
    Configuration select(const char*) const { return Configuration(); }
};
template<class T> class Ref {   // never deletes: a generator run is short
    T* p_;
public:
    Ref() : p_(0) {}
    explicit Ref(T* p) : p_(p) {}
    template<class U> Ref(const Ref<U>& o) : p_(o.get()) {}
    T*       operator->() const { return p_; }
    T&       operator*() const { return *p_; }
    T*       get() const { return p_; }
    explicit operator bool() const { return p_ != 0; }
    bool     operator!() const { return p_ == 0; }
};
template<class T> Ref<T> ref(T* p) { return Ref<T>(p); }
template<class V> class Statistics {   // Core::Statistics<V> as far as the aligner uses it; keeps the samples as well
public:
    u32            nObs_;
    V              sum_;
    std::vector<V> samples;
    Statistics(const std::string&) : nObs_(0), sum_(V()) {}
    void clear() { nObs_ = 0, sum_ = V(), samples.clear(); }
    void operator+=(V v) { ++nObs_, sum_ += v, samples.push_back(v); }
    f64  average() const { return f64(sum_) / f64(nObs_); }
};
template<class T> inline T abs(T v) { return v < 0 ? -v : v; }
}  // namespace Core
namespace Fsa {
typedef u32 StateId;
typedef s32 LabelId;
static const StateId InvalidStateId = 0x3fffffff;
static const LabelId Epsilon        = -1;
struct Weight {
    f32 v;
    Weight() : v(0) {}
    explicit Weight(f32 x) : v(x) {}
    operator f32() const { return v; }
};
struct Semiring {
    Weight one() const { return Weight(0); }
    Weight collect(Weight, Weight) const { abort(); }   // baum-welch only
};
typedef const Semiring* ConstSemiringRef;
static const Semiring   theTropical, theLog;
static ConstSemiringRef TropicalSemiring = &theTropical, LogSemiring = &theLog;
typedef int ConstAlphabetRef;
enum Type { TypeAcceptor };
typedef u32 Property;
static const Property PropertyStorage = 1, PropertyAcyclic = 2, PropertyLinear = 4, PropertySausages = 8;
struct Arc {
    StateId target_;
    Weight  weight_;
    LabelId input_, output_;
    StateId target() const { return target_; }
    LabelId input() const { return input_; }
    Weight  weight() const { return weight_; }
};
class State {
public:
    StateId          id_;
    bool             final_;
    Weight           weight_;
    std::vector<Arc> arcs_;
    typedef std::vector<Arc>::const_iterator const_iterator;
    State(StateId id) : id_(id), final_(false) {}
    StateId        id() const { return id_; }
    void           setId(StateId id) { id_ = id; }
    bool           isFinal() const { return final_; }
    void           setFinal(Weight w) { final_ = true, weight_ = w; }
    const_iterator begin() const { return arcs_.begin(); }
    const_iterator end() const { return arcs_.end(); }
    Arc*           newArc(StateId target, Weight w, LabelId input) {
        Arc a;
        a.target_ = target, a.weight_ = w, a.input_ = a.output_ = input;
        arcs_.push_back(a);
        return &arcs_.back();
    }
};
class Automaton {
public:
    virtual ~Automaton() {}
};
class StaticAutomaton : public Automaton {
public:
    std::vector<State*> states_;
    StateId             initial_;
    ConstSemiringRef    semiring_;
    StaticAutomaton() : initial_(InvalidStateId), semiring_(TropicalSemiring) {}
    size_t           size() const { return states_.size(); }
    State*           fastState(StateId s) const { return states_[s]; }
    StateId          initialStateId() const { return initial_; }
    void             setInitialStateId(StateId s) { initial_ = s; }
    void             clear() { states_.clear(); }
    void             setType(Type) {}
    void             setSemiring(ConstSemiringRef s) { semiring_ = s; }
    ConstSemiringRef semiring() const { return semiring_; }
    void             setInputAlphabet(ConstAlphabetRef) {}
    ConstAlphabetRef getInputAlphabet() const { return 0; }
    void             addProperties(Property) {}
    bool             hasProperty(Property) const { return true; }
    void             setState(State* s) {
        if (s->id() >= states_.size())
            states_.resize(s->id() + 1, 0);
        states_[s->id()] = s;
    }
    State* newState() {
        State* s = new State(states_.size());
        states_.push_back(s);
        return s;
    }
    State* newFinalState(Weight w) {
        State* s = newState();
        s->setFinal(w);
        return s;
    }
    void    deleteState(StateId) { abort(); }   // baum-welch only
    StateId maxStateId() const { return states_.size() - 1; }
    void    normalize() { abort(); }            // baum-welch only
};
typedef Core::Ref<const Automaton> ConstAutomatonRef;
static Core::Ref<StaticAutomaton>  staticCopy(ConstAutomatonRef m) {
    return Core::Ref<StaticAutomaton>(const_cast<StaticAutomaton*>(static_cast<const StaticAutomaton*>(m.get())));
}
}  // namespace Fsa
namespace Mm {
typedef f32 Score;
typedef u32 EmissionIndex;
typedef u32 MixtureIndex;
class FeatureScorer {
public:
    class ContextScorer {
    public:
        virtual ~ContextScorer() {}
        virtual EmissionIndex nEmissions() const = 0;
        virtual Score         score(EmissionIndex e) const = 0;
    };
    typedef Core::Ref<const ContextScorer> Scorer;
};
typedef FeatureScorer::ContextScorer ContextScorer;
typedef FeatureScorer::Scorer        Scorer;
class MatrixRowScorer : public ContextScorer {
    const f32* row_;
    u32        n_;
public:
    MatrixRowScorer(const f32* row, u32 n) : row_(row), n_(n) {}
    virtual EmissionIndex nEmissions() const { return n_; }
    virtual Score         score(EmissionIndex e) const;
};
__attribute__((noinline)) Score MatrixRowScorer::score(EmissionIndex e) const { return row_[e]; }
class ScaledFeatureScorer {};
class FeatureScorerScaling : public ScaledFeatureScorer {
public:
// ---- reference text: ScaledContextScorer ----
%(scaled_hh)s
};
}  // namespace Mm
namespace Am {
typedef s32 AllophoneStateIndex;
class AcousticModel {
public:
    std::unordered_map<s32, u32> emission_;
    Mm::MixtureIndex emissionIndex(AllophoneStateIndex a) const { return emission_.find(a)->second; }
};
}  // namespace Am
namespace Speech {
typedef f32 Score;
typedef u32 TimeframeIndex;
}  // namespace Speech
namespace Core {
// ---- reference text: isAlmostEqual ----
%(almost_equal)s
}  // namespace Core
namespace Search {
typedef Speech::TimeframeIndex TimeframeIndex;
typedef Speech::Score          Score;
struct LogVariability {
    bool operator()(const Core::Configuration&) const { return false; }
};
static const LogVariability paramLogVariability;
// the frame of Search::Aligner: the members its pieces below use (Aligner.hh:99-123)
class Aligner : public Core::Component {
    typedef Speech::Score Score;
public:
    Fsa::ConstAutomatonRef model_;
    class SearchSpace;
    SearchSpace*                       ss_;
    Core::Ref<const Am::AcousticModel> acousticModel_;
    Score                              acousticPruningThreshold_;
    u32                                nBestPruning_;
    Score                              minAcousticPruningThreshold_;
    Score                              maxAcousticPruningThreshold_;
    Score                              acousticPruningThresholdIncrementFactor_;
    f64                                minAverageNumberOfStateHypotheses_;
    bool                               increasePruningUntilNoScoreDifference_;
    bool                               logIterations_;
    u32                                nIterations_;
    bool                               viterbi_;
    u32                                collectGarbageTime_;
    Core::Statistics<u32>              nStateHypotheses_;
    Aligner(const Core::Configuration& c);
    void  restart();
    void  feed(Mm::FeatureScorer::Scorer scorer);
    void  feed(const std::vector<Mm::FeatureScorer::Scorer>&);
    Score alignmentScore() const;
// ---- reference text: reachedFinalState ----
%(reached)s
};
}  // namespace Search
using namespace Search;
// ---- reference text: class Aligner::SearchSpace ----
%(ss_class)s
// ---- reference text: constructor, setViterbi, setModel, clear, activateOrUpdateStateHypothesisViterbi ----
%(ss_first)s
// ---- shell: baum-welch members abort
void Aligner::SearchSpace::activateOrUpdateStateHypothesisBaumWelch(StateId, Score, StateHypothesisIndex, Am::AllophoneStateIndex, Fsa::Weight) { abort(); }
void Aligner::SearchSpace::deleteStateHypothesisBaumWelch(StateHypothesisIndex) { abort(); }
Fsa::ConstAutomatonRef Aligner::SearchSpace::getAlignmentFsaBaumWelch() const { abort(); }
// ---- reference text: addStartupHypothesis, expand, minimumScore, prune, deleteStateHypothesisViterbi ----
%(ss_search)s
// ---- reference text: collectGarbage, finalStatePotential, getAlignmentFsaViterbi ----
%(ss_result)s
// ---- reference text: getAlignmentFsa ----
%(ss_fsa)s
// ---- shell: the constructor with the members' values handed in by the driver
Aligner::Aligner(const Core::Configuration& c)
        : Core::Component(c), ss_(0), acousticPruningThreshold_(0), nBestPruning_(Core::Type<s32>::max), logIterations_(false), nIterations_(0),
          viterbi_(true), collectGarbageTime_(500), nStateHypotheses_("active states after pruning") {
    ss_ = new SearchSpace(select("search"));
    ss_->setViterbi(true);
}
// ---- reference text: Aligner::restart, feed, feed(vector), alignmentScore ----
%(aligner)s
// ---- this generator's own driver (no reference text) ----
class ScaledAccess : public Mm::FeatureScorerScaling::ScaledContextScorer {
public:
    ScaledAccess(Mm::Scorer s, Mm::Score scale) : Mm::FeatureScorerScaling::ScaledContextScorer(s, scale) {}
};
// One segment.  arcs of state i: [arc_off[i], arc_off[i + 1]); label_of / emission_of: the acoustic model's table.  Outputs: label,
// emission, arc_score [T] (-1, -1, 0 for an empty automaton), survivors [T], summary = score, last threshold; counts = reached,
// n_iterations, automaton states; avg = average, sum.
extern "C" int ref_align(int n_states, int initial, const unsigned char* is_final, const float* final_weight, const int* arc_off, const int* arc_target,
                         const int* arc_label, const float* arc_weight, int n_labels, const int* label_of, const int* emission_of, int T, int n_columns,
                         const float* scores, float lo, float hi, float factor, double min_avg, int incr, float scale, int* label, int* emission,
                         float* arc_score, int* survivors, float* summary, int* counts, double* avg) {
    Fsa::StaticAutomaton* m = new Fsa::StaticAutomaton;
    for (int i = 0; i < n_states; ++i) {
        Fsa::State* s = new Fsa::State(i);
        if (is_final[i])
            s->setFinal(Fsa::Weight(final_weight[i]));
        for (int a = arc_off[i]; a < arc_off[i + 1]; ++a)
            s->newArc(arc_target[a], Fsa::Weight(arc_weight[a]), arc_label[a]);
        m->setState(s);
    }
    m->setInitialStateId(initial);
    Am::AcousticModel* am = new Am::AcousticModel;
    for (int i = 0; i < n_labels; ++i)
        am->emission_[label_of[i]] = emission_of[i];
    Core::Configuration c;
    Aligner             al(c);
    al.minAcousticPruningThreshold_ = lo, al.maxAcousticPruningThreshold_ = hi, al.acousticPruningThresholdIncrementFactor_ = factor;
    al.minAverageNumberOfStateHypotheses_ = min_avg, al.increasePruningUntilNoScoreDifference_ = incr != 0;
    // Aligner::setModel (Aligner.cc:575-585)
    al.model_         = Fsa::ConstAutomatonRef(m);
    al.acousticModel_ = Core::Ref<const Am::AcousticModel>(am);
    al.ss_->setModel(al.model_);
    al.ss_->addStartupHypothesis();
    al.nStateHypotheses_.clear();
    al.acousticPruningThreshold_ = al.maxAcousticPruningThreshold_;
    std::vector<Mm::Scorer> scorers;
    for (int t = 0; t < T; ++t) {
        Mm::Scorer row(new Mm::MatrixRowScorer(scores + (size_t)t * n_columns, n_columns));
        scorers.push_back(scale == 1.f ? row : Mm::Scorer(new ScaledAccess(row, scale)));
    }
    al.feed(scorers);
    summary[0] = al.alignmentScore(), summary[1] = al.acousticPruningThreshold_;
    counts[0] = al.reachedFinalState(), counts[1] = al.nIterations_;
    avg[0] = al.nStateHypotheses_.average(), avg[1] = (double)al.nStateHypotheses_.sum_;
    for (int t = 0; t < T; ++t)
        survivors[t] = t < (int)al.nStateHypotheses_.samples.size() ? (int)al.nStateHypotheses_.samples[t] : -1, label[t] = emission[t] = -1, arc_score[t] = 0;
    Fsa::ConstAutomatonRef        f = al.ss_->getAlignmentFsa();
    const Fsa::StaticAutomaton*   r = static_cast<const Fsa::StaticAutomaton*>(f.get());
    counts[2]                       = (int)r->size();
    if (r->initialStateId() == Fsa::InvalidStateId)
        return 0;
    if ((int)r->size() != T + 1)
        return 1;
    for (int t = 0; t < T; ++t) {
        const Fsa::State* s = r->fastState(t);
        if (s->end() - s->begin() != 1 || s->begin()->target() != (Fsa::StateId)(t + 1))
            return 2;
        label[t] = s->begin()->input(), emission[t] = am->emissionIndex(label[t]), arc_score[t] = (f32)s->begin()->weight();
    }
    return r->fastState(T)->isFinal() ? 0 : 3;
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-fno-access-control", "-fno-devirtualize",
         "-fno-devirtualize-speculatively", "-D_GNU_SOURCE", "-DSPRINT_RELEASE_BUILD", "-I" + REF, "-I/usr/include/libxml2", "-w"]
TIE_CASES = ("tie_labels", "tie_rank_order", "tie_finals", "tie_random0", "tie_random1", "tie_random2")
FIELDS = ("label", "emission", "arc_score", "survivors", "score", "reached", "n_iterations", "last_threshold", "average_states", "state_sum",
          "automaton_states")


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
    gen = os.path.join(tmp, "align_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "align_%s.so" % flavour)
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    L.ref_align.restype = C.c_int
    return L, int(fma or 0)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def flat(g):
    """a graph of tests/align_reference.py as the arrays of amx_align_graphs (one segment) and the acoustic model's label -> emission table"""
    off, tgt, emi, lab, wgt, table = [0], [], [], [], [], {}
    for arcs in g["arcs"]:
        for t, e, l, w in arcs:
            tgt.append(t), emi.append(e), lab.append(l), wgt.append(w)
            assert table.setdefault(int(l), int(e)) == int(e), "label %d has two emission indices" % l
        off.append(len(tgt))
    return dict(n_states=np.array(g["n_states"], np.int32), initial=np.array(g["initial"], np.int32), is_final=g["final"].astype(np.uint8),
                final_weight=g["final_weight"].astype(np.float32), arc_offsets=np.array(off, np.int32), arc_target=np.array(tgt, np.int32),
                arc_emission=np.array(emi, np.int32), arc_label=np.array(lab, np.int32), arc_weight=np.array(wgt, np.float32),
                label_of=np.array(sorted(table), np.int32), emission_of=np.array([table[k] for k in sorted(table)], np.int32))


def run(L, cases):
    a = {}
    for name, c in cases.items():
        x, s = flat(c["graph"]), np.ascontiguousarray(c["scores"], np.float32)
        cfg = dict(ar.DEFAULTS)
        cfg.update(c["cfg"])
        T = len(s)
        label, emission, survivors = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32)
        arc = np.zeros(T, np.float32)
        summary, counts, avg = np.zeros(2, np.float32), np.zeros(3, np.int32), np.zeros(2, np.float64)
        st = L.ref_align(int(x["n_states"]), int(x["initial"]), p(x["is_final"]), p(x["final_weight"]), p(x["arc_offsets"]), p(x["arc_target"]),
                         p(x["arc_label"]), p(x["arc_weight"]), len(x["label_of"]), p(x["label_of"]), p(x["emission_of"]), T, s.shape[1], p(s),
                         C.c_float(cfg["min_acoustic_pruning"]), C.c_float(cfg["max_acoustic_pruning"]), C.c_float(cfg["increment_factor"]),
                         C.c_double(cfg["min_average_number_of_states"]), int(cfg["increase_until_no_score_difference"]), C.c_float(cfg["score_scale"]),
                         p(label), p(emission), p(arc), p(survivors), p(summary), p(counts), p(avg))
        assert st == 0, "%s: the alignment automaton is not the linear one expected (%d)" % (name, st)
        k = name + "/"
        a[k + "label"], a[k + "emission"], a[k + "arc_score"], a[k + "survivors"] = label, emission, arc, survivors
        a[k + "score"], a[k + "last_threshold"] = summary[0].copy(), summary[1].copy()
        a[k + "reached"], a[k + "n_iterations"], a[k + "automaton_states"] = counts[0].copy(), counts[1].copy(), counts[2].copy()
        a[k + "average_states"], a[k + "state_sum"] = avg[0].copy(), np.array(int(avg[1]), np.int64)
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def lowest_id_wins(g, scores):
    """dense Viterbi without pruning in which every tie goes to the lowest state id (strict < in id and arc order) -> (score, labels)"""
    n, T, F = g["n_states"], len(scores), np.float32
    cur = {g["initial"]: (F(0), None)}
    back = []
    for t in range(T):
        new = {}
        for s in sorted(cur):
            for target, e, l, w in g["arcs"][s]:
                sco = F(F(cur[s][0] + F(w)) + scores[t][e])
                if target not in new or sco < new[target][0]:
                    new[target] = (sco, (s, l))
        back.append(new)
        cur = new
    best, at = None, None
    for s in sorted(cur):
        if g["final"][s]:
            v = F(F(g["final_weight"][s]) + cur[s][0])
            if best is None or v < best:
                best, at = v, s
    labels = []
    for t in range(T - 1, -1, -1):
        at, l = back[t][at][1]
        labels.append(l)
    return best, labels[::-1]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_align.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_align_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    cases = ar.cases()
    arrays = {}
    for name, c in cases.items():
        for k, v in flat(c["graph"]).items():
            arrays["in/%s/%s" % (name, k)] = v
        arrays["in/%s/scores" % name] = np.ascontiguousarray(c["scores"], np.float32)
        cfg = dict(ar.DEFAULTS)
        cfg.update(c["cfg"])
        arrays["cfg/" + name] = np.array([cfg[k] for k in ("min_acoustic_pruning", "max_acoustic_pruning", "increment_factor",
                                                           "min_average_number_of_states", "increase_until_no_score_difference", "score_scale")], np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        got = {}
        for fl in ("off", "fma"):
            L, n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)
            got[fl] = run(L, cases)
    for k, v in got["off"].items():
        arrays["off/" + k] = v
    differ = [k for k, v in got["fma"].items() if not same_bits(v, got["off"][k])]
    for k in differ:
        arrays["fma/" + k] = got["fma"][k]
    arrays["fma_differs"] = np.array(differ if differ else [""])
    arrays["fma_arrays_compared"] = np.array(len(got["fma"]))
    other = []
    for name in TIE_CASES:
        score, labels = lowest_id_wins(cases[name]["graph"], cases[name]["scores"])
        assert same_bits(np.float32(score), got["off"][name + "/score"]), "%s: the lowest-id path does not tie with the reference's (%r, %r)" % (
            name, score, got["off"][name + "/score"])
        if labels != got["off"][name + "/label"].tolist():
            other.append(name)
    assert {"tie_labels", "tie_finals"} <= set(other), "the tie cases do not tell list order from id order: %s" % other
    arrays["ties_where_lowest_id_differs"] = np.array(other)
    first = got["off"]["min_average/average_states"]
    assert got["off"]["min_average/n_iterations"] > got["off"]["defaults_gauss/n_iterations"] - 1 and first >= 18.0
    assert got["off"]["prune_best_first/n_iterations"] == 3 and got["off"]["factor1/n_iterations"] == 1
    assert not got["off"]["unreachable/reached"] and got["off"]["unreachable/score"] == np.finfo(np.float32).max
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    print("  fma instructions: off %d, fma %d" % (int(arrays["fma_instructions/off"]), int(arrays["fma_instructions/fma"])))
    print("  fma copies that differ from off: %d of %d %s" % (len(differ), len(got["fma"]), differ[:6]))
    print("  tie cases in which the lowest state id would have chosen other labels: %s" % other)
    for name in ("empty", "empty_final"):
        print("  %s: score %r reached %d iterations %d average %r automaton states %d" % (
            name, got["off"][name + "/score"], got["off"][name + "/reached"], got["off"][name + "/n_iterations"], got["off"][name + "/average_states"],
            got["off"][name + "/automaton_states"]))


if __name__ == "__main__":
    main()
