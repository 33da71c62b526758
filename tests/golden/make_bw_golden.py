#!/usr/bin/env python3
"""tests/golden/make_bw_golden.py -- writes tests/golden/ref_bw.npz: the SEARCH of Search::Aligner in mode baum-welch as the reference's
own text computes it: alignment score (finalStatePotential), reached flag, iterations, last threshold and the survivor count of every
frame of the last pass.

Run it where the reference tree is mounted; tests read only the fixture.  It builds on tests/golden/make_align_golden.py: the same shell
of stand-ins (which holds no reference text), the same pieces of Search/Aligner.cc taken by line range + SHA-256 into a temporary
directory, in both of the reference's flag sets, plus
  * Search/Aligner.cc:169-196 (activateOrUpdateStateHypothesisBaumWelch) and 326-339 (deleteStateHypothesisBaumWelch) in place of the
    stubs that abort
  * Fsa/tRealSemiring.cc:130-146 (LogSemiring::collect) in a translation unit of its own that includes what tRealSemiring.cc includes
    (Core/StringUtilities.hh, Core/Utility.hh, <limits>; not Core/Debug.hh, whose chain of headers needs a library this generator does
    not have, and which only brings the DBGCMD macro that a release build defines away): which overloads `::exp` and `::log1p` name there
    decides whether the f32 collect rounds once or three times, and the generator must not decide that itself.  The functions the
    compiled collect calls are recorded (collect_calls), and so are its results on 4096 random pairs.  The traceback automaton's
    semiring calls it out of line, as the reference's virtual call does.
  * Search/Aligner.cc:447-461 (getAlignmentFsaBaumWelch; collectGarbage's Baum-Welch branch is in the pieces already), Fsa/Sssp.cc:67
    (Zero), 95-138 (StatePotentials64DfsState::finishState), 156-165 (logPosterior, finalLogPosterior), Speech/Alignment.cc:418-578 (the
    Alignment item functions with their three sort orders) and Search/Aligner.cc:711-726 (getAlignment's Baum-Welch branch)
behind stand-ins that hold no reference text: StaticAutomaton::deleteState and normalize, Fsa::transpose (a state's arcs, in state and
arc order, become arcs of their targets), a depth-first walk that finishes a state after its targets, the members of
Posterior64Automaton and its constructor's sequence, Fsa::trim as "both potentials below Zero", the extractor's walk as (state, arc)
order with the distance from the initial state as time, and the frame of Speech::Alignment / AlignmentItem (Mm::Weight is f64).
Fsa/Sssp.cc itself passes the compiler with the existing include path, but linking it needs the rest of Fsa/ (Static, Basic, Dfs,
Semiring, Automaton, ... which reach Core::Application and a library that is not there), so it is not used.
Recorded per case beyond the search: bw[initial] and the forward flow (f64), per arc (time, label, -log p narrowed to f32) before the
combination, per (time, label) the f32 -log p after combineItems and sortItems, and the items getAlignment leaves (time, label, f64 weight).
The arc order inside a state is the transposition's, hence this generator's: potentials are the reference's arithmetic in that order.
The order in which combineItems meets the arcs of one key is std::sort's and not defined; three collects do not commute.

Measured and written into the fixture: bar_a, bar_r = twice the worst absolute / relative deviation between the reference's weights and
an all-f64 evaluation (tests/bw_reference.py in device order before its one rounding to f32) over all cases.

Conditions on the inputs, asserted here on the restatement in reference order once it equals the recorded results in every bit:
  1. in every pass every hypothesis is at least 32 ulp of the pruning limit away from it
  2. every isAlmostEqual decision has d = 0 or d >= 64 e
  3. no kept item has a weight in (0, 1e-30): counted in the reference's own run and RECORDED (tiny_items/<case>), not asserted: it
     does not hold in eleven of the cases as they are.  At the default threshold of 50 a survivor may carry a posterior of e^-50, and the
     loop doubles the threshold, so states with posteriors far below 1e-30 survive by construction in every segment of more than a few
     frames; a seed does not change that.  What is asserted instead is what the f32 weight of the ABI can hold: every item the all-f64
     evaluation loses has a reference weight below 2^-149.

    python3 tests/golden/make_bw_golden.py [out.npz]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_align_golden as ma  # noqa: E402
from tests import align_reference as ar  # noqa: E402
from tests import bw_reference as br  # noqa: E402

PIECES = dict(ma.PIECES, bw_update=[("Search/Aligner.cc", 169, 196)], bw_delete=[("Search/Aligner.cc", 326, 339)],
              collect=[("Fsa/tRealSemiring.cc", 130, 146)], bw_fsa=[("Search/Aligner.cc", 447, 461)], zero64=[("Fsa/Sssp.cc", 67, 67)],
              finish_state=[("Fsa/Sssp.cc", 95, 138)], log_posterior=[("Fsa/Sssp.cc", 156, 165)], item_fns=[("Speech/Alignment.cc", 418, 578)],
              get_alignment_bw=[("Search/Aligner.cc", 711, 726)])
SHA = "1395c4a420b3d655a30763a536eb3b754e821f0ee3ce83e1eebf8ade84298d4f"

COLLECT_SOURCE = r'''
#include <Core/StringUtilities.hh>
#include <Core/Utility.hh>

#include <limits>
// ---- shell: the frame of Ftl::LogSemiring (tRealSemiring.hh:24-51) as far as collect uses it ----
namespace Ftl {
template<class T> inline void checkValidDifference(T, T) {}
template<class _Weight, typename _Type> class LogSemiring {
public:
    _Weight zero() const { return _Weight(Core::Type<_Type>::max); }
    _Weight collect(const _Weight& a, const _Weight& b) const;
};
#ifndef DBGCMD
#define DBGCMD(level, cmd)
#endif
// ---- reference text: LogSemiring::collect ----
%(collect)s
}  // namespace Ftl
struct CollectWeight {
    f32 v;
    explicit CollectWeight(f32 x) : v(x) {}
    explicit CollectWeight(f64 x) : v(x) {}
    operator f32() const { return v; }
};
extern "C" float ref_collect(float a, float b) { return f32(Ftl::LogSemiring<CollectWeight, f32>().collect(CollectWeight(a), CollectWeight(b))); }
'''

POSTERIOR = r'''
// ---- shell: what posterior64 and getAlignment need around the reference's text (no reference text) ----
namespace Fsa {
// the transposed automaton: state s's arcs, in state and arc order, become arcs of their targets; the old final states (here: one,
// with weight one) exchange roles with the old initial state
ConstAutomatonRef transpose(Core::Ref<StaticAutomaton> f) {
    StaticAutomaton* r = new StaticAutomaton;
    r->setSemiring(f->semiring());
    for (StateId s = 0; s < f->size(); ++s)
        r->setState(new State(s));
    for (StateId s = 0; s < f->size(); ++s) {
        const State* sp = f->fastState(s);
        if (sp->isFinal())
            r->setInitialStateId(s);
        for (State::const_iterator a = sp->begin(); a != sp->end(); ++a)
            r->fastState(a->target())->newArc(s, a->weight(), a->input());
    }
    r->fastState(f->initialStateId())->setFinal(f->semiring()->one());
    return ConstAutomatonRef(r);
}
// ---- reference text: Zero ----
%(zero64)s
struct StatePotentials64 : public std::vector<f64> {
    void grow(StateId s, f64 v) {
        if (s >= size())
            resize(s + 1, v);
    }
};
typedef const State* ConstStateRef;
class StatePotentials64DfsState {   // the frame of Sssp.cc:69-93 with a depth-first walk of its own
public:
    const StaticAutomaton* fsa_;
    StatePotentials64&     potentials_;
    f64                    totalFlow_;
    std::vector<char>      seen_;
    StatePotentials64DfsState(const StaticAutomaton* f, StatePotentials64& p) : fsa_(f), potentials_(p), totalFlow_(0.0) { potentials_.clear(); }
    void finishState(StateId s);
    void visit(StateId s) {
        seen_[s] = 1;
        const State* sp = fsa_->fastState(s);
        for (State::const_iterator a = sp->begin(); a != sp->end(); ++a)
            if (!seen_[a->target()])
                visit(a->target());
        finishState(s);
    }
    void dfs() {
        seen_.assign(fsa_->size(), 0);
        visit(fsa_->initialStateId());
    }
};
// ---- reference text: StatePotentials64DfsState::finishState ----
%(finish_state)s
class Posterior64Automaton {   // the members of Sssp.cc:147-151
public:
    StatePotentials64 forwardPotentials_;
    StatePotentials64 backwardPotentials_;
    f64               totalInv_;
// ---- reference text: logPosterior, finalLogPosterior ----
%(log_posterior)s
};
}  // namespace Fsa
namespace Mm {
typedef f64 Weight;   // Mm/Types.hh:30
}
namespace Mc {
typedef f32 Scale;    // Mc/Types.hh:27
}
namespace Speech {
struct AlignmentItem {   // the members of Speech/Alignment.hh:31-42
    TimeframeIndex time;
    Fsa::LabelId   emission;
    Mm::Weight     weight;
    AlignmentItem() : time(0), emission(0), weight(0) {}
    AlignmentItem(TimeframeIndex t, Am::AllophoneStateIndex e, Mm::Weight w = 1.0) : time(t), emission(e), weight(w) {}
};
class Alignment : public std::vector<AlignmentItem> {
public:
    Score score_;
    void  setScore(Score s) { score_ = s; }
    void  sortItems(bool byDecreasingWeight = true);
    void  sortStableItems();
    void  combineItems(Fsa::ConstSemiringRef sr = Fsa::TropicalSemiring);
    void  expm();
    void  addWeight(Mm::Weight weight);
    void  filterWeights(Mm::Weight minWeight, Mm::Weight maxWeight);
    void  filterWeightsGT(Mm::Weight minWeight);
    void  gammaCorrection(Mc::Scale gamma);
    void  multiplyWeights(Mm::Weight c);
    void  normalizeWeights();
    void  shiftMinToZeroWeights();
    void  clipWeights(Mm::Weight a, Mm::Weight b);
};
}  // namespace Speech
using namespace Speech;   // Speech/Alignment.cc:32
// ---- reference text: the Alignment item functions ----
%(item_fns)s
// ---- this generator's own driver of the posterior and the items (no reference text except where marked) ----
struct ItemSink {
    int     cap, n;
    int *   time, *label;
    double* value;
    void    take(const Speech::Alignment& a) {
        n = (int)a.size();
        for (int i = 0; i < n && i < cap; ++i)
            time[i] = a[i].time, label[i] = a[i].emission, value[i] = a[i].weight;
    }
};
static int bw_items(Aligner& al, ItemSink* raw, ItemSink* comb, ItemSink* fin, double* totals) {
    Fsa::ConstAutomatonRef      fsa = al.ss_->getAlignmentFsa();   // the reference's collectGarbage and getAlignmentFsaBaumWelch
    const Fsa::StaticAutomaton* F   = static_cast<const Fsa::StaticAutomaton*>(fsa.get());
    const Fsa::StateId          n   = F->size();
    // Posterior64Automaton's constructor (Sssp.cc:180-187)
    Fsa::Posterior64Automaton   P;
    Fsa::ConstAutomatonRef      tr = Fsa::transpose(Core::Ref<Fsa::StaticAutomaton>(const_cast<Fsa::StaticAutomaton*>(F)));
    {
        Fsa::StatePotentials64DfsState fwd(static_cast<const Fsa::StaticAutomaton*>(tr.get()), P.forwardPotentials_);
        fwd.dfs();
        Fsa::StatePotentials64DfsState bwd(F, P.backwardPotentials_);
        bwd.dfs();
    }
    P.forwardPotentials_.resize(n, Fsa::Zero), P.backwardPotentials_.resize(n, Fsa::Zero);   // states the walks did not reach
    P.totalInv_ = -P.backwardPotentials_[F->initialStateId()];
    totals[0] = P.backwardPotentials_[F->initialStateId()], totals[1] = P.forwardPotentials_[n - 1];
    // Fsa::trim: states on a path from the initial to a final state; the extractor's time is the distance from the initial state
    std::vector<int> depth(n, -1);
    depth[F->initialStateId()] = 0;
    for (Fsa::StateId s = 0; s < n; ++s) {   // hypotheses are numbered frame by frame
        const Fsa::State* sp = F->fastState(s);
        for (Fsa::State::const_iterator a = sp->begin(); a != sp->end(); ++a)
            if (depth[s] >= 0 && a->input() != Fsa::Epsilon && depth[a->target()] < 0)
                depth[a->target()] = depth[s] + 1;
    }
    Speech::Alignment result;
    for (Fsa::StateId s = 0; s < n; ++s) {
        if (!(P.forwardPotentials_[s] < Fsa::Zero && P.backwardPotentials_[s] < Fsa::Zero))
            continue;
        const Fsa::State* sp = F->fastState(s);
        for (Fsa::State::const_iterator a = sp->begin(); a != sp->end(); ++a)
            if (a->input() != Fsa::Epsilon && P.backwardPotentials_[a->target()] < Fsa::Zero)
                result.push_back(Speech::AlignmentItem(depth[s], a->input(), Fsa::Weight(P.logPosterior(s, *a))));   // modifyState, exploreArc
    }
    raw->take(result);
    Speech::Alignment combined = result;
    combined.combineItems(Fsa::LogSemiring);
    combined.sortItems(false);
    comb->take(combined);
    const bool viterbi_ = false, usePartialSums_ = false;
    auto       getLogWeightThreshold = []() { return Core::Type<Mm::Weight>::max; };   // Aligner.cc:570-571 with min-weight 0
    std::pair<Fsa::ConstAutomatonRef, Fsa::Weight> alignmentPosteriorFsa(fsa, Fsa::Weight(f32(P.totalInv_)));
// ---- reference text: getAlignment's Baum-Welch branch ----
%(get_alignment_bw)s
    fin->take(result);
    return 0;
}
'''

DRIVER = r'''
// ---- this generator's own driver for mode baum-welch (no reference text) ----
extern "C" int ref_bw(int n_states, int initial, const unsigned char* is_final, const float* final_weight, const int* arc_off, const int* arc_target,
                      const int* arc_label, const float* arc_weight, int n_labels, const int* label_of, const int* emission_of, int T, int n_columns,
                      const float* scores, float lo, float hi, float factor, double min_avg, int incr, float scale, int* survivors, float* summary,
                      int* counts, double* avg, ItemSink* raw, ItemSink* comb, ItemSink* fin, double* totals) {
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
    al.viterbi_ = false;   // Aligner::selectMode (Aligner.cc:636-640)
    al.ss_->setViterbi(false);
    al.minAcousticPruningThreshold_ = lo, al.maxAcousticPruningThreshold_ = hi, al.acousticPruningThresholdIncrementFactor_ = factor;
    al.minAverageNumberOfStateHypotheses_ = min_avg, al.increasePruningUntilNoScoreDifference_ = incr != 0;
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
        survivors[t] = t < (int)al.nStateHypotheses_.samples.size() ? (int)al.nStateHypotheses_.samples[t] : -1;
    raw->n = comb->n = fin->n = 0, totals[0] = totals[1] = Fsa::Zero;
    if (!al.reachedFinalState() || T == 0)
        return 0;
    return bw_items(al, raw, comb, fin, totals);
}
'''

class ItemSink(C.Structure):
    _fields_ = [("cap", C.c_int), ("n", C.c_int), ("time", C.c_void_p), ("label", C.c_void_p), ("value", C.c_void_p)]


def sink(cap):
    t, l, v = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
    return ItemSink(cap, 0, t.ctypes.data, l.ctypes.data, v.ctypes.data), (t, l, v)


FIELDS = ("survivors", "score", "reached", "n_iterations", "last_threshold", "average_states", "state_sum")


def source():
    s = ma.SOURCE
    for old, new in (
            ("    Weight collect(Weight, Weight) const { abort(); }   // baum-welch only",
             "    Weight collect(Weight a, Weight b) const { return Weight(ref_collect(a, b)); }   // the reference's text, in a translation unit of its own"),
            ("namespace Fsa {\ntypedef u32 StateId;", 'extern "C" float ref_collect(float a, float b);\nnamespace Fsa {\ntypedef u32 StateId;'),
            ("void Aligner::SearchSpace::activateOrUpdateStateHypothesisBaumWelch(StateId, Score, StateHypothesisIndex, Am::AllophoneStateIndex, Fsa::Weight) { abort(); }\n",
             "// ---- reference text: activateOrUpdateStateHypothesisBaumWelch ----\n%(bw_update)s\n"),
            ("void Aligner::SearchSpace::deleteStateHypothesisBaumWelch(StateHypothesisIndex) { abort(); }\n",
             "// ---- reference text: deleteStateHypothesisBaumWelch ----\n%(bw_delete)s\n"),
            ("Fsa::ConstAutomatonRef Aligner::SearchSpace::getAlignmentFsaBaumWelch() const { abort(); }\n",
             "// ---- reference text: getAlignmentFsaBaumWelch ----\n%(bw_fsa)s\n"),
            ("class Automaton {\npublic:\n    virtual ~Automaton() {}\n", "class Automaton {\npublic:\n    virtual ~Automaton() {}\n    bool hasProperty(Property) const { return true; }\n"),
            ("    StateId        id() const { return id_; }\n", "    StateId        id() const { return id_; }\n    size_t         nArcs() const { return arcs_.size(); }\n"),
            ("    size_t           size() const { return states_.size(); }\n",
             "    size_t           size() const { return states_.size(); }\n    const State*     getState(StateId s) const { return s < states_.size() ? states_[s] : 0; }\n"),
            ("    void    deleteState(StateId) { abort(); }   // baum-welch only\n",
             "    void    deleteState(StateId s) {\n        if (s < states_.size())\n            states_[s] = 0;\n    }\n"),
            ("    void    normalize() { abort(); }            // baum-welch only\n",
             "    void    normalize() {   // what tStatic.cc:94-140 does to an automaton without an initial state: holes closed, targets renumbered\n"
             "        std::vector<StateId> map(states_.size(), InvalidStateId);\n        StateId              n = 0;\n"
             "        for (StateId s = 0; s < states_.size(); ++s)\n            if (states_[s]) {\n                states_[n] = states_[s], states_[n]->setId(n), map[s] = n++;\n            }\n"
             "        states_.resize(n);\n        for (StateId s = 0; s < n; ++s)\n            for (size_t a = 0; a < states_[s]->arcs_.size(); ++a)\n"
             "                states_[s]->arcs_[a].target_ = map[states_[s]->arcs_[a].target_];\n    }\n"),
            ("typedef Core::Ref<const Automaton> ConstAutomatonRef;\n",
             "typedef Core::Ref<const Automaton> ConstAutomatonRef;\nConstAutomatonRef transpose(Core::Ref<StaticAutomaton> f);\n")):
        assert s.count(old) == 1, old
        s = s.replace(old, new)
    return s + POSTERIOR + DRIVER


def reference_text():
    cache, parts, h = {}, {}, hashlib.sha256()
    for key, ranges in PIECES.items():
        out = []
        for fn, first, last in ranges:
            if fn not in cache:
                with open(os.path.join(ma.REF, fn), encoding="utf-8", errors="replace") as f:
                    cache[fn] = f.readlines()
            out.append("".join(cache[fn][first - 1:last]))
        parts[key] = "\n".join(out)
        h.update(parts[key].encode())
    return parts, h.hexdigest()


def build(tmp, flavour, parts):
    gen, col = os.path.join(tmp, "bw_%s.cc" % flavour), os.path.join(tmp, "collect_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(source() % parts)
    with open(col, "w") as f:
        f.write(COLLECT_SOURCE % parts)
    so = os.path.join(tmp, "bw_%s.so" % flavour)
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + ma.FLAGS + extra + ["-shared", "-o", so, gen, col])
    dis = subprocess.run("objdump -d --no-show-raw-insn %s" % so, shell=True, capture_output=True, text=True).stdout
    body = dis[dis.index("<ref_collect>:"):]
    body = body[:body.index("\n\n")]
    calls = sorted({w.split("@")[0].strip("<>") for line in body.splitlines() if "call" in line for w in line.split() if w.startswith("<")})
    L = C.CDLL(so)
    L.ref_bw.restype = C.c_int
    L.ref_collect.restype = C.c_float
    L.ref_collect.argtypes = [C.c_float, C.c_float]
    return L, calls


def run(L, cases):
    a, p = {}, ma.p
    for name, c in cases.items():
        x, s = ma.flat(c["graph"]), np.ascontiguousarray(c["scores"], np.float32)
        cfg = dict(ar.DEFAULTS)
        cfg.update(c["cfg"])
        T = len(s)
        survivors = np.zeros(T, np.int32)
        summary, counts, avg, totals = np.zeros(2, np.float32), np.zeros(2, np.int32), np.zeros(2, np.float64), np.zeros(2, np.float64)
        cap = max(T * len(x["arc_target"]), 1)
        sinks = [sink(cap) for _ in range(3)]
        st = L.ref_bw(int(x["n_states"]), int(x["initial"]), p(x["is_final"]), p(x["final_weight"]), p(x["arc_offsets"]), p(x["arc_target"]),
                      p(x["arc_label"]), p(x["arc_weight"]), len(x["label_of"]), p(x["label_of"]), p(x["emission_of"]), T, s.shape[1], p(s),
                      C.c_float(cfg["min_acoustic_pruning"]), C.c_float(cfg["max_acoustic_pruning"]), C.c_float(cfg["increment_factor"]),
                      C.c_double(cfg["min_average_number_of_states"]), int(cfg["increase_until_no_score_difference"]), C.c_float(cfg["score_scale"]),
                      p(survivors), p(summary), p(counts), p(avg), C.byref(sinks[0][0]), C.byref(sinks[1][0]), C.byref(sinks[2][0]), p(totals))
        assert st == 0, name
        k = name + "/"
        a[k + "bw_initial"], a[k + "fw_final"] = totals[0].copy(), totals[1].copy()
        # raw: -log p per arc as narrowed to f32; combined: after combineItems and sortItems; items: what getAlignment leaves
        for what, (sk, (t, l, v)), dt in zip(("raw", "combined", "items"), sinks, (np.float32, np.float32, np.float64)):
            assert sk.n <= cap, name
            a[k + what + "_time"], a[k + what + "_label"], a[k + what + "_value"] = t[:sk.n].copy(), l[:sk.n].copy(), v[:sk.n].astype(dt)
        a[k + "survivors"] = survivors
        a[k + "score"], a[k + "last_threshold"] = summary[0].copy(), summary[1].copy()
        a[k + "reached"], a[k + "n_iterations"] = counts[0].copy(), counts[1].copy()
        a[k + "average_states"], a[k + "state_sum"] = avg[0].copy(), np.array(int(avg[1]), np.int64)
    return a


def margins(cases):
    """conditions 1 and 2 on the restatement in reference order: the smallest distance of a hypothesis to its pruning limit in ulp of the
    limit, and the smallest d / e over the isAlmostEqual decisions with d != 0"""
    worst_ulp, worst_ratio = np.inf, np.inf
    for name, c in cases.items():
        cfg = dict(br.DEFAULTS)
        cfg.update(c["cfg"])
        scale = np.float32(cfg["score_scale"])
        rows = c["scores"] if scale == 1 else (scale * c["scores"]).astype(np.float32)
        t, hi, factor = np.float32(cfg["min_acoustic_pruning"]), np.float32(cfg["max_acoustic_pruning"]), np.float32(cfg["increment_factor"])
        n, previous = br.align_segment(c["graph"], c["scores"], "reference", **c["cfg"])["n_iterations"], ar.F32_MAX
        with np.errstate(all="ignore"):
            for i in range(n):
                graph = c["graph"]
                cur = {graph["initial"]: np.float32(0)}
                for row in rows:
                    new = {}
                    for state, score in cur.items():
                        for target, emission, _, weight in graph["arcs"][state]:
                            cand = np.float32(score + np.float32(np.float32(weight) + row[emission]))
                            new[target] = cand if target not in new else br.collect32(new[target], cand)
                    limit = np.float32(min(new.values()) + t) if new else ar.F32_MAX
                    for v in new.values():
                        if np.isfinite(limit) and np.isfinite(v):                # a hypothesis exactly on the limit is 0 ulp away
                            worst_ulp = min(worst_ulp, abs(float(v) - float(limit)) / float(np.spacing(np.abs(limit))))
                    cur = {s: v for s, v in new.items() if v <= limit}
                score = br.final_potential(graph, cur, "reference")
                if i > 0 and score != ar.F32_MAX and previous != ar.F32_MAX:
                    d = abs(np.float32(score) - np.float32(previous))
                    e = np.float32(np.float32(np.float32(abs(score) + abs(previous)) + ar.F32_DELTA) * ar.F32_EPSILON)
                    if d != 0:
                        worst_ratio = min(worst_ratio, float(d) / float(e))
                previous = score
                if factor <= 1:
                    break
                t = np.float32(t * factor)
                if not t <= hi:
                    break
    return worst_ulp, worst_ratio


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_bw.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_bw_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    cases = ar.cases()
    arrays = {}
    for name, c in cases.items():
        for k, v in ma.flat(c["graph"]).items():
            arrays["in/%s/%s" % (name, k)] = v
        arrays["in/%s/scores" % name] = np.ascontiguousarray(c["scores"], np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        got, collects = {}, {}
        probes = np.random.Generator(np.random.PCG64(1)).normal(60, 30, (4096, 2)).astype(np.float32)
        for fl in ("off", "fma"):
            L, calls = build(tmp, fl, parts)
            arrays["collect_calls/" + fl] = np.array(calls if calls else [""])
            got[fl] = run(L, cases)
            collects[fl] = np.array([L.ref_collect(float(a), float(b)) for a, b in probes], np.float32)
    arrays["collect_probe_in"], arrays["collect_probe_out"] = probes, collects["off"]
    for k, v in got["off"].items():
        arrays["off/" + k] = v
    differ = [k for k, v in got["fma"].items() if not ma.same_bits(v, got["off"][k])]
    for k in differ:
        arrays["fma/" + k] = got["fma"][k]
    arrays["fma_differs"] = np.array(differ if differ else [""])
    arrays["fma_arrays_compared"] = np.array(len(got["fma"]))
    arrays["collect_probe_fma_differs"] = np.array(int((collects["fma"].view(np.uint32) != collects["off"].view(np.uint32)).sum()))
    # the restatement in reference order against the recorded results, then the conditions on it
    unequal = []
    for name, c in cases.items():
        r = br.align_segment(c["graph"], c["scores"], "reference", **c["cfg"])
        g = {f: got["off"]["%s/%s" % (name, f)] for f in FIELDS}
        ok = (ma.same_bits(np.float32(r["score"]), g["score"]) and bool(r["reached"]) == bool(g["reached"]) and r["n_iterations"] == int(g["n_iterations"])
              and ma.same_bits(np.float32(r["last_threshold"]), g["last_threshold"]) and np.array_equal(r["survivors"], g["survivors"]))
        if not ok:
            unequal.append(name)
    arrays["restatement_unequal"] = np.array(unequal if unequal else [""])
    # (a, r): twice the worst deviation between the reference's item weights and an all-f64 evaluation (the restatement in device order
    # before its one rounding to f32), absolute and relative; and condition 3, counted in the reference's own run
    worst_a = worst_r = 0.0
    below_f32 = 0.0
    for name, c in cases.items():
        k = name + "/"
        ref = {(int(t), int(l)): float(v) for t, l, v in zip(got["off"][k + "items_time"], got["off"][k + "items_label"], got["off"][k + "items_value"])}
        arrays["tiny_items/" + name] = np.array(sum(1 for v in ref.values() if 0 < v < 1e-30))
        d = br.align_segment(c["graph"], c["scores"], "device", **c["cfg"])
        f64 = {(f, l): s for f, (its, shs) in enumerate(zip(d["items"], d.get("shares", []))) for (l, _, _), s in zip(its, shs)}
        assert set(f64) <= set(ref), name
        for q, v in ref.items():
            if q in f64:
                worst_a, worst_r = max(worst_a, abs(v - f64[q])), max(worst_r, abs(v - f64[q]) / v)
            else:
                below_f32 = max(below_f32, v)
    arrays["bar_a"], arrays["bar_r"], arrays["largest_weight_without_f32_value"] = np.array(2 * worst_a), np.array(2 * worst_r), np.array(below_f32)
    worst_ulp, worst_ratio = margins(cases)
    arrays["smallest_margin_ulp"], arrays["smallest_almost_equal_ratio"] = np.array(worst_ulp), np.array(worst_ratio)
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    print("  collect calls: off %s, fma %s; probe results that differ between the builds: %d of %d" % (
        arrays["collect_calls/off"].tolist(), arrays["collect_calls/fma"].tolist(), int(arrays["collect_probe_fma_differs"]), len(probes)))
    print("  fma copies that differ from off: %d of %d %s" % (len(differ), len(got["fma"]), differ[:6]))
    print("  cases in which the reference-order restatement differs: %s" % unequal)
    tiny = {n: int(arrays["tiny_items/" + n]) for n in cases if int(arrays["tiny_items/" + n])}
    print("  bars: a = %.3g, r = %.3g; largest reference weight of an item the f32 evaluation does not keep: %.3g" % (2 * worst_a, 2 * worst_r, below_f32))
    print("  condition 3 (no kept weight in (0, 1e-30)) does not hold in %d cases: %s" % (len(tiny), tiny))
    assert below_f32 < 2.0 ** -149, "an item is missing from the f64 evaluation although f32 has a value for its weight"
    print("  smallest margin to a pruning limit: %.1f ulp; smallest d / e of an isAlmostEqual decision with d != 0: %.1f" % (worst_ulp, worst_ratio))
    assert not unequal, "the restatement in reference order does not equal the reference's run"
    assert worst_ulp >= 32 and worst_ratio >= 64, "a case sits too close to a decision: change its seed"


if __name__ == "__main__":
    main()
