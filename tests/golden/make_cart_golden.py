#!/usr/bin/env python3
"""tests/golden/make_cart_golden.py -- writes tests/golden/ref_cart.npz: decision-tree state tying as the reference computes it, from the
reference's own text.

Run it where the reference tree is mounted; tests read only the fixture.  What it compiles, in both of the reference's arithmetics (the
flag sets of oracle/ref/Makefile: -msse3 = contract=off, -msse3 -march=native = contract=fma), taken by line range + SHA-256 into a
temporary directory that is deleted afterwards:
  * Cart/DecisionTreeTrainer.cc:121-837 (class Training: init, splitNode, insertSplit, suggestSplit, commitSplit, commitHalfSplit,
    rollbackSplit, split, halfSplit, start, commitNode, finish, train, with its Node, SplitHypothesesManager, Split and statistics)
  * Speech/DecisionTreeTrainer.cc:54-90 (FeatureAccumulator::processAlignedFeature), 106 (PI), 134-234 (LogLikelihoodGain::logLikelihood),
    236-250 (its two operator())
  * Core/PriorityQueue.hh:25-118 (PriorityQueueBase with upHeap and downHeap), 123-166 (UntracedHeap), 242-251 (PriorityQueue)
  * Core/Utility.cc:61-73 (differenceUlp) and Core/Utility.hh:384-388 (isAlmostEqualUlp)
behind a shell of this file's own that holds no reference text: stand-ins for Core::Component (log, error, warning, criticalError), the
configuration and parameter classes, the XML writer (it keeps the numbers insertSplit reports: that is how the commit log leaves the
class), Cart::FloatBox, Example, ExampleList, Properties, PropertyMap, Question (it answers from a bit table by example index), DecisionTree
and its nodes, TrainingInformation, TrainingPlan, Cluster, ClusterList, Scorer, the frames of LogLikelihoodGain and FeatureAccumulator, and
the acoustic-model calls processAlignedFeature makes.

The cases are tests/cart_reference.py's cases() and this file's accumulation cases.  Recorded per case and build: the inputs, the whole
tree, the commit log, the classes, the question statistics, the counters; from the restatement the smallest gap between two compared
gains in units of their bar (decided_gap) and per node a score_bar from glibc's documented 1-ulp bound on log over that node's chain.
Asserted here, where it runs: the restatement equals the reference in every bit, in both builds, on every case; exactly the sites
cart_reference.FMA_SITES names reproduce the -march=native build; every case not named tie_* is decided; every planted defect leaves
its case.

    python3 tests/golden/make_cart_golden.py [out.npz]
"""
import ctypes as C
import hashlib
import io
import itertools
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import cart_reference as cr  # noqa: E402

REF = "/root/reference/src"
PIECES = {
    "priority_queue": [("Core/PriorityQueue.hh", 25, 118), ("Core/PriorityQueue.hh", 123, 166), ("Core/PriorityQueue.hh", 242, 251)],
    "difference_ulp": [("Core/Utility.cc", 61, 73)],
    "almost_equal_ulp": [("Core/Utility.hh", 384, 388)],
    "training": [("Cart/DecisionTreeTrainer.cc", 121, 837)],
    "accumulate": [("Speech/DecisionTreeTrainer.cc", 54, 90)],
    "pi": [("Speech/DecisionTreeTrainer.cc", 106, 106)],
    "log_likelihood": [("Speech/DecisionTreeTrainer.cc", 134, 234)],
    "gain": [("Speech/DecisionTreeTrainer.cc", 236, 250)],
}
SHA = "0635c12ddca991fb90b594ea38c79189c8ffc651c747603658d530d7a2ab2890"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/Types.hh>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <cstdlib>
#include <functional>
#include <deque>
#include <iostream>
#include <string>
#include <utility>
#include <vector>
// ---- shell: stand-ins (no reference text) ----
struct Event {
    int         kind;   // 0 open, 1 full, 2 attribute, 3 close
    std::string name;
    double      value;
};
static std::vector<Event> g_events;
static int                g_errors, g_warnings;
namespace Core {
template<class T> inline T abs(T v) { return v < 0 ? -v : v; }
s32 differenceUlp(f32, f32);
struct Configuration {
    double clip;
};
struct ParameterBool {
    ParameterBool(const char*, const char*, bool = false) {}
    bool operator()(const Configuration&) const { return false; }
};
struct ParameterFloat {
    ParameterFloat(const char*, const char*, double = 0) {}
    double operator()(const Configuration& c) const { return c.clip; }
};
struct XmlAttribute {
    template<class T> XmlAttribute(const char* n, const T& v) { g_events.push_back(Event{2, n, (double)v}); }
};
struct XmlItem {
    XmlItem operator+(const XmlAttribute&) const { return *this; }
};
struct XmlOpen : XmlItem {
    XmlOpen(const char* n) { g_events.push_back(Event{0, n, 0}); }
};
struct XmlClose : XmlItem {
    XmlClose(const char* n) { g_events.push_back(Event{3, n, 0}); }
};
struct XmlEmpty : XmlItem {
    XmlEmpty(const char*) {}
};
struct XmlFull : XmlItem {
    template<class T> XmlFull(const char* n, const T& v) { g_events.push_back(Event{1, n, (double)v}); }
};
struct XmlWriter {
    XmlWriter& operator<<(const XmlItem&) { return *this; }
};
static XmlWriter g_xml;
class Component {
public:
    struct Message {
        operator XmlWriter&() { return g_xml; }
        operator std::ostream&() { return std::cerr; }
        template<class T> Message& operator<<(const T&) { return *this; }
    };
    Configuration config;
    Component(const Configuration& c) : config(c) {}
    virtual ~Component() {}
    Message log() const { return Message(); }
    Message error() const {
        ++g_errors;
        return Message();
    }
    void error(const char*, ...) const { ++g_errors; }
    void warning(const char*, ...) const { ++g_warnings; }
    void criticalError(const char*, ...) const { ++g_errors; }
    Configuration select(const char*) const { return config; }
};
namespace omp {
inline int get_num_threads() { return 1; }
}
template<class T> struct Ref {
    T* p;
    Ref(T* q = 0) : p(q) {}
    T* operator->() const { return p; }
    T& operator*() const { return *p; }
    T* get() const { return p; }
};
}  // namespace Core
namespace Cart {
enum Answer { RASR_FALSE = 0, RASR_TRUE = 1, RASR_UNDEF = 2 };
typedef f64 Score;
class FloatBox {
    std::vector<f64> v_;
    size_t           rows_, cols_;
public:
    typedef f64*       vector_iterator;
    typedef const f64* const_vector_iterator;
    struct Row {
        f64*   p;
        size_t n;
        f64*   begin() const { return p; }
        f64*   end() const { return p + n; }
    };
    FloatBox(size_t r, size_t c) : v_(r * c, 0.0), rows_(r), cols_(c) {}
    size_t rows() const { return rows_; }
    size_t columns() const { return cols_; }
    Row    row(size_t i) { return Row{v_.data() + i * cols_, cols_}; }
};
struct Properties {
    u32 index;
    Properties(u32 i = 0) : index(i) {}
    virtual ~Properties() {}
};
struct PropertyMap {};
struct PropertyMapRef {
    PropertyMap* p;
    PropertyMapRef(PropertyMap* q = 0) : p(q) {}
    PropertyMap* get() const { return p; }
    PropertyMap& operator*() const { return *p; }
};
struct PropertyMapDiff {
    PropertyMapDiff(const Core::Configuration&, const PropertyMap&, const PropertyMap&, bool) {}
    bool hasDifferences() const { return false; }
};
struct Example {
    Properties* properties;
    FloatBox*   values;
    f64         nObs;
    Example(Properties* p, FloatBox* v) : properties(p), values(v), nObs(0) {}
};
struct ExampleRef {
    Example* p;
    ExampleRef(Example* q = 0) : p(q) {}
    Example* get() const { return p; }
    Example* operator->() const { return p; }
    Example& operator*() const { return *p; }
    bool     operator!() const { return !p; }
};
struct ExampleList : std::vector<ExampleRef> {
    PropertyMapRef map_;
    void           setMap(PropertyMapRef m) { map_ = m; }
    PropertyMapRef getMap() const { return map_; }
    PropertyMap&   map() const { return *map_; }
    void           set(size_t id, Example* e) {
        if (id >= size())
            resize(id + 1);
        (*this)[id] = ExampleRef(e);
    }
};
typedef std::vector<ExampleRef>     ConstExampleRefList;
typedef std::vector<const Example*> ExamplePtrList;
struct ExamplePtrRange {
    ExamplePtrList::const_iterator begin, end;
    ExamplePtrRange(ExamplePtrList::const_iterator b, ExamplePtrList::const_iterator e) : begin(b), end(e) {}
    size_t size() const { return end - begin; }
};
struct Question {   // answers from a bit table by example index
    const u32* bits;
    int        step, row, index;
    Answer operator()(const Properties& p) const { return (bits[p.index >> 5] >> (p.index & 31)) & 1u ? RASR_TRUE : RASR_FALSE; }
    void   write(Core::XmlWriter& xml) const { xml << Core::XmlFull("question-index", index); }
};
typedef const Question*          QuestionRef;
typedef std::vector<QuestionRef> QuestionRefList;
struct TrainingInformation {
    static constexpr u32 InvalidOrder = 0xffffffffu;
    u32              order, nObs;
    Score            score;
    TrainingInformation(u32 o, u32 n, Score s) : order(o), nObs(n), score(s) {}
};
class DecisionTree {
public:
    typedef u32 QuestionId;
    typedef u32 ClassId;
    struct Node {
        static constexpr u32 InvalidId = 0xffffffffu;
        Node *               left_, *right_;
        u32                  id_;
        TrainingInformation* info_;
        Node(Node* l, Node* r, TrainingInformation* i) : left_(l), right_(r), id_(InvalidId), info_(i) {}
        void setChilds(Node* l, Node* r) { left_ = l, right_ = r; }
    };
    QuestionRefList* questions;
    Node*            root;
    DecisionTree() : questions(0), root(0) {}
    void    setMap(PropertyMapRef) {}
    void    setQuestions(QuestionRefList* q) { questions = q; }
    void    setRoot(Node* r) { root = r; }
    ClassId classify(const Properties& p) const {
        const Node* n = root;
        while (n->left_ && n->right_)
            n = (*(*questions)[n->id_])(p) == RASR_TRUE ? n->left_ : n->right_;
        return n->id_;
    }
};
struct Cluster {
    DecisionTree::Node*  node;
    ConstExampleRefList* exampleRefs;
    Cluster(DecisionTree::Node* n, ConstExampleRefList* e) : node(n), exampleRefs(e) {}
};
struct ClusterList : std::vector<Cluster*> {
    ClusterList(const Core::Configuration&, PropertyMapRef) {}
    void add(Cluster* c) { push_back(c); }
};
class Scorer : public Core::Component {
public:
    Scorer(const Core::Configuration& c) : Core::Component(c) {}
    virtual Score operator()(const ExamplePtrRange&, const ExamplePtrRange&, const Score, Score&, Score&) const = 0;
    virtual void  operator()(const ExamplePtrRange&, Score&) const                                          = 0;
};
class DecisionTreeTrainer {
public:
    typedef TrainingInformation Information;
    struct TrainingPlan {
        struct Step {
            std::string      action;
            u32              minObs;
            Score            minGain;
            u32              nRandomQuestion;
            QuestionRefList* questionRefs;
            void             write(Core::Component::Message) const {}
        };
        typedef std::vector<Step*> StepPtrList;
        PropertyMapRef             map;
        u32                        maxLeaves;
        StepPtrList                steps;
    };
};
struct StoredProperties : Properties {
    template<class P> StoredProperties(const P& p) : Properties((u32)p.id) {}
};
}  // namespace Cart
// ---- reference text: Core::PriorityQueue ----
namespace Core {
%(priority_queue)s
}
// ---- reference text: differenceUlp, isAlmostEqualUlp ----
%(difference_ulp)s
namespace Core {
%(almost_equal_ulp)s
}
using namespace Cart;
// ---- reference text: class Training ----
%(training)s
// ---- shell
const Core::ParameterBool Cart::Training::paramDoParallel("", "");
namespace Mm {
typedef f64              Weight;
typedef std::vector<f32> FeatureVector;
}
namespace Am {
typedef s32 AllophoneStateIndex;
struct AllophoneState {
    s32 id;
};
struct Properties {
    s32 id;
    Properties(Cart::PropertyMapRef, AllophoneState s) : id(s.id) {}
};
struct AllophoneStateAlphabet {
    bool           isDisambiguator(AllophoneStateIndex) const { return false; }
    std::string    symbol(AllophoneStateIndex) const { return ""; }
    AllophoneState allophoneState(AllophoneStateIndex id) const { return AllophoneState{id}; }
};
struct AcousticModel {
    AllophoneStateAlphabet        alphabet;
    const AllophoneStateAlphabet* allophoneStateAlphabet() const { return &alphabet; }
};
}  // namespace Am
namespace Speech {
struct Feature {
    Mm::FeatureVector        v;
    const Mm::FeatureVector* mainStream() const { return &v; }
};
class FeatureAccumulator : public Core::Component {
public:
    Cart::ExampleList    examples_;
    f64                  nObs_;
    size_t               nCols_;
    Cart::PropertyMapRef map_;
    Am::AcousticModel    model_;
    FeatureAccumulator(const Core::Configuration& c) : Core::Component(c), nObs_(0), nCols_(0) {}
    const Am::AcousticModel* acousticModel() const { return &model_; }
    virtual void processAlignedFeature(Core::Ref<const Feature> f, Am::AllophoneStateIndex id);
    virtual void processAlignedFeature(Core::Ref<const Feature> f, Am::AllophoneStateIndex id, Mm::Weight w);
};
class StateTyingDecisionTreeTrainer {
public:
    class LogLikelihoodGain : public Cart::Scorer {
        typedef Cart::Scorer Precursor;
    public:
        f64                      minSigmaSquare_;
        mutable std::vector<f64> mu_;
        mutable std::vector<f64> sigmaSquare_;
        bool                     parallel_;
        LogLikelihoodGain(const Core::Configuration& c) : Precursor(c), minSigmaSquare_(c.clip), parallel_(false) {}
        Cart::Score logLikelihood(Cart::ExamplePtrList::const_iterator begin, Cart::ExamplePtrList::const_iterator end) const;
        Cart::Score operator()(const Cart::ExamplePtrRange& leftExamples, const Cart::ExamplePtrRange& rightExamples, const Cart::Score fatherLogLikelihood,
                               Cart::Score& leftChildLogLikelihood, Cart::Score& rightChildLogLikelihood) const;
        void        operator()(const Cart::ExamplePtrRange& examples, Cart::Score& score) const;
    };
};
}  // namespace Speech
using namespace Speech;
// ---- reference text: FeatureAccumulator::processAlignedFeature ----
%(accumulate)s
// ---- reference text: PI ----
%(pi)s
// ---- reference text: LogLikelihoodGain::logLikelihood ----
%(log_likelihood)s
// ---- reference text: LogLikelihoodGain::operator() ----
%(gain)s
// ---- this generator's own driver (no reference text) ----
// The corpus in order into the reference's examples; acc [n_labels x (1 + 2 dim)], rows of labels never seen stay 0.
extern "C" void ref_cart_accumulate(int T, int dim, const float* feats, const int* labels, const double* weights, int n_labels, double* acc) {
    Core::Configuration c{0.0};
    FeatureAccumulator  a(c);
    Feature             f;
    f.v.resize(dim);
    for (int t = 0; t < T; ++t) {
        if (labels[t] < 0)
            continue;   // the aligners' "no label": the frame is not handed over
        for (int d = 0; d < dim; ++d)
            f.v[d] = feats[(size_t)t * dim + d];
        if (weights)
            a.processAlignedFeature(Core::Ref<const Feature>(&f), labels[t], weights[t]);
        else
            a.processAlignedFeature(Core::Ref<const Feature>(&f), labels[t]);
    }
    for (size_t id = 0; id < a.examples_.size() && id < (size_t)n_labels; ++id) {
        if (!a.examples_[id])
            continue;
        const Cart::Example& e = *a.examples_[id];
        double*              r = acc + id * (1 + 2 * (size_t)dim);
        r[0]                   = e.nObs;
        for (int d = 0; d < dim; ++d)
            r[1 + d] = e.values->row(0).begin()[d], r[1 + dim + d] = e.values->row(1).begin()[d];
    }
}

static void walk(const DecisionTree& tree, const DecisionTree::Node* n, long long depth, long long* node_i, double* node_f) {
    const u32  o = n->info_->order;
    long long* r = node_i + (size_t)o * 7;
    r[4] = depth, r[5] = n->info_->nObs;
    node_f[o] = n->info_->score;
    if (n->left_ && n->right_) {
        const Question* q = (*tree.questions)[n->id_];
        r[0] = q->step, r[1] = q->row, r[2] = n->left_->info_->order, r[3] = n->right_->info_->order, r[6] = -1;
        walk(tree, n->left_, depth + 1, node_i, node_f);
        walk(tree, n->right_, depth + 1, node_i, node_f);
    }
    else
        r[0] = r[1] = r[2] = r[3] = -1, r[6] = n->id_;
}

// One training.  steps: per step action (0 split, 1 partition, 2 cluster), min_obs, n_questions in step_i [n_steps x 3], min_gain in step_f,
// the rows of `answers` concatenated in step_q.  Outputs: scalars_i [6] = nodes, leaves, commits, question statistics, nObs, errors;
// scalars_f [2] = initial score, total gain; node_i [nodes x 7] = step, row, left, right, depth, nObs, class (in `order`); node_f [nodes];
// classes [E]; log_i [commits x 4] = node, step, row, depth; log_f [commits x 2] = gain, total gain; qs_i [n x 6] = step, row, count,
// min / sum / max depth; qs_f [n x 3] = min / sum / max gain.
extern "C" void ref_cart_train(int E, int dim, const double* n_obs, const double* values, int Q, const u32* answers, int n_steps, const long long* step_i,
                               const double* step_f, const int* step_q, unsigned max_leaves, double clip, long long* scalars_i, double* scalars_f,
                               long long* node_i, double* node_f, int* classes, long long* log_i, double* log_f, long long* qs_i, double* qs_f) {
    const size_t        words = ((size_t)E + 31) / 32;
    Core::Configuration c{clip};
    g_events.clear();
    g_errors = g_warnings = 0;
    Cart::PropertyMap map;
    Cart::ExampleList examples;
    examples.setMap(Cart::PropertyMapRef(&map));
    for (int e = 0; e < E; ++e) {
        Cart::Example* x = new Cart::Example(new Cart::Properties((u32)e), new Cart::FloatBox(2, dim));
        x->nObs          = n_obs[e];
        for (int d = 0; d < dim; ++d)
            x->values->row(0).begin()[d] = values[(size_t)e * 2 * dim + d], x->values->row(1).begin()[d] = values[(size_t)e * 2 * dim + dim + d];
        examples.push_back(Cart::ExampleRef(x));
    }
    Cart::DecisionTreeTrainer::TrainingPlan plan;
    plan.map = Cart::PropertyMapRef(&map), plan.maxLeaves = max_leaves;
    std::deque<Cart::Question> questions;
    const int*                 q = step_q;
    for (int s = 0; s < n_steps; ++s) {
        Cart::DecisionTreeTrainer::TrainingPlan::Step* st = new Cart::DecisionTreeTrainer::TrainingPlan::Step;
        st->action = step_i[3 * s] == 0 ? "split" : step_i[3 * s] == 1 ? "partition" : "cluster";
        st->minObs = (u32)step_i[3 * s + 1], st->minGain = step_f[s], st->nRandomQuestion = 1;
        st->questionRefs = new Cart::QuestionRefList;
        for (long long k = 0; k < step_i[3 * s + 2]; ++k, ++q) {
            questions.push_back(Cart::Question{answers + (size_t)*q * words, s, *q, (int)questions.size()});
            st->questionRefs->push_back(&questions.back());
        }
        plan.steps.push_back(st);
    }
    StateTyingDecisionTreeTrainer::LogLikelihoodGain scorer(c);
    Cart::DecisionTree                               tree;
    Cart::Training                                   training(c, scorer, plan, examples, &tree);
    Cart::ClusterList*                               clusters = training.train();
    scalars_i[0] = training.nNumber_, scalars_i[1] = training.nLeaf_, scalars_i[4] = training.nObs_, scalars_i[5] = g_errors;
    scalars_f[0] = training.score_, scalars_f[1] = training.gain_;
    walk(tree, tree.root, 0, node_i, node_f);
    for (int e = 0; e < E; ++e)
        classes[e] = -1;
    for (size_t k = 0; k < clusters->size(); ++k)
        for (const Cart::ExampleRef& r : *(*clusters)[k]->exampleRefs)
            classes[r->properties->index] = (int)(*clusters)[k]->node->id_;
    long long n_log = 0;
    for (size_t i = 0; i < g_events.size(); ++i) {
        if (g_events[i].kind != 0 || g_events[i].name != "split")
            continue;
        long long* li    = log_i + 4 * n_log;
        double*    lf    = log_f + 2 * n_log;
        bool       order = false;
        li[0] = li[1] = li[2] = li[3] = -1;
        for (size_t j = i + 1; j < g_events.size(); ++j) {
            const Event& ev = g_events[j];
            if (ev.kind == 1 && ev.name == "depth")
                li[3] = (long long)ev.value;
            else if (ev.kind == 1 && ev.name == "gain")
                lf[0] = ev.value;
            else if (ev.kind == 1 && ev.name == "question-index")
                li[1] = questions[(size_t)ev.value].step, li[2] = questions[(size_t)ev.value].row;
            else if (ev.kind == 2 && ev.name == "order" && !order)
                li[0] = (long long)ev.value, order = true;
            else if (ev.kind == 1 && ev.name == "total-gain") {
                lf[1] = ev.value;
                break;
            }
        }
        ++n_log;
    }
    scalars_i[2] = n_log;
    scalars_i[3] = (long long)training.questionStats_.size();
    for (size_t k = 0; k < training.questionStats_.size(); ++k) {
        const auto& s = training.questionStats_[k];
        qs_i[6 * k] = training.questionRefs_[k]->step, qs_i[6 * k + 1] = training.questionRefs_[k]->row, qs_i[6 * k + 2] = s.count;
        qs_i[6 * k + 3] = s.minDepth, qs_i[6 * k + 4] = s.sumDepth, qs_i[6 * k + 5] = s.maxDepth;
        qs_f[3 * k] = s.minGain, qs_f[3 * k + 1] = s.sumGain, qs_f[3 * k + 2] = s.maxGain;
    }
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-fno-access-control", "-D_GNU_SOURCE", "-DSPRINT_RELEASE_BUILD",
         "-I" + REF, "-I/usr/include/libxml2", "-w"]


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
    gen = os.path.join(tmp, "cart_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "cart_%s.so" % flavour)
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    L.ref_cart_accumulate.restype = None
    L.ref_cart_train.restype = None
    return L, int(fma or 0)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack(answers):
    a = np.asarray(answers, bool)
    q, e = a.shape
    pad = np.zeros((q, (e + 31) // 32 * 32), np.uint8)
    pad[:, :e] = a
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little").view("<u4"))


def ref_train(L, c):
    """the reference's result of a case, in the restatement's form"""
    n_obs, values = np.ascontiguousarray(c["n_obs"], np.float64), np.ascontiguousarray(c["values"], np.float64)
    E, dim = len(n_obs), values.shape[1] // 2
    bits = pack(c["answers"])
    steps = c["steps"]
    step_i = np.array([[cr.ACTIONS[s["action"]], s.get("min_obs", 0), len(s["questions"])] for s in steps], np.int64).reshape(-1, 3)
    step_f = np.array([s.get("min_gain", 0.0) for s in steps], np.float64)
    step_q = np.ascontiguousarray(np.concatenate([np.asarray(s["questions"], np.int32) for s in steps]), np.int32)
    nq, nn = len(step_q), 2 * E + 1
    si, sf = np.zeros(6, np.int64), np.zeros(2)
    node_i, node_f, classes = np.zeros((nn, 7), np.int64), np.zeros(nn), np.zeros(E, np.int32)
    log_i, log_f, qs_i, qs_f = np.zeros((nn, 4), np.int64), np.zeros((nn, 2)), np.zeros((nq, 6), np.int64), np.zeros((nq, 3))
    L.ref_cart_train(E, dim, p(n_obs), p(values), len(bits), p(bits), len(steps), p(step_i), p(step_f), p(step_q), C.c_uint(c["max_leaves"]),
                     C.c_double(c["variance_clipping"]), p(si), p(sf), p(node_i), p(node_f), p(classes), p(log_i), p(log_f), p(qs_i), p(qs_f))
    n_nodes, n_leaves, n_log, n_qs, total_obs, errors = (int(v) for v in si)
    nodes = [dict(step=int(r[0]), row=int(r[1]), left=int(r[2]), right=int(r[3]), depth=int(r[4]), n_obs=int(r[5]), class_id=int(r[6]), score=float(s))
             for r, s in zip(node_i[:n_nodes], node_f[:n_nodes])]
    log = [dict(node=int(r[0]), step=int(r[1]), row=int(r[2]), depth=int(r[3]), gain=float(f[0]), total_gain=float(f[1])) for r, f in zip(log_i[:n_log], log_f[:n_log])]
    qs = [dict(step=int(r[0]), row=int(r[1]), count=int(r[2]), min_depth=int(r[3]), sum_depth=int(r[4]), max_depth=int(r[5]), min_gain=float(f[0]),
               sum_gain=float(f[1]), max_gain=float(f[2])) for r, f in zip(qs_i[:n_qs], qs_f[:n_qs])]
    return dict(nodes=nodes, classes=classes, log=log, question_stats=qs, n_obs=total_obs, initial_score=float(sf[0]), total_gain=float(sf[1]),
                errors=errors, n_leaves=n_leaves)


def same(a, b):
    return cr.discrete(a) == cr.discrete(b) and a["n_leaves"] == b["n_leaves"] and cr.floats(a).tobytes() == cr.floats(b).tobytes()


def acc_cases():
    """name -> (feats, labels, weights, n_labels)"""
    out = {}
    for name, seed, T, dim, weights in (("acc_plain", 1, 300, 5, False), ("acc_weights", 2, 700, 13, True), ("acc_d40", 3, 257, 40, True)):
        rng = np.random.Generator(np.random.PCG64(seed))
        x = (rng.standard_normal((T, dim)) * 3 + 1).astype(np.float32)
        lab = rng.integers(0, 7, T).astype(np.int32)
        lab[lab == 2] = 5
        lab[rng.random(T) < 0.05] = -1
        w = None
        if weights:
            w = rng.uniform(0.01, 2.0, T)
            w[rng.random(T) < 0.05] = 0.0
        out[name] = (x, lab, w, 8)
    return out


def ref_accumulate(L, x, lab, w, n_labels):
    acc = np.zeros((n_labels, 1 + 2 * x.shape[1]))
    L.ref_cart_accumulate(len(lab), x.shape[1], p(x), p(lab), p(w) if w is not None else None, n_labels, p(acc))
    return acc


def write_npz(path, arrays):
    """numpy.savez_compressed with fixed member times: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def store(arrays, prefix, r):
    """a result as arrays (tests/test_cart.py's load() reads them back)"""
    n = r["nodes"]
    arrays[prefix + "node_i"] = np.array([[v[k] for k in ("step", "row", "left", "right", "depth", "n_obs", "class_id")] for v in n], np.int64).reshape(-1, 7)
    arrays[prefix + "node_score"] = np.array([v["score"] for v in n], np.float64)
    arrays[prefix + "classes"] = np.asarray(r["classes"], np.int32)
    arrays[prefix + "log_i"] = np.array([[v[k] for k in ("node", "step", "row", "depth")] for v in r["log"]], np.int64).reshape(-1, 4)
    arrays[prefix + "log_f"] = np.array([[v["gain"], v["total_gain"]] for v in r["log"]], np.float64).reshape(-1, 2)
    q = r["question_stats"]
    arrays[prefix + "qs_i"] = np.array([[v[k] for k in ("step", "row", "count", "min_depth", "sum_depth", "max_depth")] for v in q], np.int64).reshape(-1, 6)
    arrays[prefix + "qs_f"] = np.array([[v["min_gain"], v["sum_gain"], v["max_gain"]] for v in q], np.float64).reshape(-1, 3)
    arrays[prefix + "scalars_i"] = np.array([r["n_obs"], r["errors"], r["n_leaves"]], np.int64)
    arrays[prefix + "scalars_f"] = np.array([r["initial_score"], r["total_gain"]], np.float64)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_cart.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_cart_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    cases, accs = cr.cases(), acc_cases()
    arrays = {}
    for name, c in cases.items():
        k = "in/%s/" % name
        arrays[k + "n_obs"], arrays[k + "values"], arrays[k + "answers"] = c["n_obs"], c["values"], pack(c["answers"])
        arrays[k + "plan"] = np.array([c["max_leaves"], c["variance_clipping"]], np.float64)
        arrays[k + "step_i"] = np.array([[cr.ACTIONS[s["action"]], s.get("min_obs", 0), len(s["questions"])] for s in c["steps"]], np.int64)
        arrays[k + "step_f"] = np.array([s.get("min_gain", 0.0) for s in c["steps"]], np.float64)
        arrays[k + "step_q"] = np.concatenate([np.asarray(s["questions"], np.int32) for s in c["steps"]])
    for name, (x, lab, w, n_labels) in accs.items():
        k = "in/%s/" % name
        arrays[k + "feats"], arrays[k + "labels"], arrays[k + "n_labels"] = x, lab, np.array(n_labels)
        if w is not None:
            arrays[k + "weights"] = w
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for fl in ("off", "fma"):
            L, n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)
            for name, c in cases.items():
                got[fl, name] = ref_train(L, c)
            for name, a in accs.items():
                got[fl, name] = ref_accumulate(L, *a)
    # the restatement without fused sites is the -msse3 build, in every bit
    rest = {}
    for fl in ("off", "fma"):
        for name, c in cases.items():
            rest[fl, name] = cr.train(contract=fl, **c)
            assert same(rest[fl, name], got[fl, name]), "the restatement (contract=%s) differs from the reference in case %s" % (fl, name)
        for name, (x, lab, w, n_labels) in accs.items():
            r = cr.accumulate(cr.accumulator(n_labels, x.shape[1]), x, lab, w, contract=fl)
            assert r.tobytes() == got[fl, name].tobytes(), "the restated accumulation (contract=%s) differs from the reference in case %s" % (fl, name)
    # which sites the native build fuses
    keys = ("variance", "constant")
    fits = []
    for combo in itertools.product((False, True), repeat=2):
        sites = dict(cr.FMA_SITES, **dict(zip(keys, combo)))
        if all(same(cr.train(contract="fma", sites=sites, **c), got["fma", n]) for n, c in cases.items() if len(c["n_obs"]) <= 200):
            fits.append(",".join("%s=%d" % kv for kv in zip(keys, combo)))
    want = ",".join("%s=%d" % (k, cr.FMA_SITES[k]) for k in keys)
    assert fits == [want], "fused forms of the scorer that reproduce the -march=native build: %s" % fits
    akeys = ("sum", "sum_sq")
    afits = []
    for combo in itertools.product((False, True), repeat=2):
        sites = dict(cr.FMA_SITES, **dict(zip(akeys, combo)))
        if all(cr.accumulate(cr.accumulator(a[3], a[0].shape[1]), a[0], a[1], a[2], contract="fma", sites=sites).tobytes() == got["fma", n].tobytes()
               for n, a in accs.items()):
            afits.append(",".join("%s=%d" % kv for kv in zip(akeys, combo)))
    awant = ",".join("%s=%d" % (k, cr.FMA_SITES[k]) for k in akeys)
    assert afits == [awant], "fused forms of the accumulation that reproduce the -march=native build: %s" % afits
    arrays["fma_sites"] = np.array([want, awant])
    differ = []
    for name in list(cases) + list(accs):
        if name in cases:
            store(arrays, "off/%s/" % name, got["off", name])
            if not same(got["off", name], got["fma", name]):
                store(arrays, "fma/%s/" % name, got["fma", name])
                differ.append(name)
        else:
            arrays["off/%s/acc" % name] = got["off", name]
            if got["off", name].tobytes() != got["fma", name].tobytes():
                arrays["fma/%s/acc" % name] = got["fma", name]
                differ.append(name)
    arrays["fma_differs"] = np.array(differ or [""])
    undecided = []
    for name in cases:
        gaps = [rest[fl, name]["decided_gap"] for fl in ("off", "fma")]
        arrays["decided_gap/" + name] = np.array(gaps, np.float64)
        arrays["decided/" + name] = np.array([g > 1.0 and not cr.is_tie(name) for g in gaps])
        for fl in ("off", "fma"):
            arrays["score_bar/%s/%s" % (fl, name)] = np.array([n["bar"] for n in rest[fl, name]["nodes"]], np.float64)
        if not (gaps[0] > 1.0 and gaps[1] > 1.0):
            undecided.append(name)
    assert all(cr.is_tie(n) for n in undecided), "cases that are not decided: %s" % undecided
    for defect, name in cr.PLANTED.items():
        assert not same(cr.train(defect=defect, **cases[name]), got["off", name]), "the planted defect %s does not leave case %s" % (defect, name)
    arrays["cases"] = np.array(list(cases))
    arrays["acc_cases"] = np.array(list(accs))
    write_npz(out, arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    print("  fma instructions: off %d, fma %d" % (int(arrays["fma_instructions/off"]), int(arrays["fma_instructions/fma"])))
    print("  cases the native build computes differently: %s" % differ)
    print("  fused sites of the native build: %s; %s" % (want, awant))
    print("  smallest decided_gap of a case not named tie_*: %.3g bars" % min(min(arrays["decided_gap/" + n]) for n in cases if not cr.is_tie(n)))
    print("  negative-gain errors: %s" % {n: got["off", n]["errors"] for n in cases if got["off", n]["errors"]})


if __name__ == "__main__":
    main()
