#!/usr/bin/env python3
"""tests/golden/make_bayes_golden.py -- writes tests/golden/ref_bayes.npz: the decisions of the `signal-bayes-classification` node and the
vectors of `signal-bayes-classification-score` as the reference's own text computes them.

Run it where the reference tree is mounted; tests read only the fixture.  What it compiles, in both of the reference's arithmetics (the
flag sets of oracle/ref/Makefile: -msse3 = contract=off, -msse3 -march=native = contract=fma), taken by line range + SHA-256 into a
temporary directory that is deleted afterwards:
  * Signal/SlidingWindow.hh:20-471 (everything between the two Flow includes and the include guard's end)
  * Signal/AprioriProbability.hh:22-53 and AprioriProbability.cc:19-27 (the classes; setClasses with std::log((f32)n), operator[])
  * Signal/LikelihoodFunction.hh:26-63, 74-108 (the classes, sumOfWeights_) and LikelihoodFunction.cc:32-45, 61-83 (setClasses, reset, feed)
  * Signal/BayesClassification.hh:36-151 (the class) and BayesClassification.cc:23-161, 182-202, 216-273 (constructor, init, feed,
    updateTimes, both classify, both getScores, argMin, reset, setClassLabels(u32), the setters, needMoreFeatureVectors,
    setUseSlidingWindow)
behind a shell of this file's own that holds no reference text: Core::Component / Configuration / XmlChannel / Statistics / Ref stand-ins,
Flow::Vector / String / Timestamp / DataPtr stand-ins, and an Mm::FeatureScorer stand-in whose score(c) returns element c of the matrix
row the driver hands in.  The statistics channel stand-in reports OPEN: that is how argMin's per-class scores are recorded (the
Core::Statistics stand-in's operator+= keeps each `score` argMin adds to it); writeStatistics is an empty function.

The driver replays the two nodes' work loops (BayesClassification.cc:384-411 and :429-444) frame by frame and records after which frame
a label or a vector left, the label or vector at the end of the stream, argMin's per-class scores for each label and sumOfWeights().
No recorded case has a label without a winner (the reference indexes classLabels_ out of range there).

Cases: n_classes 3 and 13; segments of 0, 1, 2, 40 and 300 frames; segment mode, first 16 frames, continuous with delay 0 and 5, windows
(L, delay) = (4, max), (25, max), (4, 0), (4, 3), (25, 7), window-right 1 in the first; the score node with delay 0 and 3, with and
without single-frame-classification; each without weights, with weights in [0, 2] (one of them 0) and with all weights 1.

Finding (printed by every run, kept in the fixture as fma_differs): the contract=fma build gives the same bits as contract=off in every
recorded array.  The product `featureScoreWeight * scorer->score(c)` of LikelihoodFunction.cc:77 is stored into currentScores as well as
added, so GCC does not contract it into the addition; the -march=native object holds no fused multiply-add.  The fma/ copies are kept only
where bits differ: nowhere.

    python3 tests/golden/make_bayes_golden.py [out.npz]
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"

PIECES = {
    "sliding_window": [("Signal/SlidingWindow.hh", 20, 471)],
    "apriori_hh": [("Signal/AprioriProbability.hh", 22, 53)],
    "apriori_cc": [("Signal/AprioriProbability.cc", 19, 27)],
    "likelihood_hh": [("Signal/LikelihoodFunction.hh", 26, 63), ("Signal/LikelihoodFunction.hh", 74, 108)],
    "likelihood_cc": [("Signal/LikelihoodFunction.cc", 32, 45), ("Signal/LikelihoodFunction.cc", 61, 83)],
    "bayes_hh": [("Signal/BayesClassification.hh", 36, 151)],
    "bayes_cc": [("Signal/BayesClassification.cc", 23, 161), ("Signal/BayesClassification.cc", 182, 202), ("Signal/BayesClassification.cc", 216, 273)],
}
SHA = "92ed56f42a793d4cacedd2e1a18695930fb974687e5c685b8fea7fddf995e18a"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/Types.hh>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>
// ---- shell: stand-ins (no reference text) ----
static std::vector<f32> g_argmin_scores;   // what argMin added to its statistics, in class order
static const f32*       g_row = 0;         // the score matrix row of the frame being fed
static u32              g_n_mixtures = 0;
namespace Core {
struct Configuration {};
class Component {
public:
    Component(const Configuration&) {}
    virtual ~Component() {}
    void error(const char* fmt, ...) const {
        va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr);
    }
    void criticalError(const char* fmt, ...) const {
        va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); abort();
    }
    void respondToDelayedErrors() const { abort(); }
    Configuration        select(const std::string&) const { return Configuration(); }
    const Configuration& getConfiguration() const { static Configuration c; return c; }
    std::string          name() const { return "bayes"; }
    std::string          fullName() const { return "bayes"; }
};
class XmlWriter {};
class XmlChannel : public XmlWriter {
public:
    XmlChannel(const Configuration&, const std::string&) {}
    bool isOpen() const { return true; }
};
template<class T> class Statistics {
public:
    Statistics(const char*) {}
    void operator+=(T v) { g_argmin_scores.push_back(v); }
};
template<class T> class Ref {
public:
    std::shared_ptr<T> p;
    Ref() {}
    explicit Ref(T* q) : p(q) {}
    template<class U> Ref(const Ref<U>& o) : p(o.p) {}
    T*   operator->() const { return p.get(); }
    bool operator==(int) const { return !p; }
    bool operator!=(int) const { return (bool)p; }
};
}  // namespace Core
namespace Flow {
typedef f64 Time;
class Timestamp {
    Time start_, end_;
public:
    Timestamp() : start_(0), end_(0) {}
    Time startTime() const { return start_; }
    Time endTime() const { return end_; }
    void setStartTime(Time t) { start_ = t; }
    void setEndTime(Time t) { end_ = t; }
};
class Data {
public:
    virtual ~Data() {}
};
template<class T> class Vector : public Data, public Timestamp, public std::vector<T> {};
class String : public Data, public Timestamp {
    std::string s_;
public:
    std::string& operator()() { return s_; }
};
template<class T> class DataPtr {
    T* p_;
public:
    DataPtr() : p_(0) {}
    DataPtr(T* p) : p_(p) {}
    template<class U> DataPtr(const DataPtr<U>& o) : p_((T*)o.get()) {}
    T* get() const { return p_; }
    T* operator->() const { return p_; }
};
}  // namespace Flow
namespace Mm {
class Feature {
public:
    Feature(const std::vector<f32>&) {}
};
class FeatureScorer {
public:
    class ContextScorer {
    public:
        virtual ~ContextScorer() {}
        virtual f32 score(u32 c) const = 0;
    };
    typedef Core::Ref<const ContextScorer> Scorer;
    virtual ~FeatureScorer() {}
    virtual Scorer getScorer(Core::Ref<const Feature>) const;
    virtual u32    nMixtures() const { return g_n_mixtures; }
};
class RowScorer : public FeatureScorer::ContextScorer {
    const f32* row_;
public:
    RowScorer(const f32* row) : row_(row) {}
    virtual f32 score(u32 c) const;
};
__attribute__((noinline)) f32 RowScorer::score(u32 c) const { return row_[c]; }
FeatureScorer::Scorer FeatureScorer::getScorer(Core::Ref<const Feature>) const { return Scorer(new RowScorer(g_row)); }
}  // namespace Mm
// ---- reference text: SlidingWindow (opens and closes namespace Signal itself) ----
%(sliding_window)s
namespace Signal {
// ---- reference text: AprioriProbability, UniformAprioriProbability ----
%(apriori_hh)s
// ---- reference text: LikelihoodFunction, IndependentSequenceLikelihood ----
%(likelihood_hh)s
// ---- reference text: BayesClassification ----
%(bayes_hh)s
}  // namespace Signal
using namespace Signal;
// ---- reference text: AprioriProbability.cc ----
%(apriori_cc)s
// ---- shell: what LikelihoodFunction.cc:24-30 and :47-59 ask the Mm module for
IndependentSequenceLikelihood::IndependentSequenceLikelihood(const Core::Configuration& c)
        : Component(c), Precursor(c) {
    logLikelihoodFunctions_ = Core::Ref<Mm::FeatureScorer>(new Mm::FeatureScorer);
}
bool IndependentSequenceLikelihood::setDimension(size_t) { return true; }
// ---- reference text: LikelihoodFunction.cc ----
%(likelihood_cc)s
// ---- shell: BayesClassification.cc:163-180 writes XML
void BayesClassification::writeStatistics(Core::XmlWriter&, u32, const Core::Statistics<Score>&) const {}
// ---- reference text: BayesClassification.cc ----
%(bayes_cc)s
// ---- this generator's own driver (no reference text) ----
namespace {
struct Node {
    BayesClassification b;
    Core::Configuration c;
    // BayesClassificationNode's constructor (BayesClassification.cc:305-316) and configure() (:318-319)
    Node(int n_classes, long number_of_features, long delay, int window_length, int window_right)
            : b(c) {
        g_n_mixtures = n_classes;
        b.classLabels_.resize(n_classes);
        for (int i = 0; i < n_classes; ++i)
            b.classLabels_[i] = std::to_string(i);
        b.needInit_ = true;
        b.setAprioriProbability(BayesClassification::Uniform);
        b.setLikelihoodFunction(BayesClassification::IndependentSequence);
        b.setDelay((u32)delay);
        b.setNumUsedFeatures((u32)number_of_features);
        b.setUseSlidingWindow(window_length > 0, window_length, window_right);
        b.reset();
    }
};
void take_scores(float* dst, int n_classes) {
    if ((int)g_argmin_scores.size() != n_classes)
        abort();
    std::copy(g_argmin_scores.begin(), g_argmin_scores.end(), dst);
}
}  // namespace
// BayesClassificationNode::work (:384-411), called until the end of the stream has been passed on.
// frame_label[t] / frame_scores[t]: what left after frame t (-1 / untouched: nothing); eos_*: what left at the end of the stream.
extern "C" int by_classify(int n_classes, long number_of_features, long delay, int window_length, int window_right, int T, const float* scores,
                           const float* weights, int* frame_label, float* frame_scores, int* eos_label, float* eos_scores, float* sum_of_weights,
                           int* frames_fed) {
    Node n(n_classes, number_of_features, delay, window_length, window_right);
    BayesClassification& b = n.b;
    Flow::Vector<f32> fv;
    fv.resize(1);
    int  i    = 0;
    bool done = false;
    *eos_label = -1;
    for (int t = 0; t < T; ++t)
        frame_label[t] = -1;
    while (!done) {
        Flow::String label;
        bool         got = false;
        do {
            if (i >= T) {   // getData fails: end of stream
                g_argmin_scores.clear();
                if (b.classify(label)) {
                    *eos_label = atoi(label().c_str());
                    take_scores(eos_scores, n_classes);
                }
                done = true;
                break;
            }
            g_row = scores + (size_t)i * n_classes;
            const float w = weights ? weights[i] : 1.0f;   // featureScoreWeight(): 1 without the second input
            fv.setStartTime(i);
            fv.setEndTime(i + 1);
            ++i;
            g_argmin_scores.clear();
            got = b.classify(label, fv, w);
        } while (!got);
        if (done)
            break;
        frame_label[i - 1] = atoi(label().c_str());
        take_scores(frame_scores + (size_t)(i - 1) * n_classes, n_classes);
        if (!b.needMoreFeatureVectors()) {   // the rest of the stream is read, not scored; the label and the end of stream leave together
            *frames_fed = i;
            i           = T;
            done        = true;
            *sum_of_weights = b.likelihoodFunction_->sumOfWeights();
            return 0;
        }
    }
    *frames_fed     = i;
    *sum_of_weights = b.likelihoodFunction_ ? b.likelihoodFunction_->sumOfWeights() : 0.f;
    return 0;
}
// BayesClassificationScoreNode::work (:429-444).  emitted[t] = 1: out[t] left after frame t; *eos = 1: eos_out left at the end of stream
extern "C" int by_scores(int n_classes, long delay, int single_frame, int T, const float* scores, const float* weights, float* out,
                         unsigned char* emitted, int* eos, float* eos_out) {
    Node n(n_classes, 0x7fffffffL, delay, -1, 0);
    BayesClassification& b = n.b;
    Flow::Vector<f32> fv;
    fv.resize(1);
    int  i    = 0;
    bool done = false;
    *eos      = 0;
    for (int t = 0; t < T; ++t)
        emitted[t] = 0;
    while (!done) {
        Flow::Vector<f32> v;
        bool              classified = false;
        do {
            if (i >= T) {
                if (b.getScores(v)) {
                    *eos = 1;
                    std::copy(v.begin(), v.end(), eos_out);
                }
                done = true;
                break;
            }
            g_row = scores + (size_t)i * n_classes;
            const float w = weights ? weights[i] : 1.0f;
            ++i;
            classified = b.getScores(v, fv, w);
            if (classified && single_frame)
                b.reset();
        } while (!classified);
        if (done)
            break;
        emitted[i - 1] = 1;
        std::copy(v.begin(), v.end(), out + (size_t)(i - 1) * n_classes);
    }
    return 0;
}
extern "C" float by_prior(int n_classes) {
    Core::Configuration       c;
    UniformAprioriProbability p(c);
    std::vector<std::string>  labels(n_classes);
    p.setClasses(labels);
    return p[0];
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-fno-access-control", "-D_GNU_SOURCE",
         "-DSPRINT_RELEASE_BUILD", "-I" + REF, "-I/usr/include/libxml2", "-w"]
INT_MAX = 2 ** 31 - 1
N_CLASSES = (3, 13)
LENGTHS = (0, 1, 2, 40, 300)
# name -> (number_of_features, delay, window_length, window_right)
CLASSIFY = {
    "segment": (INT_MAX, INT_MAX, -1, 0),
    "first16": (16, INT_MAX, -1, 0),
    "continuous0": (INT_MAX, 0, -1, 0),
    "continuous5": (INT_MAX, 5, -1, 0),
    "window4": (INT_MAX, INT_MAX, 4, 1),
    "window25": (INT_MAX, INT_MAX, 25, 0),
    "window4_d0": (INT_MAX, 0, 4, 0),
    "window4_d3": (INT_MAX, 3, 4, 0),
    "window25_d7": (INT_MAX, 7, 25, 0),
}
# name -> (delay, single_frame)
SCORES = {"scores_d0": (0, 0), "scores_d3": (3, 0), "single_d0": (0, 1), "single_d3": (3, 1)}
WEIGHTS = ("none", "random", "ones")


def inputs(n_classes, T):
    """scores f32 [T, n_classes] of mixed magnitude (N(50, 30), a few values near 1e4), weights in [0, 2] with one 0"""
    rng = np.random.Generator(np.random.PCG64(1000 * n_classes + T))
    s = rng.normal(50.0, 30.0, (T, n_classes)).astype(np.float32)
    if T:
        hit = rng.random((T, n_classes)) < 0.03
        s[hit] = (1e4 + rng.normal(0.0, 50.0, (T, n_classes))).astype(np.float32)[hit]
    w = (rng.random(T) * 2.0).astype(np.float32)
    if T > 1:
        w[T // 2] = 0.0
    return s, w


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
    gen = os.path.join(tmp, "bayes_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "bayes_%s.so" % flavour)
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
    u8p = np.ctypeslib.ndpointer(np.uint8, flags="C")
    L.by_classify.restype = C.c_int
    L.by_classify.argtypes = [C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p, i32p, f32p, C.POINTER(C.c_int), f32p,
                              C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.by_scores.restype = C.c_int
    L.by_scores.argtypes = [C.c_int, C.c_long, C.c_int, C.c_int, f32p, C.c_void_p, f32p, u8p, C.POINTER(C.c_int), f32p]
    L.by_prior.restype = C.c_float
    L.by_prior.argtypes = [C.c_int]
    return L, int(fma or 0)


def weights_of(kind, w):
    return {"none": None, "random": w, "ones": np.ones_like(w)}[kind]


def run(L):
    """every recorded array of one build; the segments of LENGTHS lie one after the other along the first axis (offsets np.cumsum)"""
    a = {}
    ones_equal = True
    for nc in N_CLASSES:
        a["prior/%d" % nc] = np.float32(L.by_prior(nc))
        rec = {}
        for T in LENGTHS:
            s, w = inputs(nc, T)
            s = np.ascontiguousarray(s)
            for wk in WEIGHTS:
                wv = weights_of(wk, w)
                wp = wv.ctypes.data if wv is not None else None
                for name, (nof, delay, wl, wr) in CLASSIFY.items():
                    fl = np.zeros(T, np.int32)
                    fs = np.full((T, nc), np.nan, np.float32)
                    el, fed, sw = C.c_int(), C.c_int(), C.c_float()
                    es = np.full((1, nc), np.nan, np.float32)
                    assert L.by_classify(nc, nof, delay, wl, wr, T, s, wp, fl, fs, C.byref(el), es, C.byref(sw), C.byref(fed)) == 0
                    rec.setdefault("c/%d/%s/%s" % (nc, wk, name), []).append(
                        {"frame_label": fl, "frame_scores": fs, "eos_label": np.array([el.value], np.int32), "eos_scores": es,
                         "sum_of_weights": np.array([sw.value], np.float32), "frames_fed": np.array([fed.value], np.int32)})
                for name, (delay, single) in SCORES.items():
                    out = np.full((T, nc), np.nan, np.float32)
                    em = np.zeros(T, np.uint8)
                    eos = C.c_int()
                    eo = np.full((1, nc), np.nan, np.float32)
                    assert L.by_scores(nc, delay, single, T, s, wp, out, em, C.byref(eos), eo) == 0
                    rec.setdefault("s/%d/%s/%s" % (nc, wk, name), []).append(
                        {"out": out, "emitted": em, "eos": np.array([eos.value], np.int32), "eos_out": eo})
        for k, parts in rec.items():
            for field in parts[0]:
                a[k + "/" + field] = np.concatenate([p[field] for p in parts])
    # all weights 1 must be what no weight stream gives; only the verdict is kept
    for k in [k for k in a if "/ones/" in k]:
        ones_equal = ones_equal and same_bits(a[k], a[k.replace("/ones/", "/none/")])
        del a[k]
    a["ones_equal_none"] = np.array(ones_equal)
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_bayes.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_bayes_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    arrays = {}
    for nc in N_CLASSES:
        for T in LENGTHS:
            arrays["in/%d/%d/scores" % (nc, T)], arrays["in/%d/%d/weights" % (nc, T)] = inputs(nc, T)
    for name, cfg in CLASSIFY.items():
        arrays["cfg/classify/" + name] = np.array(cfg, np.int64)
    for name, cfg in SCORES.items():
        arrays["cfg/scores/" + name] = np.array(cfg, np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        got = {}
        for fl in ("off", "fma"):
            L, n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)   # fused multiply-adds in the generated object (objdump)
            got[fl] = run(L)
    for k, v in got["off"].items():
        arrays["off/" + k] = v
    differ = [k for k, v in got["fma"].items() if not same_bits(v, got["off"][k])]
    for k in differ:
        arrays["fma/" + k] = got["fma"][k]
    arrays["fma_differs"] = np.array(differ if differ else [""])
    arrays["fma_arrays_compared"] = np.array(len(got["fma"]))
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    print("  fma instructions: off %d, fma %d" % (int(arrays["fma_instructions/off"]), int(arrays["fma_instructions/fma"])))
    print("  fma copies that differ from off: %d of %d %s" % (len(differ), len(got["fma"]), differ[:8]))


if __name__ == "__main__":
    main()
