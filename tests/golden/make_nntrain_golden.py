#!/usr/bin/env python3
"""tests/golden/make_nntrain_golden.py -- writes tests/golden/ref_nntrain.npz: what the tests of the NN training statistics read.

Run it where the reference tree is mounted; tests read only the fixture.  Three parts.

1. The element-wise functions of the pass as the reference's own text computes them.  The member functions of Math::FastMatrix<T> are
   taken from Math/FastMatrix.hh by line range + SHA-256 into a temporary directory and compiled (g++ -O2 -ffp-contract=off) behind a
   shell of stand-ins that holds no reference text: the data members and accessors of FastMatrix / FastVector, require_* as no-ops,
   Core::Type<f32>::min / max as the IEEE values, Core::Application::us()->warning as a no-op.  Nothing of it is committed.
     argMax 898-911, sigmoid / tanh / rectified derivative 1018-1034 and 1049-1057, addKroneckerDelta 1059-1070,
     nClassificationErrors 1087-1101, crossEntropyObjectiveFunction and its weighted form 1103-1130, clip 1305-1311
   Recorded on random and edge inputs: ties, exact zeros, +-0, NaN, +-max, and the random values, among which the generator counts (and
   asserts to be present) those whose double product rounds differently from an f32 one.

2. Prior, finalize and the file, as the reference's own text computes them.  Nn/Prior.cc:127-156 (setFromClassCounts),
   Nn/Statistics.cc:145-173 (finalize), 344-389 (write), 583-604 (writeHeader, getMagic) and Nn/NeuralNetworkTrainer.cc:446-462
   (writeMeanAndStandardDeviation), by line range + SHA-256, compiled with the flags of oracle/ref/Makefile against the reference's own
   headers by include path (Core::BinaryOutputStream, Math::Vector and Math::Matrix with their write(), Core::Type) and linked with
   oracle/_ref/libref.so, which holds the reference's Core/BinaryStream.cc (run the build first).  Stand-ins without reference text: the
   members of Statistics, Prior and MeanAndVarianceTrainer; the device vector / matrix as far as the text uses it (scale = BLAS scal,
   add = axpy, element-wise product, convert); Math::copy; log / warning / the statistics channel as a closed sink.
   Recorded: the log prior for three back-off counts over counts with zeros and a zero class weight; mean and standard deviation of
   19 components; the bytes Statistics<f32>::write emits for a small object (3-4-2) under each of the 15 flag masks, with the flat
   buffer they came from.

3. The bars.  Every configuration of the GPU tests (tests/nntrain_reference.py: gpu_cases()) is evaluated twice by the restatement: all
   matrix products in f64, and all of them in f32 through sgemm (numpy's OpenBLAS; the reference links a BLAS sgemm for Math::gemm<f32>)
   with the sequential f32 sums of the reference.  Per network and layer, the gradient bar is 4 x the worst deviation of the sgemm
   evaluation from the f64 one, relative to that layer's largest |gradient|; the bias-gradient, feature-sum and objective bars are
   measured the same way.  The factor is 4 because the order of a sum is the reference's free choice and the device's differs from
   both.  Tests read the bars from the fixture; no tolerance is written into a test.
   Four configurations are stored whole (the flat buffers of both evaluations) so that a drift of the restatement shows.
   These whole passes are the RESTATEMENT's, not the reference driver's: Nn/FeedForwardTrainer.cc drives a NeuralNetwork of layer
   objects, a criterion and a statistics object, and compiling that behind stand-ins was not done.  What ties the restatement's pass to
   the reference is part 1 (every element-wise step, bit for bit), part 2, and the finite-difference test of tests/test_nntrain.py.

Condition on the inputs, asserted here: in every configuration every frame's two largest softmax values differ by at least 64 ulp, and
the two evaluations count the same classification errors, so the error count does not depend on the order of a sum.  Exact ties are
planted separately (part 1, and the tests' own tie case).

    python3 tests/golden/make_nntrain_golden.py [out.npz]
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
from tests import nntrain_reference as nr  # noqa: E402

REF = os.environ.get("AMX_REFERENCE", "/root/reference/src")
PIECES = [("Math/FastMatrix.hh", 898, 911), ("Math/FastMatrix.hh", 1018, 1034), ("Math/FastMatrix.hh", 1049, 1070), ("Math/FastMatrix.hh", 1087, 1130),
          ("Math/FastMatrix.hh", 1305, 1311)]
SHA = "09b672597be05a3189f8b262ab7a7e6b96bb27f22e2df74c558b379908058ceb"
WHOLE = ("a-21-T129", "a-32-T300-class_weights+clip+disregard+frame_weights+pre", "b-3-T128-pre", "b-2-T31-class_weights")

SHELL = r'''
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <typeinfo>
#include <vector>
typedef uint32_t u32;
typedef float    f32;
typedef double   f64;
// ---- shell (no reference text): what the member functions below touch ----
namespace Core {
template<class T> struct Type;
template<> struct Type<f32> { static constexpr f32 max = +3.40282347e+38F; static constexpr f32 min = -3.40282347e+38F; };
struct Application { static Application* us() { static Application a; return &a; } void warning(const char*, ...) {} };
}
#define require_eq(a, b) ((void)0)
#define require_lt(a, b) ((void)0)
namespace Math {
template<class T> struct FastVector {
    const T* p; u32 n;
    u32 nRows() const { return n; }
    u32 size() const { return n; }
    const T& operator[](u32 i) const { return p[i]; }
};
template<class T> struct FastMatrix {
    u32 nRows_, nColumns_; T* elem_;
    u32 nRows() const { return nRows_; }
    u32 nColumns() const { return nColumns_; }
    T& at(u32 i, u32 j) { return *(elem_ + j * nRows_ + i); }
    const T& at(u32 i, u32 j) const { return *(elem_ + j * nRows_ + i); }
    u32 argMax(u32 column) const;
    void elementwiseMultiplicationWithSigmoidDerivative(const FastMatrix<T>& X);
    void elementwiseMultiplicationWithTanhDerivative(const FastMatrix<T>& X);
    void elementwiseMultiplicationWithRectifiedDerivative(const FastMatrix<T>& X);
    template<typename S> void addKroneckerDelta(const FastVector<S>& alignment, const T scale);
    template<typename S> u32 nClassificationErrors(const FastVector<S>& alignment);
    template<typename S> T crossEntropyObjectiveFunction(const FastVector<S>& alignment);
    template<typename S> T weightedCrossEntropyObjectiveFunction(const FastVector<S>& alignment, const FastVector<T>& weights);
    void clip(const T maxAbsValue);
};
// ---- reference text ----
%(pieces)s
}  // namespace Math
// ---- shell: the calls, on [frames x units] row-major memory = the reference's column-major [units x frames] ----
typedef Math::FastMatrix<f32> M;
extern "C" {
void ref_argmax(float* p, u32 frames, u32 units, u32* out) { M m{units, frames, p}; for (u32 t = 0; t < frames; ++t) out[t] = m.argMax(t); }
void ref_sigmoid(float* e, float* y, u32 n) { M m{n, 1, e}, x{n, 1, y}; m.elementwiseMultiplicationWithSigmoidDerivative(x); }
void ref_tanh(float* e, float* y, u32 n) { M m{n, 1, e}, x{n, 1, y}; m.elementwiseMultiplicationWithTanhDerivative(x); }
void ref_rectified(float* e, float* y, u32 n) { M m{n, 1, e}, x{n, 1, y}; m.elementwiseMultiplicationWithRectifiedDerivative(x); }
void ref_clip(float* e, u32 n, float c) { M m{n, 1, e}; m.clip(c); }
void ref_kronecker(float* p, u32 frames, u32 units, const u32* label, float scale) { M m{units, frames, p}; m.addKroneckerDelta(Math::FastVector<u32>{label, frames}, scale); }
u32 ref_errors(float* p, u32 frames, u32 units, const u32* label) { M m{units, frames, p}; return m.nClassificationErrors(Math::FastVector<u32>{label, frames}); }
float ref_ce(float* p, u32 frames, u32 units, const u32* label) { M m{units, frames, p}; return m.crossEntropyObjectiveFunction(Math::FastVector<u32>{label, frames}); }
float ref_wce(float* p, u32 frames, u32 units, const u32* label, const float* w) {
    M m{units, frames, p};
    return m.weightedCrossEntropyObjectiveFunction(Math::FastVector<u32>{label, frames}, Math::FastVector<f32>{w, frames});
}
}
'''


def pieces():
    cache, out, h = {}, [], hashlib.sha256()
    for fn, first, last in PIECES:
        if fn not in cache:
            with open(os.path.join(REF, fn), encoding="utf-8", errors="replace") as f:
                cache[fn] = f.readlines()
        out.append("".join(cache[fn][first - 1:last]))
    text = "\n".join(out)
    h.update(text.encode())
    return text, h.hexdigest()


def build(tmp):
    text, sha = pieces()
    if sha != SHA:
        raise SystemExit("make_nntrain_golden: the reference text at the recorded line ranges hashes to %s, not %s" % (sha, SHA))
    src, lib = os.path.join(tmp, "nntrain_ref.cc"), os.path.join(tmp, "libnntrain_ref.so")
    with open(src, "w") as f:
        f.write(SHELL % {"pieces": text})
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-w", "-o", lib, src])
    return C.CDLL(lib)


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


def element_wise(L):
    rng = np.random.Generator(np.random.PCG64(20250))
    f32 = np.float32
    out = {}
    # derivatives: random pairs plus every pair of the edge values
    edge = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 0.25, 1e-30, -1e-30, 3.4028235e38, -3.4028235e38, np.nan, 0.99999994, 1.0000001, 1e-45], f32)
    ee, yy = np.meshgrid(edge, edge)
    e = np.concatenate([rng.standard_normal(4096).astype(f32), ee.ravel()])
    y = np.concatenate([rng.uniform(-1, 1, 4096).astype(f32), yy.ravel()])
    out["ew_e"], out["ew_y"] = e, y
    for name, fn in (("sigmoid", L.ref_sigmoid), ("tanh", L.ref_tanh), ("rectified", L.ref_rectified)):
        r = e.copy()
        yc = y.copy()
        fn(fp(r), fp(yc), C.c_uint32(len(r)))
        out["ew_" + name] = r
    with np.errstate(all="ignore"):
        f32_sig = e * (y * (f32(1) - y))
        f32_tanh = e * (f32(1) - y * y)
    n_sig = int((f32_sig[:4096].view(np.uint32) != out["ew_sigmoid"][:4096].view(np.uint32)).sum())
    n_tanh = int((f32_tanh[:4096].view(np.uint32) != out["ew_tanh"][:4096].view(np.uint32)).sum())
    assert n_sig > 100 and n_tanh > 100, (n_sig, n_tanh)   # the inputs do tell the double product from an f32 one
    out["ew_differs_from_f32"] = np.array([n_sig, n_tanh])
    clips = np.array([0.01, 1.0, 3.4028235e38], f32)
    out["clip_c"] = clips
    for i, c in enumerate(clips):
        r = e.copy()
        L.ref_clip(fp(r), C.c_uint32(len(r)), C.c_float(c))
        out["ew_clip%d" % i] = r
    # criterion: softmax-like rows with planted ties, all-equal rows, rows of -max / -inf / NaN, zeros at the label
    T, n = 64, 37
    p = rng.dirichlet(np.ones(n), T).astype(f32)
    p[0, :] = p[0, 5]                    # all equal: the first wins
    p[1, 7] = p[1, 30] = p[1].max() * 2  # a tie of the two largest: the first wins
    p[2, :] = -3.4028235e38              # nothing is greater than the start value: 0
    p[3, :] = -np.inf
    p[4, :] = np.nan
    p[5, 0] = np.nan                     # a NaN never wins
    p[6, 3] = 0.0                        # label 3 below: log(0)
    p[7, n - 1] = p[7].max() * 2         # the last unit
    label = rng.integers(0, n, T).astype(np.uint32)
    label[0], label[1], label[2], label[6], label[7] = 0, 30, 0, 3, n - 1
    w = rng.uniform(0.25, 2.0, T).astype(f32)
    out["cr_p"], out["cr_label"], out["cr_w"] = p, label, w
    am = np.zeros(T, np.uint32)
    pc = p.copy()
    L.ref_argmax(fp(pc), T, n, fp(am))
    out["cr_argmax"] = am
    L.ref_errors.restype = C.c_uint32
    out["cr_errors"] = np.array([L.ref_errors(fp(pc), T, n, fp(label))], np.uint32)
    k = p.copy()
    L.ref_kronecker(fp(k), T, n, fp(label), C.c_float(-1.0))
    out["cr_kronecker"] = k
    L.ref_ce.restype = L.ref_wce.restype = C.c_float
    fin = np.arange(8, T)                # the finite rows: a sequential f32 objective
    pf, lf, wf = np.ascontiguousarray(p[fin]), np.ascontiguousarray(label[fin]), np.ascontiguousarray(w[fin])
    out["cr_finite_rows"] = fin
    out["cr_ce"] = np.array([L.ref_ce(fp(pf), len(fin), n, fp(lf))], f32)
    out["cr_wce"] = np.array([L.ref_wce(fp(pf), len(fin), n, fp(lf), fp(wf))], f32)
    # with the row whose label has p = 0: the objective is +inf and stays so
    rows = np.arange(6, T)
    pz, lz, wz = np.ascontiguousarray(p[rows]), np.ascontiguousarray(label[rows]), np.ascontiguousarray(w[rows])
    out["cr_wce_with_zero"] = np.array([L.ref_wce(fp(pz), len(rows), n, fp(lz), fp(wz))], f32)
    return out


# ------------------------------------------------------------------------------------ part 3: prior, finalize, the file
STAT_PIECES = {"prior": ("Nn/Prior.cc", 127, 156), "finalize": ("Nn/Statistics.cc", 145, 173), "write": ("Nn/Statistics.cc", 344, 389),
               "header": ("Nn/Statistics.cc", 583, 604), "mean_dev": ("Nn/NeuralNetworkTrainer.cc", 446, 462)}
STAT_SHA = "5544c95b121c1473544df044ef21d606f29b38b01f272551466f9d35042b4f29"
STAT_DIMS = [3, 4, 2]     # the small object whose file is recorded under each flag mask

STAT_SHELL = r"""
// The reference's own headers by include path (as oracle/ref/Makefile compiles its units; nothing is copied): Core::BinaryOutputStream,
// Math::Vector / Math::Matrix with their write(), Core::Type, require().  Linked against oracle/_ref/libref.so for Core/BinaryStream.cc.
#include <Core/BinaryStream.hh>
#include <Core/Types.hh>
#include <Math/Matrix.hh>
#include <Math/Vector.hh>
#include <cmath>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>
// ---- shell (no reference text) ----
namespace Math {
template<class T> void copy(int n, const T* x, int incx, T* y, int incy) { for (int i = 0; i < n; ++i) y[i * incy] = x[i * incx]; }
}
struct Sink { template<class X> Sink& operator<<(const X&) { return *this; } bool isOpen() const { return false; } };
namespace Nn {
// what the statistics use of Math::CudaVector / CudaMatrix: BLAS scal (x = alpha * x), axpy (y = alpha * x + y), element-wise product
template<class T> struct Vec {
    std::vector<T> v;
    Vec() {}
    explicit Vec(u32 n) : v(n) {}
    u32 size() const { return v.size(); }
    u32 nRows() const { return v.size(); }
    void resize(u32 n) { v.resize(n); }
    T& at(u32 i) { return v[i]; }
    const T& at(u32 i) const { return v[i]; }
    const T* begin() const { return v.data(); }
    void initComputation(bool = true) {}
    void finishComputation(bool = true) {}
    void scale(T a) { for (T& x : v) x = a * x; }
    void copy(const Vec& o) { v = o.v; }
    void elementwiseMultiplication(const Vec& o) { for (u32 i = 0; i < v.size(); ++i) v[i] = v[i] * o.v[i]; }
    void add(const Vec& o, T a) { for (u32 i = 0; i < v.size(); ++i) { T p = a * o.v[i]; v[i] = p + v[i]; } }
    void convert(Math::Vector<T>& m) const { m.resize(v.size()); for (u32 i = 0; i < v.size(); ++i) m[i] = v[i]; }
};
template<class T> struct Mat {
    u32 r = 0, c = 0; std::vector<T> v;   // column-major like FastMatrix
    u32 nRows() const { return r; }
    u32 nColumns() const { return c; }
    T& at(u32 i, u32 j) { return v[j * r + i]; }
    const T& at(u32 i, u32 j) const { return v[j * r + i]; }
    void scale(T a) { for (T& x : v) x = a * x; }
    void convert(Math::Matrix<T>& m) const { m.resize(r, c); for (u32 i = 0; i < r; ++i) for (u32 j = 0; j < c; ++j) m[i][j] = at(i, j); }
};
template<class T> class Statistics {
public:
    typedef Vec<T> NnVector;
    typedef Mat<T> NnMatrix;
    bool hasClassCounts_ = false, hasMeanAndVariance_ = false, hasBaseStatistics_ = false, hasGradient_ = false, singlePrecision_ = true;
    bool isComputing_ = false, isFinalized_ = false;
    static const u32 version_ = 2;
    u32 nObservations_ = 0, nClassificationErrors_ = 0;
    T totalWeight_ = 0, objectiveFunction_ = 0;
    std::map<u32, u32> classCount_;
    NnVector sum_, sumOfSquares_;
    std::vector<std::vector<NnMatrix>> gradientWeights_;
    std::vector<NnVector> gradientBias_;
    u32 classCount(u32 c) const { auto it = classCount_.find(c); return it == classCount_.end() ? 0 : it->second; }
    u32 nObservations() const { return nObservations_; }
    NnVector& featureSum() { return sum_; }
    NnVector& squaredFeatureSum() { return sumOfSquares_; }
    void finishComputation(bool = true) {}
    void finalize(bool normalizeByNOfObservations);
    bool write(Core::BinaryOutputStream& os) const;
    bool writeHeader(Core::BinaryOutputStream& o) const;
    const std::string getMagic() const;
};
template<class T> class Prior {
public:
    Vec<T> logPrior_;
    const u32 backOffCount_;
    Sink statisticsChannel_;
    explicit Prior(u32 b) : backOffCount_(b) {}
    Sink log(const char*) { return Sink(); }
    Sink warning(const char*) { return Sink(); }
    void setFromClassCounts(const Statistics<T>& statistics, const Math::Vector<T>& classWeights);
};
template<class T> class MeanAndVarianceTrainer {
public:
    Math::Vector<T> mean_, standardDeviation_;
    std::string meanFile_, standardDeviationFile_;
    Sink log(const char*) { return Sink(); }
    void saveVector(const std::string&, const Math::Vector<T>&) {}
    void writeMeanAndStandardDeviation(Statistics<T>& statistics);
};
// ---- reference text ----
%(prior)s
%(finalize)s
%(write)s
%(header)s
%(mean_dev)s
}  // namespace Nn
// ---- shell: the calls ----
extern "C" {
void ref_prior(const u32* counts, u32 n, const float* class_weights, u32 back_off, float* out) {
    Nn::Statistics<f32> s;
    for (u32 c = 0; c < n; ++c) if (counts[c]) s.classCount_[c] = counts[c];
    Math::Vector<f32> w(n);
    for (u32 c = 0; c < n; ++c) w[c] = class_weights[c];
    Nn::Prior<f32> p(back_off);
    p.setFromClassCounts(s, w);
    for (u32 c = 0; c < n; ++c) out[c] = p.logPrior_.at(c);
}
void ref_mean_dev(const float* sum, const float* sq, u32 dim, float total_weight, u32 n_obs, float* mean, float* dev) {
    Nn::Statistics<f32> s;
    s.hasMeanAndVariance_ = true, s.nObservations_ = n_obs, s.totalWeight_ = total_weight;
    s.sum_.v.assign(sum, sum + dim), s.sumOfSquares_.v.assign(sq, sq + dim);
    Nn::MeanAndVarianceTrainer<f32> t;
    t.writeMeanAndStandardDeviation(s);
    for (u32 i = 0; i < dim; ++i) mean[i] = t.mean_[i], dev[i] = t.standardDeviation_[i];
}
// gw: per layer [in x out] row-major, one after the other; gb: per layer [out]
u32 ref_write(u32 mask, u32 n_obs, float total_weight, u32 n_err, float objective, const u32* counts, u32 n_out, const float* sum, const float* sq, u32 dim,
              u32 n_layers, const u32* in, const u32* out, const float* gw, const float* gb, unsigned char* buf, u32 cap) {
    Nn::Statistics<f32> s;
    s.hasClassCounts_ = mask & 1, s.hasMeanAndVariance_ = mask & 2, s.hasBaseStatistics_ = mask & 4, s.hasGradient_ = mask & 8;
    s.nObservations_ = n_obs, s.totalWeight_ = total_weight, s.nClassificationErrors_ = n_err, s.objectiveFunction_ = objective;
    for (u32 c = 0; c < n_out; ++c) if (counts[c]) s.classCount_[c] = counts[c];
    s.sum_.v.assign(sum, sum + dim), s.sumOfSquares_.v.assign(sq, sq + dim);
    for (u32 l = 0; l < n_layers; ++l) {
        Nn::Mat<f32> m;
        m.r = in[l], m.c = out[l], m.v.resize(in[l] * out[l]);
        for (u32 i = 0; i < in[l]; ++i) for (u32 j = 0; j < out[l]; ++j) m.at(i, j) = gw[i * out[l] + j];
        gw += in[l] * out[l];
        s.gradientWeights_.push_back(std::vector<Nn::Mat<f32>>(1, m));
        Nn::Vec<f32> b(out[l]);
        for (u32 j = 0; j < out[l]; ++j) b.at(j) = gb[j];
        gb += out[l];
        s.gradientBias_.push_back(b);
    }
    std::ostringstream os;
    Core::BinaryOutputStream bos(os);
    s.write(bos);
    const std::string r = os.str();
    if (r.size() <= cap) memcpy(buf, r.data(), r.size());
    return (u32)r.size();
}
}
"""


def build_statistics(tmp):
    cache, parts, h = {}, {}, hashlib.sha256()
    for key, (fn, first, last) in STAT_PIECES.items():
        if fn not in cache:
            with open(os.path.join(REF, fn), encoding="utf-8", errors="replace") as f:
                cache[fn] = f.readlines()
        parts[key] = "".join(cache[fn][first - 1:last])
        h.update(parts[key].encode())
    if h.hexdigest() != STAT_SHA:
        raise SystemExit("make_nntrain_golden: the statistics text at the recorded line ranges hashes to %s, not %s" % (h.hexdigest(), STAT_SHA))
    refdir = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(refdir, "libref.so")):
        raise SystemExit("make_nntrain_golden: oracle/_ref/libref.so is missing: run the build first (it holds the reference's Core/BinaryStream.cc)")
    src, lib = os.path.join(tmp, "nnstat_ref.cc"), os.path.join(tmp, "libnnstat_ref.so")
    with open(src, "w") as f:
        f.write(STAT_SHELL % parts)
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-msse3", "-ffp-contract=off", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-D_GNU_SOURCE",
                           "-DSPRINT_RELEASE_BUILD", "-I" + REF, "-I/usr/include/libxml2", "-w", "-shared", "-o", lib, src, "-L" + refdir, "-lref",
                           "-Wl,-rpath," + refdir])
    return C.CDLL(lib)


def stat_object(mask):
    """a small object's flat buffer (tests/nntrain_reference.py: layout) with values that do not survive a wrong narrowing or order"""
    dims = STAT_DIMS
    y = nr.layout(dims, dims[0], dims[-1], mask)
    rng = np.random.Generator(np.random.PCG64(300 + mask))
    a = (rng.standard_normal(y["size"]) * 3).astype(np.float32).astype(np.float64)
    t = y["tail"]
    a[t], a[t + 1], a[t + 2], a[t + 3] = 1000 + mask, (17 + mask if mask & nr.BASE else 0), np.float32(812.625 + mask), (np.float32(2345.5 + mask) if mask & nr.BASE else 0)
    if mask & nr.CLASS_COUNTS:
        a[y["class_counts"]:y["class_counts"] + dims[-1]] = [0, 40 + mask]     # a class never seen is not written
    return a


def statistics_part(L):
    f32, out = np.float32, {}
    rng = np.random.Generator(np.random.PCG64(77))
    # Prior::setFromClassCounts
    n = 23
    counts = rng.integers(0, 500, n).astype(np.uint32)
    counts[[2, 9]] = 0
    cw = rng.uniform(0.5, 2.0, n).astype(f32)
    cw[5] = 0.0                       # a zero class weight: Type<f32>::min
    out["prior_counts"], out["prior_class_weights"], out["prior_back_off"] = counts, cw, np.array([0, 1, 7], np.uint32)
    for b in out["prior_back_off"]:
        r = np.zeros(n, f32)
        L.ref_prior(fp(counts), n, fp(cw), C.c_uint32(int(b)), fp(r))
        out["prior_log/%d" % b] = r
    # finalize + writeMeanAndStandardDeviation
    dim = 19
    tw = f32(4321.75)
    mean_true = rng.uniform(-3, 3, dim)
    s = (mean_true * tw + rng.standard_normal(dim)).astype(f32)
    q = ((mean_true ** 2 + rng.uniform(0.01, 4.0, dim)) * tw).astype(f32)
    mean, dev = np.zeros(dim, f32), np.zeros(dim, f32)
    L.ref_mean_dev(fp(s), fp(q), dim, C.c_float(tw), 5000, fp(mean), fp(dev))
    out["md_sum"], out["md_square_sum"], out["md_total_weight"], out["md_mean"], out["md_deviation"] = s, q, np.array([tw], f32), mean, dev
    # Statistics<f32>::write under each flag mask
    dims = STAT_DIMS
    L.ref_write.restype = C.c_uint32
    for mask in range(1, 16):
        a = stat_object(mask)
        full = nr.layout(dims, dims[0], dims[-1], 15)
        y = nr.layout(dims, dims[0], dims[-1], mask)
        t = y["tail"]
        cnt = (a[y["class_counts"]:y["class_counts"] + dims[-1]] if mask & nr.CLASS_COUNTS else np.zeros(dims[-1])).astype(np.uint32)
        sm = (a[y["feature_sum"]:y["feature_sum"] + dims[0]] if mask & nr.MEAN_AND_VARIANCE else np.zeros(dims[0])).astype(f32)
        sq = (a[y["feature_square_sum"]:y["feature_square_sum"] + dims[0]] if mask & nr.MEAN_AND_VARIANCE else np.zeros(dims[0])).astype(f32)
        n_layers = len(dims) - 1 if mask & nr.GRADIENT else 0
        gw = np.concatenate([a[y["gradient_weights"][l]:y["gradient_weights"][l] + dims[l] * dims[l + 1]] for l in range(n_layers)] or [np.zeros(1)]).astype(f32)
        gb = np.concatenate([a[y["gradient_bias"][l]:y["gradient_bias"][l] + dims[l + 1]] for l in range(n_layers)] or [np.zeros(1)]).astype(f32)
        ins, outs = np.array(dims[:-1], np.uint32), np.array(dims[1:], np.uint32)
        buf = np.zeros(4096, np.uint8)
        length = L.ref_write(mask, int(a[t]), C.c_float(a[t + 2]), int(a[t + 1]), C.c_float(a[t + 3]), fp(cnt), dims[-1], fp(sm), fp(sq), dims[0], n_layers, fp(ins), fp(outs),
                             fp(gw), fp(gb), fp(buf), len(buf))
        assert 0 < length <= len(buf), (mask, length)
        out["write_flat/%d" % mask], out["write_bytes/%d" % mask] = a, buf[:length].copy()
    out["write_dims"] = np.array(dims)
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / m) if m > 0 else 0.0


def bars():
    out, worst = {}, {}
    mask = nr.CLASS_COUNTS | nr.MEAN_AND_VARIANCE | nr.BASE | nr.GRADIENT
    min_gap = np.inf
    for key, kw in nr.gpu_cases().items():
        net, x, e, w = nr.variant(**kw)
        a = nr.accumulate(net, x, e, w, mask=mask, products="f64")
        b = nr.accumulate(net, x, e, w, mask=mask, products="f32")
        gap = nr.min_top2_gap_ulp(a["softmax"])
        assert gap >= 64, (key, gap)
        min_gap = min(min_gap, gap)
        assert a["n_classification_errors"] == b["n_classification_errors"] and np.array_equal(a["class_counts"], b["class_counts"]), key
        name = kw["name"]
        for l in range(len(net.Ws)):
            for block in ("gradient_weights", "gradient_bias"):
                k = "bar_%s/%s/%d" % (block, name, l)
                worst[k] = max(worst.get(k, 0.0), rel(b[block][l], a[block][l]))
        for block in ("feature_sum", "feature_square_sum"):
            k = "bar_%s/%s" % (block, name)
            worst[k] = max(worst.get(k, 0.0), rel(b[block], a[block]))
        k = "bar_objective/%s" % name
        worst[k] = max(worst.get(k, 0.0), abs(b["objective"] - a["objective"]) / abs(a["objective"]))
        if key in WHOLE:
            dims = net.dims
            out["whole_f64/" + key] = nr.flat(a, dims, dims[0], dims[-1], mask)
            out["whole_f32/" + key] = nr.flat(b, dims, dims[0], dims[-1], mask)
    assert all(("whole_f64/" + k) in out for k in WHOLE), [k for k in WHOLE if ("whole_f64/" + k) not in out]
    for k, v in worst.items():
        assert v > 0, k
        out[k] = np.array([4.0 * v])
    out["min_top2_gap_ulp"] = np.array([min_gap])
    return out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_nntrain.npz")
    with tempfile.TemporaryDirectory() as tmp:
        out = element_wise(build(tmp))
        out.update(statistics_part(build_statistics(tmp)))
    out.update(bars())
    np.savez_compressed(dst, **out)
    for k in sorted(out):
        if k.startswith("bar_"):
            print("%-40s %.3g" % (k, out[k][0]))
    print("wrote %s (%d arrays, %d bytes)" % (dst, len(out), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
