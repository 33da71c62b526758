"""Generates tests/golden/ref_nnstep.npz: what the tests of NN mini-batch training read (include/amx.h, "NN mini-batch training").  Run it
where the reference tree is mounted; tests read only the fixture.  Three parts.

(a) The reference's own text.  Taken by line range + SHA-256 into a temporary directory and compiled (g++ -O2) behind a shell of
    stand-ins that holds no reference text; nothing of it is committed.  The stand-ins' vector and matrix operations (add = saxpy,
    scale = sscal, l1norm = sasum, sumOfSquares = sdot, addOuterProduct = sger, multiply = sgemv) call the OpenBLAS that scipy bundles,
    handed in by address.
      Math/FastVector.hh 459-478 (addSummedColumns, addSquaredSummedColumns), 499-509 and Math/FastMatrix.hh 1290-1303 (l1clipping),
      Nn/NeuralNetworkLayer.cc 233-262 (the two statistics updates), 285-334 (getActivationMean, getActivationVariance),
      Nn/Statistics.cc 145-173 (finalize), Nn/Regularizer.cc 73-119, 128-165, 181-234 (objectiveFunction / addGradient of the three),
      Nn/MeanNormalizedSgdEstimator.cc 50-126, 135-158 (both estimate bodies; the step sizes are caught in Core::vector2str).
    Recorded: the clip on zeros of both signs, the threshold and its neighbours, subnormals and infinities; on a 5-4-3 network the
    regularisers, finalize and both estimators (plain, a layer without predecessor, with means -- one of smoothing none, one a trace, a
    zero mean among them --, a frozen layer), once on random values (element-wise outputs) and once on dyadic values whose sums are exact
    in f32 in any order (every output); the layer's statistics over three batches in a build with -ffp-contract=fast -mfma and in one
    with -ffp-contract=off.  One piece is a stand-in and not the reference's text: initializeActivationStatistics, without old files
    (zero sums); the rule for old-activations-*-file stays transcribed in the restatement.
(b) The bars.  Anything behind a sum whose order BLAS leaves open gets 4 x the distance between the restatement evaluated with f64 sums
    (what the tests compare the device with) and with the reference's f32 sums (sequential asum / dot / gemv, numpy's sgemm in the pass),
    relative to the block's largest magnitude -- the order of a sum is the reference's free choice, and the device's differs from both:
    the regulariser's objective (as the tests form it, the rounding of the f32 sum included) and the step sizes over update_cases(),
    the gradient of a group of two mini-batches, the update term of the bias with statistics over stat_cases(), every stored
    trajectory step and objective.  Activation sums over two chunks: 4 x the distance between the library's chunk order and the
    reference's one chain.  Tests read the bars from here; no tolerance is written into a test.
(c) Three whole trajectories of the f64 evaluation, parameters after update steps 1, 2 and 10, with the objective of every step.

Conditions on the inputs, asserted here: both evaluations count the same classification errors in every mini-batch; before an L1 clip
no weight lies within 4 ulp of the clip threshold (the planted ones of part (a) apart); the objective after step 10 lies below the one
after step 1.

usage: python tests/golden/make_nnstep_golden.py [output.npz]
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

from tests import nnstep_reference as ns  # noqa: E402

F32 = np.float32

# ------------------------------------------------------------------------------------ part (a): the reference's own text behind stand-ins
REF = os.environ.get("AMX_REFERENCE", "/root/reference/src")
PIECES = [("vector_sums", "Math/FastVector.hh", 459, 478), ("vector_clip", "Math/FastVector.hh", 499, 509), ("matrix_clip", "Math/FastMatrix.hh", 1290, 1303),
          ("layer_update", "Nn/NeuralNetworkLayer.cc", 233, 262), ("layer_mean", "Nn/NeuralNetworkLayer.cc", 285, 334),
          ("finalize", "Nn/Statistics.cc", 145, 173), ("reg_l1", "Nn/Regularizer.cc", 73, 119), ("reg_l2", "Nn/Regularizer.cc", 128, 165),
          ("reg_centered", "Nn/Regularizer.cc", 181, 234), ("estimate", "Nn/MeanNormalizedSgdEstimator.cc", 50, 126),
          ("estimate_clip", "Nn/MeanNormalizedSgdEstimator.cc", 135, 158)]
SHA = "5047d836995fe24bb43b62b8e92a6be04cf6245bc7df537c0381487d181db692"

SHELL = r'''
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
typedef uint32_t u32;
typedef float    f32;
typedef double   f64;
// ---- shell (no reference text) ----
#define require(a) ((void)0)
#define require_eq(a, b) ((void)0)
// the BLAS the stand-ins call: the OpenBLAS that the NN pieces of the oracle recipe link, handed in by address
typedef void  (*axpy_t)(int, float, const float*, int, float*, int);
typedef void  (*scal_t)(int, float, float*, int);
typedef void  (*ger_t)(int, int, int, float, const float*, int, const float*, int, float*, int);
typedef void  (*gemv_t)(int, int, int, int, float, const float*, int, const float*, int, float, float*, int);
typedef float (*asum_t)(int, const float*, int);
typedef float (*dot_t)(int, const float*, int, const float*, int);
static axpy_t b_axpy; static scal_t b_scal; static ger_t b_ger; static gemv_t b_gemv; static asum_t b_asum; static dot_t b_dot;
static std::vector<f32> g_step_sizes;
struct Sink { template<class X> Sink& operator<<(const X&) { return *this; } bool isOpen() const { return true; } };
namespace Core {
template<class T> std::string vector2str(const std::vector<T>& v, const char*) { g_step_sizes.assign(v.begin(), v.end()); return std::string(); }
struct Application { static Application* us() { static Application a; return &a; } void criticalError(const char*, ...) {} };
}
namespace Math {
template<class T> T asum(int n, const T* x, int inc) { return b_asum(n, x, inc); }
template<class T> struct FastMatrix {
    u32 nRows_ = 0, nColumns_ = 0; T* elem_ = nullptr;
    u32 nRows() const { return nRows_; }
    u32 nColumns() const { return nColumns_; }
    T& at(u32 i, u32 j) { return *(elem_ + j * nRows_ + i); }
    const T& at(u32 i, u32 j) const { return *(elem_ + j * nRows_ + i); }
    void l1clipping(const T value);
};
template<class T> struct FastVector {
    u32 nRows_ = 0; T* elem_ = nullptr;
    u32 nRows() const { return nRows_; }
    T& at(u32 i) { return elem_[i]; }
    const T& at(u32 i) const { return elem_[i]; }
    template<typename S> void addSummedColumns(const FastMatrix<S>& matrix, const S scale = 1);
    void addSquaredSummedColumns(const FastMatrix<T>& matrix, const T scale = 1);
    void l1clipping(const T value);
};
// ---- reference text ----
%(vector_sums)s
%(vector_clip)s
%(matrix_clip)s
}  // namespace Math
// ---- shell: the device vector / matrix as far as the text uses them; every BLAS-backed operation calls the BLAS ----
namespace Nn {
template<class T> struct Vec : Math::FastVector<T> {
    std::vector<T> store;
    Vec() {}
    explicit Vec(u32 n) { resize(n); }
    Vec(const Vec& o) : Math::FastVector<T>() { *this = o; }
    Vec& operator=(const Vec& o) { store = o.store; fix(); return *this; }
    void fix() { this->nRows_ = store.size(); this->elem_ = store.data(); }
    void resize(u32 n) { store.resize(n); fix(); }
    u32 size() const { return store.size(); }
    bool isComputing() const { return true; }
    void initComputation(bool = true) {}
    void finishComputation(bool = true) {}
    void setToZero() { std::fill(store.begin(), store.end(), T(0)); }
    void copy(const Vec& o) { store = o.store; fix(); }
    void add(const Vec& o, T a = 1) { b_axpy(size(), a, o.store.data(), 1, store.data(), 1); }
    void scale(T a) { b_scal(size(), a, store.data(), 1); }
    T l1norm() const { return b_asum(size(), store.data(), 1); }
    T sumOfSquares() const { return b_dot(size(), store.data(), 1, store.data(), 1); }
    void elementwiseMultiplication(const Vec& o) { for (u32 i = 0; i < size(); ++i) store[i] = store[i] * o.store[i]; }
    void addConstantElementwise(T c) { for (u32 i = 0; i < size(); ++i) store[i] = store[i] + c; }
    void sign(const Vec& o) { for (u32 i = 0; i < size(); ++i) store[i] = o.store[i] == 0 ? 0 : copysignf(1.0, o.store[i]); }
};
template<class T> struct Mat : Math::FastMatrix<T> {
    std::vector<T> store;
    Mat() {}
    Mat(const Mat& o) : Math::FastMatrix<T>() { *this = o; }
    Mat& operator=(const Mat& o) { store = o.store; this->nRows_ = o.nRows_; this->nColumns_ = o.nColumns_; this->elem_ = store.data(); return *this; }
    void resize(u32 r, u32 c) { store.resize((size_t)r * c); this->nRows_ = r; this->nColumns_ = c; this->elem_ = store.data(); }
    u32 size() const { return store.size(); }
    void copy(const Mat& o) { *this = o; }
    void add(const Mat& o, T a = 1) { b_axpy(size(), a, o.store.data(), 1, store.data(), 1); }
    void scale(T a) { b_scal(size(), a, store.data(), 1); }
    T l1norm() const { return b_asum(size(), store.data(), 1); }
    T sumOfSquares() const { return b_dot(size(), store.data(), 1, store.data(), 1); }
    void sign(const Mat& o) { for (u32 i = 0; i < size(); ++i) store[i] = o.store[i] == 0 ? 0 : copysignf(1.0, o.store[i]); }
    void addOuterProduct(const Vec<T>& x, const Vec<T>& y, T alpha) { b_ger(102, this->nRows_, this->nColumns_, alpha, x.store.data(), 1, y.store.data(), 1, store.data(), this->nRows_); }
    void multiply(const Vec<T>& x, Vec<T>& y, bool transposed, T alpha, T beta) const {
        b_gemv(102, transposed ? 112 : 111, this->nRows_, this->nColumns_, alpha, store.data(), this->nRows_, x.store.data(), 1, beta, y.store.data(), 1);
    }
};
template<class T> struct NeuralNetworkLayer {
    typedef Vec<T> NnVector;
    typedef Mat<T> NnMatrix;
    enum { none, exponentialTrace, noStatistics };
    bool trainable = true; T regConst = 0, rate = 1;
    NnVector bias; std::vector<NnMatrix> weights; std::vector<u32> predecessors;
    bool activationStatisticsNeedInit_ = true, refreshMean_ = true, refreshVariance_ = true;
    NnVector activationSum_, activationSumOfSquares_, activationMean_, activationVariance_;
    u32 nObservations_ = 0; int statisticsSmoothing_ = noStatistics;
    T exponentialTraceInterpolationFactor_ = 0.5, activationVarianceInterpolation_ = 1.0;
    std::string oldMeanFile_, oldStandardDeviationFile_;
    bool isTrainable() const { return trainable; }
    T regularizationConstant() const { return regConst; }
    T learningRate() const { return rate; }
    NnVector* getBias() { return &bias; }
    NnMatrix* getWeights(u32 s) { return &weights[s]; }
    u32 nInputActivations() const { return weights.size(); }
    u32 nPredecessors() const { return predecessors.size(); }
    u32 getPredecessor(u32 s) const { return predecessors[s]; }
    bool hasActivationStatistics() const { return statisticsSmoothing_ != noStatistics; }
    void initializeActivationStatistics(const NnMatrix& output) {  // without old files: zero sums
        activationSum_.resize(output.nRows()); activationSumOfSquares_.resize(output.nRows());
        activationSum_.setToZero(); activationSumOfSquares_.setToZero(); activationStatisticsNeedInit_ = false;
    }
    void nonSmoothedStatisticsUpdate(const NnMatrix& output);
    void exponentialTraceStatisticsUpdate(const NnMatrix& output);
    NnVector& getActivationMean();
    NnVector& getActivationVariance();
};
template<class T> struct NeuralNetwork {
    std::vector<NeuralNetworkLayer<T>> layers;
    u32 nLayers() const { return layers.size(); }
    NeuralNetworkLayer<T>& getLayer(u32 l) { return layers[l]; }
};
template<class T> struct Statistics {
    typedef Vec<T> NnVector;
    bool isFinalized_ = false, hasGradient_ = true, hasMeanAndVariance_ = false;
    u32 nObservations_ = 0; T objectiveFunction_ = 0, totalWeight_ = 0;
    std::vector<std::vector<Mat<T>>> gradientWeights_; std::vector<Vec<T>> gradientBias_;
    NnVector sum_, sumOfSquares_;
    std::vector<Mat<T>>& gradientWeights(u32 l) { return gradientWeights_[l]; }
    Vec<T>& gradientBias(u32 l) { return gradientBias_[l]; }
    bool hasGradient() const { return hasGradient_; }
    u32 nObservations() const { return nObservations_; }
    void finalize(bool normalizeByNOfObservations = true);
};
template<class T> struct L1Regularizer {
    Mat<T> signMatrix_; Vec<T> signVector_;
    typedef Vec<T> NnVector; typedef Mat<T> NnMatrix;
    T objectiveFunction(NeuralNetwork<T>& network, T factor);
    void addGradient(NeuralNetwork<T>& network, Statistics<T>& statistics, T factor);
};
template<class T> struct L2Regularizer {
    typedef Vec<T> NnVector; typedef Mat<T> NnMatrix;
    T objectiveFunction(NeuralNetwork<T>& network, T factor);
    void addGradient(NeuralNetwork<T>& network, Statistics<T>& statistics, T factor);
};
template<class T> struct CenteredL2Regularizer {
    typedef Vec<T> NnVector; typedef Mat<T> NnMatrix;
    NeuralNetwork<T> centerNetwork_; Vec<T> diffVector_; Mat<T> diffMatrix_;
    T objectiveFunction(NeuralNetwork<T>& network, T factor);
    void addGradient(NeuralNetwork<T>& network, Statistics<T>& statistics, T factor);
};
template<class T> struct MeanNormalizedSgd {
    typedef Vec<T> NnVector; typedef Mat<T> NnMatrix;
    bool firstEstimation_ = false, logStepSize_ = true; T initialLearningRate_ = 1, biasLearningRate_ = 1; Sink statisticsChannel_;
    void checkForStatistics(NeuralNetwork<T>&) {}
    void estimate(NeuralNetwork<T>& network, Statistics<T>& statistics);
};
template<class T> struct MeanNormalizedSgdL1Clipping : MeanNormalizedSgd<T> {
    typedef MeanNormalizedSgd<T> Precursor;
    typedef Vec<T> NnVector; typedef Mat<T> NnMatrix;
    using Precursor::logStepSize_; using Precursor::statisticsChannel_;
    void estimate(NeuralNetwork<T>& network, Statistics<T>& statistics);
};
// ---- reference text ----
%(layer_update)s
%(layer_mean)s
%(finalize)s
%(reg_l1)s
%(reg_l2)s
%(reg_centered)s
%(estimate)s
%(estimate_clip)s
}  // namespace Nn
// ---- shell: the calls.  A network travels as flat arrays: per layer W [in x out] column-major (= [out][in] row-major), bias [out] ----
using namespace Nn;
static void fill(NeuralNetwork<f32>& net, Statistics<f32>* st, int L, const int* dims, const float* par, const float* grad, const float* c, const float* rate,
                 const int* trainable, const int* n_pred) {
    net.layers.resize(L);
    if (st) { st->gradientWeights_.resize(L); st->gradientBias_.resize(L); }
    size_t off = 0;
    for (int l = 0; l < L; ++l) {
        auto& y = net.layers[l];
        const int in = dims[l], out = dims[l + 1];
        y.weights.resize(1); y.weights[0].resize(in, out); y.bias.resize(out);
        if (st) { st->gradientWeights_[l].resize(1); st->gradientWeights_[l][0].resize(in, out); st->gradientBias_[l].resize(out); }
        for (int i = 0; i < in * out; ++i) { y.weights[0].store[i] = par[off + i]; if (st) st->gradientWeights_[l][0].store[i] = grad[off + i]; }
        off += (size_t)in * out;
        for (int i = 0; i < out; ++i) { y.bias.store[i] = par[off + i]; if (st) st->gradientBias_[l].store[i] = grad[off + i]; }
        off += out;
        y.regConst = c[l]; y.rate = rate[l]; y.trainable = trainable[l] != 0;
        y.predecessors.clear();
        if (n_pred[l]) y.predecessors.push_back(l - 1 < 0 ? 0 : l - 1);
    }
}
static void dump(NeuralNetwork<f32>& net, Statistics<f32>* st, float* par, float* grad) {
    size_t off = 0;
    for (size_t l = 0; l < net.layers.size(); ++l) {
        auto& y = net.layers[l];
        const size_t nw = y.weights[0].store.size(), nb = y.bias.store.size();
        for (size_t i = 0; i < nw; ++i) { par[off + i] = y.weights[0].store[i]; if (st) grad[off + i] = st->gradientWeights_[l][0].store[i]; }
        off += nw;
        for (size_t i = 0; i < nb; ++i) { par[off + i] = y.bias.store[i]; if (st) grad[off + i] = st->gradientBias_[l].store[i]; }
        off += nb;
    }
}
extern "C" {
void ref_set_blas(void* axpy, void* scal, void* ger, void* gemv, void* asum, void* dot) {
    b_axpy = (axpy_t)axpy; b_scal = (scal_t)scal; b_ger = (ger_t)ger; b_gemv = (gemv_t)gemv; b_asum = (asum_t)asum; b_dot = (dot_t)dot;
}
void ref_vector_clip(float* v, u32 n, float value) { Math::FastVector<f32> x; x.nRows_ = n; x.elem_ = v; x.l1clipping(value); }
void ref_matrix_clip(float* v, u32 rows, u32 cols, float value) { Math::FastMatrix<f32> x; x.nRows_ = rows; x.nColumns_ = cols; x.elem_ = v; x.l1clipping(value); }
// regulariser kind 1 / 2 / 3; center: the centre's parameters (kind 3); returns objectiveFunction, grad <- addGradient
float ref_regularizer(int kind, int L, const int* dims, const float* par, float* grad, const float* center, const float* c, const int* trainable, float factor_obj,
                      float factor_grad) {
    std::vector<float> rate(L, 1.f); std::vector<int> pred(L, 1);
    NeuralNetwork<f32> net; Statistics<f32> st;
    fill(net, &st, L, dims, par, grad, c, rate.data(), trainable, pred.data());
    float obj = 0;
    if (kind == 1) { L1Regularizer<f32> r; obj = r.objectiveFunction(net, factor_obj); r.addGradient(net, st, factor_grad); }
    if (kind == 2) { L2Regularizer<f32> r; obj = r.objectiveFunction(net, factor_obj); r.addGradient(net, st, factor_grad); }
    if (kind == 3) {
        CenteredL2Regularizer<f32> r;
        fill(r.centerNetwork_, nullptr, L, dims, center, nullptr, c, rate.data(), trainable, pred.data());
        obj = r.objectiveFunction(net, factor_obj); r.addGradient(net, st, factor_grad);
    }
    std::vector<float> p(1 << 16);
    dump(net, &st, p.data(), grad);
    return obj;
}
// Statistics::finalize on the gradient and the objective
float ref_finalize(int L, const int* dims, float* grad, u32 n_obs, float objective, int normalize) {
    std::vector<float> par(1 << 16, 0.f), one(L, 1.f); std::vector<int> tr(L, 1);
    NeuralNetwork<f32> net; Statistics<f32> st;
    fill(net, &st, L, dims, par.data(), grad, one.data(), one.data(), tr.data(), tr.data());
    st.nObservations_ = n_obs; st.objectiveFunction_ = objective;
    st.finalize(normalize != 0);
    dump(net, &st, par.data(), grad);
    return st.objectiveFunction_;
}
// estimate: mean[l] nullable = the activation mean of what feeds layer l (given as the sum of a layer with nObservations 1 ... n_obs_mean)
void ref_estimate(int clipping, int L, const int* dims, float* par, float* grad, const float* c, const float* rate, const int* trainable, const int* n_pred,
                  const float* const* act_sum, const u32* act_nobs, const int* act_trace, float eta, float eta_bias, float* steps) {
    NeuralNetwork<f32> net; Statistics<f32> st;
    fill(net, &st, L, dims, par, grad, c, rate, trainable, n_pred);
    // the feeding layers' statistics live in the layer objects: layer l - 1 feeds layer l; the feeder of layer 0 is appended as an extra layer
    net.layers.resize(L + 1);
    for (int l = 0; l < L; ++l) {
        if (!act_sum[l]) continue;
        const int src = l == 0 ? L : l - 1;
        auto& y = net.layers[src];
        y.statisticsSmoothing_ = act_trace[l] ? NeuralNetworkLayer<f32>::exponentialTrace : NeuralNetworkLayer<f32>::none;
        y.activationStatisticsNeedInit_ = false; y.nObservations_ = act_nobs[l];
        y.activationSum_.resize(dims[l]); y.activationSumOfSquares_.resize(dims[l]); y.activationMean_.resize(dims[l]);
        for (int i = 0; i < dims[l]; ++i) y.activationSum_.store[i] = act_sum[l][i];
        if (l == 0 && n_pred[0]) net.layers[0].predecessors[0] = L;
    }
    net.layers[L].trainable = false; net.layers[L].weights.resize(1);
    g_step_sizes.clear();
    if (clipping) { MeanNormalizedSgdL1Clipping<f32> e; e.initialLearningRate_ = eta; e.biasLearningRate_ = eta_bias; e.estimate(net, st); }
    else { MeanNormalizedSgd<f32> e; e.initialLearningRate_ = eta; e.biasLearningRate_ = eta_bias; e.estimate(net, st); }
    for (int l = 0; l < L; ++l) steps[l] = g_step_sizes[l];
    net.layers.resize(L);
    dump(net, &st, par, grad);
}
// a layer's statistics over a sequence of batches: Y [frames x n] row-major per batch = the reference's column-major [n x frames]
void ref_layer_statistics(int trace, float f, u32 n, int n_batches, const u32* frames, const float* Y, float* sum, float* sumsq, float* mean, float* variance, u32* n_obs) {
    NeuralNetworkLayer<f32> y;
    y.statisticsSmoothing_ = trace ? NeuralNetworkLayer<f32>::exponentialTrace : NeuralNetworkLayer<f32>::none;
    y.exponentialTraceInterpolationFactor_ = f;
    size_t off = 0;
    for (int b = 0; b < n_batches; ++b) {
        Mat<f32> out; out.resize(n, frames[b]);
        for (size_t i = 0; i < (size_t)n * frames[b]; ++i) out.store[i] = Y[off + i];
        off += (size_t)n * frames[b];
        if (trace) y.exponentialTraceStatisticsUpdate(out); else y.nonSmoothedStatisticsUpdate(out);
    }
    y.activationMean_.resize(n); y.activationVariance_.resize(n);
    Vec<f32>& m = y.getActivationMean(); Vec<f32>& v = y.getActivationVariance();
    for (u32 i = 0; i < n; ++i) { sum[i] = y.activationSum_.store[i]; sumsq[i] = y.activationSumOfSquares_.store[i]; mean[i] = m.store[i]; variance[i] = v.store[i]; }
    *n_obs = y.nObservations_;
}
}
'''


def ref_pieces():
    cache, out, h = {}, {}, hashlib.sha256()
    for name, fn, first, last in PIECES:
        if fn not in cache:
            with open(os.path.join(REF, fn), encoding="utf-8", errors="replace") as f:
                cache[fn] = f.readlines()
        out[name] = "".join(cache[fn][first - 1:last])
        h.update(out[name].encode())
    return out, h.hexdigest()


def openblas():
    """the OpenBLAS that scipy bundles (the one the NN pieces of the oracle recipe link): addresses of its cblas entry points"""
    import glob

    import scipy
    base = os.path.dirname(os.path.dirname(scipy.__file__))
    lib = C.CDLL(sorted(glob.glob(os.path.join(base, "scipy.libs", "libscipy_openblas*.so")))[0])
    return lib, [C.cast(getattr(lib, "scipy_cblas_" + n), C.c_void_p) for n in ("saxpy", "sscal", "sger", "sgemv", "sasum", "sdot")]


def build_ref(tmp, contract):
    text, sha = ref_pieces()
    if sha != SHA:
        raise SystemExit("make_nnstep_golden: the reference text at the recorded line ranges hashes to %s, not %s" % (sha, SHA))
    tag = "fma" if contract else "off"
    src, lib = os.path.join(tmp, "nnstep_ref_%s.cc" % tag), os.path.join(tmp, "libnnstep_ref_%s.so" % tag)
    with open(src, "w") as f:
        f.write(SHELL % text)
    flags = ["-ffp-contract=fast", "-mfma"] if contract else ["-ffp-contract=off"]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-w"] + flags + ["-o", lib, src])
    L = C.CDLL(lib)
    blas, addr = openblas()
    L.ref_set_blas(*addr)
    L._blas = blas
    L.ref_regularizer.restype = L.ref_finalize.restype = C.c_float
    return L


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


A_DIMS = [5, 4, 3]


def a_network(rng, dyadic):
    """flat parameters and gradient of the 5-4-3 network of part (a), per layer W [out][in] then the bias; dyadic: multiples of 1/8, so
    that every sum of the case is exact in f32 whatever its order"""
    n = sum(i * o + o for i, o in zip(A_DIMS[:-1], A_DIMS[1:]))
    if dyadic:
        return (rng.integers(-16, 17, n) / 8).astype(F32), (rng.integers(-16, 17, n) / 8).astype(F32), (rng.integers(-8, 9, n) / 8).astype(F32)
    par, grad, cen = (rng.standard_normal(n).astype(F32) for _ in range(3))
    par[[0, 7, 21]] = [0.0, -0.0, 1e-42]       # exact zeros of both signs and a subnormal under sign() and the axpy
    return par, grad, cen


def a_split(flat, transpose):
    """flat -> per layer (W [out, in] or G [in, out], bias)"""
    out, off = [], 0
    for i, o in zip(A_DIMS[:-1], A_DIMS[1:]):
        W = flat[off:off + i * o].reshape(o, i)
        off += i * o
        out.append((W.T.copy() if transpose else W.copy(), flat[off:off + o].copy()))
        off += o
    return out


def part_a(tmp):
    out = {}
    L = build_ref(tmp, True)
    Loff = build_ref(tmp, False)
    rng = np.random.Generator(np.random.PCG64(777))
    dims = np.array(A_DIMS, np.int32)
    # ---- the two l1clipping bodies: zeros of both signs, the threshold and its neighbours, subnormals, infinities, random values
    v = F32(0.125)
    st = np.spacing(v)
    w = np.concatenate([np.array([0.0, -0.0, v, -v, v + st, -(v + st), v - st, -(v - st), 1e-42, -1e-42, 1.0, -1.0, np.inf, -np.inf, 2 * v, -2 * v], F32),
                        rng.standard_normal(48).astype(F32) * F32(0.2)])
    out["a/clip_in"], out["a/clip_value"] = w, np.array([v, 0.0, 1e-42], F32)
    for k, value in enumerate(out["a/clip_value"]):
        a, b = w.copy(), w.copy()
        L.ref_vector_clip(fp(a), len(a), C.c_float(value))
        L.ref_matrix_clip(fp(b), 8, len(b) // 8, C.c_float(value))
        out["a/clip_vector%d" % k], out["a/clip_matrix%d" % k] = a, b
    # ---- regularisers, finalize, estimate: a random case (element-wise results) and a dyadic one (everything)
    c, trainable = np.array([0.3, 0.25], F32), np.array([1, 1], np.int32)
    for tag, dyadic in (("random", False), ("dyadic", True)):
        par, grad, cen = a_network(rng, dyadic)
        out["a/%s/par" % tag], out["a/%s/grad" % tag], out["a/%s/center" % tag] = par, grad, cen
        cc = np.array([0.25, 0.5], F32) if dyadic else c
        out["a/%s/c" % tag] = cc
        for kind in (1, 2, 3):
            for tr_tag, tr in (("", trainable), ("_frozen1", np.array([1, 0], np.int32))):
                g = grad.copy()
                obj = L.ref_regularizer(kind, 2, fp(dims), fp(par), fp(g), fp(cen), fp(cc), fp(tr), C.c_float(16.0), C.c_float(24.0))
                out["a/%s/reg%d%s_grad" % (tag, kind, tr_tag)], out["a/%s/reg%d%s_objective" % (tag, kind, tr_tag)] = g, np.array([obj], F32)
        for n_obs, normalize in ((129, 1), (1, 1), (129, 0), (16, 1)):
            g = grad.copy()
            obj = L.ref_finalize(2, fp(dims), fp(g), n_obs, C.c_float(7.5), normalize)
            out["a/%s/finalize_%d_%d_grad" % (tag, n_obs, normalize)], out["a/%s/finalize_%d_%d_objective" % (tag, n_obs, normalize)] = g, np.array([obj], F32)
        # estimate: layer 1 is fed by layer 0 (statistics: none with 4 observations, or a trace); layer 0 with and without a predecessor
        sums = [(rng.integers(-8, 9, d) / 4).astype(F32) if dyadic else rng.standard_normal(d).astype(F32) for d in A_DIMS[:2]]
        if not dyadic:
            sums[1][2] = 0.0        # a zero mean
        out["a/%s/act_sum0" % tag], out["a/%s/act_sum1" % tag] = sums
        rate = np.array([0.5, 2.0], F32)
        for clipping in (0, 1):
            for case, n_pred, stats, tr in (("plain", [1, 1], [0, 0], [1, 1]), ("nopred", [0, 1], [0, 1], [1, 1]), ("means", [1, 1], [1, 1], [1, 1]),
                                            ("frozen", [1, 1], [1, 1], [0, 1])):
                p, g, steps = par.copy(), grad.copy(), np.zeros(2, F32)
                ptr = (C.c_void_p * 2)(*[fp(s_) if on else None for s_, on in zip(sums, stats)])
                nobs, trace = np.array([4, 1], np.uint32), np.array([0, 1], np.int32)
                L.ref_estimate(clipping, 2, fp(dims), fp(p), fp(g), fp(cc), fp(rate), fp(np.array(tr, np.int32)), fp(np.array(n_pred, np.int32)), ptr, fp(nobs),
                               fp(trace), C.c_float(0.25), C.c_float(0.5), fp(steps))
                key = "a/%s/estimate%d_%s" % (tag, clipping, case)
                out[key + "_par"], out[key + "_grad"], out[key + "_steps"] = p, g, steps
    # ---- the layer's statistics in both builds of the reference: three batches of a 6-unit layer
    frames = np.array([40, 1, 129], np.uint32)
    Y = rng.standard_normal((int(frames.sum()), 6)).astype(F32)
    Y[3, 1] = 0.0
    Y[5, 2] = 1e-42
    out["a/stat_frames"], out["a/stat_Y"] = frames, Y
    for contract, lib in (("fma", L), ("off", Loff)):
        for trace in (0, 1):
            for nb in (1, 3):
                res = [np.zeros(6, F32) for _ in range(4)]
                n_obs = C.c_uint32(0)
                lib.ref_layer_statistics(trace, C.c_float(0.75), 6, nb, fp(frames), fp(Y), fp(res[0]), fp(res[1]), fp(res[2]), fp(res[3]), C.byref(n_obs))
                for name, r in zip(("sum", "sumsq", "mean", "variance"), res):
                    out["a/stat_%s_%s_%d/%s" % (contract, "trace" if trace else "none", nb, name)] = r
                out["a/stat_%s_%s_%d/n_obs" % (contract, "trace" if trace else "none", nb)] = np.array([n_obs.value], np.uint32)
    assert not np.array_equal(out["a/stat_fma_none_3/sum"].view(np.uint32), out["a/stat_off_none_3/sum"].view(np.uint32)) or \
        not np.array_equal(out["a/stat_fma_trace_3/sumsq"].view(np.uint32), out["a/stat_off_trace_3/sumsq"].view(np.uint32))   # the inputs tell the builds apart
    return out


# ------------------------------------------------------------------------------------ the bars and the trajectories

def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / m) if m > 0 else 0.0


def assert_clear_of_the_clip(tr, key):
    """the weights just before the clip (the plain estimator's result) keep 4 ulp from the threshold v: the clip's branch is the same in
    both evaluations and on the device"""
    cfg = tr.cfg
    if cfg.estimator != ns.SGD_L1_CLIPPING:
        return
    plain = ns.Cfg(tr.L, cfg.eta, cfg.eta_bias, cfg.eta_l, cfg.c, cfg.trainable, cfg.regularizer, cfg.center, ns.SGD, cfg.A, cfg.normalize, True, cfg.update_input)
    plain.stat_mode = cfg.stat_mode
    G, g, _ = ns.finalize(cfg, tr.G, tr.g, [0.0], tr.n_obs) if not tr.finalized else (tr.G, tr.g, None)
    Ws, bs, _ = ns.estimate(plain, tr.net.Ws, tr.net.bs, [m.copy() for m in G], [m.copy() for m in g], tr.sums, bool(tr.net.pre), tr.means())
    for l, (W, b) in enumerate(zip(Ws, bs)):
        v = F32(F32(cfg.c[l] * cfg.eta) * cfg.eta_l[l])
        for p in (W, b):
            d = np.abs(np.abs(p) - v)
            assert (d[p != 0] > 4 * np.spacing(np.maximum(np.abs(p[p != 0]), v))).all(), (key, l)


def update_bars():
    worst = {}
    for key in sorted(ns.update_cases()):
        name = ns.update_cases()[key][0]
        a, x, e, w = ns.update_case(key, "f64")
        b, _, _, _ = ns.update_case(key, "f32")
        sa, sb = a.step_accumulate(x, e, w), b.step_accumulate(x, e, w)
        assert sa["n_classification_errors"] == sb["n_classification_errors"], key
        assert_clear_of_the_clip(a, key)
        if a.cfg.regularizer != ns.NONE:
            # what the tests form: the group's objective minus its criterion part, both f32 (the objective is criterion + regulariser
            # rounded once, so half an ulp of the objective belongs to the figure), against the regulariser's objective with f64 sums
            oa = ns.regularizer_objective(a.cfg, a.net.Ws, a.net.bs, a.n_obs, "f64")
            ob = ns.regularizer_objective(b.cfg, b.net.Ws, b.net.bs, b.n_obs, "f32")
            formed = float(F32(a.criterion + ob)) - float(a.criterion)
            k = "bar_regularizer_objective/%s" % name
            worst[k] = max(worst.get(k, 0.0), (abs(formed - float(oa)) + 0.5 * float(np.spacing(F32(a.objective)))) / abs(float(oa)))
        # the step sizes on the SAME statistics (the f64 evaluation's): asum alone separates the two
        G, g, _ = ns.finalize(a.cfg, a.G, a.g, [0.0], a.n_obs)
        _, _, s64 = ns.estimate(a.cfg, a.net.Ws, a.net.bs, G, g, "f64")
        _, _, s32 = ns.estimate(a.cfg, a.net.Ws, a.net.bs, G, g, "f32")
        for l in range(a.L):
            k = "bar_step_size/%s/%d" % (name, l)
            worst[k] = max(worst.get(k, 0.0), abs(float(s32[l]) - float(s64[l])) / abs(float(s64[l])))
        # a group of two mini-batches (the second one the first reversed): the f32 statistic after both
        for t in (a, b):
            t.cfg.A = 2
            t.n = 0
            t.step_accumulate(x, e, w)
            t.step_accumulate(x[::-1], e[::-1], w[::-1])
            t.cfg.A = 1
        for l in range(a.L):
            for block, pa, pb in (("gradient_weights", a.G[l], b.G[l]), ("gradient_bias", a.g[l], b.g[l])):
                k = "bar_group_%s/%s/%d" % (block, name, l)
                worst[k] = max(worst.get(k, 0.0), rel(pb, pa))
    # with activation statistics: the update term of the bias is behind a gemv; sums over two chunks against the reference's one chain
    for key in sorted(ns.stat_cases()):
        name = ns.stat_cases()[key][0]
        a, x, e, w = ns.stat_case(key, "f64")
        b, _, _, _ = ns.stat_case(key, "f32")
        sa, sb = a.step_accumulate(x, e, w), b.step_accumulate(x, e, w)
        assert sa["n_classification_errors"] == sb["n_classification_errors"], key
        assert_clear_of_the_clip(a, key)
        G, g, _ = ns.finalize(a.cfg, a.G, a.g, [0.0], a.n_obs)
        for sums, store in (("f64", {}), ("f32", {})):
            Gc, gc = [m.copy() for m in G], [m.copy() for m in g]
            ns.estimate(a.cfg, a.net.Ws, a.net.bs, Gc, gc, sums, means=a.means())
            store["g"] = gc
            if sums == "f64":
                g64 = gc
            else:
                g32 = gc
        for l in range(1, a.L):
            k = "bar_delta_bias/%s/%d" % (name, l)
            worst[k] = max(worst.get(k, 0.0), rel(g32[l], g64[l]))
        a300, x3, e3, w3 = ns.stat_case(key, "f64", T=300)
        Xs, idx = a300.layer_inputs(x3, e3)
        for p_, st in enumerate(a300.stats):
            if st is None:
                continue
            one = ns.ActStat(st.mode, st.f, st.n)
            st.update(Xs[p_], idx)
            one.update(Xs[p_], idx, single_chain=True)
            k = "bar_activation_sums/%s" % name
            worst[k] = max(worst.get(k, 0.0), rel(st.sum, one.sum), rel(st.sumsq, one.sumsq))
    out = {}
    for k, v in worst.items():
        assert v > 0, k
        out[k] = np.array([4.0 * v])
    return out


def trajectories():
    out = {}
    for key in ns.TRAJECTORIES:
        a, batches = ns.trajectory(key, "f64")
        b, _ = ns.trajectory(key, "f32")
        A, objective, objective32 = a.cfg.A, [], []
        for i, (x, e, w) in enumerate(batches):
            sa, sb = a.step_accumulate(x, e, w), b.step_accumulate(x, e, w)
            assert sa["n_classification_errors"] == sb["n_classification_errors"], (key, i)
            if (i + 1) % A:
                continue
            assert_clear_of_the_clip(a, key)
            a.step_estimate()
            b.step_estimate()
            step = (i + 1) // A
            objective.append(a.objective)
            objective32.append(b.objective)
            if step in ns.TRAJECTORY_STEPS:
                for l in range(a.L):
                    for p, pa, pb in (("W", a.net.Ws[l], b.net.Ws[l]), ("b", a.net.bs[l], b.net.bs[l])):
                        out["traj/%s/%d/%s%d" % (key, step, p, l)] = pa.copy()
                        v = rel(pb, pa)
                        assert v > 0, (key, step, p, l)
                        out["bar_traj/%s/%d/%s%d" % (key, step, p, l)] = np.array([4.0 * v])
        out["traj_objective/%s" % key] = np.array(objective, F32)
        out["bar_traj_objective/%s" % key] = np.array([4.0 * rel(objective32, objective)])
        assert objective[-1] < objective[0], (key, objective)
    return out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_nnstep.npz")
    with tempfile.TemporaryDirectory() as tmp:
        out = part_a(tmp)
    out.update(update_bars())
    out.update(trajectories())
    np.savez_compressed(dst, **out)
    for k in sorted(out):
        if k.startswith("bar_") and not k.startswith("bar_traj"):
            print("%-48s %.3g" % (k, out[k][0]))
    for k in sorted(out):
        if k.startswith("traj_objective"):
            print(k, out[k])
    print("wrote %s (%d arrays, %d bytes)" % (dst, len(out), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
