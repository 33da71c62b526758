#!/usr/bin/env python3
"""tests/golden/make_nnseq_golden.py -- writes tests/golden/ref_nnseq.npz: what the tests of the sequence-discriminative NN training read.

Run it where the reference tree is mounted; tests read only the fixture.  Four parts.

1. The collection, the rejection loop and the arc score as the reference's own text computes them.  Taken by line range + SHA-256 into
   a temporary directory and compiled (g++ -O2 -ffp-contract=off) behind a shell of stand-ins that holds no reference text:
     Lattice/Accumulator.hh:114-143        Key, KeyHash, KeyEquality, Collector::collect
     Lattice/Accumulator.tcc:71-72         AcousticAccumulator::discoverState's weight test
     Nn/LatticeAccumulators.hh:81-93       CachedAcousticAccumulator::process / finish (factor_ * collected)
     Nn/LatticeAccumulators.cc:44-49       ErrorSignalAccumulator::accumulate (errorSignal_->at(row, col) += w)
     Nn/MmiSegmentwiseNnTrainer.cc:79-85   the frame rejection loop
     Nn/EmissionLatticeRescorer.cc:221-223 _score's loop over the alignment items
   Stand-ins: the matrix (column-major `at` / operator(), as Math::FastMatrix), ClassLabelWrapper's table look-up, the members the text
   names, verify_ge as a counter, an arc with weight().  Fsa::multiply(fsa, -1) is an f32 product done here.  Nothing of it is committed.
   The restatement (tests/nnseq_reference.py) is held to that text IN EVERY BIT on every segment of the GPU tests' batch under the three
   flows, on the order-sensitive key and on the narrowing case; the generator stops if one differs.
2. The smoothing and the weighting as the reference's own text orders them: Nn/SegmentwiseNnTrainer.cc:644-654 (the prior's
   addToAllColumns, applySoftmax, then scale, add, addKroneckerDelta on the error signal) and :211 (multiplyColumnsByScalars), by line range
   + SHA-256, compiled into the same library against a matrix stand-in whose members are the BLAS calls Math::FastMatrix makes of them
   (Math/FastMatrix.hh:915-931, 1356-1361, 1415-1420: scale = sscal, add = saxpy, addToAllColumns = saxpy per column,
   multiplyColumnsByScalars = sscal per column; addKroneckerDelta = `at(alignment[column], column) += scale`, :1061-1070, whose text
   make_nntrain_golden.py compiles), with scipy's OpenBLAS behind them as for ref_nnstep.npz.  applySoftmax calls back into the
   restatement's softmax (pinned by ref_nntrain.npz) and records the matrix it was given, so the prior's step is compared too.  The
   restatement's error signal after smoothing and weighting equals the text's in every bit on every segment of the MMI flow, with and
   without a prior; the generator stops if one differs.
3. The bars of the sums that go through GEMMs: every flow the GPU tests hold to a bar is evaluated twice by the restatement, all matrix
   products in f64, and all of them in f32 through sgemm with per-chunk partial sums; per layer the bar is 4 x the worst deviation
   between the two, relative to the block's largest magnitude (the factor as in make_nntrain_golden.py).
4. The derivative test's bar: on a lattice of a few arcs, all in f64, the largest |MMI error signal - central difference of the
   objective| over the top output's cells at step DERIVATIVE_STEP; the bar is 4 x that.

    python3 tests/golden/make_nnseq_golden.py [out.npz] [--accept: take the text whatever its hash]
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
from tests import nnseq_reference as sr  # noqa: E402

REF = os.environ.get("AMX_REFERENCE", "/root/reference/src")
F32, F64 = np.float32, np.float64
PIECES = {
    "collector": ("Lattice/Accumulator.hh", 114, 143),
    "weight_test": ("Lattice/Accumulator.tcc", 71, 72),
    "process_finish": ("Nn/LatticeAccumulators.hh", 81, 93),
    "esa": ("Nn/LatticeAccumulators.cc", 44, 49),
    "rejection": ("Nn/MmiSegmentwiseNnTrainer.cc", 79, 85),
    "score": ("Nn/EmissionLatticeRescorer.cc", 221, 223),
    "smooth": ("Nn/SegmentwiseNnTrainer.cc", 644, 654),
    "weight": ("Nn/SegmentwiseNnTrainer.cc", 211, 211),
}
TEXT_SHA256 = "f4d3e96d545e1465e331e9e55b47273622624aff489e279d9dbe96051431a03d"
DERIVATIVE_STEP = 1e-5
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-w"]

SOURCE = r'''
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>
typedef float    f32;
typedef double   f64;
typedef uint32_t u32;
typedef int32_t  s32;
static int g_verify_failed;
#define verify_ge(a, b) do { if (!((a) >= (b))) ++g_verify_failed; } while (0)
namespace Speech { typedef u32 TimeframeIndex; struct AlignmentItem { u32 time; u32 emission; }; }
namespace Mm { typedef u32 MixtureIndex; typedef f64 Weight; }
namespace Lattice {
%(collector)s
}
struct ClassLabelWrapper {
    const s32* map;
    u32 getOutputIndexFromClassIndex(u32 m) const { return (u32)map[m]; }
};
struct MatrixStandIn {   // column-major, as Math::FastMatrix
    f32* d;
    u32  rows;
    f32& at(u32 r, u32 c) { return d[(size_t)c * rows + r]; }
    f32  operator()(u32 r, u32 c) const { return d[(size_t)c * rows + r]; }
};
template<class V> struct VectorStandIn {
    V*  d;
    u32 n;
    u32 size() const { return n; }
    V&  at(u32 i) { return d[i]; }
};
namespace Nn {
template<typename T>
class ErrorSignalAccumulator {
public:
    typedef MatrixStandIn    NnMatrix;
    NnMatrix*                errorSignal_;
    const ClassLabelWrapper* labelWrapper_;
    void accumulate(Speech::TimeframeIndex t, Mm::MixtureIndex m, Mm::Weight w);
};
%(esa)s
template<class Trainer> struct PrecursorStandIn {
    typedef Speech::TimeframeIndex TimeframeIndex;
    Trainer*   trainer_;
    Mm::Weight weightThreshold_;
};
struct ArcStandIn {
    f32 w;
    f32 weight() const { return w; }
};
template<class Trainer>
class CachedAcousticAccumulator : public PrecursorStandIn<Trainer> {
public:
    typedef PrecursorStandIn<Trainer> Precursor;
    Lattice::Collector collector_;
    Mm::Weight         factor_;
    void process(typename Precursor::TimeframeIndex, Mm::MixtureIndex, Mm::Weight);
    void finish();
    void accumulate(Speech::TimeframeIndex t, Mm::MixtureIndex m, Mm::Weight w) { this->trainer_->accumulate(t, m, w); }
    void arc(const ArcStandIn* a, int n, const s32* time, const s32* emission) {
%(weight_test)s
                for (int i = 0; i < n; ++i)
                    process(time[i], emission[i], weight);
            }
    }
};
%(process_finish)s
struct TrainerStandIn {
    VectorStandIn<u32>         alignment_;
    VectorStandIn<f32>         weights_;
    std::vector<MatrixStandIn> errorSignal_;
    f32                        frameRejectionThreshold_;
    u32 reject() {
        u32 nRejectedObsInSeq = 0;
%(rejection)s
        return nRejectedObsInSeq;
    }
};
struct NetworkStandIn {
    MatrixStandIn top;
    MatrixStandIn& getTopLayerOutput() { return top; }
};
struct RescorerStandIn {
    NetworkStandIn    net;
    ClassLabelWrapper wrapper;
    NetworkStandIn&          network() { return net; }
    const ClassLabelWrapper& labelWrapper() const { return wrapper; }
    f32 score(const std::vector<Speech::AlignmentItem>* alignment) {
        f32 score = 0;   // the log semiring's one
%(score)s
        return score;
    }
};
// ---- the smoothing: the matrix members are the BLAS calls Math::FastMatrix makes of them
typedef void (*saxpy_t)(int, float, const float*, int, float*, int);
typedef void (*sscal_t)(int, float, float*, int);
typedef void (*softmax_t)(f32*, u32, u32);
static saxpy_t   g_saxpy;
static sscal_t   g_sscal;
static softmax_t g_softmax;
struct SmoothMatrix {   // column-major [rows x cols]
    f32* d;
    u32  rows, cols;
    f32& at(u32 r, u32 c) { return d[(size_t)c * rows + r]; }
    void initComputation() {}
    void scale(f32 alpha) { g_sscal((int)(rows * cols), alpha, d, 1); }
    void add(const SmoothMatrix& X, f32 alpha) { g_saxpy((int)(rows * cols), alpha, X.d, 1, d, 1); }
    void addKroneckerDelta(VectorStandIn<u32>& alignment, const f32 scale) {
        for (u32 column = 0; column < cols; column++)
            at(alignment.at(column), column) += scale;
    }
    void addToAllColumns(VectorStandIn<f32>& v, f32 alpha) {
        for (u32 i = 0; i < cols; i++)
            g_saxpy((int)rows, alpha, v.d, 1, d + (size_t)i * rows, 1);
    }
    void multiplyColumnsByScalars(VectorStandIn<f32>& scalars) {
        for (u32 i = 0; i < cols; i++)
            g_sscal((int)rows, scalars.d[i], &at(0, i), 1);
    }
};
struct SmoothNetwork {
    SmoothMatrix  top;
    SmoothMatrix& getTopLayerOutput() { return top; }
};
struct TopLayerStandIn {
    void applySoftmax(SmoothMatrix& m) { g_softmax(m.d, m.rows, m.cols); }
};
struct StatisticsStandIn {
    bool hasGradient() const { return true; }
};
struct SmoothTrainer {
    f32                       priorScale_, ceSmoothingWeight_;
    VectorStandIn<f32>        prior_, weights_;
    VectorStandIn<u32>        alignment_;
    std::vector<SmoothMatrix> errorSignal_;
    SmoothNetwork             net;
    TopLayerStandIn           top_layer, *topLayer_ = &top_layer;
    StatisticsStandIn         stats, *statistics_ = &stats;
    SmoothNetwork&            network() { return net; }
    void smooth() {
%(smooth)s
    }
    void weight() {
%(weight)s
    }
};
}  // namespace Nn
extern "C" {
void ref_set_blas(void* axpy, void* scal, void* softmax) {
    Nn::g_saxpy = (Nn::saxpy_t)axpy, Nn::g_sscal = (Nn::sscal_t)scal, Nn::g_softmax = (Nn::softmax_t)softmax;
}
void ref_smooth(int n_out, int T, f32* E, f32* top, f32* prior, f32 prior_scale, f32 lambda, u32* alignment, f32* weights) {
    Nn::SmoothTrainer t;
    t.priorScale_ = prior_scale, t.ceSmoothingWeight_ = lambda;
    t.prior_ = {prior, (u32)n_out}, t.weights_ = {weights, (u32)T}, t.alignment_ = {alignment, (u32)T};
    t.errorSignal_.push_back(Nn::SmoothMatrix{E, (u32)n_out, (u32)T});
    t.net.top = Nn::SmoothMatrix{top, (u32)n_out, (u32)T};
    t.smooth();
    t.weight();
}
void ref_pass(int n_out, f32* E, const s32* map, double threshold, double factor, int n_arcs, const f32* arc_w, const long* item_off, const s32* time,
              const s32* emission) {
    MatrixStandIn     m{E, (u32)n_out};
    ClassLabelWrapper wrap{map};
    Nn::ErrorSignalAccumulator<f32> esa;
    esa.errorSignal_ = &m, esa.labelWrapper_ = &wrap;
    Nn::CachedAcousticAccumulator<Nn::ErrorSignalAccumulator<f32>> acc;
    acc.trainer_ = &esa, acc.weightThreshold_ = threshold, acc.factor_ = factor;
    for (int a = 0; a < n_arcs; ++a) {
        Nn::ArcStandIn arc{arc_w[a]};
        acc.arc(&arc, (int)(item_off[a + 1] - item_off[a]), time + item_off[a], emission + item_off[a]);
    }
    acc.finish();
}
int ref_reject(int n_out, int T, f32* E, u32* alignment, f32* weights, f32 threshold, int* failed) {
    Nn::TrainerStandIn t;
    t.alignment_ = {alignment, (u32)T}, t.weights_ = {weights, (u32)T}, t.frameRejectionThreshold_ = threshold;
    t.errorSignal_.push_back(MatrixStandIn{E, (u32)n_out});
    g_verify_failed = 0;
    const u32 n = t.reject();
    *failed = g_verify_failed;
    return (int)n;
}
f32 ref_score(int n_out, f32* top, const s32* map, int n, const s32* time, const s32* emission) {
    Nn::RescorerStandIn r;
    r.net.top = MatrixStandIn{top, (u32)n_out}, r.wrapper.map = map;
    std::vector<Speech::AlignmentItem> al;
    for (int i = 0; i < n; ++i)
        al.push_back(Speech::AlignmentItem{(u32)time[i], (u32)emission[i]});
    return r.score(&al);
}
}
'''


def reference_text():
    parts, h = {}, hashlib.sha256()
    for key, (fn, first, last) in PIECES.items():
        with open(os.path.join(REF, fn), encoding="utf-8", errors="replace") as f:
            parts[key] = "".join(f.readlines()[first - 1:last])
        h.update(parts[key].encode())
    return parts, h.hexdigest()


def build(tmp, parts):
    gen, so = os.path.join(tmp, "nnseq_ref.cc"), os.path.join(tmp, "nnseq_ref.so")
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", so, gen])
    L = C.CDLL(so)
    f32p, s32p, u32p, i64p = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.float32, np.int32, np.uint32, np.int64))
    L.ref_pass.restype, L.ref_pass.argtypes = None, [C.c_int, f32p, s32p, C.c_double, C.c_double, C.c_int, f32p, i64p, s32p, s32p]
    L.ref_reject.restype, L.ref_reject.argtypes = C.c_int, [C.c_int, C.c_int, f32p, u32p, f32p, C.c_float, C.POINTER(C.c_int)]
    L.ref_score.restype, L.ref_score.argtypes = C.c_float, [C.c_int, f32p, s32p, C.c_int, s32p, s32p]
    L.ref_smooth.restype, L.ref_smooth.argtypes = None, [C.c_int, C.c_int, f32p, f32p, f32p, C.c_float, C.c_float, u32p, f32p]
    return L


SOFTMAX_T = C.CFUNCTYPE(None, C.POINTER(C.c_float), C.c_uint, C.c_uint)


def openblas():
    """the OpenBLAS that scipy bundles: the library and the addresses of cblas_saxpy and cblas_sscal"""
    import glob

    import scipy
    base = os.path.dirname(os.path.dirname(scipy.__file__))
    lib = C.CDLL(sorted(glob.glob(os.path.join(base, "scipy.libs", "libscipy_openblas*.so")))[0])
    return lib, [C.cast(getattr(lib, "scipy_cblas_" + n), C.c_void_p) for n in ("saxpy", "sscal")]


def reference_segment(L, net, T, s, passes, align, w, threshold, rejection):
    """the passes of one segment through the compiled text: (E, rejected, w)"""
    E = np.zeros((T, net.n_outputs), F32)
    cmap = np.ascontiguousarray(net.class_to_output, np.int32)
    rejected, w = 0, np.array(w, F32)
    for ps in passes:
        t = ps["tables"]
        a0, a1 = int(t["arc_offsets"][s]), int(t["arc_offsets"][s + 1])
        io = np.ascontiguousarray(t["item_offsets"][a0:a1 + 1], np.int64)
        aw = np.array(ps["arc_weight"][a0:a1], F32)
        if ps.get("negate"):
            aw = (aw * F32(-1.0)).astype(F32)   # Fsa::multiply(fsa, Weight(-1.0))
        if a1 > a0:
            L.ref_pass(net.n_outputs, E, cmap, float(threshold), float(ps.get("factor", 1.0)), a1 - a0, np.ascontiguousarray(aw), io - io[0],
                       np.ascontiguousarray(t["item_frame"][io[0]:io[-1]], np.int32), np.ascontiguousarray(t["item_emission"][io[0]:io[-1]], np.int32))
        if ps.get("role", sr.ADD) != sr.ADD and rejection > 0:
            failed = C.c_int()
            rejected += L.ref_reject(net.n_outputs, T, E, np.ascontiguousarray(align, np.uint32), w, F32(rejection), C.byref(failed))
            assert failed.value == 0
        if ps.get("role", sr.ADD) == sr.REJECT_CLEAR:
            E[:] = 0
    return E, rejected, w


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "tests", "golden", "ref_nnseq.npz"))
    parts, sha = reference_text()
    if sha != TEXT_SHA256 and "--accept" not in sys.argv:
        sys.exit("the reference text hashes to %s, expected %s (--accept to take it)" % (sha, TEXT_SHA256))
    fx = {"text_sha256": np.frombuffer(sha.encode(), np.uint8)}
    net, off, feats, emission, den, num, w_den, w_num, w_me = sr.gpu_batch()
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp, parts)
        # 1. collection and rejection on the GPU tests' batch
        for flow, passes in sr.gpu_flows().items():
            want = sr.process(net, feats, off, emission, passes, np.zeros(5, F32), rejection=0.3)
            for s, seg in enumerate(want["segments"]):
                T = int(off[s + 1] - off[s])
                align = sr.alignment(net, emission[off[s] - off[0]:off[s + 1] - off[0]])
                E, rejected, w = reference_segment(L, net, T, s, passes, align, net.class_weights[align], sr.EPSILON, 0.3)
                assert np.array_equal(bits(E), bits(seg["E_lattice"])), (flow, s)
                assert rejected == seg["rejected"] and np.array_equal(bits(w), bits(seg["w"])), (flow, s)
                fx["E_lattice/%s/%d" % (flow, s)], fx["w/%s/%d" % (flow, s)] = bits(E), bits(w)
                fx["rejected/%s/%d" % (flow, s)] = np.array([rejected], np.int64)
            print("%s: the restatement's error signal, weights and rejections equal the reference text's on 5 segments" % flow)
        # the order-sensitive key and the narrowing case
        e0 = int(sr.valid_classes(net)[7])
        tables, w, thr = sr.order_case(e0)
        ps = [dict(tables=tables, arc_weight=w, factor=1.0)]
        E, _, _ = reference_segment(L, net, 1, 0, ps, None, np.ones(1, F32), thr, 0.0)
        mine, _ = sr.lattice_error(net, 1, 0, ps, None, None, thr)
        assert np.array_equal(bits(E), bits(mine)) and E[0, sr.class_to_output(net, e0)] == F32(1.0)
        fx["order/E"] = bits(E)
        ps, thr = sr.narrowing_case(e0)
        E, _, _ = reference_segment(L, net, 1, 0, ps, None, np.ones(1, F32), thr, 0.0)
        mine, _ = sr.lattice_error(net, 1, 0, ps, None, None, thr)
        assert np.array_equal(bits(E), bits(mine)) and E[0, sr.class_to_output(net, e0)] == F32(1.0 + 2.0 ** -23)
        fx["narrowing/E"] = bits(E)
        # the arc scores on the restatement's own top output
        cmap = np.ascontiguousarray(net.class_to_output, np.int32)
        for s in range(5):
            _, z = sr.forward(net, feats[off[s]:off[s + 1]])
            z = np.ascontiguousarray(z, F32)
            mine, ref = sr.arc_scores(net, z, den, s), []
            for _, frames, ems in sr.segment_arcs(den, s):
                ref.append(L.ref_score(net.n_outputs, z, cmap, len(frames), np.ascontiguousarray(frames, np.int32), np.ascontiguousarray(ems, np.int32)) if len(frames) else F32(0))
            assert np.array_equal(bits(mine), bits(np.array(ref, F32))), s
            fx["scores/%d" % s] = bits(mine)
        print("the restatement's arc scores equal the reference text's")
        # 2. the smoothing and the weighting in the order of the reference's text, BLAS behind the matrix members
        from tests import nntrain_reference as nr
        blas, addr = openblas()
        seen = {}

        def softmax_cb(ptr, rows, cols):   # column-major [rows x cols] = the restatement's [T x n_out]
            z = np.ctypeslib.as_array(ptr, shape=(cols, rows))
            seen["z"] = z.copy()
            z[:] = nr.softmax(z)
        cb = SOFTMAX_T(softmax_cb)
        L.ref_set_blas(addr[0], addr[1], C.cast(cb, C.c_void_p))
        lam = F32(0.3)
        log_prior = np.log(np.random.Generator(np.random.PCG64(13)).dirichlet(np.ones(net.n_outputs))).astype(F32)
        for tag, prior, scale in (("", None, 0.0), ("_prior", log_prior, 0.7)):
            want = sr.process(net, feats, off, emission, sr.gpu_flows()["mmi"], np.zeros(5, F32), lam=float(lam), rejection=0.3, log_prior=prior, prior_scale=scale)
            for s, seg in enumerate(want["segments"]):
                T = len(seg["w"])
                align = sr.alignment(net, emission[off[s] - off[0]:off[s + 1] - off[0]])
                _, z = sr.forward(net, feats[off[s]:off[s + 1]])
                E, top = np.array(seg["E_lattice"], F32), np.array(z, F32)
                L.ref_smooth(net.n_outputs, T, E, top, np.zeros(net.n_outputs, F32) if prior is None else prior, F32(scale), lam, np.ascontiguousarray(align, np.uint32),
                             np.array(seg["w"], F32))
                if prior is not None:   # the prior's step: saxpy per column against the restatement's fused multiply-add
                    assert np.array_equal(bits(seen["z"]), bits(sr.fma32(F32(scale), prior[None, :], z))), (tag, s)
                assert np.array_equal(bits(top), bits(seg["p"])), (tag, s)
                assert np.array_equal(bits(E), bits(seg["E"])), (tag, s)
                fx["E_smooth%s/%d" % (tag, s)] = bits(E)
        fx["smooth_log_prior"] = log_prior
        print("the restatement's smoothing and weighting equal the reference text's over BLAS on 5 segments, with and without a prior")
    # 3. the bars
    for flow, lam in (("mmi", 0.0), ("me-rejection", 0.25)):
        objective = np.linspace(-3, 5, 5).astype(F32)
        a = sr.process(net, feats, off, emission, sr.gpu_flows()[flow], objective, lam=lam, rejection=0.3, products="f64")["stats"]
        b = sr.process(net, feats, off, emission, sr.gpu_flows()[flow], objective, lam=lam, rejection=0.3, products="f32")["stats"]
        for l in range(3):
            for block in ("gradient_weights", "gradient_bias"):
                bar = 4 * np.abs(a[block][l] - b[block][l]).max() / np.abs(a[block][l]).max()
                assert 0 < bar < 1e-3, (flow, block, l, bar)
                fx["bar_%s/%s/%d" % (block, flow, l)] = np.array([bar], F64)
                print("bar %s %s[%d] = %.3g" % (flow, block, l, bar))
        fx["chunked/%s" % flow] = np.concatenate([g.reshape(-1) for g in b["gradient_weights"]])
    # 4. the derivative test
    dev = sr.mmi_derivative_deviation(*sr.derivative_case(), DERIVATIVE_STEP)
    print("derivative: max deviation %.3g at step %g" % (dev, DERIVATIVE_STEP))
    assert 0 < dev < 1e-8
    fx["derivative_bar"], fx["derivative_step"] = np.array([4 * dev], F64), np.array([DERIVATIVE_STEP], F64)
    np.savez_compressed(out, **fx)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
