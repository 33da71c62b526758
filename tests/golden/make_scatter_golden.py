#!/usr/bin/env python3
"""tests/golden/make_scatter_golden.py -- writes tests/golden/ref_scatter.npz: the LDA scatter-matrix estimation as the reference's
own text computes it.

Run it where the reference tree is mounted and `oracle/_ref/` has been built (`__graft_entry__.build()`); tests read only the
fixture.  What it compiles, in both of the reference's arithmetics (the flag sets of oracle/ref/Makefile: -msse3 = contract=off,
-msse3 -march=native = contract=fma), taken by line range + SHA-256 into a temporary directory that is deleted afterwards:
  * Signal/ScatterEstimator.cc:38-55 (ScatterMatrixEstimator::initialize, accumulate), :63-113 (finalize, finalizeVectorSquareSum,
    read, write, setDimension), :211-234 (ScatterMatricesEstimator::initialize, accumulate), :245-292 (finalize,
    getTotalVectorSum), :337-383 (read, write, setNumberOfClasses)
behind a class shell that declares the members of ScatterEstimator.hh:38-56 and :131-143 (the real header derives from
Core::Component, which pulls in the configuration system; the shell supplies `error`, and `paramShallNormalize(config)` as a
member that returns the flag the driver sets).  Math::Matrix / Math::Vector are the reference's headers as they are;
Core/BinaryStream.cc comes compiled and unmodified from oracle/_ref/libref.so / libref_native.so.
An entry point of this file's own (sc_run) drives them the way TextDependentScatterMatricesEstimator::processAlignedFeature and
ScatterMatricesEstimator::write do: accumulate every frame whose class lies inside the model, dump the members, write the
accumulator file, read it back into a second estimator, finalize with and without normalisation.

Recorded per case (dim 5 and 13, 4 classes; Gaussian and exact frames; weighted and unweighted): the inputs, the flat accumulator,
the accumulator file's bytes, the accumulator as read back from the file, the three matrices with and without normalisation; the
contract=fma copies only where their bits differ from contract=off (expected: nowhere).

    python3 tests/golden/make_scatter_golden.py [out.npz]
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
sys.path.insert(0, ROOT)

# (file, first line, last line): the reference text, in the order it is written out; SHA-256 of the concatenation below
PIECES = {
    "base": [("Signal/ScatterEstimator.cc", 38, 55), ("Signal/ScatterEstimator.cc", 63, 113)],
    "classes": [("Signal/ScatterEstimator.cc", 211, 234), ("Signal/ScatterEstimator.cc", 245, 292), ("Signal/ScatterEstimator.cc", 337, 383)],
}
SHA = "85291ef90ad8e49c9cf261ad583e614e123d0b16584b0e19a22dfc2ee8169788"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/BinaryStream.hh>
#include <Core/Types.hh>
#include <Math/Matrix.hh>
#include <Math/Vector.hh>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>
namespace Signal {
// ---- shell: the members of ScatterEstimator.hh:38-56 and the methods the text below defines
class ScatterMatrixEstimator {
public:
    typedef u32               ClassIndex;
    typedef f32               Data;
    typedef f64               Sum;
    typedef f64               Count;
    typedef Math::Matrix<Sum> ScatterMatrix;
    struct ShallNormalize {
        bool value;
        bool operator()(int) const { return value; }
    } paramShallNormalize;   // stands in for the static Core::ParameterBool read from the configuration
    int  config;
    bool errorSeen;
    void error(const char*, ...) { errorSeen = true; }
    size_t            featureDimension_;
    Math::Matrix<Sum> vectorSquareSum_;
    bool              needInit_;
    ScatterMatrixEstimator() : config(0), errorSeen(false), featureDimension_(0), needInit_(true) { paramShallNormalize.value = true; }
    void         finalizeVectorSquareSum();
    void         initialize();
    void         accumulate(const Math::Vector<Data>&, f32 weight = 1.0);
    bool         finalize();
    virtual bool read(Core::BinaryInputStream&);
    virtual bool write(Core::BinaryOutputStream&);
    void         setDimension(size_t dimension);
};
// ---- shell: the members of ScatterEstimator.hh:131-143
class ScatterMatricesEstimator : public ScatterMatrixEstimator {
    typedef ScatterMatrixEstimator Precursor;
public:
    ClassIndex                     nClasses_;
    std::vector<Math::Vector<Sum>> vectorSums_;
    std::vector<Count>             counts_;
    ScatterMatricesEstimator() : nClasses_(0) {}
    void  initialize(bool deepInitialization = true);
    Count getTotalCount() const {
        return std::accumulate(counts_.begin(), counts_.end(), Count(0));
    }
    Math::Vector<Sum> getTotalVectorSum() const;
    virtual bool      read(Core::BinaryInputStream&);
    virtual bool      write(Core::BinaryOutputStream&);
    void              setNumberOfClasses(size_t nClasses);
    void              accumulate(ClassIndex classIndex, const Math::Vector<Data>&, f32 weight = 1);
    bool              finalize(ScatterMatrix& betweenClassScatterMatrix, ScatterMatrix& withinClassScatterMatrix, ScatterMatrix& totalScatterMatrix);
};
}  // namespace Signal
using namespace Signal;
// ---- reference text: ScatterMatrixEstimator ----
%(base)s
// ---- reference text: ScatterMatricesEstimator ----
%(classes)s
// ---- this generator's own entry point (no reference text) ----
static void dump(const ScatterMatricesEstimator& e, double* flat) {
    for (size_t i = 0; i < e.featureDimension_; ++i)
        for (size_t j = 0; j <= i; ++j)
            *flat++ = e.vectorSquareSum_[i][j];
    for (size_t c = 0; c < e.vectorSums_.size(); ++c)
        for (size_t j = 0; j < e.vectorSums_[c].size(); ++j)
            *flat++ = e.vectorSums_[c][j];
    for (size_t c = 0; c < e.counts_.size(); ++c)
        *flat++ = e.counts_[c];
}
static void copy_out(const Math::Matrix<f64>& m, double* out) {
    for (size_t i = 0; i < m.nRows(); ++i)
        for (size_t j = 0; j < m.nColumns(); ++j)
            *out++ = m[i][j];
}
// mats: [normalize 0 | 1][between | within | total][dim x dim]; returns 0, or a negative step number
extern "C" int sc_run(int dim, int n_classes, int T, const float* feats, const unsigned* cls, const float* weight, const char* path,
                      double* acc, double* acc_read, double* mats) {
    ScatterMatricesEstimator e;
    e.setDimension(dim);
    e.setNumberOfClasses(n_classes);
    e.initialize();
    Math::Vector<f32> x(dim);
    for (int t = 0; t < T; ++t) {
        if (cls[t] >= (unsigned)n_classes)
            continue;   // no label / outside the model: the caller's rule, accumulate() requires classIndex < nClasses_
        for (int i = 0; i < dim; ++i)
            x[i] = feats[(size_t)t * dim + i];
        if (weight)
            e.accumulate(cls[t], x, weight[t]);
        else
            e.accumulate(cls[t], x);
    }
    dump(e, acc);
    {
        Core::BinaryOutputStream bos(path);
        if (!bos || !e.write(bos))
            return -1;
    }
    ScatterMatricesEstimator r;
    {
        Core::BinaryInputStream bis(path);
        if (!bis || !r.read(bis))
            return -2;
    }
    if (r.featureDimension_ != (size_t)dim || r.nClasses_ != (u32)n_classes)
        return -3;
    dump(r, acc_read);
    for (int normalize = 0; normalize < 2; ++normalize) {
        ScatterMatricesEstimator f;   // finalize mirrors the square sum in place: a fresh copy from the file each time
        Core::BinaryInputStream  bis(path);
        if (!bis || !f.read(bis))
            return -4;
        f.paramShallNormalize.value = normalize != 0;
        Math::Matrix<f64> b, w, t;
        if (!f.finalize(b, w, t))
            return -5;
        copy_out(b, mats + ((size_t)normalize * 3 + 0) * dim * dim);
        copy_out(w, mats + ((size_t)normalize * 3 + 1) * dim * dim);
        copy_out(t, mats + ((size_t)normalize * 3 + 2) * dim * dim);
    }
    return 0;
}
// finalize without observations: 1 if it fails with the error reported
extern "C" int sc_empty_fails(int dim, int n_classes) {
    ScatterMatricesEstimator e;
    e.setDimension(dim);
    e.setNumberOfClasses(n_classes);
    e.initialize();
    Math::Matrix<f64> b, w, t;
    return !e.finalize(b, w, t) && e.errorSeen ? 1 : 0;
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-D_GNU_SOURCE", "-DSPRINT_RELEASE_BUILD",
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
    gen = os.path.join(tmp, "scatter_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "scatter_%s.so" % flavour)
    lib = "ref" if flavour == "off" else "ref_native"
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen, "-L" + os.path.join(ROOT, "oracle", "_ref"), "-l" + lib,
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_ref")])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    f64p = np.ctypeslib.ndpointer(np.float64, flags="C")
    L.sc_run.restype = C.c_int
    L.sc_run.argtypes = [C.c_int, C.c_int, C.c_int, f32p, np.ctypeslib.ndpointer(np.uint32, flags="C"), C.c_void_p, C.c_char_p, f64p, f64p, f64p]
    L.sc_empty_fails.restype = C.c_int
    L.sc_empty_fails.argtypes = [C.c_int, C.c_int]
    return L, int(fma or 0)


N_CLASSES = 4


def cases():
    """name -> (feats f32 [T, dim], classes u32 [T], weights f32 [T] or None)"""
    from tests import scatter_reference as sr
    out = {}
    for dim in (5, 13):
        T = 40
        rng = np.random.Generator(np.random.PCG64(100 + dim))
        cls = sr.alignment(T, N_CLASSES, "runs", seed=dim, skip_every=9)
        cls[T // 2:] = sr.alignment(T, N_CLASSES, "random", seed=dim + 1, skip_every=9)[T // 2:]
        # class 3 stays empty at dim 5: finalize skips a class without observations
        if dim == 5:
            cls[cls == 3] = 1
        gauss = (rng.standard_normal((T, dim)) * 3 + rng.standard_normal(dim)).astype(np.float32)
        gw = rng.uniform(0.05, 2.0, T).astype(np.float32)
        exact = sr.exact_features(T, dim, seed=200 + dim)[0]
        ew = sr.exact_weights(T, seed=300 + dim)[0]
        for kind, x, w in (("gauss", gauss, gw), ("exact", exact, ew)):
            out["d%d/%s/unweighted" % (dim, kind)] = (x, cls, None)
            out["d%d/%s/weighted" % (dim, kind)] = (x, cls, w)
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_scatter.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_scatter_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    from tests import scatter_reference as sr
    arrays = {"n_classes": np.array(N_CLASSES)}
    with tempfile.TemporaryDirectory() as tmp:
        libs = {}
        for fl in ("off", "fma"):
            libs[fl], n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)   # fused multiply-adds in the generated object (objdump)
            arrays["empty_finalize_fails/" + fl] = np.array(libs[fl].sc_empty_fails(5, N_CLASSES))
        for name, (x, cls, w) in cases().items():
            T, dim = x.shape
            size = sr.layout(dim, N_CLASSES)[2]
            arrays[name + "/feats"], arrays[name + "/classes"] = x, cls
            if w is not None:
                arrays[name + "/weights"] = w
            got = {}
            for fl, L in libs.items():
                path = os.path.join(tmp, "acc_%s.bin" % fl)
                acc, back, mats = np.zeros(size), np.zeros(size), np.zeros((2, 3, dim, dim))
                r = L.sc_run(dim, N_CLASSES, T, np.ascontiguousarray(x), np.ascontiguousarray(cls), None if w is None else w.ctypes.data,
                             path.encode(), acc, back, mats)
                assert r == 0, (name, fl, r)
                with open(path, "rb") as f:
                    got[fl] = dict(acc=acc, acc_read=back, file=np.frombuffer(f.read(), np.uint8).copy(), matrices=mats[0], matrices_normalized=mats[1])
            for fl in got:
                for k, v in got[fl].items():
                    if fl == "fma" and same_bits(v, got["off"][k]):
                        arrays["%s/fma/%s_same_as_off" % (name, k)] = np.array(1)
                        continue
                    arrays["%s/%s/%s" % (name, fl, k)] = v
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    for k in sorted(arrays):
        if "fma_instructions" in k or "empty_finalize" in k:
            print("  %s = %d" % (k, int(arrays[k])))
    print("  fma copies that differ from off: %d" % sum(1 for k in arrays if "/fma/" in k and "same_as_off" not in k))


if __name__ == "__main__":
    main()
