#!/usr/bin/env python3
"""tests/golden/make_cmllr_golden.py -- writes tests/golden/ref_cmllr.npz: constrained MLLR as the reference's own text computes it.

Run it where the reference tree is mounted and `oracle/_ref/` has been built (`__graft_entry__.build()`); tests read only the
fixture.  What it compiles, in both of the reference's arithmetics (the flag sets of oracle/ref/Makefile: -msse3 = contract=off,
-msse3 -march=native = contract=fma), taken by line range + SHA-256 into a temporary directory that is deleted afterwards:
  * Mm/AffineFeatureTransformAccumulator.cc:21-377 (constructors, accumulate unweighted and weighted, finalize, compact, estimate, score,
    combine, read, write; `dump`, which needs the XML writer's configuration, is left out)
  * Mm/AffineFeatureTransformAccumulator.hh:38-92 (the class body; the header itself includes Mm/MixtureSet.hh and with it the
    configuration system)
  * Math/Lapack/MatrixTools.hh:29-99 (invert) and :112-148 (logDeterminant)
behind stand-ins of this file's own for Mm/Types.hh's typedefs, Mm::MixtureSet, Mm::Feature, the accumulator's base class and
Core::Application.  Math::Matrix / Math::Vector are the reference's
headers as they are; Core/BinaryStream.cc comes compiled and unmodified from oracle/_ref/libref.so / libref_native.so.  getrf / getri
are handed in BY ADDRESS from the OpenBLAS that scipy bundles (scipy_dgetrf_ / scipy_dgetri_).
Every flavour is compiled twice: with Mm::FeatureType = f32 as in Mm/Types.hh (accumulators, files, the f32 transform, score), and with
FeatureType = f64, which changes ONE thing: estimate returns its f64 transform without the narrowing (the features are the same f32
values either way, Sum(x) widens them or is the identity).  That is the value the bar is measured on.

An entry point of this file's own drives them as Speech::KeyedEstimator::processAlignedFeature and
AffineFeatureTransformEstimator::postProcess do: accumulate a key's frames in corpus order, dump the members, write the accumulator
behind Core::IoRef's tag (`os << typeName()`, Core/IoRef.hh:119-122), read it back, finalize, estimate, score.

Recorded per case: the inputs, the flat accumulator of all keys after the first call (a cut inside a segment) and at the end, every
key's accumulator file, per estimated key the transform after every iteration (f32 and f64), its score and the XML transform file
(`os << transform` on a Core::XmlOutputStream, Core/XmlStream.cc from oracle/_ref) of the last one, in both builds; an
accumulator or file of more than 64 KiB (the F = M = 45 case) as the SHA-256 of its bytes, which pins every bit as well.  The
generator also measures the BAR of estimate and score: 4 x the largest distance, over the cases and both builds, between
tests/cmllr_reference.py (its own LU, nothing fused) and the reference's text with OpenBLAS's LU, on the f64 transform (absolute, and
relative to the transform's largest element) and on the score.  It checks that every estimated G has a condition number below 1e6.

    python3 tests/golden/make_cmllr_golden.py [out.npz]
"""
import ctypes as C
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"
sys.path.insert(0, ROOT)

PIECES = {
    "lapack": [("Math/Lapack/MatrixTools.hh", 29, 99), ("Math/Lapack/MatrixTools.hh", 112, 148)],
    "header": [("Mm/AffineFeatureTransformAccumulator.hh", 38, 92)],
    "accumulator": [("Mm/AffineFeatureTransformAccumulator.cc", 21, 377)],
}
SHA = "a79ecce7c377830e60fe7f277b39b9e0e077c00fcbda35fb88982f79f6c830eb"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/BinaryStream.hh>
#include <Core/ReferenceCounting.hh>
#include <Core/Types.hh>
#include <Math/Matrix.hh>
#include <Math/Vector.hh>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
// ---- shell: hope() stays in a release build and is defined in Core/Assertions.cc, which is not compiled here
#include <cstdlib>
namespace AssertionsPrivate {
void hopeDisappointed(const char* expr, const char* function, const char* filename, unsigned int line) {
    std::cerr << "hope disappointed: " << expr << " in " << function << std::endl;
    abort();
}
}
// ---- shell: what Math/Lapack/MatrixTools.hh's text calls
static int cm_lapack_failed = 0;
namespace Core {
struct Application {
    struct Message {
        template<class T> Message& operator<<(const T&) { return *this; }
    };
    static Application* us() { static Application a; return &a; }
    Message criticalError(const char*) { cm_lapack_failed = 1; return Message(); }
    Message warning(const char*) { cm_lapack_failed = 1; return Message(); }
};
}
typedef void (*getrf_fn)(int*, int*, double*, int*, int*, int*);
typedef void (*getri_fn)(int*, double*, int*, int*, double*, int*, int*);
static getrf_fn cm_getrf = 0;
static getri_fn cm_getri = 0;
namespace Math { namespace Lapack {
inline void getrf(int* m, int* n, double* a, int* lda, int* ipiv, int* info) { cm_getrf(m, n, a, lda, ipiv, info); }
inline void getri(int* n, double* a, int* lda, int* ipiv, double* work, int* lwork, int* info) { cm_getri(n, a, lda, ipiv, work, lwork, info); }
// ---- reference text: invert, logDeterminant ----
%(lapack)s
} }
// ---- shell: Mm/Types.hh's types, Mm::MixtureSet as far as accumulate reads it, the accumulator's base class
struct CmAccess;
namespace Mm {
typedef f32 MeanType;
typedef f32 VarianceType;
typedef f64 Weight;
typedef u32 MixtureIndex;
typedef u32 DensityIndex;
typedef u32 MeanIndex;
typedef u32 CovarianceIndex;
typedef f64 Sum;
#ifdef CM_WIDE
typedef f64 FeatureType;   // estimate's return value keeps its f64 bits; the feature VALUES stay f32
#else
typedef f32 FeatureType;
#endif
typedef std::vector<FeatureType> FeatureVector;
typedef std::vector<MeanType>    Mean;
struct Feature {
    typedef const FeatureVector* VectorRef;
};
struct GaussDensity {
    MeanIndex       m;
    CovarianceIndex c;
    MeanIndex       meanIndex() const { return m; }
    CovarianceIndex covarianceIndex() const { return c; }
};
struct DiagonalCovariance {
    std::vector<VarianceType>        d;
    const std::vector<VarianceType>& diagonal() const { return d; }
};
struct MixtureSet : public Core::ReferenceCounted {
    std::vector<GaussDensity>       densities;
    std::vector<Mean>               means;
    std::vector<DiagonalCovariance> covariances;
    const GaussDensity*       density(DensityIndex i) const { return &densities[i]; }
    const Mean*               mean(MeanIndex i) const { return &means[i]; }
    const DiagonalCovariance* covariance(CovarianceIndex i) const { return &covariances[i]; }
    size_t                    nCovariances() const { return covariances.size(); }
};
struct AbstractAdaptationAccumulator {
    virtual ~AbstractAdaptationAccumulator() {}
};
class AffineFeatureTransformAccumulator : public AbstractAdaptationAccumulator {
    friend struct ::CmAccess;
// ---- reference text: the class body of Mm/AffineFeatureTransformAccumulator.hh ----
%(header)s
};
}  // namespace Mm
using namespace Mm;
// ---- reference text: Mm/AffineFeatureTransformAccumulator.cc ----
%(accumulator)s
// ---- this generator's own entry points (no reference text) ----
struct CmRun {
    Core::Ref<MixtureSet>                          mixture;
    std::vector<AffineFeatureTransformAccumulator> acc;
    int                                            F, M;
};
struct CmAccess {   // the members are private in the reference's class body
    static void dump(const AffineFeatureTransformAccumulator& a, int pooled, double* flat);
    static bool pooled(const AffineFeatureTransformAccumulator& a) { return a.globalVarianceOptimization_; }
};
static void cm_dump(const AffineFeatureTransformAccumulator& a, int pooled, double* flat) { CmAccess::dump(a, pooled, flat); }
void CmAccess::dump(const AffineFeatureTransformAccumulator& a, int pooled, double* flat) {
    const u32 R = a.featureDimension_ + 1, M = a.modelDimension_;
    *flat++ = a.beta_;
    for (u32 i = 0; i < M; ++i)
        for (u32 j = 0; j < R; ++j)
            *flat++ = a.kAccumulator_[i][j];
    for (u32 j = 0; j < R; ++j)
        *flat++ = a.globalMeanAccumulator_[j];
    for (u32 j = 0; j < R; ++j)
        for (u32 k = j; k < R; ++k)
            *flat++ = a.globalCovarianceAccumulator_[j][k];
    if (!pooled)
        for (u32 i = 0; i < M; ++i)
            for (u32 j = 0; j < R; ++j)
                for (u32 k = j; k < R; ++k)
                    *flat++ = a.gAccumulator_[i].nRows() ? a.gAccumulator_[i][j][k] : 0.0;
}
extern "C" void cm_set_lapack(void* getrf, void* getri) {
    cm_getrf = (getrf_fn)getrf;
    cm_getri = (getri_fn)getri;
}
extern "C" void* cm_new(int F, int M, int n_keys, int n_dens, const unsigned* dens_mean, const unsigned* dens_cov, int n_mean, const float* means,
                        int n_cov, const float* vars) {
    CmRun* r   = new CmRun;
    r->F = F, r->M = M;
    MixtureSet* ms = new MixtureSet;
    for (int d = 0; d < n_dens; ++d)
        ms->densities.push_back(GaussDensity{dens_mean[d], dens_cov[d]});
    for (int i = 0; i < n_mean; ++i)
        ms->means.push_back(Mean(means + (size_t)i * M, means + (size_t)(i + 1) * M));
    for (int i = 0; i < n_cov; ++i) {
        DiagonalCovariance c;
        c.d.assign(vars + (size_t)i * M, vars + (size_t)(i + 1) * M);
        ms->covariances.push_back(c);
    }
    r->mixture = Core::Ref<MixtureSet>(ms);
    for (int k = 0; k < n_keys; ++k)
        r->acc.push_back(AffineFeatureTransformAccumulator(F, M, "key"));
    return r;
}
extern "C" void cm_free(void* p) { delete (CmRun*)p; }
extern "C" void cm_accumulate(void* p, int key, const float* x, unsigned density, int weighted, double weight) {
    CmRun*        r = (CmRun*)p;
    FeatureVector f(x, x + r->F);
    if (weighted)
        r->acc[key].accumulate(&f, density, r->mixture, weight);
    else
        r->acc[key].accumulate(&f, density, r->mixture);
}
extern "C" void cm_members(void* p, int key, int pooled, double* flat) { cm_dump(((CmRun*)p)->acc[key], pooled, flat); }
// write behind Core::IoRef's tag, read back into a fresh accumulator and dump that: 0, or a negative step number
extern "C" int cm_file(void* p, int key, int pooled, const char* path, double* flat_read) {
    CmRun* r = (CmRun*)p;
    {
        Core::BinaryOutputStream os(path);
        if (!os)
            return -1;
        os << r->acc[key].typeName();
        if (!r->acc[key].write(os))
            return -2;
    }
    Core::BinaryInputStream is(path);
    std::string             tag;
    is >> tag;
    if (!is || tag != r->acc[key].typeName())
        return -3;
    AffineFeatureTransformAccumulator back;
    if (!back.read(is))
        return -4;
    if (CmAccess::pooled(back) != (pooled != 0))
        return -5;
    cm_dump(back, pooled, flat_read);
    return 0;
}
extern "C" void cm_combine(void* p, int key, int other, double weight) {
    CmRun* r = (CmRun*)p;
    r->acc[key].combine(r->acc[other], weight);
}
// the transform file of AffineFeatureTransformEstimator::postProcess (Speech/AffineFeatureTransformEstimator.cc:128-132): `os << transform`
extern "C" int cm_transform_file(const char* path, int rows, int cols, const float* t) {
    Math::Matrix<f32> m(rows, cols);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j)
            m[i][j] = t[(size_t)i * cols + j];
    Core::XmlOutputStream os(path);
    if (!os.good())
        return -1;
    os << m;
    return 0;
}
// finalize + estimate + score on a COPY of the key's accumulator.  out [M x (F + 1)] in FeatureType; returns 0, or 1 when LAPACK failed
extern "C" int cm_estimate(void* p, int key, int iterations, double min_obs, int criterion, const float* initial, int initial_cols, void* out,
                           double* score) {
    CmRun*                            r = (CmRun*)p;
    AffineFeatureTransformAccumulator a = r->acc[key];
    cm_lapack_failed                    = 0;
    a.finalize();
    AffineFeatureTransformAccumulator::Transform t;
    if (initial) {
        AffineFeatureTransformAccumulator::Transform ini(r->M, initial_cols);
        for (int i = 0; i < r->M; ++i)
            for (int j = 0; j < initial_cols; ++j)
                ini[i][j] = initial[(size_t)i * initial_cols + j];
        t = a.estimate(iterations, min_obs, (AffineFeatureTransformAccumulator::Criterion)criterion, ini);
    }
    else
        t = a.estimate(iterations, min_obs, (AffineFeatureTransformAccumulator::Criterion)criterion);
    FeatureType* o = (FeatureType*)out;
    for (size_t i = 0; i < t.nRows(); ++i)
        for (size_t j = 0; j < t.nColumns(); ++j)
            *o++ = t[i][j];
    if (score)
        *score = a.score(t, (AffineFeatureTransformAccumulator::Criterion)criterion);
    return cm_lapack_failed;
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


def openblas():
    import scipy
    libs = glob.glob(os.path.join(os.path.dirname(os.path.dirname(scipy.__file__)), "scipy.libs", "libscipy_openblas*.so"))
    assert libs, "the OpenBLAS that scipy bundles was not found"
    L = C.CDLL(libs[0])
    return C.cast(L.scipy_dgetrf_, C.c_void_p), C.cast(L.scipy_dgetri_, C.c_void_p), L


def build(tmp, flavour, wide, parts, lapack):
    name = "cmllr_%s%s" % (flavour, "_wide" if wide else "")
    gen = os.path.join(tmp, name + ".cc")
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, name + ".so")
    lib = "ref" if flavour == "off" else "ref_native"
    extra = ([] if flavour == "off" else ["-march=native"]) + (["-DCM_WIDE"] if wide else [])
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen, "-L" + os.path.join(ROOT, "oracle", "_ref"), "-l" + lib,
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_ref")])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    f32p, f64p, u32p = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.float32, np.float64, np.uint32))
    L.cm_set_lapack.argtypes = [C.c_void_p, C.c_void_p]
    L.cm_new.restype = C.c_void_p
    L.cm_new.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u32p, u32p, C.c_int, f32p, C.c_int, f32p]
    L.cm_free.argtypes = [C.c_void_p]
    L.cm_accumulate.argtypes = [C.c_void_p, C.c_int, f32p, C.c_uint, C.c_int, C.c_double]
    L.cm_members.argtypes = [C.c_void_p, C.c_int, C.c_int, f64p]
    L.cm_file.restype = C.c_int
    L.cm_file.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, f64p]
    L.cm_combine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
    L.cm_estimate.restype = C.c_int
    L.cm_estimate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.cm_transform_file.restype = C.c_int
    L.cm_transform_file.argtypes = [C.c_char_p, C.c_int, C.c_int, f32p]
    L.cm_set_lapack(lapack[0], lapack[1])
    return L, int(fma or 0)


MIN_OBS = 10.0


def exact_model(M, seed):
    """means k / 16, variances powers of two, per-density covariances: with features k / 64 and weights j / 16 no operation rounds"""
    from tests import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    m = synth.gmm_cart(4, 1, 3, M, seed=seed, pooled=False)
    m["means"] = (rng.integers(-32, 33, m["means"].shape) / 16.0).astype(np.float32)
    m["variances"] = (2.0 ** rng.integers(-1, 3, m["variances"].shape)).astype(np.float32)
    return m


def cases():
    """name -> dict(model, F, n_keys, feats, frame_offsets, seg_key, emission, best, weight or None, cut, iterations, initial or None)"""
    from tests import synth
    out = {}
    for (F, M, T0, iters) in ((5, 5, 40, 3), (13, 9, 60, 3), (45, 45, 160, 2)):
        for pooled in (False, True):
            for weighted in (False, True):
                for kind in ("gauss", "exact"):
                    if F == 45 and (pooled or not weighted or kind == "exact"):
                        continue   # one case at F = M = 45
                    if kind == "exact" and pooled:
                        continue
                    seed = 1000 * F + 10 * pooled + weighted
                    rng = np.random.Generator(np.random.PCG64(seed))
                    model = exact_model(M, seed) if kind == "exact" else synth.gmm_cart(5, 1, 3, M, seed=seed, pooled=pooled)
                    # key 0: two segments around one of key 2; key 1: no frame; key 2: fewer frames than min-observation-weight
                    lens = [T0 // 2 + 3, 4, T0 - T0 // 2 - 3, 3]
                    seg_key = np.array([0, 2, 0, 2], np.int32)
                    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                    T = int(off[-1])
                    if kind == "gauss":
                        feats = (rng.standard_normal((T, F)) * 1.5 + rng.standard_normal(F)).astype(np.float32)
                        weight = rng.uniform(0.05, 2.0, T) if weighted else None
                    else:
                        feats = (rng.integers(-256, 257, (T, F)) / 64.0).astype(np.float32)
                        weight = rng.integers(0, 33, T) / 16.0 if weighted else None
                    if weighted:
                        weight[[2, T // 2]] = 0.0
                    n_mix = len(model["mix_offsets"]) - 1
                    emission = rng.integers(0, n_mix, T).astype(np.int32)
                    emission[[5, T - 2]] = -1
                    ks = (model["mix_offsets"][1:] - model["mix_offsets"][:-1]).astype(np.int64)
                    best = np.array([rng.integers(0, ks[e]) if e >= 0 else 0xFFFFFFFF for e in emission], np.uint32)
                    initial = None
                    if F == 13:   # an F-column initial transform: a zero column goes in front
                        initial = np.zeros((M, F), np.float32)
                        initial[np.arange(M), np.arange(M)] = 1.0
                        initial += (rng.standard_normal((M, F)) * 0.01).astype(np.float32)
                    if F == 5 and pooled:   # an (F + 1)-column initial transform: taken as it is
                        initial = np.zeros((M, F + 1), np.float32)
                        initial[np.arange(M), np.arange(M) + 1] = 1.0
                        initial += (rng.standard_normal((M, F + 1)) * 0.01).astype(np.float32)
                    name = "f%dm%d/%s/%s/%s" % (F, M, "pooled" if pooled else "full", "weighted" if weighted else "unweighted", kind)
                    out[name] = dict(model=model, F=F, n_keys=3, feats=feats, frame_offsets=off, seg_key=seg_key, emission=emission, best=best,
                                     weight=weight, cut=int(off[0] + lens[0] // 2), iterations=iters, initial=initial)
    return out


BIG = 1 << 16


def store(arrays, name, v):
    """a recorded result; one of more than 64 KiB (the accumulators and files of the F = M = 45 case) as the SHA-256 of its bytes"""
    v = np.ascontiguousarray(v)
    if v.nbytes > BIG:
        arrays[name + "_sha256"] = np.frombuffer(hashlib.sha256(v.tobytes()).digest(), np.uint8).copy()
    else:
        arrays[name] = v


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_reference(L, Lw, c, tmp):
    """everything the reference's text gives for one case in one build"""
    from tests import cmllr_reference as cr
    model, F, n_keys = c["model"], c["F"], c["n_keys"]
    M, pooled = int(model["dim"]), cr.is_pooled(model)
    size = cr.layout(F, M, pooled)["size"]
    args = (F, M, n_keys, len(model["dens_mean"]), np.ascontiguousarray(model["dens_mean"], np.uint32), np.ascontiguousarray(model["dens_cov"], np.uint32),
            model["means"].shape[0], np.ascontiguousarray(model["means"], np.float32), model["variances"].shape[0],
            np.ascontiguousarray(model["variances"], np.float32))
    h, hw = L.cm_new(*args), Lw.cm_new(*args)
    key_of = np.full(len(c["feats"]), -1)
    for s, k in enumerate(c["seg_key"]):
        key_of[c["frame_offsets"][s]:c["frame_offsets"][s + 1]] = k
    got = {}

    def dump():
        flat = np.zeros(n_keys * size)
        for k in range(n_keys):
            one = np.zeros(size)
            L.cm_members(h, k, int(pooled), one)
            flat[k * size:(k + 1) * size] = one
        return flat

    for t in range(len(c["feats"])):
        if t == c["cut"]:
            got["acc_cut"] = dump()
        e = int(c["emission"][t])
        if e < 0 or key_of[t] < 0:
            continue
        d = int(model["dens_index"][int(model["mix_offsets"][e]) + int(c["best"][t])])
        x = np.ascontiguousarray(c["feats"][t, :F])
        for lib, hh in ((L, h), (Lw, hw)):
            lib.cm_accumulate(hh, int(key_of[t]), x, d, int(c["weight"] is not None), float(c["weight"][t]) if c["weight"] is not None else 1.0)
    got["acc"] = dump()
    for k in (0, 2):
        path = os.path.join(tmp, "acc.bin")
        back = np.zeros(size)
        r = L.cm_file(h, k, int(pooled), path.encode(), back)
        assert r == 0, r
        assert same_bits(back, got["acc"][k * size:(k + 1) * size]), "the file does not give the members back"
        with open(path, "rb") as f:
            got["file/key%d" % k] = np.frombuffer(f.read(), np.uint8).copy()
    ini = c["initial"]
    inip, cols = (None, 0) if ini is None else (np.ascontiguousarray(ini).ctypes.data, ini.shape[1])
    R = F + 1
    for crit, cname in ((cr.NAIVE, "naive"), (cr.MMI_PRIME, "mmi")):
        its = [1] if crit == cr.NAIVE else list(range(1, c["iterations"] + 1))
        t32, t64, sc = np.zeros((len(its), M, R), np.float32), np.zeros((len(its), M, R), np.float64), np.zeros(len(its))
        for n, it in enumerate(its):
            s = C.c_double()
            assert L.cm_estimate(h, 0, it, MIN_OBS, crit, inip, cols, t32[n].ctypes.data, C.byref(s)) == 0
            sc[n] = s.value
            assert Lw.cm_estimate(hw, 0, it, MIN_OBS, crit, inip, cols, t64[n].ctypes.data, None) == 0
            assert same_bits(t64[n].astype(np.float32), t32[n]), "the wide build's transform does not narrow to the f32 build's"
        got["%s/transform" % cname], got["%s/transform64" % cname], got["%s/score" % cname] = t32, t64, sc
        path = os.path.join(tmp, "transform.xml")   # the file postProcess writes for the key: `os << transform`
        assert L.cm_transform_file(path.encode(), M, R, np.ascontiguousarray(t32[-1])) == 0
        with open(path, "rb") as f:
            got["%s/transform_file" % cname] = np.frombuffer(f.read(), np.uint8).copy()
    # key 2 lies below min-observation-weight: mmi-prime returns the initial transform (:204-205)
    t = np.zeros((M, R), np.float32)
    assert L.cm_estimate(h, 2, 2, MIN_OBS, cr.MMI_PRIME, inip, cols, t.ctypes.data, None) == 0
    got["below_min_obs/transform"] = t
    # combine: key 0 += 0.5 * key 2
    L.cm_combine(h, 0, 2, 0.5)
    one = np.zeros(size)
    L.cm_members(h, 0, int(pooled), one)
    got["combined"] = one
    L.cm_free(h)
    Lw.cm_free(hw)
    return got


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_cmllr.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_cmllr_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    from tests import cmllr_reference as cr
    lapack = openblas()
    arrays = {"min_obs_weight": np.array(MIN_OBS)}
    bar = dict(transform_abs=0.0, transform_rel=0.0, score_abs=0.0, score_rel=0.0)
    worst_cond = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        libs = {}
        for fl in ("off", "fma"):
            L, n_fma = build(tmp, fl, False, parts, lapack)
            Lw, _ = build(tmp, fl, True, parts, lapack)
            libs[fl] = (L, Lw)
            arrays["fma_instructions/" + fl] = np.array(n_fma)
        for name, c in cases().items():
            model, F = c["model"], c["F"]
            M, pooled = int(model["dim"]), cr.is_pooled(model)
            var = model["variances"][0] if pooled else None
            size = cr.layout(F, M, pooled)["size"]
            for k in ("feats", "frame_offsets", "seg_key", "emission", "best"):
                arrays["%s/%s" % (name, k)] = c[k]
            for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov", "means", "variances", "log_weight"):
                arrays["%s/model/%s" % (name, k)] = model[k]
            arrays[name + "/cut"], arrays[name + "/iterations"] = np.array(c["cut"]), np.array(c["iterations"])
            if c["weight"] is not None:
                arrays[name + "/weight"] = np.asarray(c["weight"], np.float64)
            if c["initial"] is not None:
                arrays[name + "/initial"] = c["initial"]
            got = {fl: run_reference(libs[fl][0], libs[fl][1], c, tmp) for fl in libs}
            for fl in got:
                for k, v in got[fl].items():
                    if fl == "fma" and same_bits(v, got["off"][k]):
                        arrays["%s/fma/%s_same_as_off" % (name, k)] = np.array(1)
                        continue
                    store(arrays, "%s/%s/%s" % (name, fl, k), v)
                # the bar: the restatement on the reference's accumulator of this build
                acc0 = got[fl]["acc"][:size]
                fin = cr.finalize(acc0, F, M, var)
                worst_cond = max(worst_cond, max(np.linalg.cond(g) for g in fin["G"]))
                for crit, cname in ((cr.NAIVE, "naive"), (cr.MMI_PRIME, "mmi")):
                    n_it = 1 if crit == cr.NAIVE else c["iterations"]
                    e = cr.estimate(acc0, F, M, n_it, MIN_OBS, crit, c["initial"], var)
                    mine = e["transform64"][None] if crit == cr.NAIVE else e["iterations"]
                    ref = got[fl]["%s/transform64" % cname]
                    for a, b in zip(mine, ref):
                        d = float(np.abs(a - b).max())
                        bar["transform_abs"] = max(bar["transform_abs"], d)
                        bar["transform_rel"] = max(bar["transform_rel"], d / float(np.abs(b).max()))
                    for n in range(len(ref)):
                        s = cr.score(acc0, F, M, got[fl]["%s/transform" % cname][n], crit, var)
                        d = abs(s - got[fl]["%s/score" % cname][n])
                        bar["score_abs"] = max(bar["score_abs"], d)
                        bar["score_rel"] = max(bar["score_rel"], d / abs(got[fl]["%s/score" % cname][n]))
                    if crit == cr.MMI_PRIME:   # what `1 / 2` as an integer division leaves of the root's choice
                        arrays["%s/%s/mmi/first_root_chosen" % (name, fl)] = np.array([ch[0] for ch in e["choices"]])
    assert worst_cond < 1e6, "an accumulated G has condition number %g" % worst_cond
    arrays["worst_condition_number"] = np.array(worst_cond)
    for k, v in bar.items():
        arrays["measured/" + k] = np.array(v)
        arrays["bar/" + k] = np.array(4 * v)
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    for k in sorted(arrays):
        if k.startswith(("fma_instructions", "measured/", "bar/", "worst_")):
            print("  %s = %g" % (k, float(arrays[k])))
    differ = sorted(k for k in arrays if "/fma/" in k and "same_as_off" not in k)
    print("  fma copies that differ from off: %d" % len(differ))
    for k in differ:
        print("    " + k)


if __name__ == "__main__":
    main()
