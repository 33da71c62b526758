#!/usr/bin/env python3
"""tests/golden/make_mllr_golden.py -- writes tests/golden/ref_mllr.npz: MLLR as the reference's own text computes it.

Run it where the reference tree is mounted and `oracle/_ref/` has been built (`__graft_entry__.build()`); tests read only the
fixture.  What it compiles, in both of the reference's arithmetics (the flag sets of oracle/ref/Makefile: -msse3 = contract=off,
-msse3 -march=native = contract=fma), taken by line range + SHA-256 into a temporary directory that is deleted afterwards:
  * Mm/MllrAdaptation.hh:34-412 (the typedefs, every class body, propagate)
  * Mm/MllrAdaptation.cc:21-417, :444-715, :741-841 (everything but the two accumulate(alignment, ...) overloads, which need the
    acoustic model and the feature scorer; the adapter's loop over the alignment is this file's own)
  * Math/Lapack/Svd.hh:24-33, Math/Lapack/Svd.cc:21-99 (pseudoInvert, solveLinearLeastSquares), Math/Lapack/MatrixTools.hh:101-108
behind stand-ins of this file's own for Mm/Types.hh's typedefs, Mm::MixtureSet, Am::AdaptationTree (Am/AdaptationTree.cc:95-99: prune,
then the silence class appended), Core::Component, Core::Configuration, Core::ParameterFloat and Core::XmlChannel.  Math::Matrix /
Math::Vector and Core::BinaryTree are the reference's as they are (Core/BinaryTree.cc is compiled unmodified from where it lies);
Core/BinaryStream.cc and Core/XmlStream.cc come compiled and unmodified from oracle/_ref/libref.so / libref_native.so.  dgelsd is
handed in BY ADDRESS from the OpenBLAS that scipy bundles (scipy_dgelsd_).

An entry point of this file's own drives them as Speech::ModelTransformEstimator does: accumulate a key's frames in corpus order, dump
the leaf accumulators, write the accumulator behind Core::IoRef's tag, read it back, adaptor() on a copy, the adaptor's file (written,
read back, written again), adaptMixtureSet on a copy of the mixture set.

Recorded per case: the inputs, the tree as the reference's BinaryTree answers after prune(), leafIndex_, the flat accumulator of all
keys after the first call (a cut inside a segment) and at the end, the accumulator files, and per estimated key and threshold pair the
matrices, their ids, the index vector, count_, the adaptor file and the adapted means, in both builds.  The generator also measures
the BAR of the full estimator's W: 4 x the largest distance, over the cases and both builds, between tests/mllr_reference.py (Jacobi
eigen-decomposition, as rasr_amd/csrc/mllr_host.cpp) and the reference's text with OpenBLAS's dgelsd, absolute and relative to the
matrix's largest element.  It asserts the condition on the inputs: over every G that is inverted no singular value lies in
[1e-14, 1e-10] x the largest, at least one such G is rank-deficient and at least one has full rank.

    python3 tests/golden/make_mllr_golden.py [out.npz]
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
    "svd": [("Math/Lapack/Svd.hh", 24, 33), ("Math/Lapack/Svd.cc", 21, 99), ("Math/Lapack/MatrixTools.hh", 101, 108)],
    "header": [("Mm/MllrAdaptation.hh", 34, 412)],
    "body": [("Mm/MllrAdaptation.cc", 21, 417), ("Mm/MllrAdaptation.cc", 444, 715), ("Mm/MllrAdaptation.cc", 741, 841)],
}
SHA = "015b4f9d40aa10002cf8b960374702f10d2461f8c71fc08cc1a090865efa32d7"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/BinaryStream.hh>
#include <Core/BinaryTree.hh>
#include <Core/ReferenceCounting.hh>
#include <Core/Types.hh>
#include <Core/XmlStream.hh>
#include <Math/Matrix.hh>
#include <Math/Vector.hh>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <stack>
#include <string>
#include <vector>
// ---- shell: hope() stays in a release build and is defined in Core/Assertions.cc, which is not compiled here
namespace AssertionsPrivate {
void hopeDisappointed(const char* expr, const char* function, const char* filename, unsigned int line) {
    std::cerr << "hope disappointed: " << expr << " in " << function << std::endl;
    abort();
}
}
// ---- shell: the configuration system as far as Mm/MllrAdaptation.* uses it
static double ml_min_obs = 1000, ml_min_sil = 500;
static int    ml_failed  = 0;
namespace Core {
struct Configuration {};
struct Message {
    template<class T> Message& operator<<(const T&) { return *this; }
};
struct Component {
    Configuration config;
    Component(const Configuration& c) : config(c) {}
    Message log(const char* = "", ...) const { return Message(); }
    Message criticalError(const char* = "", ...) const { ml_failed = 1; return Message(); }
};
struct XmlChannel {
    XmlChannel(const Configuration&, const char*) {}
    bool isOpen() const { return false; }
    template<class T> XmlChannel& operator<<(const T&) { return *this; }
};
struct ParameterFloat {
    std::string name;
    ParameterFloat(const char* n, const char*, double, double = 0) : name(n) {}
    double operator()(const Configuration&) const { return name == "min-observation" ? ml_min_obs : ml_min_sil; }
    double operator()(const Configuration&, double fromFile) const { return fromFile; }
};
}
typedef void (*gelsd_fn)(int*, int*, int*, double*, int*, double*, int*, double*, double*, int*, double*, int*, int*, int*);
static gelsd_fn ml_gelsd = 0;
namespace Math { namespace Lapack {
inline void dgelsd(s32* m, s32* n, s32* nrhs, f64* a, s32* lda, f64* b, s32* ldb, f64* s, f64* rcond, s32* rank, f64* work, s32* lwork, s32* iwork,
                   s32* info) {
    ml_gelsd(m, n, nrhs, a, lda, b, ldb, s, rcond, rank, work, lwork, iwork, info);
}
// ---- reference text: Svd.hh's constants, pseudoInvert, solveLinearLeastSquares, MatrixTools.hh's pseudoInvert ----
%(svd)s
} }
// ---- shell: Mm/Types.hh's types, Mm::MixtureSet and Am::AdaptationTree as far as the estimators and adaptors read them
namespace Speech { struct Alignment {}; }
namespace Mm {
typedef f32 MeanType;
typedef f32 VarianceType;
typedef f32 FeatureType;
typedef f64 Weight;
typedef f64 Sum;
typedef u32 MixtureIndex;
typedef u32 DensityIndex;
typedef u32 MeanIndex;
typedef u32 CovarianceIndex;
typedef u32 ComponentIndex;
typedef std::string ClusterId;
typedef std::vector<FeatureType> FeatureVector;
typedef std::vector<MeanType>    Mean;   // Mm/GaussDensity.hh:69: class Mean : public std::vector<MeanType>
struct Feature : public Core::ReferenceCounted {
    typedef const FeatureVector* VectorRef;
};
struct GaussDensity {
    MeanIndex       m;
    CovarianceIndex c;
    MeanIndex       meanIndex() const { return m; }
    CovarianceIndex covarianceIndex() const { return c; }
};
struct Covariance {
    std::vector<VarianceType>        d;
    const std::vector<VarianceType>& diagonal() const { return d; }
};
struct Mixture {
    std::vector<DensityIndex> dens;
    size_t       nDensities() const { return dens.size(); }
    DensityIndex densityIndex(size_t i) const { return dens[i]; }
};
struct MixtureSet : public Core::ReferenceCounted {
    ComponentIndex            dim;
    std::vector<Mixture>      mixtures;
    std::vector<GaussDensity> densities;
    mutable std::vector<Mean> means;
    std::vector<Covariance>   covariances;
    ComponentIndex      dimension() const { return dim; }
    MixtureIndex        nMixtures() const { return mixtures.size(); }
    const Mixture*      mixture(MixtureIndex i) const { return &mixtures[i]; }
    const GaussDensity* density(DensityIndex i) const { return &densities[i]; }
    Mean*               mean(MeanIndex i) const { return &means[i]; }
    const Covariance*   covariance(CovarianceIndex i) const { return &covariances[i]; }
};
struct AssigningFeatureScorer : public Core::ReferenceCounted {};
struct AbstractAdaptationAccumulator : public Core::ReferenceCounted {
    virtual ~AbstractAdaptationAccumulator() {}
};
}
namespace Am {
struct MixtureSetAdaptor : public Core::ReferenceCounted {};
struct AdaptationTree : public Core::ReferenceCounted {
    Core::BinaryTree::LeafIndexVector leafIndex_;
    u32                               nLeafs_;
    Core::Ref<Core::BinaryTree>       tree_;
    std::set<Mm::MixtureIndex>        silence_;
    Core::BinaryTree::LeafIndexVector leafIndex() const { return leafIndex_; }
    u32                               nLeafs() const { return nLeafs_; }
    Core::Ref<Core::BinaryTree>       tree() const { return tree_; }
    const std::set<Mm::MixtureIndex>& silenceMixtures() const { return silence_; }
};
}
#define private public
#define protected public
// ---- reference text: Mm/MllrAdaptation.hh ----
%(header)s
// ---- reference text: Mm/MllrAdaptation.cc ----
%(body)s
#undef private
#undef protected
// ---- this generator's own code (no reference text) ----
void ShiftAdaptorViterbiEstimator::accumulate(const Speech::Alignment&, const std::vector<Core::Ref<const Mm::Feature>>&,
                                              Core::Ref<const Am::MixtureSetAdaptor>, Core::Ref<const Mm::AssigningFeatureScorer>) {}
void FullAdaptorViterbiEstimator::accumulate(const Speech::Alignment&, const std::vector<Core::Ref<const Mm::Feature>>&,
                                             Core::Ref<const Am::MixtureSetAdaptor>, Core::Ref<const Mm::AssigningFeatureScorer>) {}
struct MlRun {
    Core::Ref<MixtureSet>                      mixture;
    Core::Ref<Am::AdaptationTree>              tree;
    std::vector<FullAdaptorViterbiEstimator*>  full;
    std::vector<ShiftAdaptorViterbiEstimator*> shift;
    int                                        D, mode, nLeafs;
    AdaptorEstimator* est(int key) { return mode == 0 ? (AdaptorEstimator*)full[key] : (AdaptorEstimator*)shift[key]; }
};
static void ml_dump(const FullAdaptorViterbiEstimator& e, double* flat) {
    for (u32 l = 0; l < e.leafZAccumulators_.size(); ++l) {
        const Matrix z = e.leafZAccumulators_[l].matrix(), g = e.leafGAccumulators_[l].matrix();
        *flat++ = e.leafZAccumulators_[l].count();
        for (u32 i = 0; i < z.nRows(); ++i)
            for (u32 j = 0; j < z.nColumns(); ++j)
                *flat++ = z[i][j];
        *flat++ = e.leafGAccumulators_[l].count();
        for (u32 i = 0; i < g.nRows(); ++i)
            for (u32 j = 0; j < g.nColumns(); ++j)
                *flat++ = g[i][j];
    }
}
static void ml_dump(const ShiftAdaptorViterbiEstimator& e, double* flat) {
    for (u32 l = 0; l < e.countAccumulators_.size(); ++l) {
        *flat++ = e.countAccumulators_[l];
        for (u32 d = 0; d < e.betaAccumulators_[l].size(); ++d)
            *flat++ = e.betaAccumulators_[l][d];
        for (u32 d = 0; d < e.shiftAccumulators_[l].size(); ++d)
            *flat++ = e.shiftAccumulators_[l][d];
    }
}
extern "C" void ml_set_lapack(void* gelsd) { ml_gelsd = (gelsd_fn)gelsd; }
extern "C" void ml_set_thresholds(double obs, double sil) { ml_min_obs = obs, ml_min_sil = sil; }
// the tree from its structure (id, leaf number | invalidId per entry, pre-order), pruned as Am/AdaptationTree.cc:95-99 does
extern "C" void* ml_new(int mode, int D, int n_keys, int n_mix, const unsigned* mix_off, const unsigned* dens_index, int n_dens,
                        const unsigned* dens_mean, const unsigned* dens_cov, int n_mean, const float* means, int n_cov, const float* vars,
                        int n_struct, const int* struct_id, const int* struct_leaf, int base_classes, int n_sil, const int* sil) {
    MlRun* r = new MlRun;
    r->D = D, r->mode = mode;
    MixtureSet* ms = new MixtureSet;
    ms->dim        = D;
    for (int m = 0; m < n_mix; ++m) {
        Mixture mix;
        for (unsigned k = mix_off[m]; k < mix_off[m + 1]; ++k)
            mix.dens.push_back(dens_index[k]);
        ms->mixtures.push_back(mix);
    }
    for (int d = 0; d < n_dens; ++d)
        ms->densities.push_back(GaussDensity{dens_mean[d], dens_cov[d]});
    for (int i = 0; i < n_mean; ++i)
        ms->means.push_back(Mean(means + (size_t)i * D, means + (size_t)(i + 1) * D));
    for (int i = 0; i < n_cov; ++i) {
        Covariance c;
        c.d.assign(vars + (size_t)i * D, vars + (size_t)(i + 1) * D);
        ms->covariances.push_back(c);
    }
    r->mixture = Core::Ref<MixtureSet>(ms);
    Core::BinaryTree::TreeStructure structure;
    for (int i = 0; i < n_struct; ++i)
        structure.push_back(Core::BinaryTree::TreeStructureEntry(struct_id[i], struct_leaf[i] < 0 ? Core::BinaryTree::invalidId : struct_leaf[i]));
    Am::AdaptationTree* at = new Am::AdaptationTree;
    at->tree_              = Core::ref(new Core::BinaryTree(structure));
    at->leafIndex_         = at->tree_->prune(base_classes);
    (*at->leafIndex_).push_back(base_classes);
    at->nLeafs_ = base_classes + 1;
    for (int i = 0; i < n_sil; ++i)
        at->silence_.insert(sil[i]);
    r->tree   = Core::Ref<Am::AdaptationTree>(at);
    r->nLeafs = at->nLeafs_;
    Core::Configuration c;
    for (int k = 0; k < n_keys; ++k) {
        char name[32];
        snprintf(name, sizeof name, "key%%d", k);
        if (mode == 0) {
            r->full.push_back(new FullAdaptorViterbiEstimator(c, Core::Ref<const MixtureSet>(r->mixture), r->tree));
            r->full.back()->clusterId() = name;
        }
        else {
            r->shift.push_back(new ShiftAdaptorViterbiEstimator(c, Core::Ref<const MixtureSet>(r->mixture), r->tree));
            r->shift.back()->clusterId() = name;
        }
    }
    return ml_failed ? 0 : r;
}
extern "C" int ml_leaf_index(void* p, int* out) {
    MlRun* r = (MlRun*)p;
    for (size_t i = 0; i < r->tree->leafIndex_->size(); ++i)
        out[i] = (*r->tree->leafIndex_)[i];
    return r->tree->leafIndex_->size();
}
// the tree as the estimator sees it: n_ids = numberOfNodes + numberOfLeafs; left / right / previous / leaf number for every id below the
// root (-1 elsewhere), the leaf list
extern "C" int ml_tree(void* p, int* root, int* left, int* right, int* previous, int* leaf_number, int* n_leaf_list, int* leaf_list) {
    Core::Ref<Core::BinaryTree> t = ((MlRun*)p)->tree->tree_;
    const int n = t->numberOfNodes() + t->numberOfLeafs();
    for (int i = 0; i < n; ++i)
        left[i] = right[i] = previous[i] = leaf_number[i] = -1;
    *root = t->root();
    std::stack<int> st;
    st.push(t->root());
    while (!st.empty()) {
        const int id = st.top();
        st.pop();
        if (id >= n)
            return -1;
        const int pr = t->previous(id);
        previous[id] = pr == Core::BinaryTree::invalidId ? -1 : pr;
        if (t->isLeaf(id))
            leaf_number[id] = t->leafNumber((Core::BinaryTree::Id)id);
        else {
            left[id] = t->left(id), right[id] = t->right(id);
            st.push(right[id]);
            st.push(left[id]);
        }
    }
    int k = 0;
    for (Core::BinaryTree::LeafList::const_iterator q = t->leafList().begin(); q != t->leafList().end(); ++q)
        leaf_list[k++] = t->id(q);
    *n_leaf_list = k;
    return n;
}
extern "C" void ml_free(void* p) {
    MlRun* r = (MlRun*)p;
    for (size_t i = 0; i < r->full.size(); ++i)
        delete r->full[i];
    for (size_t i = 0; i < r->shift.size(); ++i)
        delete r->shift[i];
    delete r;
}
extern "C" void ml_accumulate(void* p, int key, const float* x, unsigned density, unsigned mixture, int weighted, double weight) {
    MlRun*        r = (MlRun*)p;
    FeatureVector f(x, x + r->D);
    if (weighted)
        r->est(key)->accumulate(&f, density, mixture, r->mixture, weight);
    else
        r->est(key)->accumulate(&f, density, mixture, r->mixture);
}
extern "C" void ml_members(void* p, int key, double* flat) {
    MlRun* r = (MlRun*)p;
    if (r->mode == 0)
        ml_dump(*r->full[key], flat);
    else
        ml_dump(*r->shift[key], flat);
}
// write behind Core::IoRef's tag, read back into a fresh estimator and dump that: 0, or a negative step number
extern "C" int ml_file(void* p, int key, const char* path, double* flat_read, double* thresholds) {
    MlRun* r = (MlRun*)p;
    {
        Core::BinaryOutputStream os(path);
        if (!os)
            return -1;
        os << r->est(key)->typeName();
        if (!r->est(key)->write(os))
            return -2;
    }
    Core::BinaryInputStream is(path);
    std::string             tag;
    is >> tag;
    if (!is || tag != r->est(key)->typeName())
        return -3;
    Core::Configuration c;
    if (r->mode == 0) {
        FullAdaptorViterbiEstimator back(c, r->tree);
        if (!back.read(is))
            return -4;
        ml_dump(back, flat_read);
        thresholds[0] = back.minAdaptationObservations_, thresholds[1] = back.minSilenceObservations_;
        if (back.clusterId() != r->est(key)->clusterId() || back.dimension_ != (u32)r->D)
            return -5;
    }
    else {
        ShiftAdaptorViterbiEstimator back(c, r->tree);
        if (!back.read(is))
            return -4;
        ml_dump(back, flat_read);
        thresholds[0] = back.minAdaptationObservations_, thresholds[1] = back.minSilenceObservations_;
        if (back.clusterId() != r->est(key)->clusterId() || back.dimension_ != (u32)r->D)
            return -5;
    }
    return 0;
}
template<class A>
static int ml_adaptor_out(MlRun* r, Core::Ref<Adaptor> ad, const char* cluster, int* n_mat, int* ids, double* mats, int* index, float* adapted,
                          const char* path, const char* path2) {
    A* a             = dynamic_cast<A*>(ad.get());
    a->clusterId()   = cluster;
    int n            = 0;
    for (MatrixConstIterator q = a->adaptationMatrices_.begin(); q != a->adaptationMatrices_.end(); ++q, ++n) {
        ids[n] = q->first;
        for (u32 i = 0; i < q->second.nRows(); ++i)
            for (u32 j = 0; j < q->second.nColumns(); ++j)
                *mats++ = q->second[i][j];
    }
    *n_mat = n;
    for (size_t m = 0; m < a->adaptationMatrixIndex_.size(); ++m)
        index[m] = a->adaptationMatrixIndex_[m];
    {
        Core::BinaryOutputStream os(path);
        os << a->typeName();
        if (!a->write(os))
            return -2;
    }
    {
        Core::BinaryInputStream is(path);
        std::string             tag;
        is >> tag;
        if (!is || tag != a->typeName())
            return -3;
        Core::Configuration c;
        A                   back(c);
        if (!back.read(is))
            return -4;
        Core::BinaryOutputStream os(path2);
        os << back.typeName();
        if (!back.write(os))
            return -5;
    }
    MixtureSet* copy = new MixtureSet(*r->mixture);   // adaptMixtureSet swaps the means in
    Core::Ref<MixtureSet> ref(copy);
    a->adaptMixtureSet(ref);
    for (size_t i = 0; i < copy->means.size(); ++i)
        for (int d = 0; d < r->D; ++d)
            *adapted++ = copy->means[i][d];
    return 0;
}
// adaptor() on a COPY of the key's estimator (estimateWMatrices erases from w_ / shift_)
extern "C" int ml_estimate(void* p, int key, double min_obs, double min_sil, int* n_mat, int* ids, double* mats, int* index, double* counts,
                           int* n_counts, float* adapted, const char* path, const char* path2) {
    MlRun* r  = (MlRun*)p;
    ml_failed = 0;
    char name[32];
    snprintf(name, sizeof name, "key%%d", key);
    int status;
    if (r->mode == 0) {
        FullAdaptorViterbiEstimator e(*r->full[key]);
        e.minAdaptationObservations_ = min_obs, e.minSilenceObservations_ = min_sil;
        Core::Ref<Adaptor> ad = e.adaptor();
        *n_counts = e.count_.size();
        for (size_t i = 0; i < e.count_.size(); ++i)
            counts[i] = e.count_[i];
        status = ml_adaptor_out<FullAdaptor>(r, ad, name, n_mat, ids, mats, index, adapted, path, path2);
    }
    else {
        ShiftAdaptorViterbiEstimator e(*r->shift[key]);
        e.minAdaptationObservations_ = min_obs, e.minSilenceObservations_ = min_sil;
        Core::Ref<Adaptor> ad = e.adaptor();
        *n_counts = e.count_.size();
        for (size_t i = 0; i < e.count_.size(); ++i)
            counts[i] = e.count_[i];
        status = ml_adaptor_out<ShiftAdaptor>(r, ad, name, n_mat, ids, mats, index, adapted, path, path2);
    }
    return ml_failed ? 1 : status;
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
    return C.cast(L.scipy_dgelsd_, C.c_void_p), L


def build(tmp, flavour, parts, lapack):
    name = "mllr_%s" % flavour
    gen = os.path.join(tmp, name + ".cc")
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, name + ".so")
    lib = "ref" if flavour == "off" else "ref_native"
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen, os.path.join(REF, "Core", "BinaryTree.cc"),
                           "-L" + os.path.join(ROOT, "oracle", "_ref"), "-l" + lib, "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_ref")])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    f32p, f64p, u32p, i32p = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.float32, np.float64, np.uint32, np.int32))
    L.ml_set_lapack.argtypes = [C.c_void_p]
    L.ml_set_thresholds.argtypes = [C.c_double, C.c_double]
    L.ml_new.restype = C.c_void_p
    L.ml_new.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u32p, u32p, C.c_int, u32p, u32p, C.c_int, f32p, C.c_int, f32p, C.c_int, i32p, i32p, C.c_int,
                         C.c_int, i32p]
    L.ml_leaf_index.argtypes = [C.c_void_p, i32p]
    L.ml_tree.argtypes = [C.c_void_p, C.POINTER(C.c_int), i32p, i32p, i32p, i32p, C.POINTER(C.c_int), i32p]
    L.ml_free.argtypes = [C.c_void_p]
    L.ml_accumulate.argtypes = [C.c_void_p, C.c_int, f32p, C.c_uint, C.c_uint, C.c_int, C.c_double]
    L.ml_members.argtypes = [C.c_void_p, C.c_int, f64p]
    L.ml_file.argtypes = [C.c_void_p, C.c_int, C.c_char_p, f64p, f64p]
    L.ml_estimate.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int), i32p, f64p, i32p, f64p, C.POINTER(C.c_int), f32p,
                              C.c_char_p, C.c_char_p]
    L.ml_set_lapack(lapack[0])
    return L, int(fma or 0)


# the unpruned tree: one leaf per non-silence mixture (7), ids in split order so that prune(3) keeps ids 0 .. 4.  (id, leaf | -1), pre-order
STRUCTURE = [(0, -1), (1, -1), (3, -1), (5, 0), (6, 1), (4, -1), (7, 2), (8, 3), (2, -1), (9, -1), (11, 4), (12, 5), (10, 6)]
BASE_CLASSES = 3
N_MIX = 8
SILENCE = [7]
THRESHOLDS = {"low": (45.0, 10.0), "default": (1000.0, 500.0), "silence_high": (45.0, 400.0)}


def cases():
    """name -> dict(model, mode, n_keys, feats, frame_offsets, seg_key, emission, best, weight or None, cut)"""
    from tests import synth
    from tests import mllr_reference as mr
    out = {}
    for mode, mname in ((mr.FULL, "full"), (mr.SHIFT, "shift")):
        for D in (3, 5, 16):
            for weighted in (False, True):
                if mode == mr.SHIFT and D == 16:
                    continue
                seed = 100 * D + 10 * mode + weighted
                rng = np.random.Generator(np.random.PCG64(seed))
                model = synth.gmm_cart(N_MIX, 2, 2, D, seed=seed, pooled=False)
                # key 0: two segments around one of key 2; key 1: no frame; key 2: fewer frames than min-observation
                lens = [90, 6, 110, 5]
                seg_key = np.array([0, 2, 0, 2], np.int32)
                off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                T = int(off[-1])
                feats = (rng.standard_normal((T, D)) * 1.5 + rng.standard_normal(D)).astype(np.float32)
                weight = rng.uniform(0.05, 2.0, T) if weighted else None
                if weighted:
                    weight[[2, T // 2]] = 0.0
                # mixtures 0, 1 (leaf 0) often, 2, 3 (leaf 1) rarely, 4 .. 6 (leaf 2) in between, 7 (silence) some
                emission = rng.choice(N_MIX, T, p=[0.2, 0.2, 0.06, 0.06, 0.1, 0.1, 0.1, 0.18]).astype(np.int32)
                emission[[5, T - 2]] = -1
                best = np.array([rng.integers(0, 2) if e >= 0 else 0xFFFFFFFF for e in emission], np.uint32)
                out["%s/d%d/%s" % (mname, D, "weighted" if weighted else "unweighted")] = dict(
                    model=model, mode=mode, n_keys=3, feats=feats, frame_offsets=off, seg_key=seg_key, emission=emission, best=best, weight=weight,
                    cut=int(off[0] + lens[0] // 2))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_reference(L, c, tmp):
    """everything the reference's text gives for one case in one build"""
    from tests import mllr_reference as mr
    model, mode, n_keys = c["model"], c["mode"], c["n_keys"]
    D = int(model["dim"])
    sid = np.array([s[0] for s in STRUCTURE], np.int32)
    sleaf = np.array([s[1] for s in STRUCTURE], np.int32)
    h = L.ml_new(mode, D, n_keys, N_MIX, np.ascontiguousarray(model["mix_offsets"], np.uint32), np.ascontiguousarray(model["dens_index"], np.uint32),
                 len(model["dens_mean"]), np.ascontiguousarray(model["dens_mean"], np.uint32), np.ascontiguousarray(model["dens_cov"], np.uint32),
                 model["means"].shape[0], np.ascontiguousarray(model["means"], np.float32), model["variances"].shape[0],
                 np.ascontiguousarray(model["variances"], np.float32), len(sid), sid, sleaf, BASE_CLASSES, len(SILENCE), np.array(SILENCE, np.int32))
    assert h
    got = {}
    leaf_index = np.zeros(N_MIX, np.int32)
    assert L.ml_leaf_index(h, leaf_index) == N_MIX
    n_leafs = BASE_CLASSES + 1
    cap = 64
    left, right, prev, leafno, llist = (np.zeros(cap, np.int32) for _ in range(5))
    root, nll = C.c_int(), C.c_int()
    n_ids = L.ml_tree(h, C.byref(root), left, right, prev, leafno, C.byref(nll), llist)
    assert 0 < n_ids <= cap
    tree = dict(root=np.array(root.value), left=left[:n_ids].copy(), right=right[:n_ids].copy(), previous=prev[:n_ids].copy(),
                leaf_number=leafno[:n_ids].copy(), leaf_list=llist[:nll.value].copy(), silence_mixtures=np.array(SILENCE, np.int32))
    got["leaf_of_mixture"] = leaf_index
    for k, v in tree.items():
        got["tree/" + k] = v
    ls = mr.leaf_size(mode, D)
    size = n_leafs * ls
    key_of = np.full(len(c["feats"]), -1)
    for s, k in enumerate(c["seg_key"]):
        key_of[c["frame_offsets"][s]:c["frame_offsets"][s + 1]] = k

    def dump():
        flat = np.zeros(n_keys * size)
        for k in range(n_keys):
            one = np.zeros(size)
            L.ml_members(h, k, one)
            flat[k * size:(k + 1) * size] = one
        return flat

    for t in range(len(c["feats"])):
        if t == c["cut"]:
            got["acc_cut"] = dump()
        e = int(c["emission"][t])
        if e < 0 or key_of[t] < 0:
            continue
        d = int(model["dens_index"][int(model["mix_offsets"][e]) + int(c["best"][t])])
        x = np.ascontiguousarray(c["feats"][t, :D])
        L.ml_accumulate(h, int(key_of[t]), x, d, e, int(c["weight"] is not None), float(c["weight"][t]) if c["weight"] is not None else 1.0)
    got["acc"] = dump()
    L.ml_set_thresholds(*THRESHOLDS["default"])
    for k in (0, 2):
        path = os.path.join(tmp, "acc.bin")
        back, thr = np.zeros(size), np.zeros(2)
        r = L.ml_file(h, k, path.encode(), back, thr)
        assert r == 0, r
        assert same_bits(back, got["acc"][k * size:(k + 1) * size]), "the file does not give the members back"
        with open(path, "rb") as f:
            got["file/key%d" % k] = np.frombuffer(f.read(), np.uint8).copy()
    n_mean = model["means"].shape[0]
    per = D if mode == mr.SHIFT else D * (D + 1)
    for key, names in ((0, ("low", "default", "silence_high")), (2, ("low",))):
        for name in names:
            n, nc = C.c_int(), C.c_int()
            ids, mats, index = np.zeros(cap, np.int32), np.zeros(cap * per), np.zeros(N_MIX, np.int32)
            counts, adapted = np.zeros(cap), np.zeros((n_mean, D), np.float32)
            p1, p2 = os.path.join(tmp, "adaptor.bin"), os.path.join(tmp, "adaptor2.bin")
            r = L.ml_estimate(h, key, THRESHOLDS[name][0], THRESHOLDS[name][1], C.byref(n), ids, mats, index, counts, C.byref(nc), adapted, p1.encode(),
                              p2.encode())
            assert r == 0, r
            assert nc.value == n_ids
            b1, b2 = open(p1, "rb").read(), open(p2, "rb").read()
            assert b1 == b2, "the adaptor file read back and written again differs"
            pre = "est/key%d/%s/" % (key, name)
            got[pre + "matrix_ids"] = ids[:n.value].copy()
            got[pre + "matrices"] = mats[:n.value * per].reshape((n.value, D) if mode == mr.SHIFT else (n.value, D, D + 1)).copy()
            got[pre + "matrix_of_mixture"] = index
            got[pre + "node_count"] = counts[:n_ids].copy()
            got[pre + "adapted_means"] = adapted
            got[pre + "adaptor_file"] = np.frombuffer(b1, np.uint8).copy()
    L.ml_free(h)
    return got, tree, leaf_index


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_mllr.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_mllr_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    from tests import mllr_reference as mr
    lapack = openblas()
    arrays = {}
    for name, (a, b) in THRESHOLDS.items():
        arrays["thresholds/" + name] = np.array([a, b])
    bar = dict(w_abs=0.0, w_rel=0.0)
    ranks = []
    with tempfile.TemporaryDirectory() as tmp:
        libs = {}
        for fl in ("off", "fma"):
            libs[fl], n_fma = build(tmp, fl, parts, lapack)
            arrays["fma_instructions/" + fl] = np.array(n_fma)
        for name, c in cases().items():
            model, mode = c["model"], c["mode"]
            D = int(model["dim"])
            n_leafs = BASE_CLASSES + 1
            size = n_leafs * mr.leaf_size(mode, D)
            for k in ("feats", "frame_offsets", "seg_key", "emission", "best"):
                arrays["%s/%s" % (name, k)] = c[k]
            for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov", "means", "variances", "log_weight"):
                arrays["%s/model/%s" % (name, k)] = model[k]
            arrays[name + "/cut"], arrays[name + "/mode"], arrays[name + "/n_leafs"] = np.array(c["cut"]), np.array(mode), np.array(n_leafs)
            if c["weight"] is not None:
                arrays[name + "/weight"] = np.asarray(c["weight"], np.float64)
            got = {}
            for fl in libs:
                got[fl], tree, leaf_index = run_reference(libs[fl], c, tmp)
            for fl in got:
                for k, v in got[fl].items():
                    if fl == "fma" and same_bits(v, got["off"][k]):
                        arrays["%s/fma/%s_same_as_off" % (name, k)] = np.array(1)
                        continue
                    arrays["%s/%s/%s" % (name, fl, k)] = v
                if mode != mr.FULL:
                    continue
                # the bar and the condition on the inputs: the restatement on the reference's accumulator of this build
                for key, names in ((0, ("low", "silence_high")),):
                    for tname in names:
                        e = mr.estimate(got[fl]["acc"][key * size:(key + 1) * size], tree, leaf_index, mode, D, n_leafs, THRESHOLDS[tname][0],
                                        THRESHOLDS[tname][1], contract=fl)
                        ref = got[fl]["est/key%d/%s/matrices" % (key, tname)]
                        assert np.array_equal(e["matrix_ids"], got[fl]["est/key%d/%s/matrix_ids" % (key, tname)])
                        for a, b in zip(e["matrices"], ref):
                            d = float(np.abs(a - b).max())
                            bar["w_abs"] = max(bar["w_abs"], d)
                            bar["w_rel"] = max(bar["w_rel"], d / float(np.abs(b).max()))
                        for lam in e["eigenvalues"].values():
                            s = np.sort(np.abs(lam))[::-1]
                            rel = s / s[0]
                            assert not np.any((rel >= 1e-14) & (rel <= 1e-10)), "a singular value of an inverted G lies in [1e-14, 1e-10] x the largest: %r" % (rel,)
                            ranks.append((int((rel > 1e-12).sum()), len(s)))
    assert any(r < n for r, n in ranks), "no inverted G is rank-deficient"
    assert any(r == n for r, n in ranks), "no inverted G has full rank"
    arrays["inverted/rank_and_order"] = np.array(ranks)
    for k, v in bar.items():
        arrays["measured/" + k] = np.array(v)
        arrays["bar/" + k] = np.array(4 * v)
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    for k in sorted(arrays):
        if k.startswith(("fma_instructions", "measured/", "bar/")):
            print("  %s = %g" % (k, float(arrays[k])))
    print("  inverted G: %d, rank-deficient %d, full rank %d" % (len(ranks), sum(r < n for r, n in ranks), sum(r == n for r, n in ranks)))
    differ = sorted(k for k in arrays if "/fma/" in k and "same_as_off" not in k)
    print("  fma copies that differ from off: %d" % len(differ))
    for k in differ:
        print("    " + k)


if __name__ == "__main__":
    main()
