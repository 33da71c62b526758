#!/usr/bin/env python3
"""Writes tests/golden/ref_ebw.npz: the EBW corpus pass as the reference's own text computes it, in both of its arithmetics.

What it compiles (the flag sets of oracle/ref/Makefile: -msse3 = contract "off", -msse3 -march=native = contract "fma"), taken by line
range + SHA-256 into a temporary directory that is deleted afterwards, behind stand-ins of this file's own for the types and the classes
around it.  This file holds none of the reference's program text:
  weight_test   Lattice/Accumulator.tcc:71-72         AcousticAccumulator::discoverState's weight test
  collector     Lattice/Accumulator.hh:114-143        Key, KeyHash, KeyEquality, Collector
  functors      Mm/Utilities.hh:108-153               plusWeighted, plusSquare, plusSquareWeighted
  unrolled      Mm/Utilities.hh:204-252               unrolledTransform
  accumulate    Mm/VectorAccumulator.hh:64-67         VectorAccumulator::accumulate(v, weight)
  mix_decl      Mm/MixtureEstimator.hh:59             AbstractMixtureEstimator::accumulate(index, x, weight), its declaration
  mix_num       Mm/MixtureEstimator.cc:92-97          ... and its text: weights_ += weight
  disc_decl     Mm/DiscriminativeMixtureEstimator.hh:53       accumulateDenominator's declaration (virtual)
  disc_den      Mm/DiscriminativeMixtureEstimator.cc:59-66    ... and its text: weights_ -= weight
  ebw_decl      Mm/EbwDiscriminativeMixtureEstimator.hh:53    the EBW class's declaration (virtual)
  ebw_den       Mm/EbwDiscriminativeMixtureEstimator.cc:109-116  ... and its text: denWeights_ += weight, no call of the precursor
  vec_write .. ebw_set_write   every write(Core::BinaryOutputStream&) from EbwDiscriminativeMixtureSetEstimator::write
                (Mm/EbwDiscriminativeMixtureSetEstimator.cc:91-105) through DiscriminativeMixtureSetEstimator::write (:115-119),
                AbstractMixtureSetEstimator::write and writeHeader (Mm/AbstractMixtureSetEstimator.cc:481-509, :416-420), the mixture
                estimators' (Mm/MixtureEstimator.cc:163-170, Mm/EbwDiscriminativeMixtureEstimator.cc:148-154), the density's
                (Mm/GaussDensityEstimator.cc:58-63), the mean's and covariance's (:133-135, :186-188,
                Mm/EbwDiscriminativeGaussDensityEstimator.cc:55-58, :150-153) down to VectorAccumulator::write
                (Mm/VectorAccumulator.hh:96-100), with getWeight / getDenWeight (Mm/MixtureEstimator.hh:65-67,
                Mm/EbwDiscriminativeMixtureEstimator.hh:63-65): the estimator file's bytes, recorded per case
The mixture estimators are called as Mm::DiscriminativeMixtureSetEstimator calls them, through the reference to the base class that its
mixtureEstimator() returns (Mm/DiscriminativeMixtureSetEstimator.hh:35) on an object of the class that
EbwDiscriminativeMixtureSetEstimator::createMixtureEstimator makes: the virtual call reaches the EBW class's text, which does not
subtract the denominator's weight from weights_.  The fixture records that (and, beside it, the slot weights the base class's text would leave: `<case>/<build>/base_class_weights`).
The pass around them is this file's: per segment the denominator accumulator over the arcs with -w, then the numerator accumulator
(Speech/SegmentwiseGmmTrainer.cc:164-166); finish() walks the Collector, and the order in which ITS unordered_map walked is recorded, so
that tests/ebw_reference.py, given that order, is held to the reference in every bit of every accumulator.  read() is not compiled here.
  est_*         the estimate: Mm/IterationConstants.cc:20-733 whole (with the class of IterationConstants.hh:34-76), the estimate, dtSum, dtWeight
                and weight(dns) functions of the EBW mean, covariance and mixture estimators and their i-smoothing variants, the discriminative
                removal, ISmoothingCovarianceEstimator::iSum / getObjectiveFunction, ISmoothingMixtureEstimator::getObjectiveFunction,
                Mixture's weight functions, logExpNorm, applyMinimumVariance, isPositiveDefinite (the ranges are in PIECES).  The driver
                restates DiscriminativeMixtureSetEstimator::estimate and the finalize functions step by step; the walks of the reference's
                hash tables are recorded, bar (b) is measured, the conditions on the cases are asserted (estimate_cases below).

Bar (a), the distance between the library's key order and the reference's hash order: over the cases and both builds the largest
|device order - hash order| / max(1, |hash order|) over the cells; the bar is 4 x that, the project's usual margin, written into the
fixture.  Measured against the reference's text, never against the library.

    python3 tests/golden/make_ebw_golden.py [reference source tree] [--accept: take the text whatever its hash]
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
REF = next((a for a in sys.argv[1:] if not a.startswith("--")), "/root/reference/src")

from tests import ebw_reference as er   # noqa: E402
from tests import synth                 # noqa: E402

PIECES = {
    "weight_test": [("Lattice/Accumulator.tcc", 71, 72)],
    "collector": [("Lattice/Accumulator.hh", 114, 143)],
    "functors": [("Mm/Utilities.hh", 108, 153)],
    "unrolled": [("Mm/Utilities.hh", 204, 252)],
    "accumulate": [("Mm/VectorAccumulator.hh", 64, 67)],
    "mix_decl": [("Mm/MixtureEstimator.hh", 59, 59)],
    "mix_num": [("Mm/MixtureEstimator.cc", 92, 97)],
    "disc_decl": [("Mm/DiscriminativeMixtureEstimator.hh", 53, 53)],
    "disc_den": [("Mm/DiscriminativeMixtureEstimator.cc", 59, 66)],
    "ebw_decl": [("Mm/EbwDiscriminativeMixtureEstimator.hh", 53, 53)],
    "ebw_den": [("Mm/EbwDiscriminativeMixtureEstimator.cc", 109, 116)],
    # the estimator file: every write(Core::BinaryOutputStream&) on the way from the mixture set down to the vector accumulators
    "vec_write": [("Mm/VectorAccumulator.hh", 96, 100)],
    "mean_write": [("Mm/GaussDensityEstimator.cc", 133, 135)],
    "cov_write": [("Mm/GaussDensityEstimator.cc", 186, 188)],
    "dens_write": [("Mm/GaussDensityEstimator.cc", 58, 63)],
    "ebw_mean_write": [("Mm/EbwDiscriminativeGaussDensityEstimator.cc", 55, 58)],
    "ebw_cov_write": [("Mm/EbwDiscriminativeGaussDensityEstimator.cc", 150, 153)],
    "mix_write": [("Mm/MixtureEstimator.cc", 163, 170)],
    "ebw_mix_write": [("Mm/EbwDiscriminativeMixtureEstimator.cc", 148, 154)],
    "mix_weight": [("Mm/MixtureEstimator.hh", 65, 67)],
    "ebw_den_weight": [("Mm/EbwDiscriminativeMixtureEstimator.hh", 63, 65)],
    "set_header": [("Mm/AbstractMixtureSetEstimator.cc", 416, 420)],
    "disc_magic": [("Mm/DiscriminativeMixtureSetEstimator.hh", 42, 44)],
    "set_write": [("Mm/AbstractMixtureSetEstimator.cc", 481, 509)],
    "disc_set_write": [("Mm/DiscriminativeMixtureSetEstimator.cc", 115, 119)],
    "ebw_set_write": [("Mm/EbwDiscriminativeMixtureSetEstimator.cc", 91, 105)],
    # the estimate: all of IterationConstants.cc that is built, the estimators' estimate / dtSum / dtWeight / weight(dns), the removal,
    # the i-smoothing classes' iSum and objective, Mixture's weight functions
    "est_plus_weighted": [("Mm/Utilities.hh", 108, 122)],
    "est_plus_square": [("Mm/Utilities.hh", 124, 133)],
    "est_log_exp_norm": [("Mm/Utilities.hh", 43, 51)],
    "est_positive_definite": [("Mm/GaussDensity.hh", 215, 218)],
    "est_mixture_weight": [("Mm/Mixture.hh", 56, 58)],
    "est_mixture_cc": [("Mm/Mixture.cc", 56, 74), ("Mm/Mixture.cc", 109, 135)],
    "est_disc_mean_hh": [("Mm/DiscriminativeGaussDensityEstimator.hh", 49, 56)],
    "est_disc_cov_hh": [("Mm/DiscriminativeGaussDensityEstimator.hh", 74, 81)],
    "est_ebw_mean_hh": [("Mm/EbwDiscriminativeGaussDensityEstimator.hh", 68, 85)],
    "est_ebw_mean_cc": [("Mm/EbwDiscriminativeGaussDensityEstimator.cc", 73, 105)],
    "est_ebw_mean_is_hh": [("Mm/EbwDiscriminativeGaussDensityEstimator.hh", 108, 110)],
    "est_ebw_mean_is_cc": [("Mm/EbwDiscriminativeGaussDensityEstimator.cc", 114, 121)],
    "est_apply_minimum_variance": [("Mm/GaussDensityEstimator.cc", 227, 235)],
    "est_ebw_cov_getmean_hh": [("Mm/EbwDiscriminativeGaussDensityEstimator.hh", 123, 125)],
    "est_ebw_cov_hh": [("Mm/EbwDiscriminativeGaussDensityEstimator.hh", 142, 154)],
    "est_ebw_cov_cc": [("Mm/EbwDiscriminativeGaussDensityEstimator.cc", 165, 207)],
    "est_is_cov_cc": [("Mm/ISmoothingGaussDensityEstimator.cc", 56, 89)],
    "est_ebw_cov_is_protected_hh": [("Mm/EbwDiscriminativeGaussDensityEstimator.hh", 168, 173)],
    "est_ebw_cov_is_hh": [("Mm/EbwDiscriminativeGaussDensityEstimator.hh", 182, 184)],
    "est_ebw_cov_is_cc": [("Mm/EbwDiscriminativeGaussDensityEstimator.cc", 222, 229)],
    "est_mix_get_weight_hh": [("Mm/MixtureEstimator.hh", 65, 67)],
    "est_abstract_mix_cc": [("Mm/MixtureEstimator.cc", 38, 47), ("Mm/MixtureEstimator.cc", 81, 84)],
    "est_disc_mix_hh": [("Mm/DiscriminativeMixtureEstimator.hh", 58, 61)],
    "est_disc_mix_cc": [("Mm/DiscriminativeMixtureEstimator.cc", 28, 49), ("Mm/DiscriminativeMixtureEstimator.cc", 68, 75)],
    "est_ebw_mix_hh": [("Mm/EbwDiscriminativeMixtureEstimator.hh", 41, 43)],
    "est_ebw_mix_cc": [("Mm/EbwDiscriminativeMixtureEstimator.cc", 34, 91), ("Mm/EbwDiscriminativeMixtureEstimator.cc", 123, 136)],
    "est_is_mix_cc": [("Mm/ISmoothingMixtureEstimator.cc", 34, 37), ("Mm/ISmoothingMixtureEstimator.cc", 54, 61)],
    "est_ebw_mix_is_hh": [("Mm/EbwDiscriminativeMixtureEstimator.hh", 83, 85)],
    "est_ebw_mix_is_cc": [("Mm/EbwDiscriminativeMixtureEstimator.cc", 198, 202)],
    "est_ic_hh": [("Mm/IterationConstants.hh", 34, 76)],
    "est_ic_cc": [("Mm/IterationConstants.cc", 20, 733)],
}
TEXT_SHA256 = "afdd342f9880bdcecc2a409d720c30cc07321121055d5ff7cc4d45b6df146381"

SOURCE = r'''
#include <algorithm>
#include <cstdint>
#include <functional>
#include <iterator>
#include <unordered_map>
#include <vector>
typedef float    f32;
typedef double   f64;
typedef uint32_t u32;
#define require(x)
namespace Speech { typedef u32 TimeframeIndex; }
namespace Mm {
typedef u32 MixtureIndex;
typedef f64 Weight;
typedef f64 Sum;
typedef f32 FeatureType;
%(functors)s
%(unrolled)s
template<class InputType, class PlusOperation, class PlusWeightedOperation>
struct Accumulator {
    typedef Sum          SumType;
    std::vector<SumType> sum_;
    Weight               weight_;
%(accumulate)s
};
// ---- the mixture estimators: stand-ins for the classes, the reference's text for the three functions and two declarations
#define require_(x)
#define required_cast(T, p) static_cast<T>(p)
typedef u32                      DensityIndex;
typedef std::vector<FeatureType> FeatureVector;
struct GaussDensityEstimator {
    int    num_calls = 0, den_calls = 0;
    Weight last      = 0;
    void   accumulate(const FeatureVector&, Weight w) { ++num_calls, last = w; }
};
struct DiscriminativeGaussDensityEstimator : public GaussDensityEstimator {
    void accumulateDenominator(const FeatureVector&, Weight w) { ++den_calls, last = w; }
};
struct DensityRef {   // Core::Ref
    GaussDensityEstimator* p;
    GaussDensityEstimator* get() const { return p; }
    GaussDensityEstimator* operator->() const { return p; }
};
class AbstractMixtureEstimator {
public:
    std::vector<DensityRef> densityEstimators_;
    std::vector<Weight>     weights_;
    virtual ~AbstractMixtureEstimator() {}
    DensityIndex nDensities() const { return densityEstimators_.size(); }
%(mix_decl)s
};
%(mix_num)s
class DiscriminativeMixtureEstimator : public AbstractMixtureEstimator {
public:
    typedef AbstractMixtureEstimator Precursor;
%(disc_decl)s
};
%(disc_den)s
class EbwDiscriminativeMixtureEstimator : public DiscriminativeMixtureEstimator {
public:
    typedef DiscriminativeMixtureEstimator Precursor;
    std::vector<Weight>                    denWeights_;
%(ebw_decl)s
};
%(ebw_den)s
}  // namespace Mm
namespace Lattice {
%(collector)s
struct Arc {
    f32 w;
    f32 weight() const { return w; }
};
struct Walker {
    Mm::Weight weightThreshold_;
    int over(const Arc* a) {
%(weight_test)s
            return 1;
        }
        return 0;
    }
};
}  // namespace Lattice
extern "C" {
int eb_over(float w, double threshold) {
    Lattice::Walker walker;
    walker.weightThreshold_ = threshold;
    Lattice::Arc arc{w};
    return walker.over(&arc);
}
// one accumulator of one segment: the items in the order they are processed; out: the keys as finish() meets them
int eb_collect(int n, const u32* t, const u32* m, const double* w, u32* kt, u32* km, double* kw) {
    Lattice::Collector c;
    for (int i = 0; i < n; ++i)
        c.collect(Lattice::Key(t[i], m[i]), w[i]);
    int k = 0;
    for (Lattice::Collector::const_iterator it = c.begin(); it != c.end(); ++it, ++k)
        kt[k] = it->first.t, km[k] = it->first.m, kw[k] = it->second;
    return k;
}
// one key through the mixture estimator of `n` densities: side 0 accumulate, 1 accumulateDenominator; ebw 1: the class the EBW mixture set
// creates, 0: the base class.  Returns (calls of the density's accumulate) + 16 * (calls of its accumulateDenominator)
int eb_mixture(int ebw, int n, double* weights, double* den_weights, int index, int side, double w) {
    std::vector<Mm::DiscriminativeGaussDensityEstimator> dens(n);
    Mm::EbwDiscriminativeMixtureEstimator                e;
    Mm::DiscriminativeMixtureEstimator                   b;
    Mm::DiscriminativeMixtureEstimator&                  m = ebw ? static_cast<Mm::DiscriminativeMixtureEstimator&>(e) : b;   // mixtureEstimator()
    for (int i = 0; i < n; ++i)
        m.densityEstimators_.push_back(Mm::DensityRef{&dens[i]});
    m.weights_.assign(weights, weights + n);
    e.denWeights_.assign(den_weights, den_weights + n);
    Mm::FeatureVector x(1, 0.f);
    if (side)
        m.accumulateDenominator(index, x, w);
    else
        m.accumulate(index, x, w);
    std::copy(m.weights_.begin(), m.weights_.end(), weights);
    if (ebw)
        std::copy(e.denWeights_.begin(), e.denWeights_.end(), den_weights);
    return dens[index].last == w ? dens[index].num_calls + 16 * dens[index].den_calls : -1;
}
void eb_accumulate(int square, int dim, double* sum, double* weight, const float* x, double w) {
    std::vector<f32> v(x, x + dim);
    if (square) {
        Mm::Accumulator<Mm::FeatureType, Mm::plusSquare<Mm::Sum>, Mm::plusSquareWeighted<Mm::Sum>> a;
        a.sum_.assign(sum, sum + dim), a.weight_ = *weight;
        a.accumulate(v, w);
        std::copy(a.sum_.begin(), a.sum_.end(), sum), *weight = a.weight_;
    }
    else {
        Mm::Accumulator<Mm::FeatureType, std::plus<Mm::Sum>, Mm::plusWeighted<Mm::Sum>> a;
        a.sum_.assign(sum, sum + dim), a.weight_ = *weight;
        a.accumulate(v, w);
        std::copy(a.sum_.begin(), a.sum_.end(), sum), *weight = a.weight_;
    }
}
}
'''

# the estimator file.  Stand-ins: the stream (bytes as a little-endian Core::BinaryOutputStream leaves them), Core::Ref, the index maps (the
# model's own index order, which is what the reference's maps give an estimator built from that model), the class skeletons
SOURCE_FILE = r'''
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <numeric>
#include <string>
#include <vector>
typedef float    f32;
typedef double   f64;
typedef uint32_t u32;
namespace Core {
class BinaryOutputStream {
public:
    std::string buf;
    void        write(const char* p, size_t n) { buf.append(p, n); }
    template<class T>
    struct Iterator {
        typedef std::output_iterator_tag iterator_category;
        typedef void value_type; typedef std::ptrdiff_t difference_type; typedef void pointer; typedef void reference;
        BinaryOutputStream* o;
        explicit Iterator(BinaryOutputStream& s) : o(&s) {}
        Iterator& operator*() { return *this; }
        Iterator& operator++() { return *this; }
        Iterator  operator++(int) { return *this; }
        Iterator& operator=(const T& v);
    };
};
inline BinaryOutputStream& operator<<(BinaryOutputStream& o, u32 v) { o.write((const char*)&v, 4); return o; }
inline BinaryOutputStream& operator<<(BinaryOutputStream& o, f64 v) { o.write((const char*)&v, 8); return o; }
template<class T> BinaryOutputStream::Iterator<T>& BinaryOutputStream::Iterator<T>::operator=(const T& v) { *o << v; return *this; }
template<class T> struct Ref {
    T* p;
    Ref(T* q = 0) : p(q) {}
    T* get() const { return p; }
    T* operator->() const { return p; }
    bool operator==(const Ref& r) const { return p == r.p; }
};
struct Log { template<class T> Log& operator<<(const T&) { return *this; } };
}  // namespace Core
namespace Mm {
typedef u32 MeanIndex; typedef u32 CovarianceIndex; typedef u32 DensityIndex; typedef u32 MixtureIndex; typedef u32 ComponentIndex;
typedef f64 Weight; typedef f64 Sum;
template<class T> struct ReferenceIndexMap {
    std::vector<Core::Ref<T>> v;
    size_t             size() const { return v.size(); }
    const Core::Ref<T>& operator[](u32 i) const { return v[i]; }
    u32                operator[](const Core::Ref<T>& r) const { return (u32)(std::find(v.begin(), v.end(), r) - v.begin()); }
};
struct Accumulator {
    typedef Sum          SumType;
    std::vector<SumType> sum_;
    Weight               weight_;
%(vec_write)s
};
struct AbstractMeanEstimator { virtual ~AbstractMeanEstimator() {} virtual void write(Core::BinaryOutputStream&) const = 0; };
struct MeanEstimator : AbstractMeanEstimator { Accumulator accumulator_; virtual void write(Core::BinaryOutputStream&) const; };
%(mean_write)s
struct DiscriminativeMeanEstimator : MeanEstimator {};
struct EbwDiscriminativeMeanEstimator : DiscriminativeMeanEstimator {
    typedef DiscriminativeMeanEstimator Precursor;
    Accumulator  denAccumulator_;
    virtual void write(Core::BinaryOutputStream&) const;
};
%(ebw_mean_write)s
struct AbstractCovarianceEstimator { virtual ~AbstractCovarianceEstimator() {} virtual void write(Core::BinaryOutputStream&) const = 0; };
struct CovarianceEstimator : AbstractCovarianceEstimator { Accumulator accumulator_; virtual void write(Core::BinaryOutputStream&) const; };
%(cov_write)s
struct DiscriminativeCovarianceEstimator : CovarianceEstimator {};
struct EbwDiscriminativeCovarianceEstimator : DiscriminativeCovarianceEstimator {
    typedef DiscriminativeCovarianceEstimator Precursor;
    Accumulator  denAccumulator_;
    virtual void write(Core::BinaryOutputStream&) const;
};
%(ebw_cov_write)s
struct GaussDensityEstimator {
    Core::Ref<AbstractMeanEstimator>       meanEstimator_;
    Core::Ref<AbstractCovarianceEstimator> covarianceEstimator_;
    virtual ~GaussDensityEstimator() {}
    virtual void write(Core::BinaryOutputStream&, const ReferenceIndexMap<AbstractMeanEstimator>&, const ReferenceIndexMap<AbstractCovarianceEstimator>&) const;
};
%(dens_write)s
struct AbstractMixtureEstimator {
    std::vector<Core::Ref<GaussDensityEstimator>> densityEstimators_;
    std::vector<Weight>                           weights_;
    virtual ~AbstractMixtureEstimator() {}
    virtual void write(Core::BinaryOutputStream&, const ReferenceIndexMap<GaussDensityEstimator>&) const;
%(mix_weight)s
};
%(mix_write)s
struct DiscriminativeMixtureEstimator : AbstractMixtureEstimator {};
struct EbwDiscriminativeMixtureEstimator : DiscriminativeMixtureEstimator {
    typedef DiscriminativeMixtureEstimator Precursor;
    std::vector<Weight> denWeights_;
    virtual void write(Core::BinaryOutputStream&, const ReferenceIndexMap<GaussDensityEstimator>&) const;
%(ebw_den_weight)s
};
%(ebw_mix_write)s
struct AbstractMixtureSetEstimator;
struct MixtureSetEstimatorIndexMap {
    const AbstractMixtureSetEstimator& s;
    MixtureSetEstimatorIndexMap(const AbstractMixtureSetEstimator& e) : s(e) {}
    const ReferenceIndexMap<AbstractMeanEstimator>&       meanMap() const;
    const ReferenceIndexMap<AbstractCovarianceEstimator>& covarianceMap() const;
    const ReferenceIndexMap<GaussDensityEstimator>&       densityMap() const;
};
struct AbstractMixtureSetEstimator {
    u32                                              version_ = 2;
    ComponentIndex                                   dimension_ = 0;
    std::vector<Core::Ref<AbstractMixtureEstimator>> mixtureEstimators_;
    ReferenceIndexMap<AbstractMeanEstimator>         means;
    ReferenceIndexMap<AbstractCovarianceEstimator>   covs;
    ReferenceIndexMap<GaussDensityEstimator>         dens;
    virtual ~AbstractMixtureSetEstimator() {}
    virtual const std::string magic() const = 0;
    Core::Log         log(const char* = "") const { return Core::Log(); }
    void              writeHeader(Core::BinaryOutputStream&);
    virtual void      write(Core::BinaryOutputStream&);
    AbstractMixtureEstimator& mixtureEstimator(MixtureIndex m) { return *mixtureEstimators_[m].get(); }
};
const ReferenceIndexMap<AbstractMeanEstimator>&       MixtureSetEstimatorIndexMap::meanMap() const { return s.means; }
const ReferenceIndexMap<AbstractCovarianceEstimator>& MixtureSetEstimatorIndexMap::covarianceMap() const { return s.covs; }
const ReferenceIndexMap<GaussDensityEstimator>&       MixtureSetEstimatorIndexMap::densityMap() const { return s.dens; }
%(set_header)s
%(set_write)s
struct DiscriminativeMixtureSetEstimator : AbstractMixtureSetEstimator {
    typedef AbstractMixtureSetEstimator Precursor;
%(disc_magic)s
    Sum          objectiveFunction_ = 0;
    Sum          objectiveFunction() const { return objectiveFunction_; }
    virtual void write(Core::BinaryOutputStream&);
};
%(disc_set_write)s
struct EbwDiscriminativeMixtureSetEstimator : DiscriminativeMixtureSetEstimator {
    typedef DiscriminativeMixtureSetEstimator Precursor;
    virtual void write(Core::BinaryOutputStream&);
    EbwDiscriminativeMixtureEstimator& mixtureEstimator(MixtureIndex m) { return *static_cast<EbwDiscriminativeMixtureEstimator*>(mixtureEstimators_[m].get()); }
};
%(ebw_set_write)s
}  // namespace Mm
extern "C" long eb_file(int dim, int n_mix, int n_dens, int n_mean, int n_cov, const u32* mix_off, const u32* dens_index, const u32* dens_mean,
                        const u32* dens_cov, const double* acc, char* out, long capacity) {
    using namespace Mm;
    const long nk = mix_off[n_mix], block = nk + (long)(n_mean + n_cov) * (1 + dim);
    std::vector<EbwDiscriminativeMeanEstimator>       means(n_mean);
    std::vector<EbwDiscriminativeCovarianceEstimator> covs(n_cov);
    std::vector<GaussDensityEstimator>                dens(n_dens);
    std::vector<EbwDiscriminativeMixtureEstimator>    mixes(n_mix);
    EbwDiscriminativeMixtureSetEstimator              set;
    set.dimension_ = dim;
    for (int side = 0; side < 2; ++side) {
        const double* b = acc + side * block;   // [slot weights | mean weights | mean sums | covariance weights | covariance sums]
        for (int i = 0; i < n_mean; ++i) {
            Accumulator& a = side ? means[i].denAccumulator_ : means[i].accumulator_;
            a.weight_ = b[nk + i], a.sum_.assign(b + nk + n_mean + (long)i * dim, b + nk + n_mean + (long)(i + 1) * dim);
        }
        const double* c = b + nk + (long)n_mean * (1 + dim);
        for (int i = 0; i < n_cov; ++i) {
            Accumulator& a = side ? covs[i].denAccumulator_ : covs[i].accumulator_;
            a.weight_ = c[i], a.sum_.assign(c + n_cov + (long)i * dim, c + n_cov + (long)(i + 1) * dim);
        }
    }
    for (int i = 0; i < n_mean; ++i) set.means.v.push_back(&means[i]);
    for (int i = 0; i < n_cov; ++i) set.covs.v.push_back(&covs[i]);
    for (int d = 0; d < n_dens; ++d) {
        dens[d].meanEstimator_ = &means[dens_mean[d]], dens[d].covarianceEstimator_ = &covs[dens_cov[d]];
        set.dens.v.push_back(&dens[d]);
    }
    for (int m = 0; m < n_mix; ++m) {
        for (u32 k = mix_off[m]; k < mix_off[m + 1]; ++k) {
            mixes[m].densityEstimators_.push_back(&dens[dens_index[k]]);
            mixes[m].weights_.push_back(acc[k]);
            mixes[m].denWeights_.push_back(acc[block + k]);
        }
        set.mixtureEstimators_.push_back(&mixes[m]);
    }
    set.objectiveFunction_ = acc[2 * block];
    Core::BinaryOutputStream os;
    static_cast<AbstractMixtureSetEstimator&>(set).write(os);   // a virtual call, as the trainer's write() makes it
    if ((long)os.buf.size() <= capacity)
        memcpy(out, os.buf.data(), os.buf.size());
    return (long)os.buf.size();
}
'''

# the estimate.  Stand-ins: Core (Ref, Component, the parameters, the log and XML sinks), the numeric types, the class skeletons; every
# function body that computes is the reference's.  verify / require / ensure do not abort here: they set a flag that the driver returns.
# The driver at the end restates DiscriminativeMixtureSetEstimator::estimate and the two finalize functions step by step.
SOURCE_EST = r'''
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <iostream>
#include <iterator>
#include <map>
#include <numeric>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
typedef float    f32;
typedef double   f64;
typedef uint32_t u32;
typedef int32_t  s32;
// what the reference would abort on is recorded instead: 1 verify, 2 require, 4 ensure, 8 defect
static int eb_failed = 0;
#define verify(x) do { if (!(x)) eb_failed |= 1; } while (0)
#define verify_(x) verify(x)
#define require(x) do { if (!(x)) eb_failed |= 2; } while (0)
#define require_(x) require(x)
#define ensure(x) do { if (!(x)) eb_failed |= 4; } while (0)
#define defect() do { eb_failed |= 8; } while (0)
#define required_cast(T, p) static_cast<T>(p)
namespace Core {
template<class T> struct Type;
template<> struct Type<f64> {
    static constexpr f64 max = +1.7976931348623157e+308, min = -1.7976931348623157e+308, epsilon = 2.2204460492503131e-16, delta = 2.2250738585072014e-308;
};
template<> struct Type<f32> {
    static constexpr f32 max = +3.40282347e+38F, min = -3.40282347e+38F, epsilon = 1.19209290e-07F, delta = 1.17549435e-38F;
};
template<class T> class Ref {
    T* p_;
public:
    Ref() : p_(0) {}
    Ref(T* p) : p_(p) {}
    template<class S> Ref(const Ref<S>& r) : p_(r.get()) {}
    T*   get() const { return p_; }
    T*   operator->() const { return p_; }
    T&   operator*() const { return *p_; }
    bool operator==(const Ref& r) const { return p_ == r.p_; }
    explicit operator bool() const { return p_ != 0; }
};
struct Configuration { std::map<std::string, double> v; };
struct ParameterFloat {
    std::string name; double def;
    ParameterFloat(const char* n, const char*, double d = 0, double = 0, double = 0) : name(n), def(d) {}
    double operator()(const Configuration& c) const { auto it = c.v.find(name); return it == c.v.end() ? def : it->second; }
    double operator()(const Configuration& c, double d) const { auto it = c.v.find(name); return it == c.v.end() ? d : it->second; }
};
struct Choice {
    template<class... A> Choice(A...) {}
    static int endMark() { return -1; }
};
struct ParameterChoice {
    std::string name; int def;
    ParameterChoice(const char* n, const Choice*, const char*, int d) : name(n), def(d) {}
    int operator()(const Configuration& c) const { auto it = c.v.find(name); return it == c.v.end() ? def : (int)it->second; }
};
struct Log { template<class T> Log& operator<<(const T&) { return *this; } };
struct XmlOpen { XmlOpen(const char*) {} };
struct XmlClose { XmlClose(const char*) {} };
struct NullBuf : std::streambuf { int overflow(int c) override { return c; } };
class XmlWriter : public std::ostream {
    NullBuf b_;
public:
    XmlWriter() : std::ostream(&b_) {}
};
inline XmlWriter& operator<<(XmlWriter& o, const XmlOpen&) { return o; }
inline XmlWriter& operator<<(XmlWriter& o, const XmlClose&) { return o; }
inline std::string form(const char*, ...) { return std::string(); }
template<class T> T abs(T v) { return v < 0 ? -v : v; }
class Component {
protected:
    Configuration config;
public:
    Component(const Configuration& c) : config(c) {}
    virtual ~Component() {}
    Log                  log(const char* = "") const { return Log(); }
    const Configuration& select(const char*) const { return config; }
    XmlWriter&           clog() const { static XmlWriter w; return w; }
};
struct Application {
    static Application* us() { static Application a; return &a; }
    Log log(const char* = "") { return Log(); }
    Log warning(const char* = "") { return Log(); }
};
}  // namespace Core
namespace Mm {
typedef u32 MixtureIndex; typedef u32 DensityIndex; typedef u32 MeanIndex; typedef u32 CovarianceIndex; typedef u32 ComponentIndex;
typedef f64 Weight; typedef f64 Sum; typedef f64 IterationConstant;
typedef f32 FeatureType; typedef f32 MeanType; typedef f32 VarianceType;
template<class T> struct hashReference { size_t operator()(const Core::Ref<T>& r) const { return reinterpret_cast<size_t>(r.get()); } };
%(est_plus_weighted)s
%(est_plus_square)s
%(est_log_exp_norm)s
struct VecAcc {
    typedef Sum      SumType;
    std::vector<Sum> sum_;
    Weight           weight_ = 0;
    size_t                  size() const { return sum_.size(); }
    const std::vector<Sum>& sum() const { return sum_; }
    Weight                  weight() const { return weight_; }
};
class Mean : public std::vector<MeanType> {
    typedef std::vector<MeanType> Precursor;
public:
    Mean(ComponentIndex dimension = 0, MeanType value = 0) : Precursor(dimension, value) {}
    Mean(const Precursor& v) : Precursor(v) {}
    virtual ~Mean() {}
};
class Covariance {
public:
    virtual ~Covariance() {}
    virtual const std::vector<VarianceType>& diagonal() const = 0;
};
class DiagonalCovariance : public Covariance {
public:
    std::vector<VarianceType> buffer_;
    DiagonalCovariance(const std::vector<VarianceType>& b) : buffer_(b) {}
    virtual const std::vector<VarianceType>& diagonal() const { return buffer_; }
%(est_positive_definite)s
};
class AbstractMixture {
protected:
    std::vector<DensityIndex> densityIndices_;
public:
    virtual ~AbstractMixture() {}
    DensityIndex nDensities() const { return densityIndices_.size(); }
    DensityIndex densityIndex(DensityIndex i) const { return densityIndices_[i]; }
    void         addDensity(DensityIndex i) { densityIndices_.push_back(i); }
    void         removeDensity(DensityIndex i) { densityIndices_.erase(densityIndices_.begin() + i); }
};
class Mixture : public AbstractMixture {
    typedef AbstractMixture Precursor;
    std::vector<Weight> logWeights_;
public:
    void addLogDensity(DensityIndex index, Weight logWeight);
    void addDensity(DensityIndex index, Weight weight);
    void normalizeWeights();
%(est_mixture_weight)s
    Weight       logWeight(DensityIndex i) const { return logWeights_[i]; }
    DensityIndex densityIndexWithMaxWeight() const;
    void         removeDensitiesWithLowWeight(Weight minWeight, bool normalizeWeights);
    void         removeDensity(DensityIndex index);
};
%(est_mixture_cc)s
class AbstractEstimationAccumulator { public: virtual ~AbstractEstimationAccumulator() {} };
class AbstractMeanEstimator : public AbstractEstimationAccumulator {};
class AbstractCovarianceEstimator : public AbstractEstimationAccumulator {};
class CovarianceToMeanSetMap {
public:
    typedef std::unordered_set<Core::Ref<AbstractMeanEstimator>, hashReference<AbstractMeanEstimator>> MeanSet;
    std::unordered_map<Core::Ref<AbstractCovarianceEstimator>, MeanSet, hashReference<AbstractCovarianceEstimator>> map_;
    const MeanSet& operator[](Core::Ref<AbstractCovarianceEstimator> e) const { return map_.find(e)->second; }
};
template<class T> class ReferenceIndexMap {
public:
    std::vector<Core::Ref<T>> v;
    size_t              size() const { return v.size(); }
    const Core::Ref<T>& operator[](u32 i) const { return v[i]; }
    u32                 operator[](const Core::Ref<T>& r) const { return (u32)(std::find(v.begin(), v.end(), r) - v.begin()); }
    void                add(const Core::Ref<T>& r) { if (std::find(v.begin(), v.end(), r) == v.end()) v.push_back(r); }
};
// ---- means
class MeanEstimator : public AbstractMeanEstimator {
public:
    typedef VecAcc Accumulator;
    Accumulator    accumulator_;
    MeanEstimator(ComponentIndex d = 0) { accumulator_.sum_.resize(d); }
    const std::vector<Accumulator::SumType>& sum() const { return accumulator_.sum(); }
    virtual Weight                           weight() const { return accumulator_.weight(); }
};
class DiscriminativeMeanEstimator : public MeanEstimator {
public:
    std::vector<MeanType> previousMean_;
    DiscriminativeMeanEstimator(ComponentIndex d = 0) : MeanEstimator(d) {}
%(est_disc_mean_hh)s
};
class EbwDiscriminativeMeanEstimator : public DiscriminativeMeanEstimator {
public:
    Accumulator       denAccumulator_;
    IterationConstant iterationConstant_;
    EbwDiscriminativeMeanEstimator(ComponentIndex d = 0) : DiscriminativeMeanEstimator(d), iterationConstant_(1) { denAccumulator_.sum_.resize(d); }
    virtual Mean* estimate();
%(est_ebw_mean_hh)s
    void setIterationConstant(IterationConstant);
};
%(est_ebw_mean_cc)s
class ISmoothingMeanEstimator {
    std::vector<MeanType> iMean_;
    Weight                constant_;
public:
    ISmoothingMeanEstimator() : constant_(0) {}
    virtual ~ISmoothingMeanEstimator() {}
    void                         setIMean(const std::vector<MeanType>& m) { iMean_ = m; }
    const std::vector<MeanType>& iMean() const { return iMean_; }
    MeanType                     iMean(ComponentIndex i) const { return iMean_[i]; }
    void                         setConstant(Weight c) { constant_ = c; }
    Weight                       constant() const { return constant_; }
};
class EbwDiscriminativeMeanEstimatorWithISmoothing : public EbwDiscriminativeMeanEstimator, public ISmoothingMeanEstimator {
    typedef EbwDiscriminativeMeanEstimator Precursor;
protected:
    typedef ISmoothingMeanEstimator ISmoothing;
public:
    EbwDiscriminativeMeanEstimatorWithISmoothing(ComponentIndex d = 0) : Precursor(d) {}
    virtual std::vector<Accumulator::SumType> dtSum() const;
%(est_ebw_mean_is_hh)s
};
%(est_ebw_mean_is_cc)s
// ---- covariances
class CovarianceEstimator : public AbstractCovarianceEstimator {
public:
    typedef VecAcc Accumulator;
    Accumulator    accumulator_;
    CovarianceEstimator(ComponentIndex d = 0) { accumulator_.sum_.resize(d); }
    const std::vector<Accumulator::SumType>& sum() const { return accumulator_.sum(); }
    virtual Weight                           weight() const { return accumulator_.weight(); }
    void applyMinimumVariance(VarianceType minimumVariance, DiagonalCovariance& result) const;
};
%(est_apply_minimum_variance)s
class DiscriminativeCovarianceEstimator : public CovarianceEstimator {
public:
    std::vector<VarianceType> previousCovariance_;
    DiscriminativeCovarianceEstimator(ComponentIndex d = 0) : CovarianceEstimator(d) {}
%(est_disc_cov_hh)s
};
class EbwDiscriminativeCovarianceEstimator : public DiscriminativeCovarianceEstimator {
public:
    Accumulator denAccumulator_;
protected:
%(est_ebw_cov_getmean_hh)s
public:
    EbwDiscriminativeCovarianceEstimator(ComponentIndex d = 0) : DiscriminativeCovarianceEstimator(d) { denAccumulator_.sum_.resize(d); }
    virtual Covariance* estimate(const CovarianceToMeanSetMap&, VarianceType minimumVariance);
%(est_ebw_cov_hh)s
};
%(est_ebw_cov_cc)s
class ISmoothingCovarianceEstimator {
protected:
    typedef VecAcc Accumulator;
private:
    Core::Ref<DiscriminativeCovarianceEstimator> parent_;
    std::vector<VarianceType>                    iCovariance_;
    Weight                                       constant_;
    mutable std::vector<Accumulator::SumType>*   iSum_;
protected:
    virtual const std::vector<MeanType>& iMean(Core::Ref<AbstractMeanEstimator>) const = 0;
public:
    ISmoothingCovarianceEstimator() : constant_(0), iSum_(0) {}
    virtual ~ISmoothingCovarianceEstimator() { delete iSum_; }
    void set(Core::Ref<DiscriminativeCovarianceEstimator> parent) { parent_ = parent; }
    void setICovariance(const std::vector<VarianceType>& v) { iCovariance_ = v; }
    const std::vector<VarianceType>& iCovariance() const { return iCovariance_; }
    Accumulator::SumType iSum(const CovarianceToMeanSetMap::MeanSet&, ComponentIndex i) const;
    Sum                  getObjectiveFunction(const CovarianceToMeanSetMap&);
    void   setConstant(Weight c) { constant_ = c; }
    Weight constant() const { return constant_; }
};
%(est_is_cov_cc)s
class EbwDiscriminativeCovarianceEstimatorWithISmoothing : public EbwDiscriminativeCovarianceEstimator, public ISmoothingCovarianceEstimator {
    typedef EbwDiscriminativeCovarianceEstimator Precursor;
protected:
    typedef ISmoothingCovarianceEstimator ISmoothing;
%(est_ebw_cov_is_protected_hh)s
public:
    EbwDiscriminativeCovarianceEstimatorWithISmoothing(ComponentIndex d = 0) : Precursor(d) { ISmoothing::set(Core::Ref<DiscriminativeCovarianceEstimator>(this)); }
    virtual std::vector<Precursor::Accumulator::SumType> dtSum(const CovarianceToMeanSetMap::MeanSet&) const;
%(est_ebw_cov_is_hh)s
};
%(est_ebw_cov_is_cc)s
// ---- densities
class GaussDensityEstimator {
public:
    Core::Ref<AbstractMeanEstimator>       meanEstimator_;
    Core::Ref<AbstractCovarianceEstimator> covarianceEstimator_;
    virtual ~GaussDensityEstimator() {}
    Core::Ref<AbstractMeanEstimator>       mean() const { return meanEstimator_; }
    Core::Ref<AbstractCovarianceEstimator> covariance() const { return covarianceEstimator_; }
};
class DiscriminativeGaussDensityEstimator : public GaussDensityEstimator {};
class EbwDiscriminativeGaussDensityEstimator : public DiscriminativeGaussDensityEstimator {
public:
    void setIterationConstant(IterationConstant);
};
// this file's own in place of Mm/EbwDiscriminativeGaussDensityEstimator.cc:23-25 (a one-line forwarder): it also records the order in which
// IterationConstants::set walks the reference's hash tables (covariance by covariance, density by density)
static std::vector<const void*> eb_dens_walk;
void EbwDiscriminativeGaussDensityEstimator::setIterationConstant(IterationConstant ic) {
    eb_dens_walk.push_back(this);
    required_cast(EbwDiscriminativeMeanEstimator*, meanEstimator_.get())->setIterationConstant(ic);
}
// ---- mixtures
class AbstractMixtureEstimator {
public:
    typedef std::vector<Core::Ref<GaussDensityEstimator>> DensityEstimators;
    DensityEstimators   densityEstimators_;
    std::vector<Weight> weights_;
    virtual ~AbstractMixtureEstimator() {}
    DensityIndex             nDensities() const { return densityEstimators_.size(); }
    const DensityEstimators& densityEstimators() const { return densityEstimators_; }
    DensityIndex             densityIndexWithMaxWeight() const;
    virtual void             removeDensity(DensityIndex indexInMixture);
%(est_mix_get_weight_hh)s
};
%(est_abstract_mix_cc)s
class DiscriminativeMixtureEstimator : public AbstractMixtureEstimator {
    typedef AbstractMixtureEstimator Precursor;
public:
    std::vector<Weight> previousMixtureWeights_;
    virtual void removeDensity(DensityIndex indexInMixture);
    virtual void removeDensitiesWithLowWeight(Weight minObservationWeight, Weight minRelativeWeight = 0);
%(est_disc_mix_hh)s
    Weight logPreviousMixtureWeight(DensityIndex dns) const;
};
%(est_disc_mix_cc)s
class EbwDiscriminativeMixtureEstimator : public DiscriminativeMixtureEstimator {
    typedef DiscriminativeMixtureEstimator Precursor;
public:
    std::vector<Weight> denWeights_;
    u32                 nIterations_ = 100;
    virtual void removeDensity(DensityIndex indexInMixture);
    void         estimateMixtureWeights(std::vector<Weight>&, bool normalizeWeights = true) const;
%(est_ebw_mix_hh)s
    virtual Mixture* estimate(const ReferenceIndexMap<GaussDensityEstimator>& densityMap, bool normalizeWeights = true);
};
%(est_ebw_mix_cc)s
class ISmoothingMixtureEstimator {
    DiscriminativeMixtureEstimator* parent_;
public:
    std::vector<Weight> iMixtureWeights_;
private:
    Weight constant_;
protected:
    virtual void removeDensity(DensityIndex indexInMixture);
public:
    ISmoothingMixtureEstimator() : parent_(0), constant_(0) {}
    virtual ~ISmoothingMixtureEstimator() {}
    void           set(DiscriminativeMixtureEstimator* p) { parent_ = p; }
    Sum            getObjectiveFunction() const;
    virtual Weight iMixtureWeight(DensityIndex dns) const { return iMixtureWeights_[dns]; }
    void           setConstant(Weight c) { constant_ = c; }
    Weight         constant() const { return constant_; }
    u32            nMixtureWeights() const { return iMixtureWeights_.size(); }
};
%(est_is_mix_cc)s
class EbwDiscriminativeMixtureEstimatorWithISmoothing : public EbwDiscriminativeMixtureEstimator, public ISmoothingMixtureEstimator {
    typedef EbwDiscriminativeMixtureEstimator Precursor;
protected:
    typedef ISmoothingMixtureEstimator ISmoothing;
public:
    EbwDiscriminativeMixtureEstimatorWithISmoothing() { ISmoothing::set(this); }
    virtual void removeDensity(DensityIndex indexInMixture);
%(est_ebw_mix_is_hh)s
};
%(est_ebw_mix_is_cc)s
struct AbstractMixtureSetEstimator { typedef std::vector<Core::Ref<AbstractMixtureEstimator>> MixtureEstimators; };
}  // namespace Mm
namespace InternalIc {
struct AugmentedDensityEstimator;
class CovarianceToDensitySetMap;
}  // namespace InternalIc
namespace Mm {
%(est_ic_hh)s
}  // namespace Mm
using namespace Mm;
%(est_ic_cc)s

// ------------------------------------------------------------------------------------------------ the driver (this file's own)
extern "C" int eb_estimate(int dim, int n_mix, int n_dens, int n_mean, int n_cov, const u32* mix_off, const u32* dens_index, const u32* dens_mean,
                           const u32* dens_cov, const double* acc, const double* prev_logw, const float* prev_means, const float* prev_vars,
                           int ism, const double* i_logw, const float* i_means, const float* i_vars, const double* cfg,
                           u32* o_counts /* n_dens, n_mean, n_cov, n_slots */, u32* o_mix_off, u32* o_dens_index, double* o_logw, u32* o_dens_old,
                           u32* o_mean_old, u32* o_cov_old, float* o_means, float* o_vars, double* o_icd, double* o_objective,
                           s32* o_cov_walk, s32* o_cov_dens_walk /* [n_dens]: densities in cim order */, s32* o_cov_mean_walk /* [n_mean] */,
                           s32* o_cov_mean_count /* [n_cov] by walk */) {
    eb_failed = 0;
    eb_dens_walk.clear();
    const long nk = mix_off[n_mix], block = nk + (long)(n_mean + n_cov) * (1 + dim);
    const double min_obs = cfg[0], min_rel = cfg[1], min_var = cfg[2];
    const bool   normalize = cfg[3] != 0;
    Core::Configuration config;
    config.v["type"] = cfg[4], config.v["step-size"] = cfg[5], config.v["minimum-icd"] = cfg[6], config.v["beta"] = cfg[7];
    if (!std::isnan(cfg[8]))
        config.v["sigma-minimum"] = cfg[8];
    config.v["sigma-minimum-factor"] = cfg[9];
    std::vector<EbwDiscriminativeMeanEstimator*>         means(n_mean);
    std::vector<EbwDiscriminativeCovarianceEstimator*>   covs(n_cov);
    std::vector<EbwDiscriminativeGaussDensityEstimator>  dens(n_dens);
    std::vector<EbwDiscriminativeMixtureEstimator*>      mixes(n_mix);
    for (int i = 0; i < n_mean; ++i) {
        if (ism) {
            EbwDiscriminativeMeanEstimatorWithISmoothing* e = new EbwDiscriminativeMeanEstimatorWithISmoothing(dim);
            e->setIMean(std::vector<MeanType>(i_means + (long)i * dim, i_means + (long)(i + 1) * dim)), e->setConstant(cfg[11]);
            means[i] = e;
        }
        else
            means[i] = new EbwDiscriminativeMeanEstimator(dim);
        for (int side = 0; side < 2; ++side) {
            const double* b = acc + side * block;
            VecAcc&       a = side ? means[i]->denAccumulator_ : means[i]->accumulator_;
            a.weight_ = b[nk + i], a.sum_.assign(b + nk + n_mean + (long)i * dim, b + nk + n_mean + (long)(i + 1) * dim);
        }
        means[i]->previousMean_.assign(prev_means + (long)i * dim, prev_means + (long)(i + 1) * dim);
    }
    for (int i = 0; i < n_cov; ++i) {
        if (ism) {
            EbwDiscriminativeCovarianceEstimatorWithISmoothing* e = new EbwDiscriminativeCovarianceEstimatorWithISmoothing(dim);
            e->setICovariance(std::vector<VarianceType>(i_vars + (long)i * dim, i_vars + (long)(i + 1) * dim)), e->setConstant(cfg[11]);
            covs[i] = e;
        }
        else
            covs[i] = new EbwDiscriminativeCovarianceEstimator(dim);
        for (int side = 0; side < 2; ++side) {
            const double* c = acc + side * block + nk + (long)n_mean * (1 + dim);
            VecAcc&       a = side ? covs[i]->denAccumulator_ : covs[i]->accumulator_;
            a.weight_ = c[i], a.sum_.assign(c + n_cov + (long)i * dim, c + n_cov + (long)(i + 1) * dim);
        }
        covs[i]->previousCovariance_.assign(prev_vars + (long)i * dim, prev_vars + (long)(i + 1) * dim);
    }
    for (int d = 0; d < n_dens; ++d)
        dens[d].meanEstimator_ = means[dens_mean[d]], dens[d].covarianceEstimator_ = covs[dens_cov[d]];
    AbstractMixtureSetEstimator::MixtureEstimators mixtureEstimators_;
    for (int m = 0; m < n_mix; ++m) {
        Mixture previous, ismoothing;   // Mixture::weight(): exp of the log weight
        EbwDiscriminativeMixtureEstimatorWithISmoothing* is = ism ? new EbwDiscriminativeMixtureEstimatorWithISmoothing : 0;
        mixes[m] = ism ? is : new EbwDiscriminativeMixtureEstimator;
        mixes[m]->nIterations_ = (u32)cfg[10];
        for (u32 k = mix_off[m]; k < mix_off[m + 1]; ++k) {
            previous.addLogDensity(dens_index[k], prev_logw[k]);
            mixes[m]->densityEstimators_.push_back(&dens[dens_index[k]]);
            mixes[m]->weights_.push_back(acc[k]);
            mixes[m]->denWeights_.push_back(acc[block + k]);
            mixes[m]->previousMixtureWeights_.push_back(previous.weight(k - mix_off[m]));
            if (ism) {
                ismoothing.addLogDensity(dens_index[k], i_logw[k]);
                is->iMixtureWeights_.push_back(ismoothing.weight(k - mix_off[m]));
            }
        }
        if (ism)
            is->setConstant(cfg[12]);
        mixtureEstimators_.push_back(mixes[m]);
    }
    // DiscriminativeMixtureSetEstimator::estimate (Mm/DiscriminativeMixtureSetEstimator.cc:136-160), step by step
    if (min_obs != 0 || min_rel != 0)
        for (int m = 0; m < n_mix; ++m)
            mixes[m]->removeDensitiesWithLowWeight(min_obs, min_rel);
    ReferenceIndexMap<AbstractMeanEstimator>       meanMap;
    ReferenceIndexMap<AbstractCovarianceEstimator> covMap;
    ReferenceIndexMap<GaussDensityEstimator>       densMap;
    for (int m = 0; m < n_mix; ++m)
        for (DensityIndex d = 0; d < mixes[m]->nDensities(); ++d) {   // MixtureSetEstimatorIndexMap (AbstractMixtureSetEstimator.cc:804-817)
            Core::Ref<GaussDensityEstimator> e = mixes[m]->densityEstimators_[d];
            meanMap.add(e->meanEstimator_), covMap.add(e->covarianceEstimator_), densMap.add(e);
        }
    CovarianceToMeanSetMap meanSetMap;   // GaussDensityEstimator.cc:241-245
    for (size_t i = 0; i < densMap.size(); ++i)
        meanSetMap.map_[densMap[(u32)i]->covarianceEstimator_].insert(densMap[(u32)i]->meanEstimator_);
    {   // EbwDiscriminativeMixtureSetEstimator::initialize (Mm/EbwDiscriminativeMixtureSetEstimator.cc:67-73)
        IterationConstants* ic = IterationConstants::createIterationConstants(config);
        if (!ic)
            return eb_failed | 16;
        ic->set(mixtureEstimators_, meanSetMap);
        delete ic;
    }
    std::vector<Mixture*> newMixtures;
    for (int m = 0; m < n_mix; ++m)
        newMixtures.push_back(mixes[m]->estimate(densMap, normalize));
    std::vector<Mean*> newMeans;
    for (size_t i = 0; i < meanMap.size(); ++i)
        newMeans.push_back(static_cast<EbwDiscriminativeMeanEstimator*>(meanMap[(u32)i].get())->estimate());
    std::vector<Covariance*> newCovs;
    for (size_t i = 0; i < covMap.size(); ++i)
        newCovs.push_back(static_cast<EbwDiscriminativeCovarianceEstimator*>(covMap[(u32)i].get())->estimate(meanSetMap, (VarianceType)min_var));
    *o_objective = 0;
    if (ism) {   // finalize (EbwDiscriminativeMixtureSetEstimator.cc:152-158) -> ISmoothingMixtureSetEstimator::getObjectiveFunction (:96-115)
        for (int m = 0; m < n_mix; ++m)      // distributePreviousMixtureSet(toEstimate)
            for (DensityIndex d = 0; d < mixes[m]->nDensities(); ++d)
                mixes[m]->previousMixtureWeights_[d] = newMixtures[m]->weight(d);
        for (size_t i = 0; i < meanMap.size(); ++i) {
            DiscriminativeMeanEstimator* e = static_cast<DiscriminativeMeanEstimator*>(static_cast<EbwDiscriminativeMeanEstimator*>(meanMap[(u32)i].get()));
            e->previousMean_.assign(newMeans[i]->begin(), newMeans[i]->end());
        }
        for (size_t i = 0; i < covMap.size(); ++i)
            static_cast<EbwDiscriminativeCovarianceEstimator*>(covMap[(u32)i].get())->previousCovariance_ = newCovs[i]->diagonal();
        Sum iOfW = 0;
        for (int m = 0; m < n_mix; ++m)
            iOfW += static_cast<EbwDiscriminativeMixtureEstimatorWithISmoothing*>(mixes[m])->getObjectiveFunction();
        Sum iOfM = 0;
        for (size_t i = 0; i < covMap.size(); ++i)
            iOfM += static_cast<EbwDiscriminativeCovarianceEstimatorWithISmoothing*>(static_cast<EbwDiscriminativeCovarianceEstimator*>(covMap[(u32)i].get()))
                            ->getObjectiveFunction(meanSetMap);
        *o_objective = iOfW + iOfM;
    }
    if (min_rel != 0)   // DiscriminativeMixtureSetEstimator::finalize (:92-98)
        for (int m = 0; m < n_mix; ++m)
            newMixtures[m]->removeDensitiesWithLowWeight(min_rel, normalize);
    // out
    auto old_of = [&](const void* p, int what) -> s32 {
        if (what == 0) { for (int d = 0; d < n_dens; ++d) if ((const void*)&dens[d] == p) return d; }
        if (what == 1) { for (int i = 0; i < n_mean; ++i) if ((const void*)static_cast<AbstractMeanEstimator*>(means[i]) == p) return i; }
        if (what == 2) { for (int i = 0; i < n_cov; ++i) if ((const void*)static_cast<AbstractCovarianceEstimator*>(covs[i]) == p) return i; }
        return -1;
    };
    o_counts[0] = (u32)densMap.size(), o_counts[1] = (u32)meanMap.size(), o_counts[2] = (u32)covMap.size();
    u32 pos = 0;
    o_mix_off[0] = 0;
    for (int m = 0; m < n_mix; ++m) {
        for (DensityIndex d = 0; d < newMixtures[m]->nDensities(); ++d, ++pos)
            o_dens_index[pos] = newMixtures[m]->densityIndex(d), o_logw[pos] = newMixtures[m]->logWeight(d);
        o_mix_off[m + 1] = pos;
    }
    o_counts[3] = pos;
    for (size_t i = 0; i < densMap.size(); ++i)
        o_dens_old[i] = (u32)old_of(densMap[(u32)i].get(), 0);
    for (size_t i = 0; i < meanMap.size(); ++i) {
        o_mean_old[i] = (u32)old_of(meanMap[(u32)i].get(), 1);
        std::copy(newMeans[i]->begin(), newMeans[i]->end(), o_means + i * dim);
        o_icd[i] = static_cast<EbwDiscriminativeMeanEstimator*>(meanMap[(u32)i].get())->iterationConstant_;
    }
    for (size_t i = 0; i < covMap.size(); ++i) {
        o_cov_old[i] = (u32)old_of(covMap[(u32)i].get(), 2);
        std::copy(newCovs[i]->diagonal().begin(), newCovs[i]->diagonal().end(), o_vars + i * dim);
    }
    std::vector<const void*> eb_cov_walk;   // the covariances in the order their densities were walked
    for (size_t i = 0; i < eb_dens_walk.size(); ++i) {
        const void* c = static_cast<const EbwDiscriminativeGaussDensityEstimator*>(eb_dens_walk[i])->covarianceEstimator_.get();
        if (std::find(eb_cov_walk.begin(), eb_cov_walk.end(), c) == eb_cov_walk.end())
            eb_cov_walk.push_back(c);
    }
    for (size_t i = 0; i < eb_cov_walk.size(); ++i)
        o_cov_walk[i] = old_of(eb_cov_walk[i], 2);
    for (size_t i = 0; i < eb_dens_walk.size(); ++i)
        o_cov_dens_walk[i] = old_of(eb_dens_walk[i], 0);
    size_t mpos = 0;
    for (size_t i = 0; i < eb_cov_walk.size(); ++i) {
        const CovarianceToMeanSetMap::MeanSet& set = meanSetMap.map_.find(Core::Ref<AbstractCovarianceEstimator>(
                                                             (AbstractCovarianceEstimator*)eb_cov_walk[i]))->second;
        o_cov_mean_count[i] = (s32)set.size();
        for (CovarianceToMeanSetMap::MeanSet::const_iterator it = set.begin(); it != set.end(); ++it)
            o_cov_mean_walk[mpos++] = old_of(it->get(), 1);
    }
    for (auto p : newMixtures) delete p;
    for (auto p : newMeans) delete p;
    for (auto p : newCovs) delete p;
    for (auto p : means) delete p;
    for (auto p : covs) delete p;
    for (auto p : mixes) delete p;
    return eb_failed;
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-D_GNU_SOURCE", "-DSPRINT_RELEASE_BUILD", "-w"]


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


def build_file(tmp, parts):
    gen, so = os.path.join(tmp, "ebw_file.cc"), os.path.join(tmp, "ebw_file.so")
    with open(gen, "w") as f:
        f.write(SOURCE_FILE % parts)
    subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", so, gen])
    L = C.CDLL(so)
    u32p, f64p = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.uint32, np.float64))
    L.eb_file.restype = C.c_long
    L.eb_file.argtypes = [C.c_int] * 5 + [u32p] * 4 + [f64p, C.c_char_p, C.c_long]
    return L


def reference_file(L, model, acc):
    m = model
    args = (int(m["dim"]), len(m["mix_offsets"]) - 1, len(m["dens_mean"]), m["means"].shape[0], m["variances"].shape[0],
            np.ascontiguousarray(m["mix_offsets"], np.uint32), np.ascontiguousarray(m["dens_index"], np.uint32),
            np.ascontiguousarray(m["dens_mean"], np.uint32), np.ascontiguousarray(m["dens_cov"], np.uint32), np.ascontiguousarray(acc, np.float64))
    buf = C.create_string_buffer(1 << 20)
    n = L.eb_file(*args, buf, len(buf))
    assert 0 < n <= len(buf)
    return buf.raw[:n]


TYPES = {"global-rwth": 0, "local-rwth": 1, "cambridge": 2}


def build_estimate(tmp, flavour, parts):
    gen, so = os.path.join(tmp, "ebw_est_%s.cc" % flavour), os.path.join(tmp, "ebw_est_%s.so" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE_EST % parts)
    subprocess.check_call(["g++"] + FLAGS + ([] if flavour == "off" else ["-march=native"]) + ["-shared", "-o", so, gen])
    L = C.CDLL(so)
    u32p, f64p, f32p, s32p = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.uint32, np.float64, np.float32, np.int32))
    L.eb_estimate.argtypes = [C.c_int] * 5 + [u32p] * 4 + [f64p, f64p, f32p, f32p, C.c_int, f64p, f32p, f32p, f64p] + \
        [u32p, u32p, u32p, f64p, u32p, u32p, u32p, f32p, f32p, f64p, f64p, s32p, s32p, s32p, s32p]
    return L


def reference_estimate(L, model, acc, prev, ism, cfg):
    """the reference's estimate on one case; also the orders in which its hash tables were walked"""
    c = dict(er.ESTIMATE_DEFAULTS)
    c.update(cfg)
    dim, nk, n_mix = int(model["dim"]), int(model["mix_offsets"][-1]), len(model["mix_offsets"]) - 1
    n_dens, n_mean, n_cov = len(model["dens_mean"]), prev["means"].shape[0], prev["variances"].shape[0]
    cf = np.array([c["min_observation_weight"], c["min_relative_weight"], c["min_variance"], float(c["normalize_mixture_weights"]), TYPES[c["type"]],
                   c["step_size"], c["minimum_icd"], c["beta"], np.nan if c["sigma_minimum"] is None else c["sigma_minimum"],
                   c["sigma_minimum_factor"], c["number_of_iterations"], c["i_smoothing_means"], c["i_smoothing_weights"]], np.float64)
    i = ism if ism is not None else prev
    counts, mo, di, lw = np.zeros(4, np.uint32), np.zeros(n_mix + 1, np.uint32), np.zeros(nk, np.uint32), np.zeros(nk)
    dold, mold, cold = np.zeros(n_dens, np.uint32), np.zeros(n_mean, np.uint32), np.zeros(n_cov, np.uint32)
    om, ov, icd, obj = np.zeros((n_mean, dim), np.float32), np.zeros((n_cov, dim), np.float32), np.zeros(n_mean), np.zeros(1)
    cw, cdw, cmw, cmc = np.full(n_cov, -1, np.int32), np.full(n_dens, -1, np.int32), np.full(n_mean, -1, np.int32), np.zeros(n_cov, np.int32)
    failed = L.eb_estimate(dim, n_mix, n_dens, n_mean, n_cov, *(np.ascontiguousarray(model[k], np.uint32) for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov")),
                           np.ascontiguousarray(acc, np.float64), np.ascontiguousarray(prev["log_weight"], np.float64), np.ascontiguousarray(prev["means"], np.float32),
                           np.ascontiguousarray(prev["variances"], np.float32), int(ism is not None), np.ascontiguousarray(i["log_weight"], np.float64),
                           np.ascontiguousarray(i["means"], np.float32), np.ascontiguousarray(i["variances"], np.float32), cf,
                           counts, mo, di, lw, dold, mold, cold, om, ov, icd, obj, cw, cdw, cmw, cmc)
    assert failed == 0, "the reference would have aborted (%d)" % failed
    nd, nm, nc, ns = (int(v) for v in counts)
    cov_walk, dens_walk = [int(v) for v in cw if v >= 0], [int(v) for v in cdw if v >= 0]
    cov_dens = {cv: [d for d in dens_walk if int(model["dens_cov"][d]) == cv] for cv in cov_walk}
    cov_means, pos = {}, 0
    for n, cv in enumerate(cov_walk):
        cov_means[cv] = [int(v) for v in cmw[pos:pos + cmc[n]]]
        pos += int(cmc[n])
    return dict(mix_offsets=mo, dens_index=di[:ns], log_weight=lw[:ns], means=om[:nm], variances=ov[:nc], icd=icd[:nm], i_objective=float(obj[0]),
                orders=dict(cov_walk=cov_walk, cov_densities=cov_dens, cov_means=cov_means))


def build(tmp, flavour, parts):
    gen, so = os.path.join(tmp, "ebw_%s.cc" % flavour), os.path.join(tmp, "ebw_%s.so" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    subprocess.check_call(["g++"] + FLAGS + ([] if flavour == "off" else ["-march=native"]) + ["-shared", "-o", so, gen])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    u32p, f64p, f32p = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.uint32, np.float64, np.float32))
    L.eb_over.argtypes = [C.c_float, C.c_double]
    L.eb_collect.argtypes = [C.c_int, u32p, u32p, f64p, u32p, u32p, f64p]
    L.eb_accumulate.argtypes = [C.c_int, C.c_int, f64p, f64p, f32p, C.c_double]
    L.eb_mixture.argtypes = [C.c_int, C.c_int, f64p, f64p, C.c_int, C.c_int, C.c_double]
    return L, int(fma or 0)


KS = (1, 5, 3, 2, 4, 5)


def case(D, pooled, seed):
    """three segments (6, 0 arcs in the middle one, 23 frames), 90 arcs over 20 binary exponents, arcs at the threshold, without items,
    and three arcs 33 exponents apart on one key, whose collection rounds"""
    rng = np.random.Generator(np.random.PCG64(seed))
    model = synth.gmm_cart(len(KS), 1, 5, D, seed=seed, pooled=pooled, ks=KS)
    lens, n_arcs = (6, 4, 23), (30, 0, 60)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    a_off, w, i_off, fr, em = [0], [], [0], [], []
    for n, a in zip(lens, n_arcs):
        for i in range(a):
            length = int(rng.integers(0, min(n, 9) + 1)) if i % 9 else 0
            start = int(rng.integers(0, n - length + 1))
            frames, emis = np.arange(start, start + length), rng.integers(0, 4, length)
            mag = float(rng.uniform(1, 2)) * 2.0 ** -int(rng.integers(0, 20))
            sign = 1.0 if rng.random() < 0.5 else -1.0
            if i % 25 == 3:
                mag = float(er.EPSILON)
            if i % 25 == 4:
                mag = float(np.nextafter(er.EPSILON, np.float32(1)))
            if n == 6 and i >= 27:
                frames, emis, sign = np.array([2]), np.array([3]), 1.0
                mag = 1024.0 * (1 + 2.0 ** -23) if i == 27 else 2.0 ** -22 * (1 + 2.0 ** -21)
            w.append(sign * mag)
            fr.extend(frames)
            em.extend(emis)
            i_off.append(len(fr))
        a_off.append(len(w))
    T = int(off[-1])
    feats = (rng.standard_normal((T, D)) * 1.5 + 0.5).astype(np.float32)
    best = np.stack([rng.integers(0, k, T) for k in KS], axis=1).astype(np.uint32)
    best[rng.random(best.shape) < 0.03] = 0xFFFFFFFF                                 # no density: the key is left out
    return dict(model=model, frame_offsets=off, arc_offsets=np.array(a_off, np.int64), arc_weight=np.array(w, np.float32),
                item_offsets=np.array(i_off, np.int64), item_frame=np.array(fr, np.int32), item_emission=np.array(em, np.int32), feats=feats,
                best=best)


def run_reference(L, c):
    """(flat buffer, key order as positions in er.collect()'s list, collected weights in that order)"""
    model, off = c["model"], c["frame_offsets"]
    o, D = er.layout(model), int(model["dim"])
    acc, base = np.zeros(o["size"], np.float64), np.zeros(o["size"], np.float64)   # base: only its slot weights are filled
    mine = er.collect(off, c["arc_offsets"], c["arc_weight"], c["item_offsets"], c["item_frame"], c["item_emission"])
    place = {(k["side"], k["frame"], k["mixture"]): i for i, k in enumerate(mine)}
    order, weights = [], []
    moff = model["mix_offsets"].astype(np.int64)
    for s in range(len(off) - 1):
        for side in (er.DEN, er.NUM):                                                 # SegmentwiseGmmTrainer.cc:164-166
            t, m, w = [], [], []
            for a in range(int(c["arc_offsets"][s]), int(c["arc_offsets"][s + 1])):
                aw = np.float32(-c["arc_weight"][a]) if side == er.DEN else np.float32(c["arc_weight"][a])   # Fsa::multiply(fsa, -1)
                if not L.eb_over(float(aw), float(er.EPSILON)):
                    continue
                for i in range(int(c["item_offsets"][a]), int(c["item_offsets"][a + 1])):
                    t.append(int(c["item_frame"][i])), m.append(int(c["item_emission"][i])), w.append(float(aw))
            n = len(t)
            kt, km, kw = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
            nk = L.eb_collect(n, np.array(t + [0], np.uint32), np.array(m + [0], np.uint32), np.array(w + [0.0], np.float64), kt, km, kw)
            for j in range(nk):
                frame, mix, wk = int(off[s] - off[0]) + int(kt[j]), int(km[j]), float(kw[j])
                order.append(place[(side, frame, mix)])
                weights.append(wk)
                d = int(c["best"][frame, mix])
                if d >= moff[mix + 1] - moff[mix]:
                    continue
                slot = int(moff[mix] + d)
                dens = int(model["dens_index"][slot])
                mean, cov = int(model["dens_mean"][dens]), int(model["dens_cov"][dens])
                p = "num" if side == er.NUM else "den"
                k0, k1 = int(moff[mix]), int(moff[mix + 1])
                for ebw, a in ((1, acc), (0, base)):          # the EBW mixture estimator, and the base class beside it
                    wts, den = a[o["num_mixture_weights"] + k0:o["num_mixture_weights"] + k1].copy(), a[o["den_density_weights"] + k0:o["den_density_weights"] + k1].copy()
                    calls = L.eb_mixture(ebw, k1 - k0, wts, den, d, 1 if side == er.DEN else 0, wk)
                    assert calls == (16 if side == er.DEN else 1), calls   # the density is reached once, on the key's side, with its weight
                    a[o["num_mixture_weights"] + k0:o["num_mixture_weights"] + k1], a[o["den_density_weights"] + k0:o["den_density_weights"] + k1] = wts, den
                x = np.ascontiguousarray(c["feats"][frame])
                for square, what, row in ((0, "mean", mean), (1, "cov", cov)):
                    s0, w0 = o["%s_%s_sums" % (p, what)] + row * D, o["%s_%s_weights" % (p, what)] + row
                    sums, weight = acc[s0:s0 + D].copy(), acc[w0:w0 + 1].copy()
                    L.eb_accumulate(square, D, sums, weight, x, wk)
                    acc[s0:s0 + D], acc[w0] = sums, weight[0]
    assert sorted(order) == list(range(len(mine)))
    return acc, np.array(order, np.int64), np.array(weights, np.float64), base[:o["num_mean_weights"]].copy()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def estimate_cases(parts, out):
    """the estimate on the cases of tests/test_ebw.py (ESTIMATE_CASES x its seeds), both builds.  Recorded: the new set, the iteration
    constants, the i-smoothing objective, the walks of the reference's hash tables.  Asserted: given those walks the restatement is the
    reference in every bit; with one covariance per density the library's order (ascending index) is too; with a shared covariance the
    two orders agree in every discrete outcome, and their largest distance over the cases and builds times 4 is bar (b)."""
    import json

    from tests import test_ebw as te
    worst, reached = 0.0, dict(clamped=0, fallback=0, removed=0, dk_above_default=0, xi_branch=0, floored=0)
    with tempfile.TemporaryDirectory() as tmp:
        libs = {fl: build_estimate(tmp, fl, parts) for fl in ("off", "fma")}
        names = []
        for n, case in enumerate(te.ESTIMATE_CASES):
            D, pooled, use_ism, cfg = case[:4]
            for seed in (20, 21):
                name = "estimate/%d/%d" % (n, seed)
                names.append(name)
                model, acc, ism = te.statistics(D, pooled, seed, tweak=(case + (None,))[4])
                i = ism if use_ism else None
                out[name + "/cfg"] = np.array(json.dumps(cfg))
                for fl, L in libs.items():
                    r = reference_estimate(L, model, acc, model, i, cfg)
                    mine = er.estimate(model, acc, model, i, cfg, fl, orders=r["orders"])
                    lib = er.estimate(model, acc, model, i, cfg, fl)
                    for k in ("mix_offsets", "dens_index", "log_weight", "means", "variances"):
                        assert np.asarray(mine["model"][k]).tobytes() == np.asarray(r[k]).tobytes(), (name, fl, k)
                        out["%s/%s/%s" % (name, fl, k)] = np.asarray(r[k])
                    assert np.array_equal(bits(mine["icd"]), bits(r["icd"])), (name, fl, "icd")
                    assert not use_ism or bits([mine["i_objective"]])[0] == bits([r["i_objective"]])[0], (name, fl, "objective")
                    out["%s/%s/icd" % (name, fl)], out["%s/%s/i_objective" % (name, fl)] = r["icd"], np.array(r["i_objective"])
                    out["%s/%s/cov_walk" % (name, fl)] = np.array(r["orders"]["cov_walk"], np.int32)
                    out["%s/%s/dens_walk" % (name, fl)] = np.array([d for cv in r["orders"]["cov_walk"] for d in r["orders"]["cov_densities"][cv]], np.int32)
                    out["%s/%s/mean_walk" % (name, fl)] = np.array([j for cv in r["orders"]["cov_walk"] for j in r["orders"]["cov_means"][cv]], np.int32)
                    for k in ("dk_dim", "dk_positive", "clamped", "fallback", "floored", "removed"):
                        assert np.array_equal(np.asarray(lib[k]), np.asarray(mine[k])), (name, fl, "the discrete outcome %s depends on the order" % k)
                    if not pooled:
                        for k in ("log_weight", "means", "variances"):
                            assert np.asarray(lib["model"][k]).tobytes() == np.asarray(r[k]).tobytes(), (name, fl, k, "per-density covariances leave no order")
                        assert np.array_equal(bits(lib["icd"]), bits(r["icd"]))
                    else:
                        for a, b in ((lib["model"]["means"], r["means"]), (lib["model"]["variances"], r["variances"]), (lib["icd"], r["icd"]),
                                     (np.exp(lib["model"]["log_weight"]), np.exp(r["log_weight"]))):
                            a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
                            worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))))
                    reached["clamped"] += len(mine["clamped"]) > 0
                    reached["fallback"] += len(mine["fallback"]) > 0
                    reached["removed"] += len(mine["removed"]) > 0
                    reached["floored"] += len(mine["floored"]) > 0
                    reached["dk_above_default"] += bool((mine["dk_min"] > 1).any())
                    reached["xi_branch"] += bool((mine["xi"] != float(dict(er.ESTIMATE_DEFAULTS, **cfg)["beta"])).any())
    out["estimate_cases"] = np.array(names)
    out["bar_b_measured"], out["bar_b"] = np.array(worst), np.array(4.0 * worst)
    out["estimate_reached"] = np.array(json.dumps(reached))
    print("estimate: %d cases, bar (b) measured %.3g -> %.3g, reached %s" % (len(names), worst, 4.0 * worst, reached))
    for k in ("clamped", "fallback", "removed", "dk_above_default", "xi_branch", "floored"):
        assert reached[k] > 0, "no case reaches: " + k


def main():
    parts, sha = reference_text()
    if "--accept" not in sys.argv:
        assert sha == TEXT_SHA256, "the reference's text changed: %s" % sha
    out, worst = {"text_sha256": np.array(sha)}, 0.0
    with tempfile.TemporaryDirectory() as tmp:
        libs = {fl: build(tmp, fl, parts) for fl in ("off", "fma")}
        LF = build_file(tmp, parts)
        assert libs["off"][1] == 0 and libs["fma"][1] > 0, "the two builds are not the two arithmetics"
        names = []
        for D, pooled, seed in ((1, False, 1), (5, False, 2), (5, True, 3), (39, True, 4)):
            name = "d%d/%s" % (D, "pooled" if pooled else "density")
            names.append(name)
            c = case(D, pooled, seed)
            for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov", "means", "variances", "log_weight"):
                out["%s/model/%s" % (name, k)] = c["model"][k]
            for k in ("frame_offsets", "arc_offsets", "arc_weight", "item_offsets", "item_frame", "item_emission", "feats", "best"):
                out["%s/%s" % (name, k)] = c[k]
            keys = er.collect(c["frame_offsets"], c["arc_offsets"], c["arc_weight"], c["item_offsets"], c["item_frame"], c["item_emission"])
            for fl, (L, _) in libs.items():
                acc, order, weights, base_w = run_reference(L, c)
                out["%s/%s/base_class_weights" % (name, fl)] = base_w
                # what the two classes do with a denominator key: the EBW class leaves weights_ to the numerator, the base class subtracts
                nk = len(base_w)
                assert np.all(acc[:nk] >= 0) and np.any(base_w < 0) and not np.array_equal(acc[:nk], base_w)
                sub = er.accumulate(c["model"], c["feats"], c["best"], keys, order, fl, defect="denominator-subtracted")
                assert np.array_equal(bits(sub[:nk]), bits(base_w)), "the planted defect is the base class's text"
                out["%s/%s/acc" % (name, fl)], out["%s/%s/order" % (name, fl)], out["%s/%s/weights" % (name, fl)] = acc, order, weights
                # the restatement in the recorded order is the reference in every bit; so are the collected weights
                mine = er.accumulate(c["model"], c["feats"], c["best"], keys, order, fl)
                assert np.array_equal(bits(mine), bits(acc)), (name, fl, np.argwhere(bits(mine) != bits(acc))[:5])
                assert np.array_equal(bits([keys[i]["weight"] for i in order]), bits(weights)), (name, fl)
                dev = er.accumulate(c["model"], c["feats"], c["best"], keys, "device", fl)
                worst = max(worst, float(np.max(np.abs(dev - acc) / np.maximum(1.0, np.abs(acc)))))
            # the estimator file of the first build's accumulators, with three segments' objectives in the last cell
            filed = out[name + "/off/acc"].copy()
            for obj in (0.1, -3.25e-3, 7.0):
                er.accumulate_objective(c["model"], filed, obj)
            raw = reference_file(LF, c["model"], filed)
            # writeHeader writes eight bytes of the five-letter magic: the two behind its terminator are whatever the string's buffer
            # holds (read() compares with strcmp and never looks at them).  They are recorded as zeros
            assert raw[:6] == b"DTACC\0"
            raw = raw[:6] + b"\0\0" + raw[8:]
            assert raw == er.file_bytes(c["model"], filed), (name, "the restatement's file bytes are not the reference's")
            out[name + "/file_acc"], out[name + "/file"] = filed, np.frombuffer(raw, np.uint8)
            if D > 1:
                assert not np.array_equal(bits(out[name + "/off/acc"]), bits(out[name + "/fma/acc"])), "the two builds agree on " + name
        out["cases"] = np.array(names)
    assert worst > 0.0
    out["bar_a_measured"], out["bar_a"] = np.array(worst), np.array(4.0 * worst)
    estimate_cases(parts, out)
    path = os.path.join(ROOT, "tests", "golden", "ref_ebw.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): text %s, bar (a) measured %.3g -> %.3g" % (path, os.path.getsize(path), sha[:12], worst, 4.0 * worst))


if __name__ == "__main__":
    main()
