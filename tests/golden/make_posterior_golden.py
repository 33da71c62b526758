#!/usr/bin/env python3
"""tests/golden/make_posterior_golden.py -- writes tests/golden/ref_posterior.npz: state posteriors as Mm::StatePosteriorFeatureScorer
computes them and combined scores as Mm::CombinedFeatureScorer does, from the reference's own text.

Run it where the reference tree is mounted; tests read only the fixture.  What it compiles, in both of the reference's arithmetics (the
flag sets of oracle/ref/Makefile: -msse3 = contract=off, -msse3 -march=native = contract=fma), taken by line range + SHA-256 into a
temporary directory that is deleted afterwards:
  * Mm/DensityToWeightMap.hh:23-40 (the map class)
  * Mm/StatePosteriorFeatureScorer.hh:35-242 (the class with its filter and context scorer)
  * Mm/StatePosteriorFeatureScorer.cc:20-29 (the context scorer's constructor), 31-69, 81-116, 129-143, 162-165 (_workDensityScores,
    workMixtureScores, pruneScores, workPosteriors, workLikelihoods, each WITHOUT its statistics-channel block: the shell closes the
    function after the piece) and 176-284 (the work* drivers, reset, the accessors, the candidate-list posteriorsAndMixtures)
  * Mm/CombinedFeatureScorer.cc:42-59 (CombinedContextScorer::score) and Mm/ScaledFeatureScorer.hh:47-76 (ScaledContextScorer)
behind a shell of this file's own that holds no reference text: Core::Configuration / Ref / ReferenceCounted / XmlChannel / Parameter*
stand-ins, Mm::Feature, an Mm::AssigningFeatureScorer whose context scorer returns element m of the score row and of the best-density row
the driver hands in (RowScorer), Mm::CachedAssigningFeatureScorer, Mm::FeatureScorer::ContextScorer and the CombinedFeatureScorer frame.

Findings (printed by every run, kept in the fixture):
  * mixture_mode_degenerate: workMixtureScores (cc:81-102) never assigns minimumScore_, which reset() left at DBL_MAX.  So in the
    reference posteriorsAndMixtures() forms p = DBL_MAX - s, sum = inf and every posterior 0 with logZ = inf, and pruneScores prunes
    nothing on the mixture paths.  The arithmetic the issue describes (minimum, threshold above it, log1p of the rest) is what
    _workDensityScores + pruneScores + workPosteriors compute, so the fixture's mixture-keyed cases run THAT path with one density per
    mixture (topology "identity": key = mixture index).  likelihoodAndMixtures() without a threshold is recorded from the mixture path.
  * fma_differs: which recorded arrays the -march=native build computes differently.  `prior + scale_ * scorer->score(mix)` (cc:43,
    cc:265) is contracted there into one fused multiply-add; with scale = 1 the product is exact and both builds agree.  The combination
    (the product is a virtual call's return value) is never contracted.

Per frame the generator recomputes log1p(sum) with the sum in increasing index order and in a pairwise order, and the relative distance
of every recorded f64 posterior to the nearest midpoint between two neighbouring f32 values.  It asserts that the three logZ agree to
1e-11 relative and that at most 1 % of the posteriors lie within 1e-11 relative of such a midpoint.

    python3 tests/golden/make_posterior_golden.py [out.npz]
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
    "dwm_hh": [("Mm/DensityToWeightMap.hh", 23, 40)],
    "sp_hh": [("Mm/StatePosteriorFeatureScorer.hh", 35, 242)],
    "sp_ctor": [("Mm/StatePosteriorFeatureScorer.cc", 20, 29)],
    "sp_density_scores": [("Mm/StatePosteriorFeatureScorer.cc", 31, 69)],
    "sp_mixture_prune": [("Mm/StatePosteriorFeatureScorer.cc", 81, 116)],
    "sp_posteriors": [("Mm/StatePosteriorFeatureScorer.cc", 129, 143)],
    "sp_likelihoods": [("Mm/StatePosteriorFeatureScorer.cc", 162, 165)],
    "sp_rest": [("Mm/StatePosteriorFeatureScorer.cc", 176, 284)],
    "scaled_hh": [("Mm/ScaledFeatureScorer.hh", 47, 76)],
    "combined_cc": [("Mm/CombinedFeatureScorer.cc", 42, 59)],
}
SHA = "051ecf561fccd4cbc22c383a04c48178dde2f1037313e8cc92540351410df1b7"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/Types.hh>
#include <Core/Hash.hh>
#include <Mm/Types.hh>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>
// ---- shell: stand-ins (no reference text) ----
static const f32* g_row  = 0;   // the score matrix row of the frame
static const u32* g_best = 0;   // its best-density row
static u32        g_n_mixtures = 0;
static std::vector<std::vector<u32>> g_topology;
namespace Core {
struct Configuration {};
class ReferenceCounted {
public:
    virtual ~ReferenceCounted() {}
};
struct ParameterFloat {};
struct ParameterBool {};
struct ParameterIntVector {};
class XmlChannel {};
template<class T> class Ref {
public:
    std::shared_ptr<T> p;
    Ref() {}
    explicit Ref(T* q) : p(q) {}
    template<class U> Ref(const Ref<U>& o) : p(o.p) {}
    T*       operator->() const { return p.get(); }
    T&       operator*() const { return *p; }
    T*       get() const { return p.get(); }
    explicit operator bool() const { return (bool)p; }
    bool     operator!() const { return !p; }
};
}  // namespace Core
namespace Mm {
class Feature {};
class AbstractMixtureSet;
class AssigningFeatureScorer {
public:
    struct ScoreAndBestDensity {
        Score  score;
        size_t bestDensity;
    };
    class AssigningContextScorer {
    public:
        virtual ~AssigningContextScorer() {}
        virtual Score            score(MixtureIndex m) const;
        virtual Score            score(MixtureIndex, DensityInMixture) const { abort(); }   // viterbi = false only
        virtual DensityInMixture bestDensity(MixtureIndex m) const;
    };
    typedef Core::Ref<const AssigningContextScorer> AssigningScorer;
    virtual ~AssigningFeatureScorer() {}
    virtual AssigningScorer getAssigningScorer(Core::Ref<const Feature>) const { return AssigningScorer(new AssigningContextScorer); }
    virtual AssigningScorer getAssigningScorer(const FeatureVector&) const { return AssigningScorer(new AssigningContextScorer); }
    virtual MixtureIndex    nMixtures() const { return g_n_mixtures; }
    virtual ComponentIndex  dimension() const { return 1; }
    virtual DensityIndex    nDensities() const { return 0; }
    virtual const std::vector<DensityIndex>& densitiesInMixture(MixtureIndex m) const { return g_topology[m]; }
};
// RowScorer: out of line, so that neither build sees through the call
__attribute__((noinline)) Score AssigningFeatureScorer::AssigningContextScorer::score(MixtureIndex m) const { return g_row[m]; }
__attribute__((noinline)) DensityInMixture AssigningFeatureScorer::AssigningContextScorer::bestDensity(MixtureIndex m) const { return g_best[m]; }
class CachedAssigningFeatureScorer : public AssigningFeatureScorer {
public:
    class CachedAssigningContextScorer : public AssigningContextScorer {
    protected:
        const CachedAssigningFeatureScorer* featureScorer_;
    public:
        CachedAssigningContextScorer(const CachedAssigningFeatureScorer* fs, size_t) : featureScorer_(fs) {}
    };
    virtual ScoreAndBestDensity calculateScoreAndDensity(const CachedAssigningContextScorer*, MixtureIndex) const = 0;
};
// ---- reference text: DensityToWeightMap ----
%(dwm_hh)s
// ---- reference text: StatePosteriorFeatureScorer (class, Filter, CachedStatePosteriorContextScorer) ----
%(sp_hh)s
}  // namespace Mm
using namespace Mm;
// ---- reference text: the context scorer's constructor ----
%(sp_ctor)s
// ---- reference text: _workDensityScores up to its statistics block; the shell closes it ----
%(sp_density_scores)s
}
// ---- reference text: workMixtureScores, pruneScores up to its statistics block ----
%(sp_mixture_prune)s
}
// ---- reference text: workPosteriors up to its statistics block ----
%(sp_posteriors)s
}
// ---- reference text: workLikelihoods up to its statistics block ----
%(sp_likelihoods)s
}
// ---- reference text: work* drivers, reset, accessors, candidate lists ----
%(sp_rest)s
// ---- shell: what the class declares and the driver does not use
StatePosteriorFeatureScorer::StatePosteriorFeatureScorer(const Core::Configuration&)
        : scale_(1), pruningThreshold_(DBL_MAX), viterbi_(true), contextPriors_(false), margin_(0) {}
AssigningFeatureScorer::ScoreAndBestDensity StatePosteriorFeatureScorer::calculateScoreAndDensity(
        const CachedAssigningFeatureScorer::CachedAssigningContextScorer*, MixtureIndex) const { return ScoreAndBestDensity(); }
AssigningFeatureScorer::AssigningScorer StatePosteriorFeatureScorer::getAssigningScorer(Core::Ref<const Feature>) const { return AssigningScorer(); }
AssigningFeatureScorer::AssigningScorer StatePosteriorFeatureScorer::getAssigningScorer(const FeatureVector&) const { return AssigningScorer(); }
// ---- shell: the frame of the combination
namespace Mm {
class FeatureScorer {
public:
    class ContextScorer {
    public:
        virtual ~ContextScorer() {}
        virtual EmissionIndex nEmissions() const = 0;
        virtual Score         score(EmissionIndex e) const = 0;
    };
    typedef Core::Ref<const ContextScorer> Scorer;
};
typedef FeatureScorer::ContextScorer ContextScorer;
typedef FeatureScorer::Scorer        Scorer;
class MatrixRowScorer : public ContextScorer {
    const f32* row_;
    u32        n_;
public:
    MatrixRowScorer(const f32* row, u32 n) : row_(row), n_(n) {}
    virtual EmissionIndex nEmissions() const { return n_; }
    virtual Score         score(EmissionIndex e) const;
};
__attribute__((noinline)) Score MatrixRowScorer::score(EmissionIndex e) const { return row_[e]; }
class ScaledFeatureScorer {};
class FeatureScorerScaling : public ScaledFeatureScorer {
public:
// ---- reference text: ScaledContextScorer ----
%(scaled_hh)s
};
class CombinedFeatureScorer {
public:
    typedef std::vector<MixtureIndex>         MixtureIndexTableRow;
    typedef std::vector<MixtureIndexTableRow> MixtureIndexTable;
    MixtureIndexTable mixtureIndexTable_;
    class CombinedContextScorer : public ContextScorer {
    public:
        const CombinedFeatureScorer* combinedFeatureScorer_;
        const MixtureIndexTable&     mixtureIndexTable_;
        std::vector<Scorer>          contextScorers_;
        CombinedContextScorer(const CombinedFeatureScorer* fs) : combinedFeatureScorer_(fs), mixtureIndexTable_(fs->mixtureIndexTable_) {}
        virtual EmissionIndex nEmissions() const { return mixtureIndexTable_.size(); }
        virtual Score         score(EmissionIndex e) const;
    };
};
}  // namespace Mm
// ---- reference text: CombinedContextScorer::score ----
%(combined_cc)s
// ---- this generator's own driver (no reference text) ----
typedef StatePosteriorFeatureScorer::CachedStatePosteriorContextScorer CS;
namespace {
struct Setup {
    Core::Configuration         c;
    StatePosteriorFeatureScorer fs;
    StatePosteriorFeatureScorer::FilterRef filter;
    std::vector<s32>            disregard;
    Setup(int n, double scale, double threshold, double margin, int nf, const int* fm, const double* fp, int nd, const int* dis,
          const int* topo_off, const u32* topo)
            : fs(c), filter(new StatePosteriorFeatureScorer::Filter) {
        g_n_mixtures = n;
        g_topology.assign(n, std::vector<u32>());
        for (int m = 0; m < n; ++m)
            g_topology[m].assign(topo + topo_off[m], topo + topo_off[m + 1]);
        fs.fs_               = Core::Ref<const AssigningFeatureScorer>(new AssigningFeatureScorer);
        fs.scale_            = scale;
        fs.pruningThreshold_ = threshold;
        fs.margin_           = margin;
        for (int i = 0; i < nf; ++i)
            (*filter)[fm[i]] = fp[i];
        disregard.assign(dis, dis + nd);
    }
    CS* scorer() {   // StatePosteriorFeatureScorer::getAssigningScorer (cc:387-394)
        CS* cs = new CS(Core::Ref<const Feature>(new Feature), &fs, g_n_mixtures);
        cs->setFilter(filter, disregard);
        cs->setScale(fs.scale_);
        return cs;
    }
};
}  // namespace
// posteriorsAndDensities(margin_mixture[t]) per frame.  Outputs are keyed by MIXTURE: column m holds what the map holds under
// key[t][m] = topology[m][best[t][m]]; stored / post are NaN where the map has no such key (filtered or pruned).
extern "C" int sp_density(int n, double scale, double threshold, double margin, int nf, const int* fm, const double* fp, int nd, const int* dis,
                          const int* topo_off, const u32* topo, int T, const float* scores, const u32* best, const int* margin_mixture,
                          double* stored, double* post, double* min_score, long* min_key, double* log_z, int* n_active) {
    Setup s(n, scale, threshold, margin, nf, fm, fp, nd, dis, topo_off, topo);
    const double nan = std::nan("");
    for (int t = 0; t < T; ++t) {
        g_row  = scores + (size_t)t * n;
        g_best = best + (size_t)t * n;
        std::unique_ptr<CS> cs(s.scorer());
        const StatePosteriorFeatureScorer::PosteriorsAndDensities& p = cs->posteriorsAndDensities(margin_mixture[t] < 0 ? invalidMixture : (u32)margin_mixture[t]);
        for (int m = 0; m < n; ++m) {
            const u32 key = g_topology[m][g_best[m]];
            const bool in = s.filter->find(m) != s.filter->end();
            stored[(size_t)t * n + m] = in && cs->scores_.count(key) ? cs->scores_.find(key)->second : nan;
            post[(size_t)t * n + m]   = in && p.count(key) ? p.find(key)->second : nan;
        }
        min_score[t] = cs->minimumScore();
        min_key[t]   = cs->minimumIndex() == Core::Type<u32>::max ? -1 : (long)cs->minimumIndex();
        log_z[t]     = cs->logZ();
        n_active[t]  = (int)p.size();
    }
    return 0;
}
// posteriorsAndMixtures() (what = 0) or likelihoodAndMixtures() (what = 1) per frame, keyed by mixture
extern "C" int sp_mixture(int what, int n, double scale, double threshold, int nf, const int* fm, const double* fp, int T, const float* scores,
                          double* out, double* min_score, double* log_z) {
    std::vector<int> off(n + 1);
    std::vector<u32> topo(n);
    for (int m = 0; m <= n; ++m)
        off[m] = m;
    for (int m = 0; m < n; ++m)
        topo[m] = m;
    Setup s(n, scale, threshold, 0, nf, fm, fp, 0, 0, off.data(), topo.data());
    const double nan = std::nan("");
    for (int t = 0; t < T; ++t) {
        g_row = scores + (size_t)t * n;
        std::unique_ptr<CS> cs(s.scorer());
        const StatePosteriorFeatureScorer::PosteriorsAndMixtures& p = what ? cs->likelihoodAndMixtures() : cs->posteriorsAndMixtures();
        for (int m = 0; m < n; ++m)
            out[(size_t)t * n + m] = p.count(m) ? p.find(m)->second : nan;
        min_score[t] = cs->minimumScore();
        log_z[t]     = what ? nan : cs->logZ();
    }
    return 0;
}
// posteriorsAndMixtures(IndicesAndWeights&) per frame: list f = entries [off[f], off[f + 1])
extern "C" int sp_lists(int n, double scale, int T, const float* scores, const long* off, const int* mixture, const double* prior, double* out) {
    std::vector<int> toff(n + 1);
    std::vector<u32> topo(n);
    for (int m = 0; m <= n; ++m)
        toff[m] = m;
    for (int m = 0; m < n; ++m)
        topo[m] = m;
    Setup s(n, scale, DBL_MAX, 0, 0, 0, 0, 0, 0, toff.data(), topo.data());
    for (int t = 0; t < T; ++t) {
        g_row = scores + (size_t)t * n;
        std::unique_ptr<CS> cs(s.scorer());
        StatePosteriorFeatureScorer::IndicesAndWeights l;
        for (long i = off[t]; i < off[t + 1]; ++i)
            l.push_back(StatePosteriorFeatureScorer::IndexAndWeight(mixture[i], prior[i]));
        cs->posteriorsAndMixtures(l);
        for (long i = off[t]; i < off[t + 1]; ++i)
            out[i] = l[i - off[t]].w;
    }
    return 0;
}
class ScaledAccess : public FeatureScorerScaling::ScaledContextScorer {
public:
    ScaledAccess(Scorer s, Score scale) : FeatureScorerScaling::ScaledContextScorer(s, scale) {}
};
// CombinedContextScorer::score(e) for every frame and emission; table is [n_emissions x n_models], scores[i] is [T x width[i]]
extern "C" int cb_combine(int n_models, int n_emissions, const int* table, const float* scale, int T, const float* const* scores, const int* width,
                          float* out) {
    CombinedFeatureScorer fs;
    fs.mixtureIndexTable_.resize(n_emissions);
    for (int e = 0; e < n_emissions; ++e)
        fs.mixtureIndexTable_[e].assign(table + (size_t)e * n_models, table + (size_t)(e + 1) * n_models);
    for (int t = 0; t < T; ++t) {
        CombinedFeatureScorer::CombinedContextScorer cs(&fs);
        for (int i = 0; i < n_models; ++i)
            cs.contextScorers_.push_back(Scorer(new ScaledAccess(Scorer(new MatrixRowScorer(scores[i] + (size_t)t * width[i], width[i])), scale[i])));
        for (int e = 0; e < n_emissions; ++e)
            out[(size_t)t * n_emissions + e] = cs.score(e);
    }
    return 0;
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-fno-access-control", "-D_GNU_SOURCE",
         "-DSPRINT_RELEASE_BUILD", "-I" + REF, "-I/usr/include/libxml2", "-w"]
DBL_MAX = np.finfo(np.float64).max
LENGTHS = (1, 2, 40)
T_ALL = sum(LENGTHS)
SCALES = (1.0, 0.37)
THRESHOLDS = (DBL_MAX, 30.0, 1e-3)
MARGINS = (0.0, 2.5)


def cases():
    """name -> dict(n, scale, prior, threshold, margin, topology, filter).  n = 3: every combination; n = 13: every third; n = 200: two."""
    out = {}
    i = 0
    for n in (3, 13):
        for scale in SCALES:
            for prior in ("zero", "random"):
                for thr in THRESHOLDS:
                    for margin in MARGINS:
                        topo = "identity" if i % 2 == 0 else "permuted"
                        filt = "holes" if (i % 5 == 3 and n > 3) else "all"
                        if n == 3 or i % 3 == 0:
                            out["n%d_%02d" % (n, i)] = dict(n=n, scale=scale, prior=prior, threshold=thr, margin=margin, topology=topo,
                                                            filter=filt)
                        i += 1
    out["n200_a"] = dict(n=200, scale=0.37, prior="zero", threshold=DBL_MAX, margin=0.0, topology="identity", filter="all")
    out["n200_b"] = dict(n=200, scale=1.0, prior="random", threshold=30.0, margin=2.5, topology="permuted", filter="all")
    return out


def inputs(name, c):
    """scores f32 [T, n] (N(50, 30), a few near 1e4), best densities, topology (CSR), filter, disregard list, margin mixtures"""
    n = c["n"]
    rng = np.random.Generator(np.random.PCG64(abs(hash_name(name))))
    s = rng.normal(50.0, 30.0, (T_ALL, n)).astype(np.float32)
    hit = rng.random((T_ALL, n)) < 0.03
    s[hit] = (1e4 + rng.normal(0.0, 50.0, (T_ALL, n))).astype(np.float32)[hit]
    if c["topology"] == "identity":
        sizes = np.ones(n, np.int64)
    else:
        sizes = rng.integers(1, 4, n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    nd = int(off[-1])
    topo = (np.arange(nd) if c["topology"] == "identity" else rng.permutation(nd)).astype(np.uint32)
    best = (rng.integers(0, 1 << 30, (T_ALL, n)) % sizes[None, :]).astype(np.uint32)
    if c["filter"] == "all":
        fm = np.arange(n, dtype=np.int32)
        dis = np.zeros(0, np.int32)
    else:
        fm = np.sort(rng.choice(n, n - max(1, n // 4), replace=False)).astype(np.int32)
        dis = np.array([int(fm[1]), int(fm[-1]), n + 5], np.int32)   # two filtered mixtures and a number that is none
    fp = np.zeros(len(fm)) if c["prior"] == "zero" else rng.random(len(fm)) * 5.0
    # the margin mixture: the frame's minimum on even frames, another filtered mixture on odd ones, none on every fifth
    kept = np.array([m for m in fm if m not in set(dis.tolist())], np.int64)
    prior_of = dict(zip(fm.tolist(), fp.tolist()))
    sv = np.stack([np.array([prior_of[m] for m in kept]) + c["scale"] * s[t, kept].astype(np.float64) for t in range(T_ALL)])
    amin = kept[np.argmin(sv, axis=1)]
    mm = np.full(T_ALL, -1, np.int32)
    if c["margin"] != 0.0:
        for t in range(T_ALL):
            if t % 5 == 4:
                continue
            mm[t] = amin[t] if t % 2 == 0 else kept[(int(np.where(kept == amin[t])[0][0]) + 1) % len(kept)]
    return dict(scores=s, best=best, topo_off=off, topo=topo, filter_mixture=fm, filter_prior=fp, disregard=dis, margin_mixture=mm)


def hash_name(name):
    return int(hashlib.sha256(name.encode()).hexdigest()[:12], 16)


def list_inputs(n):
    """candidate lists over the frames of inputs('n%d_00')-like scores: lengths 0, 1, 2, n and longer than n (repeated mixtures)"""
    rng = np.random.Generator(np.random.PCG64(7000 + n))
    s = rng.normal(50.0, 30.0, (T_ALL, n)).astype(np.float32)
    hit = rng.random((T_ALL, n)) < 0.03
    s[hit] = (1e4 + rng.normal(0.0, 50.0, (T_ALL, n))).astype(np.float32)[hit]
    lens = [(0, 1, 2, n, n + 7)[t % 5] for t in range(T_ALL)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mix = rng.integers(0, n, int(off[-1])).astype(np.int32)
    pri = rng.random(int(off[-1])) * 5.0
    return s, off, mix, pri


COMBINE = {
    # name -> (n_models, n_emissions, widths, columns (i = identity, p = permuted / gathered), scales)
    "m1_identity": (1, 13, (13,), "i", (1.0,)),
    "m1_scaled": (1, 13, (13,), "p", (0.1,)),
    "m2_mixed": (2, 40, (40, 17), "ip", (1.0, 3.7)),
    "m3_mixed": (3, 70, (70, 70, 31), "pip", (0.1, 3.7, 1.0)),
    "m3_identity": (3, 65, (65, 65, 65), "iii", (3.7, 0.1, 1.0)),
}


def combine_inputs(name):
    nm, ne, widths, cols, scales = COMBINE[name]
    rng = np.random.Generator(np.random.PCG64(hash_name(name)))
    table = np.zeros((ne, nm), np.int32)
    mats = []
    for i in range(nm):
        table[:, i] = np.arange(ne) if cols[i] == "i" else rng.integers(0, widths[i], ne)
        m = rng.normal(50.0, 30.0, (T_ALL, widths[i])).astype(np.float32)
        hit = rng.random(m.shape) < 0.03
        m[hit] = (1e4 + rng.normal(0.0, 50.0, m.shape)).astype(np.float32)[hit]
        mats.append(m)
    return table, np.array(scales, np.float32), mats


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
    gen = os.path.join(tmp, "posterior_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "posterior_%s.so" % flavour)
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    for fn in ("sp_density", "sp_mixture", "sp_lists", "cb_combine"):
        getattr(L, fn).restype = C.c_int
    return L, int(fma or 0)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(L):
    a = {}
    degenerate = True
    for name, c in cases().items():
        x = inputs(name, c)
        n = c["n"]
        stored = np.empty((T_ALL, n))
        post = np.empty((T_ALL, n))
        mn, lz = np.empty(T_ALL), np.empty(T_ALL)
        mk = np.empty(T_ALL, np.int64)
        na = np.empty(T_ALL, np.int32)
        fm, fp, dis = x["filter_mixture"], x["filter_prior"], x["disregard"]
        assert L.sp_density(n, C.c_double(c["scale"]), C.c_double(c["threshold"]), C.c_double(c["margin"]), len(fm), p(fm), p(fp), len(dis), p(dis),
                            p(x["topo_off"]), p(x["topo"]), T_ALL, p(x["scores"]), p(x["best"]), p(x["margin_mixture"]), p(stored), p(post), p(mn), p(mk),
                            p(lz), p(na)) == 0
        k = "d/" + name + "/"
        a[k + "stored"], a[k + "post"], a[k + "min"], a[k + "min_key"], a[k + "logz"], a[k + "n_active"] = stored, post, mn, mk, lz, na
        # the node's sorted sparse vector (StatePosteriorFeatureScorerNode.cc:49-57): keys in increasing order, f32 values; -1 pads
        key = x["topo"][x["topo_off"][:-1][None, :] + x["best"].astype(np.int64)].astype(np.int64)
        si = np.full((T_ALL, n), -1, np.int32)
        sv = np.zeros((T_ALL, n), np.float32)
        for t in range(T_ALL):
            act = np.nonzero(~np.isnan(post[t]))[0]
            order = act[np.argsort(key[t, act])]
            si[t, :len(order)] = key[t, order]
            sv[t, :len(order)] = post[t, order].astype(np.float32)
        a[k + "sparse_index"], a[k + "sparse_value"] = si, sv
        if c["margin"] == 0.0 and c["topology"] == "identity":
            # the mixture paths themselves: posteriors are degenerate (see the module text), likelihoods are exp(-s) without pruning
            out = np.empty((T_ALL, n))
            m2, l2 = np.empty(T_ALL), np.empty(T_ALL)
            fmk = np.array([m for m in fm if m not in set(dis.tolist())], np.int32)
            fpk = np.array([fp[list(fm).index(m)] for m in fmk], np.float64)
            assert L.sp_mixture(0, n, C.c_double(c["scale"]), C.c_double(c["threshold"]), len(fmk), p(fmk), p(fpk), T_ALL, p(x["scores"]), p(out), p(m2),
                                p(l2)) == 0
            degenerate = degenerate and bool(np.all(m2 == DBL_MAX)) and bool(np.all(np.nan_to_num(out) == 0.0)) and bool(np.all(np.isinf(l2)))
            if c["threshold"] == DBL_MAX and n < 200:
                assert L.sp_mixture(1, n, C.c_double(c["scale"]), C.c_double(c["threshold"]), len(fmk), p(fmk), p(fpk), T_ALL, p(x["scores"]), p(out),
                                    p(m2), p(l2)) == 0
                a["l/" + name + "/likelihood"] = out.copy()
    a["mixture_mode_degenerate"] = np.array(degenerate)
    for n in (3, 13, 200):
        for scale in SCALES:
            s, off, mix, pri = list_inputs(n)
            out = np.empty(int(off[-1]))
            assert L.sp_lists(n, C.c_double(scale), T_ALL, p(s), p(off), p(mix), p(pri), p(out)) == 0
            a["c/%d/%g/post" % (n, scale)] = out
    for name in COMBINE:
        table, scales, mats = combine_inputs(name)
        nm, ne, widths, _, _ = COMBINE[name]
        ptrs = (C.c_void_p * nm)(*[m.ctypes.data for m in mats])
        w = np.array(widths, np.int32)
        out = np.empty((T_ALL, ne), np.float32)
        assert L.cb_combine(nm, ne, p(np.ascontiguousarray(table)), p(scales), T_ALL, ptrs, p(w), p(out)) == 0
        a["b/" + name + "/out"] = out
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def midpoint_distance(x):
    """relative distance of each f64 value to the nearest midpoint between two neighbouring f32 values (inf for 0, NaN and values
    outside the f32 range)"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        f = x.astype(np.float32)
        lo = np.where(f.astype(np.float64) <= x, f, np.nextafter(f, np.float32(-np.inf)))
        hi = np.nextafter(lo, np.float32(np.inf))
        mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
        d = np.abs(x - mid) / np.abs(x)
    d[~np.isfinite(d) | (x == 0) | np.isnan(x)] = np.inf
    return d


def pairwise(v):
    v = list(v)
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else 0.0


def check_orders(arrays, prefix):
    """log1p(sum) in increasing index order and pairwise against the recorded logZ; midpoint statistics.  Returns (worst, share)."""
    def get(k):
        return arrays[prefix + k] if prefix + k in arrays else arrays["off/" + k]
    worst, near, total = 0.0, 0, 0
    for name, c in cases().items():
        k = "d/" + name + "/"
        stored, post, mn, lz, mk = get(k + "stored"), get(k + "post"), get(k + "min"), get(k + "logz"), get(k + "min_key")
        x = inputs(name, c)
        key = x["topo"][x["topo_off"][:-1][None, :] + x["best"].astype(np.int64)].astype(np.int64)
        dist = midpoint_distance(post)
        if prefix + k + "post" in arrays:
            arrays[prefix + k + "midpoint"] = np.minimum(dist, 1.0).astype(np.float32)   # 1: far (also 0, NaN, outside f32)
        act = ~np.isnan(post)
        near += int(np.sum(dist[act] <= 1e-11))
        total += int(np.sum(act))
        for t in range(stored.shape[0]):
            idx = [m for m in np.nonzero(act[t])[0] if key[t, m] != mk[t]]
            with np.errstate(all="ignore"):
                terms = [np.exp(mn[t] - stored[t, m]) for m in idx]
            inc = 0.0
            for v in terms:
                inc += v
            for total_sum in (inc, pairwise(terms)):
                z = np.log1p(total_sum) - mn[t]
                worst = max(worst, abs(z - lz[t]) / max(abs(lz[t]), np.finfo(np.float64).tiny))
    return worst, near / max(total, 1)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_posterior.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_posterior_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    arrays = {}
    for name, c in cases().items():
        for k, v in inputs(name, c).items():
            arrays["in/d/%s/%s" % (name, k)] = v
        arrays["cfg/" + name] = np.array([c["n"], c["scale"], c["threshold"], c["margin"]], np.float64)
    for n in (3, 13, 200):
        s, off, mix, pri = list_inputs(n)
        arrays["in/c/%d/scores" % n], arrays["in/c/%d/offsets" % n], arrays["in/c/%d/mixture" % n], arrays["in/c/%d/prior" % n] = s, off, mix, pri
    for name in COMBINE:
        table, scales, mats = combine_inputs(name)
        arrays["in/b/%s/table" % name], arrays["in/b/%s/scales" % name] = table, scales
        for i, m in enumerate(mats):
            arrays["in/b/%s/scores%d" % (name, i)] = m
    with tempfile.TemporaryDirectory() as tmp:
        got = {}
        for fl in ("off", "fma"):
            L, n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)
            got[fl] = run(L)
    for k, v in got["off"].items():
        arrays["off/" + k] = v
    differ = [k for k, v in got["fma"].items() if not same_bits(v, got["off"][k])]
    for k in differ:
        arrays["fma/" + k] = got["fma"][k]
    arrays["fma_differs"] = np.array(differ if differ else [""])
    arrays["fma_arrays_compared"] = np.array(len(got["fma"]))
    worst, share = 0.0, 0.0
    for prefix in ("off/", "fma/"):
        w, s = check_orders(arrays, prefix)
        worst, share = max(worst, w), max(share, s)
    arrays["order_worst_logz_distance"] = np.array(worst)
    arrays["midpoint_share"] = np.array(share)
    assert worst <= 1e-11, "logZ moves by %g relative with the order of the sum: choose other seeds" % worst
    assert share <= 0.01, "%g of the posteriors lie within 1e-11 of an f32 midpoint: choose other seeds" % share
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    print("  fma instructions: off %d, fma %d" % (int(arrays["fma_instructions/off"]), int(arrays["fma_instructions/fma"])))
    print("  fma copies that differ from off: %d of %d %s" % (len(differ), len(got["fma"]), differ[:6]))
    print("  mixture mode degenerate in the reference: %s / %s" % (bool(got["off"]["mixture_mode_degenerate"]), bool(got["fma"]["mixture_mode_degenerate"])))
    print("  worst logZ distance between summation orders %.3g, share of posteriors within 1e-11 of an f32 midpoint %.3g" % (worst, share))


if __name__ == "__main__":
    main()
