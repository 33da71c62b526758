// ebw_host.cpp -- the host side of EBW training (include/amx.h, section "EBW"): the binary estimator file of
// Mm::EbwDiscriminativeMixtureSetEstimator and the file-level sum, on the flat accumulator that ebw.hip fills.  Nothing here needs a
// device.
//
// The file has the layout of the "MIXSET" estimator file, version 2 (Mm/AbstractMixtureSetEstimator.cc:404-508), under the discriminative
// estimators' own magic "DTACC" (Mm/DiscriminativeMixtureSetEstimator.hh:42-44), with what the discriminative classes append to every record:
//   char[8] "DTACC\0\0\0" | u32 version | u32 dimension      writeHeader (:416-420) writes eight bytes of a five-letter string: the two
//                                                            behind its terminator are whatever the string's buffer held; zeros here.
//                                                            read() compares with strcmp (:405-411), so it never looks at them
//   u32 nMeans       { numerator  u32 dim, f64 sum[dim], f64 weight | denominator the same }   Mm/VectorAccumulator.hh:80-100,
//   u32 nCovariances { numerator  u32 dim, f64 sum[dim], f64 weight | denominator the same }   EbwDiscriminativeGaussDensityEstimator.cc:55-58, :150-153
//   u32 nDensities   { u32 meanIndex, u32 covarianceIndex }                                     Mm/GaussDensityEstimator.cc:46-62
//   u32 nMixtures    { u32 n, { u32 densityIndex, f64 weight } x n, f64 denWeight x n }         Mm/MixtureEstimator.cc:163-170,
//                                                                                              EbwDiscriminativeMixtureEstimator.cc:148-154
//   f64 objective                                                                              DiscriminativeMixtureSetEstimator.cc:115-119
// little endian like every Core::BinaryStream file.  weight of a mixture entry is weights_, which the EBW mixture
// estimator adds to for numerator keys only (its accumulateDenominator does not call the base class's `weights_ -= weight`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <algorithm>
#include <cfloat>
#include <map>
#include <memory>

#include "common.hpp"
#include "mixture_set.hpp"

extern "C++" {
namespace {

struct EbwLayout {
    long long nk, n_mean, n_cov, dim;
    long long mw[2], ms[2], cw[2], cs[2], den_dw, objective, size;   // [0] numerator, [1] denominator
};

int ebw_layout(const amx_gmm_model* t, const char* who, EbwLayout* l) {
    AMX_REQUIRE(t, AMX_ERR_INVALID, "%s: NULL topology", who);
    AMX_REQUIRE(t->dim >= 1 && t->n_mix >= 1 && t->n_dens >= 1 && t->n_mean >= 1 && t->n_cov >= 1, AMX_ERR_INVALID,
                "%s: bad topology (dim %d, %d mixtures, %d densities, %d means, %d covariances)", who, t->dim, t->n_mix, t->n_dens, t->n_mean, t->n_cov);
    AMX_REQUIRE(t->mix_offsets && t->dens_index && t->dens_mean && t->dens_cov, AMX_ERR_INVALID, "%s: NULL topology array", who);
    AMX_REQUIRE(t->mix_offsets[0] == 0, AMX_ERR_INVALID, "%s: mix_offsets[0] is not 0", who);
    for (int m = 0; m < t->n_mix; ++m)
        AMX_REQUIRE(t->mix_offsets[m + 1] >= t->mix_offsets[m], AMX_ERR_INVALID, "%s: mix_offsets decrease at mixture %d", who, m);
    l->nk = t->mix_offsets[t->n_mix], l->n_mean = t->n_mean, l->n_cov = t->n_cov, l->dim = t->dim;
    for (long long k = 0; k < l->nk; ++k)
        AMX_REQUIRE(t->dens_index[k] < (uint32_t)t->n_dens, AMX_ERR_INVALID, "%s: entry %lld: density %u is outside [0, %d)", who, k, t->dens_index[k],
                    t->n_dens);
    for (int d = 0; d < t->n_dens; ++d)
        AMX_REQUIRE(t->dens_mean[d] < (uint32_t)t->n_mean && t->dens_cov[d] < (uint32_t)t->n_cov, AMX_ERR_INVALID,
                    "%s: density %d: mean %u or covariance %u is outside the model", who, d, t->dens_mean[d], t->dens_cov[d]);
    long long pos = 0;
    for (int side = 0; side < 2; ++side) {
        if (side)
            l->den_dw = pos;
        pos += l->nk;   // side 0: the mixture weights (weights_)
        l->mw[side] = pos, pos += l->n_mean;
        l->ms[side] = pos, pos += l->n_mean * l->dim;
        l->cw[side] = pos, pos += l->n_cov;
        l->cs[side] = pos, pos += l->n_cov * l->dim;
    }
    l->objective = pos, l->size = pos + 1;
    return AMX_OK;
}

template<class T>
bool put(FILE* f, T v) {
    return fwrite(&v, sizeof(T), 1, f) == 1;   // little-endian host
}
template<class T>
bool get(FILE* f, T* v) {
    return fread(v, sizeof(T), 1, f) == 1;
}

}  // namespace
}  // extern "C++"

extern "C" {

long amx_ebw_topology_accumulator_size(const amx_gmm_model* topology) {
    EbwLayout l;
    return ebw_layout(topology, "amx_ebw_topology_accumulator_size", &l) == AMX_OK ? (long)l.size : 0;
}

int amx_ebw_accumulator_write(const amx_gmm_model* t, const double* acc, const char* path) {
    const char* who = "amx_ebw_accumulator_write";
    EbwLayout   l;
    AMX_TRY(ebw_layout(t, who, &l));
    AMX_REQUIRE(acc && path, AMX_ERR_INVALID, "%s: NULL argument", who);
    FILE* f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    const char   magic[8] = {'D', 'T', 'A', 'C', 'C', 0, 0, 0};
    const size_t D        = (size_t)l.dim;
    bool         ok       = fwrite(magic, 1, 8, f) == 8 && put(f, (uint32_t)2) && put(f, (uint32_t)l.dim);
    auto         vec      = [&](const double* sums, double weight) { return put(f, (uint32_t)l.dim) && fwrite(sums, 8, D, f) == D && put(f, weight); };
    ok                    = ok && put(f, (uint32_t)l.n_mean);
    for (long long i = 0; ok && i < l.n_mean; ++i)
        ok = vec(acc + l.ms[0] + i * l.dim, acc[l.mw[0] + i]) && vec(acc + l.ms[1] + i * l.dim, acc[l.mw[1] + i]);
    ok = ok && put(f, (uint32_t)l.n_cov);
    for (long long i = 0; ok && i < l.n_cov; ++i)
        ok = vec(acc + l.cs[0] + i * l.dim, acc[l.cw[0] + i]) && vec(acc + l.cs[1] + i * l.dim, acc[l.cw[1] + i]);
    ok = ok && put(f, (uint32_t)t->n_dens);
    for (int d = 0; ok && d < t->n_dens; ++d)
        ok = put(f, t->dens_mean[d]) && put(f, t->dens_cov[d]);
    ok = ok && put(f, (uint32_t)t->n_mix);
    for (int m = 0; ok && m < t->n_mix; ++m) {
        ok = put(f, (uint32_t)(t->mix_offsets[m + 1] - t->mix_offsets[m]));
        for (uint32_t k = t->mix_offsets[m]; ok && k < t->mix_offsets[m + 1]; ++k)
            ok = put(f, t->dens_index[k]) && put(f, acc[k]);
        for (uint32_t k = t->mix_offsets[m]; ok && k < t->mix_offsets[m + 1]; ++k)
            ok = put(f, acc[l.den_dw + k]);
    }
    ok = ok && put(f, acc[l.objective]);
    ok = (fclose(f) == 0) && ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: write to '%s' failed", who, path);
    return AMX_OK;
}

int amx_ebw_accumulator_read(const amx_gmm_model* t, const char* path, double* acc) {
    const char* who = "amx_ebw_accumulator_read";
    EbwLayout   l;
    AMX_TRY(ebw_layout(t, who, &l));
    AMX_REQUIRE(acc && path, AMX_ERR_INVALID, "%s: NULL argument", who);
    FILE* f = fopen(path, "rb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    std::vector<double> a((size_t)l.size, 0.0);   // the caller's buffer is written only by a file that was read to its end
    char                magic[8] = {0};
    uint32_t            version = 0, dim = 0, n = 0;
    const char*         why = nullptr;
    const size_t        D   = (size_t)l.dim;
    bool                ok  = fread(magic, 1, 8, f) == 8 && get(f, &version) && get(f, &dim);
    if (ok && memcmp(magic, "DTACC", 6) != 0)   // strcmp(_magic, magic().c_str()): the letters and the terminator
        why = "not a DTACC estimator file (the magic of Mm::DiscriminativeMixtureSetEstimator)";
    else if (ok && version < 2)
        why = "version below 2: the file holds no objective function (DiscriminativeMixtureSetEstimator.cc:105-113)";
    else if (ok && version > 2)
        why = "unknown version";
    else if (ok && (long long)dim != l.dim)
        why = "dimension differs from the model";
    auto vec = [&](double* sums, double* weight) {
        uint32_t size = 0;
        return get(f, &size) && (long long)size == l.dim && fread(sums, 8, D, f) == D && get(f, weight);
    };
    ok = ok && !why && get(f, &n) && (long long)n == l.n_mean;
    for (long long i = 0; ok && i < l.n_mean; ++i)
        ok = vec(&a[l.ms[0] + i * l.dim], &a[l.mw[0] + i]) && vec(&a[l.ms[1] + i * l.dim], &a[l.mw[1] + i]);
    ok = ok && get(f, &n) && (long long)n == l.n_cov;
    for (long long i = 0; ok && i < l.n_cov; ++i)
        ok = vec(&a[l.cs[0] + i * l.dim], &a[l.cw[0] + i]) && vec(&a[l.cs[1] + i * l.dim], &a[l.cw[1] + i]);
    ok = ok && get(f, &n) && (int)n == t->n_dens;
    for (int d = 0; ok && d < t->n_dens; ++d) {
        uint32_t mi = 0, ci = 0;
        ok          = get(f, &mi) && get(f, &ci) && mi == t->dens_mean[d] && ci == t->dens_cov[d];
    }
    ok = ok && get(f, &n) && (int)n == t->n_mix;
    for (int m = 0; ok && m < t->n_mix; ++m) {
        ok = get(f, &n) && n == t->mix_offsets[m + 1] - t->mix_offsets[m];
        for (uint32_t k = t->mix_offsets[m]; ok && k < t->mix_offsets[m + 1]; ++k) {
            uint32_t d = 0;
            ok         = get(f, &d) && d == t->dens_index[k] && get(f, &a[k]);
        }
        for (uint32_t k = t->mix_offsets[m]; ok && k < t->mix_offsets[m + 1]; ++k)
            ok = get(f, &a[l.den_dw + k]);
    }
    ok = ok && get(f, &a[l.objective]);
    char rest = 0;
    if (ok && !why && fread(&rest, 1, 1, f) == 1)
        why = "bytes behind the objective function";
    fclose(f);
    if (why) {
        amx::set_error("%s: '%s': %s", who, path, why);
        return AMX_ERR_INVALID;
    }
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: '%s' is truncated or its topology differs from the model", who, path);
    memcpy(acc, a.data(), a.size() * sizeof(double));
    return AMX_OK;
}

// combine-mixture-set-estimators: every sum, weight and the objective of `add` added to `acc` (AbstractMixtureSetEstimator::accumulate(is, os),
// Mm/AbstractMixtureSetEstimator.cc:170-300, DiscriminativeMixtureSetEstimator.cc:162-177).  The files carry no order beyond their own:
// a + b per cell
int amx_ebw_accumulator_combine(const amx_gmm_model* t, double* acc, const double* add) {
    const char* who = "amx_ebw_accumulator_combine";
    EbwLayout   l;
    AMX_TRY(ebw_layout(t, who, &l));
    AMX_REQUIRE(acc && add, AMX_ERR_INVALID, "%s: NULL argument", who);
    for (long long i = 0; i < l.size; ++i)
        AMX_REQUIRE(std::isfinite(acc[i]) && std::isfinite(add[i]), AMX_ERR_INVALID, "%s: entry %lld of an accumulator is not finite", who, i);
    for (long long i = 0; i < l.size; ++i)
        acc[i] += add[i];
    return AMX_OK;
}


void amx_ebw_estimate_cfg_default(amx_ebw_estimate_cfg* c) {
    if (!c)
        return;
    c->min_observation_weight = 5, c->min_relative_weight = 0, c->min_variance = 0, c->normalize_mixture_weights = 1;   // AbstractMixtureSetEstimator.cc:24-59
    c->iteration_constants = AMX_EBW_IC_GLOBAL_RWTH, c->step_size = 1.1, c->minimum_icd = 1;                            // IterationConstants.cc:648-672
    c->beta = 1, c->sigma_minimum = -1, c->sigma_minimum_factor = 1e-5;                                                 // :166-171, :239-253
    c->number_of_iterations = 100;                                                                                      // EbwDiscriminativeMixtureEstimator.cc:24-27
    c->i_smoothing_means = 0, c->i_smoothing_weights = 0;                                                               // ISmoothingMixtureSetEstimator.cc:27-35
    c->viterbi = 1, c->estimator = AMX_EBW_ESTIMATOR_EBW, c->contract = AMX_CONTRACT_OFF;
}

int amx_ebw_estimate(const amx_gmm_model* t, const double* acc, const amx_gmm_model* previous, const amx_gmm_model* ismoothing,
                     const amx_ebw_estimate_cfg* cfg_in, amx_mixture_set** out, amx_ebw_estimate_info* info, double* iteration_constants) {
    const char* who = "amx_ebw_estimate";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    EbwLayout l;
    AMX_TRY(ebw_layout(t, who, &l));
    AMX_REQUIRE(acc && previous, AMX_ERR_INVALID, "%s: NULL accumulator or previous mixture set", who);
    amx_ebw_estimate_cfg c;
    amx_ebw_estimate_cfg_default(&c);
    if (cfg_in)
        c = *cfg_in;
    AMX_REQUIRE(c.viterbi != 0, AMX_ERR_UNSUPPORTED, "%s: viterbi = false (getDensityPosteriorProbabilities) is not supported", who);
    AMX_REQUIRE(c.estimator != AMX_EBW_ESTIMATOR_RPROP, AMX_ERR_UNSUPPORTED, "%s: the Rprop estimators are not supported: only EBW is", who);
    AMX_REQUIRE(c.estimator == AMX_EBW_ESTIMATOR_EBW, AMX_ERR_INVALID, "%s: unknown estimator %d", who, c.estimator);
    AMX_REQUIRE(c.iteration_constants != AMX_EBW_IC_CAMBRIDGE, AMX_ERR_UNSUPPORTED,
                "%s: iteration constants of type cambridge are not supported: the reference's maximumRoot starts with require(false)", who);
    AMX_REQUIRE(c.iteration_constants == AMX_EBW_IC_GLOBAL_RWTH || c.iteration_constants == AMX_EBW_IC_LOCAL_RWTH, AMX_ERR_INVALID,
                "%s: unknown type of iteration constants %d", who, c.iteration_constants);
    AMX_REQUIRE(c.contract == AMX_CONTRACT_OFF || c.contract == AMX_CONTRACT_FMA, AMX_ERR_INVALID, "%s: unknown contract %d", who, c.contract);
    AMX_REQUIRE(c.number_of_iterations >= 0, AMX_ERR_INVALID, "%s: number_of_iterations %d is negative", who, c.number_of_iterations);
    for (long long i = 0; i < l.size; ++i)
        AMX_REQUIRE(std::isfinite(acc[i]), AMX_ERR_INVALID, "%s: entry %lld of the accumulator is not finite", who, i);
    const int    dim = t->dim, n_mix = t->n_mix;
    const size_t D   = (size_t)dim;
    const bool   ism = ismoothing != nullptr, fused = c.contract == AMX_CONTRACT_FMA;
    for (const amx_gmm_model* s : {previous, ismoothing}) {
        if (!s)
            continue;
        const char* name = s == previous ? "previous" : "i-smoothing";
        bool        same = s->dim == t->dim && s->n_mix == t->n_mix && s->n_dens == t->n_dens && s->n_mean == t->n_mean && s->n_cov == t->n_cov &&
                    s->mix_offsets && s->dens_index && s->dens_mean && s->dens_cov && s->log_weight && s->means && s->variances;
        same = same && memcmp(s->mix_offsets, t->mix_offsets, ((size_t)n_mix + 1) * 4) == 0 && memcmp(s->dens_index, t->dens_index, (size_t)l.nk * 4) == 0 &&
               memcmp(s->dens_mean, t->dens_mean, (size_t)t->n_dens * 4) == 0 && memcmp(s->dens_cov, t->dens_cov, (size_t)t->n_dens * 4) == 0;
        AMX_REQUIRE(same, AMX_ERR_INVALID, "%s: %s mixture set differs in topology", who, name);
    }
    // tying the reference cannot handle, or handles by the order of a hash walk
    {
        std::vector<int> owner((size_t)t->n_dens, -1), mean_owner((size_t)t->n_mean, -1);
        for (int m = 0; m < n_mix; ++m)
            for (uint32_t k = t->mix_offsets[m]; k < t->mix_offsets[m + 1]; ++k) {
                const uint32_t d = t->dens_index[k];
                AMX_REQUIRE(owner[d] < 0, AMX_ERR_UNSUPPORTED, "%s: density %u is shared by mixtures %d and %d (the reference requires that no density is)", who,
                            d, owner[d], m);
                owner[d] = m;
            }
        for (int d = 0; d < t->n_dens; ++d)
            if (owner[(size_t)d] >= 0) {
                const uint32_t j = t->dens_mean[d];
                AMX_REQUIRE(mean_owner[j] < 0, AMX_ERR_UNSUPPORTED,
                            "%s: mean %u is shared by densities %d and %d: its iteration constant would be the one the reference's hash walk sets last", who, j,
                            mean_owner[j], d);
                mean_owner[j] = d;
            }
        if (c.iteration_constants == AMX_EBW_IC_LOCAL_RWTH)
            for (int m = 0; m < n_mix; ++m)
                for (uint32_t k = t->mix_offsets[m]; k < t->mix_offsets[m + 1]; ++k)
                    AMX_REQUIRE(t->dens_cov[t->dens_index[k]] == t->dens_cov[t->dens_index[t->mix_offsets[m]]], AMX_ERR_UNSUPPORTED,
                                "%s: local-rwth: the densities of mixture %d use more than one covariance, and the reference's result would depend on which "
                                "one its hash walk meets first",
                                who, m);
    }
    auto mad = [fused](double a, double b, double s) { return fused ? __builtin_fma(a, b, s) : a * b + s; };
    auto cmax = [](double a, double b) { return a < b ? b : a; };   // std::max
    const double cm = ism ? c.i_smoothing_means : 0.0, cw = ism ? c.i_smoothing_weights : 0.0;
    const double *W = acc, *DW = acc + l.den_dw;
    const double *nw = acc + l.mw[0], *dw = acc + l.mw[1], *ns = acc + l.ms[0], *ds = acc + l.ms[1], *cs = acc + l.cs[0], *cds = acc + l.cs[1];
    std::vector<double> prev_w((size_t)l.nk), i_w((size_t)l.nk, 0.0);
    for (long long k = 0; k < l.nk; ++k) {   // Mixture::weight(): exp of the log weight
        prev_w[(size_t)k] = std::exp(previous->log_weight[k]);
        if (ism)
            i_w[(size_t)k] = std::exp(ismoothing->log_weight[k]);
    }
    const float *pm = previous->means, *pv = previous->variances, *im = ism ? ismoothing->means : nullptr, *iv = ism ? ismoothing->variances : nullptr;

    // removeDensitiesWithLowWeight (DiscriminativeMixtureEstimator.cc:34-49)
    std::vector<std::vector<uint32_t>> mixtures((size_t)n_mix);
    int                                n_removed = 0;
    for (int m = 0; m < n_mix; ++m) {
        std::vector<uint32_t>& slots = mixtures[(size_t)m];
        for (uint32_t k = t->mix_offsets[m]; k < t->mix_offsets[m + 1]; ++k)
            slots.push_back(k);
        if (!slots.empty() && (c.min_observation_weight != 0 || c.min_relative_weight != 0)) {
            uint32_t dmax = 0;
            for (uint32_t i = 1; i < slots.size(); ++i)
                if (W[slots[i]] > W[slots[dmax]])
                    dmax = i;
            for (uint32_t i = 0; i < slots.size();) {
                const bool enough = W[slots[i]] >= c.min_observation_weight, enough_rel = prev_w[slots[i]] >= c.min_relative_weight;
                if ((!enough || !enough_rel) && i != dmax) {
                    slots.erase(slots.begin() + i);
                    --dmax;   // as the reference has it: after every removal, in u32
                    ++n_removed;
                }
                else
                    ++i;
            }
        }
    }
    // MixtureSetEstimatorIndexMap: first appearance (AbstractMixtureSetEstimator.cc:804-817)
    std::vector<uint32_t> dens_old, mean_old, cov_old;
    std::vector<int>      new_dens((size_t)t->n_dens, -1), new_mean((size_t)t->n_mean, -1), new_cov((size_t)t->n_cov, -1);
    std::vector<int>      dens_mix((size_t)t->n_dens, -1);
    std::vector<uint32_t> dens_slot((size_t)t->n_dens, 0);
    for (int m = 0; m < n_mix; ++m)
        for (uint32_t k : mixtures[(size_t)m]) {
            const uint32_t d = t->dens_index[k], j = t->dens_mean[d], cv = t->dens_cov[d];
            if (new_mean[j] < 0)
                new_mean[j] = (int)mean_old.size(), mean_old.push_back(j);
            if (new_cov[cv] < 0)
                new_cov[cv] = (int)cov_old.size(), cov_old.push_back(cv);
            if (new_dens[d] < 0)
                new_dens[d] = (int)dens_old.size(), dens_old.push_back(d);
            dens_mix[d] = m, dens_slot[d] = k;
        }
    // per covariance its densities and means in ascending new index (the reference: the order of a hash table)
    std::vector<std::vector<uint32_t>> cov_dens(cov_old.size()), cov_means(cov_old.size());
    for (uint32_t d : dens_old) {
        cov_dens[(size_t)new_cov[t->dens_cov[d]]].push_back(d);
        cov_means[(size_t)new_cov[t->dens_cov[d]]].push_back(t->dens_mean[d]);
    }
    for (auto& v : cov_means)
        std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return new_mean[a] < new_mean[b]; });

    auto dt_weight = [&](uint32_t j) {
        const double w = nw[j] - dw[j];
        return ism ? w + cm : w;
    };
    auto dt_sum = [&](uint32_t j, size_t i) {
        const double s = ns[j * D + i] - ds[j * D + i];
        return ism ? mad(cm, (double)im[j * D + i], s) : s;
    };
    std::vector<std::vector<double>> i_sum(cov_old.size());
    if (ism)
        for (size_t n = 0; n < cov_old.size(); ++n) {   // ISmoothingCovarianceEstimator::iSum (ISmoothingGaussDensityEstimator.cc:56-71)
            i_sum[n].resize(D);
            for (size_t i = 0; i < D; ++i) {
                double s = (double)iv[cov_old[n] * D + i] * (double)cov_means[n].size();
                for (uint32_t j : cov_means[n]) {
                    const double y = (double)im[j * D + i];
                    s              = mad(y, y, s);
                }
                i_sum[n][i] = s;
            }
        }
    auto cov_dt_sum = [&](size_t n, size_t i) {
        const double s = cs[cov_old[n] * D + i] - cds[cov_old[n] * D + i];
        return ism ? mad(cm, i_sum[n][i], s) : s;
    };
    // Xi (IterationConstants.cc:166-203)
    std::vector<double> xi((size_t)n_mix);
    for (int m = 0; m < n_mix; ++m) {
        double max_abs = 0, max_num_den = 0;
        for (uint32_t k : mixtures[(size_t)m]) {
            const uint32_t j = t->dens_mean[t->dens_index[k]];
            const double   a = std::fabs(dt_weight(j));
            if (max_abs < a)
                max_abs = a, max_num_den = cmax(dt_weight(j) + dw[j], dw[j]);
        }
        const double den = (max_abs < max_num_den && max_num_den > 0) ? 1 + (max_abs - 1) * max_abs / max_num_den : 1;
        xi[(size_t)m]    = c.beta / den;
    }
    // sigma-minimum (:255-280)
    float smallest = FLT_MAX;
    for (uint32_t cv : cov_old)
        for (size_t i = 0; i < D; ++i)
            smallest = std::min(smallest, pv[cv * D + i]);
    const double sigma = c.sigma_minimum >= 0 ? c.sigma_minimum : c.sigma_minimum_factor * (double)smallest;
    // minimumDk (:285-326).  The native build shares dtWeight * previousMean between t2 and t3 and hoists sigmaMinimum * dtWeight out of
    // the loop over the components: those three are never fused
    std::vector<double> dk_min(cov_old.size()), num(D), den(D);
    for (size_t n = 0; n < cov_old.size(); ++n) {
        for (size_t i = 0; i < D; ++i)
            num[i] = 0.0 - cov_dt_sum(n, i), den[i] = 0.0;
        for (uint32_t d : cov_dens[n]) {
            const uint32_t j   = t->dens_mean[d];
            const double   dtw = dt_weight(j), x = xi[(size_t)dens_mix[d]], pw = prev_w[dens_slot[d]];
            for (size_t i = 0; i < D; ++i) {
                const double p = (double)pm[j * D + i], dts = dt_sum(j, i), prod = dtw * p;
                const double t2 = 2 * dts - prod, t3 = dts - prod;
                num[i] = num[i] + sigma * dtw;
                num[i] = mad(t2, p, num[i]);
                num[i] = mad(x * t3, t3, num[i]);
                den[i] = mad((double)pv[cov_old[n] * D + i] - sigma, pw, den[i]);
            }
        }
        double ratio_max = num[0] / den[0];
        for (size_t i = 1; i < D; ++i)
            if (ratio_max < num[i] / den[i])
                ratio_max = num[i] / den[i];
        dk_min[n] = ratio_max > 0 ? ratio_max : 0;
    }
    auto d_k = [&](uint32_t d) {
        double v = 1 / xi[(size_t)dens_mix[d]];
        v -= dt_weight(t->dens_mean[d]);
        if (prev_w[dens_slot[d]] > 0)
            v /= prev_w[dens_slot[d]];
        return v;
    };
    std::vector<double> icd((size_t)t->n_mean, 1.0), b_cov(cov_old.size()), b_mix((size_t)n_mix, 0.0);
    std::vector<char>   b_mix_set((size_t)n_mix, 0);
    for (size_t n = 0; n < cov_old.size(); ++n) {
        if (c.iteration_constants == AMX_EBW_IC_GLOBAL_RWTH) {   // GlobalIcb (:344-375)
            double ic = 1;
            for (uint32_t d : cov_dens[n])
                ic = cmax(ic, cmax(d_k(d), dk_min[n]));
            b_cov[n] = ic * c.step_size;
        }
        else   // LocalIcb (:408-438)
            for (uint32_t d : cov_dens[n]) {
                const size_t m = (size_t)dens_mix[d];
                if (!b_mix_set[m])
                    b_mix[m] = c.step_size * cmax(1.0, dk_min[n]), b_mix_set[m] = 1;
                b_mix[m] = cmax(c.step_size * d_k(d), b_mix[m]);
            }
    }
    for (size_t n = 0; n < cov_old.size(); ++n)
        for (uint32_t d : cov_dens[n]) {   // set (:477-484, :520-527)
            double ic = c.iteration_constants == AMX_EBW_IC_GLOBAL_RWTH ? b_cov[n] : b_mix[(size_t)dens_mix[d]];
            ic *= prev_w[dens_slot[d]];
            ic = cmax(c.minimum_icd, ic);
            AMX_REQUIRE(std::isfinite(ic) && ic >= 0, AMX_ERR_INVALID, "%s: the iteration constant of density %u is %g (the reference verifies that it is finite and not negative)",
                        who, d, ic);
            icd[t->dens_mean[d]] = ic;
        }

    std::unique_ptr<amx_mixture_set> r(new amx_mixture_set);
    r->dim = dim;
    r->mix_off.assign(1, 0);
    // estimateMixtureWeights (EbwDiscriminativeMixtureEstimator.cc:39-91), estimate (:123-136)
    int                 n_clamped = 0;
    std::vector<double> w, kk, lw;
    std::vector<char>   was_clamped;
    std::vector<std::vector<uint32_t>> out_slots = mixtures;
    std::vector<std::vector<double>>   out_lw((size_t)n_mix);
    auto log_exp_norm = [](const std::vector<double>& v) {   // Mm/Utilities.hh:43-51
        size_t mx = 0;
        for (size_t i = 1; i < v.size(); ++i)
            if (v[mx] < v[i])
                mx = i;
        double s = 0;
        for (size_t i = 0; i < v.size(); ++i)
            if (i != mx)
                s += std::exp(v[i] - v[mx]);
        return std::log1p(s) + v[mx];
    };
    for (int m = 0; m < n_mix; ++m) {
        const std::vector<uint32_t>& slots = mixtures[(size_t)m];
        const size_t                 n     = slots.size();
        double                       total = 0.0;
        for (uint32_t k : slots)
            total += W[k];
        auto weight = [&](uint32_t k) { return ism ? mad(i_w[k], cw, W[k]) : W[k]; };
        if (n > 1 && total > DBL_EPSILON) {
            w.assign(n, 0.0), kk.assign(n, 0.0), was_clamped.assign(n, 0);
            double k_max = 0;
            for (size_t i = 0; i < n; ++i) {
                w[i] = prev_w[slots[i]];
                if (w[i] > DBL_EPSILON)
                    k_max = cmax(k_max, DW[slots[i]] / w[i]);
                else
                    w[i] = 0;
            }
            for (size_t i = 0; i < n; ++i)
                if (w[i] > 0)
                    kk[i] = k_max - DW[slots[i]] / w[i];
            for (int it = 0; it < c.number_of_iterations; ++it) {
                for (size_t i = 0; i < n; ++i) {
                    if (w[i] > 0)
                        w[i] = mad(kk[i], w[i], weight(slots[i]));
                    if (w[i] < 0) {
                        w[i] = 0;
                        if (!was_clamped[i])
                            was_clamped[i] = 1, ++n_clamped;
                    }
                }
                if (c.normalize_mixture_weights) {
                    double s = 0;
                    for (double v : w)
                        s += v;
                    if (s > DBL_MIN)
                        for (double& v : w)
                            v = v / s;
                    else
                        std::fill(w.begin(), w.end(), 1 / (double)n);
                }
            }
        }
        else
            w.assign(n, c.normalize_mixture_weights ? 1 / (double)n : 1.0);
        lw.resize(n);
        for (size_t i = 0; i < n; ++i)
            lw[i] = w[i] > 0 ? std::log(w[i]) : -DBL_MAX;   // Mixture::addDensity (Mixture.cc:63-66)
        if (c.normalize_mixture_weights && n) {
            const double norm = log_exp_norm(lw);
            for (double& v : lw)
                v -= norm;
        }
        out_lw[(size_t)m] = lw;
    }
    // EbwDiscriminativeMeanEstimator::estimate (EbwDiscriminativeGaussDensityEstimator.cc:73-89)
    int n_fallback = 0;
    r->means.assign(mean_old.size() * D, 0.f);
    for (size_t n = 0; n < mean_old.size(); ++n) {
        const uint32_t j      = mean_old[n];
        const double   weight = dt_weight(j) + icd[j];
        for (size_t i = 0; i < D; ++i)
            r->means[n * D + i] = weight > 0 ? (float)(mad(icd[j], (double)pm[j * D + i], dt_sum(j, i)) / weight) : pm[j * D + i];
        n_fallback += !(weight > 0);
    }
    // EbwDiscriminativeCovarianceEstimator::estimate (:165-198)
    int         n_floored = 0;
    const float min_var   = (float)c.min_variance;
    r->variances.assign(cov_old.size() * D, 0.f);
    for (size_t n = 0; n < cov_old.size(); ++n) {
        double weight = 0;
        for (size_t i = 0; i < D; ++i)
            num[i] = cov_dt_sum(n, i);
        for (uint32_t j : cov_means[n]) {
            const double tmp = dt_weight(j) + icd[j];
            weight += tmp;
            for (size_t i = 0; i < D; ++i) {
                const double mean     = (double)r->means[(size_t)new_mean[j] * D + i];
                double       prev_sum = (double)pv[cov_old[n] * D + i];
                prev_sum += (double)(pm[j * D + i] * pm[j * D + i]);   // MeanType * MeanType: an f32 product
                prev_sum *= icd[j];
                num[i] = num[i] + (fused ? __builtin_fma(-(tmp * mean), mean, prev_sum) : prev_sum - tmp * mean * mean);
            }
        }
        AMX_REQUIRE(weight > 0, AMX_ERR_INVALID, "%s: covariance %u: the summed weight %g is not positive (the reference verifies that it is)", who, cov_old[n], weight);
        for (size_t i = 0; i < D; ++i) {
            float v = (float)(num[i] / weight);
            AMX_REQUIRE(v > 0, AMX_ERR_INVALID, "%s: covariance %u: component %zu of the estimated variance is %g, not positive (the reference verifies isPositiveDefinite)",
                        who, cov_old[n], i, (double)v);
            if (min_var != 0 && v < min_var)
                v = min_var, ++n_floored;
            r->variances[n * D + i] = v;
        }
    }
    // the i-smoothing objective on the new set (ISmoothingMixtureSetEstimator.cc:96-115, ISmoothingMixtureEstimator.cc:54-61,
    // ISmoothingGaussDensityEstimator.cc:73-89)
    double i_objective = 0;
    if (ism) {
        double of_w = 0, of_m = 0;
        for (int m = 0; m < n_mix; ++m) {
            double s = 0;
            for (size_t i = 0; i < mixtures[(size_t)m].size(); ++i) {
                const double pw = std::exp(out_lw[(size_t)m][i]);
                s               = mad(i_w[mixtures[(size_t)m][i]], std::log(cmax(pw, DBL_MIN)), s);
            }
            of_w += cw * s;
        }
        for (size_t n = 0; n < cov_old.size(); ++n) {
            double       s    = 0;
            const double size = (double)cov_means[n].size();
            for (size_t i = 0; i < D; ++i) {
                const float sig = r->variances[n * D + i];
                s               = mad(size, std::log(2 * M_PI * sig), s);
                double tt       = i_sum[n][i];
                for (uint32_t j : cov_means[n]) {
                    const float p = r->means[(size_t)new_mean[j] * D + i];
                    tt += p * (p - 2 * im[j * D + i]);   // f32 arithmetic throughout
                }
                s += tt / sig;
            }
            of_m += -0.5 * cm * s;
        }
        i_objective = of_w + of_m;
    }
    // finalize (DiscriminativeMixtureSetEstimator.cc:92-98): Mixture::removeDensitiesWithLowWeight (Mixture.cc:113-129), whose
    // densityIndexWithMaxWeight compares two iterators and so protects no density
    if (c.min_relative_weight != 0)
        for (int m = 0; m < n_mix; ++m) {
            std::vector<double>& v = out_lw[(size_t)m];
            if (v.empty())
                continue;
            const double limit = std::exp(log_exp_norm(v)) * c.min_relative_weight;
            for (size_t i = 0; i < v.size();) {
                if (std::exp(v[i]) < limit) {
                    v.erase(v.begin() + (long)i);
                    out_slots[(size_t)m].erase(out_slots[(size_t)m].begin() + (long)i);
                }
                else
                    ++i;
            }
            if (c.normalize_mixture_weights && !v.empty()) {
                const double norm = log_exp_norm(v);
                for (double& x : v)
                    x -= norm;
            }
        }
    for (int m = 0; m < n_mix; ++m) {
        for (size_t i = 0; i < out_slots[(size_t)m].size(); ++i) {
            r->dens_index.push_back((uint32_t)new_dens[t->dens_index[out_slots[(size_t)m][i]]]);
            r->log_weight.push_back(out_lw[(size_t)m][i]);
        }
        r->mix_off.push_back((uint32_t)r->dens_index.size());
    }
    for (uint32_t d : dens_old) {
        r->dens_mean.push_back((uint32_t)new_mean[t->dens_mean[d]]);
        r->dens_cov.push_back((uint32_t)new_cov[t->dens_cov[d]]);
    }
    if (iteration_constants)
        for (size_t n = 0; n < mean_old.size(); ++n)
            iteration_constants[n] = icd[mean_old[n]];
    if (info) {
        info->i_smoothing_objective = i_objective, info->sigma_minimum = sigma;
        info->n_removed = n_removed, info->n_clamped = n_clamped, info->n_mean_fallback = n_fallback, info->n_floored = n_floored;
    }
    *out = r.release();
    return AMX_OK;
}

}  // extern "C"
