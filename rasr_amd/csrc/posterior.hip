// posterior.hip -- two consumers of a [frames x emissions] score matrix that is already on the device (include/amx.h, sections "State
// posteriors" and "Model combination"): Mm::StatePosteriorFeatureScorer with viterbi = true, and Mm::CombinedFeatureScorer.
//
// posterior_kernel: one group (a wave for rows up to kPostWaveRow mixtures, four waves above) per frame, three passes over the row.  A
// pass re-reads the f32 row (from L2 or the Infinity Cache; 40 KB at 10 000 mixtures) and forms s = prior + scale * score again, which costs one
// conversion and one multiply-add, instead of staging 80 KB of f64 in LDS, which would leave one group per CU.
//   pass 1  the minimum of s and its first index (strict <, as StatePosteriorFeatureScorer.cc:49-52)
//   pass 2  the f64 sum of exp(min - stored) over the survivors other than the minimum, and the survivors' count
//   pass 3  exp(p - log1p(sum)) per survivor, 0 elsewhere; the survivors compacted in index order by ballot and prefix count
// The sum's order is fixed per row: every lane adds its own elements in increasing index order (element e belongs to lane (e / 4) % lanes),
// then a butterfly over the lanes of a wave and the waves' sums in wave order.  Nothing depends on the other frames of a call.
// The library is compiled with -ffp-contract=off; mad<FMA> marks the one site the reference's -march=native build contracts
// (`prior + scale_ * scorer->score(mix)`, cc:43 and cc:265; tests/golden/ref_posterior.npz records that it does).
// combine_kernel: one lane per (frame, emission), the models' terms added in model order, each product rounded before it is added.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.hpp"

struct amx_posterior {
    amx_ctx*          ctx = nullptr;
    amx_posterior_cfg cfg{};
    std::vector<double>   filter;      // [n_mixtures] prior as set; NaN: not in the filter
    std::vector<int>      disregard;   // erased from the filter as mixture indices (StatePosteriorFeatureScorer.hh:148-154)
    std::vector<double>   effective;   // filter without the disregarded mixtures
    bool                  plain = true;   // every mixture with prior 0: no prior table is read
    bool                  prior_stale = true;
    std::vector<uint32_t> topo_off, topo;   // CSR: densities of mixture m = topo[topo_off[m] .. topo_off[m + 1])
    bool                  monotone = false, topo_stale = true;
    long long             shared_density = -1;
    amx::DevBuf<double>   d_prior;
    amx::DevBuf<uint32_t> d_topo_off, d_topo, d_best;
    amx::DevBuf<float>    d_gmm;
    amx::DevBuf<long long>          d_list_off;
    amx::DevBuf<unsigned long long> d_count;   // [0]: frames without a minimum
};

struct amx_combine {
    amx_ctx* ctx = nullptr;
    int      n_models = 0, n_emissions = 0;
    unsigned identity = 0;   // bit i: column i of the table is 0, 1, 2, ...
    int      n_mixtures[AMX_COMBINE_MAX_MODELS] = {};
    float    scale[AMX_COMBINE_MAX_MODELS]      = {};
    std::vector<int32_t>  table;   // [n_models][n_emissions]
    bool                  stale = true;
    amx::DevBuf<int32_t>  d_table;
};

namespace amx {

constexpr int kPostThreads = 256;
constexpr int kPostWaveRow = 256;   // rows up to this many mixtures take one wave (at most one pass of four elements per lane)
constexpr int kCombineThreads = 256;
constexpr int kCombinePerLane = 4;

struct PostArgs {
    const float*    scores;
    long long       ld;
    int             n, vec;     // vec: every row starts on a 16-byte boundary
    int             vec32, vec64;   // the same for the rows of out32 / out64: whole groups of four leave as 16-byte non-temporal stores
    const double*   prior;      // NULL: every mixture, prior 0
    double          scale, threshold, margin;
    int             prune, likelihood;
    const uint32_t* best;       // density-keyed mode, else NULL
    long long       best_ld;
    const uint32_t* topo_off;
    const uint32_t* topo;
    const int32_t*  margin_mixture;
    float*          out32;
    long long       out32_ld;
    double*         out64;
    long long       out64_ld;
    double*         log_z;
    double*         min_score;
    int32_t*        min_index;
    int32_t*        n_survivors;
    int32_t*        sp_index;
    float*          sp_value;
    int32_t*        sp_count;
    int             capacity;
    unsigned long long* no_minimum;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1)
        v += __shfl_xor(v, k, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1)
        v += __shfl_xor(v, k, 64);
    return v;
}
// the smaller value; on equal values the smaller index (idx < 0: no value)
__device__ __forceinline__ void wave_min(double& v, int& idx) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const double ov = __shfl_xor(v, k, 64);
        const int    oi = __shfl_xor(idx, k, 64);
        if (oi >= 0 && (idx < 0 || ov < v || (ov == v && oi < idx))) {
            v   = ov;
            idx = oi;
        }
    }
}

typedef float  f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// the four scores of elements e0 .. e0 + 3 of a row of n; elements past the row read as 0 and are never used
__device__ __forceinline__ void load4(const float* __restrict__ row, int e0, int n, int vec, float x[4]) {
    if (vec && e0 + 3 < n) {
        const float4 v = *reinterpret_cast<const float4*>(row + e0);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    }
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            x[j] = e0 + j < n ? row[e0 + j] : 0.f;
    }
}

template<int NT, bool FMA>
__global__ __launch_bounds__(NT) void posterior_kernel(PostArgs a) {
    constexpr int NW = NT / 64;
    __shared__ double   sh_d[NW];
    __shared__ int      sh_i[NW];
    __shared__ int      sh_c[2][NW];
    const long long     t    = blockIdx.x;
    const int           tid  = threadIdx.x;
    const int           lane = tid & 63, wave = tid >> 6;
    const int           n    = a.n;
    const float*        row  = a.scores + t * a.ld;
    const int           chunks = (n + NT * 4 - 1) / (NT * 4);
    const int           mm   = a.margin_mixture ? a.margin_mixture[t] : -1;

    // pass 1: the minimum of the un-margined values (cc:49-52, cc:91-94)
    double mn = DBL_MAX;
    int    mi = -1;
    for (int c = 0; c < chunks; ++c) {
        const int e0 = (c * NT + tid) * 4;
        float     x[4];
        load4(row, e0, n, a.vec, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = e0 + j;
            if (m >= n)
                continue;
            const double pr = a.prior ? a.prior[m] : 0.0;
            if (pr != pr)
                continue;
            const double s = mad<FMA>(a.scale, (double)x[j], pr);
            if (s < mn) {
                mn = s;
                mi = m;
            }
        }
    }
    wave_min(mn, mi);
    if (NW > 1) {
        if (lane == 0) {
            sh_d[wave] = mn;
            sh_i[wave] = mi;
        }
        __syncthreads();
        mn = sh_d[0], mi = sh_i[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const double ov = sh_d[w];
            const int    oi = sh_i[w];
            if (oi >= 0 && (mi < 0 || ov < mn || (ov == mn && oi < mi))) {
                mn = ov;
                mi = oi;
            }
        }
        __syncthreads();
    }
    const bool none = mi < 0 || !(mn >= -DBL_MAX);   // no mixture below DBL_MAX, or the minimum is -inf
    if (none) {
        for (int m = tid; m < n; m += NT) {
            if (a.out32)
                a.out32[t * a.out32_ld + m] = 0.f;
            if (a.out64)
                a.out64[t * a.out64_ld + m] = 0.0;
        }
        if (tid == 0) {
            if (a.log_z && !a.likelihood)
                a.log_z[t] = 0.0;
            if (a.min_score)
                a.min_score[t] = DBL_MAX;
            if (a.min_index)
                a.min_index[t] = -1;
            if (a.n_survivors)
                a.n_survivors[t] = 0;
            if (a.sp_count)
                a.sp_count[t] = 0;
            atomicAdd(a.no_minimum, 1ull);
        }
        return;
    }
    const double limit = a.threshold + mn;   // pruneScores (cc:105-107)

    // pass 2: sum of exp(min - stored) over the survivors except the minimum's entry (cc:131-138)
    double sum = 0.0;
    int    cnt = 0;
    for (int c = 0; c < chunks; ++c) {
        const int e0 = (c * NT + tid) * 4;
        float     x[4];
        load4(row, e0, n, a.vec, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = e0 + j;
            if (m >= n)
                continue;
            const double pr = a.prior ? a.prior[m] : 0.0;
            if (pr != pr)
                continue;
            double s = mad<FMA>(a.scale, (double)x[j], pr);
            if (m == mm)
                s += a.margin;   // cc:46-48: on the stored score only
            if (a.prune && !(s < limit))
                continue;
            ++cnt;
            if (m != mi && !a.likelihood)
                sum += exp(mn - s);
        }
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    if (NW > 1) {
        if (lane == 0) {
            sh_d[wave] = sum;
            sh_i[wave] = cnt;
        }
        __syncthreads();
        sum = sh_d[0], cnt = sh_i[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            sum += sh_d[w];
            cnt += sh_i[w];
        }
    }
    const double log_zs = log1p(sum);   // cc:139
    if (tid == 0) {
        if (a.log_z && !a.likelihood)
            a.log_z[t] = log_zs - mn;   // cc:143
        if (a.min_score)
            a.min_score[t] = mn;
        if (a.min_index)
            a.min_index[t] = mi;
        if (a.n_survivors)
            a.n_survivors[t] = cnt;
        if (a.sp_count)
            a.sp_count[t] = cnt;
    }

    // pass 3: the posteriors (cc:140-142) or likelihoods (cc:163-165); the survivors in index order
    const unsigned long long below = (1ull << lane) - 1ull;
    int                      base  = 0;
    for (int c = 0; c < chunks; ++c) {
        const int e0 = (c * NT + tid) * 4;
        float     x[4];
        load4(row, e0, n, a.vec, x);
        double v[4];
        bool   live[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = e0 + j;
            live[j]     = false;
            v[j]        = 0.0;
            if (m >= n)
                continue;
            const double pr = a.prior ? a.prior[m] : 0.0;
            if (pr == pr) {
                double s = mad<FMA>(a.scale, (double)x[j], pr);
                if (m == mm)
                    s += a.margin;
                if (!a.prune || s < limit) {
                    live[j] = true;
                    v[j]    = a.likelihood ? exp(-s) : exp((mn - s) - log_zs);
                }
            }
        }
        // the dense matrices are written once and read by a later kernel or the host: streamed past L2, 16 bytes a lane where the rows allow
        if (a.out32 && e0 < n) {
            float* o = a.out32 + t * a.out32_ld + e0;
            if (a.vec32 && e0 + 3 < n)
                nt_store(f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]}, reinterpret_cast<f32x4*>(o));
            else
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e0 + j < n)
                        nt_store((float)v[j], o + j);
        }
        if (a.out64 && e0 < n) {
            double* o = a.out64 + t * a.out64_ld + e0;
            if (a.vec64 && e0 + 3 < n) {
                nt_store(f64x2{v[0], v[1]}, reinterpret_cast<f64x2*>(o));
                nt_store(f64x2{v[2], v[3]}, reinterpret_cast<f64x2*>(o + 2));
            }
            else
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e0 + j < n)
                        nt_store(v[j], o + j);
        }
        if (a.sp_index) {   // wave-uniform
            int before = 0, total = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long b = __ballot(live[j]);
                before += __popcll(b & below);
                total += __popcll(b);
            }
            int pos = base + before;
            if (NW > 1) {
                if (lane == 0)
                    sh_c[c & 1][wave] = total;
                __syncthreads();
                total = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const int wt = sh_c[c & 1][w];
                    if (w < wave)
                        pos += wt;
                    total += wt;
                }
            }
            base += total;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!live[j])
                    continue;
                if (pos < a.capacity) {
                    const int m = e0 + j;
                    int key = m;
                    if (a.best) {   // a best density past the mixture's list is read as its last one, never out of the table
                        const uint32_t k0 = a.topo_off[m], k1 = a.topo_off[m + 1];
                        const uint32_t k  = k0 + a.best[t * a.best_ld + m];
                        key               = (int)a.topo[k < k1 ? k : k1 - 1];
                    }
                    a.sp_index[t * a.capacity + pos] = key;
                    a.sp_value[t * a.capacity + pos] = (float)v[j];
                }
                ++pos;
            }
        }
    }
}

struct ListArgs {
    const float*     scores;
    long long        ld;
    int              n;
    double           scale;
    const long long* off;       // [T + 1]
    const int32_t*   mixture;
    const double*    prior;
    double*          out64;
    float*           out32;
    unsigned long long* no_minimum;
};

// posteriorsAndMixtures(IndicesAndWeights&) (cc:258-284): one wave per frame, entry i of the list belongs to lane i % 64
template<bool FMA>
__global__ __launch_bounds__(64) void posterior_list_kernel(ListArgs a) {
    const long long t    = blockIdx.x;
    const int       lane = threadIdx.x;
    const long long b = a.off[t], e = a.off[t + 1];
    if (e <= b)
        return;
    const float* row = a.scores + t * a.ld;
    auto score_of = [&](long long i) {
        const int m = a.mixture[i];
        // an index outside the model is never read: its score is +inf
        const double x = m >= 0 && m < a.n ? (double)row[m] : (double)INFINITY;
        return mad<FMA>(a.scale, x, a.prior[i]);   // cc:265
    };
    double mn = DBL_MAX;
    int    mi = -1;
    for (long long i = b + lane; i < e; i += 64) {
        const double s = score_of(i);
        if (s < mn) {
            mn = s;
            mi = (int)(i - b);
        }
    }
    wave_min(mn, mi);
    double sum = 0.0;
    for (long long i = b + lane; i < e; i += 64)
        if ((int)(i - b) != mi)
            sum += exp(mn - score_of(i));   // cc:274-277
    sum                 = wave_sum(sum);
    const double log_z  = log1p(sum);
    const bool   none   = mi < 0 || !(mn >= -DBL_MAX);
    for (long long i = b + lane; i < e; i += 64) {
        const double p = none ? 0.0 : exp((mn - score_of(i)) - log_z);   // cc:282
        if (a.out64)
            a.out64[i] = p;
        if (a.out32)
            a.out32[i] = (float)p;
    }
    if (none && lane == 0)
        atomicAdd(a.no_minimum, 1ull);
}

struct CombineArgs {
    const float*   s[AMX_COMBINE_MAX_MODELS];
    long long      ld[AMX_COMBINE_MAX_MODELS];
    float          scale[AMX_COMBINE_MAX_MODELS];
    const int32_t* table;   // [n_models][n_emissions]
    unsigned       identity;
    int            n_models, n_emissions, chunks;
    float*         out;
    long long      out_ld;
};

// CombinedContextScorer::score (CombinedFeatureScorer.cc:42-59) with ScaledContextScorer::score (ScaledFeatureScorer.hh:65-67)
__global__ __launch_bounds__(kCombineThreads) void combine_kernel(CombineArgs a) {
    const long long t     = blockIdx.x / a.chunks;
    const int       chunk = blockIdx.x % a.chunks;
#pragma unroll
    for (int j = 0; j < kCombinePerLane; ++j) {
        const int e = (chunk * kCombinePerLane + j) * kCombineThreads + threadIdx.x;
        if (e >= a.n_emissions)
            continue;
        float r = 0.f;   // :43
        for (int i = 0; i < a.n_models; ++i) {
            const int   m    = (a.identity >> i) & 1u ? e : a.table[(long long)i * a.n_emissions + e];
            const float term = a.scale[i] * a.s[i][t * a.ld[i] + m];   // the callee's return value: rounded
            r += term;                                                  // :53
        }
        nt_store(r, a.out + t * a.out_ld + e);
    }
}

static void posterior_effective(amx_posterior* h, std::vector<double>* eff) {
    *eff = h->filter;
    for (int d : h->disregard)
        if (d >= 0 && d < (int)eff->size())
            (*eff)[d] = std::nan("");
}

static bool posterior_empty(const std::vector<double>& eff) {
    for (double p : eff)
        if (p == p)
            return false;
    return true;
}

static void posterior_commit(amx_posterior* h, std::vector<double>&& eff) {
    h->effective = std::move(eff);
    h->plain     = true;
    for (double p : h->effective)
        if (p != p || p != 0.0)
            h->plain = false;
    h->prior_stale = true;
}

static int posterior_topology(amx_posterior* h, const uint32_t* off, const uint32_t* dens, const char* who) {
    const int n = h->cfg.n_mixtures;
    AMX_REQUIRE(off && dens, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(off[0] == 0, AMX_ERR_INVALID, "%s: mix_offsets[0] is %u, not 0", who, off[0]);
    for (int m = 0; m < n; ++m)
        AMX_REQUIRE(off[m] < off[m + 1], AMX_ERR_INVALID, "%s: mixture %d has no density", who, m);
    h->topo_off.assign(off, off + n + 1);
    h->topo.assign(dens, dens + off[n]);
    h->monotone       = true;
    h->shared_density = -1;
    // monotone: every density of mixture m is below every density of mixture m + 1, so keys sort as mixtures do
    uint32_t prev_max = 0;
    for (int m = 0; m < n; ++m) {
        uint32_t lo = UINT_MAX, hi = 0;
        for (uint32_t k = off[m]; k < off[m + 1]; ++k)
            lo = std::min(lo, dens[k]), hi = std::max(hi, dens[k]);
        if (m && lo <= prev_max)
            h->monotone = false;
        prev_max = m ? std::max(prev_max, hi) : hi;
    }
    std::vector<std::pair<uint32_t, int>> owner;
    owner.reserve(h->topo.size());
    for (int m = 0; m < n; ++m)
        for (uint32_t k = off[m]; k < off[m + 1]; ++k)
            owner.emplace_back(dens[k], m);
    std::sort(owner.begin(), owner.end());
    for (size_t i = 1; i < owner.size(); ++i)
        if (owner[i].first == owner[i - 1].first && owner[i].second != owner[i - 1].second) {
            h->shared_density = owner[i].first;
            break;
        }
    h->topo_stale = true;
    return AMX_OK;
}

}  // namespace amx

extern "C" {


void amx_posterior_default_cfg(amx_posterior_cfg* cfg) {
    if (!cfg)
        return;
    cfg->n_mixtures        = 0;
    cfg->scale             = 1.0;       // paramScale (StatePosteriorFeatureScorer.cc:299-303)
    cfg->pruning_threshold = DBL_MAX;   // paramPruningThreshold (:289-292)
    cfg->margin            = 0.0;       // paramMargin (:305-309)
    cfg->viterbi           = 1;         // paramViterbi (:294-297)
}

int amx_posterior_create(amx_ctx* ctx, const amx_posterior_cfg* cfg, amx_posterior** out) {
    AMX_REQUIRE(out, AMX_ERR_INVALID, "amx_posterior_create: NULL argument");
    *out = nullptr;
    AMX_REQUIRE(cfg, AMX_ERR_INVALID, "amx_posterior_create: NULL argument");
    AMX_REQUIRE(cfg->n_mixtures >= 1, AMX_ERR_INVALID, "amx_posterior_create: n_mixtures is %d", cfg->n_mixtures);
    AMX_REQUIRE(cfg->viterbi, AMX_ERR_UNSUPPORTED,
                "amx_posterior_create: viterbi = false needs the score of every density of a mixture, which no scorer of this library exports");
    AMX_REQUIRE(cfg->scale == cfg->scale && cfg->pruning_threshold == cfg->pruning_threshold && cfg->margin == cfg->margin, AMX_ERR_INVALID,
                "amx_posterior_create: scale, pruning_threshold or margin is not a number");
    std::unique_ptr<amx_posterior> h(new amx_posterior);
    h->ctx = ctx;
    h->cfg = *cfg;
    h->filter.assign((size_t)cfg->n_mixtures, 0.0);   // DefaultFilter (:361-368)
    amx::posterior_commit(h.get(), std::vector<double>(h->filter));
    *out = h.release();
    return AMX_OK;
}

void amx_posterior_destroy(amx_posterior* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_posterior_set_filter(amx_posterior* h, int n, const int* mixture, const double* prior) {
    const char* who = "amx_posterior_set_filter";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n >= 1 && mixture, AMX_ERR_INVALID, "%s: the filter is empty", who);
    std::vector<double> f((size_t)h->cfg.n_mixtures, std::nan(""));
    for (int i = 0; i < n; ++i) {
        AMX_REQUIRE(mixture[i] >= 0 && mixture[i] < h->cfg.n_mixtures, AMX_ERR_INVALID, "%s: mixture[%d] = %d is outside the %d mixtures", who, i, mixture[i],
                    h->cfg.n_mixtures);
        const double p = prior ? prior[i] : 0.0;
        AMX_REQUIRE(p == p, AMX_ERR_INVALID, "%s: prior[%d] is not a number", who, i);
        f[mixture[i]] = p;   // a repeated mixture keeps its last prior, as PriorMap::operator[] does
    }
    std::vector<double> old = std::move(h->filter);
    h->filter               = std::move(f);
    std::vector<double> eff;
    amx::posterior_effective(h, &eff);
    if (amx::posterior_empty(eff)) {
        h->filter = std::move(old);
        AMX_REQUIRE(false, AMX_ERR_INVALID, "%s: the filter is empty once the disregard list is erased from it", who);
    }
    amx::posterior_commit(h, std::move(eff));
    return AMX_OK;
}

int amx_posterior_set_default_filter(amx_posterior* h) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_posterior_set_default_filter: NULL handle");
    std::vector<int> all((size_t)h->cfg.n_mixtures);
    for (int m = 0; m < h->cfg.n_mixtures; ++m)
        all[m] = m;
    return amx_posterior_set_filter(h, h->cfg.n_mixtures, all.data(), nullptr);
}

int amx_posterior_set_single_filter(amx_posterior* h, int mixture) {   // SingleMixtureFilter (:380-385)
    return amx_posterior_set_filter(h, 1, &mixture, nullptr);
}

int amx_posterior_set_disregard(amx_posterior* h, int n, const int* numbers) {
    const char* who = "amx_posterior_set_disregard";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n >= 0 && (n == 0 || numbers), AMX_ERR_INVALID, "%s: n is %d", who, n);
    std::vector<int> old = std::move(h->disregard);
    h->disregard.assign(numbers, numbers + n);
    std::vector<double> eff;
    amx::posterior_effective(h, &eff);
    if (amx::posterior_empty(eff)) {
        h->disregard = std::move(old);
        AMX_REQUIRE(false, AMX_ERR_INVALID, "%s: the filter is empty once the disregard list is erased from it", who);
    }
    amx::posterior_commit(h, std::move(eff));
    return AMX_OK;
}

int amx_posterior_filter(const amx_posterior* h, int* n, int* mixture, double* prior) {
    AMX_REQUIRE(h && n, AMX_ERR_INVALID, "amx_posterior_filter: NULL argument");
    int k = 0;
    for (int m = 0; m < h->cfg.n_mixtures; ++m) {
        if (h->effective[m] != h->effective[m])
            continue;
        if (mixture)
            mixture[k] = m;
        if (prior)
            prior[k] = h->effective[m];
        ++k;
    }
    *n = k;
    return AMX_OK;
}

int amx_posterior_set_topology(amx_posterior* h, const uint32_t* mix_offsets, const uint32_t* dens_index) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_posterior_set_topology: NULL handle");
    return amx::posterior_topology(h, mix_offsets, dens_index, "amx_posterior_set_topology");
}

int amx_posterior_set_topology_gmm(amx_posterior* h, const amx_gmm* gmm) {
    const char* who = "amx_posterior_set_topology_gmm";
    AMX_REQUIRE(h && gmm, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(amx_gmm_n_mixtures(gmm) == h->cfg.n_mixtures, AMX_ERR_INVALID, "%s: the model has %d mixtures, the handle %d", who, amx_gmm_n_mixtures(gmm),
                h->cfg.n_mixtures);
    int nk = 0;
    AMX_TRY(amx_gmm_topology(gmm, &nk, nullptr, nullptr));
    std::vector<uint32_t> off((size_t)h->cfg.n_mixtures + 1), dens((size_t)std::max(nk, 1));
    AMX_TRY(amx_gmm_topology(gmm, &nk, off.data(), dens.data()));
    return amx::posterior_topology(h, off.data(), dens.data(), who);
}

int amx_posterior_topology_info(const amx_posterior* h, int* monotone, long long* shared_density) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_posterior_topology_info: NULL handle");
    AMX_REQUIRE(!h->topo_off.empty(), AMX_ERR_STATE, "amx_posterior_topology_info: no topology was set");
    if (monotone)
        *monotone = h->monotone ? 1 : 0;
    if (shared_density)
        *shared_density = h->shared_density;
    return AMX_OK;
}

int amx_posterior_dev(amx_posterior* h, int mode, const float* scores_dev, int scores_ld, int T, const uint32_t* best_density_dev, int best_ld,
                      const int32_t* margin_mixture_dev, const amx_posterior_out* out, unsigned long long* no_minimum) {
    const char* who = "amx_posterior_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    const int n = h->cfg.n_mixtures;
    AMX_REQUIRE(mode == AMX_POSTERIOR_MIXTURE || mode == AMX_POSTERIOR_LIKELIHOOD || mode == AMX_POSTERIOR_DENSITY, AMX_ERR_INVALID, "%s: mode %d", who, mode);
    AMX_REQUIRE(T >= 0 && scores_ld >= n, AMX_ERR_INVALID, "%s: T %d, scores_ld %d with %d mixtures", who, T, scores_ld, n);
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL out", who);
    AMX_REQUIRE((!out->posterior_f32_dev || out->posterior_f32_ld >= n) && (!out->posterior_f64_dev || out->posterior_f64_ld >= n), AMX_ERR_INVALID,
                "%s: posterior_f32_ld %d, posterior_f64_ld %d with %d mixtures", who, out->posterior_f32_ld, out->posterior_f64_ld, n);
    const bool sparse = out->sparse_index_dev || out->sparse_value_dev || out->sparse_count_dev;
    AMX_REQUIRE(!sparse || (out->sparse_index_dev && out->sparse_value_dev && out->sparse_count_dev && out->sparse_capacity >= 0), AMX_ERR_INVALID,
                "%s: the sparse form needs sparse_index_dev, sparse_value_dev, sparse_count_dev and sparse_capacity >= 0", who);
    const bool density = mode == AMX_POSTERIOR_DENSITY;
    if (density) {
        AMX_REQUIRE(!h->topo_off.empty(), AMX_ERR_STATE, "%s: density-keyed posteriors need a topology (amx_posterior_set_topology)", who);
        AMX_REQUIRE(h->shared_density < 0, AMX_ERR_UNSUPPORTED,
                    "%s: density %lld belongs to two mixtures; what the reference stores under it depends on its hash order", who, h->shared_density);
        AMX_REQUIRE(T == 0 || (best_density_dev && best_ld >= n), AMX_ERR_INVALID, "%s: density-keyed posteriors need best_density_dev with best_ld >= %d", who, n);
    }
    else
        AMX_REQUIRE(!margin_mixture_dev, AMX_ERR_INVALID, "%s: margin_mixture_dev acts in density-keyed mode only (workMixtureScores has no margin)", who);
    if (no_minimum)
        *no_minimum = 0;
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(scores_dev, AMX_ERR_INVALID, "%s: NULL scores_dev", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    if (!h->plain && h->prior_stale) {
        AMX_HIP(hipStreamSynchronize(ctx->stream));   // an earlier call may still read the old table
        AMX_TRY(h->d_prior.upload(h->effective.data(), h->effective.size()));
        h->prior_stale = false;
    }
    if (density && h->topo_stale) {
        AMX_HIP(hipStreamSynchronize(ctx->stream));
        AMX_TRY(h->d_topo_off.upload(h->topo_off.data(), h->topo_off.size()));
        AMX_TRY(h->d_topo.upload(h->topo.data(), h->topo.size()));
        h->topo_stale = false;
    }
    AMX_TRY(h->d_count.reserve(1));
    AMX_HIP(hipMemsetAsync(h->d_count.get(), 0, sizeof(unsigned long long), ctx->stream));
    amx::PostArgs a{};
    a.scores = scores_dev, a.ld = scores_ld, a.n = n;
    a.vec    = ((uintptr_t)scores_dev % 16 == 0 && scores_ld % 4 == 0) ? 1 : 0;
    a.prior  = h->plain ? nullptr : h->d_prior.get();
    a.scale = h->cfg.scale, a.threshold = h->cfg.pruning_threshold, a.margin = h->cfg.margin;
    a.prune      = h->cfg.pruning_threshold < DBL_MAX ? 1 : 0;   // cc:106
    a.likelihood = mode == AMX_POSTERIOR_LIKELIHOOD ? 1 : 0;
    if (density) {
        a.best = best_density_dev, a.best_ld = best_ld, a.topo_off = h->d_topo_off.get(), a.topo = h->d_topo.get();
        a.margin_mixture = margin_mixture_dev;
    }
    a.out32 = out->posterior_f32_dev, a.out32_ld = out->posterior_f32_ld, a.out64 = out->posterior_f64_dev, a.out64_ld = out->posterior_f64_ld;
    a.vec32 = ((uintptr_t)a.out32 % 16 == 0 && a.out32_ld % 4 == 0) ? 1 : 0;
    a.vec64 = ((uintptr_t)a.out64 % 16 == 0 && a.out64_ld % 2 == 0) ? 1 : 0;
    a.log_z = out->log_z_dev, a.min_score = out->min_dev, a.min_index = out->min_index_dev, a.n_survivors = out->n_survivors_dev;
    a.sp_index = out->sparse_index_dev, a.sp_value = out->sparse_value_dev, a.sp_count = out->sparse_count_dev, a.capacity = out->sparse_capacity;
    a.no_minimum = h->d_count.get();
    const bool fma = ctx->contract == AMX_CONTRACT_FMA;
    {
        amx::ScopedKernelTimer timer(ctx, "posterior");
        const dim3 grid((unsigned)T);
        if (n <= amx::kPostWaveRow) {
            if (fma)
                hipLaunchKernelGGL((amx::posterior_kernel<64, true>), grid, dim3(64), 0, ctx->stream, a);
            else
                hipLaunchKernelGGL((amx::posterior_kernel<64, false>), grid, dim3(64), 0, ctx->stream, a);
        }
        else {
            if (fma)
                hipLaunchKernelGGL((amx::posterior_kernel<amx::kPostThreads, true>), grid, dim3(amx::kPostThreads), 0, ctx->stream, a);
            else
                hipLaunchKernelGGL((amx::posterior_kernel<amx::kPostThreads, false>), grid, dim3(amx::kPostThreads), 0, ctx->stream, a);
        }
        AMX_HIP(hipGetLastError());
    }
    if (no_minimum) {
        AMX_HIP(hipMemcpyAsync(no_minimum, h->d_count.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return AMX_OK;
}

int amx_posterior_lists_dev(amx_posterior* h, const float* scores_dev, int scores_ld, int T, const long long* list_offsets, const int32_t* mixture_dev,
                            const double* prior_dev, double* posterior_f64_dev, float* posterior_f32_dev, unsigned long long* no_minimum) {
    const char* who = "amx_posterior_lists_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    const int n = h->cfg.n_mixtures;
    AMX_REQUIRE(T >= 0 && scores_ld >= n, AMX_ERR_INVALID, "%s: T %d, scores_ld %d with %d mixtures", who, T, scores_ld, n);
    if (no_minimum)
        *no_minimum = 0;
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(list_offsets, AMX_ERR_INVALID, "%s: NULL list_offsets", who);
    std::vector<long long> off((size_t)T + 1);
    AMX_REQUIRE(list_offsets[0] >= 0, AMX_ERR_INVALID, "%s: negative list offset", who);
    for (int t = 0; t <= T; ++t) {
        AMX_REQUIRE(t == 0 || list_offsets[t - 1] <= list_offsets[t], AMX_ERR_INVALID, "%s: list offsets decrease at frame %d", who, t - 1);
        off[t] = list_offsets[t];
    }
    if (off[T] == off[0])
        return AMX_OK;
    AMX_REQUIRE(scores_dev && mixture_dev && prior_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_TRY(h->d_list_off.reserve(off.size()));
    // `off` is pageable and dies with this call: the copy is waited for (it also orders the table behind an earlier call that reads it)
    AMX_HIP(hipMemcpyAsync(h->d_list_off.get(), off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    AMX_TRY(h->d_count.reserve(1));
    AMX_HIP(hipMemsetAsync(h->d_count.get(), 0, sizeof(unsigned long long), ctx->stream));
    amx::ListArgs a{};
    a.scores = scores_dev, a.ld = scores_ld, a.n = n, a.scale = h->cfg.scale, a.off = h->d_list_off.get();
    a.mixture = mixture_dev, a.prior = prior_dev, a.out64 = posterior_f64_dev, a.out32 = posterior_f32_dev, a.no_minimum = h->d_count.get();
    {
        amx::ScopedKernelTimer timer(ctx, "posterior_list");
        if (ctx->contract == AMX_CONTRACT_FMA)
            hipLaunchKernelGGL(amx::posterior_list_kernel<true>, dim3((unsigned)T), dim3(64), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL(amx::posterior_list_kernel<false>, dim3((unsigned)T), dim3(64), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    if (no_minimum) {
        AMX_HIP(hipMemcpyAsync(no_minimum, h->d_count.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return AMX_OK;
}

int amx_posterior_gmm_dev(amx_posterior* h, amx_gmm* gmm, int gmm_mode, int mode, const float* feats_dev, int T, const int32_t* margin_mixture_dev,
                          const amx_posterior_out* out, unsigned long long* no_minimum) {
    const char* who = "amx_posterior_gmm_dev";
    AMX_REQUIRE(h && gmm, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    const int n = h->cfg.n_mixtures;
    AMX_REQUIRE(amx_gmm_n_mixtures(gmm) == n, AMX_ERR_INVALID, "%s: the model has %d mixtures, the handle %d", who, amx_gmm_n_mixtures(gmm), n);
    AMX_REQUIRE(T >= 0, AMX_ERR_INVALID, "%s: T %d", who, T);
    const bool density = mode == AMX_POSTERIOR_DENSITY;
    if (T) {
        AMX_REQUIRE(feats_dev, AMX_ERR_INVALID, "%s: NULL feats_dev", who);
        AMX_HIP(hipSetDevice(h->ctx->device));
        AMX_TRY(h->d_gmm.reserve((size_t)T * n));
        if (density)
            AMX_TRY(h->d_best.reserve((size_t)T * n));
        AMX_TRY(amx_gmm_score_dev(gmm, gmm_mode, feats_dev, T, h->d_gmm.get(), density ? h->d_best.get() : nullptr));
    }
    return amx_posterior_dev(h, mode, h->d_gmm.get(), n, T, density ? h->d_best.get() : nullptr, n, margin_mixture_dev, out, no_minimum);
}

int amx_combine_create(amx_ctx* ctx, int n_models, int n_emissions, const int* n_mixtures, const int* table, const float* scale, amx_combine** out) {
    const char* who = "amx_combine_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(n_models >= 1 && n_models <= AMX_COMBINE_MAX_MODELS, AMX_ERR_INVALID, "%s: n_models is %d, not 1 .. %d", who, n_models,
                AMX_COMBINE_MAX_MODELS);
    AMX_REQUIRE(n_emissions >= 1, AMX_ERR_INVALID, "%s: n_emissions is %d", who, n_emissions);
    AMX_REQUIRE(n_mixtures && table && scale, AMX_ERR_INVALID, "%s: NULL argument", who);
    std::unique_ptr<amx_combine> h(new amx_combine);
    h->ctx = ctx, h->n_models = n_models, h->n_emissions = n_emissions;
    h->table.resize((size_t)n_models * n_emissions);
    for (int i = 0; i < n_models; ++i) {
        AMX_REQUIRE(n_mixtures[i] >= 1, AMX_ERR_INVALID, "%s: n_mixtures[%d] is %d", who, i, n_mixtures[i]);
        h->n_mixtures[i] = n_mixtures[i];
        h->scale[i]      = scale[i];
        bool identity    = true;
        for (int e = 0; e < n_emissions; ++e) {
            const int m = table[(size_t)e * n_models + i];
            // verifyMixtureIndexTable (CombinedFeatureScorer.cc:91-98)
            AMX_REQUIRE(m >= 0 && m < n_mixtures[i], AMX_ERR_INVALID, "%s: table[%d][%d] = %d is outside the %d mixtures of model %d", who, e, i, m,
                        n_mixtures[i], i);
            h->table[(size_t)i * n_emissions + e] = m;
            identity                             = identity && m == e;
        }
        if (identity)
            h->identity |= 1u << i;
    }
    *out = h.release();
    return AMX_OK;
}

void amx_combine_destroy(amx_combine* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_combine_identity_columns(const amx_combine* h, unsigned* mask) {
    AMX_REQUIRE(h && mask, AMX_ERR_INVALID, "amx_combine_identity_columns: NULL argument");
    *mask = h->identity;
    return AMX_OK;
}

int amx_combine_dev(amx_combine* h, int T, const float* const* scores_dev, const int* ld, float* out_dev, int out_ld) {
    const char* who = "amx_combine_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(T >= 0 && out_ld >= h->n_emissions, AMX_ERR_INVALID, "%s: T %d, out_ld %d with %d emissions", who, T, out_ld, h->n_emissions);
    AMX_REQUIRE(scores_dev && ld, AMX_ERR_INVALID, "%s: NULL argument", who);
    for (int i = 0; i < h->n_models; ++i)
        AMX_REQUIRE(ld[i] >= h->n_mixtures[i], AMX_ERR_INVALID, "%s: ld[%d] is %d with %d mixtures", who, i, ld[i], h->n_mixtures[i]);
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(out_dev, AMX_ERR_INVALID, "%s: NULL out_dev", who);
    amx::CombineArgs a{};
    for (int i = 0; i < h->n_models; ++i) {
        AMX_REQUIRE(scores_dev[i], AMX_ERR_INVALID, "%s: NULL scores_dev[%d]", who, i);
        AMX_REQUIRE(!amx::views_alias(scores_dev[i], ld[i], h->n_mixtures[i], out_dev, out_ld, h->n_emissions, T), AMX_ERR_INVALID,
                    "%s: out_dev overlaps the scores of model %d", who, i);
        a.s[i] = scores_dev[i], a.ld[i] = ld[i], a.scale[i] = h->scale[i];
    }
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    if (h->stale) {
        AMX_TRY(h->d_table.upload(h->table.data(), h->table.size()));
        h->stale = false;
    }
    a.table = h->d_table.get(), a.identity = h->identity, a.n_models = h->n_models, a.n_emissions = h->n_emissions;
    a.chunks = amx::ceil_div(h->n_emissions, amx::kCombineThreads * amx::kCombinePerLane);
    a.out = out_dev, a.out_ld = out_ld;
    const long long groups = (long long)T * a.chunks;
    AMX_REQUIRE(groups < (1ll << 31), AMX_ERR_INVALID, "%s: %d frames of %d emissions are more than one call takes", who, T, h->n_emissions);
    amx::ScopedKernelTimer timer(ctx, "combine");
    hipLaunchKernelGGL(amx::combine_kernel, dim3((unsigned)groups), dim3(amx::kCombineThreads), 0, ctx->stream, a);
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

}  // extern "C"
