// mllr.hip -- MLLR on the device (include/amx.h, section "MLLR"): the corpus pass of Mm::FullAdaptorViterbiEstimator::accumulate and
// Mm::ShiftAdaptorViterbiEstimator::accumulate (Mm/MllrAdaptation.cc:381-416, :599-653, :693-714) per key and regression class (leaf),
// and the adapted mean table of one key (FullAdaptor / ShiftAdaptor::adaptMixtureSet, :59-79, :146-170).  Files and the estimate are
// mllr_host.cpp's.
//
// Order.  Per (key, leaf, cell) the reference adds that key's frames of that leaf in corpus order into an f64.  Three steps:
//   1. mllr_resolve_kernel: every frame's (mean, covariance, leaf) and the checks, before anything is written.
//   2. mllr_lists_kernel, one workgroup per key: it walks the key's segments in ascending order twice.  The first walk counts the
//      frames of every leaf (integer counters in LDS), an exclusive scan of the counters gives every leaf's place in the key's part
//      of the list, the second walk writes every frame to (its leaf's cursor + the number of earlier frames of that leaf in the same
//      chunk of 256).  The list of a (key, leaf) is therefore ascending whatever the launch looks like; the only atomics are integer
//      additions whose sum does not depend on their order.
//   3. mllr_acc_kernel, one workgroup per (key, leaf, tile of 256 cells): it walks the list in stages of kMllrStage frames (feature
//      rows, means, variances of the shift estimator and weights in LDS); a lane owns one cell, whose chain starts from what the
//      buffer holds, stays in a register and is written back once.  No floating-point atomic, no partial sums.
// The time of step 3 is that of the longest list's dependent f64 additions; steps 1 and 2 read every frame once.
// The library is compiled with -ffp-contract=off; mad<FMA> marks the sites the reference's -march=native build contracts
// (tests/golden/ref_mllr.npz holds both builds).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "common.hpp"
#include "gmm_internal.hpp"

namespace amx {

constexpr int kMllrThreads  = 256;
constexpr int kMllrStage    = 16;     // frames staged in LDS at a time: 3 x 16 x 255 floats at most (48 KB)
constexpr int kMllrMaxDim   = 255;
constexpr int kMllrMaxKeys  = 65535;  // a key is one workgroup of mllr_lists_kernel
constexpr int kMllrMaxLeafs = 4096;   // a counter per leaf in LDS (16 KB)

struct MllrSeg {
    long long begin, end;   // frames [begin, end) of one segment
};

// ---- every frame's (mean, covariance, leaf) and the checks.  bad = min over the offending frames of (frame << 3 | kind):
// 1 emission outside the model, 2 density outside the mixture, 3 non-finite feature, 4 non-finite weight
__global__ __launch_bounds__(kMllrThreads) void mllr_resolve_kernel(const float* __restrict__ feats, long long ld, int D, long long t0, long long n,
                                                                    const int32_t* __restrict__ emission, const uint32_t* __restrict__ best, int best_ld,
                                                                    const double* __restrict__ weight, int n_mix, const uint32_t* __restrict__ mix_off,
                                                                    const uint32_t* __restrict__ k_dens, const uint32_t* __restrict__ d_mean,
                                                                    const uint32_t* __restrict__ d_cov, const int* __restrict__ leaf_of_mix,
                                                                    int* __restrict__ frame_mean, int* __restrict__ frame_cov, int* __restrict__ frame_leaf,
                                                                    unsigned long long* bad) {
    const long long i = (long long)blockIdx.x * kMllrThreads + threadIdx.x;
    if (i >= n)
        return;
    const long long t = t0 + i;
    const int32_t   e = emission[t];
    int             mi = -1, ci = -1, leaf = -1, kind = 0;
    if (e != -1) {
        if (e < 0 || e >= n_mix)
            kind = 1;
        else {
            const uint32_t kk = best_ld > 0 ? best[t * best_ld + e] : best[t];
            if (kk >= mix_off[e + 1] - mix_off[e])
                kind = 2;
            else {
                const uint32_t d = k_dens[mix_off[e] + kk];
                mi = (int)d_mean[d], ci = (int)d_cov[d], leaf = leaf_of_mix[e];
                for (int c = 0; c < D; ++c)
                    if (!isfinite(feats[t * ld + c]))
                        kind = 3;
                if (weight && !isfinite(weight[t]))
                    kind = kind ? kind : 4;
            }
        }
    }
    frame_mean[i] = kind ? -1 : mi;
    frame_cov[i]  = kind ? -1 : ci;
    frame_leaf[i] = kind ? -1 : leaf;
    if (kind)
        atomicMin(bad, ((unsigned long long)i << 3) | (unsigned long long)kind);
}

// ---- per (key, leaf) the ascending list of its frames (indices relative to t_base).  grid: x = key.  LDS: n_leafs counters.
__global__ __launch_bounds__(kMllrThreads) void mllr_lists_kernel(const int* __restrict__ key_seg, const MllrSeg* __restrict__ segs, long long t_base,
                                                                  const int* __restrict__ frame_leaf, int n_leafs, const int* __restrict__ key_base,
                                                                  int* __restrict__ list, int* __restrict__ list_start, int* __restrict__ list_count) {
    extern __shared__ int s_cnt[];   // [n_leafs]: counts, then cursors
    __shared__ int        s_leaf[kMllrThreads];
    const int key = blockIdx.x, tid = threadIdx.x;
    const int s_begin = key_seg[key], s_end = key_seg[key + 1];
    for (int l = tid; l < n_leafs; l += kMllrThreads)
        s_cnt[l] = 0;
    __syncthreads();
    for (int s = s_begin; s < s_end; ++s) {
        const MllrSeg seg = segs[s];
        for (long long t = seg.begin + tid; t < seg.end; t += kMllrThreads) {
            const int l = frame_leaf[t - t_base];
            if (l >= 0)
                atomicAdd(&s_cnt[l], 1);   // an integer count: the sum does not depend on the order
        }
    }
    __syncthreads();
    if (tid == 0) {
        int run = key_base[key];
        for (int l = 0; l < n_leafs; ++l) {
            const int c                            = s_cnt[l];
            list_start[(long long)key * n_leafs + l] = run;
            list_count[(long long)key * n_leafs + l] = c;
            s_cnt[l]                               = run;
            run += c;
        }
    }
    __syncthreads();
    for (int s = s_begin; s < s_end; ++s) {
        const MllrSeg seg = segs[s];
        for (long long t = seg.begin; t < seg.end; t += kMllrThreads) {   // all lanes run every chunk
            const bool in = t + tid < seg.end;
            const int  l  = in ? frame_leaf[t + tid - t_base] : -1;
            s_leaf[tid]   = l;
            __syncthreads();
            if (l >= 0) {
                int rank = 0;
                for (int j = 0; j < tid; ++j)
                    rank += s_leaf[j] == l;
                list[s_cnt[l] + rank] = (int)(t + tid - t_base);
            }
            __syncthreads();
            if (l >= 0)
                atomicAdd(&s_cnt[l], 1);
            __syncthreads();
        }
    }
}

struct MllrArgs {
    const float*  feats;
    long long     ld;
    int           D, n_leafs;
    long long     t_base;
    const int*    frame_mean;
    const int*    frame_cov;
    const double* weight;
    const float*  means;   // [n_mean x D]
    const float*  vars;    // [n_cov x D]
    const int*    list;
    const int*    list_start;
    const int*    list_count;
    double*       acc;
    long long     leaf_size;
};

// ---- the chains.  grid: x = key * n_leafs + leaf, y = 256 cells of the (key, leaf) block.  LDS: [stage][D] x, mean (, variance)
// full:  [count_Z | Z: D x R | count_G | G: R x R], R = D + 1 (:599-653);  shift: [count | beta: D | shift: D] (:381-416)
template<bool SHIFT, bool FMA, bool WEIGHTED>
__global__ __launch_bounds__(kMllrThreads) void mllr_acc_kernel(MllrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_w[kMllrStage];
    const int D = a.D, R = D + 1, tid = threadIdx.x;
    float*    s_x = reinterpret_cast<float*>(s_raw);   // [stage][D]
    float*    s_m = s_x + kMllrStage * D;
    float*    s_v = s_m + kMllrStage * D;              // shift only

    const long long pair  = blockIdx.x;
    const int       count = a.list_count[pair];
    if (count == 0)
        return;
    const int*      list   = a.list + a.list_start[pair];
    const long long cell   = (long long)blockIdx.y * kMllrThreads + tid;
    const bool      active = cell < a.leaf_size;
    // full: 0 a count, 1 Z[i][j], 2 G[i][j];  shift: 0 count, 1 beta[i], 2 shift[i]
    int kind = 0, i = 0, j = 0;
    if (active) {
        if (SHIFT) {
            if (cell >= 1 + D)
                kind = 2, i = (int)(cell - 1 - D);
            else if (cell >= 1)
                kind = 1, i = (int)(cell - 1);
        }
        else {
            const long long g0 = 1 + (long long)D * R;
            if (cell > g0)
                kind = 2, i = (int)((cell - g0 - 1) / R), j = (int)((cell - g0 - 1) - (long long)i * R);
            else if (cell >= 1 && cell < g0)
                kind = 1, i = (int)((cell - 1) / R), j = (int)((cell - 1) - (long long)i * R);
        }
    }
    double* p   = a.acc + pair * a.leaf_size + cell;
    double  sum = active ? *p : 0.0;

    for (int f0 = 0; f0 < count; f0 += kMllrStage) {
        const int n = count - f0 < kMllrStage ? count - f0 : kMllrStage;
        if (tid < n)
            s_w[tid] = a.weight ? a.weight[a.t_base + list[f0 + tid]] : 1.0;
        for (int idx = tid; idx < n * D; idx += kMllrThreads) {
            const int       f = idx / D, c = idx - f * D;
            const long long fi = list[f0 + f];
            s_x[idx]           = a.feats[(a.t_base + fi) * a.ld + c];
            s_m[idx]           = a.means[(long long)a.frame_mean[fi] * D + c];
            if (SHIFT)
                s_v[idx] = a.vars[(long long)a.frame_cov[fi] * D + c];
        }
        __syncthreads();
        if (active)
            for (int f = 0; f < n; ++f) {
                const double w = s_w[f];
                if (SHIFT) {
                    if (kind == 0)
                        sum += WEIGHTED ? w : 1.0;                                   // :391, :410
                    else if (kind == 1)
                        sum += (WEIGHTED ? w : 1.0) / (double)s_v[f * D + i];        // :393, :412
                    else if (WEIGHTED)
                        sum += w * (double)(s_x[f * D + i] - s_m[f * D + i]) / (double)s_v[f * D + i];   // :414
                    else
                        sum += (double)((s_x[f * D + i] - s_m[f * D + i]) / s_v[f * D + i]);             // :395, f32 arithmetic
                }
                else if (kind == 0)
                    sum += 1.0;                                                      // count_++ (:602, :614, :638, :647)
                else {
                    const double l = kind == 1 ? (double)s_x[f * D + i] : (i == 0 ? 1.0 : (double)s_m[f * D + i - 1]);
                    const double r = j == 0 ? 1.0 : (double)s_m[f * D + j - 1];
                    // :605 / :617, :641 / :650.  l * r is exact; of the weighted sums the -march=native build fuses Z's and leaves G's apart
                    sum = !WEIGHTED ? sum + l * r : kind == 1 ? mad<FMA>(w * l, r, sum) : mad<false>(w * l, r, sum);
                }
            }
        __syncthreads();
    }
    if (active)
        *p = sum;
}

// ---- adapted means: lane = mean, grid y strides over the rows.  slot[mean] = the place of its mixture's matrix, -1 = copy
template<bool SHIFT, bool FMA>
__global__ __launch_bounds__(256) void mllr_adapt_kernel(const float* __restrict__ means, int n_mean, int D, const int* __restrict__ slot,
                                                         const double* __restrict__ mats, float* __restrict__ out) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= n_mean)
        return;
    const float* x = means + m * D;
    const int    s = slot[m], R = D + 1;
    for (int r = blockIdx.y; r < D; r += gridDim.y) {
        float y;
        if (s < 0)
            y = x[r];
        else if (SHIFT)
            y = (float)(mats[(long long)s * D + r] + (double)x[r]);   // Vector<f64> + Vector<f64>(mean), narrowed once (:72)
        else {
            const double* w = mats + ((long long)s * D + r) * R;
            double        v = mad<FMA>(w[0], 1.0, 0.0);               // Matrix * Vector over [1, m] (:162-163)
            for (int k = 1; k < R; ++k)
                v = mad<FMA>(w[k], (double)x[k - 1], v);
            y = (float)v;
        }
        out[m * D + r] = y;
    }
}

}  // namespace amx

struct amx_mllr {
    amx_internal_gmm_view gmm{};
    int                   D = 0, mode = 0, n_keys = 0, n_leafs = 0, device = 0;
    amx_mllr_shape        shape{};
    std::vector<int>      mean_mix;   // mean -> the one mixture that reaches it, -1 = none
    amx::DevBuf<float>    d_vars;     // [n_cov x D]
    amx::DevBuf<int>      d_leaf_of_mix;
    // per-call workspace
    amx::DevBuf<int>                d_frame;   // [4 x frames]: mean, covariance, leaf, list
    amx::DevBuf<int>                d_key;     // key_seg [n_keys + 1], key_base [n_keys]
    amx::DevBuf<amx::MllrSeg>       d_segs;
    amx::DevBuf<int>                d_lists;   // start, count [n_keys x n_leafs] each
    amx::DevBuf<unsigned long long> d_bad;
    amx::DevBuf<double>             d_mats;
    amx::DevBuf<int>                d_slot;
};

extern "C" {

int amx_mllr_create(amx_gmm* gmm, int mode, int n_keys, int n_leafs, const int* leaf_of_mixture, amx_mllr** out) {
    const char* who = "amx_mllr_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(gmm && leaf_of_mixture, AMX_ERR_INVALID, "%s: NULL gmm handle or leaf_of_mixture", who);
    AMX_REQUIRE(mode != AMX_MLLR_BAND, AMX_ERR_UNSUPPORTED, "%s: mode band (mllr-adaptation = band, MODULE_ADAPT_ADVANCED) is not supported: only full and shift are", who);
    AMX_REQUIRE(mode != AMX_MLLR_SEMI_TIED, AMX_ERR_UNSUPPORTED,
                "%s: mode semi-tied (mllr-adaptation = semi-tied, MODULE_ADAPT_ADVANCED) is not supported: only full and shift are", who);
    AMX_REQUIRE(mode == AMX_MLLR_FULL || mode == AMX_MLLR_SHIFT, AMX_ERR_INVALID, "%s: unknown mode %d", who, mode);
    std::unique_ptr<amx_mllr> h(new amx_mllr);
    AMX_TRY(amx_internal_gmm_view_get(gmm, &h->gmm));
    const int D = h->gmm.dim, n_mix = h->gmm.n_mix;
    AMX_REQUIRE(D <= amx::kMllrMaxDim, AMX_ERR_UNSUPPORTED, "%s: dimension %d is larger than %d", who, D, amx::kMllrMaxDim);
    AMX_REQUIRE(n_keys >= 1, AMX_ERR_INVALID, "%s: n_keys %d is not positive", who, n_keys);
    AMX_REQUIRE(n_keys <= amx::kMllrMaxKeys, AMX_ERR_UNSUPPORTED, "%s: n_keys %d is larger than %d", who, n_keys, amx::kMllrMaxKeys);
    AMX_REQUIRE(n_leafs >= 1, AMX_ERR_INVALID, "%s: n_leafs %d is not positive", who, n_leafs);
    AMX_REQUIRE(n_leafs <= amx::kMllrMaxLeafs, AMX_ERR_UNSUPPORTED, "%s: n_leafs %d is larger than %d", who, n_leafs, amx::kMllrMaxLeafs);
    for (int m = 0; m < n_mix; ++m)
        AMX_REQUIRE(leaf_of_mixture[m] >= 0 && leaf_of_mixture[m] < n_leafs, AMX_ERR_INVALID, "%s: mixture %d: leaf %d is outside [0, %d)", who, m,
                    leaf_of_mixture[m], n_leafs);
    AMX_REQUIRE(h->gmm.ctx && h->gmm.h_vars, AMX_ERR_STATE, "%s: host-only gmm handle (created without a context)", who);
    h->D = D, h->mode = mode, h->n_keys = n_keys, h->n_leafs = n_leafs;
    h->shape  = amx_mllr_shape{mode, D, n_leafs, n_keys};
    h->device = h->gmm.ctx->device;
    AMX_HIP(hipSetDevice(h->device));
    // adaptMixtureSet transforms mean(meanIndex) once per (mixture, density) visit (:155-168): a mean reached twice would be transformed twice
    std::vector<uint32_t> mix_off((size_t)n_mix + 1), d_mean((size_t)h->gmm.n_dens);
    AMX_HIP(hipMemcpy(mix_off.data(), h->gmm.d_mix_off, mix_off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    AMX_HIP(hipMemcpy(d_mean.data(), h->gmm.d_d_mean, d_mean.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint32_t> k_dens((size_t)mix_off[(size_t)n_mix]);
    AMX_HIP(hipMemcpy(k_dens.data(), h->gmm.d_k_dens, k_dens.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    h->mean_mix.assign((size_t)h->gmm.n_mean, -1);
    for (int m = 0; m < n_mix; ++m)
        for (uint32_t k = mix_off[(size_t)m]; k < mix_off[(size_t)m + 1]; ++k) {
            const uint32_t mean = d_mean[k_dens[k]];
            AMX_REQUIRE(h->mean_mix[mean] < 0, AMX_ERR_UNSUPPORTED,
                        "%s: shared means: mean %u is reached by more than one (mixture, density) pair (mixtures %d and %d); adaptMixtureSet would "
                        "transform it twice",
                        who, mean, h->mean_mix[mean], m);
            h->mean_mix[mean] = m;
        }
    AMX_TRY(h->d_vars.upload(h->gmm.h_vars, (size_t)h->gmm.n_cov * D));
    AMX_TRY(h->d_leaf_of_mix.upload(leaf_of_mixture, (size_t)n_mix));
    AMX_TRY(h->d_bad.reserve(1));
    *out = h.release();
    return AMX_OK;
}

void amx_mllr_destroy(amx_mllr* h) {
    if (!h)
        return;
    hipSetDevice(h->device);   // the handle's own copy: the buffers are freed without reading the context
    delete h;
}

int amx_mllr_describe(const amx_mllr* h, amx_mllr_shape* shape) {
    AMX_REQUIRE(h && shape, AMX_ERR_INVALID, "amx_mllr_describe: NULL argument");
    *shape = h->shape;
    return AMX_OK;
}

long amx_mllr_accumulator_size(const amx_mllr* h) {
    return h ? amx_mllr_key_size(&h->shape) * h->n_keys : 0;
}

void amx_mllr_kernel_shape(int* stage_frames, int* tile_cells) {
    if (stage_frames)
        *stage_frames = amx::kMllrStage;
    if (tile_cells)
        *tile_cells = amx::kMllrThreads;
}

int amx_mllr_accumulate_dev(amx_mllr* h, const float* feats_dev, int feats_ld, int n_seg, const long* frame_offsets, const int* seg_key,
                            const int32_t* emission_dev, const uint32_t* best_density_dev, int best_density_ld, const double* weight_dev,
                            double* acc_dev) {
    const char* who = "amx_mllr_accumulate_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_seg >= 0 && feats_ld >= h->D, AMX_ERR_INVALID, "%s: n_seg %d, feats_ld %d (dimension %d)", who, n_seg, feats_ld, h->D);
    AMX_REQUIRE(best_density_ld == 0 || best_density_ld >= h->gmm.n_mix, AMX_ERR_INVALID, "%s: best_density_ld %d is neither 0 nor >= %d mixtures", who,
                best_density_ld, h->gmm.n_mix);
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(frame_offsets && seg_key, AMX_ERR_INVALID, "%s: NULL frame_offsets or seg_key", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: frame_offsets[0] = %ld is negative", who, frame_offsets[0]);
    for (int s = 0; s < n_seg; ++s) {
        AMX_REQUIRE(frame_offsets[s + 1] >= frame_offsets[s], AMX_ERR_INVALID, "%s: frame_offsets decrease at segment %d (%ld after %ld)", who, s,
                    frame_offsets[s + 1], frame_offsets[s]);
        AMX_REQUIRE(seg_key[s] >= 0 && seg_key[s] < h->n_keys, AMX_ERR_INVALID, "%s: segment %d: key %d is outside [0, %d)", who, s, seg_key[s], h->n_keys);
    }
    const long long t0 = frame_offsets[0], n = frame_offsets[n_seg] - t0;
    if (n == 0)
        return AMX_OK;
    AMX_REQUIRE(n < (1ll << 30), AMX_ERR_INVALID, "%s: %lld frames are more than one call takes", who, n);
    AMX_REQUIRE(feats_dev && emission_dev && best_density_dev && acc_dev, AMX_ERR_INVALID, "%s: NULL feats_dev, emission_dev, best_density_dev or acc_dev", who);
    amx_ctx* ctx = h->gmm.ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // every key's segments in ascending order (a counting sort by key keeps it) and the key's place in the list: the frames of the
    // keys before it
    const int                 n_keys = h->n_keys, n_leafs = h->n_leafs;
    std::vector<int>          key_tab((size_t)2 * n_keys + 1, 0);   // key_seg [n_keys + 1] | key_base [n_keys]
    std::vector<amx::MllrSeg> segs;
    int*                      key_seg  = key_tab.data();
    int*                      key_base = key_tab.data() + n_keys + 1;
    std::vector<long long>    key_frames((size_t)n_keys, 0);
    for (int s = 0; s < n_seg; ++s)
        if (frame_offsets[s + 1] > frame_offsets[s]) {
            ++key_seg[seg_key[s] + 1];
            key_frames[(size_t)seg_key[s]] += frame_offsets[s + 1] - frame_offsets[s];
        }
    long long run = 0;
    for (int k = 0; k < n_keys; ++k) {
        key_seg[k + 1] += key_seg[k];
        key_base[k] = (int)run;
        run += key_frames[(size_t)k];
    }
    segs.resize((size_t)key_seg[n_keys]);
    {
        std::vector<int> cursor(key_seg, key_seg + n_keys);
        for (int s = 0; s < n_seg; ++s)
            if (frame_offsets[s + 1] > frame_offsets[s])
                segs[(size_t)cursor[(size_t)seg_key[s]]++] = amx::MllrSeg{frame_offsets[s], frame_offsets[s + 1]};
    }
    const long long n_pairs = (long long)n_keys * n_leafs;
    AMX_TRY(h->d_frame.reserve((size_t)4 * n));
    AMX_TRY(h->d_key.reserve(key_tab.size()));
    AMX_TRY(h->d_segs.reserve(segs.size()));
    AMX_TRY(h->d_lists.reserve((size_t)2 * n_pairs));
    int* frame_mean = h->d_frame.get();
    int* frame_cov  = frame_mean + n;
    int* frame_leaf = frame_cov + n;
    int* list       = frame_leaf + n;
    int* list_start = h->d_lists.get();
    int* list_count = list_start + n_pairs;
    AMX_HIP(hipMemcpyAsync(h->d_key.get(), key_tab.data(), key_tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(h->d_segs.get(), segs.data(), segs.size() * sizeof(amx::MllrSeg), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemsetAsync(h->d_bad.get(), 0xff, sizeof(unsigned long long), st));

    // 1. indices and checks, before anything is written
    {
        amx::ScopedKernelTimer timer(ctx, "mllr_resolve");
        hipLaunchKernelGGL(amx::mllr_resolve_kernel, dim3((unsigned)amx::ceil_div(n, amx::kMllrThreads)), dim3(amx::kMllrThreads), 0, st, feats_dev,
                           (long long)feats_ld, h->D, t0, n, emission_dev, best_density_dev, best_density_ld, weight_dev, h->gmm.n_mix, h->gmm.d_mix_off,
                           h->gmm.d_k_dens, h->gmm.d_d_mean, h->gmm.d_d_cov, (const int*)h->d_leaf_of_mix.get(), frame_mean, frame_cov, frame_leaf,
                           h->d_bad.get());
        AMX_HIP(hipGetLastError());
    }
    unsigned long long bad = 0;
    AMX_HIP(hipMemcpyAsync(&bad, h->d_bad.get(), sizeof(bad), hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    if (bad != ~0ull) {
        const long long t    = t0 + (long long)(bad >> 3);
        const int       kind = (int)(bad & 7);
        int32_t         e    = 0;
        AMX_HIP(hipMemcpy(&e, emission_dev + t, sizeof(e), hipMemcpyDeviceToHost));
        if (kind == 1)
            amx::set_error("%s: frame %lld: emission index %d is outside [0, %d) and is not -1", who, t, e, h->gmm.n_mix);
        else if (kind == 2)
            amx::set_error("%s: frame %lld: the density of emission %d is outside its mixture", who, t, e);
        else
            amx::set_error("%s: frame %lld: non-finite %s", who, t, kind == 3 ? "feature" : "weight");
        return AMX_ERR_INVALID;
    }

    // 2. the lists
    {
        amx::ScopedKernelTimer timer(ctx, "mllr_lists");
        hipLaunchKernelGGL(amx::mllr_lists_kernel, dim3((unsigned)n_keys), dim3(amx::kMllrThreads), (size_t)n_leafs * sizeof(int), st,
                           (const int*)h->d_key.get(), (const amx::MllrSeg*)h->d_segs.get(), t0, (const int*)frame_leaf, n_leafs,
                           (const int*)(h->d_key.get() + n_keys + 1), list, list_start, list_count);
        AMX_HIP(hipGetLastError());
    }

    // 3. the chains
    amx::MllrArgs a{};
    a.feats = feats_dev, a.ld = feats_ld, a.D = h->D, a.n_leafs = n_leafs, a.t_base = t0, a.frame_mean = frame_mean, a.frame_cov = frame_cov;
    a.weight = weight_dev, a.means = h->gmm.d_means, a.vars = h->d_vars.get(), a.list = list, a.list_start = list_start, a.list_count = list_count;
    a.acc = acc_dev, a.leaf_size = amx_mllr_leaf_size(&h->shape);
    const bool   shift = h->mode == AMX_MLLR_SHIFT, fma = ctx->contract == AMX_CONTRACT_FMA, wt = weight_dev != nullptr;
    const size_t lds   = (size_t)amx::kMllrStage * h->D * sizeof(float) * (shift ? 3 : 2);
    {
        amx::ScopedKernelTimer timer(ctx, shift ? "mllr_acc_shift" : "mllr_acc_full");
        const dim3             grid((unsigned)n_pairs, (unsigned)amx::ceil_div(a.leaf_size, amx::kMllrThreads));
        auto                   kern = fma ? (wt ? amx::mllr_acc_kernel<false, true, true> : amx::mllr_acc_kernel<false, true, false>)
                                          : (wt ? amx::mllr_acc_kernel<false, false, true> : amx::mllr_acc_kernel<false, false, false>);
        if (shift)   // no contraction site in the shift estimator
            kern = wt ? amx::mllr_acc_kernel<true, false, true> : amx::mllr_acc_kernel<true, false, false>;
        hipLaunchKernelGGL(kern, grid, dim3(amx::kMllrThreads), lds, st, a);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(st));   // the workspace is the handle's, the segment lists are this call's
    return AMX_OK;
}

int amx_mllr_adapt_means_dev(amx_mllr* h, int n_matrices, const int* matrix_ids, const double* matrices, const int* matrix_of_mixture,
                             float* out_dev) {
    const char* who = "amx_mllr_adapt_means_dev";
    AMX_REQUIRE(h && matrix_ids && matrices && matrix_of_mixture && out_dev, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(n_matrices >= 1, AMX_ERR_INVALID, "%s: n_matrices %d is not positive", who, n_matrices);
    const int        D = h->D, n_mean = h->gmm.n_mean;
    const bool       shift = h->mode == AMX_MLLR_SHIFT;
    const size_t     per   = shift ? (size_t)D : (size_t)D * (D + 1);
    std::vector<int> slot((size_t)n_mean, -1), mix_slot((size_t)h->gmm.n_mix, -1);
    for (int m = 0; m < h->gmm.n_mix; ++m) {
        for (int s = 0; s < n_matrices; ++s)
            if (matrix_ids[s] == matrix_of_mixture[m]) {
                mix_slot[(size_t)m] = s;
                break;
            }
        AMX_REQUIRE(mix_slot[(size_t)m] >= 0, AMX_ERR_INVALID, "%s: mixture %d: matrix id %d is not among the %d matrices", who, m, matrix_of_mixture[m],
                    n_matrices);
    }
    for (int i = 0; i < n_mean; ++i)
        if (h->mean_mix[(size_t)i] >= 0)
            slot[(size_t)i] = mix_slot[(size_t)h->mean_mix[(size_t)i]];
    for (size_t e = 0; e < per * n_matrices; ++e)
        AMX_REQUIRE(std::isfinite(matrices[e]), AMX_ERR_INVALID, "%s: element %zu of the matrices is not finite", who, e);
    amx_ctx* ctx = h->gmm.ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    AMX_TRY(h->d_mats.reserve(per * n_matrices));
    AMX_TRY(h->d_slot.reserve((size_t)n_mean));
    AMX_HIP(hipMemcpyAsync(h->d_mats.get(), matrices, per * n_matrices * sizeof(double), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(h->d_slot.get(), slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice, st));
    {
        amx::ScopedKernelTimer timer(ctx, "mllr_adapt");
        const bool             fma = ctx->contract == AMX_CONTRACT_FMA;
        const dim3             grid((unsigned)amx::ceil_div(n_mean, 256), (unsigned)std::min(D, 64));
        auto                   kern = shift ? amx::mllr_adapt_kernel<true, false> : (fma ? amx::mllr_adapt_kernel<false, true> : amx::mllr_adapt_kernel<false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, h->gmm.d_means, n_mean, D, (const int*)h->d_slot.get(), (const double*)h->d_mats.get(), out_dev);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(st));   // the tables are this call's
    return AMX_OK;
}

}  // extern "C"
