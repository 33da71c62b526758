// cmllr.hip -- constrained MLLR on the device (include/amx.h, section "constrained MLLR"): the corpus pass of
// Mm::AffineFeatureTransformAccumulator::accumulate (Mm/AffineFeatureTransformAccumulator.cc:40-121) per key, and the application of the
// estimated transforms with the key chosen per segment.  Files, combine, estimate and score are cmllr_host.cpp's.
//
// Order.  Per (key, cell) the reference adds the key's frames in corpus order into an f64.  A segment belongs to one key, so the host
// lists every key's segments in ascending order and a workgroup walks that list frame by frame: the chain of a cell is one lane's
// register, starts from what the buffer holds and is written back once.  No floating-point atomic, no partial sums: the bits do not
// depend on the launch shape, and a corpus cut into calls anywhere gives the bits of one call.
//
// Kernels.  cmllr_g_kernel is the hot one (M x upper triangle of order F + 1 cells per key, one f64 division each per frame): a lane
// owns one (j, k) pair of the triangle and kCmllrTileM model components, forms p = xi_j * xi_k once per frame and divides it by the
// frame's variances, staged in LDS beside xi.  Triangles longer than a workgroup and models wider than a tile span several workgroups
// of one key (grid x and z).  cmllr_small_kernel carries beta, k, mean and cov (one cell per lane); it is bound by the latency of its
// chains and is not tuned.  A frame's (mean, covariance) indices are resolved and checked once, before anything is written.
// The library is compiled with -ffp-contract=off; mad<FMA> marks the sites the reference's -march=native build contracts
// (tests/golden/ref_cmllr.npz holds both builds).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "gmm_internal.hpp"

namespace amx {

constexpr int kCmllrThreads = 256;
constexpr int kCmllrStage   = 32;    // frames staged in LDS at a time
constexpr int kCmllrTileM   = 16;    // model components per workgroup of cmllr_g_kernel: 16 f64 accumulators per lane (the default)
constexpr int kCmllrTileWide = 48;   // the A/B shape: a lane keeps (nearly) all of a 45-dimensional model's accumulators
constexpr int kCmllrMaxDim  = 255;   // F + 1 <= 256: a stage of xi is at most 32 KB of LDS
constexpr int kCmllrMaxKeys = 65535; // a key is one row (y) of the two kernels' grids

struct CmllrSeg {
    long long begin, end;   // frames [begin, end) of one segment
};

struct CmllrArgs {
    const float*    feats;
    long long       ld;
    int             F, M;
    long long       t_base;       // frame of frame_mean[0]
    const int*      frame_mean;   // per frame: mean index, -1 = skip the frame
    const int*      frame_cov;    //            covariance index
    const double*   weight;
    const float*    means;        // [n_mean x M]
    const float*    vars;         // [n_cov x M]
    const int*      key_seg;      // [n_keys + 1] into segs
    const CmllrSeg* segs;
    double*         acc;
    long long       key_stride, off_mean, off_cov, off_g, tri;
};

// cell of the row-major upper triangle of an R x R matrix -> (j, k), j <= k
__device__ inline void cmllr_tri_decode(long long cell, int R, int* j, int* k) {
    int row = 0;
    while (cell >= R - row) {
        cell -= R - row;
        ++row;
    }
    *j = row;
    *k = row + (int)cell;
}

// ---- every frame's (mean, covariance) and the checks, before anything is written.  bad = min over the offending frames of
// (frame << 3 | kind): 1 emission outside the model, 2 density outside the mixture, 3 non-finite feature, 4 non-finite weight
__global__ __launch_bounds__(kCmllrThreads) void cmllr_resolve_kernel(const float* __restrict__ feats, long long ld, int F, long long t0, long long n,
                                                                      const int32_t* __restrict__ emission, const uint32_t* __restrict__ best, int best_ld,
                                                                      const double* __restrict__ weight, int n_mix, const uint32_t* __restrict__ mix_off,
                                                                      const uint32_t* __restrict__ k_dens, const uint32_t* __restrict__ d_mean,
                                                                      const uint32_t* __restrict__ d_cov, int* __restrict__ frame_mean,
                                                                      int* __restrict__ frame_cov, unsigned long long* bad) {
    const long long i = (long long)blockIdx.x * kCmllrThreads + threadIdx.x;
    if (i >= n)
        return;
    const long long t = t0 + i;
    const int32_t   e = emission[t];
    int             mi = -1, ci = -1, kind = 0;
    if (e != -1) {
        if (e < 0 || e >= n_mix)
            kind = 1;
        else {
            const uint32_t kk = best_ld > 0 ? best[t * best_ld + e] : best[t];
            if (kk >= mix_off[e + 1] - mix_off[e])
                kind = 2;
            else {
                const uint32_t d = k_dens[mix_off[e] + kk];
                mi = (int)d_mean[d], ci = (int)d_cov[d];
                for (int c = 0; c < F; ++c)
                    if (!isfinite(feats[t * ld + c]))
                        kind = 3;
                if (weight && !isfinite(weight[t]))
                    kind = kind ? kind : 4;
            }
        }
    }
    frame_mean[i] = kind ? -1 : mi;
    frame_cov[i]  = kind ? -1 : ci;
    if (kind)
        atomicMin(bad, ((unsigned long long)i << 3) | (unsigned long long)kind);
}

// xi = [1, x] of frames [t, t + n) into s_x [n][R]; their flags, weights and indices into the s_* of the caller (all lanes call)
__device__ inline void cmllr_stage(const CmllrArgs& a, long long t, int n, float* s_x, int* s_mi, int* s_ci, double* s_w) {
    const int R = a.F + 1, tid = threadIdx.x;
    if (tid < n) {
        const long long i = t + tid - a.t_base;
        s_mi[tid] = a.frame_mean[i];
        s_ci[tid] = a.frame_cov[i];
        s_w[tid]  = a.weight ? a.weight[t + tid] : 1.0;
    }
    for (int idx = tid; idx < n * R; idx += kCmllrThreads) {
        const int f = idx / R, c = idx - f * R;
        s_x[idx]    = c == 0 ? 1.f : a.feats[(t + f) * a.ld + (c - 1)];
    }
}

// ---- G[i][j][k] += xi_j * xi_k / v_i [* w] (:70, :111).  grid: x = 256 cells of the triangle, y = key, z = tile of model components
template<int TM, bool FMA, bool WEIGHTED>
__global__ __launch_bounds__(kCmllrThreads) void cmllr_g_kernel(CmllrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_v[kCmllrStage][TM];
    __shared__ double s_w[kCmllrStage];
    __shared__ int    s_mi[kCmllrStage], s_ci[kCmllrStage];
    float*            s_x = reinterpret_cast<float*>(s_raw);   // [stage][R]

    const int key = blockIdx.y, i0 = blockIdx.z * TM, tid = threadIdx.x, R = a.F + 1;
    const int s_begin = a.key_seg[key], s_end = a.key_seg[key + 1];
    if (s_begin == s_end)
        return;
    const long long cell   = (long long)blockIdx.x * kCmllrThreads + tid;
    const bool      active = cell < a.tri;
    int             j = 0, k = 0;
    if (active)
        cmllr_tri_decode(cell, R, &j, &k);
    double* g = a.acc + (long long)key * a.key_stride + a.off_g + (long long)i0 * a.tri + cell;
    double  sum[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
        sum[i] = active && i0 + i < a.M ? g[(long long)i * a.tri] : 0.0;

    for (int s = s_begin; s < s_end; ++s) {
        const CmllrSeg seg = a.segs[s];
        for (long long t = seg.begin; t < seg.end; t += kCmllrStage) {
            const int n = seg.end - t < kCmllrStage ? (int)(seg.end - t) : kCmllrStage;
            cmllr_stage(a, t, n, s_x, s_mi, s_ci, s_w);
            for (int idx = tid; idx < n * TM; idx += kCmllrThreads) {
                const int f = idx / TM, i = idx - f * TM;
                const int ci = a.frame_cov[t + f - a.t_base];
                s_v[f][i]    = ci >= 0 && i0 + i < a.M ? (double)a.vars[(long long)ci * a.M + i0 + i] : 1.0;
            }
            __syncthreads();
            if (active)
                for (int f = 0; f < n; ++f) {
                    if (s_mi[f] < 0)
                        continue;
                    const double p = (double)s_x[f * R + j] * (double)s_x[f * R + k];
                    const double w = s_w[f];
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const double q = p / s_v[f][i];
                        sum[i]         = WEIGHTED ? mad<FMA>(q, w, sum[i]) : sum[i] + q;
                    }
                }
            __syncthreads();
        }
    }
    if (active)
#pragma unroll
        for (int i = 0; i < TM; ++i)
            if (i0 + i < a.M)
                g[(long long)i * a.tri] = sum[i];
}

// ---- beta, k, mean, cov: one cell per lane, cells in the order of the flat buffer [beta | k: M x R | mean: R | cov: tri]
template<bool FMA, bool WEIGHTED>
__global__ __launch_bounds__(kCmllrThreads) void cmllr_small_kernel(CmllrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_w[kCmllrStage];
    __shared__ int    s_mi[kCmllrStage], s_ci[kCmllrStage];
    float*            s_x = reinterpret_cast<float*>(s_raw);

    const int key = blockIdx.y, tid = threadIdx.x, R = a.F + 1;
    const int s_begin = a.key_seg[key], s_end = a.key_seg[key + 1];
    if (s_begin == s_end)
        return;
    const long long cell   = (long long)blockIdx.x * kCmllrThreads + tid;
    const bool      active = cell < a.off_g;
    int             kind = 0, i = 0, j = 0, k = 0;   // 0 beta, 1 k[i][j], 2 mean[j], 3 cov[j][k]
    if (active && cell >= a.off_cov) {
        kind = 3;
        cmllr_tri_decode(cell - a.off_cov, R, &j, &k);
    }
    else if (active && cell >= a.off_mean)
        kind = 2, j = (int)(cell - a.off_mean);
    else if (active && cell >= 1)
        kind = 1, i = (int)((cell - 1) / R), j = (int)((cell - 1) - (long long)i * R);
    double* p   = a.acc + (long long)key * a.key_stride + cell;
    double  sum = active ? *p : 0.0;

    for (int s = s_begin; s < s_end; ++s) {
        const CmllrSeg seg = a.segs[s];
        for (long long t = seg.begin; t < seg.end; t += kCmllrStage) {
            const int n = seg.end - t < kCmllrStage ? (int)(seg.end - t) : kCmllrStage;
            cmllr_stage(a, t, n, s_x, s_mi, s_ci, s_w);
            __syncthreads();
            if (active)
                for (int f = 0; f < n; ++f) {
                    if (s_mi[f] < 0)
                        continue;
                    const double w  = s_w[f];
                    const double xj = (double)s_x[f * R + j];
                    if (kind == 0)
                        sum += WEIGHTED ? w : 1.0;                                           // beta_ += 1 | weight (:44, :86)
                    else if (kind == 1) {
                        const double r = (double)a.means[(long long)s_mi[f] * a.M + i] / (double)a.vars[(long long)s_ci[f] * a.M + i];
                        sum            = WEIGHTED ? mad<FMA>(r * xj, w, sum) : mad<FMA>(r, xj, sum);   // :63 / :68, :104 / :109
                    }
                    else if (kind == 2)
                        sum = WEIGHTED ? mad<FMA>(xj, w, sum) : sum + xj;                    // :76, :117
                    else {
                        const double xk = (double)s_x[f * R + k];
                        sum             = WEIGHTED ? mad<FMA>(xj * xk, w, sum) : mad<FMA>(xj, xk, sum);   // :78, :119
                    }
                }
            __syncthreads();
        }
    }
    if (active)
        *p = sum;
}

// ---- apply: y[t][r] = A_key[r][0] * 1 + sum_k A_key[r][k] x[t][k - 1], amx_matrix_multiply_dev's chain on [1, x].  lane = frame.
template<bool FMA>
__global__ __launch_bounds__(256) void cmllr_apply_kernel(const float* __restrict__ A, const int* __restrict__ has, int M, int F,
                                                          const float* __restrict__ in, long long in_ld, const long long* __restrict__ off,
                                                          const int* __restrict__ seg_key, int n_seg, float* __restrict__ out, long long out_ld) {
    const long long t0 = off[0], n = off[n_seg] - t0;
    const long long i  = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const long long t = t0 + i;
    int lo = 0, hi = n_seg;   // the segment with off[s] <= t < off[s + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (off[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    const int    key = seg_key[lo];
    const float* x   = in + t * in_ld;
    const int    R   = F + 1;
    for (int r = blockIdx.y; r < M; r += gridDim.y) {
        float y;
        if (!has[key])
            y = x[r];
        else {
            const float* m = A + ((long long)key * M + r) * R;
            y              = mad<FMA>(m[0], 1.0f, 0.f);
            for (int k = 1; k < R; ++k)
                y = mad<FMA>(m[k], x[k - 1], y);
        }
        out[t * out_ld + r] = y;
    }
}

}  // namespace amx

struct amx_cmllr {
    amx_internal_gmm_view gmm{};
    int                   F = 0, M = 0, n_keys = 0, device = 0, tile = amx::kCmllrTileM;
    bool                  pooled = false;
    amx_cmllr_shape       shape{};
    std::vector<float>    h_var0;   // the pooled model's variance vector
    amx::DevBuf<float>    d_vars;   // [n_cov x M]
    // per-call workspace
    amx::DevBuf<int>                d_frame;   // [2 x frames]: mean index, covariance index
    amx::DevBuf<int>                d_key_seg;
    amx::DevBuf<amx::CmllrSeg>      d_segs;
    amx::DevBuf<unsigned long long> d_bad;
};

extern "C" {

int amx_cmllr_create(amx_gmm* gmm, int feature_dim, int n_keys, amx_cmllr** out) {
    const char* who = "amx_cmllr_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(gmm, AMX_ERR_INVALID, "%s: NULL gmm handle", who);
    std::unique_ptr<amx_cmllr> h(new amx_cmllr);
    AMX_TRY(amx_internal_gmm_view_get(gmm, &h->gmm));
    const int M = h->gmm.dim;
    AMX_REQUIRE(feature_dim >= M, AMX_ERR_INVALID, "%s: feature_dim %d is smaller than the model's dimension %d", who, feature_dim, M);
    AMX_REQUIRE(feature_dim <= amx::kCmllrMaxDim, AMX_ERR_UNSUPPORTED, "%s: feature_dim %d is larger than %d", who, feature_dim, amx::kCmllrMaxDim);
    AMX_REQUIRE(n_keys >= 1, AMX_ERR_INVALID, "%s: n_keys %d is not positive", who, n_keys);
    AMX_REQUIRE(n_keys <= amx::kCmllrMaxKeys, AMX_ERR_UNSUPPORTED, "%s: n_keys %d is larger than %d", who, n_keys, amx::kCmllrMaxKeys);
    AMX_REQUIRE(h->gmm.ctx && h->gmm.h_vars, AMX_ERR_STATE, "%s: host-only gmm handle (created without a context)", who);
    h->F = feature_dim, h->M = M, h->n_keys = n_keys, h->pooled = h->gmm.n_cov == 1;
    h->shape = amx_cmllr_shape{feature_dim, M, n_keys, h->pooled ? 1 : 0};
    if (h->pooled)
        h->h_var0.assign(h->gmm.h_vars, h->gmm.h_vars + M);
    h->device = h->gmm.ctx->device;
    AMX_HIP(hipSetDevice(h->device));
    AMX_TRY(h->d_vars.upload(h->gmm.h_vars, (size_t)h->gmm.n_cov * M));
    AMX_TRY(h->d_bad.reserve(1));
    *out = h.release();
    return AMX_OK;
}

void amx_cmllr_destroy(amx_cmllr* h) {
    if (!h)
        return;
    hipSetDevice(h->device);   // the handle's own copy: the buffers are freed without reading the context
    delete h;
}

int amx_cmllr_describe(const amx_cmllr* h, amx_cmllr_shape* shape, float* pooled_variance) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_cmllr_describe: NULL handle");
    if (shape)
        *shape = h->shape;
    if (pooled_variance && h->pooled)
        std::copy(h->h_var0.begin(), h->h_var0.end(), pooled_variance);
    return AMX_OK;
}

long amx_cmllr_accumulator_size(const amx_cmllr* h) {
    return h ? amx_cmllr_key_size(&h->shape) * h->n_keys : 0;
}

int amx_cmllr_set_tile(amx_cmllr* h, int tile_components) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_cmllr_set_tile: NULL handle");
    AMX_REQUIRE(tile_components == amx::kCmllrTileM || tile_components == amx::kCmllrTileWide, AMX_ERR_INVALID,
                "amx_cmllr_set_tile: %d model components per workgroup; the kernel has instances for %d and %d", tile_components, amx::kCmllrTileM,
                amx::kCmllrTileWide);
    h->tile = tile_components;
    return AMX_OK;
}

void amx_cmllr_kernel_shape(int* stage_frames, int* tile_cells, int* tile_components) {
    if (stage_frames)
        *stage_frames = amx::kCmllrStage;
    if (tile_cells)
        *tile_cells = amx::kCmllrThreads;
    if (tile_components)
        *tile_components = amx::kCmllrTileM;
}

int amx_cmllr_accumulate_dev(amx_cmllr* h, const float* feats_dev, int feats_ld, int n_seg, const long* frame_offsets, const int* seg_key,
                             const int32_t* emission_dev, const uint32_t* best_density_dev, int best_density_ld, const double* weight_dev,
                             double* acc_dev) {
    const char* who = "amx_cmllr_accumulate_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_seg >= 0 && feats_ld >= h->F, AMX_ERR_INVALID, "%s: n_seg %d, feats_ld %d (feature_dim %d)", who, n_seg, feats_ld, h->F);
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

    // every key's segments in ascending order (a counting sort by key keeps it)
    std::vector<int>           key_seg((size_t)h->n_keys + 1, 0);
    std::vector<amx::CmllrSeg> segs;
    for (int s = 0; s < n_seg; ++s)
        if (frame_offsets[s + 1] > frame_offsets[s])
            ++key_seg[(size_t)seg_key[s] + 1];
    for (int k = 0; k < h->n_keys; ++k)
        key_seg[(size_t)k + 1] += key_seg[(size_t)k];
    segs.resize((size_t)key_seg[(size_t)h->n_keys]);
    {
        std::vector<int> cursor(key_seg.begin(), key_seg.end() - 1);
        for (int s = 0; s < n_seg; ++s)
            if (frame_offsets[s + 1] > frame_offsets[s])
                segs[(size_t)cursor[(size_t)seg_key[s]]++] = amx::CmllrSeg{frame_offsets[s], frame_offsets[s + 1]};
    }
    AMX_TRY(h->d_frame.reserve((size_t)2 * n));
    AMX_TRY(h->d_key_seg.reserve(key_seg.size()));
    AMX_TRY(h->d_segs.reserve(segs.size()));
    int* frame_mean = h->d_frame.get();
    int* frame_cov  = frame_mean + n;
    AMX_HIP(hipMemcpyAsync(h->d_key_seg.get(), key_seg.data(), key_seg.size() * sizeof(int), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(h->d_segs.get(), segs.data(), segs.size() * sizeof(amx::CmllrSeg), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemsetAsync(h->d_bad.get(), 0xff, sizeof(unsigned long long), st));

    // 1. indices and checks, before anything is written
    hipLaunchKernelGGL(amx::cmllr_resolve_kernel, dim3((unsigned)amx::ceil_div(n, amx::kCmllrThreads)), dim3(amx::kCmllrThreads), 0, st, feats_dev,
                       (long long)feats_ld, h->F, t0, n, emission_dev, best_density_dev, best_density_ld, weight_dev, h->gmm.n_mix, h->gmm.d_mix_off,
                       h->gmm.d_k_dens, h->gmm.d_d_mean, h->gmm.d_d_cov, frame_mean, frame_cov, h->d_bad.get());
    AMX_HIP(hipGetLastError());
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

    // 2. the chains
    amx::CmllrArgs a{};
    a.feats = feats_dev, a.ld = feats_ld, a.F = h->F, a.M = h->M, a.t_base = t0, a.frame_mean = frame_mean, a.frame_cov = frame_cov;
    a.weight = weight_dev, a.means = h->gmm.d_means, a.vars = h->d_vars.get(), a.key_seg = h->d_key_seg.get(), a.segs = h->d_segs.get();
    a.acc = acc_dev;
    const int R  = h->F + 1;
    a.tri        = (long long)R * (R + 1) / 2;
    a.off_mean   = 1 + (long long)h->M * R;
    a.off_cov    = a.off_mean + R;
    a.off_g      = a.off_cov + a.tri;
    a.key_stride = amx_cmllr_key_size(&h->shape);
    const size_t lds  = (size_t)amx::kCmllrStage * R * sizeof(float);
    const bool   fma = ctx->contract == AMX_CONTRACT_FMA, wt = weight_dev != nullptr;
    {
        amx::ScopedKernelTimer timer(ctx, "cmllr_small");
        const dim3             grid((unsigned)amx::ceil_div(a.off_g, amx::kCmllrThreads), (unsigned)h->n_keys);
        auto                   kern = fma ? (wt ? amx::cmllr_small_kernel<true, true> : amx::cmllr_small_kernel<true, false>)
                                          : (wt ? amx::cmllr_small_kernel<false, true> : amx::cmllr_small_kernel<false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(amx::kCmllrThreads), lds, st, a);
        AMX_HIP(hipGetLastError());
    }
    if (!h->pooled) {
        amx::ScopedKernelTimer timer(ctx, "cmllr_g");
        const dim3             grid((unsigned)amx::ceil_div(a.tri, amx::kCmllrThreads), (unsigned)h->n_keys, (unsigned)amx::ceil_div(h->M, h->tile));
        constexpr int          TN = amx::kCmllrTileM, TW = amx::kCmllrTileWide;
        auto                   kern = fma ? (wt ? amx::cmllr_g_kernel<TN, true, true> : amx::cmllr_g_kernel<TN, true, false>)
                                          : (wt ? amx::cmllr_g_kernel<TN, false, true> : amx::cmllr_g_kernel<TN, false, false>);
        if (h->tile == TW)
            kern = fma ? (wt ? amx::cmllr_g_kernel<TW, true, true> : amx::cmllr_g_kernel<TW, true, false>)
                       : (wt ? amx::cmllr_g_kernel<TW, false, true> : amx::cmllr_g_kernel<TW, false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(amx::kCmllrThreads), lds, st, a);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(st));   // the workspace is the handle's, the segment lists are this call's
    return AMX_OK;
}

int amx_cmllr_apply_dev(amx_ctx* ctx, const float* transforms_dev, const int* has_transform, int n_keys, int model_dim, int feature_dim,
                        const float* in_dev, int in_ld, int n_seg, const long* frame_offsets, const int* seg_key, float* out_dev, int out_ld,
                        int* n_identity_segments) {
    const char* who = "amx_cmllr_apply_dev";
    AMX_REQUIRE(ctx && has_transform, AMX_ERR_INVALID, "%s: NULL context or has_transform", who);
    AMX_REQUIRE(n_keys >= 1 && model_dim >= 1 && feature_dim >= model_dim && in_ld >= feature_dim && out_ld >= model_dim && n_seg >= 0,
                AMX_ERR_INVALID, "%s: bad shape (n_keys %d, model_dim %d, feature_dim %d, in_ld %d, out_ld %d, n_seg %d)", who, n_keys, model_dim,
                feature_dim, in_ld, out_ld, n_seg);
    if (n_identity_segments)
        *n_identity_segments = 0;
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(frame_offsets && seg_key, AMX_ERR_INVALID, "%s: NULL frame_offsets or seg_key", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: frame_offsets[0] = %ld is negative", who, frame_offsets[0]);
    int  n_identity = 0;
    bool any        = false;
    for (int s = 0; s < n_seg; ++s) {
        AMX_REQUIRE(frame_offsets[s + 1] >= frame_offsets[s], AMX_ERR_INVALID, "%s: frame_offsets decrease at segment %d (%ld after %ld)", who, s,
                    frame_offsets[s + 1], frame_offsets[s]);
        AMX_REQUIRE(seg_key[s] >= 0 && seg_key[s] < n_keys, AMX_ERR_INVALID, "%s: segment %d: key %d is outside [0, %d)", who, s, seg_key[s], n_keys);
        if (!has_transform[seg_key[s]])
            ++n_identity;
        else
            any = true;
    }
    if (n_identity_segments)
        *n_identity_segments = n_identity;
    const long long t0 = frame_offsets[0], n = frame_offsets[n_seg] - t0;
    if (n == 0)
        return AMX_OK;
    AMX_REQUIRE(n < (1ll << 38), AMX_ERR_INVALID, "%s: %lld frames are more than one call takes", who, n);
    AMX_REQUIRE(in_dev && out_dev && (transforms_dev || !any), AMX_ERR_INVALID, "%s: NULL in_dev, out_dev or transforms_dev", who);
    AMX_REQUIRE(!amx::views_alias(in_dev + t0 * in_ld, in_ld, feature_dim, out_dev + t0 * out_ld, out_ld, model_dim, n), AMX_ERR_INVALID,
                "%s: input and output views overlap", who);
    AMX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // workspace: offsets [n_seg + 1] (64-bit), keys [n_seg], flags [n_keys]
    std::vector<long long> off(frame_offsets, frame_offsets + n_seg + 1);
    const size_t           bytes = off.size() * sizeof(long long) + ((size_t)n_seg + n_keys) * sizeof(int);
    AMX_TRY(ctx->scratch.reserve(bytes));
    long long* d_off = (long long*)ctx->scratch.get();
    int*       d_key = (int*)(d_off + n_seg + 1);
    int*       d_has = d_key + n_seg;
    AMX_HIP(hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(d_key, seg_key, (size_t)n_seg * sizeof(int), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(d_has, has_transform, (size_t)n_keys * sizeof(int), hipMemcpyHostToDevice, st));
    {
        amx::ScopedKernelTimer timer(ctx, "cmllr_apply");
        const dim3             grid((unsigned)((n + 255) / 256), (unsigned)std::min(model_dim, 64));
        hipLaunchKernelGGL(ctx->contract == AMX_CONTRACT_FMA ? amx::cmllr_apply_kernel<true> : amx::cmllr_apply_kernel<false>, grid, dim3(256), 0, st,
                           transforms_dev, (const int*)d_has, model_dim, feature_dim, in_dev, (long long)in_ld, (const long long*)d_off, (const int*)d_key,
                           n_seg, out_dev, (long long)out_ld);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(st));   // the workspace is the context's, the tables are this call's
    return AMX_OK;
}

}  // extern "C"
