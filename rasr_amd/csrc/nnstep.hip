// nnstep.hip -- NN mini-batch training on the amx_nntrain handle: Nn::FeedForwardTrainer with batch-mode = false (the regulariser on
// the objective and on the gradient, Statistics::finalize, the estimator's step, accumulate-multiple-batches) and Nn::BatchEstimator.
// include/amx.h ("NN mini-batch training") states the arithmetic with the reference's file:line.  The statistics pass itself is
// nntrain.hip's (amx::nntrain_pass), which adds a call's gradient into the group's f32 statistic with the regulariser's axpy behind
// it (nntrain_reduce_step_kernel); this file holds the configuration, the group's bookkeeping and the update.
//
// Kernels and their bounds ("NN mini-batch training"):
//   nnstep_update_kernel   one pass per layer over G [Pin x Pout] and W^T [Pin x Pout]: finalize scale, the outer product with the
//                          feeding layer's activation mean, weight axpy, L1 clip; writes G, W^T and, through an LDS tile transpose,
//                          W [Pout x Pin]; the tile's sum of |G| and its part of G^T m.  HBM bound, 20 bytes per parameter
//   nnstep_bias_kernel     the same for the bias, after the layer's update kernel: it adds the tile parts of G^T m first
//   nnstep_actstat_kernel  a layer's activation statistics over the frames of a call, one thread per unit
//   nnstep_norm_kernel     the regulariser's norms, segment sums in f64;  nnstep_sum_kernel adds segment / tile sums in a fixed order
//   nnstep_book_kernel, nnstep_finalize_kernel, nnstep_stepsize_kernel   one thread / one workgroup: the group's counters and f32 chains
#include "nntrain.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace amx {

// the group block (doubles; the f32 chains are kept as f32 values in it)
enum { GRP_OBS = 0, GRP_ERR, GRP_TOTAL_WEIGHT, GRP_OBJECTIVE, GRP_CRITERION, GRP_SCALE, GRP_DO_SCALE, GRP_FINALIZED, GRP_STEP, GRP_SIZE = GRP_STEP + AMX_NNTRAIN_MAX_LAYERS };

constexpr int NS_SEG  = 4096;  // elements per segment sum of a norm: a constant of the library, so that the order depends on the shape alone
constexpr int NS_TILE = 32;    // the update kernel's tile edge
constexpr int NS_LD   = 33;    // LDS row of the transpose tile: bank (row + column) % 32 on both the row-wise write and the column-wise read

// ---- workgroup sums in a fixed order: lanes by xor-shuffle, the four waves ascending
template<class T>
__device__ __forceinline__ T block_sum(T v, T* s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = v + __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0)
        s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// ---- the regulariser's norms (Nn/Regularizer.cc:74-94,129-149,182-212): part[segment] = sum over the segment, in f64
// MODE 0: |x| (l1norm = asum);  1: x * x (sumOfSquares = dot);  2: d * d with d = x + (-1) * xc (diff.add(center, -1.0): saxpy)
template<int MODE>
__global__ __launch_bounds__(256) void nnstep_norm_kernel(const float* __restrict__ x, const float* __restrict__ xc, long long n, double* __restrict__ part) {
    __shared__ double s_red[4];
    const long long   base = (long long)blockIdx.x * NS_SEG;
    double            s    = 0.0;
#pragma unroll 4
    for (int k = 0; k < NS_SEG / 256; ++k) {
        const long long i = base + k * 256 + threadIdx.x;
        if (i < n) {
            float v = x[i];
            if (MODE == 2)
                v = fmaf(-1.f, xc[i], v);
            s += MODE == 0 ? (double)fabsf(v) : (double)v * (double)v;
        }
    }
    s = block_sum(s, s_red);
    if (threadIdx.x == 0)
        part[blockIdx.x] = s;
}

// out[0] = (f32) sum of part[0, n): thread t adds part[t], part[t + 256], ... ascending in f64, then the workgroup sum.  ONE workgroup
template<class T>
__global__ __launch_bounds__(256) void nnstep_sum_kernel(const T* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ double s_red[4];
    double            s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256)
        s += (double)part[i];
    s = block_sum(s, s_red);
    if (threadIdx.x == 0)
        out[0] = (float)s;
}

struct BookArgs {
    int   L, regularizer;
    float c[AMX_NNTRAIN_MAX_LAYERS];  // 0 = the layer takes no regulariser (not trainable, or regularization-constant 0)
};

// ---- after a call's pass: the group's counters and its f32 chains.  ONE thread
// call [4] = the pass's tail of this call; norm [2 x L] = (bias, weights) norms of the layers with c > 0
__global__ void nnstep_book_kernel(double* __restrict__ group, const double* __restrict__ call, const float* __restrict__ norm, BookArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    float objective = 0.f;
    if (a.regularizer != AMX_NNSTEP_REG_NONE)
        for (int l = 0; l < a.L; ++l) {
            if (!(a.c[l] > 0.f))
                continue;
            float tmp = norm[2 * l];
            tmp       = tmp + norm[2 * l + 1];
            if (a.regularizer == AMX_NNSTEP_REG_L1)
                tmp = tmp * a.c[l];
            else  // tmpObjectiveFunction *= regularizationConstant() / 2.0: a double factor, narrowed once
                tmp = (float)((double)tmp * ((double)a.c[l] / 2.0));
            objective = objective + tmp;
        }
    const float factor      = (float)(unsigned)call[0];  // T(batchSize)
    const float regularizer = factor * objective;
    const float criterion   = (float)call[3];
    group[GRP_OBS] += call[0];
    group[GRP_ERR] += call[1];
    group[GRP_TOTAL_WEIGHT] = (double)((float)group[GRP_TOTAL_WEIGHT] + (float)call[2]);
    float o                 = (float)group[GRP_OBJECTIVE];
    o                       = o + criterion;    // statistics_->addToObjectiveFunction(error)
    o                       = o + regularizer;  // statistics_->addToObjectiveFunction(regularizerError)
    group[GRP_OBJECTIVE]    = (double)o;
    group[GRP_CRITERION]    = (double)((float)group[GRP_CRITERION] + criterion);
}

// ---- Statistics::finalize (Nn/Statistics.cc:146-161): the scale the update kernels apply, and the objective.  ONE thread
// A group that is finalized already is not scaled again (isFinalized_); an empty group (no observations) is not scaled either.
__global__ void nnstep_finalize_kernel(double* __restrict__ group, int normalize) {
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    const float weight = normalize ? (float)(unsigned)group[GRP_OBS] : 1.0f;  // T normalizationWeight
    const bool  scale  = group[GRP_FINALIZED] == 0.0 && weight != 1.0f && weight != 0.0f;
    group[GRP_DO_SCALE] = scale ? 1.0 : 0.0;
    group[GRP_SCALE]    = scale ? (double)(float)(1.0 / (double)weight) : 1.0;
    if (scale) {
        group[GRP_OBJECTIVE] = (double)(float)((double)(float)group[GRP_OBJECTIVE] * (1.0 / (double)weight));
        group[GRP_CRITERION] = (double)(float)((double)(float)group[GRP_CRITERION] * (1.0 / (double)weight));
    }
    group[GRP_FINALIZED] = 1.0;
}

// FastMatrix::l1clipping (Math/FastMatrix.hh:1291-1303): std::max((T)0.0, w - v) is (0 < t) ? t : 0
__device__ __forceinline__ float l1_clip(float w, float v) {
    if (w > 0.f) {
        const float t = w - v;
        return 0.f < t ? t : 0.f;
    }
    if (w < 0.f) {
        const float t = w + v;
        return t < 0.f ? t : 0.f;
    }
    return w;
}

// ---- activation statistics of one layer's output Y [Tpad x ld] (Nn/NeuralNetworkLayer.cc:234-262, Math/FastVector.hh:461-478): one
// thread per unit, frames ascending, frames that did not enter the batch skipped.  A sum's chain over the call's first NT_CHUNK frames
// starts from the value the sum holds, every further chunk's chain from zero, chunk totals added ascending.  FMA: the two sites as
// the reference's default build contracts them.  T_in = the frames that entered (the call's tail).  stat [2 x n_pad]: sum, sumSq.
template<bool FMA, bool SQUARE>
__device__ __forceinline__ float actstat_chain(const float* __restrict__ y, int ld, int T, const int* __restrict__ label, float scale, float acc) {
    float total = acc;
    for (int t0 = 0; t0 < T; t0 += AMX_NNTRAIN_CHUNK) {
        float     part = t0 == 0 ? acc : 0.f;
        const int t1   = min(T, t0 + AMX_NNTRAIN_CHUNK);
        for (int t = t0; t < t1; ++t) {
            if (label[t] < 0)
                continue;
            const float v = y[(size_t)t * ld];
            part          = SQUARE ? mad<FMA>(scale * v, v, part) : mad<FMA>(scale, v, part);
        }
        total = t0 == 0 ? part : total + part;
    }
    return total;
}

template<bool FMA>
__global__ __launch_bounds__(256) void nnstep_actstat_kernel(const float* __restrict__ Y, int ld, int T, int n, int n_pad, const int* __restrict__ label,
                                                            const double* __restrict__ call_tail, int mode, float f, int init,
                                                            const float* __restrict__ initial, float* __restrict__ stat, double* __restrict__ nobs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const unsigned T_in  = (unsigned)call_tail[0];  // output.nColumns()
    const bool     trace = mode == AMX_NNSTEP_STAT_EXPONENTIAL_TRACE;
    const float*   y     = Y + i;
    float          s = stat[i], q = stat[n_pad + i];
    double         n_obs = i == 0 ? nobs[0] : 0.0;  // thread 0 alone keeps the count
    if (T_in == 0)  // nothing entered: the layer saw no batch
        return;
    if (init) {
        s = q = 0.f;
        n_obs = 0.0;
        if (initial) {  // activationSum_ = mean * nObservations_, activationSumOfSquares_ = (dev * dev + mean * mean) * nObservations_
            const unsigned n0 = trace ? 1u : T_in;
            const float    m = initial[i], d = initial[n_pad + i];
            s     = m * (float)n0;
            q     = (d * d + m * m) * (float)n0;
            n_obs = (double)n0;
        }
        else if (trace) {
            s = actstat_chain<FMA, false>(y, ld, T, label, 1.0f / (float)T_in, s);           // T(1.0) / output.nColumns()
            q = actstat_chain<FMA, true>(y, ld, T, label, (float)(1.0 / (double)T_in), q);  // 1.0 / output.nColumns(), narrowed by the call
        }
    }
    if (trace) {
        const float scale = (1.0f - f) / (float)T_in;
        s = f * s;
        s = actstat_chain<FMA, false>(y, ld, T, label, scale, s);
        q = f * q;
        q = actstat_chain<FMA, true>(y, ld, T, label, scale, q);
    }
    else {
        s = actstat_chain<FMA, false>(y, ld, T, label, 1.0f, s);
        q = actstat_chain<FMA, true>(y, ld, T, label, 1.0f, q);
        n_obs += (double)T_in;
    }
    stat[i]         = s;
    stat[n_pad + i] = q;
    if (i == 0)
        nobs[0] = n_obs;
}

// ---- the step on one layer's weights: ONE pass over G and W^T (both [Pin x Pout], the unit o contiguous), one 32 x 32 tile per
// workgroup, one float4 per thread on every side.  Per element: G *= scale (finalize); with MEAN  G = fmaf(m[i], -g[o], G)
// (addOuterProduct(mean, gradientBias, -1): sger), g the finalized bias gradient and m[i] = fmaf((f32)(1.0 / nObs), sum[i], 0) the mean
// of what feeds the layer; W = fmaf(neg_rate, G, W) (weights->add(G, -localLearningRate): saxpy) when update is set; the L1 clip when
// CLIP.  G and W^T are written back where they were read; the new weights go through an LDS tile (row NS_LD = 33 floats: the row-wise
// write of thread (r, c) and the column-wise read both land on bank (r + c) % 32, distinct within a half-wave) into W [Pout x Pin],
// the input i contiguous.  Elements outside the true in x out are written as zeros in all three, whatever G and m hold there: the
// GEMMs of the pass rely on a zero padding, and a padded unit of a sigmoid layer has an output of 0.5.
// abs_part[tile] = the tile's sum of |G| as written, f32, in the order of block_sum.  MEAN: colpart[tile_i][o] = the tile's part of
// sum_i G[i][o] m[i], one ascending chain of fused multiply-adds from zero.
template<bool CLIP, bool MEAN>
__global__ __launch_bounds__(256) void nnstep_update_kernel(float* __restrict__ G, float* __restrict__ WT, float* __restrict__ W, int Pin, int Pout, int in,
                                                           int out, const double* __restrict__ group, float neg_rate, int update, float clip,
                                                           float* __restrict__ abs_part, const float* __restrict__ gb, const float* __restrict__ act_sum,
                                                           const double* __restrict__ act_nobs, int act_trace, float* __restrict__ colpart) {
    __shared__ float s_tile[NS_TILE * NS_LD];
    __shared__ float s_dw[MEAN ? NS_TILE * NS_LD : 1];
    __shared__ float s_m[NS_TILE];
    __shared__ float s_red[4];
    const int tid = threadIdx.x, r = tid >> 3, c4 = (tid & 7) * 4;
    const int tiles_o = Pout / NS_TILE;
    const int tile_i = blockIdx.x / tiles_o, tile_o = blockIdx.x - tile_i * tiles_o;
    const int i0 = tile_i * NS_TILE, o0 = tile_o * NS_TILE;
    const bool  do_scale = group[GRP_DO_SCALE] != 0.0;
    const float scale    = (float)group[GRP_SCALE];

    if (MEAN) {
        if (tid < NS_TILE) {
            const unsigned n_obs = act_trace ? 1u : (unsigned)act_nobs[0];
            s_m[tid] = i0 + tid < in ? fmaf((float)(1.0 / (double)n_obs), act_sum[i0 + tid], 0.f) : 0.f;
        }
        __syncthreads();
    }
    const size_t at = (size_t)(i0 + r) * Pout + o0 + c4;
    const float4 g4 = *(const float4*)(G + at);
    const float4 w4 = *(const float4*)(WT + at);
    float        g[4] = {g4.x, g4.y, g4.z, g4.w}, w[4] = {w4.x, w4.y, w4.z, w4.w};
    float        sum = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (i0 + r < in && o0 + c4 + e < out) {
            if (do_scale)
                g[e] = g[e] * scale;
            if (MEAN) {
                float b = gb[o0 + c4 + e];
                if (do_scale)
                    b = b * scale;
                g[e] = fmaf(s_m[r], -b, g[e]);
            }
            if (update)
                w[e] = fmaf(neg_rate, g[e], w[e]);
            if (CLIP)
                w[e] = l1_clip(w[e], clip);
            sum = sum + fabsf(g[e]);
        }
        else
            g[e] = w[e] = 0.f;
        s_tile[r * NS_LD + c4 + e] = w[e];
        if (MEAN)
            s_dw[r * NS_LD + c4 + e] = g[e];
    }
    *(float4*)(G + at)  = make_float4(g[0], g[1], g[2], g[3]);
    *(float4*)(WT + at) = make_float4(w[0], w[1], w[2], w[3]);
    sum = block_sum(sum, s_red);  // its barrier also orders the tiles' writes before the reads below
    if (tid == 0)
        abs_part[blockIdx.x] = sum;
    if (MEAN && tid < NS_TILE) {  // column tid of the tile: bank (row + tid) % 32
        float acc = 0.f;
        for (int k = 0; k < NS_TILE; ++k)
            acc = fmaf(s_dw[k * NS_LD + tid], s_m[k], acc);
        colpart[(size_t)tile_i * Pout + o0 + tid] = acc;
    }
    // W[o0 + r][i0 + c4 .. + 3] = tile[c4 .. + 3][r]
    *(float4*)(W + (size_t)(o0 + r) * Pin + i0 + c4) =
        make_float4(s_tile[(c4 + 0) * NS_LD + r], s_tile[(c4 + 1) * NS_LD + r], s_tile[(c4 + 2) * NS_LD + r], s_tile[(c4 + 3) * NS_LD + r]);
}

// ---- the same for the bias gradient g and the bias b [Pout], after the layer's update kernel; abs_part[block] = the block's sum of |g|
// n_tiles_i > 0: g[o] = fmaf(-1, sum over the tile rows of colpart[.][o] ascending, g[o]) first (multiply(mean, g, transposed, -1, 1): sgemv)
template<bool CLIP>
__global__ __launch_bounds__(256) void nnstep_bias_kernel(float* __restrict__ g, float* __restrict__ b, int Pout, int out, const double* __restrict__ group,
                                                         float neg_rate, int update, float clip, float* __restrict__ abs_part,
                                                         const float* __restrict__ colpart, int n_tiles_i) {
    __shared__ float s_red[4];
    const int   o   = blockIdx.x * 256 + threadIdx.x;
    float       sum = 0.f;
    if (o < Pout) {
        float gv = 0.f, bv = 0.f;
        if (o < out) {
            gv = g[o], bv = b[o];
            if (group[GRP_DO_SCALE] != 0.0)
                gv = gv * (float)group[GRP_SCALE];
            if (n_tiles_i > 0) {
                float dot = 0.f;
                for (int k = 0; k < n_tiles_i; ++k)
                    dot = dot + colpart[(size_t)k * Pout + o];
                gv = fmaf(-1.f, dot, gv);
            }
            if (update)
                bv = fmaf(neg_rate, gv, bv);
            if (CLIP)
                bv = l1_clip(bv, clip);
            sum = fabsf(gv);
        }
        g[o] = gv;
        b[o] = bv;
    }
    sum = block_sum(sum, s_red);
    if (threadIdx.x == 0)
        abs_part[blockIdx.x] = sum;
}

// ---- stepSizes[layer] (Nn/MeanNormalizedSgdEstimator.cc:95-97,117-119): (0 + asum(G) * rate) + asum(g) * bias_rate, the two asums from
// the tile sums (abs_part[0, n_w)) and the bias blocks' (abs_part[n_w, n_w + n_b)), each added as nnstep_sum_kernel adds.  ONE workgroup
__global__ __launch_bounds__(256) void nnstep_stepsize_kernel(const float* __restrict__ abs_part, int n_w, int n_b, float rate, float bias_rate, int count_w,
                                                             int count_b, double* __restrict__ step) {
    __shared__ double s_red[4];
    double            s = 0.0;
    for (int i = threadIdx.x; i < n_w; i += 256)
        s += (double)abs_part[i];
    const float asum_w = (float)block_sum(s, s_red);
    __syncthreads();
    s = 0.0;
    for (int i = threadIdx.x; i < n_b; i += 256)
        s += (double)abs_part[n_w + i];
    const float asum_b = (float)block_sum(s, s_red);
    if (threadIdx.x == 0) {
        float v = 0.f;
        if (count_w)
            v = v + asum_w * rate;
        if (count_b)
            v = v + asum_b * bias_rate;
        step[0] = (double)v;
    }
}

}  // namespace amx

// ------------------------------------------------------------------------------------ host side

namespace {

using amx::NnStep;

bool layer_regularized(const NnStep& s, int l) {
    return s.regularizer != AMX_NNSTEP_REG_NONE && s.trainable[l] && s.c[l] > 0.f;
}

// layer 0's weights: the reference's loop over input streams runs to nPredecessors(), which is 0 for a layer fed by the feature stream
bool updates_weights(const amx_nntrain* h, int l) {
    const NnStep& s = h->step;
    return s.trainable[l] && (l > 0 || h->pre.n > 0 || s.update_input);
}

int require_step(const amx_nntrain* h, const char* who) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(h->step.set, AMX_ERR_STATE, "%s: no estimator is set (amx_nntrain_set_estimator)", who);
    return AMX_OK;
}

void fill_info(const amx_nntrain* h, const double* g, int updated, amx_nnstep_info* info) {
    memset(info, 0, sizeof *info);
    info->minibatch               = h->step.n;
    info->updated                 = updated;
    info->n_observations          = (long)g[amx::GRP_OBS];
    info->n_classification_errors = (long)g[amx::GRP_ERR];
    info->total_weight            = (float)g[amx::GRP_TOTAL_WEIGHT];
    info->objective               = (float)g[amx::GRP_OBJECTIVE];
    info->criterion_objective     = (float)g[amx::GRP_CRITERION];
    for (int l = 0; l < h->L; ++l)
        info->step_size[l] = (float)g[amx::GRP_STEP + l];
}

int read_info(amx_nntrain* h, int updated, amx_nnstep_info* info) {
    NnStep& s = h->step;
    AMX_HIP(hipMemcpyAsync(s.h_group.get(), s.d_group.get(), amx::GRP_SIZE * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    AMX_HIP(hipStreamSynchronize(h->ctx->stream));
    fill_info(h, s.h_group.get(), updated, info);
    return AMX_OK;
}

// the regulariser's objective of the network as it stands: norms of the regularised layers into d_norm, by the stream's order
int launch_norms(amx_nntrain* h) {
    NnStep&     s  = h->step;
    hipStream_t st = h->ctx->stream;
    if (s.regularizer == AMX_NNSTEP_REG_NONE)
        return AMX_OK;
    amx::ScopedKernelTimer timer(h->ctx, "nnstep_norms");
    for (int l = 0; l < h->L; ++l) {
        if (!layer_regularized(s, l))
            continue;
        for (int which = 0; which < 2; ++which) {  // 0 = bias, 1 = weights (the transposed image: a norm does not see the layout)
            const long long n  = which ? (long long)h->Pin[l] * h->Pout[l] : (long long)h->Pout[l];
            const float*    x  = which ? h->d_WT[l].get() : h->d_bias[l].get();
            const float*    xc = s.regularizer == AMX_NNSTEP_REG_CENTERED_L2 ? (which ? s.d_WTc[l].get() : s.d_bc[l].get()) : nullptr;
            const int       nb = (int)((n + amx::NS_SEG - 1) / amx::NS_SEG);
            double*         part = s.d_norm_part.get();
            if (s.regularizer == AMX_NNSTEP_REG_L1)
                hipLaunchKernelGGL(amx::nnstep_norm_kernel<0>, dim3(nb), dim3(256), 0, st, x, xc, n, part);
            else if (s.regularizer == AMX_NNSTEP_REG_L2)
                hipLaunchKernelGGL(amx::nnstep_norm_kernel<1>, dim3(nb), dim3(256), 0, st, x, xc, n, part);
            else
                hipLaunchKernelGGL(amx::nnstep_norm_kernel<2>, dim3(nb), dim3(256), 0, st, x, xc, n, part);
            hipLaunchKernelGGL(amx::nnstep_sum_kernel<double>, dim3(1), dim3(256), 0, st, (const double*)part, nb, s.d_norm.get() + 2 * l + which);
        }
    }
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

int launch_book(amx_nntrain* h) {
    NnStep&       s = h->step;
    amx::BookArgs a{};
    a.L           = h->L;
    a.regularizer = s.regularizer;
    for (int l = 0; l < h->L; ++l)
        a.c[l] = layer_regularized(s, l) ? s.c[l] : 0.f;
    hipLaunchKernelGGL(amx::nnstep_book_kernel, dim3(1), dim3(64), 0, h->ctx->stream, s.d_group.get(), (const double*)s.d_call.get(), (const float*)s.d_norm.get(), a);
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

// finalizeForwarding of every layer that keeps statistics, on the layer inputs the pass left in d_x
int launch_actstat(amx_nntrain* h, int T) {
    NnStep&     s  = h->step;
    hipStream_t st = h->ctx->stream;
    for (int p = 0; p < h->L; ++p) {
        if (s.stat_mode[p] == AMX_NNSTEP_STAT_NO_STATISTICS)
            continue;
        amx::ScopedKernelTimer timer(h->ctx, "nnstep_activation_statistics");
        const float* initial = s.stat_has_initial[p] ? s.d_act_initial[p].get() : nullptr;
        const dim3   grid((h->in[p] + 255) / 256);
        if (h->ctx->contract == AMX_CONTRACT_FMA)
            hipLaunchKernelGGL(amx::nnstep_actstat_kernel<true>, grid, dim3(256), 0, st, (const float*)h->d_x[p].get(), h->Pin[p], T, h->in[p], h->Pin[p],
                               (const int*)h->d_label.get(), (const double*)s.d_call.get(), s.stat_mode[p], s.stat_f[p], (int)s.stat_need_init[p], initial,
                               s.d_act[p].get(), s.d_act_nobs.get() + p);
        else
            hipLaunchKernelGGL(amx::nnstep_actstat_kernel<false>, grid, dim3(256), 0, st, (const float*)h->d_x[p].get(), h->Pin[p], T, h->in[p], h->Pin[p],
                               (const int*)h->d_label.get(), (const double*)s.d_call.get(), s.stat_mode[p], s.stat_f[p], (int)s.stat_need_init[p], initial,
                               s.d_act[p].get(), s.d_act_nobs.get() + p);
        s.stat_need_init[p] = 0;
    }
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

void make_sink(amx_nntrain* h, amx::StepSink* k, int reset) {
    NnStep& s      = h->step;
    k->call_tail   = s.d_call.get();
    k->group_tail  = s.d_group.get();
    k->reset       = reset;
    k->group_block = s.d_group.get();
    k->group_bytes = amx::GRP_SIZE * sizeof(double);
    k->regularizer = s.regularizer;
    for (int l = 0; l < h->L; ++l) {
        k->G[l] = s.d_G[l].get();
        k->g[l] = s.d_g[l].get();
        k->c[l] = layer_regularized(s, l) ? s.c[l] : 0.f;
        if (s.regularizer == AMX_NNSTEP_REG_CENTERED_L2) {
            k->WTc[l] = s.d_WTc[l].get();
            k->bc[l]  = s.d_bc[l].get();
        }
    }
}

int step_accumulate(amx_nntrain* h, const float* feats, int ldf, int T, const uint32_t* emission, const double* weight, const char* who) {
    AMX_TRY(require_step(h, who));
    AMX_REQUIRE(T >= 1, AMX_ERR_INVALID, "%s: T = %d (1..%d frames per call)", who, T, AMX_NNTRAIN_MAX_FRAMES);
    NnStep&     s     = h->step;
    hipStream_t st    = h->ctx->stream;
    const int   reset = (s.n % s.A) == 0 ? 1 : 0;  // (minibatchCount_ - 1) % accumulateMultipleBatches() == 0 with the count already raised
    AMX_HIP(hipSetDevice(h->ctx->device));
    // a refused call (bad argument, bad label) leaves everything as it was: nothing behind the pass's label check has run, the
    // clearing of a new group's block included
    AMX_HIP(hipMemsetAsync(s.d_call.get(), 0, 4 * sizeof(double), st));
    amx::StepSink sink;
    make_sink(h, &sink, reset);
    const int r = amx::nntrain_pass(h, feats, ldf, T, emission, weight, nullptr, &sink, who);
    if (r != AMX_OK)
        return r;
    s.n += 1;
    AMX_TRY(launch_actstat(h, T));
    AMX_TRY(launch_norms(h));
    AMX_TRY(launch_book(h));
    return AMX_OK;
}

int step_estimate(amx_nntrain* h, int normalize, const char* who) {
    AMX_TRY(require_step(h, who));
    NnStep&     s  = h->step;
    hipStream_t st = h->ctx->stream;
    AMX_HIP(hipSetDevice(h->ctx->device));
    hipLaunchKernelGGL(amx::nnstep_finalize_kernel, dim3(1), dim3(64), 0, st, s.d_group.get(), normalize);
    const bool   clip  = s.estimator == AMX_NNSTEP_MEAN_NORMALIZED_SGD_L1_CLIPPING;
    const double* grp  = s.d_group.get();
    for (int l = 0; l < h->L; ++l) {
        const int   Pin = h->Pin[l], Pout = h->Pout[l];
        const float rate      = s.eta * s.eta_l[l];               // learningRate * layer.learningRate()
        const float bias_rate = s.eta * s.eta_bias * s.eta_l[l];  // learningRate * biasLearningRate_ * layer.learningRate()
        const float clip_v    = s.c[l] * s.eta * s.eta_l[l];      // regularizationConstant() * learningRate * layer.learningRate()
        const int   up_w = updates_weights(h, l) ? 1 : 0, up_b = s.trainable[l] ? 1 : 0;
        const bool  do_clip = clip && s.trainable[l];
        const int   n_w = (Pin / amx::NS_TILE) * (Pout / amx::NS_TILE), n_b = (Pout + 255) / 256;
        float*      part = s.d_abs_part.get();
        // the mean of what feeds the layer enters inside the loop over input streams: only where the weights are updated
        const bool   mean    = up_w && s.stat_mode[l] != AMX_NNSTEP_STAT_NO_STATISTICS;
        const float* act_sum = mean ? s.d_act[l].get() : nullptr;
        const double* act_n  = s.d_act_nobs.get() + l;
        const int    trace   = s.stat_mode[l] == AMX_NNSTEP_STAT_EXPONENTIAL_TRACE ? 1 : 0;
        float*       colpart = s.d_colpart.get();
        AMX_REQUIRE(!mean || !s.stat_need_init[l], AMX_ERR_STATE, "%s: layer %d: the activation statistics of its input have seen no mini-batch yet", who, l);
        {
            amx::ScopedKernelTimer timer(h->ctx, "nnstep_update");
#define AMX_NNSTEP_LAUNCH(CLIP, MEAN)                                                                                                                  \
    do {                                                                                                                                               \
        hipLaunchKernelGGL((amx::nnstep_update_kernel<CLIP, MEAN>), dim3(n_w), dim3(256), 0, st, s.d_G[l].get(), h->d_WT[l].get(), h->d_W[l].get(), Pin, \
                           Pout, h->in[l], h->out[l], grp, -rate, up_w, clip_v, part, (const float*)s.d_g[l].get(), act_sum, act_n, trace, colpart);    \
        hipLaunchKernelGGL(amx::nnstep_bias_kernel<CLIP>, dim3(n_b), dim3(256), 0, st, s.d_g[l].get(), h->d_bias[l].get(), Pout, h->out[l], grp,       \
                           -bias_rate, up_b, clip_v, part + n_w, (const float*)colpart, MEAN ? Pin / amx::NS_TILE : 0);                                 \
    } while (0)
            if (do_clip && mean)
                AMX_NNSTEP_LAUNCH(true, true);
            else if (do_clip)
                AMX_NNSTEP_LAUNCH(true, false);
            else if (mean)
                AMX_NNSTEP_LAUNCH(false, true);
            else
                AMX_NNSTEP_LAUNCH(false, false);
#undef AMX_NNSTEP_LAUNCH
        }
        amx::ScopedKernelTimer timer(h->ctx, "nnstep_step_size");
        hipLaunchKernelGGL(amx::nnstep_stepsize_kernel, dim3(1), dim3(256), 0, st, (const float*)part, n_w, n_b, rate, bias_rate, s.log_step ? up_w : 0,
                           s.log_step ? up_b : 0, s.d_group.get() + amx::GRP_STEP + l);
    }
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

int copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
    AMX_HIP(hipMemcpy2D(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost));
    return AMX_OK;
}

}  // namespace

extern "C" {

void amx_nnstep_default_cfg(amx_nnstep_cfg* cfg) {
    if (!cfg)
        return;
    memset(cfg, 0, sizeof *cfg);
    cfg->learning_rate               = 1.f;
    cfg->bias_learning_rate          = 1.f;
    cfg->regularizer                 = AMX_NNSTEP_REG_NONE;
    cfg->estimator                   = AMX_NNSTEP_MEAN_NORMALIZED_SGD;
    cfg->accumulate_multiple_batches = 1;
    cfg->normalize_by_observations   = 1;
    cfg->update_input_layer_weights  = 1;
    cfg->input_smoothing             = AMX_NNSTEP_STAT_NO_STATISTICS;
    cfg->input_trace_factor          = 0.5f;
}

int amx_nntrain_set_estimator(amx_nntrain* h, const amx_nnstep_cfg* cfg) {
    AMX_REQUIRE(h && cfg, AMX_ERR_INVALID, "amx_nntrain_set_estimator: NULL argument");
    AMX_REQUIRE(h->L > 0, AMX_ERR_INVALID, "amx_nntrain_set_estimator: the handle has no network to train");
    AMX_REQUIRE(h->mask == (AMX_NNSTAT_BASE | AMX_NNSTAT_GRADIENT), AMX_ERR_INVALID,
                "amx_nntrain_set_estimator: the handle's statistics must be base statistics and the gradient, nothing else (mask %d)", h->mask);
    AMX_REQUIRE(std::isfinite(cfg->learning_rate) && std::isfinite(cfg->bias_learning_rate), AMX_ERR_INVALID,
                "amx_nntrain_set_estimator: learning_rate / bias_learning_rate is not finite");
    AMX_REQUIRE(cfg->accumulate_multiple_batches >= 1, AMX_ERR_INVALID, "amx_nntrain_set_estimator: accumulate_multiple_batches = %d (must be >= 1)",
                cfg->accumulate_multiple_batches);
    AMX_REQUIRE(cfg->regularizer >= AMX_NNSTEP_REG_NONE && cfg->regularizer <= AMX_NNSTEP_REG_CENTERED_L2, AMX_ERR_INVALID,
                "amx_nntrain_set_estimator: regularizer = %d is none of none, l1, l2, centered-l2", cfg->regularizer);
    AMX_REQUIRE(cfg->estimator == AMX_NNSTEP_MEAN_NORMALIZED_SGD || cfg->estimator == AMX_NNSTEP_MEAN_NORMALIZED_SGD_L1_CLIPPING, AMX_ERR_INVALID,
                "amx_nntrain_set_estimator: estimator = %d is neither mean-normalized-sgd nor mean-normalized-sgd-l1-clipping", cfg->estimator);
    const int L = h->L;
    amx::NnStep n;  // built aside: a refused configuration leaves the handle's as it was
    n.eta = cfg->learning_rate, n.eta_bias = cfg->bias_learning_rate;
    n.regularizer = cfg->regularizer, n.estimator = cfg->estimator, n.A = cfg->accumulate_multiple_batches;
    n.normalize = cfg->normalize_by_observations ? 1 : 0, n.log_step = cfg->log_step_size ? 1 : 0, n.update_input = cfg->update_input_layer_weights ? 1 : 0;
    for (int l = 0; l < L; ++l) {
        const float rate = cfg->layer_learning_rate ? cfg->layer_learning_rate[l] : 1.f;
        const float c    = cfg->regularization_constant ? cfg->regularization_constant[l] : 0.f;
        AMX_REQUIRE(std::isfinite(rate), AMX_ERR_INVALID, "amx_nntrain_set_estimator: layer_learning_rate[%d] is not finite", l);
        AMX_REQUIRE(c >= 0.f && std::isfinite(c), AMX_ERR_INVALID, "amx_nntrain_set_estimator: regularization_constant[%d] = %g (must be >= 0)", l, c);
        n.eta_l.push_back(rate);
        n.c.push_back(c);
        n.trainable.push_back(cfg->trainable ? (cfg->trainable[l] ? 1 : 0) : 1);
    }
    // activation statistics by the layer they feed: p = 0 the last preprocessing layer, p = l the output of layer l - 1
    std::vector<std::vector<float>> initial((size_t)L);
    n.stat_mode.assign((size_t)L, AMX_NNSTEP_STAT_NO_STATISTICS);
    n.stat_f.assign((size_t)L, 0.5f);
    n.stat_need_init.assign((size_t)L, 1);
    n.stat_has_initial.assign((size_t)L, 0);
    for (int p = 0; p < L; ++p) {
        const int    mode = p == 0 ? cfg->input_smoothing : (cfg->statistics_smoothing ? cfg->statistics_smoothing[p - 1] : 0);
        const float  f    = p == 0 ? cfg->input_trace_factor : (cfg->trace_factor ? cfg->trace_factor[p - 1] : 0.5f);
        const float* mean = p == 0 ? cfg->input_initial_mean : (cfg->initial_activation_mean ? cfg->initial_activation_mean[p - 1] : nullptr);
        const float* dev  = p == 0 ? cfg->input_initial_stddev : (cfg->initial_activation_stddev ? cfg->initial_activation_stddev[p - 1] : nullptr);
        AMX_REQUIRE(mode >= AMX_NNSTEP_STAT_NO_STATISTICS && mode <= AMX_NNSTEP_STAT_EXPONENTIAL_TRACE, AMX_ERR_INVALID,
                    "amx_nntrain_set_estimator: %s = %d is none of no-statistics, none, exponential-trace", p == 0 ? "input_smoothing" : "statistics_smoothing", mode);
        AMX_REQUIRE(p > 0 || mode == AMX_NNSTEP_STAT_NO_STATISTICS || h->pre.n > 0 || !h->ctx, AMX_ERR_INVALID,
                    "amx_nntrain_set_estimator: input_smoothing without a preprocessing layer: layer 0 is fed by the feature stream, which keeps no statistics");
        if (mode == AMX_NNSTEP_STAT_NO_STATISTICS)
            continue;
        AMX_REQUIRE(std::isfinite(f), AMX_ERR_INVALID, "amx_nntrain_set_estimator: the trace factor of layer %d's input is not finite", p);
        AMX_REQUIRE((mean != nullptr) == (dev != nullptr), AMX_ERR_INVALID,
                    "amx_nntrain_set_estimator: layer %d's input: an initial activation mean and deviation come together", p);
        n.stat_mode[p] = mode;
        n.stat_f[p]    = f;
        if (mean) {
            n.stat_has_initial[p] = 1;
            initial[p].assign((size_t)2 * h->Pin[p], 0.f);
            for (int i = 0; i < h->in[p]; ++i) {
                initial[p][i]             = mean[i];
                initial[p][h->Pin[p] + i] = dev[i];
            }
        }
    }
    if (cfg->statistics_smoothing)
        AMX_REQUIRE(cfg->statistics_smoothing[L - 1] == AMX_NNSTEP_STAT_NO_STATISTICS, AMX_ERR_UNSUPPORTED,
                    "amx_nntrain_set_estimator: statistics_smoothing[%d]: the output layer keeps no statistics (nothing reads them)", L - 1);
    if (n.regularizer == AMX_NNSTEP_REG_CENTERED_L2) {
        AMX_REQUIRE(cfg->center_W && cfg->center_bias && cfg->center_in_dim && cfg->center_out_dim, AMX_ERR_INVALID,
                    "amx_nntrain_set_estimator: centered-l2 needs center_W, center_bias, center_in_dim and center_out_dim");
        for (int l = 0; l < L; ++l) {
            AMX_REQUIRE(cfg->center_in_dim[l] == h->in[l] && cfg->center_out_dim[l] == h->out[l], AMX_ERR_INVALID,
                        "amx_nntrain_set_estimator: layer %d: the centre is %d -> %d, the network's layer %d -> %d", l, cfg->center_in_dim[l], cfg->center_out_dim[l],
                        h->in[l], h->out[l]);
            AMX_REQUIRE(cfg->center_W[l] && cfg->center_bias[l], AMX_ERR_INVALID, "amx_nntrain_set_estimator: layer %d: the centre's parameters are NULL", l);
            n.center_W.emplace_back(cfg->center_W[l], cfg->center_W[l] + (size_t)h->in[l] * h->out[l]);
            n.center_b.emplace_back(cfg->center_bias[l], cfg->center_bias[l] + h->out[l]);
        }
    }
    if (h->ctx) {
        AMX_HIP(hipSetDevice(h->ctx->device));
        AMX_HIP(hipStreamSynchronize(h->ctx->stream));  // a set before may still be in use
        n.d_G   = std::vector<amx::DevBuf<float>>(L);
        n.d_g   = std::vector<amx::DevBuf<float>>(L);
        n.d_WTc = std::vector<amx::DevBuf<float>>(L);
        n.d_bc  = std::vector<amx::DevBuf<float>>(L);
        size_t norm_part = 1, abs_part = 1;
        for (int l = 0; l < L; ++l) {
            const int    K = h->in[l], N = h->out[l], Kp = h->Pin[l], Np = h->Pout[l];
            const size_t n_w = (size_t)Kp * Np;
            std::vector<float> zero(n_w, 0.f);
            AMX_TRY(n.d_G[l].upload(zero.data(), n_w));
            AMX_TRY(n.d_g[l].upload(zero.data(), (size_t)Np));
            if (n.regularizer == AMX_NNSTEP_REG_CENTERED_L2) {
                std::vector<float> bc((size_t)Np, 0.f);
                for (int o = 0; o < N; ++o) {
                    for (int k = 0; k < K; ++k)
                        zero[(size_t)k * Np + o] = n.center_W[l][(size_t)o * K + k];
                    bc[o] = n.center_b[l][o];
                }
                AMX_TRY(n.d_WTc[l].upload(zero.data(), n_w));
                AMX_TRY(n.d_bc[l].upload(bc.data(), bc.size()));
            }
            norm_part = std::max(norm_part, (n_w + amx::NS_SEG - 1) / amx::NS_SEG);
            abs_part  = std::max(abs_part, (size_t)(Kp / amx::NS_TILE) * (Np / amx::NS_TILE) + (size_t)(Np + 255) / 256);
        }
        std::vector<double> zero((size_t)amx::GRP_SIZE, 0.0);
        std::vector<float>  zf((size_t)2 * L, 0.f);
        AMX_TRY(n.d_group.upload(zero.data(), zero.size()));
        AMX_TRY(n.d_call.upload(zero.data(), 4));
        AMX_TRY(n.d_norm.upload(zf.data(), zf.size()));
        AMX_TRY(n.d_norm_part.reserve(norm_part));
        AMX_TRY(n.d_abs_part.reserve(abs_part));
        AMX_TRY(n.h_group.reserve((size_t)amx::GRP_SIZE));
        n.d_act         = std::vector<amx::DevBuf<float>>(L);
        n.d_act_initial = std::vector<amx::DevBuf<float>>(L);
        size_t colpart  = 1;
        for (int p = 0; p < L; ++p) {
            if (n.stat_mode[p] == AMX_NNSTEP_STAT_NO_STATISTICS)
                continue;
            std::vector<float> zero2((size_t)2 * h->Pin[p], 0.f);
            AMX_TRY(n.d_act[p].upload(zero2.data(), zero2.size()));
            if (n.stat_has_initial[p])
                AMX_TRY(n.d_act_initial[p].upload(initial[p].data(), initial[p].size()));
            colpart = std::max(colpart, (size_t)(h->Pin[p] / amx::NS_TILE) * h->Pout[p]);
        }
        AMX_TRY(n.d_act_nobs.upload(zero.data(), (size_t)L));
        AMX_TRY(n.d_colpart.reserve(colpart));
    }
    n.set = true;
    n.n   = 0;
    std::swap(h->step, n);
    return AMX_OK;
}

int amx_nntrain_step_accumulate_dev(amx_nntrain* h, const float* feats, int ldf, int T, const uint32_t* emission, const double* weight) {
    return step_accumulate(h, feats, ldf, T, emission, weight, "amx_nntrain_step_accumulate_dev");
}

int amx_nntrain_step_estimate_dev(amx_nntrain* h) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_nntrain_step_estimate_dev: NULL argument");
    return step_estimate(h, h->step.normalize, "amx_nntrain_step_estimate_dev");
}

int amx_nntrain_step_dev(amx_nntrain* h, const float* feats, int ldf, int T, const uint32_t* emission, const double* weight, amx_nnstep_info* info) {
    AMX_TRY(step_accumulate(h, feats, ldf, T, emission, weight, "amx_nntrain_step_dev"));
    const int update = (h->step.n % h->step.A) == 0 ? 1 : 0;
    if (update)
        AMX_TRY(step_estimate(h, h->step.normalize, "amx_nntrain_step_dev"));
    if (info)
        AMX_TRY(read_info(h, update, info));
    return AMX_OK;
}

int amx_nntrain_step_info(amx_nntrain* h, amx_nnstep_info* info) {
    AMX_TRY(require_step(h, "amx_nntrain_step_info"));
    AMX_REQUIRE(info, AMX_ERR_INVALID, "amx_nntrain_step_info: NULL argument");
    AMX_HIP(hipSetDevice(h->ctx->device));
    AMX_TRY(read_info(h, 0, info));
    info->updated = h->step.h_group.get()[amx::GRP_FINALIZED] != 0.0 ? 1 : 0;
    return AMX_OK;
}

int amx_nntrain_estimate(amx_nntrain* h, const double* acc, amx_nnstep_info* info) {
    AMX_TRY(require_step(h, "amx_nntrain_estimate"));
    AMX_REQUIRE(acc, AMX_ERR_INVALID, "amx_nntrain_estimate: NULL argument");
    amx::NnStep&                    s = h->step;
    std::vector<std::vector<float>> gw, gb;
    uint32_t                        n_obs = 0, n_err = 0;
    float                           total_weight = 0.f, objective = 0.f;
    AMX_TRY(amx::nntrain_narrow_gradient(h, acc, &gw, &gb, &n_obs, &n_err, &total_weight, &objective, "amx_nntrain_estimate"));
    hipStream_t st = h->ctx->stream;
    AMX_HIP(hipSetDevice(h->ctx->device));
    AMX_HIP(hipStreamSynchronize(st));
    // the narrowed statistics become the group's (padded as the kernels expect them)
    for (int l = 0; l < h->L; ++l) {
        AMX_HIP(hipMemset(s.d_G[l].get(), 0, (size_t)h->Pin[l] * h->Pout[l] * sizeof(float)));
        AMX_HIP(hipMemset(s.d_g[l].get(), 0, (size_t)h->Pout[l] * sizeof(float)));
        AMX_HIP(hipMemcpy2D(s.d_G[l].get(), (size_t)h->Pout[l] * sizeof(float), gw[l].data(), (size_t)h->out[l] * sizeof(float), (size_t)h->out[l] * sizeof(float),
                            (size_t)h->in[l], hipMemcpyHostToDevice));
        AMX_HIP(hipMemcpy(s.d_g[l].get(), gb[l].data(), (size_t)h->out[l] * sizeof(float), hipMemcpyHostToDevice));
    }
    std::vector<double> group((size_t)amx::GRP_SIZE, 0.0), call(4, 0.0);
    group[amx::GRP_TOTAL_WEIGHT] = (double)total_weight;
    // the book kernel adds the "call": its observations are the regulariser's factor for the objective and, the group's being zero
    // before, for the gradient; the criterion's part of the objective is the file's
    call[0] = (double)n_obs, call[1] = (double)n_err, call[3] = (double)objective;
    AMX_HIP(hipMemcpy(s.d_group.get(), group.data(), group.size() * sizeof(double), hipMemcpyHostToDevice));
    AMX_HIP(hipMemcpy(s.d_call.get(), call.data(), 4 * sizeof(double), hipMemcpyHostToDevice));
    if (s.regularizer != AMX_NNSTEP_REG_NONE) {  // regularizer.addGradient(network, statistics, statistics.nObservations())
        amx::StepSink sink;
        make_sink(h, &sink, 0);
        AMX_TRY(amx::nntrain_add_regularizer(h, &sink));
    }
    AMX_TRY(launch_norms(h));
    AMX_TRY(launch_book(h));
    AMX_TRY(step_estimate(h, 1, "amx_nntrain_estimate"));  // statistics_->finalize(): the default argument normalizes
    if (info) {
        AMX_TRY(read_info(h, 1, info));
        info->total_weight = total_weight;  // the book kernel added the call's zero to it
    }
    return AMX_OK;
}

int amx_nntrain_get_parameters(amx_nntrain* h, int layer, int image, float* W, float* bias) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_nntrain_get_parameters: NULL argument");
    AMX_REQUIRE(h->L > 0, AMX_ERR_STATE, "amx_nntrain_get_parameters: the handle has no network");
    AMX_REQUIRE(layer >= 0 && layer < h->L, AMX_ERR_INVALID, "amx_nntrain_get_parameters: layer = %d (0..%d)", layer, h->L - 1);
    AMX_REQUIRE(image == 0 || image == 1, AMX_ERR_INVALID, "amx_nntrain_get_parameters: image = %d (0 = forward, 1 = transposed)", image);
    const int K = h->in[layer], N = h->out[layer], Kp = h->Pin[layer], Np = h->Pout[layer];
    if (!h->ctx) {
        if (W)
            memcpy(W, h->host_W[layer].data(), (size_t)K * N * sizeof(float));
        if (bias)
            memcpy(bias, h->host_bias[layer].data(), (size_t)N * sizeof(float));
        return AMX_OK;
    }
    AMX_HIP(hipSetDevice(h->ctx->device));
    AMX_HIP(hipStreamSynchronize(h->ctx->stream));
    if (W && image == 0)
        AMX_TRY(copy_rows(W, (size_t)K * sizeof(float), h->d_W[layer].get(), (size_t)Kp * sizeof(float), (size_t)K * sizeof(float), (size_t)N));
    if (W && image == 1) {
        std::vector<float> t((size_t)K * N);
        AMX_TRY(copy_rows(t.data(), (size_t)N * sizeof(float), h->d_WT[layer].get(), (size_t)Np * sizeof(float), (size_t)N * sizeof(float), (size_t)K));
        for (int k = 0; k < K; ++k)
            for (int o = 0; o < N; ++o)
                W[(size_t)o * K + k] = t[(size_t)k * N + o];
    }
    if (bias)
        AMX_HIP(hipMemcpy(bias, h->d_bias[layer].get(), (size_t)N * sizeof(float), hipMemcpyDeviceToHost));
    return AMX_OK;
}

int amx_nntrain_get_step_statistics(amx_nntrain* h, int layer, float* G, float* g) {
    AMX_TRY(require_step(h, "amx_nntrain_get_step_statistics"));
    AMX_REQUIRE(layer >= 0 && layer < h->L, AMX_ERR_INVALID, "amx_nntrain_get_step_statistics: layer = %d (0..%d)", layer, h->L - 1);
    const int K = h->in[layer], N = h->out[layer], Np = h->Pout[layer];
    AMX_HIP(hipSetDevice(h->ctx->device));
    AMX_HIP(hipStreamSynchronize(h->ctx->stream));
    if (G)
        AMX_TRY(copy_rows(G, (size_t)N * sizeof(float), h->step.d_G[layer].get(), (size_t)Np * sizeof(float), (size_t)N * sizeof(float), (size_t)K));
    if (g)
        AMX_HIP(hipMemcpy(g, h->step.d_g[layer].get(), (size_t)N * sizeof(float), hipMemcpyDeviceToHost));
    return AMX_OK;
}

int amx_nntrain_get_activation_statistics(amx_nntrain* h, int layer, float* mean, float* variance) {
    AMX_TRY(require_step(h, "amx_nntrain_get_activation_statistics"));
    AMX_REQUIRE(layer >= -1 && layer < h->L - 1, AMX_ERR_INVALID, "amx_nntrain_get_activation_statistics: layer = %d (-1..%d)", layer, h->L - 2);
    amx::NnStep& s = h->step;
    const int    p = layer + 1, n = h->in[p], Pn = h->Pin[p];
    AMX_REQUIRE(s.stat_mode[p] != AMX_NNSTEP_STAT_NO_STATISTICS, AMX_ERR_STATE, "amx_nntrain_get_activation_statistics: layer %d keeps no statistics", layer);
    AMX_REQUIRE(!s.stat_need_init[p], AMX_ERR_STATE, "amx_nntrain_get_activation_statistics: layer %d has seen no mini-batch yet", layer);
    AMX_HIP(hipSetDevice(h->ctx->device));
    AMX_HIP(hipStreamSynchronize(h->ctx->stream));
    std::vector<float> stat((size_t)2 * Pn);
    double             n_obs = 0.0;
    AMX_HIP(hipMemcpy(stat.data(), s.d_act[p].get(), stat.size() * sizeof(float), hipMemcpyDeviceToHost));
    AMX_HIP(hipMemcpy(&n_obs, s.d_act_nobs.get() + p, sizeof(double), hipMemcpyDeviceToHost));
    const unsigned count = s.stat_mode[p] == AMX_NNSTEP_STAT_EXPONENTIAL_TRACE ? 1u : (unsigned)n_obs;
    const float    a     = (float)(1.0 / (double)count);  // T(1.0 / nObservations)
    for (int i = 0; i < n; ++i) {
        const float m = std::fmaf(a, stat[i], 0.f);  // activationMean_.setToZero(); add(activationSum_, a)
        if (mean)
            mean[i] = m;
        if (variance) {  // add(mean), elementwiseMultiplication(itself), scale(-1), add(sumOfSquares, a), scale(1), addConstantElementwise(0)
            float v = m;
            v       = v * v;
            v       = -1.0f * v;
            v       = std::fmaf(a, stat[Pn + i], v);
            v       = 1.0f * v;
            v       = v + 0.0f;
            variance[i] = v;
        }
    }
    return AMX_OK;
}

int amx_nntrain_get_layer_input(amx_nntrain* h, int layer, int T, float* X) {
    AMX_REQUIRE(h && X, AMX_ERR_INVALID, "amx_nntrain_get_layer_input: NULL argument");
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "amx_nntrain_get_layer_input: the handle was created without a context");
    AMX_REQUIRE(layer >= 0 && layer < h->L, AMX_ERR_INVALID, "amx_nntrain_get_layer_input: layer = %d (0..%d)", layer, h->L - 1);
    const int K = h->in[layer], Kp = h->Pin[layer];
    AMX_REQUIRE(T >= 0 && (size_t)T * Kp <= h->d_x[layer].capacity(), AMX_ERR_INVALID, "amx_nntrain_get_layer_input: T = %d is more than the last pass held", T);
    AMX_HIP(hipSetDevice(h->ctx->device));
    AMX_HIP(hipStreamSynchronize(h->ctx->stream));
    if (T > 0)
        AMX_TRY(copy_rows(X, (size_t)K * sizeof(float), h->d_x[layer].get(), (size_t)Kp * sizeof(float), (size_t)K * sizeof(float), (size_t)T));
    return AMX_OK;
}

}  // extern "C"
