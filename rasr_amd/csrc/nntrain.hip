// nntrain.hip -- NN training statistics: Nn::FeedForwardTrainer in batch mode (forward, cross-entropy error signal, error
// backpropagation, per-layer gradient sums), Nn::MeanAndVarianceTrainer's feature sums, class counts, and the Nn::Statistics file.
// include/amx.h ("NN training statistics") states the arithmetic with the reference's file:line; this file holds the handle, the
// kernels and the host side (files, prior, mean and deviation).
//
// One call = one mini-batch of at most AMX_NNTRAIN_MAX_FRAMES frames.  Every matrix of a call is padded to multiples of 128 in both
// directions (frames and units), so that the three GEMM kinds need no bounds checks; what makes the padding harmless:
//   * padded weight rows / columns and padded bias entries are zero;
//   * the error signal of a padded frame, of a dropped frame (disregarded class) and of a padded unit is exactly zero: the error
//     kernel writes those zeros, and W^T 0 times any finite derivative stays zero.  The inputs of a dropped frame are packed as zeros,
//     so its activations are finite whatever its features hold.
// Kernels and their bounds ("NN training statistics"):
//   forward      gemm_f32_kernel (ffnn_f32.hpp), f32 MFMA bound;  softmax: the three top_* kernels of the forward node
//   error        nntrain_error_kernel: one pass over the [T x n_out] softmax, HBM bound (one read, one write)
//   E W          nntrain_gemm_bwd_kernel: the forward kernel's loop on the transposed weight image, derivative and clip in the epilogue
//   X E^T        nntrain_gemm_tn_kernel: both operands have t as the slow axis, one workgroup per (tile, frame chunk), f32 MFMA bound;
//                nntrain_reduce_kernel adds the chunk partials in ascending order and widens into the caller's buffer
//                (nntrain_reduce_step_kernel: the same total into the f32 statistic of mini-batch training, nnstep.hip)
//   column sums  nntrain_colsum_kernel: bias gradient and the weighted feature sums, one ascending-t chain per column and chunk
#include "nntrain.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace amx {

constexpr int NT_CHUNK = AMX_NNTRAIN_CHUNK;  // frames per partial sum: a constant of the library, so that the order of a sum depends on the call alone
constexpr int NT_PAD   = 128;                // every dimension of a call's matrices is padded to the GEMM tile edge

// ---- labels: class -> network output, the frame weight, and the check that no label becomes an address
// label[t] = output index, -1 for a dropped frame (disregarded class) and for the padding; w[t] = (f32)(classWeight (f32) * alignment
// weight (f64)) (Nn/BufferedAlignedFeatureProcessor.cc:209-221).  *bad = the first frame whose label is out of range.
__global__ __launch_bounds__(256) void nntrain_label_kernel(const uint32_t* __restrict__ emission, const double* __restrict__ weight,
                                                           const int* __restrict__ class_to_output, const float* __restrict__ class_weight, int T,
                                                           int Tpad, int n_classes, int n_outputs, int* __restrict__ label, float* __restrict__ w,
                                                           unsigned* __restrict__ bad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Tpad)
        return;
    int   o  = -1;
    float wt = 0.f;
    if (t < T) {
        if (emission) {
            const uint32_t e = emission[t];
            if (e >= (uint32_t)n_classes)
                atomicMin(bad, (unsigned)t);
            else {
                const int m = class_to_output ? class_to_output[e] : (int)e;
                if (m >= n_outputs)
                    atomicMin(bad, (unsigned)t);
                else
                    o = m;  // m < 0: a disregarded class, the frame never enters the batch
            }
        }
        else
            o = 0;  // mean and variance alone: every frame counts, no class is looked up
        if (o >= 0) {
            wt = (class_weight && emission) ? class_weight[o] : 1.f;
            if (weight)
                wt = (float)((double)wt * weight[t]);
        }
    }
    label[t] = o;
    w[t]     = wt;
}

// the network input of the training pass: the preprocessed features, zeros for a dropped frame
struct TrainSrc {
    FeatSrc    f;
    const int* label;
    __device__ __forceinline__ float operator()(int t, int k) const { return label[t] >= 0 ? f(t, k) : 0.f; }
};

// ---- criterion: one workgroup per frame over the softmax row p [n]
// argMax (Math/FastMatrix.hh:899-909): first strictly greater value from Core::Type<f32>::min; err[t] = (argMax != label);
// obj[t] = -(logf(p[label])) * w; E[t] = (p + (-1 at the label)) * w, clipped when the top layer is not the lowest one.  Rows of
// dropped and padded frames and the padded units of every row are written as zeros.
__global__ __launch_bounds__(256) void nntrain_error_kernel(const float* __restrict__ p, int n, int T, const int* __restrict__ label,
                                                           const float* __restrict__ w, float* __restrict__ E, int ldE, float clip, int do_clip,
                                                           unsigned* __restrict__ err, float* __restrict__ obj) {
    __shared__ float    s_val[4];
    __shared__ unsigned s_idx[4];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int o = t < T ? label[t] : -1;
    float*    e = E ? E + (size_t)t * ldE : nullptr;
    if (o < 0) {  // uniform over the workgroup
        if (e)
            for (int i = tid; i < ldE; i += 256)
                e[i] = 0.f;
        if (tid == 0) {
            err[t] = 0;
            obj[t] = 0.f;
        }
        return;
    }
    const float* row = p + (size_t)t * n;
    const float  wt  = w[t];
    float        best = -FLT_MAX;
    unsigned     bi   = 0xffffffffu;
    for (int i = tid; i < n; i += 256) {
        const float v = row[i];
        if (v > best) {
            best = v;
            bi   = (unsigned)i;
        }
        if (e) {
            float d = v;
            if (i == o)
                d = d + -1.f;  // addKroneckerDelta(alignment, -1.0)
            d = d * wt;        // multiplyColumnsByScalars(weights): scal
            if (do_clip)       // FastMatrix::clip: std::min / std::max, which keep a NaN
                d = d > 0.f ? (clip < d ? clip : d) : (d < -clip ? -clip : d);
            e[i] = d;
        }
    }
    if (e)
        for (int i = n + tid; i < ldE; i += 256)
            e[i] = 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float    ob = __shfl_xor(best, off, 64);
        const unsigned oi = (unsigned)__shfl_xor((int)bi, off, 64);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi   = oi;
        }
    }
    if ((tid & 63) == 0) {
        s_val[tid >> 6] = best;
        s_idx[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k)
            if (s_val[k] > best || (s_val[k] == best && s_idx[k] < bi)) {
                best = s_val[k];
                bi   = s_idx[k];
            }
        const unsigned arg = bi == 0xffffffffu ? 0u : bi;
        err[t]             = arg != (unsigned)o ? 1u : 0u;
        const float l      = logf(row[o]);
        obj[t]             = -l * wt;
    }
}

// ---- class counts and the tail of the buffer: ONE workgroup, so that the order of the f64 sums is fixed by T alone
// tail[0] += observations (frames that entered the batch), tail[2] += sum |w| (weights->asum()); with base statistics tail[1] +=
// classification errors, tail[3] += objective.  Class counts: one f64 atomic per distinct label of a wave (whole numbers: exact and
// order-free below 2^53), as best_state_reduce_kernel aggregates its state counts.
__global__ __launch_bounds__(256) void nntrain_tail_kernel(int T, const int* __restrict__ label, const float* __restrict__ w,
                                                          const unsigned* __restrict__ err, const float* __restrict__ obj, double* __restrict__ counts,
                                                          double* __restrict__ tail) {
    __shared__ double s_red[4][256];
    const int tid = threadIdx.x, lane = tid & 63;
    double    n_obs = 0.0, n_err = 0.0, sum_w = 0.0, sum_obj = 0.0;
    for (int base = 0; base < T; base += 256) {  // uniform trip count: every lane takes part in the ballots
        const int t  = base + tid;
        const int my = t < T ? label[t] : -1;
        if (my >= 0) {
            n_obs += 1.0;
            sum_w += (double)fabsf(w[t]);
            if (err) {
                n_err += (double)err[t];
                sum_obj += (double)obj[t];
            }
        }
        if (counts) {
            unsigned long long todo = __ballot(my >= 0);
            while (todo) {
                const int                leader = __ffsll((long long)todo) - 1;
                const int                key    = __shfl(my, leader, 64);
                const unsigned long long same   = __ballot(my == key) & todo;
                if (lane == leader)
                    atomicAdd(&counts[key], (double)__popcll(same));
                todo &= ~same;
            }
        }
    }
    s_red[0][tid] = n_obs;
    s_red[1][tid] = n_err;
    s_red[2][tid] = sum_w;
    s_red[3][tid] = sum_obj;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half)
            for (int q = 0; q < 4; ++q)
                s_red[q][tid] += s_red[q][tid + half];
        __syncthreads();
    }
    if (tid == 0) {
        tail[0] += s_red[0][0];
        tail[2] += s_red[2][0];
        if (err) {
            tail[1] += s_red[1][0];
            tail[3] += s_red[3][0];
        }
    }
}

// ---- E W: out[t][k] = (sum_n WT[k][n] E[t][n]) * f'(Y[t][k]), clipped.  The loop of gemm_f32_kernel (both operands K-contiguous,
// here K = the layer's outputs) on the transposed weight image; every dimension is padded, nothing is bounds-checked.
// WT [Kdim_pad x Npad], E [Tpad x Npad], Y and out [Tpad x ldo].
template<int ACT>
__global__ __launch_bounds__(256) void nntrain_gemm_bwd_kernel(const float* __restrict__ WT, const float* __restrict__ E, const float* __restrict__ Y,
                                                              float* __restrict__ out, int Npad, int ldo, int n_tiles_n, float clip, int do_clip) {
    __shared__ float sW[BN * FLD];
    __shared__ float sX[BT * FLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wt = wave & 1;
    const int tile_t = blockIdx.x / n_tiles_n, tile_n = blockIdx.x - tile_t * n_tiles_n;
    const int n0 = tile_n * BN, t0 = tile_t * BT;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                acc[i][j][r] = 0.f;

    for (int k0 = 0; k0 < Npad; k0 += FK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int    idx = i * 256 + tid;
            const int    row = idx >> 3, c4 = (idx & 7) * 4;
            const float4 a   = *(const float4*)(WT + (size_t)(n0 + row) * Npad + k0 + c4);
            const float4 x   = *(const float4*)(E + (size_t)(t0 + row) * Npad + k0 + c4);
            float*       dw  = sW + row * FLD + c4;
            float*       dx  = sX + row * FLD + c4;
            dw[0] = a.x; dw[1] = a.y; dw[2] = a.z; dw[3] = a.w;
            dx[0] = x.x; dx[1] = x.y; dx[2] = x.z; dx[3] = x.w;
        }
        __syncthreads();
        const int frow = lane & 31, fk = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < FK / 2; ++kk) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                a[i] = sW[(wn * 64 + i * 32 + frow) * FLD + 2 * kk + fk];
#pragma unroll
            for (int j = 0; j < 2; ++j)
                b[j] = sX[(wt * 64 + j * 32 + frow) * FLD + 2 * kk + fk];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int t = t0 + wt * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int    n  = n0 + wn * 64 + i * 32 + 8 * g + 4 * (lane >> 5);
                const float4 y4 = *(const float4*)(Y + (size_t)t * ldo + n);
                const float  y[4] = {y4.x, y4.y, y4.z, y4.w};
                float        r[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = acc[i][j][g * 4 + e];
                    if (ACT == AMX_ACT_SIGMOID)  // elem *= X * (1.0 - X): a double product narrowed once
                        v = (float)((double)v * ((double)y[e] * (1.0 - (double)y[e])));
                    else if (ACT == AMX_ACT_TANH)  // elem *= 1.0 - X * X: the square is an f32 product
                        v = (float)((double)v * (1.0 - (double)(y[e] * y[e])));
                    else if (ACT == AMX_ACT_RELU) {
                        if (y[e] <= 0.f)
                            v = 0.f;
                    }
                    if (do_clip)
                        v = v > 0.f ? (clip < v ? clip : v) : (v < -clip ? -clip : v);
                    r[e] = v;
                }
                *(float4*)(out + (size_t)t * ldo + n) = make_float4(r[0], r[1], r[2], r[3]);
            }
        }
}

// ---- X E^T: part[c][k][n] = sum over the frames t of chunk c of X[t][k] E[t][n], ascending t.  Both operands have t as the slow axis:
// a tile row is contiguous in memory, the LDS fill is coalesced float4 with no transpose, and the MFMA operands are read along a row
// (lanes 0..31) of two neighbouring frames (lanes 32..63; TN_LD = 128 + 32 puts them on the other half of the banks).
// X [Tpad x Kpad], E [Tpad x Npad], part [n_chunks x Kpad x Npad]; grid (tiles, chunks).
constexpr int TN_TS = 32;         // frames per LDS stage
constexpr int TN_LD = 128 + 32;   // LDS row (floats)

__global__ __launch_bounds__(256) void nntrain_gemm_tn_kernel(const float* __restrict__ X, const float* __restrict__ E, float* __restrict__ part, int Kpad,
                                                             int Npad, int Tpad, int n_tiles_n) {
    __shared__ float sX[TN_TS * TN_LD];
    __shared__ float sE[TN_TS * TN_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave >> 1, wn = wave & 1;
    const int tile_k = blockIdx.x / n_tiles_n, tile_n = blockIdx.x - tile_k * n_tiles_n;
    const int k0 = tile_k * 128, n0 = tile_n * 128;
    const int c  = blockIdx.y;
    const int t_begin = c * NT_CHUNK, t_end = min(Tpad, t_begin + NT_CHUNK);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                acc[i][j][r] = 0.f;

    for (int t0 = t_begin; t0 < t_end; t0 += TN_TS) {  // Tpad is a multiple of 128: whole stages
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = i * 256 + tid;
            const int row = idx >> 5, c4 = (idx & 31) * 4;
            *(float4*)(sX + row * TN_LD + c4) = *(const float4*)(X + (size_t)(t0 + row) * Kpad + k0 + c4);
            *(float4*)(sE + row * TN_LD + c4) = *(const float4*)(E + (size_t)(t0 + row) * Npad + n0 + c4);
        }
        __syncthreads();
        const int fcol = lane & 31, ft = lane >> 5;
#pragma unroll
        for (int tt = 0; tt < TN_TS / 2; ++tt) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                a[i] = sX[(2 * tt + ft) * TN_LD + wk * 64 + i * 32 + fcol];
#pragma unroll
            for (int j = 0; j < 2; ++j)
                b[j] = sE[(2 * tt + ft) * TN_LD + wn * 64 + j * 32 + fcol];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    float* const dst = part + (size_t)c * Kpad * Npad;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = k0 + wk * 64 + i * 32 + 8 * g + 4 * (lane >> 5) + e;
                    dst[(size_t)k * Npad + n] = acc[i][j][g * 4 + e];
                }
        }
}

// acc[r * cols + c] += (f64)(((0 + part[0]) + part[1]) + ...), the chunk partials in ascending order in f32; part [n_chunks][.. x ld]
__global__ __launch_bounds__(256) void nntrain_reduce_kernel(const float* __restrict__ part, int n_chunks, size_t chunk_stride, int rows, int cols, int ld,
                                                            double* __restrict__ acc) {
    const long long total = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i - (long long)r * cols);
        float     s = 0.f;
        for (int q = 0; q < n_chunks; ++q)
            s = s + part[(size_t)q * chunk_stride + (size_t)r * ld + c];
        acc[i] += (double)s;
    }
}

// The same total for mini-batch training (nnstep.hip): added to the group's f32 statistic G with ONE f32 add (a group's first call
// adds to zero), then the regulariser's axpy on the sum (Nn/Regularizer.cc:97-119,152-165,215-234), one fused multiply-add per
// element as saxpy computes it.  W has G's indexing (the transposed weight image for a layer's gradient, the bias for its bias
// gradient); Wc the centre.  factor = the group's running observations, this call's included: both counts are read from the device.
// c == 0: no regulariser for this block.
__global__ __launch_bounds__(256) void nntrain_reduce_step_kernel(const float* __restrict__ part, int n_chunks, size_t chunk_stride, int rows, int cols, int ld,
                                                                 float* __restrict__ G, int ldg, int reset, const float* __restrict__ W,
                                                                 const float* __restrict__ Wc, int regularizer, float c,
                                                                 const double* __restrict__ group_tail, const double* __restrict__ call_tail) {
    const long long total = (long long)rows * cols;
    float           cf    = 0.f;
    if (c > 0.f && regularizer != AMX_NNSTEP_REG_NONE) {
        const float factor = (float)(unsigned)(group_tail[0] + call_tail[0]);  // T(statistics.nObservations()): a u32 as f32
        cf                 = c * factor;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int    r = (int)(i / cols), col = (int)(i - (long long)r * cols);
        const size_t at = (size_t)r * ldg + col;
        float        s = 0.f;
        for (int q = 0; q < n_chunks; ++q)
            s = s + part[(size_t)q * chunk_stride + (size_t)r * ld + col];
        float v = n_chunks > 0 ? (reset ? 0.f : G[at]) + s : G[at];  // n_chunks == 0: the statistic as it is (amx_nntrain_estimate)
        if (c > 0.f) {
            const float w = W[at];
            if (regularizer == AMX_NNSTEP_REG_L2)
                v = fmaf(cf, w, v);
            else if (regularizer == AMX_NNSTEP_REG_L1)  // sign (Math/CudaMatrixKernels.cu:897-902): in == 0 ? 0 : copysignf(1.0, in)
                v = fmaf(cf, w == 0.f ? 0.f : copysignf(1.f, w), v);
            else if (regularizer == AMX_NNSTEP_REG_CENTERED_L2) {
                v = fmaf(cf, w, v);
                v = fmaf(-cf, Wc[at], v);
            }
        }
        G[at] = v;
    }
}

// ---- column sums over the frames of one chunk, one ascending-t f32 chain per column: part[c][col]
// MODE 0: src as it is (bias gradient: rows of dropped frames are zero); MODE 1: x * w; MODE 2: (x * x) * w, each product rounded to
// f32, frames that did not enter the batch skipped (Nn/NeuralNetworkTrainer.cc:465-493)
template<int MODE>
__global__ __launch_bounds__(256) void nntrain_colsum_kernel(const float* __restrict__ src, int ld, int T, int ncols, const int* __restrict__ label,
                                                            const float* __restrict__ w, float* __restrict__ part) {
    const int col = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (col >= ncols)
        return;
    const int t1 = min(T, (c + 1) * NT_CHUNK);
    float     s  = 0.f;
    for (int t = c * NT_CHUNK; t < t1; ++t) {
        if (MODE != 0 && label[t] < 0)
            continue;
        float v = src[(size_t)t * ld + col];
        if (MODE == 1)
            v = v * w[t];
        if (MODE == 2) {
            v = v * v;
            v = v * w[t];
        }
        s = s + v;
    }
    part[(size_t)c * ncols + col] = s;
}

inline int pad128(int n) {
    return (n + NT_PAD - 1) / NT_PAD * NT_PAD;
}

}  // namespace amx

// ------------------------------------------------------------------------------------ handle

namespace {

const char* act_name(int a) {
    switch (a) {
        case AMX_ACT_NONE: return "linear";
        case AMX_ACT_RELU: return "rectified";
        case AMX_ACT_SIGMOID: return "sigmoid";
        case AMX_ACT_TANH: return "tanh";
        case AMX_ACT_ELU: return "elu";
    }
    return "unknown";
}

void make_layout(amx_nntrain* h) {
    amx_nntrain_layout_info& y = h->lay;
    memset(&y, 0, sizeof y);
    y.n_layers    = h->L;
    y.feature_dim = h->feature_dim;
    y.n_outputs   = h->n_outputs;
    long off      = 0;
    for (int l = 0; l < AMX_NNTRAIN_MAX_LAYERS; ++l)
        y.gradient_weights[l] = y.gradient_bias[l] = -1;
    for (int l = 0; l < h->L; ++l) {
        y.in_dim[l]  = h->in[l];
        y.out_dim[l] = h->out[l];
        if (h->mask & AMX_NNSTAT_GRADIENT) {
            y.gradient_weights[l] = off;
            off += (long)h->in[l] * h->out[l];
            y.gradient_bias[l] = off;
            off += h->out[l];
        }
    }
    y.feature_sum = y.feature_square_sum = y.class_counts = -1;
    if (h->mask & AMX_NNSTAT_MEAN_AND_VARIANCE) {
        y.feature_sum = off;
        off += h->feature_dim;
        y.feature_square_sum = off;
        off += h->feature_dim;
    }
    if (h->mask & AMX_NNSTAT_CLASS_COUNTS) {
        y.class_counts = off;
        off += h->n_outputs;
    }
    y.tail = off;
    off += 4;
    y.size = off;
}

int check_mapping(const int* c2o, int n_classes, int n_outputs) {
    AMX_REQUIRE(n_classes > 0, AMX_ERR_INVALID, "amx_nntrain_create: class_to_output needs n_classes > 0");
    std::vector<char> seen((size_t)n_outputs, 0);
    for (int e = 0; e < n_classes; ++e) {
        const int o = c2o[e];
        AMX_REQUIRE(o >= -1 && o < n_outputs, AMX_ERR_INVALID, "amx_nntrain_create: class_to_output[%d] = %d is no output of the network (%d outputs)", e,
                    o, n_outputs);
        if (o >= 0) {
            AMX_REQUIRE(!seen[o], AMX_ERR_INVALID, "amx_nntrain_create: no one-to-one correspondence between network outputs and classes (output %d)", o);
            seen[o] = 1;
        }
    }
    return AMX_OK;
}

template<class T>
int upload_padded(amx::DevBuf<T>& d, const std::vector<T>& host) {
    return d.upload(host.data(), host.size());
}

}  // namespace

extern "C" {

void amx_nntrain_default_cfg(amx_nntrain_cfg* cfg) {
    if (!cfg)
        return;
    memset(cfg, 0, sizeof *cfg);
    cfg->statistics        = AMX_NNSTAT_BASE | AMX_NNSTAT_GRADIENT;
    cfg->error_signal_clip = FLT_MAX;
}

void amx_nntrain_destroy(amx_nntrain* h) {
    delete h;
}

int amx_nntrain_create(amx_ctx* ctx, const amx_ffnn_model* m, const amx_ffnn_layers* ext, const amx_nntrain_cfg* cfg, amx_nntrain** out) {
    AMX_REQUIRE(cfg && out, AMX_ERR_INVALID, "amx_nntrain_create: NULL argument");
    *out = nullptr;
    AMX_REQUIRE(cfg->statistics > 0 && cfg->statistics < 16, AMX_ERR_INVALID, "amx_nntrain_create: statistics = %d is no mask of the four statistics flags", cfg->statistics);
    AMX_REQUIRE(cfg->error_signal_clip > 0.f, AMX_ERR_INVALID, "amx_nntrain_create: error_signal_clip must be positive");
    std::unique_ptr<amx_nntrain> h(new amx_nntrain);
    h->ctx  = ctx;
    h->mask = cfg->statistics;
    h->clip = cfg->error_signal_clip;
    const int*  c2o       = nullptr;
    if (!m) {
        AMX_REQUIRE(!(h->mask & (AMX_NNSTAT_BASE | AMX_NNSTAT_GRADIENT)), AMX_ERR_INVALID,
                    "amx_nntrain_create: base statistics and the gradient need a network (model is NULL)");
        AMX_REQUIRE(!ext || ext->n_pre == 0, AMX_ERR_INVALID, "amx_nntrain_create: preprocessing layers without a network");
        if (h->mask & AMX_NNSTAT_MEAN_AND_VARIANCE)
            AMX_REQUIRE(cfg->feature_dim > 0, AMX_ERR_INVALID, "amx_nntrain_create: feature_dim must be positive");
        if (h->mask & AMX_NNSTAT_CLASS_COUNTS)
            AMX_REQUIRE(cfg->n_outputs > 0, AMX_ERR_INVALID, "amx_nntrain_create: n_outputs must be positive");
        h->feature_dim = std::max(cfg->feature_dim, 0);
        h->n_outputs   = std::max(cfg->n_outputs, 0);
        c2o            = cfg->class_to_output;
        h->n_classes   = c2o ? cfg->n_classes : h->n_outputs;
    }
    else {
        AMX_REQUIRE(m->n_layers >= 1 && m->n_layers <= AMX_NNTRAIN_MAX_LAYERS && m->in_dim && m->out_dim && m->W && m->bias && m->activation, AMX_ERR_INVALID,
                    "amx_nntrain_create: the model needs 1..%d layers with dimensions, weights, biases and activations", AMX_NNTRAIN_MAX_LAYERS);
        AMX_REQUIRE(m->precision == AMX_PREC_FP32, AMX_ERR_UNSUPPORTED,
                    "amx_nntrain_create: precision %d: the training pass computes in AMX_PREC_FP32 only", m->precision);
        h->L = m->n_layers;
        for (int l = 0; l < h->L; ++l) {
            AMX_REQUIRE(m->in_dim[l] > 0 && m->out_dim[l] > 0 && m->W[l] && m->bias[l], AMX_ERR_INVALID, "amx_nntrain_create: layer %d: bad dimensions or NULL parameters", l);
            AMX_REQUIRE(l == 0 || m->in_dim[l] == m->out_dim[l - 1], AMX_ERR_INVALID, "amx_nntrain_create: layer %d: input dimension %d does not follow layer %d's %d outputs",
                        l, m->in_dim[l], l - 1, m->out_dim[l - 1]);
            const int a = m->activation[l];
            AMX_REQUIRE(a >= AMX_ACT_NONE && a <= AMX_ACT_ELU, AMX_ERR_INVALID, "amx_nntrain_create: layer %d: unknown activation %d", l, a);
            AMX_REQUIRE(a != AMX_ACT_ELU, AMX_ERR_UNSUPPORTED, "amx_nntrain_create: layer %d: the derivative of the %s layer is not implemented", l, act_name(a));
            AMX_REQUIRE(!(ext && ext->maxout_groups && ext->maxout_groups[l] > 0), AMX_ERR_UNSUPPORTED,
                        "amx_nntrain_create: layer %d: backpropagation through a maxout is not implemented", l);
            h->in.push_back(m->in_dim[l]);
            h->out.push_back(m->out_dim[l]);
            h->act.push_back(a);
            h->Pin.push_back(amx::pad128(m->in_dim[l]));
            h->Pout.push_back(amx::pad128(m->out_dim[l]));
        }
        AMX_REQUIRE(m->activation[h->L - 1] == AMX_ACT_NONE, AMX_ERR_INVALID,
                    "amx_nntrain_create: layer %d: the output layer must be linear (the softmax is on top)", h->L - 1);
        h->feature_dim = h->in[0];
        h->n_outputs   = h->out[h->L - 1];
        c2o            = m->class_to_output;
        h->n_classes   = c2o ? m->n_classes : h->n_outputs;
        if (ext) {
            AMX_REQUIRE(ext->n_pre >= 0 && ext->n_pre <= AMX_NN_MAX_PRE && (ext->n_pre == 0 || ext->pre_type), AMX_ERR_INVALID,
                        "amx_nntrain_create: n_pre = %d (0..%d)", ext->n_pre, AMX_NN_MAX_PRE);
            for (int i = 0; i < ext->n_pre; ++i) {
                const int ty = ext->pre_type[i];
                AMX_REQUIRE(ty == AMX_NN_PRE_LOGARITHM || ty == AMX_NN_PRE_MEAN_AND_VARIANCE, AMX_ERR_INVALID, "amx_nntrain_create: preprocessing layer %d: unknown type %d", i, ty);
                AMX_REQUIRE(ty != AMX_NN_PRE_MEAN_AND_VARIANCE || (ext->pre_mean && ext->pre_stddev && ext->pre_mean[i] && ext->pre_stddev[i]), AMX_ERR_INVALID,
                            "amx_nntrain_create: preprocessing layer %d: mean-and-variance-normalization needs a mean and a standard deviation", i);
            }
        }
    }
    if (c2o)
        AMX_TRY(check_mapping(c2o, h->n_classes, h->n_outputs));
    if (c2o)
        h->class_to_output.assign(c2o, c2o + h->n_classes);
    h->class_weights.assign((size_t)h->n_outputs, 1.f);
    if (cfg->class_weights)
        h->class_weights.assign(cfg->class_weights, cfg->class_weights + h->n_outputs);
    make_layout(h.get());
    if (!ctx && m)  // amx_nntrain_get_parameters on a host-only handle
        for (int l = 0; l < h->L; ++l) {
            h->host_W.emplace_back(m->W[l], m->W[l] + (size_t)h->in[l] * h->out[l]);
            h->host_bias.emplace_back(m->bias[l], m->bias[l] + h->out[l]);
        }

    if (ctx) {
        AMX_HIP(hipSetDevice(ctx->device));
        if (c2o)
            AMX_TRY(h->d_c2o.upload(h->class_to_output.data(), h->class_to_output.size()));
        AMX_TRY(h->d_cw.upload(h->class_weights.data(), h->class_weights.size()));
        AMX_TRY(h->d_bad.reserve(1));
        AMX_TRY(h->h_bad.reserve(1));
        h->d_W  = std::vector<amx::DevBuf<float>>(h->L);
        h->d_WT = std::vector<amx::DevBuf<float>>(h->L);
        h->d_bias = std::vector<amx::DevBuf<float>>(h->L);
        h->d_x  = std::vector<amx::DevBuf<float>>(h->L);
        h->d_E  = std::vector<amx::DevBuf<float>>(h->L);
        for (int l = 0; l < h->L; ++l) {
            const int          K = h->in[l], N = h->out[l], Kp = h->Pin[l], Np = h->Pout[l];
            std::vector<float> W((size_t)Np * Kp, 0.f), WT((size_t)Kp * Np, 0.f), b((size_t)Np, 0.f);
            for (int n = 0; n < N; ++n) {
                for (int k = 0; k < K; ++k) {
                    const float v            = m->W[l][(size_t)n * K + k];
                    W[(size_t)n * Kp + k]  = v;
                    WT[(size_t)k * Np + n] = v;
                }
                b[n] = m->bias[l][n];
            }
            AMX_TRY(upload_padded(h->d_W[l], W));
            AMX_TRY(upload_padded(h->d_WT[l], WT));
            AMX_TRY(upload_padded(h->d_bias[l], b));
        }
        if (m && ext && ext->n_pre > 0) {
            h->d_pre_mean = std::vector<amx::DevBuf<float>>(ext->n_pre);
            h->d_pre_rstd = std::vector<amx::DevBuf<float>>(ext->n_pre);
            h->pre.n      = ext->n_pre;
            for (int i = 0; i < ext->n_pre; ++i) {
                h->pre.type[i] = ext->pre_type[i];
                h->pre.mean[i] = h->pre.rstd[i] = nullptr;
                if (ext->pre_type[i] != AMX_NN_PRE_MEAN_AND_VARIANCE)
                    continue;
                std::vector<float> r((size_t)h->in[0]);
                for (int k = 0; k < h->in[0]; ++k)
                    r[k] = 1.0f / ext->pre_stddev[i][k];  // divideRowsByScalars: scal((f32)1 / s)
                AMX_TRY(h->d_pre_mean[i].upload(ext->pre_mean[i], (size_t)h->in[0]));
                AMX_TRY(h->d_pre_rstd[i].upload(r.data(), r.size()));
                h->pre.mean[i] = h->d_pre_mean[i].get();
                h->pre.rstd[i] = h->d_pre_rstd[i].get();
            }
        }
    }
    *out = h.release();
    return AMX_OK;
}

long amx_nntrain_accumulator_size(const amx_nntrain* h) {
    return h ? h->lay.size : 0;
}

int amx_nntrain_layout(const amx_nntrain* h, amx_nntrain_layout_info* info) {
    AMX_REQUIRE(h && info, AMX_ERR_INVALID, "amx_nntrain_layout: NULL argument");
    *info = h->lay;
    return AMX_OK;
}

}  // extern "C"

namespace amx {

// ---- the launches of a pass that the segment-wise trainer (nnseq.hip) runs on its own rows: nntrain_pass goes through these too
void nntrain_launch_forward(amx_nntrain* h, int Tpad, int T, hipStream_t st) {
    const int L = h->L, n_out = h->n_outputs;
    for (int l = 0; l < L; ++l) {
        const int    ntn = h->Pout[l] / amx::BN, ntt = Tpad / amx::BT;
        const float *W = h->d_W[l].get(), *x = h->d_x[l].get(), *b = h->d_bias[l].get();
        const dim3   grid(ntn * ntt), block(256);
        if (l == L - 1)
            hipLaunchKernelGGL((amx::gemm_f32_kernel<AMX_ACT_NONE, true>), grid, block, 0, st, W, x, b, h->d_top.get(), h->Pin[l], h->Pin[l], n_out, n_out, T, ntn);
        else {
            float* o = h->d_x[l + 1].get();
            switch (h->act[l]) {
                case AMX_ACT_RELU:
                    hipLaunchKernelGGL((amx::gemm_f32_kernel<AMX_ACT_RELU, false>), grid, block, 0, st, W, x, b, o, h->Pin[l], h->Pin[l], h->Pout[l], h->out[l], T, ntn);
                    break;
                case AMX_ACT_SIGMOID:
                    hipLaunchKernelGGL((amx::gemm_f32_kernel<AMX_ACT_SIGMOID, false>), grid, block, 0, st, W, x, b, o, h->Pin[l], h->Pin[l], h->Pout[l], h->out[l], T, ntn);
                    break;
                case AMX_ACT_TANH:
                    hipLaunchKernelGGL((amx::gemm_f32_kernel<AMX_ACT_TANH, false>), grid, block, 0, st, W, x, b, o, h->Pin[l], h->Pin[l], h->Pout[l], h->out[l], T, ntn);
                    break;
                default:
                    hipLaunchKernelGGL((amx::gemm_f32_kernel<AMX_ACT_NONE, false>), grid, block, 0, st, W, x, b, o, h->Pin[l], h->Pin[l], h->Pout[l], h->out[l], T, ntn);
            }
        }
    }
}

void nntrain_launch_softmax(amx_nntrain* h, int T, hipStream_t st) {
    const int n_out = h->n_outputs;
    float* const    row_max = h->d_rowstat.get();
    float* const    row_sum = row_max + T;
    const long long total   = (long long)T * n_out;
    hipLaunchKernelGGL(amx::top_negexp_kernel, dim3(T), dim3(256), 0, st, h->d_top.get(), n_out, row_max);
    hipLaunchKernelGGL(amx::top_rowsum_kernel, dim3((T + 63) / 64), dim3(64), 0, st, (const float*)h->d_top.get(), T, n_out, row_sum);
    hipLaunchKernelGGL(amx::top_finish_kernel, dim3((int)std::min<long long>(16384, (total + 255) / 256)), dim3(256), 0, st, h->d_top.get(), total, n_out,
                       (const float*)row_sum);
}

void nntrain_launch_backward(amx_nntrain* h, int Tpad, float clip, hipStream_t st) {
    const int L = h->L;
    for (int l = L - 1; l >= 1; --l) {
        const int    ntn = h->Pin[l] / amx::BN, ntt = Tpad / amx::BT, do_clip = (l - 1 > 0 && clip < FLT_MAX) ? 1 : 0;
        const float *WT = h->d_WT[l].get(), *E = h->d_E[l].get(), *Y = h->d_x[l].get();
        float*       o = h->d_E[l - 1].get();
        const dim3   grid(ntn * ntt), block(256);
        switch (h->act[l - 1]) {
            case AMX_ACT_RELU:
                hipLaunchKernelGGL(amx::nntrain_gemm_bwd_kernel<AMX_ACT_RELU>, grid, block, 0, st, WT, E, Y, o, h->Pout[l], h->Pin[l], ntn, clip, do_clip);
                break;
            case AMX_ACT_SIGMOID:
                hipLaunchKernelGGL(amx::nntrain_gemm_bwd_kernel<AMX_ACT_SIGMOID>, grid, block, 0, st, WT, E, Y, o, h->Pout[l], h->Pin[l], ntn, clip, do_clip);
                break;
            case AMX_ACT_TANH:
                hipLaunchKernelGGL(amx::nntrain_gemm_bwd_kernel<AMX_ACT_TANH>, grid, block, 0, st, WT, E, Y, o, h->Pout[l], h->Pin[l], ntn, clip, do_clip);
                break;
            default:
                hipLaunchKernelGGL(amx::nntrain_gemm_bwd_kernel<AMX_ACT_NONE>, grid, block, 0, st, WT, E, Y, o, h->Pout[l], h->Pin[l], ntn, clip, do_clip);
        }
    }
}

void nntrain_launch_gemm_tn(amx_nntrain* h, int l, int Tpad, int tn_chunks, hipStream_t st) {
    const int Kp = h->Pin[l], Np = h->Pout[l], ntn = Np / 128, ntk = Kp / 128;
    hipLaunchKernelGGL(amx::nntrain_gemm_tn_kernel, dim3(ntk * ntn, tn_chunks), dim3(256), 0, st, (const float*)h->d_x[l].get(),
                       (const float*)h->d_E[l].get(), h->d_part.get(), Kp, Np, Tpad, ntn);
}

void nntrain_launch_bias_sums(amx_nntrain* h, int l, int T, int n_chunks, hipStream_t st) {
    hipLaunchKernelGGL(amx::nntrain_colsum_kernel<0>, dim3((h->out[l] + 255) / 256, n_chunks), dim3(256), 0, st, (const float*)h->d_E[l].get(), h->Pout[l], T,
                       h->out[l], (const int*)h->d_label.get(), (const float*)h->d_w.get(), h->d_part.get());
}

int nntrain_pass(amx_nntrain* h, const float* feats, int ldf, int T, const uint32_t* emission, const double* weight, double* acc, const StepSink* sink,
                 const char* who) {
    AMX_REQUIRE(h && (acc || sink), AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(T >= 0 && T <= AMX_NNTRAIN_MAX_FRAMES, AMX_ERR_INVALID, "%s: T = %d (0..%d frames per call)", who, T, AMX_NNTRAIN_MAX_FRAMES);
    const bool want_net  = (h->mask & (AMX_NNSTAT_BASE | AMX_NNSTAT_GRADIENT)) != 0;
    const bool want_grad = (h->mask & AMX_NNSTAT_GRADIENT) != 0, want_base = (h->mask & AMX_NNSTAT_BASE) != 0;
    const bool want_mv   = (h->mask & AMX_NNSTAT_MEAN_AND_VARIANCE) != 0, want_cc = (h->mask & AMX_NNSTAT_CLASS_COUNTS) != 0;
    AMX_REQUIRE(emission || h->mask == AMX_NNSTAT_MEAN_AND_VARIANCE, AMX_ERR_INVALID, "%s: emission_dev is NULL", who);
    if (want_net || want_mv)
        AMX_REQUIRE(feats && ldf >= h->feature_dim, AMX_ERR_INVALID, "%s: feats_dev is NULL or feats_stride %d < %d", who, ldf, h->feature_dim);
    if (T == 0)
        return AMX_OK;
    ++h->workspace_epoch;
    hipStream_t st   = h->ctx->stream;
    const int   Tpad = amx::pad128(T), n_chunks = (T + amx::NT_CHUNK - 1) / amx::NT_CHUNK, L = h->L, n_out = h->n_outputs;
    const amx_nntrain_layout_info& y = h->lay;

    // workspace
    AMX_TRY(h->d_label.reserve(Tpad));
    AMX_TRY(h->d_w.reserve(Tpad));
    AMX_TRY(h->d_err.reserve(Tpad));
    AMX_TRY(h->d_obj.reserve(Tpad));
    size_t part = 0;
    if (want_mv)
        part = std::max(part, (size_t)n_chunks * h->feature_dim);
    if (want_net) {
        AMX_TRY(h->d_top.reserve((size_t)T * n_out));
        AMX_TRY(h->d_rowstat.reserve((size_t)2 * T));
        for (int l = 0; l < L; ++l) {
            AMX_TRY(h->d_x[l].reserve((size_t)Tpad * h->Pin[l]));
            if (want_grad) {
                AMX_TRY(h->d_E[l].reserve((size_t)Tpad * h->Pout[l]));
                part = std::max(part, (size_t)n_chunks * h->Pin[l] * h->Pout[l]);
            }
        }
    }
    AMX_TRY(h->d_part.reserve(std::max<size_t>(part, 1)));

    // 1. labels, checked before anything is written
    AMX_HIP(hipMemsetAsync(h->d_bad.get(), 0xff, 4, st));
    hipLaunchKernelGGL(amx::nntrain_label_kernel, dim3(Tpad / 256 + 1), dim3(256), 0, st, emission, weight, (const int*)(h->class_to_output.empty() ? nullptr : h->d_c2o.get()),
                       (const float*)h->d_cw.get(), T, Tpad, h->n_classes, n_out, h->d_label.get(), h->d_w.get(), h->d_bad.get());
    AMX_HIP(hipGetLastError());
    AMX_HIP(hipMemcpyAsync(h->h_bad.get(), h->d_bad.get(), 4, hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    const unsigned bad = *h->h_bad.get();
    AMX_REQUIRE(bad == 0xffffffffu, AMX_ERR_INVALID, "%s: frame %u: the label is out of range (%d classes, %d network outputs)", who, bad,
                h->n_classes, n_out);
    const int*   label = h->d_label.get();
    const float* w     = h->d_w.get();
    if (sink && sink->reset && sink->group_block)  // a new group starts from zero: only now, so that a refused call leaves everything as it was
        AMX_HIP(hipMemsetAsync(sink->group_block, 0, sink->group_bytes, st));

    // 2. feature sums on the raw features
    if (want_mv) {
        amx::ScopedKernelTimer timer(h->ctx, "nntrain_feature_sums");
        const int  D = h->feature_dim;
        const dim3 grid((D + 255) / 256, n_chunks);
        const int  rb = std::min(1024, (D + 255) / 256);
        hipLaunchKernelGGL(amx::nntrain_colsum_kernel<1>, grid, dim3(256), 0, st, feats, ldf, T, D, label, w, h->d_part.get());
        hipLaunchKernelGGL(amx::nntrain_reduce_kernel, dim3(rb), dim3(256), 0, st, (const float*)h->d_part.get(), n_chunks, (size_t)D, 1, D, D, acc + y.feature_sum);
        hipLaunchKernelGGL(amx::nntrain_colsum_kernel<2>, grid, dim3(256), 0, st, feats, ldf, T, D, label, w, h->d_part.get());
        hipLaunchKernelGGL(amx::nntrain_reduce_kernel, dim3(rb), dim3(256), 0, st, (const float*)h->d_part.get(), n_chunks, (size_t)D, 1, D, D,
                           acc + y.feature_square_sum);
        AMX_HIP(hipGetLastError());
    }

    if (want_net) {
        // 3. forward, every layer's input kept (the event pairs of amx_profile_* keep the GEMM launches apart from the rest)
        {
            amx::ScopedKernelTimer timer(h->ctx, "nntrain_pack");
            const amx::TrainSrc src{amx::FeatSrc{feats, ldf, h->pre}, label};
            const int           blocks = (int)std::min<long long>(4096, ((long long)Tpad * h->Pin[0] + 255) / 256);
            hipLaunchKernelGGL(amx::pack_input_f32<amx::TrainSrc>, dim3(blocks), dim3(256), 0, st, src, T, h->in[0], h->d_x[0].get(), h->Pin[0], Tpad);
        }
        {
            amx::ScopedKernelTimer timer(h->ctx, "nntrain_gemm_forward");
            amx::nntrain_launch_forward(h, Tpad, T, st);
            AMX_HIP(hipGetLastError());
        }
        {   // the softmax of the forward node on the dense [T x n_out] scores (= -activation)
            amx::ScopedKernelTimer timer(h->ctx, "nntrain_softmax");
            amx::nntrain_launch_softmax(h, T, st);
            AMX_HIP(hipGetLastError());
        }
        // 4. criterion and the top error signal
        {
            amx::ScopedKernelTimer timer(h->ctx, "nntrain_error");
            float* Etop = want_grad ? h->d_E[L - 1].get() : nullptr;
            hipLaunchKernelGGL(amx::nntrain_error_kernel, dim3(want_grad ? Tpad : T), dim3(256), 0, st, (const float*)h->d_top.get(), n_out, T, label, w, Etop,
                               h->Pout[L - 1], h->clip, (int)(L > 1 && h->clip < FLT_MAX), h->d_err.get(), h->d_obj.get());
            AMX_HIP(hipGetLastError());
        }
    }

    // 5. class counts and the tail
    hipLaunchKernelGGL(amx::nntrain_tail_kernel, dim3(1), dim3(256), 0, st, T, label, w, (const unsigned*)(want_base ? h->d_err.get() : nullptr),
                       (const float*)h->d_obj.get(), want_cc ? acc + y.class_counts : (double*)nullptr, sink ? sink->call_tail : acc + y.tail);
    AMX_HIP(hipGetLastError());

    if (want_grad) {
        // 6. error backpropagation: E_{l-1} = (W_l^T E_l) (.) f'(Y_{l-1}); E_{l-1} is clipped unless it is the lowest layer's
        {
            amx::ScopedKernelTimer timer(h->ctx, "nntrain_gemm_backward");
            amx::nntrain_launch_backward(h, Tpad, h->clip, st);
            AMX_HIP(hipGetLastError());
        }
        // 7. gradients: G_l += X_l E_l^T, g_l += the column sums of E_l
        {
            const int tn_chunks = (Tpad + amx::NT_CHUNK - 1) / amx::NT_CHUNK;  // == n_chunks: NT_CHUNK is a multiple of the padding
            for (int l = L - 1; l >= 0; --l) {
                const int Kp = h->Pin[l], Np = h->Pout[l];
                {
                    amx::ScopedKernelTimer timer(h->ctx, "nntrain_gemm_tn");
                    amx::nntrain_launch_gemm_tn(h, l, Tpad, tn_chunks, st);
                }
                amx::ScopedKernelTimer timer(h->ctx, "nntrain_gradient_sums");
                const long long total = (long long)h->in[l] * h->out[l];
                const dim3      rgrid((int)std::min<long long>(16384, (total + 255) / 256));
                if (sink)
                    hipLaunchKernelGGL(amx::nntrain_reduce_step_kernel, rgrid, dim3(256), 0, st, (const float*)h->d_part.get(), tn_chunks, (size_t)Kp * Np, h->in[l],
                                       h->out[l], Np, sink->G[l], Np, sink->reset, (const float*)h->d_WT[l].get(), sink->WTc[l], sink->regularizer, sink->c[l],
                                       sink->group_tail, (const double*)sink->call_tail);
                else
                    hipLaunchKernelGGL(amx::nntrain_reduce_kernel, rgrid, dim3(256), 0, st, (const float*)h->d_part.get(), tn_chunks, (size_t)Kp * Np, h->in[l], h->out[l],
                                       Np, acc + y.gradient_weights[l]);
                amx::nntrain_launch_bias_sums(h, l, T, n_chunks, st);
                const dim3 bgrid(std::min(1024, (h->out[l] + 255) / 256));
                if (sink)
                    hipLaunchKernelGGL(amx::nntrain_reduce_step_kernel, bgrid, dim3(256), 0, st, (const float*)h->d_part.get(), n_chunks, (size_t)h->out[l], 1, h->out[l],
                                       h->out[l], sink->g[l], h->out[l], sink->reset, (const float*)h->d_bias[l].get(), sink->bc[l], sink->regularizer, sink->c[l],
                                       sink->group_tail, (const double*)sink->call_tail);
                else
                    hipLaunchKernelGGL(amx::nntrain_reduce_kernel, bgrid, dim3(256), 0, st, (const float*)h->d_part.get(), n_chunks, (size_t)h->out[l], 1, h->out[l],
                                       h->out[l], acc + y.gradient_bias[l]);
            }
            AMX_HIP(hipGetLastError());
        }
    }
    return AMX_OK;
}

}  // namespace amx

extern "C" {

int amx_nntrain_accumulate_dev(amx_nntrain* h, const float* feats, int ldf, int T, const uint32_t* emission, const double* weight, double* acc) {
    AMX_REQUIRE(h && acc, AMX_ERR_INVALID, "amx_nntrain_accumulate_dev: NULL argument");
    return amx::nntrain_pass(h, feats, ldf, T, emission, weight, acc, nullptr, "amx_nntrain_accumulate_dev");
}

}  // extern "C"

// ------------------------------------------------------------------------------------ files, prior, mean and deviation (host)

namespace {

struct NnStat {  // an Nn::Statistics<f32> as its file holds it
    uint32_t n_obs = 0, n_err = 0;
    float    total_weight = 0.f, objective = 0.f;
    std::map<uint32_t, uint32_t>    counts;
    std::vector<float>              sum, sq;
    std::vector<std::vector<float>> gw, gb;
};

std::string magic_of(int mask) {
    std::string m("NNSTAT");
    m += (mask & AMX_NNSTAT_CLASS_COUNTS) ? 'C' : '#';
    m += (mask & AMX_NNSTAT_MEAN_AND_VARIANCE) ? 'M' : '#';
    m += (mask & AMX_NNSTAT_BASE) ? 'B' : '#';
    m += (mask & AMX_NNSTAT_GRADIENT) ? 'G' : '#';
    m += 'S';
    m += "#####";
    return m;
}

bool put_u32(FILE* f, uint32_t v) {
    unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
    return fwrite(b, 1, 4, f) == 4;
}
bool put_f32(FILE* f, float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return put_u32(f, u);
}
bool put_vec(FILE* f, const float* v, size_t n) {  // Math::Vector<f32>::write: u32 size, elements
    bool ok = put_u32(f, (uint32_t)n);
    for (size_t i = 0; ok && i < n; ++i)
        ok = put_f32(f, v[i]);
    return ok;
}
bool get_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4)
        return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}
bool get_f32(FILE* f, float* v) {
    uint32_t u;
    if (!get_u32(f, &u))
        return false;
    memcpy(v, &u, 4);
    return true;
}

// the buffer narrowed as FeedForwardTrainer::finalize narrows its double-precision statistics into the f32 ones it writes
// a count of the buffer as the u32 a file and the prior hold: false unless it is a whole number in [0, 2^32) (a cast of anything
// else -- negative, non-finite, too large -- is undefined)
bool as_u32(double v, uint32_t* out) {
    if (!(v >= 0.0 && v < 4294967296.0) || v != std::floor(v))
        return false;
    *out = (uint32_t)v;
    return true;
}

int narrow(const amx_nntrain* h, const double* acc, NnStat* s, const char* who) {
    const amx_nntrain_layout_info& y = h->lay;
    AMX_REQUIRE(as_u32(acc[y.tail + 0], &s->n_obs), AMX_ERR_INVALID, "%s: the number of observations %g is no u32", who, acc[y.tail + 0]);
    AMX_REQUIRE(as_u32(acc[y.tail + 1], &s->n_err), AMX_ERR_INVALID, "%s: the number of classification errors %g is no u32", who, acc[y.tail + 1]);
    s->total_weight = (float)acc[y.tail + 2];
    s->objective    = (float)acc[y.tail + 3];
    if (y.class_counts >= 0)
        for (int o = 0; o < h->n_outputs; ++o) {
            uint32_t c = 0;
            AMX_REQUIRE(as_u32(acc[y.class_counts + o], &c), AMX_ERR_INVALID, "%s: the count %g of output %d is no u32", who, acc[y.class_counts + o], o);
            if (c > 0)
                s->counts[(uint32_t)o] = c;
        }
    if (y.feature_sum >= 0) {
        s->sum.resize(h->feature_dim);
        s->sq.resize(h->feature_dim);
        for (int k = 0; k < h->feature_dim; ++k) {
            s->sum[k] = (float)acc[y.feature_sum + k];
            s->sq[k]  = (float)acc[y.feature_square_sum + k];
        }
    }
    if (h->mask & AMX_NNSTAT_GRADIENT) {
        s->gw.resize(h->L);
        s->gb.resize(h->L);
        for (int l = 0; l < h->L; ++l) {
            const size_t n = (size_t)h->in[l] * h->out[l];
            s->gw[l].resize(n);
            s->gb[l].resize(h->out[l]);
            for (size_t i = 0; i < n; ++i)
                s->gw[l][i] = (float)acc[y.gradient_weights[l] + i];
            for (int i = 0; i < h->out[l]; ++i)
                s->gb[l][i] = (float)acc[y.gradient_bias[l] + i];
        }
    }
    return AMX_OK;
}

void widen(const amx_nntrain* h, const NnStat& s, double* acc) {
    const amx_nntrain_layout_info& y = h->lay;
    for (long i = 0; i < y.size; ++i)
        acc[i] = 0.0;
    acc[y.tail + 0] = (double)s.n_obs;
    acc[y.tail + 1] = (double)s.n_err;
    acc[y.tail + 2] = (double)s.total_weight;
    acc[y.tail + 3] = (double)s.objective;
    if (y.class_counts >= 0)
        for (const auto& kv : s.counts)
            acc[y.class_counts + kv.first] = (double)kv.second;
    if (y.feature_sum >= 0)
        for (int k = 0; k < h->feature_dim; ++k) {
            acc[y.feature_sum + k]        = (double)s.sum[k];
            acc[y.feature_square_sum + k] = (double)s.sq[k];
        }
    if (h->mask & AMX_NNSTAT_GRADIENT)
        for (int l = 0; l < h->L; ++l) {
            for (size_t i = 0; i < s.gw[l].size(); ++i)
                acc[y.gradient_weights[l] + i] = (double)s.gw[l][i];
            for (size_t i = 0; i < s.gb[l].size(); ++i)
                acc[y.gradient_bias[l] + i] = (double)s.gb[l][i];
        }
}

int read_stat(const amx_nntrain* h, const char* path, NnStat* s, const char* who) {
    FILE* f = fopen(path, "rb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    struct Closer {
        FILE* f;
        ~Closer() { fclose(f); }
    } closer{f};
    char magic[17] = {0};
    AMX_REQUIRE(fread(magic, 1, 16, f) == 16, AMX_ERR_INVALID, "%s: '%s' is truncated (no magic)", who, path);
    AMX_REQUIRE(memcmp(magic, "NNSTAT", 6) == 0, AMX_ERR_INVALID, "%s: '%s' is no Nn::Statistics file", who, path);
    AMX_REQUIRE(magic[10] != 'D', AMX_ERR_UNSUPPORTED, "%s: '%s' holds double-precision statistics (precision letter D)", who, path);
    const std::string want = magic_of(h->mask);
    AMX_REQUIRE(memcmp(magic, want.data(), 16) == 0, AMX_ERR_INVALID, "%s: '%s' has magic %.16s, the handle's statistics give %s", who, path, magic, want.c_str());
    uint32_t version = 0;
    AMX_REQUIRE(get_u32(f, &version), AMX_ERR_INVALID, "%s: '%s' is truncated (version)", who, path);
    AMX_REQUIRE(version == 2, AMX_ERR_INVALID, "%s: '%s': version must be \"2\" and not \"%u\"", who, path, version);
    bool ok = get_u32(f, &s->n_obs) && get_f32(f, &s->total_weight);
    if (ok && (h->mask & AMX_NNSTAT_BASE))
        ok = get_u32(f, &s->n_err) && get_f32(f, &s->objective);
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: '%s' is truncated (base statistics)", who, path);
    if (h->mask & AMX_NNSTAT_CLASS_COUNTS) {
        uint32_t n = 0;
        AMX_REQUIRE(get_u32(f, &n), AMX_ERR_INVALID, "%s: '%s' is truncated (class counts)", who, path);
        AMX_REQUIRE(n <= (uint32_t)h->n_outputs, AMX_ERR_INVALID, "%s: '%s' counts %u classes, the network has %d outputs", who, path, n, h->n_outputs);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t c = 0, k = 0;
            AMX_REQUIRE(get_u32(f, &c) && get_u32(f, &k), AMX_ERR_INVALID, "%s: '%s' is truncated (class counts)", who, path);
            AMX_REQUIRE(c < (uint32_t)h->n_outputs, AMX_ERR_INVALID, "%s: '%s' counts class %u, the network has %d outputs", who, path, c, h->n_outputs);
            s->counts[c] = k;
        }
    }
    auto get_vec = [&](std::vector<float>* v, int want_n, const char* what) -> int {
        uint32_t n = 0;
        AMX_REQUIRE(get_u32(f, &n), AMX_ERR_INVALID, "%s: '%s' is truncated (%s)", who, path, what);
        AMX_REQUIRE(n == (uint32_t)want_n, AMX_ERR_INVALID, "%s: '%s': %s has %u elements, the handle %d", who, path, what, n, want_n);
        v->resize(n);
        for (uint32_t i = 0; i < n; ++i)
            AMX_REQUIRE(get_f32(f, v->data() + i), AMX_ERR_INVALID, "%s: '%s' is truncated (%s)", who, path, what);
        return AMX_OK;
    };
    if (h->mask & AMX_NNSTAT_MEAN_AND_VARIANCE) {
        AMX_TRY(get_vec(&s->sum, h->feature_dim, "the feature sum"));
        AMX_TRY(get_vec(&s->sq, h->feature_dim, "the sum of squares"));
    }
    if (h->mask & AMX_NNSTAT_GRADIENT) {
        uint32_t nl = 0;
        AMX_REQUIRE(get_u32(f, &nl), AMX_ERR_INVALID, "%s: '%s' is truncated (gradient)", who, path);
        AMX_REQUIRE(nl == (uint32_t)h->L, AMX_ERR_INVALID, "%s: '%s' holds %u trainable layers, the network has %d", who, path, nl, h->L);
        s->gw.resize(h->L);
        s->gb.resize(h->L);
        for (int l = 0; l < h->L; ++l) {
            uint32_t ns = 0, nr = 0, nc = 0, n2 = 0;
            AMX_REQUIRE(get_u32(f, &ns) && get_u32(f, &nr) && get_u32(f, &nc) && get_u32(f, &n2), AMX_ERR_INVALID, "%s: '%s' is truncated (layer %d)", who, path, l);
            AMX_REQUIRE(ns == 1, AMX_ERR_UNSUPPORTED, "%s: '%s': layer %d has %u input streams", who, path, l, ns);
            AMX_REQUIRE(nr == (uint32_t)h->in[l] && nc == (uint32_t)h->out[l] && n2 == nr, AMX_ERR_INVALID, "%s: '%s': layer %d is %u x %u, the network's %d x %d", who,
                        path, l, nr, nc, h->in[l], h->out[l]);
            s->gw[l].resize((size_t)nr * nc);
            for (uint32_t r = 0; r < nr; ++r) {
                uint32_t len = 0;
                bool     row = get_u32(f, &len) && len == nc;
                for (uint32_t c = 0; row && c < nc; ++c)
                    row = get_f32(f, s->gw[l].data() + (size_t)r * nc + c);
                AMX_REQUIRE(row, AMX_ERR_INVALID,
                            "%s: '%s' is truncated (layer %d, row %u)", who, path, l, r);
            }
            char what[48];
            snprintf(what, sizeof what, "the bias gradient of layer %d", l);
            AMX_TRY(get_vec(&s->gb[l], h->out[l], what));
        }
    }
    return AMX_OK;
}

}  // namespace

namespace amx {

int nntrain_add_regularizer(amx_nntrain* h, const StepSink* sink) {
    hipStream_t st = h->ctx->stream;
    for (int l = 0; l < h->L; ++l) {
        if (!(sink->c[l] > 0.f))
            continue;
        const long long total = (long long)h->in[l] * h->out[l];
        hipLaunchKernelGGL(nntrain_reduce_step_kernel, dim3((int)std::min<long long>(16384, (total + 255) / 256)), dim3(256), 0, st, (const float*)nullptr, 0, (size_t)0,
                           h->in[l], h->out[l], h->Pout[l], sink->G[l], h->Pout[l], 0, (const float*)h->d_WT[l].get(), sink->WTc[l], sink->regularizer, sink->c[l],
                           sink->group_tail, (const double*)sink->call_tail);
        hipLaunchKernelGGL(nntrain_reduce_step_kernel, dim3(std::min(1024, (h->out[l] + 255) / 256)), dim3(256), 0, st, (const float*)nullptr, 0, (size_t)0, 1, h->out[l],
                           h->out[l], sink->g[l], h->out[l], 0, (const float*)h->d_bias[l].get(), sink->bc[l], sink->regularizer, sink->c[l], sink->group_tail,
                           (const double*)sink->call_tail);
    }
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

int nntrain_narrow_gradient(const amx_nntrain* h, const double* acc, std::vector<std::vector<float>>* gw, std::vector<std::vector<float>>* gb, uint32_t* n_obs,
                            uint32_t* n_err, float* total_weight, float* objective, const char* who) {
    NnStat s;
    AMX_TRY(narrow(h, acc, &s, who));
    *gw = std::move(s.gw), *gb = std::move(s.gb);
    *n_obs = s.n_obs, *n_err = s.n_err, *total_weight = s.total_weight, *objective = s.objective;
    return AMX_OK;
}

}  // namespace amx

extern "C" {

int amx_nnstat_write(const amx_nntrain* h, const double* acc, const char* path) {
    AMX_REQUIRE(h && acc && path, AMX_ERR_INVALID, "amx_nnstat_write: NULL argument");
    NnStat s;
    AMX_TRY(narrow(h, acc, &s, "amx_nnstat_write"));
    FILE* f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "amx_nnstat_write: cannot open '%s'", path);
    const std::string magic = magic_of(h->mask);
    bool              ok    = fwrite(magic.data(), 1, 16, f) == 16 && put_u32(f, 2) && put_u32(f, s.n_obs) && put_f32(f, s.total_weight);
    if (h->mask & AMX_NNSTAT_BASE)
        ok = ok && put_u32(f, s.n_err) && put_f32(f, s.objective);
    if (h->mask & AMX_NNSTAT_CLASS_COUNTS) {
        ok = ok && put_u32(f, (uint32_t)s.counts.size());
        for (const auto& kv : s.counts)
            ok = ok && put_u32(f, kv.first) && put_u32(f, kv.second);
    }
    if (h->mask & AMX_NNSTAT_MEAN_AND_VARIANCE)
        ok = ok && put_vec(f, s.sum.data(), s.sum.size()) && put_vec(f, s.sq.data(), s.sq.size());
    if (h->mask & AMX_NNSTAT_GRADIENT) {
        ok = ok && put_u32(f, (uint32_t)h->L);
        for (int l = 0; ok && l < h->L; ++l) {
            const uint32_t nr = (uint32_t)h->in[l], nc = (uint32_t)h->out[l];
            ok = put_u32(f, 1) && put_u32(f, nr) && put_u32(f, nc) && put_u32(f, nr);
            for (uint32_t r = 0; ok && r < nr; ++r)
                ok = put_vec(f, s.gw[l].data() + (size_t)r * nc, nc);
            ok = ok && put_vec(f, s.gb[l].data(), nc);
        }
    }
    ok = (fclose(f) == 0) && ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "amx_nnstat_write: write to '%s' failed", path);
    return AMX_OK;
}

int amx_nnstat_read(const amx_nntrain* h, const char* path, double* acc) {
    AMX_REQUIRE(h && acc && path, AMX_ERR_INVALID, "amx_nnstat_read: NULL argument");
    NnStat s;
    AMX_TRY(read_stat(h, path, &s, "amx_nnstat_read"));
    widen(h, s, acc);
    return AMX_OK;
}

int amx_nnstat_combine(const amx_nntrain* h, const char* const* paths, int n, double* acc) {
    AMX_REQUIRE(h && acc && paths, AMX_ERR_INVALID, "amx_nnstat_combine: NULL argument");
    AMX_REQUIRE(n >= 1, AMX_ERR_INVALID, "amx_nnstat_combine: no statistics filenames given for combination");
    NnStat total;
    AMX_REQUIRE(paths[0], AMX_ERR_INVALID, "amx_nnstat_combine: NULL path");
    AMX_TRY(read_stat(h, paths[0], &total, "amx_nnstat_combine"));
    for (int i = 1; i < n; ++i) {  // Statistics<f32>::add
        NnStat s;
        AMX_REQUIRE(paths[i], AMX_ERR_INVALID, "amx_nnstat_combine: NULL path");
        AMX_TRY(read_stat(h, paths[i], &s, "amx_nnstat_combine"));
        total.n_obs += s.n_obs;
        total.total_weight = total.total_weight + s.total_weight;
        if (h->mask & AMX_NNSTAT_BASE) {
            total.n_err += s.n_err;
            total.objective = total.objective + s.objective;
        }
        for (size_t k = 0; k < total.sum.size(); ++k) {
            total.sum[k] = total.sum[k] + s.sum[k];
            total.sq[k]  = total.sq[k] + s.sq[k];
        }
        for (const auto& kv : s.counts)
            total.counts[kv.first] += kv.second;
        for (size_t l = 0; l < total.gw.size(); ++l) {
            for (size_t k = 0; k < total.gw[l].size(); ++k)
                total.gw[l][k] = total.gw[l][k] + s.gw[l][k];
            for (size_t k = 0; k < total.gb[l].size(); ++k)
                total.gb[l][k] = total.gb[l][k] + s.gb[l][k];
        }
    }
    widen(h, total, acc);
    return AMX_OK;
}

int amx_prior_from_class_counts(const amx_nntrain* h, const double* acc, float back_off_count, float* log_prior) {
    AMX_REQUIRE(h && acc && log_prior, AMX_ERR_INVALID, "amx_prior_from_class_counts: NULL argument");
    AMX_REQUIRE(h->lay.class_counts >= 0, AMX_ERR_STATE, "amx_prior_from_class_counts: the handle keeps no class counts");
    AMX_REQUIRE(back_off_count >= 0.f && back_off_count < 4294967296.f && back_off_count == std::floor(back_off_count), AMX_ERR_INVALID,
                "amx_prior_from_class_counts: back_off_count must be a whole number (a u32 in the reference)");
    const uint32_t back_off = (uint32_t)back_off_count;
    float          total    = 0.0f;
    for (int c = 0; c < h->n_outputs; ++c) {
        uint32_t count = 0;
        AMX_REQUIRE(as_u32(acc[h->lay.class_counts + c], &count), AMX_ERR_INVALID, "amx_prior_from_class_counts: the count %g of output %d is no u32",
                    acc[h->lay.class_counts + c], c);
        float          v     = (float)std::max(count, back_off);
        v                    = v * h->class_weights[c];
        log_prior[c]         = v;
        total                = total + v;
    }
    for (int c = 0; c < h->n_outputs; ++c)
        log_prior[c] = log_prior[c] == 0 ? -FLT_MAX : std::log(log_prior[c] / total);
    return AMX_OK;
}

int amx_nnstat_mean_and_deviation(const amx_nntrain* h, const double* acc, float* mean, float* stddev) {
    AMX_REQUIRE(h && acc && mean && stddev, AMX_ERR_INVALID, "amx_nnstat_mean_and_deviation: NULL argument");
    AMX_REQUIRE(h->lay.feature_sum >= 0, AMX_ERR_STATE, "amx_nnstat_mean_and_deviation: the handle keeps no feature sums");
    const float total_weight = (float)acc[h->lay.tail + 2];
    const float a            = (float)(1.0 / total_weight);  // sum_.scale(1.0 / totalWeight_): the quotient is a double, scale takes a T
    for (int k = 0; k < h->feature_dim; ++k) {
        const float m   = (float)acc[h->lay.feature_sum + k] * a;
        const float sq  = (float)acc[h->lay.feature_square_sum + k] * a;
        const float tmp = m * m;
        const float neg = -1.0f * tmp;  // sumOfSquares_.add(tmp, (T)-1.0): axpy
        const float var = sq + neg;
        mean[k]         = m;
        stddev[k]       = std::sqrt(var);
    }
    return AMX_OK;
}

}  // extern "C"
