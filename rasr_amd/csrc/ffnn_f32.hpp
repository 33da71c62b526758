// ffnn_f32.hpp -- the exact-f32 pieces of the feed-forward network that the scorer (ffnn.hip) and the training statistics
// (nntrain.hip) share: activations, preprocessing layers, the input pack, the f32 MFMA GEMM and the softmax top layer.
#pragma once
#include "common.hpp"

#include <cmath>

namespace amx {

typedef __attribute__((ext_vector_type(16))) float f32x16;

template<int ACT>
__device__ __forceinline__ float activate(float v) {
    if (ACT == AMX_ACT_RELU)
        return v < 0.f ? 0.f : v;  // ensureMinimalValue(0)
    if (ACT == AMX_ACT_SIGMOID)
        return 1.f / (1.f + expf(-v));  // Math/FastMatrix.hh:802-808
    if (ACT == AMX_ACT_TANH)
        return tanhf(v);
    if (ACT == AMX_ACT_ELU)
        return v < 0.f ? expf(v) - 1.f : v;  // Math/FastMatrix.hh:1658-1667, alpha 1: std::exp on a float; a NaN stays NaN
    return v;
}

// ---- value sources of the operand pack kernels: what element (t, k) of the next GEMM's operand is (t < T, k < K; the rest is zero)
// preprocessing layers of amx_ffnn_layers in front of layer 0 (AMX_NN_PRE_*), in order
struct PreOps {
    int          n;
    int          type[AMX_NN_MAX_PRE];
    const float* mean[AMX_NN_MAX_PRE];
    const float* rstd[AMX_NN_MAX_PRE];  // (f32)1 / stddev, rounded on the host
};

// the input features of a network without preprocessing layers: f32 rows as they are
struct RawSrc {
    const float* x;
    int          ldx;
    __device__ __forceinline__ float operator()(int t, int k) const { return x[(size_t)t * ldx + k]; }
};

// the input features: f32 rows, through the preprocessing layers
struct FeatSrc {
    const float* x;
    int          ldx;
    PreOps       pre;
    __device__ __forceinline__ float operator()(int t, int k) const {
        float v = x[(size_t)t * ldx + k];
#pragma unroll
        for (int i = 0; i < AMX_NN_MAX_PRE; ++i) {
            if (i >= pre.n)
                break;
            if (pre.type[i] == AMX_NN_PRE_LOGARITHM)
                v = (float)log((double)v);  // Math::vr_log: the unqualified log on a float is ::log(double) there, narrowed
            else {
                v = v - pre.mean[i][k];  // addToAllColumns(mean, -1): x + (-1 * m), the product is exact
                v = v * pre.rstd[i][k];  // divideRowsByScalars: scal((f32)1 / s)
            }
        }
        return v;
    }
};

// ---- Nn::NeuralNetworkForwardNode's top layer (Nn/NeuralNetworkForwardNode.cc:140-160: the node emits network_.getTopLayerOutput()).
// The scorers keep LinearAndSoftmaxLayer's softmax switched off and negate; the node keeps it on (evaluate-softmax, default true,
// Nn/LinearAndActivationLayer.cc:85-106).  Math::FastMatrix<f32>::softmax per frame (Math/FastMatrix.hh:818-834): maximum of the
// column, x + (-1 * max), exp() = mt_vr_exp (::exp(double) narrowed, Math/FastVectorOperations.hh:57-63), the SEQUENTIAL f32 sum of
// FastVector::addSummedRows (Math/FastVector.hh:481-489), scal by (f32)1.0 / sum.
// top_negmax_kernel: one workgroup per frame; a = -score (the activation, exact), row maximum, e = exp(a - max) written in place.
static __global__ __launch_bounds__(256) void top_negexp_kernel(float* __restrict__ x, int n, float* __restrict__ g_max) {
    __shared__ float s_red[4];
    float*           row = x + (size_t)blockIdx.x * n;
    float            mx  = -__builtin_inff();
    for (int i = threadIdx.x; i < n; i += 256)
        mx = fmaxf(mx, -row[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0)
        s_red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    const float value = -1.f * mx;  // addToAllRows(tmp, -1): alpha * max, then elem + value
    for (int i = threadIdx.x; i < n; i += 256) {
        const float a = -row[i];
        row[i]        = (float)exp((double)(a + value));
    }
    if (threadIdx.x == 0)
        g_max[blockIdx.x] = mx;
}

// lane = frame: the reference's sequential f32 sum over the outputs, in output order; 64 x 64 tiles go through LDS so that the global
// reads stay coalesced
static __global__ __launch_bounds__(64) void top_rowsum_kernel(const float* __restrict__ x, int T, int n, float* __restrict__ g_sum) {
    __shared__ float s_tile[64][65];
    const int        lane = threadIdx.x, t0 = blockIdx.x * 64;
    float            acc = 0.f;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int w = min(64, n - c0);
        for (int r = 0; r < 64; ++r)
            s_tile[r][lane] = (t0 + r < T && lane < w) ? x[(size_t)(t0 + r) * n + c0 + lane] : 0.f;
        __syncthreads();
        for (int c = 0; c < w; ++c)
            acc = acc + s_tile[lane][c];
        __syncthreads();
    }
    if (t0 + lane < T)
        g_sum[t0 + lane] = acc;
}

// elementwise tail: LINEAR negates the scores (activation = -score, exact), SOFTMAX multiplies by (f32)1.0 / sum (Math::scal)
static __global__ __launch_bounds__(256) void top_finish_kernel(float* __restrict__ x, long long total, int n, const float* __restrict__ g_sum) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (g_sum) {
            const float r = 1.f / g_sum[i / n];
            x[i]          = x[i] * r;
        }
        else
            x[i] = -x[i];
    }
}

// f32 frames (or a maxout) -> f32 [Tpad x Kpad], zero padded; with Kpad = K and Tpad = T: the plain [T x K] rows
template<class S>
__global__ __launch_bounds__(256) void pack_input_f32(S src, int T, int K, float* __restrict__ out, int Kpad, int Tpad) {
    const long long n = (long long)Tpad * Kpad;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int t = (int)(i / Kpad), k = (int)(i - (long long)t * Kpad);
        out[i] = (t < T && k < K) ? src(t, k) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// fp32 GEMM (parity mode): exact f32 MFMA, register-staged LDS tiles with padded rows.
constexpr int BN = 128, BT = 128;  // f32 tile
constexpr int FK  = 32;       // k per tile
constexpr int FLD = FK + 1;   // padded row (floats) -> conflict-free column reads

template<int ACT, bool LAST>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ W, const float* __restrict__ X,
                                                      const float* __restrict__ bias, float* __restrict__ out, int Kpad, int ldx, int ldo,
                                                      int n_valid, int t_valid, int n_tiles_n) {
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

    for (int k0 = 0; k0 < Kpad; k0 += FK) {
        // 128 rows x 32 floats per operand = 1024 float4, 4 per thread
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int    idx = i * 256 + tid;
            const int    row = idx >> 3, c4 = (idx & 7) * 4;
            const float4 w   = *(const float4*)(W + (size_t)(n0 + row) * Kpad + k0 + c4);
            const float4 x   = *(const float4*)(X + (size_t)(t0 + row) * ldx + k0 + c4);
            float*       dw  = sW + row * FLD + c4;
            float*       dx  = sX + row * FLD + c4;
            dw[0] = w.x; dw[1] = w.y; dw[2] = w.z; dw[3] = w.w;
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
                const int n = n0 + wn * 64 + i * 32 + 8 * g + 4 * (lane >> 5);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = acc[i][j][g * 4 + e] + bias[n + e];
                    if (LAST) {
                        if (t < t_valid && n + e < n_valid)
                            out[(size_t)t * ldo + n + e] = -v;
                    }
                    else
                        out[(size_t)t * ldo + n + e] = activate<ACT>(v);
                }
            }
        }
}

}  // namespace amx
