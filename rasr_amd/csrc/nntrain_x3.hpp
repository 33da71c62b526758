// nntrain_x3.hpp -- the split-bf16 GEMMs of NN training (amx_nntrain_cfg.gemm = AMX_NNTRAIN_GEMM_BF16X3): the three GEMM kinds of
// nntrain.hip (forward, E W, X E^T) on v_mfma_f32_32x32x16_bf16 instead of the f32 matrix pipe.  include/amx.h ("NN training
// statistics", "Split-bf16 GEMMs") states the arithmetic; everything that is no GEMM (softmax, error, reduce, column sums, tail) is
// nntrain.hip's and is not touched.  Included by nntrain.hip alone, which dispatches to the functions at the end of this file.
//
// Every operand element v is split once, where it is produced, into hi = bf16(v) and lo = bf16(v - hi), round to nearest even
// (nntrain_split_kernel); the planes replace the f32 matrix in the GEMM's reads (4 bytes per element, as before).  Every GEMM then
// reads both operands with k contiguous:
//   forward    W   [Pout x Pin]  . X_l   [T x Pin]      k = Pin
//   E W        W^T [Pin x Pout]  . E_l   [T x Pout]     k = Pout
//   X E^T      X_l^T [Pin x T]   . E_l^T [Pout x T]     k = the frames of one chunk (grid.y = chunk)
// so activations and error signals are written twice by the split pass: as they lie and transposed (through an LDS tile).
//
// nntrain_gemm_x3_kernel: 128 x 128 tile, four waves 2 x 2, each 2 x 2 accumulators of 32 x 32.  K-tile of 32: four planes (A hi, A lo,
// B hi, B lo) of 128 rows x 64 bytes = 32 KB per stage, two stages.  The next K-tile's global loads are issued in front of the current
// tile's matrix instructions and land in LDS behind them: one barrier per K-tile.  A row's four 16-byte chunks are XOR-swizzled by
// the row, so that the ds_read_b128 of a fragment (lane: row lane & 31, k-group lane >> 5) meet no bank twice, with 32 and with 64
// banks.  One set of fragment reads feeds the three products of a k-step of 16:
//   acc += A_hi B_hi;  acc += A_hi B_lo;  acc += A_lo B_hi        (A: the operand named first in the table above)
// in this order, k ascending, one f32 accumulator chain per output element from zero.  Zero splits into two zeros, so the padding
// argument at the top of nntrain.hip holds as it stands.  Epilogues: the f32 kernels', operation for operation.
#pragma once
#include "nntrain.hpp"

namespace amx {

typedef __attribute__((ext_vector_type(8))) short x3_bf16x8;
typedef float  x3_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 x3_bf16x2 __attribute__((ext_vector_type(2)));

// two f32 -> packed bf16, round to nearest even (one v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned x3_pack(float a, float b) {
    x3_f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, x3_bf16x2));
}

// v -> hi | lo << 16
__device__ __forceinline__ unsigned x3_split(float v) {
    const unsigned hi = x3_pack(v, 0.f) & 0xffffu;
    const unsigned lo = x3_pack(v - __uint_as_float(hi << 16), 0.f) & 0xffffu;  // v - hi is exact in f32
    return hi | (lo << 16);
}

// ---- src [R x C] f32 (R, C multiples of 64) -> hi, lo [R x C] (NAT) and hiT, loT [C x R] (TR); one workgroup per 64 x 64 tile
constexpr int SP_TILE = 64;

template<bool NAT, bool TR>
__global__ __launch_bounds__(256) void nntrain_split_kernel(const float* __restrict__ src, int R, int C, x3_bf16_t* __restrict__ hi, x3_bf16_t* __restrict__ lo,
                                                           x3_bf16_t* __restrict__ hiT, x3_bf16_t* __restrict__ loT) {
    __shared__ unsigned s_tile[SP_TILE][SP_TILE + 1];
    const int tid = threadIdx.x, r0 = blockIdx.y * SP_TILE, c0 = blockIdx.x * SP_TILE;
    const int rr = tid >> 4, cc = (tid & 15) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int    row = q * 16 + rr;
        const size_t at  = (size_t)(r0 + row) * C + c0 + cc;
        const float4 v   = *(const float4*)(src + at);
        const unsigned s[4] = {x3_split(v.x), x3_split(v.y), x3_split(v.z), x3_split(v.w)};
        if (NAT) {
            *(uint2*)(hi + at) = make_uint2((s[0] & 0xffffu) | (s[1] << 16), (s[2] & 0xffffu) | (s[3] << 16));
            *(uint2*)(lo + at) = make_uint2((s[0] >> 16) | (s[1] & 0xffff0000u), (s[2] >> 16) | (s[3] & 0xffff0000u));
        }
        if (TR) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                s_tile[row][cc + e] = s[e];
        }
    }
    if (!TR)
        return;
    __syncthreads();
    const int col = tid >> 2, rg = (tid & 3) * 16;  // 16 consecutive rows of one column: 32 bytes of each transposed plane
    unsigned  h[8], l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const unsigned a = s_tile[rg + 2 * e][col], b = s_tile[rg + 2 * e + 1][col];
        h[e] = (a & 0xffffu) | (b << 16);
        l[e] = (a >> 16) | (b & 0xffff0000u);
    }
    const size_t at = (size_t)(c0 + col) * R + r0 + rg;
    *(uint4*)(hiT + at)     = make_uint4(h[0], h[1], h[2], h[3]);
    *(uint4*)(hiT + at + 8) = make_uint4(h[4], h[5], h[6], h[7]);
    *(uint4*)(loT + at)     = make_uint4(l[0], l[1], l[2], l[3]);
    *(uint4*)(loT + at + 8) = make_uint4(l[4], l[5], l[6], l[7]);
}

// ---- the GEMM core: C[a][b] = sum_k A[a][k] B[b][k] on the split planes
constexpr int X3_TILE  = 128;  // tile edge, both ways
constexpr int X3_KT    = 32;   // k per stage
constexpr int X3_PLANE = X3_TILE * 4;  // 16-byte chunks of one plane's stage: 128 rows x 4

enum { X3_FORWARD = 0, X3_FORWARD_TOP = 1, X3_BACKWARD = 2, X3_GRADIENT = 3 };

struct X3Epilogue {
    const float* bias;  // forward [Pout]
    const float* Y;     // E W: the stored f32 output of the layer below [Tpad x ldo]
    float*       out;   // forward / E W: [Tpad x ldo] (top: [T x n_valid]); X E^T: the chunk partials [chunks x Kpad x ldo]
    int          ldo, n_valid, t_valid;
    size_t       chunk_stride;
    float        clip;
    int          do_clip;
};

// chunk c of row `row` lies at slot row * 4 + (c ^ swz(row)): rows r .. r + 7 (32 banks) and r .. r + 15 (64 banks) of one chunk
// column then cover every bank once
__device__ __forceinline__ int x3_slot(int row, int c) {
    return row * 4 + (c ^ (((row >> 1) + (row >> 3)) & 3));
}

template<int EPI, int ACT>
__global__ __launch_bounds__(256) void nntrain_gemm_x3_kernel(const x3_bf16_t* __restrict__ Ahi, const x3_bf16_t* __restrict__ Alo, int lda,
                                                             const x3_bf16_t* __restrict__ Bhi, const x3_bf16_t* __restrict__ Blo, int ldb, int K,
                                                             int n_tiles_a, X3Epilogue ep) {
    __shared__ uint4 s_op[2][4][X3_PLANE];  // stage, plane (A hi, A lo, B hi, B lo): 64 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;
    const int tile_b = blockIdx.x / n_tiles_a, tile_a = blockIdx.x - tile_b * n_tiles_a;
    const int a0 = tile_a * X3_TILE, b0 = tile_b * X3_TILE;
    int       k_begin = 0, k_end = K;
    if (EPI == X3_GRADIENT) {  // the frames of chunk blockIdx.y; K = Tpad is a multiple of 128: whole stages
        k_begin = blockIdx.y * AMX_NNTRAIN_CHUNK;
        k_end   = min(K, k_begin + AMX_NNTRAIN_CHUNK);
    }
    const int n_kt = (k_end - k_begin) / X3_KT;

    // the stage's loads of this thread: two chunks per plane, rows ld_row and ld_row + 64
    const int        ld_row = tid >> 2, ld_c = tid & 3;
    const x3_bf16_t* gAh = Ahi + (size_t)(a0 + ld_row) * lda + ld_c * 8;
    const x3_bf16_t* gAl = Alo + (size_t)(a0 + ld_row) * lda + ld_c * 8;
    const x3_bf16_t* gBh = Bhi + (size_t)(b0 + ld_row) * ldb + ld_c * 8;
    const x3_bf16_t* gBl = Blo + (size_t)(b0 + ld_row) * ldb + ld_c * 8;
    const size_t     half_a = (size_t)64 * lda, half_b = (size_t)64 * ldb;
    const int        st0 = x3_slot(ld_row, ld_c), st1 = x3_slot(ld_row + 64, ld_c);
    uint4            r0, r1, r2, r3, r4, r5, r6, r7;
#define X3_FETCH(k0)                                  \
    do {                                              \
        r0 = *(const uint4*)(gAh + (k0));             \
        r1 = *(const uint4*)(gAh + half_a + (k0));    \
        r2 = *(const uint4*)(gAl + (k0));             \
        r3 = *(const uint4*)(gAl + half_a + (k0));    \
        r4 = *(const uint4*)(gBh + (k0));             \
        r5 = *(const uint4*)(gBh + half_b + (k0));    \
        r6 = *(const uint4*)(gBl + (k0));             \
        r7 = *(const uint4*)(gBl + half_b + (k0));    \
    } while (0)
#define X3_STASH(stage)                               \
    do {                                              \
        s_op[stage][0][st0] = r0, s_op[stage][0][st1] = r1; \
        s_op[stage][1][st0] = r2, s_op[stage][1][st1] = r3; \
        s_op[stage][2][st0] = r4, s_op[stage][2][st1] = r5; \
        s_op[stage][3][st0] = r6, s_op[stage][3][st1] = r7; \
    } while (0)

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q)
                acc[i][j][q] = 0.f;

    X3_FETCH(k_begin);
    X3_STASH(0);
    __syncthreads();
    const int frow = lane & 31, fk = lane >> 5;
    for (int kt = 0; kt < n_kt; ++kt) {
        const int  stage = kt & 1;
        const bool more  = kt + 1 < n_kt;
        if (more)
            X3_FETCH(k_begin + (kt + 1) * X3_KT);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            x3_bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int sa = x3_slot(wa * 64 + i * 32 + frow, 2 * ks + fk), sb = x3_slot(wb * 64 + i * 32 + frow, 2 * ks + fk);
                ah[i] = *(const x3_bf16x8*)&s_op[stage][0][sa];
                al[i] = *(const x3_bf16x8*)&s_op[stage][1][sa];
                bh[i] = *(const x3_bf16x8*)&s_op[stage][2][sb];
                bl[i] = *(const x3_bf16x8*)&s_op[stage][3][sb];
            }
            // per accumulator: hi hi, hi lo, lo hi; the four accumulators take each product in turn, so that a chain's
            // matrix instructions lie four apart
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
        }
        if (more)
            X3_STASH(stage ^ 1);  // last read in front of the previous barrier
        __syncthreads();
    }

#undef X3_FETCH
#undef X3_STASH
    // accumulator q = 4 g + e of (i, j): A row 8 g + 4 (lane >> 5) + e, B row lane & 31
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int b = b0 + wb * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int a = a0 + wa * 64 + i * 32 + 8 * g + 4 * (lane >> 5);
                if (EPI == X3_GRADIENT) {  // part[chunk][k = a][n = b]
                    float* const dst = ep.out + (size_t)blockIdx.y * ep.chunk_stride;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        dst[(size_t)(a + e) * ep.ldo + b] = acc[i][j][g * 4 + e];
                }
                else if (EPI == X3_BACKWARD) {  // out[t = b][k = a] = acc * f'(Y), clipped
                    const float4 y4 = *(const float4*)(ep.Y + (size_t)b * ep.ldo + a);
                    const float  y[4] = {y4.x, y4.y, y4.z, y4.w};
                    float        o[4];
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
                        if (ep.do_clip)
                            v = v > 0.f ? (ep.clip < v ? ep.clip : v) : (v < -ep.clip ? -ep.clip : v);
                        o[e] = v;
                    }
                    *(float4*)(ep.out + (size_t)b * ep.ldo + a) = make_float4(o[0], o[1], o[2], o[3]);
                }
                else {  // forward: out[t = b][n = a]
                    float o[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[i][j][g * 4 + e] + ep.bias[a + e];
                        if (EPI == X3_FORWARD_TOP) {
                            if (b < ep.t_valid && a + e < ep.n_valid)
                                ep.out[(size_t)b * ep.ldo + a + e] = -v;
                        }
                        else
                            o[e] = activate<ACT>(v);
                    }
                    if (EPI == X3_FORWARD)
                        *(float4*)(ep.out + (size_t)b * ep.ldo + a) = make_float4(o[0], o[1], o[2], o[3]);
                }
            }
        }
}

// ------------------------------------------------------------------------------------ host side

namespace {

// planes of a matrix of n elements: hi at p, lo at p + n
struct Planes {
    x3_bf16_t *hi, *lo;
};

Planes planes(const DevBuf<x3_bf16_t>& b, size_t n) {
    return Planes{b.get(), b.get() + n};
}

// (its own event pair inside the GEMM kinds' pairs: tools/nntrain_probe.py reports the split passes' share)
void split(amx_nntrain* h, const float* src, int R, int C, Planes nat, Planes tr, hipStream_t st) {
    ScopedKernelTimer timer(h->ctx, "nntrain_x3_split");
    const dim3 grid(C / SP_TILE, R / SP_TILE), block(256);
    if (nat.hi && tr.hi)
        hipLaunchKernelGGL((nntrain_split_kernel<true, true>), grid, block, 0, st, src, R, C, nat.hi, nat.lo, tr.hi, tr.lo);
    else if (nat.hi)
        hipLaunchKernelGGL((nntrain_split_kernel<true, false>), grid, block, 0, st, src, R, C, nat.hi, nat.lo, (x3_bf16_t*)nullptr, (x3_bf16_t*)nullptr);
    else
        hipLaunchKernelGGL((nntrain_split_kernel<false, true>), grid, block, 0, st, src, R, C, (x3_bf16_t*)nullptr, (x3_bf16_t*)nullptr, tr.hi, tr.lo);
}

template<int EPI>
void gemm(int act, dim3 grid, hipStream_t st, Planes A, int lda, Planes B, int ldb, int K, int n_tiles_a, const X3Epilogue& ep) {
    const dim3 block(256);
    if constexpr (EPI == X3_FORWARD_TOP || EPI == X3_GRADIENT) {  // no activation in these epilogues
        hipLaunchKernelGGL((nntrain_gemm_x3_kernel<EPI, AMX_ACT_NONE>), grid, block, 0, st, A.hi, A.lo, lda, B.hi, B.lo, ldb, K, n_tiles_a, ep);
    }
    else switch (act) {
        case AMX_ACT_RELU:
            hipLaunchKernelGGL((nntrain_gemm_x3_kernel<EPI, AMX_ACT_RELU>), grid, block, 0, st, A.hi, A.lo, lda, B.hi, B.lo, ldb, K, n_tiles_a, ep);
            break;
        case AMX_ACT_SIGMOID:
            hipLaunchKernelGGL((nntrain_gemm_x3_kernel<EPI, AMX_ACT_SIGMOID>), grid, block, 0, st, A.hi, A.lo, lda, B.hi, B.lo, ldb, K, n_tiles_a, ep);
            break;
        case AMX_ACT_TANH:
            hipLaunchKernelGGL((nntrain_gemm_x3_kernel<EPI, AMX_ACT_TANH>), grid, block, 0, st, A.hi, A.lo, lda, B.hi, B.lo, ldb, K, n_tiles_a, ep);
            break;
        default:
            hipLaunchKernelGGL((nntrain_gemm_x3_kernel<EPI, AMX_ACT_NONE>), grid, block, 0, st, A.hi, A.lo, lda, B.hi, B.lo, ldb, K, n_tiles_a, ep);
    }
}

}  // namespace

// the planes of a call of Tpad rows, grown like d_x / d_E; the weights' planes exist from amx_nntrain_create on
int nntrain_x3_reserve(amx_nntrain* h, int Tpad) {
    const bool grad = (h->mask & AMX_NNSTAT_GRADIENT) != 0;
    for (int l = 0; l < h->L; ++l) {
        AMX_TRY(h->p_x[l].reserve((size_t)2 * Tpad * h->Pin[l]));
        if (grad) {
            AMX_TRY(h->p_xT[l].reserve((size_t)2 * Tpad * h->Pin[l]));
            AMX_TRY(h->p_E[l].reserve((size_t)2 * Tpad * h->Pout[l]));
            AMX_TRY(h->p_ET[l].reserve((size_t)2 * Tpad * h->Pout[l]));
        }
    }
    return AMX_OK;
}

int nntrain_x3_split_weights(amx_nntrain* h, hipStream_t st) {
    for (int l = 0; l < h->L; ++l) {
        const size_t n = (size_t)h->Pin[l] * h->Pout[l];
        AMX_TRY(h->p_W[l].reserve(2 * n));
        AMX_TRY(h->p_WT[l].reserve(2 * n));
        split(h, h->d_W[l].get(), h->Pout[l], h->Pin[l], planes(h->p_W[l], n), Planes{nullptr, nullptr}, st);
        split(h, h->d_WT[l].get(), h->Pin[l], h->Pout[l], planes(h->p_WT[l], n), Planes{nullptr, nullptr}, st);
    }
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

int nntrain_x3_forward(amx_nntrain* h, int Tpad, int T, hipStream_t st) {
    AMX_TRY(nntrain_x3_reserve(h, Tpad));
    const int  L    = h->L;
    const bool grad = (h->mask & AMX_NNSTAT_GRADIENT) != 0;
    for (int l = 0; l < L; ++l) {
        const size_t nx = (size_t)Tpad * h->Pin[l];
        const Planes X  = planes(h->p_x[l], nx);
        split(h, h->d_x[l].get(), Tpad, h->Pin[l], X, grad ? planes(h->p_xT[l], nx) : Planes{nullptr, nullptr}, st);
        const int  nta = h->Pout[l] / X3_TILE;
        const dim3 grid(nta * (Tpad / X3_TILE));
        X3Epilogue ep{};
        ep.bias = h->d_bias[l].get();
        const Planes W = planes(h->p_W[l], (size_t)h->Pin[l] * h->Pout[l]);
        if (l == L - 1) {
            ep.out = h->d_top.get(), ep.ldo = h->n_outputs, ep.n_valid = h->n_outputs, ep.t_valid = T;
            gemm<X3_FORWARD_TOP>(AMX_ACT_NONE, grid, st, W, h->Pin[l], X, h->Pin[l], h->Pin[l], nta, ep);
        }
        else {
            ep.out = h->d_x[l + 1].get(), ep.ldo = h->Pout[l];
            gemm<X3_FORWARD>(h->act[l], grid, st, W, h->Pin[l], X, h->Pin[l], h->Pin[l], nta, ep);
        }
    }
    return AMX_OK;
}

// E_top's planes first (whoever filled d_E[top]: nntrain_error_kernel or nnseq.hip), then each layer's E W and the split of what it wrote
int nntrain_x3_backward(amx_nntrain* h, int Tpad, float clip, hipStream_t st) {
    AMX_TRY(nntrain_x3_reserve(h, Tpad));
    const int L = h->L;
    for (int l = L - 1; l >= 0; --l) {
        const size_t ne = (size_t)Tpad * h->Pout[l];
        const Planes E  = planes(h->p_E[l], ne);
        split(h, h->d_E[l].get(), Tpad, h->Pout[l], l > 0 ? E : Planes{nullptr, nullptr}, planes(h->p_ET[l], ne), st);
        if (l == 0)
            break;
        const int  nta = h->Pin[l] / X3_TILE;
        X3Epilogue ep{};
        ep.Y = h->d_x[l].get(), ep.out = h->d_E[l - 1].get(), ep.ldo = h->Pin[l];
        ep.clip = clip, ep.do_clip = (l - 1 > 0 && clip < FLT_MAX) ? 1 : 0;
        gemm<X3_BACKWARD>(h->act[l - 1], dim3(nta * (Tpad / X3_TILE)), st, planes(h->p_WT[l], (size_t)h->Pin[l] * h->Pout[l]), h->Pout[l], E, h->Pout[l],
                          h->Pout[l], nta, ep);
    }
    return AMX_OK;
}

int nntrain_x3_gemm_tn(amx_nntrain* h, int l, int Tpad, int tn_chunks, hipStream_t st) {
    const int  Kp = h->Pin[l], Np = h->Pout[l], nta = Kp / X3_TILE;
    X3Epilogue ep{};
    ep.out = h->d_part.get(), ep.ldo = Np, ep.chunk_stride = (size_t)Kp * Np;
    gemm<X3_GRADIENT>(AMX_ACT_NONE, dim3(nta * (Np / X3_TILE), tn_chunks), st, planes(h->p_xT[l], (size_t)Tpad * Kp), Tpad, planes(h->p_ET[l], (size_t)Tpad * Np),
                      Tpad, Tpad, nta, ep);
    return AMX_OK;
}

}  // namespace amx
