// segclust.hip -- speaker clustering of segments on the device (include/amx.h, section "segment clustering"): the model
// Signal::CorrFullCovMonoGaussianModel of Signal/SegmentClustering.{hh,cc} (one full-covariance Gaussian per segment, agglomerative clustering
// under the correlation distance of the segments' relative-likelihood features, the BIC stopping rule).  The BIC choice, the class ids and the
// key-map file are segclust_host.cpp's.
//
// Kernels.
//   segclust_acc_kernel       workgroup = (segment, 256 cells of [sum | lower triangle of the square sum]); frames staged in LDS kScStage at
//                             a time, a lane owns its cell and adds the exact products in frame order: the reference's bits, no atomics.
//   segclust_finalize_kernel  wave = model, lane = column: mean and variance with the f32 reciprocal, LU with partial pivoting in the wave's
//                             LDS slice (sc_lu), the +0.1 loop at an exact zero pivot, inverse by substitution (sc_inverse), log-determinant.
//   segclust_pack_kernel      the operands U_i, V_j of R(i|j) = f32(-0.5 n_i U_i . V_j) around the frame-weighted global mean c.
//   sc_gemm_nt_kernel<double> R = U V^T on v_mfma_f64_16x16x4_f64; <float>: the initial distances -F F^T (lower triangle) on
//                             v_mfma_f32_16x16x4_f32.  64 x 64 tile per workgroup, 2 x 2 instruction tiles per wave, operands through LDS.
//   segclust_rows_kernel      lane = row: the reference's logSum chain over a row of alpha R (tiles of R through LDS), the term of the alpha
//                             search, the feature row exp(alpha R - logSum).
//   the merge loop            per step segclust_argmin_kernel (cached row minima, the reference's tie rule), segclust_merge_kernel (merged
//                             model, sc_lu, tracker record, U of the merged model), segclust_refresh_kernel (its R row against the V of all
//                             original models), segclust_featrow_kernel (its feature row), segclust_update_kernel (the parent's row and column,
//                             row minima).  State lives in device memory; the host enqueues N - 1 rounds and synchronises once.
// The library is compiled with -ffp-contract=off and nothing here asks for a fused multiply-add: amx_set_contract changes nothing.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.hpp"

namespace amx {

// The two bounds are chosen, not tuned: D <= 64 lets a lane own a column of a model's matrix, N <= 8192 keeps the three N x N f32 matrices
// (R, the features, the distances) at 256 MB each.
constexpr int    kScMaxDim    = 64;
constexpr int    kScMaxSeg    = 8192;
constexpr double kScLn2Pi     = 1.83787706640934533908193770912475883960723876953125;   // LN_2PI of SegmentClustering.hh:34
constexpr float  kScMinLogEps = 11.513f;                                                // MINLOGEPS of Math/Vector.hh

// what the kernels of one clustering share: sizes, the slots' models (a merge replaces its parent's), the operands, the loop's state
struct ScDev {
    int       D, N, KKp;   // dimension, segments after the filter, padded inner length of R's product
    long long ld;          // leading dimension of R, F and dist: N padded to whole tiles
    float     alpha, threshold;
    unsigned* n;           // [N] frames of the slot's model
    double *  mean, *var, *inv, *logdet, *center, *u_new;
    float *   like, *row_v, *tr_score, *r_new;
    int *     bumps, *active, *row_j, *tr_parent, *tr_child, *state;   // state: parent, child of the current step
    double *  U, *V;       // [N padded x KKp]
    float *   F, *dist;    // [N padded x ld]
    unsigned* fail;        // bits: 2 a segment stays singular, 4 no pair left, 8 zero pivot in a merged model
};

constexpr int kScThreads = 256;
constexpr int kScStage   = 32;   // frames staged in LDS at a time
constexpr int kScTile    = 64;   // rows and columns of a workgroup's GEMM tile
constexpr int kScKc      = 16;   // inner length of a GEMM stage
constexpr int kScMaxBump = 100;  // rounds of the +0.1 loop before a model is given up

typedef double sc_double4 __attribute__((ext_vector_type(4)));
typedef float  sc_float4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int sc_tri(int i, int j) {   // cell of (i, j), j <= i, in the row-major lower triangle
    return i * (i + 1) / 2 + j;
}

__device__ inline void sc_tri_decode(int cell, int* i, int* j) {
    int row = 0;
    while (cell > row) {
        cell -= row + 1;
        ++row;
    }
    *i = row;
    *j = cell;
}

// ---- per-segment sums (:53-61).  grid: x = 256 cells of [sum: D | sq: lower triangle], y = segment of this call
__global__ __launch_bounds__(kScThreads) void segclust_acc_kernel(const float* __restrict__ feats, long long ld, int D, const long long* __restrict__ off,
                                                                  double* __restrict__ sums, int cells, unsigned* __restrict__ bad) {
    __shared__ float s_x[kScStage][kScMaxDim];
    const int        seg = blockIdx.y, tid = threadIdx.x, cell = blockIdx.x * kScThreads + tid;
    const bool       active = cell < cells;
    int              i = active && cell < D ? cell : 0, j = -1;   // j < 0: a cell of the sum
    if (active && cell >= D)
        sc_tri_decode(cell - D, &i, &j);
    double sum = 0.0;
    for (long long t = off[seg]; t < off[seg + 1]; t += kScStage) {
        const int n = off[seg + 1] - t < kScStage ? (int)(off[seg + 1] - t) : kScStage;
        for (int idx = tid; idx < n * D; idx += kScThreads) {
            const int   f = idx / D, c = idx - f * D;
            const float v = feats[(t + f) * ld + c];
            s_x[f][c]     = v;
            if (blockIdx.x == 0 && (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u)
                atomicOr(bad, 1u);
        }
        __syncthreads();
        if (active)
            for (int f = 0; f < n; ++f) {
                const double xi = (double)s_x[f][i];
                sum += j < 0 ? xi : xi * (double)s_x[f][j];   // the product of two widened f32 is exact
            }
        __syncthreads();
    }
    if (active)
        sums[(long long)seg * cells + cell] = sum;
}

// ---- LU with partial pivoting (first-largest rule) of a [D x D] in LDS by ONE wave (a workgroup of 64), lane = column.  perm[r]: the row
// of the input that stands in row r.  false at an exact zero pivot (or a NaN); *logdet = sum log|u_ii| in index order.
__device__ bool sc_lu(double* a, int D, int* perm, double* logdet) {
    const int lane = threadIdx.x;
    double    acc  = 0.0;
    if (lane < D)
        perm[lane] = lane;
    __syncthreads();
    for (int k = 0; k < D; ++k) {
        double v = lane >= k && lane < D ? fabs(a[lane * D + k]) : -1.0;
        int    p = lane;
#pragma unroll
        for (int m = 32; m; m >>= 1) {
            const double ov = __shfl_xor(v, m);
            const int    op = __shfl_xor(p, m);
            if (ov > v || (ov == v && op < p))
                v = ov, p = op;
        }
        if (!(v > 0.0))
            return false;
        if (p != k && lane < D) {
            const double t  = a[k * D + lane];
            a[k * D + lane] = a[p * D + lane];
            a[p * D + lane] = t;
            if (lane == 0) {
                const int q = perm[k];
                perm[k]     = perm[p];
                perm[p]     = q;
            }
        }
        __syncthreads();
        const double piv = a[k * D + k];
        acc += log(fabs(piv));
        if (lane > k && lane < D)
            a[lane * D + k] = a[lane * D + k] / piv;   // lane = row here
        __syncthreads();
        if (lane > k && lane < D) {
            const double akc = a[k * D + lane];
            for (int r = k + 1; r < D; ++r)
                a[r * D + lane] -= a[r * D + k] * akc;
        }
        __syncthreads();
    }
    *logdet = acc;
    return true;
}

// inverse from sc_lu's factors: lane c solves L U x = P e_c into column c of x [D x D] (LDS)
__device__ void sc_inverse(const double* a, int D, const int* perm, double* x) {
    const int c = threadIdx.x;
    if (c >= D)
        return;
    for (int r = 0; r < D; ++r) {
        double s = perm[r] == c ? 1.0 : 0.0;
        for (int k = 0; k < r; ++k)
            s -= a[r * D + k] * x[k * D + c];
        x[r * D + c] = s;
    }
    for (int r = D - 1; r >= 0; --r) {
        double s = x[r * D + c];
        for (int k = r + 1; k < D; ++k)
            s -= a[r * D + k] * x[k * D + c];
        x[r * D + c] = s / a[r * D + r];
    }
}

// ---- finalize (:63-77, :105-108, :141-144).  grid: x = model; 64 lanes; LDS: a [D x D], x [D x D], perm [D]
__global__ __launch_bounds__(64) void segclust_finalize_kernel(ScDev m, const double* __restrict__ sums, const int* __restrict__ keep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int D = m.D, model = blockIdx.x, lane = threadIdx.x, cells = D + D * (D + 1) / 2;
    double*   a    = reinterpret_cast<double*>(s_raw);
    double*   x    = a + D * D;
    int*      perm = reinterpret_cast<int*>(x + D * D);
    const double*  s    = sums + (long long)keep[model] * cells;
    const unsigned n    = m.n[model];
    const double   inv  = (double)(1.0f / (float)n);   // inverseNFrames = 1.0F / nFrames_: an f32 division, widened
    double*        mean = m.mean + (long long)model * D;
    double*        var  = m.var + (long long)model * D * D;
    if (lane < D)
        mean[lane] = s[lane] * inv;
    __syncthreads();
    if (lane < D)
        for (int i = 0; i < D; ++i) {
            const double q    = s[D + (i >= lane ? sc_tri(i, lane) : sc_tri(lane, i))] * inv;
            var[i * D + lane] = q - mean[i] * mean[lane];
        }
    int    bumps = 0;
    double logdet = 0.0;
    for (;;) {
        if (lane < D)
            for (int i = 0; i < D; ++i)
                a[i * D + lane] = var[i * D + lane];
        __syncthreads();
        if (sc_lu(a, D, perm, &logdet))
            break;
        if (++bumps > kScMaxBump) {
            if (lane == 0)
                atomicOr(m.fail, 2u);
            return;
        }
        __syncthreads();
        if (lane < D)
            var[lane * D + lane] += 0.1;   // variance_ += 0.1 I, while the LU meets an exact zero pivot
    }
    sc_inverse(a, D, perm, x);
    if (lane < D)
        for (int i = 0; i < D; ++i)
            m.inv[((long long)model * D + i) * D + lane] = x[i * D + lane];
    if (lane == 0) {
        m.logdet[model] = logdet;
        m.like[model]   = (float)logdet * (float)n;   // likelihood_ is an f32: narrowed, then *= nFrames_
        m.bumps[model]  = bumps;
    }
}

// c = sum_i n_i mean_i / sum_i n_i.  one workgroup, lane = dimension
__global__ void segclust_center_kernel(ScDev m) {
    const int d = threadIdx.x;
    if (d >= m.D)
        return;
    double s = 0.0, w = 0.0;
    for (int i = 0; i < m.N; ++i) {
        s += (double)m.n[i] * m.mean[(long long)i * m.D + d];
        w += (double)m.n[i];
    }
    m.center[d] = s / w;
}

// U = [sympack(var + m m^T) | m | 1 | 0 ...], m = mean - c (all lanes of a workgroup call; s_m: D doubles of LDS)
__device__ void sc_pack_u(const ScDev& m, const double* mean, const double* var, double* u, double* s_m) {
    const int D = m.D, K = D * (D + 1) / 2;
    for (int d = threadIdx.x; d < D; d += blockDim.x)
        s_m[d] = mean[d] - m.center[d];
    __syncthreads();
    for (int k = threadIdx.x; k < m.KKp; k += blockDim.x) {
        double v = 0.0;
        if (k < K) {
            int i, j;
            sc_tri_decode(k, &i, &j);
            v = var[i * D + j] + s_m[i] * s_m[j];
        }
        else if (k < K + D)
            v = s_m[k - K];
        else if (k == K + D)
            v = 1.0;
        u[k] = v;
    }
}

// grid: x = model.  V = [P_aa, P_ab + P_ba (a > b) | -(P + P^T) m | m^T P m + logdet + D LN_2PI | 0 ...], P the inverse
__global__ __launch_bounds__(kScThreads) void segclust_pack_kernel(ScDev m) {
    __shared__ double s_m[kScMaxDim], s_q[kScMaxDim];
    const int         D = m.D, K = D * (D + 1) / 2, model = blockIdx.x, tid = threadIdx.x;
    const double*     P = m.inv + (long long)model * D * D;
    sc_pack_u(m, m.mean + (long long)model * D, m.var + (long long)model * D * D, m.U + (long long)model * m.KKp, s_m);
    if (tid < D) {
        double lin = 0.0, quad = 0.0;
        for (int b = 0; b < D; ++b) {
            lin += (P[tid * D + b] + P[b * D + tid]) * s_m[b];
            quad += P[tid * D + b] * s_m[b];
        }
        m.V[(long long)model * m.KKp + K + tid] = -lin;
        s_q[tid]                                = quad * s_m[tid];
    }
    __syncthreads();
    double* v = m.V + (long long)model * m.KKp;
    for (int k = tid; k < m.KKp; k += kScThreads) {
        if (k < K) {
            int i, j;
            sc_tri_decode(k, &i, &j);
            v[k] = i == j ? P[i * D + i] : P[i * D + j] + P[j * D + i];
        }
        else if (k == K + D) {
            double q = 0.0;
            for (int d = 0; d < D; ++d)
                q += s_q[d];
            v[k] = q + m.logdet[model] + (double)D * kScLn2Pi;
        }
        else if (k > K + D)
            v[k] = 0.0;
    }
}

// ---- C = A B^T on the matrix cores.  A [rows x lda], B [cols x ldb], both padded with zeros to whole tiles and stages.
// T = double: R[i][j] = f32(-(A_i . B_j) * 0.5 * n_i) (:122-128), every tile.  T = float: dist[i][j] = -(A_i . B_j), tiles on and below the
// diagonal, cells j < i.  grid: x = tile column, y = tile row; 4 waves, wave w owns the 32 x 32 quarter (w / 2, w % 2) as 2 x 2 instruction tiles.
template<class T>
__global__ __launch_bounds__(kScThreads) void sc_gemm_nt_kernel(const T* __restrict__ A, long long lda, const T* __restrict__ B, long long ldb, int inner,
                                                                int N, const unsigned* __restrict__ n_frames, float* __restrict__ C, long long ldc) {
    constexpr bool f64 = sizeof(T) == 8;
    typedef typename std::conditional<f64, sc_double4, sc_float4>::type Acc;
    __shared__ T s_a[kScTile][kScKc + 1], s_b[kScTile][kScKc + 1];
    if (!f64 && blockIdx.x > blockIdx.y)
        return;
    const int i0 = blockIdx.y * kScTile, j0 = blockIdx.x * kScTile, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wi = (w >> 1) * 32, wj = (w & 1) * 32, l16 = lane & 15, lk = lane >> 4;
    Acc       acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
            acc[a][b] = Acc{0, 0, 0, 0};
    for (int k0 = 0; k0 < inner; k0 += kScKc) {
#pragma unroll
        for (int q = 0; q < kScTile * kScKc / kScThreads; ++q) {
            const int idx = tid + q * kScThreads, r = idx / kScKc, k = idx % kScKc;
            s_a[r][k]     = A[(i0 + r) * lda + k0 + k];
            s_b[r][k]     = B[(j0 + r) * ldb + k0 + k];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kScKc; kk += 4) {
            T av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                av[a] = s_a[wi + a * 16 + l16][kk + lk];
                bv[a] = s_b[wj + a * 16 + l16][kk + lk];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if constexpr (f64)
                        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
                    else
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // the instruction's result layout: f64 keeps row 4 r + lane / 16 in register r, f32 keeps row 4 (lane / 16) + r
                const int i = i0 + wi + a * 16 + (f64 ? 4 * r + lk : 4 * lk + r), j = j0 + wj + b * 16 + l16;
                if (i >= N || j >= N)
                    continue;
                if constexpr (f64) {
                    double x = -(double)acc[a][b][r];
                    x *= 0.5;
                    x *= (double)n_frames[i];
                    C[i * ldc + j] = (float)x;
                }
                else if (j < i)
                    C[i * ldc + j] = -(float)acc[a][b][r];
            }
}

// one step of Math::Vector<f32>::logSum (Math/Vector.hh:187-201): the reference's own rule, the branch diff > MINLOGEPS does nothing
__device__ inline float sc_logsum_step(float sum, float x) {
    const float diff = sum - x;
    if (diff > kScMinLogEps)
        return sum;
    if (diff < -kScMinLogEps)
        return x;
    if (diff < 0)
        return (float)((double)x + log(1.0 + exp((double)diff)));
    return (float)((double)sum + log(1.0 + exp(-(double)diff)));
}

// ---- rows of alpha R: lane = row, 64 rows per workgroup, tiles of R through LDS.  term (nullable): exp(alpha R[i][i] - logSum_i) of the alpha
// search (.hh:579-591); F (nullable): the feature rows exp(alpha R[i][.] - logSum_i) (:166-175)
__global__ __launch_bounds__(64) void segclust_rows_kernel(const float* __restrict__ R, long long ldr, int N, float alpha, double* __restrict__ term,
                                                           float* __restrict__ F, long long ldf) {
    __shared__ float s[64][65];
    const int        row0 = blockIdx.x * 64, tid = threadIdx.x, i = row0 + tid;
    float            sum = 0.f;
    for (int j0 = 0; j0 < N; j0 += 64) {
        for (int q = 0; q < 64; ++q)
            s[q][tid] = R[(row0 + q) * ldr + j0 + tid];
        __syncthreads();
        const int nj = N - j0 < 64 ? N - j0 : 64;
        if (i < N)
            for (int jj = 0; jj < nj; ++jj) {
                const float v = s[tid][jj] * alpha;
                sum           = j0 + jj == 0 ? v : sc_logsum_step(sum, v);
            }
        __syncthreads();
    }
    if (term && i < N)
        term[i] = exp((double)(R[i * ldr + i] * alpha - sum));
    if (!F)
        return;
    for (int j0 = 0; j0 < N; j0 += 64) {
        for (int q = 0; q < 64; ++q)
            s[q][tid] = R[(row0 + q) * ldr + j0 + tid];
        __syncthreads();
        for (int jj = 0; jj < 64; ++jj)
            s[tid][jj] = (float)exp((double)(s[tid][jj] * alpha - sum));
        __syncthreads();
        for (int q = 0; q < 64; ++q)
            if (row0 + q < N && j0 + tid < N)
                F[(row0 + q) * ldf + j0 + tid] = s[q][tid];
        __syncthreads();
    }
}

// ---- the merge loop
// (value, index) minimum of a wave, the smaller index among equal values; every lane gets the result
__device__ inline void sc_wave_min(float* v, int* idx) {
#pragma unroll
    for (int m = 32; m; m >>= 1) {
        const float ov = __shfl_xor(*v, m);
        const int   oi = __shfl_xor(*idx, m);
        if (ov < *v || (ov == *v && oi < *idx))
            *v = ov, *idx = oi;
    }
}

__device__ inline float* sc_cell(const ScDev& m, int a, int b) {   // the cell of the pair in the lower triangle
    return m.dist + (long long)(a > b ? a : b) * m.ld + (a > b ? b : a);
}

// the minimum of row i over the active j < i by one wave, findBestPair's order within the row; column `col` (if >= 0) reads `val` instead
__device__ inline void sc_row_scan(const ScDev& m, int i, int col, float val, float* v, int* j) {
    float bv = INFINITY;
    int   bj = 0x7fffffff;
    for (int c = threadIdx.x & 63; c < i; c += 64) {
        if (!m.active[c])
            continue;
        const float d = c == col ? val : m.dist[(long long)i * m.ld + c];
        if (d < bv)
            bv = d, bj = c;
    }
    sc_wave_min(&bv, &bj);
    *v = bv, *j = bj;
}

// grid: x = 4 rows; wave = row
__global__ __launch_bounds__(kScThreads) void segclust_rowmin_kernel(ScDev m) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m.N)
        return;
    float v;
    int   j;
    sc_row_scan(m, i, -1, 0.f, &v, &j);
    if ((threadIdx.x & 63) == 0)
        m.row_v[i] = v, m.row_j[i] = j;
}

// findBestPair (.hh:671-682) over the cached row minima: the strict minimum, i ascending, then j ascending.  One workgroup.  After a merge
// the parent's row is rescanned first: its cells were written by the update kernel's other waves.
__global__ __launch_bounds__(kScThreads) void segclust_argmin_kernel(ScDev m, int step) {
    __shared__ float s_v[4];
    __shared__ int   s_i[4];
    const int        tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (step > 0 && m.state[0] >= 0) {
        const int p  = m.state[0];
        float     bv = INFINITY;
        int       bj = 0x7fffffff;
        for (int c = tid; c < p; c += kScThreads) {
            if (!m.active[c])
                continue;
            const float d = m.dist[(long long)p * m.ld + c];
            if (d < bv)
                bv = d, bj = c;
        }
        sc_wave_min(&bv, &bj);
        if (lane == 0)
            s_v[w] = bv, s_i[w] = bj;
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < 4; ++q)
                if (s_v[q] < bv || (s_v[q] == bv && s_i[q] < bj))
                    bv = s_v[q], bj = s_i[q];
            m.row_v[p] = bv, m.row_j[p] = bj;
        }
        __syncthreads();
    }
    float bv = INFINITY;
    int   bi = 0x7fffffff;
    for (int i = 1 + tid; i < m.N; i += kScThreads)
        if (m.active[i] && m.row_v[i] < bv)
            bv = m.row_v[i], bi = i;
    sc_wave_min(&bv, &bi);
    if (lane == 0)
        s_v[w] = bv, s_i[w] = bi;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < 4; ++q)
            if (s_v[q] < bv || (s_v[q] == bv && s_i[q] < bi))
                bv = s_v[q], bi = s_i[q];
        const bool found = bi < m.N;   // not found: nothing finite is left (NaN distances); the merge kernel reports it
        m.state[0]       = found ? m.row_j[bi] : -1;
        m.state[1]       = found ? bi : -1;
    }
}

// condenseDistMatrix's model part (:79-103, :137-150, .hh:727-735): merged mean, variance, log-determinant, GLR, the tracker record, and the
// U of the merged model for the refresh.  One wave; LDS: a [D x D], perm [D]
__global__ __launch_bounds__(64) void segclust_merge_kernel(ScDev m, int step) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_mean[kScMaxDim], s_dx[kScMaxDim], s_dy[kScMaxDim];
    const int         D = m.D, lane = threadIdx.x, p = m.state[0], c = m.state[1];
    double*           a    = reinterpret_cast<double*>(s_raw);
    int*              perm = reinterpret_cast<int*>(a + D * D);
    if (p < 0 || c < 0 || (*m.fail & 4u)) {
        if (lane == 0)
            atomicOr(m.fail, 4u);
        return;
    }
    const unsigned nx = m.n[p], ny = m.n[c], nn = nx + ny;
    double*        mean = m.mean + (long long)p * D;
    double*        vx   = m.var + (long long)p * D * D;
    const double*  vy   = m.var + (long long)c * D * D;
    if (lane < D) {
        const double mx = mean[lane], my = m.mean[(long long)c * D + lane];
        double       v = mx * (double)nx;
        const double t = my * (double)ny;
        v += t;
        v *= (double)(1.0f / (float)nn);   // mean_ *= (1.0F / nFrames_)
        s_mean[lane] = v, s_dx[lane] = mx - v, s_dy[lane] = my - v;
    }
    __syncthreads();
    const double wx = (double)nx / (double)nn, wy = (double)ny / (double)nn;
    if (lane < D) {
        for (int i = 0; i < D; ++i) {
            double v = s_dx[i] * s_dx[lane];
            v += vx[i * D + lane];
            v *= wx;
            double t = s_dy[i] * s_dy[lane];
            t += vy[i * D + lane];
            t *= wy;
            v += t;
            vx[i * D + lane] = v;
            a[i * D + lane]  = v;
        }
        mean[lane] = s_mean[lane];
    }
    __syncthreads();
    double     logdet = 0.0;
    const bool ok     = sc_lu(a, D, perm, &logdet);
    if (lane == 0) {
        if (!ok)
            atomicOr(m.fail, 8u);   // the reference's critical LAPACK error
        float L = (float)logdet;
        L *= (float)nn;
        const float glr = 0.5f * (L - m.like[p] - m.like[c]);
        m.like[p]       = L;
        m.n[p]          = nn;
        m.active[c]     = 0;
        m.tr_parent[step] = p, m.tr_child[step] = c, m.tr_score[step] = glr - m.threshold;
    }
    __syncthreads();
    sc_pack_u(m, mean, vx, m.u_new, s_dx);
}

// R(merged | j) for every original model j: wave = column.  grid: x = 4 columns
__global__ __launch_bounds__(kScThreads) void segclust_refresh_kernel(ScDev m) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= m.N || m.state[0] < 0)
        return;
    const double* v = m.V + (long long)j * m.KKp;
    double        s = 0.0;
    for (int k = lane; k < m.KKp; k += 64)
        s += m.u_new[k] * v[k];
#pragma unroll
    for (int q = 32; q; q >>= 1)
        s += __shfl_xor(s, q);
    if (lane == 0) {
        double x = -s;
        x *= 0.5;
        x *= (double)m.n[m.state[0]];
        m.r_new[j] = (float)x;
    }
}

// the merged model's feature row (:166-175): the logSum chain is one lane's, over the row in LDS.  One workgroup; LDS: N floats
__global__ __launch_bounds__(kScThreads) void segclust_featrow_kernel(ScDev m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ float s_sum;
    float*           s = reinterpret_cast<float*>(s_raw);
    const int        p = m.state[0];
    if (p < 0)
        return;
    for (int j = threadIdx.x; j < m.N; j += kScThreads)
        s[j] = m.r_new[j] * m.alpha;
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = s[0];
        for (int j = 1; j < m.N; ++j)
            sum = sc_logsum_step(sum, s[j]);
        s_sum = sum;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < m.N; j += kScThreads)
        m.F[(long long)p * m.ld + j] = (float)exp((double)(s[j] - s_sum));
}

// updateDistMat (.hh:684-716) and the cached row minima.  wave = active row i != parent.  concatenation: the correlation distance of i and the
// merged parent; max linkage: the larger of i's distances to parent and child.  grid: x = 4 rows
template<bool MAXLINK>
__global__ __launch_bounds__(kScThreads) void segclust_update_kernel(ScDev m) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, p = m.state[0], c = m.state[1];
    if (i >= m.N || p < 0 || i == p || !m.active[i])
        return;
    float d;
    if (MAXLINK)
        d = fmaxf(*sc_cell(m, i, p), *sc_cell(m, i, c));
    else {
        const float *fi = m.F + (long long)i * m.ld, *fp = m.F + (long long)p * m.ld;
        float        s  = 0.f;
        for (int k = lane; k < m.N; k += 64)
            s += fi[k] * fp[k];
#pragma unroll
        for (int q = 32; q; q >>= 1)
            s += __shfl_xor(s, q);
        d = -s;
    }
    if (i < p) {   // a cell of the parent's row: the next argmin rescans that row
        if (lane == 0)
            *sc_cell(m, i, p) = d;
        return;
    }
    float v = m.row_v[i];
    int   j = m.row_j[i];
    if (j == p || j == c)
        sc_row_scan(m, i, p, d, &v, &j);
    else if (d < v || (d == v && p < j))
        v = d, j = p;
    if (lane == 0) {
        *sc_cell(m, i, p) = d;
        m.row_v[i] = v, m.row_j[i] = j;
    }
}

// fills (no memset node in case a caller captures the stream)
template<class T>
__global__ void sc_fill_kernel(T* p, long long n, T v) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        p[i] = v;
}

template<class T>
static int sc_fill(hipStream_t st, T* p, long long n, T v) {
    if (n <= 0)
        return AMX_OK;
    hipLaunchKernelGGL(sc_fill_kernel<T>, dim3((unsigned)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0, st, p, n, v);
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

}  // namespace amx

struct amx_segclust {
    amx_ctx*               ctx = nullptr;
    int                    D = 0, device = 0, keep_debug = 0;
    std::vector<long long> frames;   // per accumulated segment
    amx::DevBuf<double>    d_sums;   // [segments x (D + K)]
    size_t                 sums_cap = 0;
    amx::DevBuf<long long> d_off;
    amx::DevBuf<unsigned>  d_flags;  // [0] non-finite feature, [1] failures of a clustering
    // a clustering's workspace
    int                    N = 0, Np = 0, KKp = 0;
    amx::DevBuf<int>       d_int;    // keep, bumps, active, row_j, tr_parent, tr_child, state
    amx::DevBuf<unsigned>  d_n;
    amx::DevBuf<float>     d_f32;    // like, row_v, tr_score, r_new
    amx::DevBuf<double>    d_f64;    // mean, var, inv, logdet, center, u_new, term
    amx::DevBuf<double>    d_U, d_V;
    amx::DevBuf<float>     d_R, d_F, d_dist;
    // kept for amx_segclust_debug_read when keep_debug
    std::vector<double>    dbg_models;
    std::vector<float>     dbg_dist;
    bool                   have_R = false;
};

extern "C" {

int amx_segclust_create(amx_ctx* ctx, int dim, amx_segclust** out) {
    const char* who = "amx_segclust_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(dim >= 1 && dim <= amx::kScMaxDim, AMX_ERR_UNSUPPORTED, "%s: dim %d is outside 1...%d", who, dim, amx::kScMaxDim);
    std::unique_ptr<amx_segclust> h(new amx_segclust);
    h->ctx = ctx, h->D = dim;
    if (ctx) {
        h->device = ctx->device;
        AMX_HIP(hipSetDevice(h->device));
        AMX_TRY(h->d_flags.reserve(2));
    }
    *out = h.release();
    return AMX_OK;
}

void amx_segclust_destroy(amx_segclust* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->device);
    delete h;
}

void amx_segclust_kernel_shape(int* stage_frames, int* tile_cells, int* gemm_tile, int* gemm_stage) {
    if (stage_frames)
        *stage_frames = amx::kScStage;
    if (tile_cells)
        *tile_cells = amx::kScThreads;
    if (gemm_tile)
        *gemm_tile = amx::kScTile;
    if (gemm_stage)
        *gemm_stage = amx::kScKc;
}

long amx_segclust_segments(const amx_segclust* h) {
    return h ? (long)h->frames.size() : 0;
}

int amx_segclust_reset(amx_segclust* h) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_segclust_reset: NULL handle");
    h->frames.clear();
    h->have_R = false;
    return AMX_OK;
}

int amx_segclust_set_debug(amx_segclust* h, int keep) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_segclust_set_debug: NULL handle");
    h->keep_debug = keep != 0;
    return AMX_OK;
}

int amx_segclust_accumulate_dev(amx_segclust* h, const float* feats_dev, int feats_ld, int n_seg, const long* frame_offsets) {
    const char* who = "amx_segclust_accumulate_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: host-only handle (created without a context)", who);
    AMX_REQUIRE(n_seg >= 0 && feats_ld >= h->D, AMX_ERR_INVALID, "%s: n_seg %d, feats_ld %d (dim %d)", who, n_seg, feats_ld, h->D);
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(frame_offsets && feats_dev, AMX_ERR_INVALID, "%s: NULL feats_dev or frame_offsets", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: frame_offsets[0] = %ld is negative", who, frame_offsets[0]);
    for (int s = 0; s < n_seg; ++s) {
        AMX_REQUIRE(frame_offsets[s + 1] > frame_offsets[s], AMX_ERR_INVALID, "%s: segment %d has no frames (offsets %ld, %ld)", who, s, frame_offsets[s],
                    frame_offsets[s + 1]);
        AMX_REQUIRE(frame_offsets[s + 1] - frame_offsets[s] < (1ll << 32), AMX_ERR_INVALID, "%s: segment %d has more frames than a u32 counts", who, s);
    }
    const size_t S = h->frames.size();
    AMX_REQUIRE(S + n_seg <= 65535, AMX_ERR_UNSUPPORTED, "%s: more than 65535 segments accumulated", who);
    AMX_HIP(hipSetDevice(h->device));
    hipStream_t  st    = h->ctx->stream;
    const int    cells = h->D + h->D * (h->D + 1) / 2;
    const size_t need  = (S + n_seg) * cells;
    if (need > h->d_sums.capacity()) {   // grow, keeping what earlier calls appended
        amx::DevBuf<double> grown;
        AMX_TRY(grown.reserve(std::max(need, 2 * h->d_sums.capacity())));
        if (S)
            AMX_HIP(hipMemcpyAsync(grown.get(), h->d_sums.get(), S * cells * sizeof(double), hipMemcpyDeviceToDevice, st));
        AMX_HIP(hipStreamSynchronize(st));
        h->d_sums = std::move(grown);
    }
    std::vector<long long> off(frame_offsets, frame_offsets + n_seg + 1);
    AMX_TRY(h->d_off.reserve(off.size()));
    AMX_HIP(hipMemcpyAsync(h->d_off.get(), off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    AMX_TRY(amx::sc_fill(st, h->d_flags.get(), 2, 0u));
    {
        amx::ScopedKernelTimer timer(h->ctx, "segclust_acc");
        hipLaunchKernelGGL(amx::segclust_acc_kernel, dim3((unsigned)amx::ceil_div(cells, amx::kScThreads), (unsigned)n_seg), dim3(amx::kScThreads), 0, st,
                           feats_dev, (long long)feats_ld, h->D, (const long long*)h->d_off.get(), h->d_sums.get() + S * cells, cells, h->d_flags.get());
        AMX_HIP(hipGetLastError());
    }
    unsigned bad = 0;
    AMX_HIP(hipMemcpyAsync(&bad, h->d_flags.get(), sizeof bad, hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    AMX_REQUIRE(!bad, AMX_ERR_INVALID, "%s: a feature is not finite; the call's segments are not appended", who);
    for (int s = 0; s < n_seg; ++s)
        h->frames.push_back(off[s + 1] - off[s]);
    h->have_R = false;
    return AMX_OK;
}

int amx_segclust_cluster(amx_segclust* h, const amx_segclust_cfg* cfg, int32_t* class_ids, int32_t* tracker_parent, int32_t* tracker_child,
                         float* tracker_score, amx_segclust_info* info) {
    const char* who = "amx_segclust_cluster";
    AMX_REQUIRE(h && cfg, AMX_ERR_INVALID, "%s: NULL handle or cfg", who);
    AMX_REQUIRE(!cfg->infile || !cfg->infile[0], AMX_ERR_UNSUPPORTED, "%s: infile (a predefined clustering) is not built", who);
    AMX_REQUIRE(cfg->minframes >= 0 && cfg->mincluster >= 1 && cfg->maxcluster >= 1 && (cfg->amalgamation == 0 || cfg->amalgamation == 1) &&
                        std::isfinite(cfg->threshold) && std::isfinite(cfg->lambda) && std::isfinite(cfg->alpha) && std::isfinite(cfg->minalpha) &&
                        std::isfinite(cfg->maxalpha),
                AMX_ERR_INVALID, "%s: bad configuration (minframes %d, mincluster %d, maxcluster %d, amalgamation %d, or a value that is not finite)", who,
                cfg->minframes, cfg->mincluster, cfg->maxcluster, cfg->amalgamation);
    const int S = (int)h->frames.size(), D = h->D;
    std::vector<int>      keep;
    std::vector<unsigned> n_frames;
    unsigned              total = 0;
    for (int s = 0; s < S; ++s)
        if (h->frames[s] >= cfg->minframes) {
            keep.push_back(s);
            n_frames.push_back((unsigned)h->frames[s]);
            total += (unsigned)h->frames[s];
        }
    const int N = (int)keep.size();
    AMX_REQUIRE(N >= 1, AMX_ERR_INVALID, "%s: no segments received for clustering (%d accumulated, minframes %d)", who, S, cfg->minframes);
    AMX_REQUIRE(N <= amx::kScMaxSeg, AMX_ERR_UNSUPPORTED, "%s: %d segments after the minframes filter are more than %d", who, N, amx::kScMaxSeg);
    AMX_REQUIRE(cfg->mincluster <= N, AMX_ERR_UNSUPPORTED, "%s: mincluster %d is larger than the %d segments (the reference's unsigned difference wraps)", who,
                cfg->mincluster, N);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: host-only handle (created without a context)", who);
    AMX_REQUIRE(class_ids, AMX_ERR_INVALID, "%s: NULL class_ids", who);
    // threshold_ += complexity * lambda * log((f32)totalframes), f32 throughout (.hh:570-576)
    float penalty = 0.25f * (float)D * (3.0f + (float)D);
    penalty *= cfg->lambda;
    penalty *= std::log((float)total);
    const float threshold = cfg->threshold + penalty;

    AMX_HIP(hipSetDevice(h->device));
    hipStream_t st = h->ctx->stream;
    const int   K = D * (D + 1) / 2, T = amx::kScTile;
    const int   Np = (N + T - 1) / T * T, KKp = (K + D + 1 + amx::kScKc - 1) / amx::kScKc * amx::kScKc;
    h->N = N, h->Np = Np, h->KKp = KKp, h->have_R = false;
    AMX_TRY(h->d_int.reserve((size_t)6 * N + 2));
    AMX_TRY(h->d_n.reserve(N));
    AMX_TRY(h->d_f32.reserve((size_t)4 * N));
    AMX_TRY(h->d_f64.reserve((size_t)N * (D + 2 * D * D + 2) + D + KKp));
    AMX_TRY(h->d_U.reserve((size_t)Np * KKp));
    AMX_TRY(h->d_V.reserve((size_t)Np * KKp));
    AMX_TRY(h->d_R.reserve((size_t)Np * Np));
    AMX_TRY(h->d_F.reserve((size_t)Np * Np));
    AMX_TRY(h->d_dist.reserve((size_t)Np * Np));
    amx::ScDev m{};
    m.D = D, m.N = N, m.KKp = KKp, m.ld = Np, m.threshold = threshold;
    int* ip    = h->d_int.get();
    int* keepd = ip;
    m.bumps = ip + N, m.active = ip + 2 * N, m.row_j = ip + 3 * N, m.tr_parent = ip + 4 * N, m.tr_child = ip + 5 * N, m.state = ip + 6 * N;
    m.n     = h->d_n.get();
    float* fp = h->d_f32.get();
    m.like = fp, m.row_v = fp + N, m.tr_score = fp + 2 * N, m.r_new = fp + 3 * N;
    double* dp = h->d_f64.get();
    m.mean = dp, m.var = m.mean + (size_t)N * D, m.inv = m.var + (size_t)N * D * D, m.logdet = m.inv + (size_t)N * D * D, m.center = m.logdet + N;
    m.u_new = m.center + D;
    double* term = m.u_new + KKp;
    m.U = h->d_U.get(), m.V = h->d_V.get(), m.F = h->d_F.get(), m.dist = h->d_dist.get(), m.fail = h->d_flags.get() + 1;

    AMX_HIP(hipMemcpyAsync(keepd, keep.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(m.n, n_frames.data(), (size_t)N * sizeof(unsigned), hipMemcpyHostToDevice, st));
    AMX_TRY(amx::sc_fill(st, h->d_flags.get(), 2, 0u));
    AMX_TRY(amx::sc_fill(st, m.active, N, 1));
    AMX_TRY(amx::sc_fill(st, m.U, (long long)Np * KKp, 0.0));
    AMX_TRY(amx::sc_fill(st, m.V, (long long)Np * KKp, 0.0));
    AMX_TRY(amx::sc_fill(st, h->d_R.get(), (long long)Np * Np, 0.f));
    AMX_TRY(amx::sc_fill(st, m.F, (long long)Np * Np, 0.f));
    const size_t lds_lu = (size_t)2 * D * D * sizeof(double) + D * sizeof(int);
    {
        amx::ScopedKernelTimer timer(h->ctx, "segclust_finalize");
        hipLaunchKernelGGL(amx::segclust_finalize_kernel, dim3(N), dim3(64), lds_lu, st, m, (const double*)h->d_sums.get(), (const int*)keepd);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(h->ctx, "segclust_pack");
        hipLaunchKernelGGL(amx::segclust_center_kernel, dim3(1), dim3(64), 0, st, m);
        hipLaunchKernelGGL(amx::segclust_pack_kernel, dim3(N), dim3(amx::kScThreads), 0, st, m);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(h->ctx, "segclust_r_gemm");
        hipLaunchKernelGGL(amx::sc_gemm_nt_kernel<double>, dim3(Np / T, Np / T), dim3(amx::kScThreads), 0, st, (const double*)m.U, (long long)KKp,
                           (const double*)m.V, (long long)KKp, KKp, N, (const unsigned*)m.n, h->d_R.get(), (long long)Np);
        AMX_HIP(hipGetLastError());
    }
    std::vector<int> bumps(N);
    unsigned         fail = 0;
    AMX_HIP(hipMemcpyAsync(bumps.data(), m.bumps, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
    AMX_HIP(hipMemcpyAsync(&fail, m.fail, sizeof fail, hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    AMX_REQUIRE(!(fail & 2u), AMX_ERR_INVALID, "%s: a segment's covariance stays singular after %d rounds of +0.1", who, amx::kScMaxBump);
    h->have_R = true;
    if (h->keep_debug) {
        h->dbg_models.resize((size_t)N * (D + D * D + 1));
        std::vector<double> tmp((size_t)N * (D + D * D + 1));
        AMX_HIP(hipMemcpy(tmp.data(), m.mean, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost));
        AMX_HIP(hipMemcpy(tmp.data() + (size_t)N * D, m.var, (size_t)N * D * D * sizeof(double), hipMemcpyDeviceToHost));
        AMX_HIP(hipMemcpy(tmp.data() + (size_t)N * (D + D * D), m.logdet, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i) {
            double* o = h->dbg_models.data() + (size_t)i * (D + D * D + 1);
            std::copy(tmp.begin() + (size_t)i * D, tmp.begin() + (size_t)(i + 1) * D, o);
            std::copy(tmp.begin() + (size_t)N * D + (size_t)i * D * D, tmp.begin() + (size_t)N * D + (size_t)(i + 1) * D * D, o + D);
            o[D + D * D] = tmp[(size_t)N * (D + D * D) + i];
        }
    }

    // alpha (.hh:607-645): bisection from 0 with step 0.5 on the average of the rows' terms; the rows are the device's, the f32 average the host's
    float alpha = cfg->alpha;
    int   alpha_iterations = 0;
    if (alpha < 0) {
        std::vector<double> terms(N);
        float               step = 0.5f, average = 0.f;
        alpha = 0.f;
        for (;;) {
            uint32_t bits;
            std::memcpy(&bits, &step, sizeof bits);
            if (!((average < cfg->minalpha || average > cfg->maxalpha) && bits > 100u))   // !isAlmostEqualUlp(step, 0.0f, 100)
                break;
            alpha = average < cfg->minalpha ? alpha + step : alpha - step;
            step  = (float)(step / 2.0);
            {
                amx::ScopedKernelTimer timer(h->ctx, "segclust_rows");
                hipLaunchKernelGGL(amx::segclust_rows_kernel, dim3(Np / 64), dim3(64), 0, st, (const float*)h->d_R.get(), (long long)Np, N, alpha, term,
                                   (float*)nullptr, (long long)Np);
                AMX_HIP(hipGetLastError());
            }
            AMX_HIP(hipMemcpyAsync(terms.data(), term, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
            AMX_HIP(hipStreamSynchronize(st));
            float sum = 0.f;
            for (int i = 0; i < N; ++i)
                sum = (float)((double)sum + terms[i]);   // total += exp(.): the sum of an f32 and a double, narrowed
            average = sum / (float)N;
            ++alpha_iterations;
        }
    }
    m.alpha = alpha;
    {
        amx::ScopedKernelTimer timer(h->ctx, "segclust_rows");
        hipLaunchKernelGGL(amx::segclust_rows_kernel, dim3(Np / 64), dim3(64), 0, st, (const float*)h->d_R.get(), (long long)Np, N, alpha, (double*)nullptr, m.F,
                           (long long)Np);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(h->ctx, "segclust_dist_gemm");
        hipLaunchKernelGGL(amx::sc_gemm_nt_kernel<float>, dim3(Np / T, Np / T), dim3(amx::kScThreads), 0, st, (const float*)m.F, (long long)Np,
                           (const float*)m.F, (long long)Np, Np, N, (const unsigned*)nullptr, m.dist, (long long)Np);
        AMX_HIP(hipGetLastError());
    }
    if (h->keep_debug) {
        h->dbg_dist.assign((size_t)N * N, 0.f);
        AMX_HIP(hipMemcpy2DAsync(h->dbg_dist.data(), (size_t)N * sizeof(float), m.dist, (size_t)Np * sizeof(float), (size_t)N * sizeof(float), N,
                                 hipMemcpyDeviceToHost, st));
        AMX_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < N; ++i)   // the cells on and above the diagonal are never written
            std::fill(h->dbg_dist.begin() + (size_t)i * N + i, h->dbg_dist.begin() + (size_t)(i + 1) * N, 0.f);
    }

    // the merge loop: N - 1 rounds enqueued, one synchronisation
    {
        amx::ScopedKernelTimer timer(h->ctx, "segclust_loop");
        hipLaunchKernelGGL(amx::segclust_rowmin_kernel, dim3((N + 3) / 4), dim3(amx::kScThreads), 0, st, m);
        const size_t lds_merge = (size_t)D * D * sizeof(double) + D * sizeof(int);
        for (int step = 0; step < N - 1; ++step) {
            hipLaunchKernelGGL(amx::segclust_argmin_kernel, dim3(1), dim3(amx::kScThreads), 0, st, m, step);
            hipLaunchKernelGGL(amx::segclust_merge_kernel, dim3(1), dim3(64), lds_merge, st, m, step);
            if (cfg->amalgamation == 1)
                hipLaunchKernelGGL(amx::segclust_update_kernel<true>, dim3((N + 3) / 4), dim3(amx::kScThreads), 0, st, m);
            else {
                hipLaunchKernelGGL(amx::segclust_refresh_kernel, dim3((N + 3) / 4), dim3(amx::kScThreads), 0, st, m);
                hipLaunchKernelGGL(amx::segclust_featrow_kernel, dim3(1), dim3(amx::kScThreads), (size_t)N * sizeof(float), st, m);
                hipLaunchKernelGGL(amx::segclust_update_kernel<false>, dim3((N + 3) / 4), dim3(amx::kScThreads), 0, st, m);
            }
        }
        AMX_HIP(hipGetLastError());
    }
    std::vector<int32_t> tp(std::max(N - 1, 1)), tc(std::max(N - 1, 1));
    std::vector<float>   ts(std::max(N - 1, 1));
    if (N > 1) {
        AMX_HIP(hipMemcpyAsync(tp.data(), m.tr_parent, (size_t)(N - 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        AMX_HIP(hipMemcpyAsync(tc.data(), m.tr_child, (size_t)(N - 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        AMX_HIP(hipMemcpyAsync(ts.data(), m.tr_score, (size_t)(N - 1) * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    AMX_HIP(hipMemcpyAsync(&fail, m.fail, sizeof fail, hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    AMX_REQUIRE(!(fail & 4u), AMX_ERR_INVALID, "%s: no finite distance is left to merge on", who);
    AMX_REQUIRE(!(fail & 8u), AMX_ERR_INVALID, "%s: the LU of a merged covariance meets a zero pivot", who);

    std::vector<int32_t> ids(N);
    int                  n_clusters = 0, best = -1;
    AMX_TRY(amx_segclust_choose(N, tp.data(), tc.data(), ts.data(), cfg->mincluster, cfg->maxcluster, ids.data(), &n_clusters, &best));
    const int shift = N < S ? 1 : 0;   // printClustering: with a default cluster every other id moves up by one
    std::fill(class_ids, class_ids + S, 0);
    for (int i = 0; i < N; ++i)
        class_ids[keep[i]] = ids[i] + shift;
    if (N > 1) {
        if (tracker_parent)
            std::copy(tp.begin(), tp.begin() + N - 1, tracker_parent);
        if (tracker_child)
            std::copy(tc.begin(), tc.begin() + N - 1, tracker_child);
        if (tracker_score)
            std::copy(ts.begin(), ts.begin() + N - 1, tracker_score);
    }
    if (info) {
        info->n_segments = N, info->n_filtered = S - N, info->n_clusters = n_clusters, info->best_index = best;
        info->n_regularised = (int)std::count_if(bumps.begin(), bumps.end(), [](int b) { return b > 0; });
        info->alpha = alpha, info->threshold = threshold, info->alpha_iterations = alpha_iterations;
    }
    return AMX_OK;
}

long amx_segclust_debug_read(amx_segclust* h, int what, void* out, long capacity) {
    const char* who = "amx_segclust_debug_read";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    const int D = h->D, cells = D + D * (D + 1) / 2, N = h->N;
    long      n = 0;
    if (what == AMX_SEGCLUST_DEBUG_SUMS)
        n = (long)h->frames.size() * cells;
    else if (what == AMX_SEGCLUST_DEBUG_R) {
        AMX_REQUIRE(h->have_R, AMX_ERR_STATE, "%s: no clustering has run since the last segment was appended", who);
        n = (long)N * N;
    }
    else if (what == AMX_SEGCLUST_DEBUG_DIST || what == AMX_SEGCLUST_DEBUG_MODELS) {
        AMX_REQUIRE(h->have_R && h->keep_debug, AMX_ERR_STATE, "%s: no clustering has run under amx_segclust_set_debug(h, 1)", who);
        n = what == AMX_SEGCLUST_DEBUG_DIST ? (long)h->dbg_dist.size() : (long)h->dbg_models.size();
    }
    else
        AMX_REQUIRE(false, AMX_ERR_INVALID, "%s: unknown item %d", who, what);
    if (!out || capacity < n || n == 0)
        return n;
    if (what == AMX_SEGCLUST_DEBUG_SUMS) {
        AMX_HIP(hipSetDevice(h->device));
        AMX_HIP(hipMemcpy(out, h->d_sums.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    }
    else if (what == AMX_SEGCLUST_DEBUG_R) {
        AMX_HIP(hipSetDevice(h->device));
        AMX_HIP(hipMemcpy2D(out, (size_t)N * sizeof(float), h->d_R.get(), (size_t)h->Np * sizeof(float), (size_t)N * sizeof(float), N, hipMemcpyDeviceToHost));
    }
    else if (what == AMX_SEGCLUST_DEBUG_DIST)
        std::memcpy(out, h->dbg_dist.data(), (size_t)n * sizeof(float));
    else
        std::memcpy(out, h->dbg_models.data(), (size_t)n * sizeof(double));
    return n;
}

}  // extern "C"
