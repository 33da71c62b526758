// scatter.hip -- LDA scatter-matrix estimation (Signal::ScatterMatricesEstimator, src/Signal/ScatterEstimator.cc): the corpus pass on
// the device, the accumulator file and the finalize step on the host.
//
// The accumulator is ONE flat f64 buffer, in the order of the reference's accumulator file behind its two u32 headers
// (ScatterEstimator.cc:95-106, 359-376):
//   [dim (dim + 1) / 2  vectorSquareSum_, lower triangle, row-major] [n_classes x dim  vectorSums_] [n_classes  counts_]
//
// Arithmetic of one frame x (f32) of class c with weight w (f32), ScatterEstimator.cc:44-55, 227-234:
//   square[i][j] += (f64)((x_i * x_j) * w)   for j <= i: both products are f32 operations, rounded in that order, then widened
//   sums[c][i]   += (f64)(x_i * w)            (x * weight is a Math::Vector<f32>)
//   counts[c]    += (f64)w
// No multiply feeds an add without a conversion in between, so there is nothing for -ffp-contract to fuse: both contracts of the
// reference compute the same bits (tests/golden/ref_scatter.npz records that), and amx_set_contract changes nothing here.
// Sums across workgroups are f64 atomics like every training sum of this library: order undefined, exact where no addition rounds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"

namespace amx {

constexpr int kScatterBlock  = 64;  // components per side of a square-sum block: 256 lanes x (4 x 4) f64 sums
constexpr int kScatterStage  = 64;  // frames staged in LDS at a time; a frame chunk is a whole number of stages
constexpr int kScatterGroups = 4;   // workgroups per CU the square-sum grid aims at (32 KB of LDS each)

// ---- square sum.  blockIdx.x = block of the lower triangle (bi >= bj), blockIdx.y = frame chunk [y * chunk, (y + 1) * chunk).
// The workgroup stages components [bi * 64, +64) and [bj * 64, +64) of 64 frames in LDS (a skipped frame and a component >= dim as
// zeros: they add +0), lane (ty, tx) keeps rows ty * 4 .. + 3 x columns tx * 4 .. + 3 of the block in registers.  At the end the
// block goes through LDS so that each wave adds whole rows: 64 consecutive doubles per atomic wave-instruction, four rows in
// flight per workgroup.  Blocks on the diagonal add only j <= i.
template<bool WEIGHTED>
__global__ __launch_bounds__(256) void scatter_square_kernel(const float* __restrict__ feats, int in_ld, long T, int dim,
                                                             const uint32_t* __restrict__ cls, uint32_t n_classes,
                                                             const float* __restrict__ weight, int chunk, double* __restrict__ acc) {
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[kScatterBlock * kScatterBlock * sizeof(double)];
    __shared__ float                                      s_w[kScatterStage];
    float(*s_x)[2 * kScatterBlock] = reinterpret_cast<float(*)[2 * kScatterBlock]>(s_raw);  // [stage frame][i range | j range], 32 KB
    double(*s_t)[kScatterBlock]    = reinterpret_cast<double(*)[kScatterBlock]>(s_raw);     // the block on its way out, 32 KB

    // blockIdx.x -> (bi, bj), bj <= bi, in row-major order of the triangle
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x)
        ++bi;
    const int bj  = (int)blockIdx.x - bi * (bi + 1) / 2;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

    const long t_begin = (long)blockIdx.y * chunk;
    const long t_end   = t_begin + chunk < T ? t_begin + chunk : T;

    double sum[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            sum[r][c] = 0.0;

    const int col  = tid & 127;  // staging: this thread's column of s_x, frames tid / 128, + 2, + 4, ...
    const int comp = (col < kScatterBlock ? bi * kScatterBlock : bj * kScatterBlock - kScatterBlock) + col;
    for (long t0 = t_begin; t0 < t_end; t0 += kScatterStage) {
        if (tid < kScatterStage) {
            const long t    = t0 + tid;
            const bool keep = t < t_end && cls[t] < n_classes;
            s_w[tid]        = keep ? (WEIGHTED ? weight[t] : 1.f) : 0.f;
        }
        for (int f = tid >> 7; f < kScatterStage; f += 2) {
            const long t    = t0 + f;
            const bool keep = t < t_end && comp < dim && cls[t] < n_classes;
            s_x[f][col]     = keep ? feats[(size_t)t * in_ld + comp] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int f = 0; f < kScatterStage; ++f) {
            const float4 xi = *reinterpret_cast<const float4*>(&s_x[f][ty * 4]);
            const float4 xj = *reinterpret_cast<const float4*>(&s_x[f][kScatterBlock + tx * 4]);
            const float  a[4] = {xi.x, xi.y, xi.z, xi.w}, b[4] = {xj.x, xj.y, xj.z, xj.w};
            const float  w = s_w[f];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float p = a[r] * b[c];  // x_i * x[j], f32
                    if (WEIGHTED)
                        p = p * w;          // ... * weight, f32 (the unweighted form multiplies by 1.0f: exact, dropped)
                    sum[r][c] += (double)p;
                }
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            s_t[ty * 4 + r][tx * 4 + c] = sum[r][c];
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int r = wave; r < kScatterBlock; r += 4) {
        const int gi = bi * kScatterBlock + r, gj = bj * kScatterBlock + lane;
        if (gi < dim && gj <= gi)
            atomicAdd(&acc[(size_t)gi * (gi + 1) / 2 + gj], s_t[r][lane]);
    }
}

// ---- class sums and counts.  Alignments are runs of one class: a wave walks 32 consecutive frames, lane = component (256 components
// per pass), sums a run in registers and adds it to the class's row when the class changes -- the run-length pattern of
// gmm_accumulate_kernel.  One atomic wave-instruction is 64 consecutive doubles of one row.
constexpr int kScatterRun = 32;  // frames per wave

template<bool WEIGHTED>
__global__ __launch_bounds__(256) void scatter_class_kernel(const float* __restrict__ feats, int in_ld, long T, int dim,
                                                            const uint32_t* __restrict__ cls, uint32_t n_classes,
                                                            const float* __restrict__ weight, double* __restrict__ sums,
                                                            double* __restrict__ counts) {
    const int  lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long t0   = ((long)blockIdx.x * 4 + wave) * kScatterRun;
    if (t0 >= T)
        return;
    const int n = T - t0 < kScatterRun ? (int)(T - t0) : kScatterRun;
    uint32_t  my_c = 0xffffffffu;
    float     my_w = 1.f;
    if (lane < n) {
        my_c = cls[t0 + lane];
        if (WEIGHTED)
            my_w = weight[t0 + lane];
    }
    for (int base = 0; base < dim; base += 256) {
        uint32_t cur = 0xffffffffu;
        double   s[4] = {0, 0, 0, 0}, cnt = 0;
        auto     flush = [&]() {
            if (cur == 0xffffffffu)
                return;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = base + k * 64 + lane;
                if (i < dim)
                    atomicAdd(&sums[(size_t)cur * dim + i], s[k]);
                s[k] = 0;
            }
            if (base == 0 && lane == 0)
                atomicAdd(&counts[cur], cnt);
            cnt = 0;
        };
        for (int f = 0; f < n; ++f) {
            const uint32_t c = __shfl(my_c, f);
            const float    w = __shfl(my_w, f);
            if (c >= n_classes)
                continue;
            if (c != cur) {
                flush();
                cur = c;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = base + k * 64 + lane;
                if (i < dim) {
                    float y = feats[(size_t)(t0 + f) * in_ld + i];
                    if (WEIGHTED)
                        y = y * w;  // x * weight, f32
                    s[k] += (double)y;
                }
            }
            cnt += (double)w;
        }
        flush();
    }
}

}  // namespace amx

extern "C++" {
namespace {
struct ScatterLayout {
    long tri, off_sums, off_counts, size;
};
ScatterLayout scatter_layout(int dim, int n_classes) {
    ScatterLayout l;
    l.tri        = (long)dim * (dim + 1) / 2;
    l.off_sums   = l.tri;
    l.off_counts = l.off_sums + (long)n_classes * dim;
    l.size       = l.off_counts + n_classes;
    return l;
}
bool scatter_shape_ok(int dim, int n_classes) {
    return dim >= 1 && dim <= 1024 && n_classes >= 1;
}
}  // namespace
}  // extern "C++"

extern "C" {

long amx_scatter_accumulator_size(int dim, int n_classes) {
    return scatter_shape_ok(dim, n_classes) ? scatter_layout(dim, n_classes).size : 0;
}

int amx_scatter_accumulate_dev(amx_ctx* ctx, const float* feats_dev, int in_ld, long T, int dim, const uint32_t* class_dev, int n_classes,
                               const float* weight_dev, double* acc_dev) {
    AMX_REQUIRE(ctx, AMX_ERR_INVALID, "amx_scatter_accumulate_dev: NULL context");
    AMX_REQUIRE(dim >= 1 && dim <= 1024, AMX_ERR_INVALID, "amx_scatter_accumulate_dev: dim %d is outside [1, 1024]", dim);
    AMX_REQUIRE(n_classes >= 1, AMX_ERR_INVALID, "amx_scatter_accumulate_dev: n_classes %d is not positive", n_classes);
    AMX_REQUIRE(in_ld >= dim, AMX_ERR_INVALID, "amx_scatter_accumulate_dev: in_ld %d is smaller than dim %d", in_ld, dim);
    AMX_REQUIRE(T >= 0, AMX_ERR_INVALID, "amx_scatter_accumulate_dev: negative frame count %ld", T);
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(feats_dev && class_dev && acc_dev, AMX_ERR_INVALID, "amx_scatter_accumulate_dev: NULL buffer");
    AMX_HIP(hipSetDevice(ctx->device));
    const ScatterLayout l = scatter_layout(dim, n_classes);
    // frame chunks: enough of them that blocks x chunks fills every CU kScatterGroups times, each a whole number of stages
    const int  nb       = amx::ceil_div(dim, amx::kScatterBlock);
    const int  n_blocks = nb * (nb + 1) / 2;
    const int  n_cu     = ctx->n_cu > 0 ? ctx->n_cu : 256;
    const long want     = std::max(1, amx::ceil_div((long)amx::kScatterGroups * n_cu, n_blocks));
    long       chunk    = (T + want - 1) / want;
    chunk               = (chunk + amx::kScatterStage - 1) / amx::kScatterStage * amx::kScatterStage;
    AMX_REQUIRE(chunk < (1l << 30), AMX_ERR_INVALID, "amx_scatter_accumulate_dev: %ld frames are more than one call takes", T);
    const int n_chunks = amx::ceil_div(T, chunk);  // <= want <= kScatterGroups * n_cu: far inside grid.y's 65535
    {
        amx::ScopedKernelTimer timer(ctx, "scatter_square");
        hipLaunchKernelGGL(weight_dev ? amx::scatter_square_kernel<true> : amx::scatter_square_kernel<false>, dim3(n_blocks, n_chunks), dim3(256), 0,
                           ctx->stream, feats_dev, in_ld, T, dim, class_dev, (uint32_t)n_classes, weight_dev, (int)chunk, acc_dev);
        AMX_HIP(hipGetLastError());
    }
    {
        const long             groups = (T + 4 * amx::kScatterRun - 1) / (4 * amx::kScatterRun);
        AMX_REQUIRE(groups < (1l << 31), AMX_ERR_INVALID, "amx_scatter_accumulate_dev: %ld frames are more than one call takes", T);
        amx::ScopedKernelTimer timer(ctx, "scatter_class");
        hipLaunchKernelGGL(weight_dev ? amx::scatter_class_kernel<true> : amx::scatter_class_kernel<false>, dim3((unsigned)groups), dim3(256), 0,
                           ctx->stream, feats_dev, in_ld, T, dim, class_dev, (uint32_t)n_classes, weight_dev, acc_dev + l.off_sums,
                           acc_dev + l.off_counts);
        AMX_HIP(hipGetLastError());
    }
    return AMX_OK;
}

// ---- accumulator files (ScatterMatricesEstimator::write / read, ScatterEstimator.cc:95-106, 359-376; Core::BinaryOutputStream,
// little endian):  u32 dim | f64 lower triangle | u32 nClasses | f64 sums[nClasses][dim] | f64 counts[nClasses]
int amx_scatter_accumulator_write(int dim, int n_classes, const double* acc, const char* path) {
    AMX_REQUIRE(acc && path, AMX_ERR_INVALID, "amx_scatter_accumulator_write: NULL argument");
    AMX_REQUIRE(scatter_shape_ok(dim, n_classes), AMX_ERR_INVALID, "amx_scatter_accumulator_write: bad shape (dim %d, n_classes %d)", dim, n_classes);
    const ScatterLayout l = scatter_layout(dim, n_classes);
    FILE*               f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "amx_scatter_accumulator_write: cannot open '%s'", path);
    const uint32_t d = (uint32_t)dim, n = (uint32_t)n_classes;  // little-endian host
    const size_t   rest = (size_t)(l.size - l.tri);
    bool           ok = fwrite(&d, 4, 1, f) == 1 && fwrite(acc, 8, (size_t)l.tri, f) == (size_t)l.tri && fwrite(&n, 4, 1, f) == 1 &&
              fwrite(acc + l.off_sums, 8, rest, f) == rest;
    ok = (fclose(f) == 0) && ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "amx_scatter_accumulator_write: write to '%s' failed", path);
    return AMX_OK;
}

int amx_scatter_accumulator_read(const char* path, int* dim, int* n_classes, double** acc) {
    AMX_REQUIRE(path && dim && n_classes && acc, AMX_ERR_INVALID, "amx_scatter_accumulator_read: NULL argument");
    *acc = nullptr;
    FILE* f = fopen(path, "rb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "amx_scatter_accumulator_read: cannot open '%s'", path);
    uint32_t d = 0, n = 0;
    double*  a  = nullptr;
    bool     ok = fread(&d, 4, 1, f) == 1 && d >= 1 && d <= 1024;
    long     tri = 0;
    if (ok) {
        tri = (long)d * (d + 1) / 2;
        ok  = fseek(f, tri * 8, SEEK_CUR) == 0 && fread(&n, 4, 1, f) == 1 && n >= 1 && n < (1u << 31);
    }
    if (ok) {
        const ScatterLayout l = scatter_layout((int)d, (int)n);
        const size_t        rest = (size_t)(l.size - l.tri);
        a  = (double*)malloc((size_t)l.size * sizeof(double));
        ok = a != nullptr && fseek(f, 4, SEEK_SET) == 0 && fread(a, 8, (size_t)tri, f) == (size_t)tri && fseek(f, 4, SEEK_CUR) == 0 &&
             fread(a + l.off_sums, 8, rest, f) == rest;
    }
    fclose(f);
    if (!ok) {
        free(a);
        amx::set_error("amx_scatter_accumulator_read: '%s' is not a scatter accumulator file (dim in [1, 1024], at least one class) or is truncated", path);
        return AMX_ERR_INVALID;
    }
    *dim       = (int)d;
    *n_classes = (int)n;
    *acc       = a;
    return AMX_OK;
}

// ---- ScatterMatricesEstimator::finalize (ScatterEstimator.cc:245-285) in the reference's own order of f64 operations:
// Math::vectorInnerProduct(s, s) / n is (s_i * s_j) / n per element (Math/Matrix.hh:476-485, 680-685), the class-mean part adds those
// matrices in class order, and Matrix::operator/= multiplies by the reciprocal (Math/Matrix.hh:156-158).
int amx_scatter_finalize(int dim, int n_classes, const double* acc, int normalize, double* between, double* within, double* total) {
    AMX_REQUIRE(acc, AMX_ERR_INVALID, "amx_scatter_finalize: NULL accumulator");
    AMX_REQUIRE(scatter_shape_ok(dim, n_classes), AMX_ERR_INVALID, "amx_scatter_finalize: bad shape (dim %d, n_classes %d)", dim, n_classes);
    const ScatterLayout l = scatter_layout(dim, n_classes);
    const double*       sums = acc + l.off_sums;
    const double*       counts = acc + l.off_counts;
    std::vector<double> s((size_t)dim, 0.0);  // getTotalVectorSum: classes in order
    for (int c = 0; c < n_classes; ++c)
        for (int i = 0; i < dim; ++i)
            s[i] += sums[(size_t)c * dim + i];
    double N = 0.0;  // getTotalCount: std::accumulate
    for (int c = 0; c < n_classes; ++c)
        N += counts[c];
    AMX_REQUIRE(!(N == 0), AMX_ERR_INVALID, "amx_scatter_finalize: No observation has been seen.");
    std::vector<double> class_mean((size_t)dim * dim, 0.0);
    for (int c = 0; c < n_classes; ++c) {
        if (!(counts[c] > 0))
            continue;
        const double* sc = sums + (size_t)c * dim;
        for (int i = 0; i < dim; ++i)
            for (int j = 0; j < dim; ++j)
                class_mean[(size_t)i * dim + j] += (sc[i] * sc[j]) / counts[c];
    }
    const double inv = 1.0 / N;
    for (int i = 0; i < dim; ++i)
        for (int j = 0; j < dim; ++j) {
            const size_t e  = (size_t)i * dim + j;
            const double sq = j <= i ? acc[(size_t)i * (i + 1) / 2 + j] : acc[(size_t)j * (j + 1) / 2 + i];  // finalizeVectorSquareSum
            const double tm = (s[i] * s[j]) / N;
            double       b = class_mean[e] - tm, w = sq - class_mean[e], t = sq - tm;
            if (normalize) {
                b *= inv;
                w *= inv;
                t *= inv;
            }
            if (between)
                between[e] = b;
            if (within)
                within[e] = w;
            if (total)
                total[e] = t;
        }
    return AMX_OK;
}

}  // extern "C"
