// quanteq.hip -- Signal::QuantileEqualization in segment mode on a [frames x dim] feature matrix that is already on the device
// (include/amx.h, section "Quantile equalisation"): the node signal-quantile-equalization for a batch of segments.
//
// Per (segment, channel) the reference sorts the column, picks nq + 1 order statistics, searches a 201 x 201 grid of (alpha, gamma) for the
// power function that moves them onto the training quantiles, optionally a 101 x 101 grid of (lambda, rho) that mixes neighbouring
// channels, transforms every frame and normalises mean and variance of the result (Signal/QuantileEqualization.cc:149-307).
//   quanteq_quantile_kernel        one workgroup per (segment, channel): the column as order-preserving integer keys in LDS, a bitonic
//                                  network, the nq + 1 picked values leave.  It also reports the first column with a non-finite value.
//   quanteq_search_kernel          one workgroup per (segment, channel), lanes across gamma: pow(scaled_i, gamma) does not depend on alpha,
//                                  so it is taken once per (i, gamma) (the reference takes it once per grid point: same bits, 201 times the
//                                  work), then every alpha is walked.  Winner by the key (distance, index of alpha, index of gamma).
//   quanteq_combine_search_kernel  the same over (lambda, rho), lanes across rho; no pow.
//   quanteq_apply_kernel           per element: power function, then the neighbour combination from the values before it, into out.
//   quanteq_sum_kernel             one lane per (segment, channel): f64 sum and square sum over the transformed frames, oldest first.
//   quanteq_normalize_kernel       per element: - mean, / deviation.
// The transformed matrix is stored once in out and read twice (sums, normalisation) instead of being recomputed: recomputing costs one f64
// pow per element and pass (three with the combination), the store 8 bytes per element.
// The library is compiled with -ffp-contract=off; mad<FMA> marks the sites the reference's -march=native build contracts.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "common.hpp"

namespace amx {

constexpr int       kQeThreads   = 256;
constexpr int       kQeMaxFrames = AMX_QUANTEQ_MAX_SEGMENT_FRAMES;   // 64 KB of keys in LDS
constexpr int       kQeMaxNq     = AMX_QUANTEQ_MAX_QUANTILES;
constexpr int       kQeMaxGrid   = AMX_QUANTEQ_MAX_GRID_SIDE;
constexpr int       kQeMaxDim    = AMX_QUANTEQ_MAX_DIM;
constexpr int       kQeAhead     = 8;    // frames loaded ahead of the sum chain (32 ahead measured slower: DESIGN.md 4.10)
constexpr long long kQeNone      = LLONG_MAX;

// Signal/QuantileEqualization.cc:202-203: f32 loop variables, f64 steps -- the table is what that loop visits
static std::vector<float> qe_grid(float lo, float hi, double step) {
    std::vector<float> t;
    for (float a = lo; a <= hi; a = (float)((double)a + step))
        t.push_back(a);
    return t;
}

}  // namespace amx

struct amx_quanteq {
    amx_ctx*        ctx = nullptr;
    amx_quanteq_cfg cfg{};
    int             dim = 0, nq = 0;
    std::vector<float> tq;                    // [(nq + 1) x dim] training quantiles as read
    std::vector<float> grid_a, grid_g, grid_l;
    std::vector<double> sums;                 // estimate: [(nq + 1) x dim]
    unsigned long long  count = 0;
    bool                uploaded = false;
    amx::DevBuf<float>     d_tq, d_ga, d_gg, d_gl;
    amx::DevBuf<long long> d_off;
    amx::DevBuf<float>     d_cq;      // [n_seg x (nq + 1) x dim] quantiles as first taken
    amx::DevBuf<float>     d_cqt;     // the same with the interior quantiles transformed
    amx::DevBuf<float>     d_par;     // [n_seg x 6 x dim] alpha, gamma, lambda, rho, mean, deviation
    amx::DevBuf<float>     d_max;     // [n_seg x dim] maximalQuantile
    amx::DevBuf<long long> d_bad;     // [1] first (segment * dim + channel) with a non-finite value
    std::vector<float>     h_cq;
};

namespace amx {

// floats in an order-preserving integer form: -0 before +0, ascending like operator< everywhere else
__device__ __forceinline__ unsigned qe_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float qe_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the unqualified pow of QuantileEqualization.cc:208 / .hh:110 is ::pow(double, double).  Out of line: the f64 routine's registers stay
// out of the grid walk.
__device__ __noinline__ double qe_pow(double x, double y) {
    return pow(x, y);
}

// std::max(a, b)
__device__ __forceinline__ float qe_max(float a, float b) {
    return a < b ? b : a;
}

// maximalQuantile * (alpha * pow(scaled, gamma) + (1. - alpha) * scaled), narrowed (:208, :223, .hh:110); pw = pow(scaled, gamma)
template<bool FMA>
__device__ __forceinline__ float qe_power_function(float maxq, float alpha, double pw, float scaled) {
    const double a = (double)alpha;
    return (float)((double)maxq * mad<FMA>(a, pw, (1. - a) * (double)scaled));
}

// (1. - l - r) * c0 + l * c1 + r * c2, narrowed (:249, .hh:120): the first product is f64, the other two are f32 products that are
// widened before they are added, so only the first can be contracted
template<bool FMA>
__device__ __forceinline__ float qe_combine(float l, float r, float c0, float c1, float c2) {
    const double w = 1. - (double)l - (double)r;
    return (float)(mad<FMA>(w, (double)c0, (double)(l * c1)) + (double)(r * c2));
}

// the segment of absolute frame t: the last one that starts at or before it (empty segments start where the next one does)
__device__ __forceinline__ int qe_segment(const long long* __restrict__ off, int n_seg, long long t) {
    int b = 0, e = n_seg;   // off[b] <= t < off[e]
    while (e - b > 1) {
        const int m = (b + e) / 2;
        if (off[m] <= t)
            b = m;
        else
            e = m;
    }
    return b;
}

__global__ __launch_bounds__(kQeThreads) void quanteq_quantile_kernel(const float* __restrict__ in, long long in_ld, const long long* __restrict__ off,
                                                                      int dim, int nq, float* __restrict__ cq, long long* first_bad) {
    extern __shared__ unsigned qe_keys[];
    const long long seg = blockIdx.x / dim;
    const int       d   = (int)(blockIdx.x % dim);
    const long long a   = off[seg];
    const int       T   = (int)(off[seg + 1] - a);
    if (T == 0)
        return;
    int N = 1;
    while (N < T)
        N *= 2;
    bool bad = false;
    for (int t = threadIdx.x; t < N; t += kQeThreads) {
        unsigned k = 0xffffffffu;   // behind every value
        if (t < T) {
            const float v = in[(a + t) * in_ld + d];
            bad |= !(fabsf(v) <= FLT_MAX);
            k = qe_key(v);
        }
        qe_keys[t] = k;
    }
    if (bad)
        atomicMin(first_bad, seg * dim + d);
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int p = threadIdx.x; p < N / 2; p += kQeThreads) {
                const int      lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int      hi = lo | j;
                const unsigned x = qe_keys[lo], y = qe_keys[hi];
                const bool     up = (lo & k) == 0;
                if ((x > y) == up) {
                    qe_keys[lo] = y;
                    qe_keys[hi] = x;
                }
            }
        }
    __syncthreads();
    // currentQuantile_[i * dim + d] = sorted[(u32)(i * (size - 1) / nq)] (:170)
    for (int i = threadIdx.x; i <= nq; i += kQeThreads)
        cq[(seg * (nq + 1) + i) * dim + d] = qe_unkey(qe_keys[(unsigned)((unsigned long long)i * (unsigned long long)(T - 1) / (unsigned long long)nq)]);
}

struct QeSearchArgs {
    const long long* off;
    const float*     cq;      // as first taken
    const float*     tq;
    float*           cqt;     // out: interior quantiles transformed
    float*           par;
    float*           maxq;
    const float*     grid_a;
    const float*     grid_g;
    int              na, ng, dim, nq;
    float            of;
};

// key (distance, first index, second index): the first strict minimum of the reference's scan, outer loop = first index
__device__ __forceinline__ bool qe_before(float d0, int a0, int g0, float d1, int a1, int g1) {
    return d0 < d1 || (d0 == d1 && (a0 < a1 || (a0 == a1 && g0 < g1)));
}

__device__ __forceinline__ void qe_reduce(float* rd, int* ra, int* rg, float d, int a, int g) {
    const int tid = threadIdx.x;
    rd[tid] = d, ra[tid] = a, rg[tid] = g;
    for (int s = kQeThreads / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s && ra[tid + s] >= 0 && (ra[tid] < 0 || qe_before(rd[tid + s], ra[tid + s], rg[tid + s], rd[tid], ra[tid], rg[tid]))) {
            rd[tid] = rd[tid + s];
            ra[tid] = ra[tid + s];
            rg[tid] = rg[tid + s];
        }
    }
    __syncthreads();
}

template<bool FMA>
__global__ __launch_bounds__(kQeThreads) void quanteq_search_kernel(QeSearchArgs p) {
    __shared__ double pw[(kQeMaxNq - 1) * kQeThreads];   // pow(scaled_i, gamma of this lane): column tid
    __shared__ float  scaled[kQeMaxNq], tqi[kQeMaxNq];
    __shared__ float  rd[kQeThreads];
    __shared__ int    ra[kQeThreads], rg[kQeThreads];
    const long long seg = blockIdx.x / p.dim;
    const int       d   = (int)(blockIdx.x % p.dim);
    if (p.off[seg + 1] == p.off[seg])
        return;
    const int    tid = threadIdx.x, nq = p.nq, dim = p.dim, ni = nq - 1;   // interior quantiles 1 .. nq - 1
    const float* cq  = p.cq + seg * (nq + 1) * dim;
    const float  maxq = qe_max(p.of * p.tq[nq * dim + d], p.of * cq[nq * dim + d]);   // :199
    if (tid < ni) {
        tqi[tid]    = p.tq[(tid + 1) * dim + d];
        scaled[tid] = qe_max(tqi[tid], cq[(tid + 1) * dim + d]) / maxq;               // :207
    }
    __syncthreads();
    float best = FLT_MAX;   // minimalDistance = Type<f32>::max (:197)
    int   ba = -1, bg = -1;
    for (int gj = tid; gj < p.ng; gj += kQeThreads) {
        const double g = (double)p.grid_g[gj];
        for (int i = 0; i < ni; ++i)
            pw[i * kQeThreads + tid] = qe_pow((double)scaled[i], g);
        for (int ai = 0; ai < p.na; ++ai) {
            const float a = p.grid_a[ai];
            float       dist = 0.f;
            for (int i = 0; i < ni; ++i) {
                const float tmp = qe_power_function<FMA>(maxq, a, pw[i * kQeThreads + tid], scaled[i]) - tqi[i];   // :208-209
                dist            = mad<FMA>(tmp, tmp, dist);                                                       // :210
            }
            if (dist < best || (dist == best && ai < ba)) {   // :213; a later pass of this lane has a higher gamma index
                best = dist;
                ba = ai, bg = gj;
            }
        }
    }
    qe_reduce(rd, ra, rg, best, ba, bg);
    const float alpha = ra[0] >= 0 ? p.grid_a[ra[0]] : 0.f;   // init (:41-46) where no point won
    const float gamma = ra[0] >= 0 ? p.grid_g[rg[0]] : 1.f;
    float*      par   = p.par + seg * 6 * dim;
    float*      cqt   = p.cqt + seg * (nq + 1) * dim;
    if (tid == 0) {
        par[d]                = alpha;
        par[dim + d]          = gamma;
        par[2 * dim + d]      = 0.f;
        par[3 * dim + d]      = 0.f;
        p.maxq[seg * dim + d] = maxq;
        cqt[d]                = cq[d];
        cqt[nq * dim + d]     = cq[nq * dim + d];
    }
    if (tid < ni)   // :221-224
        cqt[(tid + 1) * dim + d] = qe_power_function<FMA>(maxq, alpha, qe_pow((double)scaled[tid], (double)gamma), scaled[tid]);
}

struct QeCombineArgs {
    const long long* off;
    const float*     cqt;
    const float*     tq;
    float*           par;
    const float*     grid;
    int              n, dim, nq;
    float            beta;
};

template<bool FMA>
__global__ __launch_bounds__(kQeThreads) void quanteq_combine_search_kernel(QeCombineArgs p) {
    __shared__ float c0[kQeMaxNq], c1[kQeMaxNq], c2[kQeMaxNq], tqi[kQeMaxNq];
    __shared__ float rd[kQeThreads];
    __shared__ int   ra[kQeThreads], rg[kQeThreads];
    const long long seg = blockIdx.x / p.dim;
    const int       d   = (int)(blockIdx.x % p.dim);
    if (p.off[seg + 1] == p.off[seg])
        return;
    const int    tid = threadIdx.x, nq = p.nq, dim = p.dim, ni = nq - 1;
    const float* cqt = p.cqt + seg * (nq + 1) * dim;
    if (tid < ni) {
        const int row = (tid + 1) * dim;
        c0[tid]  = cqt[row + d];
        c1[tid]  = cqt[row + (d > 0 ? d - 1 : 0)];
        c2[tid]  = cqt[row + (d + 1 < dim ? d + 1 : dim - 1)];
        tqi[tid] = p.tq[row + d];
    }
    __syncthreads();
    float best = FLT_MAX;
    int   bl = -1, br = -1;
    for (int rj = tid; rj < p.n; rj += kQeThreads) {
        const float r = p.grid[rj];
        for (int li = 0; li < p.n; ++li) {
            const float l    = p.grid[li];
            float       dist = 0.f;
            for (int i = 0; i < ni; ++i) {
                const float tmp = qe_combine<FMA>(l, r, c0[i], c1[i], c2[i]) - tqi[i];   // :249-250
                dist            = mad<FMA>(tmp, tmp, dist);
            }
            dist = mad<FMA>(mad<FMA>(l, l, r * r), p.beta, dist);   // :254
            if (dist < best || (dist == best && li < bl)) {
                best = dist;
                bl = li, br = rj;
            }
        }
    }
    qe_reduce(rd, ra, rg, best, bl, br);
    if (tid == 0 && ra[0] >= 0) {
        float* par       = p.par + seg * 6 * dim;
        par[2 * dim + d] = p.grid[ra[0]];
        par[3 * dim + d] = p.grid[rg[0]];
    }
}

struct QeApplyArgs {
    const float*     in;
    float*           out;
    long long        in_ld, out_ld;
    const long long* off;
    long long        base, frames;
    int              n_seg, dim, rpb;
    const float*     par;
    const float*     maxq;
};

// rpb frames per workgroup: the power function of every element into LDS, then the combination from there.  A workgroup reads and
// writes its own frames only, so out may be in.
template<bool FMA, bool EQ, bool COMB>
__global__ __launch_bounds__(kQeThreads) void quanteq_apply_kernel(QeApplyArgs p) {
    extern __shared__ float qe_tile[];
    __shared__ int          seg_of[kQeThreads];
    const long long f0   = (long long)blockIdx.x * p.rpb;
    const int       rows = (int)(p.frames - f0 < p.rpb ? p.frames - f0 : p.rpb);
    const int       dim  = p.dim;
    for (int r = threadIdx.x; r < rows; r += kQeThreads)
        seg_of[r] = qe_segment(p.off, p.n_seg, p.base + f0 + r);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * dim; e += kQeThreads) {
        const int       r = e / dim, d = e % dim;
        const long long t = p.base + f0 + r;
        float           v = p.in[t * p.in_ld + d];
        if (EQ) {
            const float* par   = p.par + (long long)seg_of[r] * 6 * dim;
            const float  maxq  = p.maxq[(long long)seg_of[r] * dim + d];
            const float  sv    = v / maxq;                                                        // .hh:108
            v                  = qe_power_function<FMA>(maxq, par[d], qe_pow((double)sv, (double)par[dim + d]), sv);   // .hh:110
        }
        qe_tile[e] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * dim; e += kQeThreads) {
        const int       r = e / dim, d = e % dim;
        const long long t = p.base + f0 + r;
        float           v = qe_tile[e];
        if (COMB) {
            const float* par = p.par + (long long)seg_of[r] * 6 * dim;
            v = qe_combine<FMA>(par[2 * dim + d], par[3 * dim + d], v, qe_tile[r * dim + (d > 0 ? d - 1 : 0)], qe_tile[r * dim + (d + 1 < dim ? d + 1 : dim - 1)]);
        }
        p.out[t * p.out_ld + d] = v;
    }
}

// one lane per (segment, channel), consecutive lanes consecutive channels (cpad of them); the f64 sums are one dependent chain whose
// order the reference fixes (:289-306: the transformed window is filled newest frame first by push_front, :267-280, so its index 0 is
// the OLDEST frame), the loads run ahead of it
template<bool FMA>
__global__ __launch_bounds__(kQeThreads) void quanteq_sum_kernel(const float* __restrict__ x, long long ld, const long long* __restrict__ off, int n_seg,
                                                                 int dim, int cpad, int variance, float* __restrict__ par) {
    const long long gid = (long long)blockIdx.x * kQeThreads + threadIdx.x;
    const long long seg = gid / cpad;
    const int       d   = (int)(gid % cpad);
    if (seg >= n_seg || d >= dim)
        return;
    const long long a = off[seg], n = off[seg + 1] - a;
    if (n == 0)
        return;
    const float* s = x + a * ld + d;
    double sum = 0.0, sq = 0.0;
    for (long long t0 = 0; t0 < n; t0 += kQeAhead) {
        float v[kQeAhead];
#pragma unroll
        for (int i = 0; i < kQeAhead; ++i)
            v[i] = t0 + i < n ? s[(t0 + i) * ld] : 0.f;
#pragma unroll
        for (int i = 0; i < kQeAhead; ++i) {
            if (t0 + i >= n)
                break;
            sum += (double)v[i];                                 // :295
            sq = mad<FMA>((double)v[i], (double)v[i], sq);       // :298
        }
    }
    const double size = (double)n;
    par[(seg * 6 + 4) * dim + d] = (float)(sum / size);                                             // :302
    par[(seg * 6 + 5) * dim + d] = variance ? (float)sqrt((sq - sum * sum / size) / size) : 0.f;    // :305
}

__global__ __launch_bounds__(kQeThreads) void quanteq_normalize_kernel(float* __restrict__ x, long long ld, const long long* __restrict__ off, int n_seg,
                                                                       long long base, long long frames, int dim, int variance,
                                                                       const float* __restrict__ par) {
    const long long e = (long long)blockIdx.x * kQeThreads + threadIdx.x;
    if (e >= frames * dim)
        return;
    const long long t   = base + e / dim;
    const int       d   = (int)(e % dim);
    const int       seg = qe_segment(off, n_seg, t);
    float           v   = x[t * ld + d] - par[((long long)seg * 6 + 4) * dim + d];   // .hh:126
    if (variance)
        v = v / par[((long long)seg * 6 + 5) * dim + d];                            // .hh:130
    x[t * ld + d] = v;
}

static int qe_segments(int n_seg, const long* frame_offsets, const char* who, std::vector<long long>* off, long long* frames) {
    AMX_REQUIRE(frame_offsets, AMX_ERR_INVALID, "%s: NULL segment list", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: negative frame offset", who);
    off->resize((size_t)n_seg + 1);
    for (int s = 0; s <= n_seg; ++s) {
        AMX_REQUIRE(s == 0 || frame_offsets[s - 1] <= frame_offsets[s], AMX_ERR_INVALID, "%s: frame offsets decrease at segment %d", who, s - 1);
        AMX_REQUIRE(s == 0 || frame_offsets[s] - frame_offsets[s - 1] <= kQeMaxFrames, AMX_ERR_UNSUPPORTED,
                    "%s: segment %d has %ld frames, the sort takes at most %d", who, s - 1, frame_offsets[s] - frame_offsets[s - 1], kQeMaxFrames);
        (*off)[s] = frame_offsets[s];
    }
    *frames = (*off)[n_seg] - (*off)[0];
    return AMX_OK;
}

static int qe_upload(amx_quanteq* h) {
    if (h->uploaded)
        return AMX_OK;
    AMX_TRY(h->d_tq.upload(h->tq.data(), h->tq.size()));
    AMX_TRY(h->d_ga.upload(h->grid_a.data(), h->grid_a.size()));
    AMX_TRY(h->d_gg.upload(h->grid_g.data(), h->grid_g.size()));
    AMX_TRY(h->d_gl.upload(h->grid_l.data(), h->grid_l.size()));
    AMX_TRY(h->d_bad.reserve(1));
    h->uploaded = true;
    return AMX_OK;
}

// the quantiles of every segment into d_cq; fails, before anything else ran, on a non-finite input.  Synchronises the stream.
static int qe_quantiles(amx_quanteq* h, int n_seg, const std::vector<long long>& off, const float* in_dev, int in_ld, const char* who) {
    amx_ctx*  ctx = h->ctx;
    const int dim = h->dim, nq = h->nq;
    AMX_REQUIRE((long long)n_seg * dim < (1ll << 31), AMX_ERR_INVALID, "%s: %d segments of %d channels are more than one call takes", who, n_seg, dim);
    AMX_TRY(h->d_off.reserve(off.size()));
    AMX_HIP(hipMemcpyAsync(h->d_off.get(), off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    AMX_TRY(h->d_cq.reserve((size_t)n_seg * (nq + 1) * dim));
    AMX_HIP(hipMemsetAsync(h->d_cq.get(), 0, (size_t)n_seg * (nq + 1) * dim * sizeof(float), ctx->stream));
    long long bad = kQeNone, longest = 0;
    for (int s = 0; s < n_seg; ++s)
        longest = std::max(longest, off[s + 1] - off[s]);
    size_t N = 1;
    while ((long long)N < longest)
        N *= 2;
    AMX_HIP(hipMemcpyAsync(h->d_bad.get(), &bad, sizeof(bad), hipMemcpyHostToDevice, ctx->stream));
    {
        ScopedKernelTimer timer(ctx, "quanteq_quantile");
        hipLaunchKernelGGL(quanteq_quantile_kernel, dim3((unsigned)(n_seg * dim)), dim3(kQeThreads), N * sizeof(unsigned), ctx->stream, in_dev,
                           (long long)in_ld, h->d_off.get(), dim, nq, h->d_cq.get(), h->d_bad.get());
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipMemcpyAsync(&bad, h->d_bad.get(), sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    AMX_REQUIRE(bad == kQeNone, AMX_ERR_INVALID, "%s: segment %lld, channel %lld holds a value that is not finite; nothing was written", who, bad / dim,
                bad % dim);
    return AMX_OK;
}

static int pad_channels(int n) {
    if (n > kQeThreads)
        return (n + kQeThreads - 1) / kQeThreads * kQeThreads;
    int p = 1;
    while (p < n)
        p *= 2;
    return p;
}

template<bool FMA>
static int qe_apply(amx_quanteq* h, int n_seg, const std::vector<long long>& off, long long T, const float* in_dev, int in_ld, float* out_dev, int out_ld) {
    amx_ctx*               ctx = h->ctx;
    const amx_quanteq_cfg& c   = h->cfg;
    const int              dim = h->dim, nq = h->nq;
    const unsigned         pairs = (unsigned)(n_seg * dim);
    if (c.quantiles) {
        QeSearchArgs a{};
        a.off = h->d_off.get(), a.cq = h->d_cq.get(), a.tq = h->d_tq.get(), a.cqt = h->d_cqt.get(), a.par = h->d_par.get(), a.maxq = h->d_max.get();
        a.grid_a = h->d_ga.get(), a.grid_g = h->d_gg.get(), a.na = (int)h->grid_a.size(), a.ng = (int)h->grid_g.size();
        a.dim = dim, a.nq = nq, a.of = c.overestimation_factor;
        {
            ScopedKernelTimer timer(ctx, "quanteq_search");
            hipLaunchKernelGGL(quanteq_search_kernel<FMA>, dim3(pairs), dim3(kQeThreads), 0, ctx->stream, a);
            AMX_HIP(hipGetLastError());
        }
        if (c.combination) {
            QeCombineArgs b{};
            b.off = h->d_off.get(), b.cqt = h->d_cqt.get(), b.tq = h->d_tq.get(), b.par = h->d_par.get(), b.grid = h->d_gl.get();
            b.n = (int)h->grid_l.size(), b.dim = dim, b.nq = nq, b.beta = c.beta;
            ScopedKernelTimer timer(ctx, "quanteq_combine_search");
            hipLaunchKernelGGL(quanteq_combine_search_kernel<FMA>, dim3(pairs), dim3(kQeThreads), 0, ctx->stream, b);
            AMX_HIP(hipGetLastError());
        }
    }
    const bool copy = c.quantiles || c.combination || out_dev != in_dev;
    if (copy) {
        QeApplyArgs a{};
        a.in = in_dev, a.out = out_dev, a.in_ld = in_ld, a.out_ld = out_ld, a.off = h->d_off.get(), a.base = off[0], a.frames = T;
        a.n_seg = n_seg, a.dim = dim, a.rpb = std::max(1, std::min(kQeThreads, 2048 / dim)), a.par = h->d_par.get(), a.maxq = h->d_max.get();
        const long long groups = (T + a.rpb - 1) / a.rpb;
        const size_t    lds    = (size_t)a.rpb * dim * sizeof(float);
        ScopedKernelTimer timer(ctx, "quanteq_apply");
        const dim3 grid((unsigned)groups), block(kQeThreads);
        if (c.quantiles && c.combination)
            hipLaunchKernelGGL((quanteq_apply_kernel<FMA, true, true>), grid, block, lds, ctx->stream, a);
        else if (c.quantiles)
            hipLaunchKernelGGL((quanteq_apply_kernel<FMA, true, false>), grid, block, lds, ctx->stream, a);
        else if (c.combination)
            hipLaunchKernelGGL((quanteq_apply_kernel<FMA, false, true>), grid, block, lds, ctx->stream, a);
        else
            hipLaunchKernelGGL((quanteq_apply_kernel<FMA, false, false>), grid, block, lds, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    if (c.mean) {
        const int       cpad   = pad_channels(dim);
        const long long groups = ((long long)n_seg * cpad + kQeThreads - 1) / kQeThreads;
        {
            ScopedKernelTimer timer(ctx, "quanteq_sum");
            hipLaunchKernelGGL(quanteq_sum_kernel<FMA>, dim3((unsigned)groups), dim3(kQeThreads), 0, ctx->stream, out_dev, (long long)out_ld, h->d_off.get(),
                               n_seg, dim, cpad, c.variance ? 1 : 0, h->d_par.get());
            AMX_HIP(hipGetLastError());
        }
        const long long g2 = (T * dim + kQeThreads - 1) / kQeThreads;
        ScopedKernelTimer timer(ctx, "quanteq_normalize");
        hipLaunchKernelGGL(quanteq_normalize_kernel, dim3((unsigned)g2), dim3(kQeThreads), 0, ctx->stream, out_dev, (long long)out_ld, h->d_off.get(), n_seg,
                           off[0], T, dim, c.variance ? 1 : 0, h->d_par.get());
        AMX_HIP(hipGetLastError());
    }
    return AMX_OK;
}

}  // namespace amx

extern "C" {

void amx_quanteq_default_cfg(amx_quanteq_cfg* cfg) {
    if (!cfg)
        return;
    cfg->quantiles             = 1;        // QuantileEqualization.cc:341-356
    cfg->combination           = 0;
    cfg->estimate              = 0;
    cfg->mean                  = 1;
    cfg->variance              = 0;
    cfg->number_of_quantiles   = 4;
    cfg->overestimation_factor = 1.0f;
    cfg->delta_alpha           = 0.005f;
    cfg->delta_gamma           = 0.01f;
    cfg->delta_lambda_and_rho  = 0.005f;
    cfg->beta                  = 0.05f;
    cfg->pool_quantiles        = 1;
    cfg->piecewise_linear      = 0;
    cfg->length                = INT_MAX;   // the node's two parameters have no default; this is the segment mode
    cfg->right                 = INT_MAX;
}

int amx_quanteq_create(amx_ctx* ctx, int dim, const amx_quanteq_cfg* cfg, const float* training_quantiles, amx_quanteq** out) {
    const char* who = "amx_quanteq_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(cfg, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(dim >= 1 && dim <= amx::kQeMaxDim, AMX_ERR_INVALID, "%s: dim %d is outside 1 .. %d", who, dim, amx::kQeMaxDim);
    AMX_REQUIRE(cfg->length >= INT_MAX && cfg->right >= INT_MAX, AMX_ERR_UNSUPPORTED,
                "%s: length %ld, right %ld: only the segment mode (both %d) is built, not the sliding window", who, cfg->length, cfg->right, INT_MAX);
    AMX_REQUIRE(!cfg->piecewise_linear, AMX_ERR_UNSUPPORTED, "%s: piecewise_linear is not built", who);
    AMX_REQUIRE(cfg->number_of_quantiles >= 1 && cfg->number_of_quantiles <= amx::kQeMaxNq, AMX_ERR_UNSUPPORTED,
                "%s: number_of_quantiles %d is outside 1 .. %d", who, cfg->number_of_quantiles, amx::kQeMaxNq);
    // a step <= 0 never ends the reference's loop; the side of a grid is bounded so that the f32 loop variable moves at every step
    const struct { const char* name; float step; double range; } steps[3] = {
        {"delta_alpha", cfg->delta_alpha, 1.0}, {"delta_gamma", cfg->delta_gamma, 2.0}, {"delta_lambda_and_rho", cfg->delta_lambda_and_rho, 0.5}};
    for (const auto& s : steps)
        AMX_REQUIRE(s.step > 0.f && s.range / (double)s.step + 1.0 <= (double)amx::kQeMaxGrid, AMX_ERR_UNSUPPORTED,
                    "%s: %s %g must be positive and give a grid of at most %d points a side", who, s.name, (double)s.step, amx::kQeMaxGrid);
    const bool needs_tq = cfg->quantiles && !cfg->estimate;
    AMX_REQUIRE(!needs_tq || training_quantiles, AMX_ERR_INVALID, "%s: NULL training_quantiles", who);
    AMX_REQUIRE(!cfg->estimate || cfg->quantiles, AMX_ERR_INVALID, "%s: estimate needs quantiles (the reference takes no quantiles without)", who);
    std::unique_ptr<amx_quanteq> h(new amx_quanteq);
    h->ctx = ctx;
    h->cfg = *cfg;
    h->dim = dim;
    h->nq  = cfg->number_of_quantiles;
    const size_t n = (size_t)(h->nq + 1) * dim;
    h->tq.assign(n, 0.f);
    if (needs_tq)
        std::copy(training_quantiles, training_quantiles + n, h->tq.begin());
    h->grid_a = amx::qe_grid(0.f, 1.f, (double)cfg->delta_alpha);               // :185-188, :202
    h->grid_g = amx::qe_grid(1.f, 3.f, (double)cfg->delta_gamma);               // :203
    h->grid_l = amx::qe_grid(0.f, 0.5f, (double)cfg->delta_lambda_and_rho);     // :230-233, :244-245
    h->sums.assign(n, 0.0);
    *out = h.release();
    return AMX_OK;
}

void amx_quanteq_destroy(amx_quanteq* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_quanteq_grid(const amx_quanteq* h, int which, int* n, float* values) {
    AMX_REQUIRE(h && n, AMX_ERR_INVALID, "amx_quanteq_grid: NULL argument");
    AMX_REQUIRE(which >= 0 && which <= 2, AMX_ERR_INVALID, "amx_quanteq_grid: grid %d is not 0 (alpha), 1 (gamma) or 2 (lambda and rho)", which);
    const std::vector<float>& g = which == 0 ? h->grid_a : which == 1 ? h->grid_g : h->grid_l;
    *n = (int)g.size();
    if (values)
        std::copy(g.begin(), g.end(), values);
    return AMX_OK;
}

int amx_quanteq_quantiles_read(const char* path, int dim, int nq, int pool, float* out) {
    const char* who = "amx_quanteq_quantiles_read";
    AMX_REQUIRE(path && out, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(dim >= 1 && nq >= 1, AMX_ERR_INVALID, "%s: dim %d, number of quantiles %d", who, dim, nq);
    FILE* f = fopen(path, "rt");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: Can't open training quantile file: \"%s\"", who, path);
    bool ok = true;
    for (int d = 0; d < dim && ok; ++d) {   // readTrainingQuantilesFromFile (:78-83); a short file is an error here, stale values there
        unsigned index;
        ok = fscanf(f, "%u ", &index) == 1;
        for (int i = 0; i <= nq && ok; ++i)
            ok = fscanf(f, "%f ", &out[(size_t)i * dim + d]) == 1;
    }
    fclose(f);
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: \"%s\" does not hold %d lines of an index and %d quantiles", who, path, dim, nq + 1);
    if (pool)   // :87-100
        for (int i = 0; i <= nq; ++i) {
            float average = 0.f;
            for (int d = 0; d < dim; ++d)
                average += out[(size_t)i * dim + d];
            average /= (float)(unsigned)dim;
            for (int d = 0; d < dim; ++d)
                out[(size_t)i * dim + d] = average;
        }
    return AMX_OK;
}

int amx_quanteq_quantiles_write(const char* path, int dim, int nq, const double* sums, unsigned long long count) {
    const char* who = "amx_quanteq_quantiles_write";
    AMX_REQUIRE(path && sums, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(dim >= 1 && nq >= 1, AMX_ERR_INVALID, "%s: dim %d, number of quantiles %d", who, dim, nq);
    AMX_REQUIRE(count <= 0xffffffffull, AMX_ERR_INVALID, "%s: count %llu does not fit the reference's u32 counter", who, count);
    FILE* f = fopen(path, "wt");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: Can't open training quantile output file: \"%s\"", who, path);
    const unsigned counter = (unsigned)count;
    for (int d = 0; d < dim; ++d) {   // writeEstimatedQuantilesToFile (:110-116)
        fprintf(f, "%i ", d);
        for (int i = 0; i <= nq; ++i)
            fprintf(f, "%f ", sums[(size_t)i * dim + d] / counter);
        fprintf(f, "\n");
    }
    const bool ok = !ferror(f);
    AMX_REQUIRE((fclose(f) == 0) && ok, AMX_ERR_INVALID, "%s: writing \"%s\" failed", who, path);
    return AMX_OK;
}

int amx_quanteq_apply_dev(amx_quanteq* h, int n_seg, const long* frame_offsets, const float* in_dev, int in_ld, float* out_dev, int out_ld,
                          float* params_host) {
    const char* who = "amx_quanteq_apply_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(!h->cfg.estimate, AMX_ERR_STATE, "%s: the handle estimates quantiles; its output stream is not built", who);
    const int dim = h->dim, nq = h->nq;
    AMX_REQUIRE(n_seg >= 0 && in_ld >= dim && out_ld >= dim, AMX_ERR_INVALID, "%s: n_seg %d, in_ld %d, out_ld %d with %d channels", who, n_seg, in_ld,
                out_ld, dim);
    if (n_seg == 0)
        return AMX_OK;
    std::vector<long long> off;
    long long              T = 0;
    AMX_TRY(amx::qe_segments(n_seg, frame_offsets, who, &off, &T));
    const size_t P = (size_t)dim * (6 + nq + 1);
    if (params_host)
        std::memset(params_host, 0, (size_t)n_seg * P * sizeof(float));
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(in_dev && out_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    AMX_REQUIRE(in_dev == out_dev ? in_ld == out_ld : (out_dev + (size_t)off[n_seg] * out_ld <= in_dev || in_dev + (size_t)off[n_seg] * in_ld <= out_dev),
                AMX_ERR_INVALID, "%s: in_dev and out_dev overlap without being the identical view", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_TRY(amx::qe_upload(h));
    AMX_TRY(h->d_cqt.reserve((size_t)n_seg * (nq + 1) * dim));
    AMX_TRY(h->d_par.reserve((size_t)n_seg * 6 * dim));
    AMX_TRY(h->d_max.reserve((size_t)n_seg * dim));
    if (h->cfg.quantiles)
        AMX_TRY(amx::qe_quantiles(h, n_seg, off, in_dev, in_ld, who));
    else {
        // no order statistics are taken; the finiteness of the input is not needed either (no sort)
        AMX_TRY(h->d_off.reserve(off.size()));
        AMX_HIP(hipMemcpyAsync(h->d_off.get(), off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    }
    AMX_HIP(hipMemsetAsync(h->d_par.get(), 0, (size_t)n_seg * 6 * dim * sizeof(float), ctx->stream));
    if (ctx->contract == AMX_CONTRACT_FMA)
        AMX_TRY(amx::qe_apply<true>(h, n_seg, off, T, in_dev, in_ld, out_dev, out_ld));
    else
        AMX_TRY(amx::qe_apply<false>(h, n_seg, off, T, in_dev, in_ld, out_dev, out_ld));
    if (params_host) {
        std::vector<float> par((size_t)n_seg * 6 * dim);
        h->h_cq.assign((size_t)n_seg * (nq + 1) * dim, 0.f);
        AMX_HIP(hipMemcpyAsync(par.data(), h->d_par.get(), par.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (h->cfg.quantiles)
            AMX_HIP(hipMemcpyAsync(h->h_cq.data(), h->d_cq.get(), h->h_cq.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipStreamSynchronize(ctx->stream));
        for (int s = 0; s < n_seg; ++s) {
            if (off[s + 1] == off[s])
                continue;
            float* p = params_host + (size_t)s * P;
            std::copy(par.begin() + (size_t)s * 6 * dim, par.begin() + (size_t)(s + 1) * 6 * dim, p);
            if (!h->cfg.quantiles)
                std::fill(p + dim, p + 2 * dim, 1.f);   // gamma of init (:43)
            std::copy(h->h_cq.begin() + (size_t)s * (nq + 1) * dim, h->h_cq.begin() + (size_t)(s + 1) * (nq + 1) * dim, p + 6 * dim);
        }
    }
    return AMX_OK;
}

int amx_quanteq_estimate_dev(amx_quanteq* h, int n_seg, const long* frame_offsets, const float* in_dev, int in_ld) {
    const char* who = "amx_quanteq_estimate_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(h->cfg.estimate, AMX_ERR_STATE, "%s: the handle was not created with estimate = 1", who);
    const int dim = h->dim, nq = h->nq;
    AMX_REQUIRE(n_seg >= 0 && in_ld >= dim, AMX_ERR_INVALID, "%s: n_seg %d, in_ld %d with %d channels", who, n_seg, in_ld, dim);
    if (n_seg == 0)
        return AMX_OK;
    std::vector<long long> off;
    long long              T = 0;
    AMX_TRY(amx::qe_segments(n_seg, frame_offsets, who, &off, &T));
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(in_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_TRY(amx::qe_upload(h));
    AMX_TRY(amx::qe_quantiles(h, n_seg, off, in_dev, in_ld, who));
    const size_t n = (size_t)(nq + 1) * dim;
    h->h_cq.resize((size_t)n_seg * n);
    AMX_HIP(hipMemcpyAsync(h->h_cq.data(), h->d_cq.get(), h->h_cq.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < n_seg; ++s) {   // :172 once per segment, in segment order; frameCounter_++ (:316)
        if (off[s + 1] == off[s])
            continue;
        for (size_t k = 0; k < n; ++k)
            h->sums[k] += (double)h->h_cq[(size_t)s * n + k];
        ++h->count;
    }
    return AMX_OK;
}

int amx_quanteq_estimate_result(const amx_quanteq* h, double* sums, unsigned long long* count) {
    AMX_REQUIRE(h && sums && count, AMX_ERR_INVALID, "amx_quanteq_estimate_result: NULL argument");
    AMX_REQUIRE(h->cfg.estimate, AMX_ERR_STATE, "amx_quanteq_estimate_result: the handle was not created with estimate = 1");
    std::copy(h->sums.begin(), h->sums.end(), sums);
    *count = h->count;
    return AMX_OK;
}

}  // extern "C"
