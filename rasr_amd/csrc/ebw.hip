// ebw.hip -- the corpus pass of extended Baum-Welch training (include/amx.h, section "EBW"): lattice arc weights become numerator and
// denominator statistics.  Lattice::AcousticAccumulator::discoverState and CachedAcousticAccumulator::process / finish
// (Lattice/Accumulator.tcc:66-115), Speech::SegmentwiseGmmTrainer's two accumulators (Speech/SegmentwiseGmmTrainer.cc:64-88, :160-168),
// Mm::DiscriminativeMixtureSetEstimator::accumulate / accumulateDenominator (Mm/DiscriminativeMixtureSetEstimator.cc:187-203) and what
// they reach (Mm/MixtureEstimator.cc:92-97, Mm/EbwDiscriminativeMixtureEstimator.cc:109-116).
//
// Order.  Everything that is added in floating point is added in an order that the input alone defines:
//   1. ebw_resolve_kernel: every item's segment, side and checks, its sort code (frame, mixture, side) and its arc's weight, before
//      anything is written; ebw_rows_kernel checks the feature rows that an item with a side touches.
//   2. a stable radix sort of the items by that code (integer counters per block and digit, a scan, placement by the number of
//      earlier items with the same digit): equal codes keep arc order, then item order.  The first item of every run of equal codes
//      is a key; one thread adds its run's widened weights into an f64 in that order: Collector::collect.
//   3. the best density of every key (amx_gmm_best_density_dev on the keys' gathered rows), then three list entries per key -- its
//      slot in the mixture, its mean and side, its covariance and side -- sorted by list with the same stable sort: a list holds its
//      keys in ascending (frame, mixture).
//   4. ebw_chain_kernel, one workgroup per (list, 256 cells): a lane owns one cell, whose chain starts from what the buffer holds,
//      stays in a register and is written back once.  No floating-point atomic, no partial sums: the integer atomics only count.
// The library is compiled with -ffp-contract=off; mad<FMA> marks plusWeighted and plusSquareWeighted (Mm/Utilities.hh:108-153), the
// sites a contracting build of the reference fuses.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "common.hpp"
#include "gmm_internal.hpp"

namespace amx {

constexpr int       kEbwThreads   = 256;
constexpr int       kEbwBlock     = 2048;        // elements of one workgroup of the sort and the scan: 8 chunks of 256
constexpr int       kEbwStage     = 64;          // keys of a list a chain prefetches at a time
constexpr long long kEbwMaxItems  = 1ll << 27;   // per call: positions and counts are 32-bit integers
constexpr long long kEbwMaxFrames = 1ll << 27;

__device__ __forceinline__ long long ebw_upper(const long long* __restrict__ off, long long n, long long v) {
    long long lo = 0, hi = n;   // first index with off[index] > v
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (off[mid] > v)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// ---- items and arcs.  bad = min over the offences of (index << 3 | kind): 1 an item's frame outside its segment, 2 its emission
// outside the model, 3 an arc's weight not finite, 4 (ebw_rows_kernel) a touched feature row not finite
__global__ __launch_bounds__(kEbwThreads) void ebw_resolve_kernel(long long n_items, long long n_arcs, int n_seg, const long long* __restrict__ frame_off,
                                                                  const long long* __restrict__ arc_off, const float* __restrict__ arc_w,
                                                                  const long long* __restrict__ item_off, const int32_t* __restrict__ item_frame,
                                                                  const int32_t* __restrict__ item_emission, float threshold, int n_mix, int mix_bits,
                                                                  unsigned long long sentinel, unsigned long long* __restrict__ code,
                                                                  uint32_t* __restrict__ val, int* __restrict__ touched, unsigned long long* bad) {
    const long long i = (long long)blockIdx.x * kEbwThreads + threadIdx.x;
    if (i < n_arcs && !isfinite(arc_w[i]))
        atomicMin(bad, ((unsigned long long)i << 3) | 3ull);
    if (i >= n_items)
        return;
    const long long arc = ebw_upper(item_off, n_arcs + 1, i) - 1;
    const long long seg = ebw_upper(arc_off, (long long)n_seg + 1, arc) - 1;
    const float     w   = arc_w[arc];
    const int       side = w > threshold ? 0 : (-w > threshold ? 1 : -1);   // f32, strict (Accumulator.tcc:71-72; the denominator's fsa is -w)
    const long long f = item_frame[i], len = frame_off[seg + 1] - frame_off[seg];
    const int32_t   e = item_emission[i];
    unsigned long long c = sentinel;
    uint32_t           v = 0;
    if (f < 0 || f >= len)
        atomicMin(bad, ((unsigned long long)i << 3) | 1ull);
    else if (e < 0 || e >= n_mix)
        atomicMin(bad, ((unsigned long long)i << 3) | 2ull);
    else if (side >= 0 && isfinite(w)) {
        const long long fg = frame_off[seg] - frame_off[0] + f;
        c                  = ((unsigned long long)fg << (mix_bits + 1)) | ((unsigned long long)e << 1) | (unsigned long long)side;
        v                  = __float_as_uint(side ? -w : w);
        touched[fg]        = 1;   // every writer stores the same value
    }
    code[i] = c;
    val[i]  = v;
}

__global__ __launch_bounds__(kEbwThreads) void ebw_rows_kernel(const float* __restrict__ feats, long long ld, int D, long long t0, long long n,
                                                               const int* __restrict__ touched, unsigned long long* bad) {
    const long long i = (long long)blockIdx.x * kEbwThreads + threadIdx.x;
    if (i >= n || !touched[i])
        return;
    bool ok = true;
    for (int c = 0; c < D; ++c)
        ok = ok && isfinite(feats[(t0 + i) * ld + c]);
    if (!ok)
        atomicMin(bad, ((unsigned long long)i << 3) | 4ull);
}

// ---- exclusive scan of 32-bit integers in place: a workgroup scans kEbwBlock of them and leaves its total in sums[block]
__global__ __launch_bounds__(kEbwThreads) void ebw_scan_block_kernel(int* __restrict__ data, long long n, int* __restrict__ sums) {
    __shared__ int  s[kEbwThreads];
    const int       tid  = threadIdx.x;
    const long long base = (long long)blockIdx.x * kEbwBlock + (long long)tid * 8;
    int             v[8], total = 0;
    for (int j = 0; j < 8; ++j) {
        v[j] = base + j < n ? data[base + j] : 0;
        total += v[j];
    }
    s[tid] = total;
    __syncthreads();
    for (int o = 1; o < kEbwThreads; o <<= 1) {
        const int add = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    int run = s[tid] - total;
    for (int j = 0; j < 8; ++j) {
        if (base + j < n)
            data[base + j] = run;
        run += v[j];
    }
    if (tid == kEbwThreads - 1)
        sums[blockIdx.x] = s[tid];
}

__global__ __launch_bounds__(kEbwThreads) void ebw_scan_add_kernel(int* __restrict__ data, long long n, const int* __restrict__ sums) {
    const long long i = (long long)blockIdx.x * kEbwThreads + threadIdx.x;
    if (i < n)
        data[i] += sums[i / kEbwBlock];
}

// ---- one pass of the stable sort over the 8 bits at `shift`.  table[digit * n_blocks + block]: counts, then (scanned) places
__global__ __launch_bounds__(kEbwThreads) void ebw_sort_count_kernel(const unsigned long long* __restrict__ code, long long n, int shift, int n_blocks,
                                                                     int* __restrict__ table) {
    __shared__ int  s_cnt[256];
    const int       tid = threadIdx.x;
    s_cnt[tid]          = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kEbwBlock;
    for (int c = 0; c < kEbwBlock; c += kEbwThreads) {
        const long long i = base + c + tid;
        if (i < n)
            atomicAdd(&s_cnt[(int)((code[i] >> shift) & 255)], 1);   // an integer count: the sum does not depend on the order
    }
    __syncthreads();
    table[(long long)tid * n_blocks + blockIdx.x] = s_cnt[tid];
}

__global__ __launch_bounds__(kEbwThreads) void ebw_sort_place_kernel(const unsigned long long* __restrict__ code, const uint32_t* __restrict__ val,
                                                                     long long n, int shift, int n_blocks, const int* __restrict__ table,
                                                                     unsigned long long* __restrict__ code_out, uint32_t* __restrict__ val_out) {
    __shared__ int  s_place[256];
    __shared__ int  s_digit[kEbwThreads];
    const int       tid = threadIdx.x;
    s_place[tid]        = table[(long long)tid * n_blocks + blockIdx.x];
    __syncthreads();
    const long long base = (long long)blockIdx.x * kEbwBlock;
    for (int c = 0; c < kEbwBlock; c += kEbwThreads) {   // all lanes run every chunk
        const long long          i  = base + c + tid;
        const bool               in = i < n;
        const unsigned long long k  = in ? code[i] : 0ull;
        const int                d  = in ? (int)((k >> shift) & 255) : -1;
        s_digit[tid]                = d;
        __syncthreads();
        if (in) {
            int rank = 0;
            for (int j = 0; j < tid; ++j)
                rank += s_digit[j] == d;
            const int pos = s_place[d] + rank;
            code_out[pos] = k;
            val_out[pos]  = val[i];
        }
        __syncthreads();
        if (in)
            atomicAdd(&s_place[d], 1);
        __syncthreads();
    }
}

// ---- keys: the first item of every run of equal codes
__global__ __launch_bounds__(kEbwThreads) void ebw_heads_kernel(const unsigned long long* __restrict__ code, long long n, unsigned long long sentinel,
                                                                int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * kEbwThreads + threadIdx.x;
    if (i > n)
        return;
    flag[i] = i < n && code[i] < sentinel && (i == 0 || code[i] != code[i - 1]);   // flag[n] = 0: the scan leaves the number of keys there
}

__global__ __launch_bounds__(kEbwThreads) void ebw_keys_kernel(const unsigned long long* __restrict__ code, const uint32_t* __restrict__ val, long long n,
                                                               unsigned long long sentinel, const int* __restrict__ place, int mix_bits,
                                                               unsigned long long* __restrict__ key_code, double* __restrict__ key_w,
                                                               uint32_t* __restrict__ key_mix) {
    const long long i = (long long)blockIdx.x * kEbwThreads + threadIdx.x;
    if (i >= n)
        return;
    const unsigned long long c = code[i];
    if (c >= sentinel || (i > 0 && code[i - 1] == c))
        return;
    double sum = 0.0;   // Collector::collect: operator[] starts at 0, then += in the order the arcs were walked
    for (long long q = i; q < n && code[q] == c; ++q)
        sum += (double)__uint_as_float(val[q]);
    const int k = place[i];
    key_code[k] = c;
    key_w[k]    = sum;
    key_mix[k]  = (uint32_t)((c >> 1) & ((1ull << mix_bits) - 1ull));
}

__global__ __launch_bounds__(kEbwThreads) void ebw_gather_kernel(const float* __restrict__ feats, long long ld, int D, long long t0,
                                                                 const unsigned long long* __restrict__ key_code, int mix_bits, long long n_cells,
                                                                 float* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * kEbwThreads + threadIdx.x;
    if (i >= n_cells)
        return;
    const long long k = i / D;
    const int       c = (int)(i - k * D);
    rows[i]           = feats[(t0 + (long long)(key_code[k] >> (mix_bits + 1))) * ld + c];
}

// ---- a key's three lists: [0, nk) its slot in the mixture, then (mean, side), then (covariance, side)
__global__ __launch_bounds__(kEbwThreads) void ebw_entries_kernel(int n_keys, const unsigned long long* __restrict__ key_code, const uint32_t* __restrict__ key_mix,
                                                                  const uint32_t* __restrict__ key_best, const uint32_t* __restrict__ mix_off,
                                                                  const uint32_t* __restrict__ k_dens, const uint32_t* __restrict__ d_mean,
                                                                  const uint32_t* __restrict__ d_cov, long long nk, long long n_mean,
                                                                  unsigned long long sentinel, int32_t* __restrict__ key_slot,
                                                                  unsigned long long* __restrict__ code, uint32_t* __restrict__ val) {
    const int k = blockIdx.x * kEbwThreads + threadIdx.x;
    if (k >= n_keys)
        return;
    const uint32_t     m = key_mix[k], kk = key_best[k], nd = mix_off[m + 1] - mix_off[m];
    const int          side = (int)(key_code[k] & 1ull);
    unsigned long long c0 = sentinel, c1 = sentinel, c2 = sentinel;
    int32_t            slot = -1;
    if (kk < nd) {   // "no density" leaves the key out, as amx_gmm_accumulate_weighted_dev does
        slot             = (int32_t)(mix_off[m] + kk);
        const uint32_t d = k_dens[slot];
        c0               = (unsigned long long)slot;
        c1               = (unsigned long long)(nk + 2ll * d_mean[d] + side);
        c2               = (unsigned long long)(nk + 2ll * n_mean + 2ll * d_cov[d] + side);
    }
    key_slot[k]                = slot;
    code[3ll * k] = c0, code[3ll * k + 1] = c1, code[3ll * k + 2] = c2;
    val[3ll * k] = val[3ll * k + 1] = val[3ll * k + 2] = (uint32_t)k;
}

__global__ __launch_bounds__(kEbwThreads) void ebw_bounds_kernel(const unsigned long long* __restrict__ code, long long n, unsigned long long sentinel,
                                                                 int* __restrict__ list_begin, int* __restrict__ list_end) {
    const long long i = (long long)blockIdx.x * kEbwThreads + threadIdx.x;
    if (i >= n)
        return;
    const unsigned long long c = code[i];
    if (c >= sentinel)
        return;
    if (i == 0 || code[i - 1] != c)
        list_begin[c] = (int)i;
    if (i == n - 1 || code[i + 1] != c)
        list_end[c] = (int)(i + 1);
}

struct EbwOffsets {
    long long nk, n_mean, n_cov;
    long long mw[2], ms[2], cw[2], cs[2];   // [side]: mean weights, mean sums, covariance weights, covariance sums
    long long den_dw;                       // denWeights_
};

struct EbwArgs {
    int                       D;
    EbwOffsets                o;
    const int*                list_begin;
    const int*                list_end;
    const uint32_t*           entry_key;   // the sorted lists: key numbers
    const unsigned long long* key_code;
    const double*             key_w;
    const float*              rows;        // [keys x D]
    double*                   acc;
};

// ---- the chains.  grid: x = list, y = 256 cells of a mean's or a covariance's [weight | D sums]
template<bool FMA>
__global__ __launch_bounds__(kEbwThreads) void ebw_chain_kernel(EbwArgs a) {
    __shared__ double   s_w[kEbwStage];
    __shared__ int      s_side[kEbwStage];
    __shared__ uint32_t s_key[kEbwStage];
    const long long     lid   = blockIdx.x;
    const int           begin = a.list_begin[lid], count = a.list_end[lid] - begin;
    if (count <= 0)
        return;
    const int       D = a.D, tid = threadIdx.x;
    const long long cell = (long long)blockIdx.y * kEbwThreads + tid;
    int             fam = 0, side = 0;
    bool            active;
    double*         p = a.acc;
    if (lid < a.o.nk) {   // the slot: weights_ (lane 0, numerator keys) and denWeights_ (lane 1, denominator keys)
        if (blockIdx.y > 0)
            return;
        active = tid < 2;
        p += tid == 0 ? lid : a.o.den_dw + lid;
    }
    else {
        long long j = lid - a.o.nk;
        fam         = j < 2 * a.o.n_mean ? 1 : 2;
        if (fam == 2)
            j -= 2 * a.o.n_mean;
        side   = (int)(j & 1);
        j >>= 1;
        active = cell < 1 + D;
        if (fam == 1)
            p += cell == 0 ? a.o.mw[side] + j : a.o.ms[side] + j * D + (cell - 1);
        else
            p += cell == 0 ? a.o.cw[side] + j : a.o.cs[side] + j * D + (cell - 1);
    }
    double sum = active ? *p : 0.0;
    // a stage's key numbers, weights and sides travel in registers while the stage before it is added: the chain waits for one
    // round of loads per stage (its feature values, with the next stage's key numbers), not for three dependent ones
    uint32_t nk = 0;
    double   nw = 0.0;
    int      ns = 0;
    if (tid < kEbwStage && tid < count) {
        nk = a.entry_key[begin + tid];
        nw = a.key_w[nk];
        ns = (int)(a.key_code[nk] & 1ull);
    }
    for (int f0 = 0; f0 < count; f0 += kEbwStage) {
        const int n = count - f0 < kEbwStage ? count - f0 : kEbwStage;
        if (tid < n) {
            s_key[tid]  = nk;
            s_w[tid]    = nw;
            s_side[tid] = ns;
        }
        __syncthreads();
        const bool more = tid < kEbwStage && f0 + kEbwStage + tid < count;
        if (more)
            nk = a.entry_key[begin + f0 + kEbwStage + tid];
        float x[kEbwStage];
        if (active && fam != 0 && cell != 0) {
#pragma unroll
            for (int f = 0; f < kEbwStage; ++f)
                x[f] = f < n ? a.rows[(long long)s_key[f] * D + (cell - 1)] : 0.f;
        }
        if (more) {
            nw = a.key_w[nk];
            ns = (int)(a.key_code[nk] & 1ull);
        }
        if (active) {
            if (fam == 0) {
                for (int f = 0; f < n; ++f) {
                    const double w = s_w[f];
                    // numerator: weights_[dns] += w (MixtureEstimator.cc:92-97); denominator: denWeights_[dns] += w and nothing else
                    // (EbwDiscriminativeMixtureEstimator.cc:109-116 overrides DiscriminativeMixtureEstimator.cc:59-66 without calling it,
                    // so weights_ stays the numerator's)
                    if ((tid == 1) == (s_side[f] != 0))
                        sum += w;
                }
            }
            else if (cell == 0) {
                for (int f = 0; f < n; ++f)
                    sum += s_w[f];
            }
            else {
#pragma unroll
                for (int f = 0; f < kEbwStage; ++f)
                    if (f < n) {
                        const double w = s_w[f], y = (double)x[f];
                        sum            = fam == 1 ? mad<FMA>(w, y, sum) : mad<FMA>(w * y, y, sum);   // x + w * y;  x + w * y * y
                    }
            }
        }
        __syncthreads();
    }
    if (active)
        *p = sum;
}

__global__ void ebw_objective_kernel(double* cell, float objective) {
    *cell += (double)objective;   // accumulateObjectiveFunction(f32)
}

}  // namespace amx

struct amx_ebw {
    amx_gmm*              scorer = nullptr;
    amx_internal_gmm_view gmm{};
    amx_ebw_cfg           cfg{};
    int                   D = 0, device = 0;
    long long             nk = 0;
    amx_ebw_offsets       off{};
    int                   n_keys = 0, mix_bits = 1;   // the last call's keys
    amx_ebw_call_shape    last{};                     // ... and the launches it ran
    // per-call workspace
    amx::DevBuf<long long>          d_off;       // frame, arc and item offsets
    amx::DevBuf<float>              d_arc_w;
    amx::DevBuf<int32_t>            d_item;      // frames, emissions
    amx::DevBuf<unsigned long long> d_code[2];   // the sort's two sides: items
    amx::DevBuf<uint32_t>           d_val[2];
    amx::DevBuf<unsigned long long> d_ecode[2];  // list entries
    amx::DevBuf<uint32_t>           d_eval[2];
    amx::DevBuf<int>                d_table, d_scan_ws, d_flag, d_touched, d_lists;
    amx::DevBuf<unsigned long long> d_key_code;
    amx::DevBuf<double>             d_key_w;
    amx::DevBuf<uint32_t>           d_key_mix, d_key_best;
    amx::DevBuf<int32_t>            d_key_slot;
    amx::DevBuf<float>              d_rows;
    amx::DevBuf<unsigned long long> d_bad;
};

namespace {

int bit_length(long long v) {   // bits that hold every value of [0, v]
    int b = 1;
    while ((v >> b) != 0)
        ++b;
    return b;
}

// exclusive scan in place; ws holds the block totals of every level.  *levels (nullable) counts the levels that ran
int ebw_scan(hipStream_t st, int* data, long long n, int* ws, int* levels = nullptr) {
    const long long nb = (n + amx::kEbwBlock - 1) / amx::kEbwBlock;
    if (levels)
        ++*levels;
    hipLaunchKernelGGL(amx::ebw_scan_block_kernel, dim3((unsigned)nb), dim3(amx::kEbwThreads), 0, st, data, n, ws);
    AMX_HIP(hipGetLastError());
    if (nb > 1) {
        AMX_TRY(ebw_scan(st, ws, nb, ws + nb, levels));
        hipLaunchKernelGGL(amx::ebw_scan_add_kernel, dim3((unsigned)amx::ceil_div(n, amx::kEbwThreads)), dim3(amx::kEbwThreads), 0, st, data, n,
                           (const int*)ws);
        AMX_HIP(hipGetLastError());
    }
    return AMX_OK;
}

size_t ebw_scan_ws(long long n) {
    size_t total = 0;
    while (n > 1) {
        n = (n + amx::kEbwBlock - 1) / amx::kEbwBlock;
        total += (size_t)n;
    }
    return total + 1;
}

// stable sort of (code, val) by the low `bits` bits of code; *side: which of the two buffers holds the result; what ran goes to
// *passes, *blocks and *recursed (the scan of the digit table took more than one level)
int ebw_sort(amx_ebw* h, hipStream_t st, amx::DevBuf<unsigned long long>* code, amx::DevBuf<uint32_t>* val, long long n, int bits, int* side,
             int* passes, int* blocks, int* recursed) {
    const int nb = (int)((n + amx::kEbwBlock - 1) / amx::kEbwBlock);
    if (h->d_table.capacity() < (size_t)256 * nb || h->d_scan_ws.capacity() < ebw_scan_ws(256ll * nb))
        AMX_HIP(hipStreamSynchronize(st));   // a workspace that grows is freed first: nothing in flight may still read it
    AMX_TRY(h->d_table.reserve((size_t)256 * nb));
    AMX_TRY(h->d_scan_ws.reserve(ebw_scan_ws(256ll * nb)));
    int cur = 0;
    *passes = 0, *blocks = nb, *recursed = 0;
    for (int shift = 0; shift < bits; shift += 8, cur ^= 1) {
        int levels = 0;
        hipLaunchKernelGGL(amx::ebw_sort_count_kernel, dim3((unsigned)nb), dim3(amx::kEbwThreads), 0, st, (const unsigned long long*)code[cur].get(), n, shift,
                           nb, h->d_table.get());
        AMX_HIP(hipGetLastError());
        AMX_TRY(ebw_scan(st, h->d_table.get(), 256ll * nb, h->d_scan_ws.get(), &levels));
        ++*passes;
        if (levels > 1)
            *recursed = 1;
        hipLaunchKernelGGL(amx::ebw_sort_place_kernel, dim3((unsigned)nb), dim3(amx::kEbwThreads), 0, st, (const unsigned long long*)code[cur].get(),
                           (const uint32_t*)val[cur].get(), n, shift, nb, (const int*)h->d_table.get(), code[cur ^ 1].get(), val[cur ^ 1].get());
        AMX_HIP(hipGetLastError());
    }
    *side = cur;
    return AMX_OK;
}

}  // namespace

extern "C" {

void amx_ebw_cfg_default(amx_ebw_cfg* cfg) {
    if (!cfg)
        return;
    cfg->weight_threshold = 1.1920928955078125e-07f;   // Core::Type<f32>::epsilon
    cfg->viterbi          = 1;
}

int amx_ebw_create(amx_gmm* gmm, const amx_ebw_cfg* cfg, amx_ebw** out) {
    const char* who = "amx_ebw_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(gmm, AMX_ERR_INVALID, "%s: NULL gmm handle", who);
    std::unique_ptr<amx_ebw> h(new amx_ebw);
    amx_ebw_cfg_default(&h->cfg);
    if (cfg)
        h->cfg = *cfg;
    AMX_REQUIRE(h->cfg.viterbi != 0, AMX_ERR_UNSUPPORTED,
                "%s: viterbi = false (getDensityPosteriorProbabilities) is not supported: only the best density of a key's mixture is", who);
    AMX_REQUIRE(!std::isnan(h->cfg.weight_threshold), AMX_ERR_INVALID, "%s: weight_threshold is not a number", who);
    AMX_TRY(amx_internal_gmm_view_get(gmm, &h->gmm));
    h->scorer = gmm;
    h->D      = h->gmm.dim;
    const long long n_mean = h->gmm.n_mean, n_cov = h->gmm.n_cov, D = h->D;
    const long long base   = amx_gmm_accumulator_size(gmm);
    h->nk                  = base - n_mean * (1 + D) - n_cov * (1 + D);
    AMX_REQUIRE(h->nk + 2 * n_mean + 2 * n_cov < (1ll << 31), AMX_ERR_UNSUPPORTED, "%s: the model is too large", who);
    amx_ebw_offsets& o = h->off;
    o.num_mixture_weights = 0, o.num_mean_weights = h->nk, o.num_mean_sums = o.num_mean_weights + n_mean;
    o.num_cov_weights = o.num_mean_sums + n_mean * D, o.num_cov_sums = o.num_cov_weights + n_cov;
    o.den_density_weights = base, o.den_mean_weights = base + h->nk, o.den_mean_sums = o.den_mean_weights + n_mean;
    o.den_cov_weights = o.den_mean_sums + n_mean * D, o.den_cov_sums = o.den_cov_weights + n_cov;
    o.objective = o.den_cov_sums + n_cov * D, o.size = o.objective + 1;
    o.n_slots = h->nk, o.n_means = n_mean, o.n_covariances = n_cov, o.dim = D;
    if (h->gmm.ctx) {
        h->device = h->gmm.ctx->device;
        AMX_HIP(hipSetDevice(h->device));
        // a scorer without diagonal-maximum tables on the device cannot give a key's density: refused here (a call of no frames runs
        // that check and launches nothing), not inside the first pass.  Every scorer handle created on a context uploads those tables
        // today, so no test can reach this refusal through the ABI: whoever adds a scorer without them owes the test
        AMX_TRY(amx_gmm_best_density_dev(gmm, nullptr, 0, nullptr, nullptr, nullptr));
        AMX_TRY(h->d_bad.reserve(1));
    }
    *out = h.release();
    return AMX_OK;
}

void amx_ebw_destroy(amx_ebw* h) {
    if (!h)
        return;
    if (h->gmm.ctx)
        hipSetDevice(h->device);
    delete h;
}

long amx_ebw_accumulator_size(const amx_ebw* h) {
    return h ? (long)h->off.size : 0;
}

int amx_ebw_layout(const amx_ebw* h, amx_ebw_offsets* out) {
    AMX_REQUIRE(h && out, AMX_ERR_INVALID, "amx_ebw_layout: NULL argument");
    *out = h->off;
    return AMX_OK;
}

int amx_ebw_accumulate_objective(amx_ebw* h, float objective, double* acc_dev) {
    const char* who = "amx_ebw_accumulate_objective";
    AMX_REQUIRE(h && acc_dev, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(h->gmm.ctx, AMX_ERR_STATE, "%s: host-only gmm handle (created without a context)", who);
    AMX_REQUIRE(std::isfinite(objective), AMX_ERR_INVALID, "%s: the objective is not finite", who);
    AMX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(amx::ebw_objective_kernel, dim3(1), dim3(1), 0, h->gmm.ctx->stream, acc_dev + h->off.objective, objective);
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

int amx_ebw_accumulate_dev(amx_ebw* h, const float* feats_dev, int feats_ld, int n_seg, const long* frame_offsets, const long* arc_offsets,
                           const float* arc_weight, const long* item_offsets, const int32_t* item_frame, const int32_t* item_emission,
                           double* acc_dev) {
    const char* who = "amx_ebw_accumulate_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    h->last = amx_ebw_call_shape{};   // before any refusal: the shape is this call's, never the one before's
    AMX_REQUIRE(n_seg >= 0 && feats_ld >= h->D, AMX_ERR_INVALID, "%s: n_seg %d, feats_ld %d (dimension %d)", who, n_seg, feats_ld, h->D);
    AMX_REQUIRE(h->gmm.ctx, AMX_ERR_STATE, "%s: host-only gmm handle (created without a context)", who);
    h->n_keys = 0;
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(frame_offsets && arc_offsets, AMX_ERR_INVALID, "%s: NULL frame_offsets or arc_offsets", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: frame_offsets[0] = %ld is negative", who, frame_offsets[0]);
    AMX_REQUIRE(arc_offsets[0] == 0, AMX_ERR_INVALID, "%s: arc_offsets[0] = %ld is not 0", who, arc_offsets[0]);
    for (int s = 0; s < n_seg; ++s) {
        AMX_REQUIRE(frame_offsets[s + 1] >= frame_offsets[s], AMX_ERR_INVALID, "%s: frame_offsets decrease at segment %d (%ld after %ld)", who, s,
                    frame_offsets[s + 1], frame_offsets[s]);
        AMX_REQUIRE(arc_offsets[s + 1] >= arc_offsets[s], AMX_ERR_INVALID, "%s: arc_offsets decrease at segment %d (%ld after %ld)", who, s,
                    arc_offsets[s + 1], arc_offsets[s]);
    }
    const long long t0 = frame_offsets[0], n = frame_offsets[n_seg] - t0, n_arcs = arc_offsets[n_seg];
    if (n_arcs == 0)
        return AMX_OK;
    AMX_REQUIRE(arc_weight && item_offsets, AMX_ERR_INVALID, "%s: NULL arc_weight or item_offsets", who);
    AMX_REQUIRE(item_offsets[0] == 0, AMX_ERR_INVALID, "%s: item_offsets[0] = %ld is not 0", who, item_offsets[0]);
    for (long long a = 0; a < n_arcs; ++a)
        AMX_REQUIRE(item_offsets[a + 1] >= item_offsets[a], AMX_ERR_INVALID, "%s: item_offsets decrease at arc %lld (%ld after %ld)", who, a,
                    item_offsets[a + 1], item_offsets[a]);
    const long long n_items = item_offsets[n_arcs];
    AMX_REQUIRE(n < amx::kEbwMaxFrames, AMX_ERR_INVALID, "%s: %lld frames are more than one call takes", who, n);
    AMX_REQUIRE(n_items < amx::kEbwMaxItems && n_arcs < amx::kEbwMaxItems, AMX_ERR_INVALID, "%s: %lld arcs with %lld items are more than one call takes",
                who, n_arcs, n_items);
    AMX_REQUIRE(n_items == 0 || (item_frame && item_emission), AMX_ERR_INVALID, "%s: NULL item_frame or item_emission", who);
    AMX_REQUIRE(feats_dev && acc_dev, AMX_ERR_INVALID, "%s: NULL feats_dev or acc_dev", who);
    amx_ctx* ctx = h->gmm.ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int   D = h->D, n_mix = h->gmm.n_mix;

    // the tables
    std::vector<long long> off;
    off.reserve((size_t)2 * n_seg + 2 + (size_t)n_arcs + 1);
    off.insert(off.end(), frame_offsets, frame_offsets + n_seg + 1);
    off.insert(off.end(), arc_offsets, arc_offsets + n_seg + 1);
    off.insert(off.end(), item_offsets, item_offsets + n_arcs + 1);
    const long long n_slots = std::max<long long>(n_items, 1);
    AMX_TRY(h->d_off.reserve(off.size()));
    AMX_TRY(h->d_arc_w.reserve((size_t)n_arcs));
    AMX_TRY(h->d_item.reserve((size_t)2 * n_slots));
    AMX_TRY(h->d_touched.reserve((size_t)std::max<long long>(n, 1)));
    for (int i = 0; i < 2; ++i) {
        AMX_TRY(h->d_code[i].reserve((size_t)n_slots));
        AMX_TRY(h->d_val[i].reserve((size_t)n_slots));
    }
    AMX_TRY(h->d_flag.reserve((size_t)n_slots + 1));
    AMX_HIP(hipMemcpyAsync(h->d_off.get(), off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(h->d_arc_w.get(), arc_weight, (size_t)n_arcs * sizeof(float), hipMemcpyHostToDevice, st));
    if (n_items) {
        AMX_HIP(hipMemcpyAsync(h->d_item.get(), item_frame, (size_t)n_items * sizeof(int32_t), hipMemcpyHostToDevice, st));
        AMX_HIP(hipMemcpyAsync(h->d_item.get() + n_slots, item_emission, (size_t)n_items * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    AMX_HIP(hipMemsetAsync(h->d_bad.get(), 0xff, sizeof(unsigned long long), st));
    AMX_HIP(hipMemsetAsync(h->d_touched.get(), 0, (size_t)std::max<long long>(n, 1) * sizeof(int), st));
    const long long* d_frame_off = h->d_off.get();
    const long long* d_arc_off   = d_frame_off + n_seg + 1;
    const long long* d_item_off  = d_arc_off + n_seg + 1;

    // 1. sides, codes and checks, before anything is written
    const int                mix_bits = bit_length(n_mix - 1), frame_bits = bit_length(std::max<long long>(n, 1) - 1);
    const int                code_bits = frame_bits + mix_bits + 1;
    const unsigned long long sentinel  = 1ull << code_bits;
    {
        amx::ScopedKernelTimer timer(ctx, "ebw_resolve");
        hipLaunchKernelGGL(amx::ebw_resolve_kernel, dim3((unsigned)amx::ceil_div(std::max(n_items, n_arcs), amx::kEbwThreads)), dim3(amx::kEbwThreads), 0, st,
                           n_items, n_arcs, n_seg, d_frame_off, d_arc_off, (const float*)h->d_arc_w.get(), d_item_off, (const int32_t*)h->d_item.get(),
                           (const int32_t*)(h->d_item.get() + n_slots), h->cfg.weight_threshold, n_mix, mix_bits, sentinel, h->d_code[0].get(),
                           h->d_val[0].get(), h->d_touched.get(), h->d_bad.get());
        AMX_HIP(hipGetLastError());
        if (n > 0) {
            hipLaunchKernelGGL(amx::ebw_rows_kernel, dim3((unsigned)amx::ceil_div(n, amx::kEbwThreads)), dim3(amx::kEbwThreads), 0, st, feats_dev,
                               (long long)feats_ld, D, t0, n, (const int*)h->d_touched.get(), h->d_bad.get());
            AMX_HIP(hipGetLastError());
        }
    }
    unsigned long long bad = 0;
    AMX_HIP(hipMemcpyAsync(&bad, h->d_bad.get(), sizeof(bad), hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    if (bad != ~0ull) {
        const long long i    = (long long)(bad >> 3);
        const int       kind = (int)(bad & 7);
        if (kind == 1)
            amx::set_error("%s: item %lld: frame %d is outside its segment", who, i, item_frame[i]);
        else if (kind == 2)
            amx::set_error("%s: item %lld: emission index %d is outside [0, %d)", who, i, item_emission[i], n_mix);
        else if (kind == 3)
            amx::set_error("%s: arc %lld: non-finite weight", who, i);
        else
            amx::set_error("%s: frame %lld: non-finite feature", who, t0 + i);
        return AMX_ERR_INVALID;
    }
    if (n_items == 0)
        return AMX_OK;

    // 2. the items in (frame, mixture, side) order, the keys and their collected weights
    int side = 0;
    {
        amx::ScopedKernelTimer timer(ctx, "ebw_sort_items");
        AMX_TRY(ebw_sort(h, st, h->d_code, h->d_val, n_items, code_bits + 1, &side, &h->last.item_sort_passes, &h->last.item_blocks,
                         &h->last.item_table_recursed));
    }
    const unsigned long long* s_code = h->d_code[side].get();
    const uint32_t*           s_val  = h->d_val[side].get();
    if (h->d_scan_ws.capacity() < ebw_scan_ws(n_items + 1))
        AMX_HIP(hipStreamSynchronize(st));
    AMX_TRY(h->d_scan_ws.reserve(ebw_scan_ws(n_items + 1)));
    int n_keys = 0;
    {
        amx::ScopedKernelTimer timer(ctx, "ebw_keys");
        hipLaunchKernelGGL(amx::ebw_heads_kernel, dim3((unsigned)amx::ceil_div(n_items + 1, amx::kEbwThreads)), dim3(amx::kEbwThreads), 0, st, s_code, n_items,
                           sentinel, h->d_flag.get());
        AMX_HIP(hipGetLastError());
        AMX_TRY(ebw_scan(st, h->d_flag.get(), n_items + 1, h->d_scan_ws.get()));
        AMX_HIP(hipMemcpyAsync(&n_keys, h->d_flag.get() + n_items, sizeof(int), hipMemcpyDeviceToHost, st));
        AMX_HIP(hipStreamSynchronize(st));
    }
    if (n_keys == 0)
        return AMX_OK;
    AMX_TRY(h->d_key_code.reserve((size_t)n_keys));
    AMX_TRY(h->d_key_w.reserve((size_t)n_keys));
    AMX_TRY(h->d_key_mix.reserve((size_t)n_keys));
    AMX_TRY(h->d_key_best.reserve((size_t)n_keys));
    AMX_TRY(h->d_key_slot.reserve((size_t)n_keys));
    AMX_TRY(h->d_rows.reserve((size_t)n_keys * D));
    const long long n_entries = 3ll * n_keys;
    for (int i = 0; i < 2; ++i) {
        AMX_TRY(h->d_ecode[i].reserve((size_t)n_entries));
        AMX_TRY(h->d_eval[i].reserve((size_t)n_entries));
    }
    const long long n_lists = h->nk + 2ll * h->gmm.n_mean + 2ll * h->gmm.n_cov;
    AMX_TRY(h->d_lists.reserve((size_t)2 * n_lists));
    {
        amx::ScopedKernelTimer timer(ctx, "ebw_keys");
        hipLaunchKernelGGL(amx::ebw_keys_kernel, dim3((unsigned)amx::ceil_div(n_items, amx::kEbwThreads)), dim3(amx::kEbwThreads), 0, st, s_code, s_val, n_items,
                           sentinel, (const int*)h->d_flag.get(), mix_bits, h->d_key_code.get(), h->d_key_w.get(), h->d_key_mix.get());
        AMX_HIP(hipGetLastError());
        hipLaunchKernelGGL(amx::ebw_gather_kernel, dim3((unsigned)amx::ceil_div((long long)n_keys * D, amx::kEbwThreads)), dim3(amx::kEbwThreads), 0, st,
                           feats_dev, (long long)feats_ld, D, t0, (const unsigned long long*)h->d_key_code.get(), mix_bits, (long long)n_keys * D,
                           h->d_rows.get());
        AMX_HIP(hipGetLastError());
    }
    h->n_keys = n_keys, h->mix_bits = mix_bits;

    // 3. the best density of every key, its three lists
    AMX_TRY(amx_gmm_best_density_dev(h->scorer, h->d_rows.get(), n_keys, h->d_key_mix.get(), h->d_key_best.get(), nullptr));
    const int                list_bits = bit_length(n_lists - 1);
    const unsigned long long list_end  = 1ull << list_bits;
    {
        amx::ScopedKernelTimer timer(ctx, "ebw_sort_lists");
        hipLaunchKernelGGL(amx::ebw_entries_kernel, dim3((unsigned)amx::ceil_div(n_keys, amx::kEbwThreads)), dim3(amx::kEbwThreads), 0, st, n_keys,
                           (const unsigned long long*)h->d_key_code.get(), (const uint32_t*)h->d_key_mix.get(), (const uint32_t*)h->d_key_best.get(),
                           h->gmm.d_mix_off, h->gmm.d_k_dens, h->gmm.d_d_mean, h->gmm.d_d_cov, h->nk, (long long)h->gmm.n_mean, list_end,
                           h->d_key_slot.get(), h->d_ecode[0].get(), h->d_eval[0].get());
        AMX_HIP(hipGetLastError());
        AMX_TRY(ebw_sort(h, st, h->d_ecode, h->d_eval, n_entries, list_bits + 1, &side, &h->last.list_sort_passes, &h->last.list_blocks,
                         &h->last.list_table_recursed));
        AMX_HIP(hipMemsetAsync(h->d_lists.get(), 0, (size_t)2 * n_lists * sizeof(int), st));
        hipLaunchKernelGGL(amx::ebw_bounds_kernel, dim3((unsigned)amx::ceil_div(n_entries, amx::kEbwThreads)), dim3(amx::kEbwThreads), 0, st,
                           (const unsigned long long*)h->d_ecode[side].get(), n_entries, list_end, h->d_lists.get(), h->d_lists.get() + n_lists);
        AMX_HIP(hipGetLastError());
    }

    // 4. the chains
    amx::EbwArgs a{};
    a.D = D, a.o.nk = h->nk, a.o.n_mean = h->gmm.n_mean, a.o.n_cov = h->gmm.n_cov;
    a.o.mw[0] = h->off.num_mean_weights, a.o.ms[0] = h->off.num_mean_sums, a.o.cw[0] = h->off.num_cov_weights, a.o.cs[0] = h->off.num_cov_sums;
    a.o.mw[1] = h->off.den_mean_weights, a.o.ms[1] = h->off.den_mean_sums, a.o.cw[1] = h->off.den_cov_weights, a.o.cs[1] = h->off.den_cov_sums;
    a.o.den_dw = h->off.den_density_weights;
    a.list_begin = h->d_lists.get(), a.list_end = h->d_lists.get() + n_lists, a.entry_key = h->d_eval[side].get();
    a.key_code = h->d_key_code.get(), a.key_w = h->d_key_w.get(), a.rows = h->d_rows.get(), a.acc = acc_dev;
    {
        amx::ScopedKernelTimer timer(ctx, "ebw_chains");
        const dim3             grid((unsigned)n_lists, (unsigned)amx::ceil_div(1 + D, amx::kEbwThreads));
        hipLaunchKernelGGL((ctx->contract == AMX_CONTRACT_FMA ? amx::ebw_chain_kernel<true> : amx::ebw_chain_kernel<false>), grid, dim3(amx::kEbwThreads),
                           0, st, a);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(st));   // the workspace is the handle's, the tables are this call's
    return AMX_OK;
}

void amx_ebw_kernel_shape(int* block_items, int* stage_keys, int* threads) {
    if (block_items)
        *block_items = amx::kEbwBlock;
    if (stage_keys)
        *stage_keys = amx::kEbwStage;
    if (threads)
        *threads = amx::kEbwThreads;
}

int amx_ebw_last_shape(const amx_ebw* h, amx_ebw_call_shape* out) {
    AMX_REQUIRE(h && out, AMX_ERR_INVALID, "amx_ebw_last_shape: NULL argument");
    *out = h->last;
    return AMX_OK;
}

int amx_ebw_last_keys(const amx_ebw* h, int capacity, int* n_keys, long* frame, int32_t* mixture, int32_t* side, double* weight, int32_t* slot) {
    const char* who = "amx_ebw_last_keys";
    AMX_REQUIRE(h && n_keys, AMX_ERR_INVALID, "%s: NULL argument", who);
    *n_keys = h->n_keys;
    if (!frame && !mixture && !side && !weight && !slot)
        return AMX_OK;
    AMX_REQUIRE(capacity >= h->n_keys, AMX_ERR_INVALID, "%s: capacity %d is below the %d keys", who, capacity, h->n_keys);
    if (h->n_keys == 0)
        return AMX_OK;
    AMX_HIP(hipSetDevice(h->device));
    const size_t                    nkeys = (size_t)h->n_keys;
    std::vector<unsigned long long> code(nkeys);
    AMX_HIP(hipMemcpy(code.data(), h->d_key_code.get(), nkeys * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nkeys; ++k) {
        if (frame)
            frame[k] = (long)(code[k] >> (h->mix_bits + 1));
        if (mixture)
            mixture[k] = (int32_t)((code[k] >> 1) & ((1ull << h->mix_bits) - 1ull));
        if (side)
            side[k] = (int32_t)(code[k] & 1ull);
    }
    if (weight)
        AMX_HIP(hipMemcpy(weight, h->d_key_w.get(), nkeys * sizeof(double), hipMemcpyDeviceToHost));
    if (slot)
        AMX_HIP(hipMemcpy(slot, h->d_key_slot.get(), nkeys * sizeof(int32_t), hipMemcpyDeviceToHost));
    return AMX_OK;
}

}  // extern "C"
