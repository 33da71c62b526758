// histogram.hip -- histogram normalisation on the device: the corpus pass of Speech::HistogramEstimator (Speech/HistogramEstimator.cc,
// Signal/Histogram.hh:46-48, 107-112, Signal/LookupTable.hh:69-72, 178-202) and the two look-ups of Signal::HistogramNormalization::apply
// (Signal/HistogramNormalization.cc:68-75).
//
// Estimation.  A finished histogram depends only on the multiset of bucket indices k = (s32)round(x / bucket_size): offset_ = -min k,
// size = max k - min k + 1, f_[b] = number of frames with k = b - offset_ (as f32, which stops at 2^24).  The quotient is the correctly
// rounded f32 division (the compiler's default for `/`), round() is half away from zero (roundf).  One call is three steps:
//   hist_range_kernel   min / max k of every dimension over the call's frames and one flag for a value the cast is undefined for
//   host                reads those 2 dim + 1 integers (ONE synchronisation per call), grows the flat count buffer if a window grew
//   hist_count_kernel   counts: u32 atomics, in a workgroup-private LDS table for narrow windows, straight to memory for wide ones
// Both kernels read rows coalesced: consecutive lanes take consecutive components of a frame.
//
// Application.  out = inverse[ cdf_key[x] ]: two dependent gathers per element, the key chosen per segment inside the kernel.
#include <algorithm>
#include <climits>
#include <cstring>

#include "histogram.hpp"

namespace amx {

constexpr int kHistThreads = 256;

// element e of a chunk of frames is (frame e / dim, component e % dim); a thread walks e = tid, tid + 256, ... without dividing again
struct ElementWalk {
    long t;
    int  d, step_t, step_d, dim;
    __device__ ElementWalk(long t0, int tid, int dim_) : dim(dim_) {
        t      = t0 + tid / dim;
        d      = tid % dim;
        step_t = kHistThreads / dim;
        step_d = kHistThreads % dim;
    }
    __device__ void next() {
        t += step_t;
        d += step_d;
        if (d >= dim) {
            d -= dim;
            ++t;
        }
    }
};

// range[0 .. dim) = min k, range[dim .. 2 dim) = max k (initialised by the host to INT_MAX / INT_MIN), range[2 dim] = 1 if a value is not
// finite or |x / bucket_size| >= 2^30.  Workgroup-private min / max in LDS (read first, an atomic only when it would change something).
__global__ __launch_bounds__(kHistThreads) void hist_range_kernel(const float* __restrict__ feats, int in_ld, long T, int dim, float bucket_size,
                                                                  long frames_per_group, int* __restrict__ range) {
    extern __shared__ int s_range[];  // [2 dim]
    const int tid = threadIdx.x;
    for (int i = tid; i < dim; i += kHistThreads) {
        s_range[i]       = INT_MAX;
        s_range[dim + i] = INT_MIN;
    }
    __syncthreads();
    const long t0 = (long)blockIdx.x * frames_per_group;
    const long t1 = t0 + frames_per_group < T ? t0 + frames_per_group : T;
    bool       bad = false;
    for (ElementWalk w(t0, tid, dim); w.t < t1; w.next()) {
        const float q = feats[(size_t)w.t * in_ld + w.d] / bucket_size;
        if (!(fabsf(q) < kHistMaxQuotient)) {
            bad = true;
            continue;
        }
        const int k = (int)roundf(q);
        if (k < s_range[w.d])
            atomicMin(&s_range[w.d], k);
        if (k > s_range[dim + w.d])
            atomicMax(&s_range[dim + w.d], k);
    }
    if (bad)
        atomicOr(&range[2 * dim], 1);
    __syncthreads();
    for (int i = tid; i < dim; i += kHistThreads) {
        if (s_range[i] != INT_MAX)
            atomicMin(&range[i], s_range[i]);
        if (s_range[dim + i] != INT_MIN)
            atomicMax(&range[dim + i], s_range[dim + i]);
    }
}

// meta[d]: the window of dimension d and where it counts.  The range pass has shown every k to lie inside its window; the comparison
// below still keeps a bucket outside it (a buffer changed between the two kernels) from reaching memory.
__global__ __launch_bounds__(kHistThreads) void hist_count_kernel(const float* __restrict__ feats, int in_ld, long T, int dim, float bucket_size,
                                                                  long frames_per_group, const HistDimMeta* __restrict__ meta, int lds_words,
                                                                  uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t s_tab[];  // [lds_words]
    const int tid = threadIdx.x;
    for (int i = tid; i < lds_words; i += kHistThreads)
        s_tab[i] = 0;
    __syncthreads();
    const long t0 = (long)blockIdx.x * frames_per_group;
    const long t1 = t0 + frames_per_group < T ? t0 + frames_per_group : T;
    for (ElementWalk w(t0, tid, dim); w.t < t1; w.next()) {
        const float       q = feats[(size_t)w.t * in_ld + w.d] / bucket_size;
        const HistDimMeta m = meta[w.d];
        if (!(fabsf(q) < kHistMaxQuotient))
            continue;
        const int b = (int)roundf(q) - m.kmin;  // |k|, |kmin| < 2^30: no overflow
        if ((unsigned)b >= (unsigned)m.size)
            continue;
        if (m.lds_off >= 0)
            atomicAdd(&s_tab[m.lds_off + b], 1u);
        else
            atomicAdd(&counts[m.off + b], 1u);
    }
    if (lds_words == 0)
        return;
    __syncthreads();
    for (int d = 0; d < dim; ++d) {
        const HistDimMeta m = meta[d];
        if (m.lds_off < 0)
            continue;
        for (int i = tid; i < m.size; i += kHistThreads) {
            const uint32_t v = s_tab[m.lds_off + i];
            if (v)
                atomicAdd(&counts[m.off + i], v);
        }
    }
}

// a look-up as the reference's release build does it, with the one rule added that a bucket outside the table is the nearest end bucket
// (what LookupTable::insert does on a table that may not grow); *clamped counts those.  NaN: bucket 0, counted, and the caller writes NaN.
__device__ __forceinline__ float hist_lookup(const TableMeta& m, float x, unsigned& clamped) {
    float r = roundf(x / m.bucket_size);
    if (r != r) {
        ++clamped;
        return m.values[0];
    }
    r             = fminf(fmaxf(r, -2147483648.f), 2147483520.f);
    long long b   = (long long)(int)r + m.offset;
    const bool lo = b < 0, hi = b >= m.size;
    if (lo || hi) {
        ++clamped;
        b = lo ? 0 : m.size - 1;
    }
    return m.values[b];
}

// seg[0 .. n_seg] frame offsets, seg[n_seg + 1 .. 2 n_seg] keys.  A workgroup takes frames_per_group frames; it finds the segment of its
// first frame by bisection (uniform over the workgroup), a thread then steps forward from there as its frame index grows.
__global__ __launch_bounds__(kHistThreads) void histnorm_apply_kernel(const float* in, int in_ld, float* out, int out_ld, int dim, int n_seg,
                                                                      const long long* __restrict__ seg, const TableMeta* __restrict__ meta,
                                                                      long frames_per_group, unsigned long long* __restrict__ clamped) {
    const int       tid   = threadIdx.x;
    const long long first = seg[0], last = seg[n_seg];
    const long      t0 = first + (long)blockIdx.x * frames_per_group;
    const long      t1 = t0 + frames_per_group < last ? t0 + frames_per_group : last;
    int             lo = 0, hi = n_seg - 1;  // the last segment s with seg[s] <= t0
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= t0)
            lo = mid;
        else
            hi = mid - 1;
    }
    int      s = lo;
    unsigned c_test = 0, c_inv = 0;
    for (ElementWalk w(t0, tid, dim); w.t < t1; w.next()) {
        while (s + 1 < n_seg && seg[s + 1] <= w.t)
            ++s;
        const int       key = (int)seg[n_seg + 1 + s];
        const float     x   = in[(size_t)w.t * in_ld + w.d];
        const TableMeta mt  = meta[(size_t)(1 + key) * dim + w.d];
        const TableMeta mi  = meta[w.d];
        const float     p   = hist_lookup(mt, x, c_test);
        float           y   = hist_lookup(mi, p, c_inv);
        if (x != x)
            y = x;
        out[(size_t)w.t * out_ld + w.d] = y;
    }
    // one atomic per wave and counter, and only where something was clamped
    for (int o = 32; o > 0; o >>= 1) {
        c_test += __shfl_down(c_test, o);
        c_inv += __shfl_down(c_inv, o);
    }
    if ((tid & 63) == 0) {
        if (c_test)
            atomicAdd(&clamped[0], (unsigned long long)c_test);
        if (c_inv)
            atomicAdd(&clamped[1], (unsigned long long)c_inv);
    }
}

// frames per workgroup: enough workgroups to fill the chip a few times, each with at least a few thousand elements
static long frames_per_group(const amx_ctx* ctx, long T, int dim) {
    const long n_cu   = ctx->n_cu > 0 ? ctx->n_cu : 256;
    const long least  = std::max<long>(1, (16 * kHistThreads + dim - 1) / dim);
    const long spread = (T + 8 * n_cu - 1) / (8 * n_cu);
    return std::max(least, spread);
}

// the device's counts -> the host's
int hist_sync_host(const amx_histogram* hc) {
    amx_histogram* h = const_cast<amx_histogram*>(hc);
    if (h->host_valid || h->frozen)
        return AMX_OK;
    AMX_HIP(hipSetDevice(h->ctx->device));
    AMX_HIP(hipStreamSynchronize(h->ctx->stream));
    for (int d = 0; d < h->dim; ++d) {
        HistCounts& c = h->counts[d];
        c.offset      = -h->d_kmin[d];
        c.c.resize((size_t)h->d_size[d]);
        if (h->d_size[d])
            AMX_HIP(hipMemcpy(c.c.data(), h->d_counts->get() + h->d_off[d], (size_t)h->d_size[d] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    h->host_valid = true;
    return AMX_OK;
}

// the device's flat buffer laid out for windows [kmin[d], kmin[d] + size[d]), holding what `from` (host counts, or the old device buffer)
// held; the old buffer is released
static int hist_lay_out(amx_histogram* h, const std::vector<int32_t>& kmin, const std::vector<int32_t>& size, bool from_host) {
    std::vector<long long> off((size_t)h->dim + 1, 0);
    for (int d = 0; d < h->dim; ++d)
        off[d + 1] = off[d] + size[d];
    std::unique_ptr<DevBuf<uint32_t>> fresh(new DevBuf<uint32_t>);
    AMX_TRY(fresh->reserve((size_t)std::max<long long>(off[h->dim], 1)));
    AMX_HIP(hipMemsetAsync(fresh->get(), 0, (size_t)std::max<long long>(off[h->dim], 1) * sizeof(uint32_t), h->ctx->stream));
    for (int d = 0; d < h->dim; ++d) {
        if (from_host) {
            const HistCounts& c = h->counts[d];
            if (!c.c.empty())
                AMX_HIP(hipMemcpyAsync(fresh->get() + off[d] + (-(long long)c.offset - kmin[d]), c.c.data(), c.c.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                       h->ctx->stream));
        }
        else if (h->d_size[d])
            AMX_HIP(hipMemcpyAsync(fresh->get() + off[d] + ((long long)h->d_kmin[d] - kmin[d]), h->d_counts->get() + h->d_off[d],
                                   (size_t)h->d_size[d] * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->ctx->stream));
    }
    AMX_HIP(hipStreamSynchronize(h->ctx->stream));  // the old buffer is freed below, the host's vectors may change
    h->d_counts = std::move(fresh);
    h->d_kmin = kmin;
    h->d_size = size;
    h->d_off  = off;
    return AMX_OK;
}

}  // namespace amx

extern "C" {

int amx_histogram_accumulate_dev(amx_histogram* h, const float* feats_dev, int in_ld, long T) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_histogram_accumulate_dev: NULL handle");
    AMX_REQUIRE(!h->frozen, AMX_ERR_STATE,
                "amx_histogram_accumulate_dev: the handle was read from a file whose values are not counts; it only serves tables");
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "amx_histogram_accumulate_dev: the handle has no context (amx_histogram_attach)");
    AMX_REQUIRE(in_ld >= h->dim && T >= 0, AMX_ERR_INVALID, "amx_histogram_accumulate_dev: in_ld %d < dim %d or negative frame count %ld", in_ld, h->dim, T);
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(feats_dev, AMX_ERR_INVALID, "amx_histogram_accumulate_dev: NULL buffer");
    AMX_REQUIRE((unsigned long long)T <= 0xffffffffull - h->frames, AMX_ERR_INVALID,
                "amx_histogram_accumulate_dev: %ld more frames would take the handle past 2^32 - 1 frames (it holds %llu)", T, h->frames);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    const int  dim    = h->dim;
    const long fpg    = amx::frames_per_group(ctx, T, dim);
    const long groups = (T + fpg - 1) / fpg;
    AMX_REQUIRE(groups < (1l << 31), AMX_ERR_INVALID, "amx_histogram_accumulate_dev: %ld frames are more than one call takes", T);

    // 1. the range of this call's frames
    std::vector<int> range((size_t)2 * dim + 1, 0);
    std::fill(range.begin(), range.begin() + dim, INT_MAX);
    std::fill(range.begin() + dim, range.begin() + 2 * dim, INT_MIN);
    AMX_TRY(h->d_range.reserve(range.size()));
    AMX_HIP(hipMemcpyAsync(h->d_range.get(), range.data(), range.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    {
        amx::ScopedKernelTimer timer(ctx, "hist_range");
        hipLaunchKernelGGL(amx::hist_range_kernel, dim3((unsigned)groups), dim3(amx::kHistThreads), (size_t)2 * dim * sizeof(int), ctx->stream, feats_dev, in_ld, T,
                           dim, h->bucket_size, fpg, h->d_range.get());
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipMemcpyAsync(range.data(), h->d_range.get(), range.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    AMX_REQUIRE(range[2 * dim] == 0, AMX_ERR_INVALID,
                "amx_histogram_accumulate_dev: a frame holds a value that is not finite or lies 2^30 buckets or more from zero; nothing was added");

    // 2. the windows: what the handle holds, widened by this call
    const bool           have = h->dev_valid;
    std::vector<int32_t> kmin((size_t)dim), size((size_t)dim);
    bool                 grew = !have;
    for (int d = 0; d < dim; ++d) {
        long long lo = range[d], hi = range[dim + d];
        long long old_lo = 0, old_n = 0;
        if (have) {
            old_lo = h->d_kmin[d];
            old_n  = h->d_size[d];
        }
        else if (!h->counts[d].c.empty()) {
            old_lo = -(long long)h->counts[d].offset;
            old_n  = (long long)h->counts[d].c.size();
        }
        if (old_n) {
            lo = std::min(lo, old_lo);
            hi = std::max(hi, old_lo + old_n - 1);
        }
        kmin[d] = (int32_t)lo;
        size[d] = (int32_t)(hi - lo + 1);  // < 2^31: |lo|, |hi| < 2^30
        grew    = grew || lo != old_lo || size[d] != old_n;
    }
    if (grew)
        AMX_TRY(amx::hist_lay_out(h, kmin, size, !have));
    h->dev_valid = true;

    // 3. where each dimension counts
    std::vector<amx::HistDimMeta> meta((size_t)dim);
    int                           lds_words = 0;
    for (int d = 0; d < dim; ++d) {
        meta[d].off     = h->d_off[d];
        meta[d].kmin    = kmin[d];
        meta[d].size    = size[d];
        meta[d].lds_off = -1;
        meta[d].pad     = 0;
        if (size[d] <= amx::kHistLdsBuckets && lds_words + size[d] <= amx::kHistLdsCapacity) {
            meta[d].lds_off = lds_words;
            lds_words += size[d];
            ++h->n_lds;
        }
        else
            ++h->n_global;
    }
    AMX_TRY(h->d_meta.reserve(meta.size()));
    AMX_HIP(hipMemcpyAsync(h->d_meta.get(), meta.data(), meta.size() * sizeof(amx::HistDimMeta), hipMemcpyHostToDevice, ctx->stream));
    {
        amx::ScopedKernelTimer timer(ctx, "hist_count");
        hipLaunchKernelGGL(amx::hist_count_kernel, dim3((unsigned)groups), dim3(amx::kHistThreads), (size_t)lds_words * sizeof(uint32_t), ctx->stream, feats_dev,
                           in_ld, T, dim, h->bucket_size, fpg, h->d_meta.get(), lds_words, h->d_counts->get());
        AMX_HIP(hipGetLastError());
    }
    // `meta` and `range` are pageable: the asynchronous copies above have taken them before they returned
    h->host_valid = false;
    h->frames += (unsigned long long)T;
    ++h->n_calls;
    return AMX_OK;
}

int amx_histnorm_apply_dev(amx_histnorm* h, int n_seg, const long* frame_offsets, const int* key_of_segment, const float* in_dev, int in_ld, float* out_dev,
                           int out_ld, unsigned long long* clamped) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_histnorm_apply_dev: NULL handle");
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "amx_histnorm_apply_dev: the handle was created without a context");
    AMX_REQUIRE(!h->inverse.empty(), AMX_ERR_STATE, "amx_histnorm_apply_dev: several training histograms need amx_histnorm_set_scales first");
    AMX_REQUIRE(n_seg >= 0 && in_ld >= h->dim && out_ld >= h->dim, AMX_ERR_INVALID, "amx_histnorm_apply_dev: n_seg %d, in_ld %d, out_ld %d with dim %d", n_seg,
                in_ld, out_ld, h->dim);
    if (clamped)
        clamped[0] = clamped[1] = 0;
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(frame_offsets && key_of_segment, AMX_ERR_INVALID, "amx_histnorm_apply_dev: NULL segment list");
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "amx_histnorm_apply_dev: negative frame offset");
    std::vector<long long> seg((size_t)2 * n_seg + 1);
    for (int s = 0; s < n_seg; ++s) {
        AMX_REQUIRE(frame_offsets[s] <= frame_offsets[s + 1], AMX_ERR_INVALID, "amx_histnorm_apply_dev: frame offsets decrease at segment %d", s);
        AMX_REQUIRE(key_of_segment[s] >= 0 && key_of_segment[s] < (int)h->keys.size(), AMX_ERR_INVALID,
                    "amx_histnorm_apply_dev: No test-histogram found for key %d of segment %d (%zu keys were added).", key_of_segment[s], s, h->keys.size());
        seg[s]             = frame_offsets[s];
        seg[n_seg + 1 + s] = key_of_segment[s];
    }
    seg[n_seg]   = frame_offsets[n_seg];
    const long T = frame_offsets[n_seg] - frame_offsets[0];
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(in_dev && out_dev, AMX_ERR_INVALID, "amx_histnorm_apply_dev: NULL buffer");
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    const int dim = h->dim;
    if (h->meta_dirty) {
        // tables that are new since the last call, and the list of all of them
        AMX_HIP(hipStreamSynchronize(ctx->stream));  // a kernel still in flight may read what is replaced here
        std::vector<float>     flat;
        std::vector<long long> at((size_t)dim);
        for (int d = 0; d < dim; ++d) {
            at[d] = (long long)flat.size();
            flat.insert(flat.end(), h->inverse[d].f.begin(), h->inverse[d].f.end());
        }
        AMX_TRY(h->d_inverse.upload(flat.data(), flat.size()));
        std::vector<amx::TableMeta> meta((size_t)(1 + h->keys.size()) * dim);
        for (int d = 0; d < dim; ++d)
            meta[d] = amx::TableMeta{h->d_inverse.get() + at[d], h->inverse[d].bucket_size, h->inverse[d].offset, (int)h->inverse[d].f.size(), 0};
        for (size_t k = 0; k < h->keys.size(); ++k) {
            if (k >= h->d_keys.size()) {
                flat.clear();
                for (int d = 0; d < dim; ++d)
                    flat.insert(flat.end(), h->keys[k][d].f.begin(), h->keys[k][d].f.end());
                h->d_keys.emplace_back(new amx::DevBuf<float>);
                AMX_TRY(h->d_keys.back()->upload(flat.data(), flat.size()));
            }
            const float* p = h->d_keys[k]->get();
            for (int d = 0; d < dim; ++d) {
                const amx::LookupTable& t   = h->keys[k][d];
                meta[(1 + k) * dim + d] = amx::TableMeta{p, t.bucket_size, t.offset, (int)t.f.size(), 0};
                p += t.f.size();
            }
        }
        AMX_TRY(h->d_meta.upload(meta.data(), meta.size()));
        h->meta_dirty = false;
    }
    AMX_TRY(h->d_seg.reserve(seg.size()));
    AMX_HIP(hipMemcpyAsync(h->d_seg.get(), seg.data(), seg.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    AMX_TRY(h->d_clamped.reserve(2));
    AMX_HIP(hipMemsetAsync(h->d_clamped.get(), 0, 2 * sizeof(unsigned long long), ctx->stream));
    const long fpg    = amx::frames_per_group(ctx, T, dim);
    const long groups = (T + fpg - 1) / fpg;
    AMX_REQUIRE(groups < (1l << 31), AMX_ERR_INVALID, "amx_histnorm_apply_dev: %ld frames are more than one call takes", T);
    {
        amx::ScopedKernelTimer timer(ctx, "histnorm_apply");
        hipLaunchKernelGGL(amx::histnorm_apply_kernel, dim3((unsigned)groups), dim3(amx::kHistThreads), 0, ctx->stream, in_dev, in_ld, out_dev, out_ld, dim, n_seg,
                           h->d_seg.get(), h->d_meta.get(), fpg, h->d_clamped.get());
        AMX_HIP(hipGetLastError());
    }
    if (clamped) {
        AMX_HIP(hipMemcpyAsync(clamped, h->d_clamped.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return AMX_OK;
}

}  // extern "C"
