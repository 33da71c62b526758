// latword.hip -- word-level measures of a word lattice's arcs (include/amx.h, section "Lattice word measures"): the time-frame word
// posteriors 1 - p_t(w | x) summed or maximised over an arc's frames (Lattice/TimeframeError.cc:86-289), the frame-word accuracy
// (:294-395) and the approximate word accuracy (Lattice/Accuracy.cc:361-473), from the tables amx_latpost_run_dev takes and the -log
// posteriors it leaves on the device.
//
// The table is the work: one cell per (segment, label, frame), fed by every arc of that label that covers the frame, in the reference's
// discover order, through its LogCollector (Fsa/tRealSemiring.cc:168-194).  latword_host.cpp has sorted a segment's arcs stably by
// label, so a label's records are its feeds in order, and a (label, block of 64 frames) is one wave's unit with a lane per frame:
//   staging   64 records per trip go through the wave's own LDS slice as (start, end, weight): one coalesced load per lane, the weight
//             gathered from the posteriors by arc; a ballot of "touches this block" lets the wave step over the records that miss it,
//             and every lane then tests its own frame against a broadcast read.
//   lists     a label with kLwListArcs records and more (silence, noise) would make every one of its blocks stage all of them; there
//             latword_list_kernel first writes, per block, the indices of the records that touch it, by ballot and popcount prefix in
//             record order, and the unit stages from its list.  The host has only counted, so each list has its place.
//   passes    the collector's result needs the final minimum before its sum: pass 1 takes it per lane, pass 2 re-runs the running minimum
//             and the f32 sum in order.  ::exp and ::log1p are the f64 overloads in the reference's translation unit and `sum +=` adds
//             in f64 and narrows, so that is what a lane does.  No atomics but the refusal word, no order that depends on the batch.
//   marks     the frame-word accuracy runs the same units over the correct lattice with a mark per cell, and a wave per row turns the
//             marks into a prefix count: an arc's count is one subtraction.
// The arc kernels: a lane per arc chains (or maximises) over its frames in time order; an arc of kLwWaveFrames frames and more is taken
// by a wave that loads 64 cells at once and chains them by broadcast.  The approximate word accuracy is a lane per arc with two binary
// searches into its segment's sorted interval table (start ascending, running maximum of the ends) and the arithmetic of
// accuracy.hip's approximate mode.
#include <cfloat>
#include <chrono>
#include <cmath>

#include "common.hpp"
#include "latword_plan.hpp"

namespace amx {

constexpr int kLwWaves   = 4;
constexpr int kLwThreads = 64 * kLwWaves;
static_assert(kLwBlockFrames == 64, "a lane per frame");

struct LwArgs {
    const LwRec*  rec;
    const LwRow*  row;
    const LwUnit* unit;
    const int*    wide_unit;
    int           n_units, n_wide, n_rows;
    int*          list;
    const float*  arc_weight;
    float*        cell;     // scores; marks and their prefix counts are int32 in the same memory
    unsigned long long* bad;   // row << 32 | frame of the first cell the reference would refuse
    const int *   arc_start, *arc_end, *arc_row, *long_arc, *arc_seg, *arc_label, *seg_interval;
    const LwInterval* interval;
    int           n_arcs, n_long;
    float         normalization;
    float*        out;
};

__device__ __forceinline__ void lw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Per block of a wide row: the records that touch it, in record order.
__global__ __launch_bounds__(kLwThreads) void latword_list_kernel(LwArgs p) {
    const int wi = blockIdx.x * kLwWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wi >= p.n_wide)
        return;
    const LwUnit u = p.unit[p.wide_unit[wi]];
    const LwRow  r = p.row[u.row];
    int          n = 0;
    for (int i0 = 0; i0 < r.n_rec; i0 += 64) {
        const int i   = i0 + lane;
        bool      hit = false;
        if (i < r.n_rec) {
            const LwRec c = p.rec[r.rec0 + i];
            hit           = c.start < u.f0 + kLwBlockFrames && c.end > u.f0;
        }
        const unsigned long long m   = __ballot(hit);
        const int                pos = n + __popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < u.n_list)
            p.list[u.list0 + pos] = i;
        n += __popcll(m);
    }
}

// One wave per unit.  Every value that steers control flow outside the per-lane code is the same in all lanes: it comes from the unit,
// the row or a ballot.
template<bool MARK>
__global__ __launch_bounds__(kLwThreads) void latword_cell_kernel(LwArgs p) {
    __shared__ int   s_start[kLwWaves][64], s_end[kLwWaves][64];
    __shared__ float s_w[kLwWaves][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, ui = blockIdx.x * kLwWaves + w;
    if (ui >= p.n_units)
        return;
    const LwUnit u = p.unit[ui];
    const LwRow  r = p.row[u.row];
    const int    t = u.f0 + lane, n = u.n_list >= 0 ? u.n_list : r.n_rec;
    // a trip: 64 records into the slice; the ballot of those that touch the block
    auto stage = [&](int i0) {
        const int i   = i0 + lane;
        bool      hit = false;
        lw_wave_sync();   // the slice's readers of the trip before are done
        if (i < n) {
            const unsigned li = u.n_list >= 0 ? (unsigned)p.list[u.list0 + i] : (unsigned)i;
            const LwRec    c  = p.rec[r.rec0 + (li < (unsigned)r.n_rec ? (int)li : 0)];   // a list entry is a record of the row
            hit           = c.start < u.f0 + kLwBlockFrames && c.end > u.f0;
            s_start[w][lane] = c.start, s_end[w][lane] = c.end;
            if (!MARK)
                s_w[w][lane] = p.arc_weight[c.arc];
        }
        lw_wave_sync();
        return __ballot(hit);
    };
    float m_last = 0.f;
    int   fed    = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {   // pass 1: the final minimum, by the collector's own comparison
        unsigned long long hits = stage(i0);
        while (hits) {
            const int j = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            if (s_start[w][j] <= t && t < s_end[w][j]) {
                if (!MARK) {
                    const float a = s_w[w][j];
                    m_last        = fed == 0 || a < m_last ? a : m_last;
                }
                ++fed;
            }
        }
    }
    if (MARK) {
        int* mark = reinterpret_cast<int*>(p.cell) + r.cell0;
        if (t < r.hi)
            mark[1 + t - r.lo] = fed ? 1 : 0;
        if (t == r.lo)
            mark[0] = 0;
        return;
    }
    float m = 0.f, sum = 0.f;
    int   k = 0;
    if (__any(fed > 1))
        for (int i0 = 0; i0 < n; i0 += 64) {   // pass 2: the running minimum and the sum, in order
            unsigned long long hits = stage(i0);
            while (hits) {
                const int j = __ffsll((long long)hits) - 1;
                hits &= hits - 1;
                if (s_start[w][j] <= t && t < s_end[w][j]) {
                    const float a = s_w[w][j];
                    if (k == 0)
                        m = a;   // the constructor's initial weight
                    else {
                        float v = a;   // feed(): a tie is stored, not taken
                        if (a < m)
                            v = m, m = a;
                        const double term = exp((double)(m_last - v));
                        sum               = k == 1 ? (float)term : (float)((double)sum + term);
                    }
                    ++k;
                }
            }
        }
    if (t >= r.hi)
        return;
    float score = 0.f;
    if (fed) {
        const float pr = fed == 1 ? m_last : (float)((double)m_last - log1p((double)sum));
        if (!(pr > -0.001f))   // the reference's verify(p > tolerance_)
            atomicMin(p.bad, ((unsigned long long)(unsigned)u.row << 32) | (unsigned)t);
        score = (float)(1.0 - exp(-(double)pr));
    }
    p.cell[r.cell0 + t - r.lo] = score;
}

// One wave per row: marks -> the number of marked frames before each frame.
__global__ __launch_bounds__(kLwThreads) void latword_prefix_kernel(LwArgs p) {
    const int ri = blockIdx.x * kLwWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ri >= p.n_rows)
        return;
    const LwRow r    = p.row[ri];
    int*        mark = reinterpret_cast<int*>(p.cell) + r.cell0 + 1;
    const int   span = r.hi - r.lo;
    int         carry = 0;
    for (int i0 = 0; i0 < span; i0 += 64) {
        const int i = i0 + lane;
        int       s = i < span ? mark[i] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(s, o, 64);
            if (lane >= o)
                s += up;
        }
        s += carry;
        if (i < span)
            mark[i] = s;
        carry = __shfl(s, 63, 64);
    }
}

template<bool FMA>
__device__ __forceinline__ float lw_den(float normalization, int start, int end) {
    return mad<FMA>(normalization, (float)(unsigned)(end - start - 1), 1.f);   // the reference's u32 difference
}

// A lane per arc.  MODE: the configuration's mode but APPROXIMATE_WORD.
template<int MODE, bool FMA>
__global__ __launch_bounds__(256) void latword_arc_kernel(LwArgs p) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= p.n_arcs)
        return;
    const int row = p.arc_row[a], s = p.arc_start[a], e = p.arc_end[a];
    float     v   = 0.f;
    if (row != kLwArcUnreached) {
        if (MODE != AMX_LATWORD_FRAME_WORD_ACCURACY && e - s >= kLwWaveFrames)
            return;   // latword_arc_wave_kernel's
        if (MODE == AMX_LATWORD_FRAME_WORD_ACCURACY) {
            int count = 0;
            if (row >= 0) {
                const LwRow r   = p.row[row];
                const int*  pre = reinterpret_cast<const int*>(p.cell) + r.cell0;
                const int   b = s < r.lo ? r.lo : (s > r.hi ? r.hi : s), x = e < r.lo ? r.lo : (e > r.hi ? r.hi : e);
                count           = pre[x - r.lo] - pre[b - r.lo];
            }
            v = (float)count / lw_den<FMA>(p.normalization, s, e);
        }
        else {
            float acc = MODE == AMX_LATWORD_TIMEFRAME_ERROR_MAX ? -FLT_MAX : 0.f;
            if (row >= 0) {
                const LwRow  r = p.row[row];
                const float* c = p.cell + r.cell0;
                for (int t = s; t < e; ++t) {
                    const float x = c[t - r.lo];
                    acc           = MODE == AMX_LATWORD_TIMEFRAME_ERROR_MAX ? (acc < x ? x : acc) : acc + x;
                }
            }
            v = MODE == AMX_LATWORD_TIMEFRAME_ERROR_MAX ? acc : acc / lw_den<FMA>(p.normalization, s, e);
        }
    }
    p.out[a] = v;
}

// A wave per long arc: 64 cells per load, chained by broadcast in time order.
template<bool MAX, bool FMA>
__global__ __launch_bounds__(kLwThreads) void latword_arc_wave_kernel(LwArgs p) {
    const int li = blockIdx.x * kLwWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (li >= p.n_long)
        return;
    const int    a = p.long_arc[li], s = p.arc_start[a], e = p.arc_end[a];
    const LwRow  r = p.row[p.arc_row[a]];
    const float* c = p.cell + r.cell0;
    float        acc = MAX ? -FLT_MAX : 0.f;
    for (int t0 = s; t0 < e; t0 += 64) {
        const float x = t0 + lane < e ? c[t0 + lane - r.lo] : 0.f;
        const int   n = e - t0 < 64 ? e - t0 : 64;
        for (int j = 0; j < n; ++j) {
            const float xj = __shfl(x, j, 64);
            acc            = MAX ? (acc < xj ? xj : acc) : acc + xj;
        }
    }
    if (lane == 0)
        p.out[a] = MAX ? acc : acc / lw_den<FMA>(p.normalization, s, e);
}

// Approximate word accuracy: a lane per arc; the window of intervals that can overlap [hs, he) lies between two binary searches.
__global__ __launch_bounds__(256) void latword_approx_kernel(LwArgs p) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= p.n_arcs)
        return;
    float v = 0.f;
    if (p.arc_row[a] != kLwArcUnreached) {
        const int         g = p.arc_seg[a], n = p.seg_interval[g + 1] - p.seg_interval[g], hs = p.arc_start[a], he = p.arc_end[a], tk = p.arc_label[a];
        const LwInterval* I = p.interval + p.seg_interval[g];
        int               lo = 0, hi = n, b = 0, x = n;
        while (lo < hi) {   // first interval whose running maximum of the ends is above hs
            const int m = (lo + hi) >> 1;
            if (I[m].maxend > hs)
                hi = m;
            else
                lo = m + 1;
        }
        while (b < x) {   // first interval that starts at he or later
            const int m = (b + x) >> 1;
            if (I[m].start >= he)
                x = m;
            else
                b = m + 1;
        }
        float best = -FLT_MAX;
        bool  any  = false;
        for (int i = lo; i < b; ++i) {
            const LwInterval r = I[i];
            if (r.end > hs) {
                const float o   = (float)((he < r.end ? he : r.end) - (hs > r.start ? hs : r.start)) / (float)(r.end - r.start);
                const float acc = -1.f + (r.label == tk ? 2.f : 1.f) * o;
                best = acc > best ? acc : best, any = true;
            }
        }
        v = any ? best : 0.f;
    }
    p.out[a] = v;
}

template<class T>
static int lw_upload(amx_ctx* ctx, DevBuf<T>& d, const std::vector<T>& v) {
    AMX_TRY(d.reserve(v.size() ? v.size() : 1));
    if (!v.empty())
        AMX_HIP(hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return AMX_OK;
}

}  // namespace amx

struct amx_latword {
    amx_ctx*        ctx = nullptr;
    amx_latword_cfg cfg{};
    amx::DevBuf<amx::LwRec>      d_rec;
    amx::DevBuf<amx::LwRow>      d_row;
    amx::DevBuf<amx::LwUnit>     d_unit;
    amx::DevBuf<amx::LwInterval> d_interval;
    amx::DevBuf<int>             d_wide, d_list, d_arc_start, d_arc_end, d_arc_row, d_long, d_arc_seg, d_arc_label, d_seg_interval;
    amx::DevBuf<float>           d_cell;
    amx::DevBuf<unsigned long long> d_bad;
    // of the last call that ended
    std::vector<amx::LwRow> last_row;
    std::vector<int>        last_seg_row;
    bool                    last_scores = false;
    double                  last_plan_ms = 0, last_upload_ms = 0;
};

extern "C" {

int amx_latword_create(amx_ctx* ctx, const amx_latword_cfg* cfg, amx_latword** out) {
    const char* who = "amx_latword_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    amx_latword_cfg c;
    amx_latword_cfg_default(&c);
    if (cfg)
        c = *cfg;
    AMX_REQUIRE(c.mode >= AMX_LATWORD_TIMEFRAME_ERROR_SUM && c.mode <= AMX_LATWORD_APPROXIMATE_WORD, AMX_ERR_INVALID,
                "%s: mode %d is none (the exact accuracies, the smoothed accuracy and the mask, soft and weighted variants are not built)", who, c.mode);
    AMX_REQUIRE(std::isfinite(c.normalization), AMX_ERR_INVALID, "%s: normalization %g is not finite", who, (double)c.normalization);
    std::unique_ptr<amx_latword> h(new amx_latword);
    h->ctx = ctx, h->cfg = c;
    *out = h.release();
    return AMX_OK;
}

void amx_latword_destroy(amx_latword* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_latword_run_dev(amx_latword* h, const amx_latword_lattices* lat, const amx_latword_lattices* correct, const int32_t* short_pause_label,
                        int n_short_pause, const float* arc_weight_dev, float* arc_value_dev, amx_latword_info* info) {
    const char* who = "amx_latword_run_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    const int  mode      = h->cfg.mode;
    const bool timeframe = mode == AMX_LATWORD_TIMEFRAME_ERROR_SUM || mode == AMX_LATWORD_TIMEFRAME_ERROR_MAX;
    amx::LwPlan p;
    const auto  t0 = std::chrono::steady_clock::now();
    AMX_TRY(amx::latword_plan(h->cfg, lat, correct, short_pause_label, n_short_pause, who, &p));
    const auto t1 = std::chrono::steady_clock::now();
    if (info)
        for (int g = 0; g < p.n_seg; ++g)
            info[g] = p.info[(size_t)g];
    if (p.n_arcs == 0)
        return AMX_OK;
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(arc_value_dev && (!timeframe || arc_weight_dev), AMX_ERR_INVALID, "%s: NULL arc_value_dev, or a time-frame mode without arc_weight_dev", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    h->last_row.clear(), h->last_seg_row.clear();
    const amx::LwTable& tb = timeframe ? p.hyp : p.ref;
    std::vector<int32_t> labels;
    if (mode == AMX_LATWORD_APPROXIMATE_WORD)
        labels.assign(lat->arc_label, lat->arc_label + p.n_arcs);
    AMX_TRY(amx::lw_upload(ctx, h->d_rec, tb.rec));
    AMX_TRY(amx::lw_upload(ctx, h->d_row, tb.row));
    AMX_TRY(amx::lw_upload(ctx, h->d_unit, tb.unit));
    AMX_TRY(amx::lw_upload(ctx, h->d_wide, tb.wide_unit));
    AMX_TRY(amx::lw_upload(ctx, h->d_arc_start, p.arc_start));
    AMX_TRY(amx::lw_upload(ctx, h->d_arc_end, p.arc_end));
    AMX_TRY(amx::lw_upload(ctx, h->d_arc_row, p.arc_row));
    AMX_TRY(amx::lw_upload(ctx, h->d_long, p.long_arc));
    AMX_TRY(amx::lw_upload(ctx, h->d_arc_seg, p.arc_seg));
    AMX_TRY(amx::lw_upload(ctx, h->d_arc_label, labels));
    AMX_TRY(amx::lw_upload(ctx, h->d_seg_interval, p.seg_interval));
    AMX_TRY(amx::lw_upload(ctx, h->d_interval, p.interval));
    AMX_TRY(h->d_list.reserve((size_t)std::max(tb.n_list, 1ll)));
    AMX_TRY(h->d_cell.reserve((size_t)std::max(tb.n_cells, 1ll)));
    AMX_TRY(h->d_bad.reserve(1));
    AMX_HIP(hipMemsetAsync(h->d_bad.get(), 0xff, sizeof(unsigned long long), ctx->stream));
    h->last_plan_ms   = std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->last_upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();

    amx::LwArgs a{};
    a.rec = h->d_rec.get(), a.row = h->d_row.get(), a.unit = h->d_unit.get(), a.wide_unit = h->d_wide.get();
    a.n_units = (int)tb.unit.size(), a.n_wide = (int)tb.wide_unit.size(), a.n_rows = (int)tb.row.size();
    a.list = h->d_list.get(), a.arc_weight = arc_weight_dev, a.cell = h->d_cell.get(), a.bad = h->d_bad.get();
    a.arc_start = h->d_arc_start.get(), a.arc_end = h->d_arc_end.get(), a.arc_row = h->d_arc_row.get(), a.long_arc = h->d_long.get();
    a.arc_seg = h->d_arc_seg.get(), a.arc_label = h->d_arc_label.get(), a.seg_interval = h->d_seg_interval.get(), a.interval = h->d_interval.get();
    a.n_arcs = (int)p.n_arcs, a.n_long = (int)p.long_arc.size(), a.normalization = h->cfg.normalization, a.out = arc_value_dev;
    const dim3 threads(amx::kLwThreads), arcs((unsigned)amx::ceil_div(p.n_arcs, 256));
    const bool fma = ctx->contract == AMX_CONTRACT_FMA;
    if (mode != AMX_LATWORD_APPROXIMATE_WORD) {
        if (a.n_wide) {
            amx::ScopedKernelTimer timer(ctx, "latword_list");
            hipLaunchKernelGGL(amx::latword_list_kernel, dim3((unsigned)amx::ceil_div(a.n_wide, amx::kLwWaves)), threads, 0, ctx->stream, a);
            AMX_HIP(hipGetLastError());
        }
        if (a.n_units) {
            amx::ScopedKernelTimer timer(ctx, "latword_cells");
            const dim3 grid((unsigned)amx::ceil_div(a.n_units, amx::kLwWaves));
            if (timeframe)
                hipLaunchKernelGGL(amx::latword_cell_kernel<false>, grid, threads, 0, ctx->stream, a);
            else
                hipLaunchKernelGGL(amx::latword_cell_kernel<true>, grid, threads, 0, ctx->stream, a);
            AMX_HIP(hipGetLastError());
        }
    }
    if (timeframe) {
        unsigned long long bad = 0;
        AMX_HIP(hipMemcpyAsync(&bad, a.bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipStreamSynchronize(ctx->stream));
        if (bad != ~0ull) {
            const amx::LwRow& r = tb.row[(size_t)(bad >> 32)];
            amx::set_error("%s: segment %d, frame %d, label %d: the collected -log posterior is not above -0.001 (the reference's verify)", who, r.seg,
                           (int)(unsigned)bad, r.label);
            return AMX_ERR_INVALID;
        }
        {
            amx::ScopedKernelTimer timer(ctx, "latword_arcs");
            if (mode == AMX_LATWORD_TIMEFRAME_ERROR_MAX)
                hipLaunchKernelGGL((amx::latword_arc_kernel<AMX_LATWORD_TIMEFRAME_ERROR_MAX, false>), arcs, dim3(256), 0, ctx->stream, a);
            else if (fma)
                hipLaunchKernelGGL((amx::latword_arc_kernel<AMX_LATWORD_TIMEFRAME_ERROR_SUM, true>), arcs, dim3(256), 0, ctx->stream, a);
            else
                hipLaunchKernelGGL((amx::latword_arc_kernel<AMX_LATWORD_TIMEFRAME_ERROR_SUM, false>), arcs, dim3(256), 0, ctx->stream, a);
            AMX_HIP(hipGetLastError());
        }
        if (a.n_long) {
            amx::ScopedKernelTimer timer(ctx, "latword_arcs_wave");
            const dim3 grid((unsigned)amx::ceil_div(a.n_long, amx::kLwWaves));
            if (mode == AMX_LATWORD_TIMEFRAME_ERROR_MAX)
                hipLaunchKernelGGL((amx::latword_arc_wave_kernel<true, false>), grid, threads, 0, ctx->stream, a);
            else if (fma)
                hipLaunchKernelGGL((amx::latword_arc_wave_kernel<false, true>), grid, threads, 0, ctx->stream, a);
            else
                hipLaunchKernelGGL((amx::latword_arc_wave_kernel<false, false>), grid, threads, 0, ctx->stream, a);
            AMX_HIP(hipGetLastError());
        }
    }
    else if (mode == AMX_LATWORD_FRAME_WORD_ACCURACY) {
        if (a.n_rows) {
            amx::ScopedKernelTimer timer(ctx, "latword_prefix");
            hipLaunchKernelGGL(amx::latword_prefix_kernel, dim3((unsigned)amx::ceil_div(a.n_rows, amx::kLwWaves)), threads, 0, ctx->stream, a);
            AMX_HIP(hipGetLastError());
        }
        amx::ScopedKernelTimer timer(ctx, "latword_arcs");
        if (fma)
            hipLaunchKernelGGL((amx::latword_arc_kernel<AMX_LATWORD_FRAME_WORD_ACCURACY, true>), arcs, dim3(256), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL((amx::latword_arc_kernel<AMX_LATWORD_FRAME_WORD_ACCURACY, false>), arcs, dim3(256), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    else {
        amx::ScopedKernelTimer timer(ctx, "latword_approximate");
        hipLaunchKernelGGL(amx::latword_approx_kernel, arcs, dim3(256), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(ctx->stream));   // the uploads' host copies go away
    h->last_row = tb.row, h->last_seg_row = tb.seg_row, h->last_scores = timeframe;
    return AMX_OK;
}

int amx_latword_last_row(const amx_latword* h, int segment, int32_t label, int* lo, int* hi, int capacity, float* score) {
    const char* who = "amx_latword_last_row";
    AMX_REQUIRE(h && lo && hi, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(h->ctx && h->last_scores, AMX_ERR_STATE, "%s: no time-frame call has ended on this handle", who);
    AMX_REQUIRE(segment >= 0 && segment + 1 < (int)h->last_seg_row.size(), AMX_ERR_INVALID, "%s: segment %d outside the last call's", who, segment);
    *lo = *hi = 0;
    for (int i = h->last_seg_row[(size_t)segment]; i < h->last_seg_row[(size_t)segment + 1]; ++i) {
        const amx::LwRow& r = h->last_row[(size_t)i];
        if (r.label != label)
            continue;
        *lo = r.lo, *hi = r.hi;
        if (score) {
            AMX_REQUIRE(capacity >= r.hi - r.lo, AMX_ERR_INVALID, "%s: the row has %d frames, the buffer holds %d", who, r.hi - r.lo, capacity);
            AMX_HIP(hipSetDevice(h->ctx->device));
            AMX_HIP(hipMemcpy(score, h->d_cell.get() + r.cell0, (size_t)(r.hi - r.lo) * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return AMX_OK;
}

int amx_latword_last_timing(const amx_latword* h, double* plan_ms, double* upload_ms) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_latword_last_timing: NULL handle");
    if (plan_ms)
        *plan_ms = h->last_plan_ms;
    if (upload_ms)
        *upload_ms = h->last_upload_ms;
    return AMX_OK;
}

}  // extern "C"
