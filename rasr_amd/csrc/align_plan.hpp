// align_plan.hpp -- what the alignment entry points share (align.hip: Viterbi, align_bw.hip: Baum-Welch): the limits, the pass loop of
// Aligner::feed, the host's plan of a batch (checks, distinct emissions, arcs by target), the kernel that gathers the compact score
// matrix and the configuration checks of the search parameters.
#pragma once
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "common.hpp"

namespace amx {

constexpr int    kAlignThreads   = 256;
constexpr int    kAlignWaves     = kAlignThreads / 64;
constexpr int    kAlignMaxStates = AMX_ALIGN_MAX_STATES;
constexpr int    kAlignMaxCols   = AMX_ALIGN_MAX_EMISSIONS;
constexpr int    kAlignPerThread = kAlignMaxStates / kAlignThreads;   // ranks a lane scans
constexpr int    kAlignRowRegs   = kAlignMaxCols / kAlignThreads;     // words of the next frame's row a lane holds
constexpr size_t kAlignLdsBytes  = 128 * 1024;                        // of the CU's 160 KB
constexpr float  kAlignF32Max    = 3.402823466e+38f;                  // Core::Type<f32>::max
static_assert(kAlignMaxStates % kAlignThreads == 0 && kAlignMaxCols % kAlignThreads == 0, "whole words per lane");
static_assert(AMX_ALIGN_MAX_OUT_ARCS == 64, "one 64-bit mask per source");

// Core::isAlmostEqual(f32, f32) with tolerance 1 (Core/Utility.hh:316-321)
__host__ __device__ inline bool align_almost_equal(float a, float b) {
    const float d = fabsf(a - b);
    const float e = (fabsf(a) + fabsf(b) + 1.17549435e-38f) * 1.19209290e-07f * 1.f;
    return d < e;
}

struct AlignLoop {
    float  lo, hi, factor;
    double min_avg;
    int    incr;
};

// whether the pass at threshold t with this outcome ends Aligner::feed's loop (:617-625)
__host__ __device__ inline bool align_pass_ends(const AlignLoop& c, float t, bool reached, double avg, float score, float previous) {
    if (c.factor <= 1)
        return true;
    if (reached && avg >= c.min_avg) {
        if (!c.incr)
            return true;
        if (t > c.lo && align_almost_equal(score, previous))
            return true;
    }
    return false;
}

// The pass at threshold *t pruned nothing and did not end the loop: every later pass repeats its outcome.  Counts them as the loop would
// run them and leaves the threshold of the last one in *t.  A repeated outcome ends the loop at the next pass or never.
__host__ __device__ inline void align_count_repeats(const AlignLoop& c, float* t, bool reached, double avg, float score, int* n_iterations,
                                                    unsigned long long* counted) {
    float next = *t * c.factor;
    if (!(next <= c.hi))
        return;
    const bool once = align_pass_ends(c, next, reached, avg, score, score);   // next > lo: a factor above 1 moves a positive threshold
    do {
        ++*n_iterations;
        ++*counted;
        *t   = next;
        next = next * c.factor;
    } while (!once && next <= c.hi);
}

// steps of for (t = lo; t <= hi; t *= factor), at most `cap` + 1
inline int align_steps(float lo, float hi, float factor, int cap) {
    int n = 0;
    for (float t = lo; t <= hi && n <= cap; t *= factor) {
        ++n;
        if (factor <= 1)
            break;
    }
    return n;
}

// the checks of the search parameters that amx_align_create and amx_bw_create share
inline int align_check_search_cfg(const char* who, float lo, float hi, float factor, double min_average, int n_best_pruning, float score_scale) {
    AMX_REQUIRE(n_best_pruning >= INT_MAX, AMX_ERR_UNSUPPORTED,
                "%s: n_best_pruning %d: the reference's n-best selection is not defined on ties; only INT_MAX (off) is built", who, n_best_pruning);
    AMX_REQUIRE(!std::isnan(lo) && !std::isnan(hi) && !std::isnan(factor) && !std::isnan(score_scale) && !std::isnan(min_average),
                AMX_ERR_INVALID, "%s: min_acoustic_pruning, max_acoustic_pruning, increment_factor, min_average_number_of_states or score_scale is not a number", who);
    AMX_REQUIRE(lo > 0.f, AMX_ERR_INVALID, "%s: min_acoustic_pruning %g must be positive", who, (double)lo);
    // the constructor's check (:543-550)
    AMX_REQUIRE(!(lo > hi) && !(factor <= 1.f && lo != hi), AMX_ERR_INVALID,
                "%s: Inconsistent acoustic pruning settings: min_acoustic_pruning=%g max_acoustic_pruning=%g increment_factor=%g", who, (double)lo,
                (double)hi, (double)factor);
    AMX_REQUIRE(amx::align_steps(lo, hi, factor, AMX_ALIGN_MAX_PASSES) <= AMX_ALIGN_MAX_PASSES, AMX_ERR_UNSUPPORTED,
                "%s: increment_factor %g takes more than the limit of %d passes from min_acoustic_pruning %g to max_acoustic_pruning %g",
                who, (double)factor, AMX_ALIGN_MAX_PASSES, (double)lo, (double)hi);
    return AMX_OK;
}

struct AlignSeg {
    long long frame0;    // first row of scores_dev
    long long cm0;       // first word of the compact matrix
    long long bp0;       // first word of the back-pointers
    int       frames, n_states, state0, initial;
    int       n_cols, col0;    // distinct emissions and where their list starts
    int       in0, n_in;       // incoming arcs (by target)
};

// an arc in by-target order: x = source | ordinal in the source << 16, y = column of the compact matrix, z = weight bits,
// w = the arc's number in source order (global)
typedef int4 AlignArc;

// the host's plan of a call
struct AlignPlan {
    std::vector<AlignSeg>      seg;
    std::vector<long long>     off;         // [n_seg + 1] rows
    std::vector<int>           cols;        // distinct emission indices per segment
    std::vector<int>           in_off;      // [states + 1]
    std::vector<AlignArc>      in_arc;
    std::vector<unsigned char> is_final;
    std::vector<float>         final_w;
    std::vector<int>           arc_src, arc_label, arc_emission, arc_col;   // by source-order arc number
    std::vector<float>         arc_w;
    long long                  cm_words = 0, bp_words = 0, frames = 0;
    int                        max_states = 0, max_cols = 0, max_in = 0;
};

// Checks a batch and lays it out for the kernels.  Touches no device.
inline int align_plan(int n_seg, const long* frame_offsets, const amx_align_graphs* g, int n_columns, const char* who, AlignPlan* p) {
    AMX_REQUIRE(frame_offsets && g, AMX_ERR_INVALID, "%s: NULL segment list or graphs", who);
    AMX_REQUIRE(g->state_offsets && g->initial_state && g->is_final && g->final_weight && g->arc_offsets, AMX_ERR_INVALID, "%s: NULL graph table", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: negative frame offset", who);
    AMX_REQUIRE(g->state_offsets[0] == 0 && g->arc_offsets[0] == 0, AMX_ERR_INVALID, "%s: state_offsets and arc_offsets start at 0", who);
    p->off.resize((size_t)n_seg + 1);
    for (int s = 0; s <= n_seg; ++s) {
        AMX_REQUIRE(s == 0 || frame_offsets[s - 1] <= frame_offsets[s], AMX_ERR_INVALID, "%s: frame offsets decrease at segment %d", who, s - 1);
        AMX_REQUIRE(s == 0 || g->state_offsets[s - 1] < g->state_offsets[s], AMX_ERR_INVALID, "%s: segment %d has no state", who, s - 1);
        p->off[s] = frame_offsets[s];
    }
    p->frames         = p->off[n_seg] - p->off[0];
    const int n_states = g->state_offsets[n_seg];
    for (int i = 0; i < n_states; ++i)
        AMX_REQUIRE(g->arc_offsets[i] <= g->arc_offsets[i + 1], AMX_ERR_INVALID, "%s: arc offsets decrease at state %d", who, i);
    const int n_arcs = g->arc_offsets[n_states];
    AMX_REQUIRE(n_arcs == 0 || (g->arc_target && g->arc_emission && g->arc_label && g->arc_weight), AMX_ERR_INVALID, "%s: NULL arc table", who);
    p->seg.resize(n_seg);
    p->in_off.assign((size_t)n_states + 1, 0);
    p->in_arc.resize(n_arcs);
    p->is_final.assign(g->is_final, g->is_final + n_states);
    p->final_w.assign(g->final_weight, g->final_weight + n_states);
    p->arc_src.resize(n_arcs), p->arc_label.assign(g->arc_label, g->arc_label + n_arcs), p->arc_emission.assign(g->arc_emission, g->arc_emission + n_arcs);
    p->arc_col.resize(n_arcs), p->arc_w.assign(g->arc_weight, g->arc_weight + n_arcs);
    std::vector<int> fill;
    for (int s = 0; s < n_seg; ++s) {
        const int s0 = g->state_offsets[s], S = g->state_offsets[s + 1] - s0;
        const int a0 = g->arc_offsets[s0], a1 = g->arc_offsets[s0 + S];
        AMX_REQUIRE(S <= kAlignMaxStates, AMX_ERR_UNSUPPORTED, "%s: segment %d has %d states, more than the limit of %d states per segment", who, s, S,
                    kAlignMaxStates);
        AMX_REQUIRE(g->initial_state[s] >= 0 && g->initial_state[s] < S, AMX_ERR_INVALID, "%s: segment %d: initial_state %d outside its %d states", who, s,
                    g->initial_state[s], S);
        for (int i = s0; i < s0 + S; ++i) {
            AMX_REQUIRE(!g->is_final[i] || !std::isnan(g->final_weight[i]), AMX_ERR_INVALID, "%s: segment %d: final_weight of state %d is not a number", who, s,
                        i - s0);
            AMX_REQUIRE(g->arc_offsets[i + 1] - g->arc_offsets[i] <= AMX_ALIGN_MAX_OUT_ARCS, AMX_ERR_UNSUPPORTED,
                        "%s: segment %d: state %d has %d arcs, more than the limit of %d arcs out of a state", who, s, i - s0, g->arc_offsets[i + 1] - g->arc_offsets[i],
                        AMX_ALIGN_MAX_OUT_ARCS);
        }
        // the distinct emissions, in increasing order
        std::vector<int> used;
        for (int a = a0; a < a1; ++a) {
            AMX_REQUIRE(g->arc_target[a] >= 0 && g->arc_target[a] < S, AMX_ERR_INVALID, "%s: segment %d: arc_target[%d] = %d outside its %d states", who, s, a,
                        g->arc_target[a], S);
            AMX_REQUIRE(g->arc_emission[a] >= 0 && g->arc_emission[a] < n_columns, AMX_ERR_INVALID,
                        "%s: segment %d: arc_emission[%d] = %d outside the %d columns", who, s, a, g->arc_emission[a], n_columns);
            AMX_REQUIRE(!std::isnan(g->arc_weight[a]), AMX_ERR_INVALID, "%s: segment %d: arc_weight[%d] is not a number", who, s, a);
            used.push_back(g->arc_emission[a]);
        }
        std::sort(used.begin(), used.end());
        used.erase(std::unique(used.begin(), used.end()), used.end());
        AMX_REQUIRE((int)used.size() <= kAlignMaxCols, AMX_ERR_UNSUPPORTED, "%s: segment %d uses %zu emission indices, more than the limit of %d per segment",
                    who, s, used.size(), kAlignMaxCols);
        AlignSeg& sg = p->seg[s];
        sg.frame0 = p->off[s], sg.frames = (int)(p->off[s + 1] - p->off[s]);
        AMX_REQUIRE(p->off[s + 1] - p->off[s] <= INT_MAX / std::max(S, std::max((int)used.size(), 1)), AMX_ERR_UNSUPPORTED,
                    "%s: segment %d has %lld frames, more than one call takes", who, s, p->off[s + 1] - p->off[s]);
        sg.n_states = S, sg.state0 = s0, sg.initial = g->initial_state[s];
        sg.n_cols = (int)used.size(), sg.col0 = (int)p->cols.size();
        sg.in0 = a0, sg.n_in = a1 - a0;
        sg.cm0 = p->cm_words, sg.bp0 = p->bp_words;
        p->cm_words += (long long)sg.frames * sg.n_cols;
        p->bp_words += (long long)sg.frames * S;
        p->cols.insert(p->cols.end(), used.begin(), used.end());
        p->max_states = std::max(p->max_states, S), p->max_cols = std::max(p->max_cols, sg.n_cols), p->max_in = std::max(p->max_in, sg.n_in);
        // transpose: count, offsets, fill; arcs of one target stay in (source, ordinal) order
        fill.assign(S, 0);
        for (int a = a0; a < a1; ++a)
            ++fill[g->arc_target[a]];
        p->in_off[s0] = a0;
        for (int i = 0; i < S; ++i) {
            p->in_off[(size_t)s0 + i + 1] = p->in_off[(size_t)s0 + i] + fill[i];
            fill[i]                       = p->in_off[(size_t)s0 + i];
        }
        for (int i = s0; i < s0 + S; ++i)
            for (int a = g->arc_offsets[i]; a < g->arc_offsets[i + 1]; ++a) {
                const int col = (int)(std::lower_bound(used.begin(), used.end(), g->arc_emission[a]) - used.begin());
                int       wbits;
                std::memcpy(&wbits, &g->arc_weight[a], sizeof wbits);
                p->arc_src[a] = i - s0, p->arc_col[a] = col;
                p->in_arc[fill[g->arc_target[a]]++] = make_int4((i - s0) | ((a - g->arc_offsets[i]) << 16), col, wbits, a);
            }
    }
    return AMX_OK;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v             = u < v ? u : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o, 64);
    return v;
}

// static: align.hip and align_bw.hip each launch their own copy
static __global__ __launch_bounds__(kAlignThreads) void align_gather_kernel(const float* __restrict__ scores, long long scores_ld, const long long* __restrict__ off,
                                                                     int n_seg, const AlignSeg* __restrict__ seg, const int* __restrict__ cols, float scale,
                                                                     float* __restrict__ cm) {
    const long long t = off[0] + blockIdx.x;
    int             b = 0, e = n_seg;   // off[b] <= t < off[e]
    while (e - b > 1) {
        const int m = (b + e) / 2;
        if (off[m] <= t)
            b = m;
        else
            e = m;
    }
    const AlignSeg sg  = seg[b];
    const float*   row = scores + t * scores_ld;
    float*         out = cm + sg.cm0 + (t - sg.frame0) * sg.n_cols;
    for (int j = threadIdx.x; j < sg.n_cols; j += kAlignThreads) {
        const float v = row[cols[sg.col0 + j]];
        out[j]        = scale == 1.f ? v : scale * v;   // ScaledContextScorer::score: one rounding
    }
}

template<class T>
static int align_upload(amx_ctx* ctx, DevBuf<T>& d, const std::vector<T>& v) {
    AMX_TRY(d.reserve(v.size() ? v.size() : 1));
    if (!v.empty())
        AMX_HIP(hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return AMX_OK;
}


}  // namespace amx
