// align.hip -- Search::Aligner in Viterbi mode on a [frames x emissions] score matrix that is already on the device (include/amx.h, section
// "Viterbi alignment"): what Speech::AlignmentNode runs, for a batch of segments.
//
// The recursion is sequential in time and parallel over states and segments.  align_gather_kernel copies the columns a segment's graph
// uses into a compact [frames x distinct emissions] matrix (score_scale applied there); align_search_kernel runs all pruning passes of
// one segment in one workgroup, the state scores and list positions in LDS; align_traceback_kernel follows the back-pointers of the
// last pass and writes label, emission index and arc score per frame.  Only f32 additions and comparisons happen.
//
// The reference's hypothesis LIST decides every tie (Aligner.cc:144-167, :408-419), so the dense kernel carries each active state's
// position in it as a rank.  A candidate of target s is keyed (rank of its source << 6 | ordinal of the arc in its source): candidates
// arrive in key order there.  s takes the minimal score, among ties the largest key; its position in the new list follows its SMALLEST
// key.  Those first keys are distinct (an arc has one target), so they are marked in one 64-bit mask per source rank, and the new rank
// is the number of marked keys below: an exclusive scan of the masks' popcounts plus the popcount of the mask below the arc.
#include "align_plan.hpp"

namespace amx {

struct AlignSummary {
    float              score;
    int                reached, n_iterations;
    float              last_threshold;
    double             average;
    unsigned long long sum;
    int                best_state, nan;
    unsigned long long passes_run, passes_counted;
};

struct AlignArgs {
    const AlignSeg*      seg;
    const int*           in_off;     // [states + 1] by target, global
    const AlignArc*      in_arc;
    const unsigned char* is_final;   // [states]
    const float*         final_w;    // [states]
    const float*         cm;
    int*                 bp;
    AlignSummary*        summary;
    AlignLoop            loop;
    int                  lds_states, lds_cols, lds_arcs;   // LDS capacities of this launch; lds_arcs 0: arcs are read from memory
};

// One workgroup per segment.  Every __syncthreads() below sits in control flow whose conditions are the same in all lanes: frame and
// state counts come from the segment table, the pass loop's decisions from values every lane reduced out of LDS alike.
__global__ __launch_bounds__(kAlignThreads) void align_search_kernel(AlignArgs p) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ float s_min[kAlignWaves];
    __shared__ int   s_cnt[kAlignWaves], s_scan[kAlignWaves], s_nan;
    __shared__ float s_bv[kAlignWaves];
    __shared__ int   s_br[kAlignWaves], s_bs[kAlignWaves];
    const int      tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AlignSeg sg  = p.seg[blockIdx.x];
    const int      S = sg.n_states, E = sg.n_cols, T = sg.frames;
    // LDS: arcs | masks | scores[2] | ranks[2] | bases | incoming offsets | rows[2]
    AlignArc*           l_arc  = (AlignArc*)lds_raw;
    unsigned long long* mask   = (unsigned long long*)(l_arc + p.lds_arcs);
    float*              score  = (float*)(mask + p.lds_states);
    int*                rank   = (int*)(score + 2 * p.lds_states);
    int*                base   = rank + 2 * p.lds_states;
    int*                in_off = base + p.lds_states;
    float*              row    = (float*)(in_off + p.lds_states + 1);
    const AlignArc*     arcs   = p.in_arc + sg.in0;   // generic: LDS when the launch has room for them
    if (p.lds_arcs) {
        for (int a = tid; a < sg.n_in; a += kAlignThreads)
            l_arc[a] = p.in_arc[sg.in0 + a];
        arcs = l_arc;
    }
    for (int s = tid; s <= S; s += kAlignThreads)
        in_off[s] = p.in_off[sg.state0 + s] - sg.in0;
    if (tid == 0)
        s_nan = 0;
    const float*    cm      = p.cm + sg.cm0;
    int*            bp      = p.bp + sg.bp0;
    const AlignLoop lp      = p.loop;
    float           t       = lp.lo, previous = kAlignF32Max, pass_score = kAlignF32Max;
    int             n_iter = 0, best_state = -1;
    unsigned long long sum = 0, passes_run = 0, passes_counted = 0;
    double          avg  = 0;
    bool            nan  = false;
    __syncthreads();
    while (t <= lp.hi) {
        ++n_iter, ++passes_run;
        // restart(): the startup hypothesis alone (:198-204)
        for (int s = tid; s < S; s += kAlignThreads) {
            rank[s]  = s == sg.initial ? 0 : -1;
            score[s] = 0.f;
            mask[s]  = 0;
        }
        if (T > 0)
            for (int j = tid; j < E; j += kAlignThreads)
                row[j] = cm[j];
        int  cur = 0, n_prev = 1;
        bool pruned = false;
        sum         = 0;
        __syncthreads();
        for (int f = 0; f < T; ++f) {
            const int    nxt   = cur ^ 1;
            const float* sc    = score + cur * p.lds_states;
            const int*   rk    = rank + cur * p.lds_states;
            float*       sn    = score + nxt * p.lds_states;
            int*         rn    = rank + nxt * p.lds_states;
            const float* rw    = row + (f & 1) * p.lds_cols;
            const bool   ahead = f + 1 < T;
            float        pre[kAlignRowRegs];   // the next frame's row, on its way while this one is worked on
#pragma unroll
            for (int k = 0; k < kAlignRowRegs; ++k) {
                const int j = k * kAlignThreads + tid;
                pre[k]      = ahead && j < E ? cm[(long long)(f + 1) * E + j] : 0.f;
            }
            // expansion and recombination, one target state at a time (:215-252, :144-167)
            bool met_nan = false;
            for (int s = tid; s < S; s += kAlignThreads) {
                int   first = INT_MAX, bkey = -1, barc = -1;
                float best  = 0.f;
                for (int a = in_off[s]; a < in_off[s + 1]; ++a) {
                    const AlignArc q   = arcs[a];
                    const int      src = q.x & 0xffff;
                    const int      r   = rk[src];
                    if (r < 0)
                        continue;
                    const int   key = (r << 6) | (q.x >> 16);
                    const float sco = (sc[src] + __int_as_float(q.z)) + rw[q.y];
                    met_nan         = met_nan || sco != sco;
                    first           = key < first ? key : first;
                    if (bkey < 0 || sco < best || (sco == best && key > bkey))
                        best = sco, bkey = key, barc = q.w;
                }
                if (bkey >= 0) {
                    atomicOr(&mask[first >> 6], 1ull << (first & 63));
                    sn[s]                     = best;
                    bp[(long long)f * S + s] = barc;
                }
                rn[s] = bkey >= 0 ? first : -1;
            }
            if (met_nan)
                s_nan = 1;
            __syncthreads();
            // exclusive scan of the masks' popcounts over the previous frame's ranks
            int cnt[kAlignPerThread], mine = 0;
#pragma unroll
            for (int k = 0; k < kAlignPerThread; ++k) {
                const int r = tid * kAlignPerThread + k;
                cnt[k]      = r < n_prev ? __popcll(mask[r]) : 0;
                mine += cnt[k];
            }
            int incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(incl, o, 64);
                incl += lane >= o ? u : 0;
            }
            if (lane == 63)
                s_scan[wave] = incl;
            __syncthreads();
            int before = incl - mine, n_new = 0;
#pragma unroll
            for (int w = 0; w < kAlignWaves; ++w) {
                before += w < wave ? s_scan[w] : 0;
                n_new += s_scan[w];
            }
#pragma unroll
            for (int k = 0; k < kAlignPerThread; ++k) {
                const int r = tid * kAlignPerThread + k;
                if (r < n_prev)
                    base[r] = before;
                before += cnt[k];
            }
            __syncthreads();
            // the new ranks, and minimumScore() (:254-261)
            float m = kAlignF32Max;
            for (int s = tid; s < S; s += kAlignThreads) {
                const int key = rn[s];
                if (key >= 0) {
                    rn[s] = base[key >> 6] + __popcll(mask[key >> 6] & ((1ull << (key & 63)) - 1ull));
                    m     = sn[s] < m ? sn[s] : m;
                }
            }
            m = wave_min(m);
            if (lane == 0)
                s_min[wave] = m;
            __syncthreads();
            m = kAlignF32Max;
#pragma unroll
            for (int w = 0; w < kAlignWaves; ++w)
                m = s_min[w] < m ? s_min[w] : m;
            const float limit = m + t;   // :597
            int         kept  = 0;
            for (int s = tid; s < S; s += kAlignThreads)
                if (rn[s] >= 0) {
                    if (sn[s] <= limit)   // :295
                        ++kept;
                    else
                        rn[s] = -1;
                }
            kept = wave_sum(kept);
            if (lane == 0)
                s_cnt[wave] = kept;
            for (int r = tid; r < n_prev; r += kAlignThreads)
                mask[r] = 0;
            if (ahead) {
                float* rnext = row + ((f + 1) & 1) * p.lds_cols;
#pragma unroll
                for (int k = 0; k < kAlignRowRegs; ++k) {
                    const int j = k * kAlignThreads + tid;
                    if (j < E)
                        rnext[j] = pre[k];
                }
            }
            __syncthreads();
            kept = 0;
#pragma unroll
            for (int w = 0; w < kAlignWaves; ++w)
                kept += s_cnt[w];
            sum += (unsigned)kept;   // nStateHypotheses_ += nStateHypothesesCurFrame() (:600)
            pruned = pruned || kept < n_new;
            n_prev = n_new;
            cur    = nxt;
        }
        nan = s_nan != 0;   // written before a barrier every lane has passed
        if (nan)
            break;
        // finalStatePotential (:385-405) and the best final hypothesis (:408-419): the smallest value, among equals the first in the list
        {
            const float* sc = score + cur * p.lds_states;
            const int*   rk = rank + cur * p.lds_states;
            float        bv = kAlignF32Max;
            int          br = INT_MAX, bs = -1;
            for (int s = tid; s < S; s += kAlignThreads)
                if (rk[s] >= 0 && p.is_final[sg.state0 + s]) {
                    const float v = p.final_w[sg.state0 + s] + sc[s];
                    if (v < kAlignF32Max && (bs < 0 || v < bv || (v == bv && rk[s] < br)))
                        bv = v, br = rk[s], bs = s;
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int   orr = __shfl_xor(br, o, 64), os = __shfl_xor(bs, o, 64);
                if (os >= 0 && (bs < 0 || ov < bv || (ov == bv && orr < br)))
                    bv = ov, br = orr, bs = os;
            }
            if (lane == 0)
                s_bv[wave] = bv, s_br[wave] = br, s_bs[wave] = bs;
            __syncthreads();
            bv = kAlignF32Max, br = INT_MAX, bs = -1;
#pragma unroll
            for (int w = 0; w < kAlignWaves; ++w)
                if (s_bs[w] >= 0 && (bs < 0 || s_bv[w] < bv || (s_bv[w] == bv && s_br[w] < br)))
                    bv = s_bv[w], br = s_br[w], bs = s_bs[w];
            pass_score = bs >= 0 ? bv : kAlignF32Max;
            best_state = bs;
        }
        avg                = (double)(unsigned)sum / (double)(unsigned)T;   // Core::Statistics<u32>::average: 0 / 0 for no frame
        const bool reached = pass_score != kAlignF32Max;
        __syncthreads();   // s_b* and the state buffers are free for the next pass
        if (align_pass_ends(lp, t, reached, avg, pass_score, previous))
            break;
        previous = pass_score;
        if (!pruned) {
            align_count_repeats(lp, &t, reached, avg, pass_score, &n_iter, &passes_counted);
            break;
        }
        const float next = t * lp.factor;
        if (!(next <= lp.hi))
            break;
        t = next;
    }
    if (tid == 0) {
        AlignSummary r;
        r.score          = nan ? kAlignF32Max : pass_score;
        r.reached        = !nan && pass_score != kAlignF32Max;
        r.n_iterations   = n_iter;
        r.last_threshold = t;
        r.average        = nan ? 0.0 : avg;
        r.sum            = nan ? 0 : sum;
        r.best_state     = r.reached ? best_state : -1;
        r.nan            = nan;
        r.passes_run = passes_run, r.passes_counted = passes_counted;
        p.summary[blockIdx.x] = r;
    }
}

struct AlignTraceArgs {
    const AlignSeg*     seg;
    const AlignSummary* summary;
    const int*          bp;
    const float*        cm;
    const int *         arc_src, *arc_label, *arc_emission, *arc_col;
    const float*        arc_w;
    int*                path;   // [frames of the call] the arcs of the best path
    long long           base;   // off[0]
    int32_t *           label, *emission;
    float*              arc_score;   // nullable
};

// One wave per segment: lane 0 follows the back-pointers from the best final state (:430-442); then the scores along the path are formed
// again in frame order, 64 frames' operands loaded at a time: score[hyp] = (score[trace] + weight) + emission is what the winner was given.
__global__ __launch_bounds__(64) void align_traceback_kernel(AlignTraceArgs p) {
    const AlignSeg     sg   = p.seg[blockIdx.x];
    const AlignSummary r    = p.summary[blockIdx.x];
    const int          lane = threadIdx.x, T = sg.frames, S = sg.n_states;
    if (!r.reached) {
        for (int f = lane; f < T; f += 64) {
            p.label[sg.frame0 + f] = -1, p.emission[sg.frame0 + f] = -1;
            if (p.arc_score)
                p.arc_score[sg.frame0 + f] = 0.f;
        }
        return;
    }
    int* path = p.path + (sg.frame0 - p.base);
    if (lane == 0) {
        int s = r.best_state;
        for (int f = T - 1; f >= 0; --f) {
            const int a = p.bp[sg.bp0 + (long long)f * S + s];
            __hip_atomic_store(path + f, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s = p.arc_src[a];
        }
    }
    __threadfence();
    __syncthreads();
    float prev = 0.f;
    for (int f0 = 0; f0 < T; f0 += 64) {
        const int  f  = f0 + lane;
        const bool in = f < T;
        const int  a  = in ? __hip_atomic_load(path + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const float w = in ? p.arc_w[a] : 0.f;
        const float e = in ? p.cm[sg.cm0 + (long long)f * sg.n_cols + p.arc_col[a]] : 0.f;
        float       mine = 0.f;
        const int   n    = T - f0 < 64 ? T - f0 : 64;
        for (int i = 0; i < n; ++i) {
            const float next = (prev + __shfl(w, i, 64)) + __shfl(e, i, 64);
            if (lane == i)
                mine = next - prev;   // :438
            prev = next;
        }
        if (in) {
            p.label[sg.frame0 + f] = p.arc_label[a], p.emission[sg.frame0 + f] = p.arc_emission[a];
            if (p.arc_score)
                p.arc_score[sg.frame0 + f] = mine;
        }
    }
}

}  // namespace amx

struct amx_align {
    amx_ctx*      ctx = nullptr;
    amx_align_cfg cfg{};
    amx::AlignPlan plan;   // of the last call: the uploads read it until the call's synchronisation
    amx::DevBuf<amx::AlignSeg>     d_seg;
    amx::DevBuf<long long>         d_off;
    amx::DevBuf<int>               d_cols, d_in_off, d_arc_src, d_arc_label, d_arc_emission, d_arc_col, d_bp, d_path;
    amx::DevBuf<amx::AlignArc>     d_in_arc;
    amx::DevBuf<unsigned char>     d_is_final;
    amx::DevBuf<float>             d_final_w, d_arc_w, d_cm;
    amx::DevBuf<amx::AlignSummary> d_summary;
    std::vector<amx::AlignSummary> summary;
    bool                           lds_raised = false;
};

extern "C" {

void amx_align_default_cfg(amx_align_cfg* cfg) {
    if (!cfg)
        return;
    cfg->min_acoustic_pruning               = 50.f;      // paramMinAcousticPruningThreshold (Aligner.cc:473-476)
    cfg->max_acoustic_pruning               = FLT_MAX;   // :478-481
    cfg->increment_factor                   = 2.f;       // :483-486
    cfg->min_average_number_of_states       = 0.0;       // :488-491
    cfg->increase_until_no_score_difference = 1;         // :493-496
    cfg->n_best_pruning                     = INT_MAX;   // :516-518
    cfg->mode                               = AMX_ALIGN_VITERBI;   // :508-509
    cfg->score_scale                        = 1.f;
}

int amx_align_create(amx_ctx* ctx, const amx_align_cfg* cfg, amx_align** out) {
    AMX_REQUIRE(out, AMX_ERR_INVALID, "amx_align_create: NULL argument");
    *out = nullptr;
    AMX_REQUIRE(cfg, AMX_ERR_INVALID, "amx_align_create: NULL argument");
    AMX_REQUIRE(cfg->mode == AMX_ALIGN_VITERBI || cfg->mode == AMX_ALIGN_BAUM_WELCH, AMX_ERR_INVALID, "amx_align_create: mode %d is none", cfg->mode);
    AMX_REQUIRE(cfg->mode == AMX_ALIGN_VITERBI, AMX_ERR_UNSUPPORTED,
                "amx_align_create: mode baum-welch is not built on this handle (amx_bw_create has it); mode viterbi is");
    AMX_TRY(amx::align_check_search_cfg("amx_align_create", cfg->min_acoustic_pruning, cfg->max_acoustic_pruning, cfg->increment_factor,
                                        cfg->min_average_number_of_states, cfg->n_best_pruning, cfg->score_scale));
    std::unique_ptr<amx_align> h(new amx_align);
    h->ctx = ctx;
    h->cfg = *cfg;
    *out   = h.release();
    return AMX_OK;
}

void amx_align_destroy(amx_align* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_align_viterbi_dev(amx_align* h, int n_seg, const long* frame_offsets, const amx_align_graphs* graphs, const float* scores_dev, int scores_ld,
                          int n_columns, int32_t* label_dev, int32_t* emission_dev, float* arc_score_dev, amx_align_result* result,
                          unsigned long long counters[3]) {
    const char* who = "amx_align_viterbi_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_seg >= 0 && n_columns >= 1 && scores_ld >= n_columns, AMX_ERR_INVALID, "%s: n_seg %d, scores_ld %d with %d columns", who, n_seg, scores_ld,
                n_columns);
    if (counters)
        counters[0] = counters[1] = counters[2] = 0;
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(result, AMX_ERR_INVALID, "%s: NULL result", who);
    amx::AlignPlan& p = h->plan;
    p                 = amx::AlignPlan();
    AMX_TRY(amx::align_plan(n_seg, frame_offsets, graphs, n_columns, who, &p));
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(p.frames == 0 || (scores_dev && label_dev && emission_dev), AMX_ERR_INVALID, "%s: NULL buffer", who);
    AMX_REQUIRE(p.frames < (1ll << 31), AMX_ERR_UNSUPPORTED, "%s: %lld frames are more than one call takes", who, p.frames);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_TRY(amx::align_upload(ctx, h->d_seg, p.seg));
    AMX_TRY(amx::align_upload(ctx, h->d_off, p.off));
    AMX_TRY(amx::align_upload(ctx, h->d_cols, p.cols));
    AMX_TRY(amx::align_upload(ctx, h->d_in_off, p.in_off));
    AMX_TRY(amx::align_upload(ctx, h->d_in_arc, p.in_arc));
    AMX_TRY(amx::align_upload(ctx, h->d_is_final, p.is_final));
    AMX_TRY(amx::align_upload(ctx, h->d_final_w, p.final_w));
    AMX_TRY(amx::align_upload(ctx, h->d_arc_src, p.arc_src));
    AMX_TRY(amx::align_upload(ctx, h->d_arc_label, p.arc_label));
    AMX_TRY(amx::align_upload(ctx, h->d_arc_emission, p.arc_emission));
    AMX_TRY(amx::align_upload(ctx, h->d_arc_col, p.arc_col));
    AMX_TRY(amx::align_upload(ctx, h->d_arc_w, p.arc_w));
    AMX_TRY(h->d_cm.reserve((size_t)std::max<long long>(p.cm_words, 1)));
    AMX_TRY(h->d_bp.reserve((size_t)std::max<long long>(p.bp_words, 1)));
    AMX_TRY(h->d_path.reserve((size_t)std::max<long long>(p.frames, 1)));
    AMX_TRY(h->d_summary.reserve(n_seg));
    if (p.frames) {
        amx::ScopedKernelTimer timer(ctx, "align_gather");
        hipLaunchKernelGGL(amx::align_gather_kernel, dim3((unsigned)p.frames), dim3(amx::kAlignThreads), 0, ctx->stream, scores_dev, (long long)scores_ld,
                           h->d_off.get(), n_seg, h->d_seg.get(), h->d_cols.get(), h->cfg.score_scale, h->d_cm.get());
        AMX_HIP(hipGetLastError());
    }
    {
        amx::AlignArgs a{};
        a.seg = h->d_seg.get(), a.in_off = h->d_in_off.get(), a.in_arc = h->d_in_arc.get(), a.is_final = h->d_is_final.get(), a.final_w = h->d_final_w.get();
        a.cm = h->d_cm.get(), a.bp = h->d_bp.get(), a.summary = h->d_summary.get();
        a.loop = amx::AlignLoop{h->cfg.min_acoustic_pruning, h->cfg.max_acoustic_pruning, h->cfg.increment_factor, h->cfg.min_average_number_of_states,
                                h->cfg.increase_until_no_score_difference ? 1 : 0};
        a.lds_states = p.max_states, a.lds_cols = std::max(p.max_cols, 1);
        // per state: a mask (8), two scores, two ranks, a base, an offset (6 x 4); two rows; the arcs when they fit beside them
        size_t lds = (size_t)a.lds_states * 32 + 4 + (size_t)a.lds_cols * 8;
        lds        = (lds + 15) / 16 * 16;
        a.lds_arcs = lds + (size_t)p.max_in * sizeof(amx::AlignArc) <= amx::kAlignLdsBytes ? p.max_in : 0;
        lds += (size_t)a.lds_arcs * sizeof(amx::AlignArc);
        if (lds > 48 * 1024 && !h->lds_raised) {
            AMX_HIP(hipFuncSetAttribute((const void*)amx::align_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)amx::kAlignLdsBytes));
            h->lds_raised = true;
        }
        amx::ScopedKernelTimer timer(ctx, "align_search");
        hipLaunchKernelGGL(amx::align_search_kernel, dim3((unsigned)n_seg), dim3(amx::kAlignThreads), lds, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    if (p.frames) {
        amx::AlignTraceArgs a{};
        a.seg = h->d_seg.get(), a.summary = h->d_summary.get(), a.bp = h->d_bp.get(), a.cm = h->d_cm.get();
        a.arc_src = h->d_arc_src.get(), a.arc_label = h->d_arc_label.get(), a.arc_emission = h->d_arc_emission.get(), a.arc_col = h->d_arc_col.get();
        a.arc_w = h->d_arc_w.get(), a.path = h->d_path.get(), a.base = p.off[0];
        a.label = label_dev, a.emission = emission_dev, a.arc_score = arc_score_dev;
        amx::ScopedKernelTimer timer(ctx, "align_traceback");
        hipLaunchKernelGGL(amx::align_traceback_kernel, dim3((unsigned)n_seg), dim3(64), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    h->summary.resize(n_seg);
    AMX_HIP(hipMemcpyAsync(h->summary.data(), h->d_summary.get(), (size_t)n_seg * sizeof(amx::AlignSummary), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < n_seg; ++s) {
        const amx::AlignSummary& r = h->summary[s];
        result[s].score = r.score, result[s].reached_final = r.reached, result[s].n_iterations = r.n_iterations;
        result[s].last_threshold = r.last_threshold, result[s].average_states = r.average, result[s].state_sum = r.sum;
        if (counters)
            counters[0] += r.nan ? 1 : 0, counters[1] += r.passes_run, counters[2] += r.passes_counted;
    }
    return AMX_OK;
}

}  // extern "C"
