// arcalign.hip -- the alignments of a word lattice's arcs (include/amx.h, section "Lattice word-arc alignment"): what
// Speech::PhonemeSequenceAlignmentGenerator::getAlignment runs per distinct (pronunciation, begin time, end time), one Search::Aligner in
// Viterbi mode on the frames [tbeg, tend) of a segment, for tens of thousands of such keys per call on the score matrix in device memory.
//
// The search is align.hip's in every rule (expansion order, recombination, pruning, the loop of thresholds, the first-best final
// hypothesis, the NaN rule) and in its tie scheme: a candidate of target s is keyed (rank of its source << 6 | ordinal of the arc in its
// source), s takes the minimal score and among equals the largest key, and its place in the new list is the number of FIRST keys below
// its own, counted with one 64-bit mask per source rank and an exclusive scan of the masks' popcounts.  The split of the work is another:
// a word arc has 3-60 states and 3-150 frames, so ONE WAVE runs a key, four independent waves share a workgroup, and nothing inside the
// key loop is a workgroup barrier.  State s lives in lane s % 64, slot s / 64 (NS slots: 1 for graphs of <= 64 states and columns, 4 for
// <= 256); a lane keeps its states' scores and ranks in registers and mirrors them in the wave's own slice of LDS, where the targets read
// their sources.  Windows overlap, so there is no compact matrix: a lane fetches its columns of row t + 1 from the score matrix itself
// (L2 serves the overlap) while frame t is worked on.  One byte per (frame, state) -- the ordinal of the winning arc in the target's
// incoming list -- goes to a global workspace; after the last pass the same wave stages those bytes back through LDS, lane 0 follows
// them, and the wave forms (score + weight) + emission again in frame order, 64 frames' operands at a time, for the arc scores and the
// emission-score chain.  Only f32 additions and comparisons happen.
#include <numeric>

#include "align_plan.hpp"

namespace amx {

constexpr int kArcWaves       = 4;                // independent waves (keys in flight) per workgroup
constexpr int kArcThreads     = 64 * kArcWaves;
constexpr int kArcMaxStates   = AMX_ARCALIGN_MAX_STATES;
constexpr int kArcMaxIn       = AMX_ARCALIGN_MAX_IN_ARCS;
constexpr int kArcMaxFrames   = AMX_ARCALIGN_MAX_FRAMES;
constexpr int kArcTraceFrames = 16;               // frames of back-pointers staged into LDS at a time
// Bytes of back-pointers one launch may hold; a call with more is cut into several launches.  Chosen, not tuned: it rests on nothing
// measured, only on staying well below the card's memory next to a score matrix of gigabytes.
constexpr long long kArcBpCapBytes = 256ll << 20;
// arcs a slice holds; a graph with more reads them from memory.  768 arcs are a 256-state left-to-right HMM with loop, forward and skip.
template<int NS> constexpr int kArcLdsArcs = NS == 1 ? 256 : 1024;
// workgroups per CU the launch is sized for: 16 waves (NS = 1, 15 KB each workgroup) and 8 waves (NS = 4, 60 KB).  Chosen, not tuned.
template<int NS> constexpr int kArcBlocksPerCu = NS == 1 ? 4 : 2;
static_assert(kArcMaxStates == 256 && kArcMaxIn == 255, "a source and a back-pointer are one byte each");

// a wave's slice of LDS.  The search's state and the traceback's staged back-pointers never live at the same time.
template<int NS>
struct ArcSlice {
    union {
        struct {
            unsigned long long mask[64 * NS];   // per source rank: the first keys' arc ordinals
            float              score[64 * NS];  // mirror of the lanes' registers, by state
            int                rank[64 * NS];
            int                base[64 * NS];   // exclusive scan of the masks' popcounts
            float              row[64 * NS];    // the frame's gathered, scaled scores by column of the graph
        } s;
        unsigned char bp[kArcTraceFrames * 64 * NS];
    };
    int  in_off[64 * NS + 2];                   // by target, relative to the graph's first arc
    int2 arc[kArcLdsArcs<NS>];
};
static_assert(sizeof(ArcSlice<4>) * kArcWaves <= 64 * 1024 && sizeof(ArcSlice<4>) * 8 <= 160 * 1024, "eight waves of the wide variant fit a CU");
static_assert(kArcTraceFrames <= 8 + 4 * 4, "the staged bytes fit the search's state (24 bytes per state)");

struct ArcKey {
    long long row0;   // first row of the window in scores_dev
    long long bp0;    // first byte of the key's back-pointers in the launch's workspace
    int       slot0, frames, graph, out;   // out: the key's index in the caller's order
};

struct ArcSummary {
    float              score;
    int                reached, n_iterations;
    float              last_threshold;
    double             average;
    unsigned long long sum;
    int                nan, pad;
    unsigned long long passes_run, passes_counted;
};

struct ArcArgs {
    const ArcKey*        key;      // of this launch, in dealing order
    int                  n_keys;
    const AlignSeg*      graph;    // align_plan's view of the graphs (frames unused)
    const int*           in_off;   // [states + 1] by target, global
    const int2*          arc2;     // by target: x = source | ordinal in the source << 8 | column << 16, y = weight bits
    const AlignArc*      in_arc;   // by target, align_plan's form: the traceback reads the arc's number from it
    const int*           cols;
    const unsigned char* is_final;
    const float*         final_w;
    const int *          arc_label, *arc_emission;   // by source-order arc number
    const float*         scores;
    long long            ld;
    float                scale;
    unsigned char*       bp;
    int32_t *            label, *emission;
    float *              arc_score, *key_score, *key_emission;   // arc_score nullable
    ArcSummary*          summary;
    AlignLoop            loop;
};

// Orders the wave's LDS traffic: the hardware runs a wave's LDS operations in program order, the fences keep the compiler to it.
__device__ __forceinline__ void arc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float arc_scaled(float scale, float v) {
    return scale == 1.f ? v : scale * v;   // ScaledContextScorer::score: one rounding
}

// One wave per key; the keys of a launch are dealt to the waves with a static stride in the host's order (descending frames x states).
// Every value that steers control flow outside the per-state code is the same in all lanes of the wave: it comes from the key, the
// graph or a wave reduction.
template<int NS>
__global__ __launch_bounds__(kArcThreads) void arcalign_search_kernel(ArcArgs p) {
    __shared__ ArcSlice<NS> slices[kArcWaves];
    const int       lane = threadIdx.x & 63;
    ArcSlice<NS>&   L    = slices[threadIdx.x >> 6];
    const AlignLoop lp   = p.loop;
    for (int ki = blockIdx.x * kArcWaves + (threadIdx.x >> 6); ki < p.n_keys; ki += gridDim.x * kArcWaves) {
        const ArcKey   key = p.key[ki];
        const AlignSeg g   = p.graph[key.graph];
        const int      S = g.n_states, E = g.n_cols, T = key.frames;
        arc_wave_sync();   // the previous key's reads of the slice are done
        for (int s = lane; s <= S; s += 64)
            L.in_off[s] = p.in_off[g.state0 + s] - g.in0;
        const int2* arcs = p.arc2 + g.in0;   // generic: LDS when the slice has room for them
        if (g.n_in <= kArcLdsArcs<NS>) {
            for (int a = lane; a < g.n_in; a += 64)
                L.arc[a] = p.arc2[g.in0 + a];
            arcs = L.arc;
        }
        int   in_b[NS], in_e[NS], col[NS];
        float fin_w[NS];
        bool  fin[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int s = lane + 64 * k;
            in_b[k]     = s < S ? p.in_off[g.state0 + s] - g.in0 : 0;
            in_e[k]     = s < S ? p.in_off[g.state0 + s + 1] - g.in0 : 0;
            col[k]      = s < E ? p.cols[g.col0 + s] : 0;
            fin[k]      = s < S && p.is_final[g.state0 + s];
            fin_w[k]    = fin[k] ? p.final_w[g.state0 + s] : 0.f;
        }
        const float*   rows = p.scores + key.row0 * p.ld;
        unsigned char* bp   = p.bp + key.bp0;
        float          t = lp.lo, previous = kAlignF32Max, pass_score = kAlignF32Max;
        int            n_iter = 0, best_state = -1;
        unsigned long long sum = 0, passes_run = 0, passes_counted = 0;
        double         avg = 0;
        bool           nan = false;
        while (t <= lp.hi) {
            ++n_iter, ++passes_run;
            // restart(): the startup hypothesis alone (Aligner.cc:198-204)
            float sc[NS];
            int   rk[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int s = lane + 64 * k;
                sc[k] = 0.f, rk[k] = s == g.initial ? 0 : -1;
                if (s < S)
                    L.s.score[s] = 0.f, L.s.rank[s] = rk[k], L.s.mask[s] = 0;
                if (s < E)
                    L.s.row[s] = arc_scaled(p.scale, rows[col[k]]);
            }
            int  n_prev = 1;
            bool pruned = false, met_nan = false;
            sum         = 0;
            arc_wave_sync();
            for (int f = 0; f < T; ++f) {
                const bool ahead = f + 1 < T;
                float      pre[NS];   // the next frame's columns, on their way while this frame is worked on
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    pre[k] = ahead && lane + 64 * k < E ? arc_scaled(p.scale, rows[(long long)(f + 1) * p.ld + col[k]]) : 0.f;
                // expansion and recombination, a lane's target states one at a time (:215-252, :144-167)
                int nk[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    int   first = INT_MAX, bkey = -1, barc = 0;
                    float best  = 0.f;
                    for (int a = in_b[k]; a < in_e[k]; ++a) {
                        const int2 q   = arcs[a];
                        const int  src = q.x & 0xff;
                        const int  r   = L.s.rank[src];
                        if (r < 0)
                            continue;
                        const int   ck  = (r << 6) | ((q.x >> 8) & 63);
                        const float sco = (L.s.score[src] + __int_as_float(q.y)) + L.s.row[q.x >> 16];
                        met_nan         = met_nan || sco != sco;
                        first           = ck < first ? ck : first;
                        if (bkey < 0 || sco < best || (sco == best && ck > bkey))
                            best = sco, bkey = ck, barc = a;
                    }
                    if (bkey >= 0) {
                        atomicOr(&L.s.mask[first >> 6], 1ull << (first & 63));
                        bp[(long long)f * S + lane + 64 * k] = (unsigned char)(barc - in_b[k]);
                    }
                    sc[k] = best;
                    nk[k] = bkey >= 0 ? first : -1;
                }
                arc_wave_sync();
                // exclusive scan of the masks' popcounts over the previous frame's ranks, NS of them per lane
                int cnt[NS], mine = 0;
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const int r = lane * NS + k;
                    cnt[k]      = r < n_prev ? __popcll(L.s.mask[r]) : 0;
                    mine += cnt[k];
                }
                int incl = mine;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int u = __shfl_up(incl, o, 64);
                    incl += lane >= o ? u : 0;
                }
                const int n_new  = __shfl(incl, 63, 64);
                int       before = incl - mine;
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const int r = lane * NS + k;
                    if (r < n_prev)
                        L.s.base[r] = before;
                    before += cnt[k];
                }
                arc_wave_sync();
                // the new ranks, minimumScore() (:254-261) and prune (:294-301)
                float m = kAlignF32Max;
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    rk[k] = -1;
                    if (nk[k] >= 0) {
                        rk[k] = L.s.base[nk[k] >> 6] + __popcll(L.s.mask[nk[k] >> 6] & ((1ull << (nk[k] & 63)) - 1ull));
                        m     = sc[k] < m ? sc[k] : m;
                    }
                }
                m                 = wave_min(m);
                const float limit = m + t;   // :597
                int         kept  = 0;
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    if (rk[k] >= 0) {
                        if (sc[k] <= limit)   // :295
                            ++kept;
                        else
                            rk[k] = -1;
                    }
                kept = wave_sum(kept);
                arc_wave_sync();   // masks and bases are read; the mirrors may change
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const int r = lane * NS + k, s = lane + 64 * k;
                    if (r < n_prev)
                        L.s.mask[r] = 0;
                    if (s < S)
                        L.s.score[s] = sc[k], L.s.rank[s] = rk[k];
                    if (ahead && s < E)
                        L.s.row[s] = pre[k];
                }
                arc_wave_sync();
                sum += (unsigned)kept;   // nStateHypotheses_ += nStateHypothesesCurFrame() (:600)
                pruned = pruned || kept < n_new;
                n_prev = n_new;
            }
            nan = __any(met_nan) != 0;
            if (nan)
                break;
            // finalStatePotential (:385-405) and the best final hypothesis (:408-419): the smallest value, among equals the first in the list
            {
                float bv = kAlignF32Max;
                int   br = INT_MAX, bs = -1;
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    if (rk[k] >= 0 && fin[k]) {
                        const float v = fin_w[k] + sc[k];
                        if (v < kAlignF32Max && (bs < 0 || v < bv || (v == bv && rk[k] < br)))
                            bv = v, br = rk[k], bs = lane + 64 * k;
                    }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ov  = __shfl_xor(bv, o, 64);
                    const int   orr = __shfl_xor(br, o, 64), os = __shfl_xor(bs, o, 64);
                    if (os >= 0 && (bs < 0 || ov < bv || (ov == bv && orr < br)))
                        bv = ov, br = orr, bs = os;
                }
                pass_score = bs >= 0 ? bv : kAlignF32Max;
                best_state = bs;
            }
            avg                = (double)(unsigned)sum / (double)(unsigned)T;   // Core::Statistics<u32>::average
            const bool reached = pass_score != kAlignF32Max;
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
        const bool reached = !nan && pass_score != kAlignF32Max;
        int32_t*   label   = p.label + key.slot0;
        int32_t*   emis    = p.emission + key.slot0;
        float*     arcsc   = p.arc_score ? p.arc_score + key.slot0 : nullptr;
        float      es      = 0.f;   // EmissionLatticeRescorerAutomaton::_score: one chain from 0 in frame order
        if (!reached) {
            for (int f = lane; f < T; f += 64) {
                label[f] = -1, emis[f] = -1;
                if (arcsc)
                    arcsc[f] = 0.f;
            }
        }
        else {
            // lane 0 follows the back-pointers of the last pass from the best final state (:430-442); the key's own label slots hold
            // the path (arcs by target, relative to the graph) until the labels replace it
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");   // the wave's byte stores, before other lanes load them
            int s = best_state;
            for (int f1 = T; f1 > 0; f1 -= kArcTraceFrames) {
                const int f0 = f1 > kArcTraceFrames ? f1 - kArcTraceFrames : 0;
                arc_wave_sync();
                const unsigned char* from = bp + (long long)f0 * S;
                for (int i = lane; i < (f1 - f0) * S; i += 64)
                    L.bp[i] = from[i];
                arc_wave_sync();
                if (lane == 0)
                    for (int f = f1 - 1; f >= f0; --f) {
                        const int a = L.in_off[s] + L.bp[(f - f0) * S + s];
                        __hip_atomic_store(label + f, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        s = arcs[a].x & 0xff;
                    }
                s = __shfl(s, 0, 64);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
            // score[hyp] = (score[trace] + weight) + emission is what the winner was given: formed again in frame order
            float prev = 0.f;
            for (int f0 = 0; f0 < T; f0 += 64) {
                const int      f  = f0 + lane;
                const bool     in = f < T;
                const int      a  = in ? __hip_atomic_load(label + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                const AlignArc q  = in ? p.in_arc[g.in0 + a] : make_int4(0, 0, 0, 0);
                const int      em = in ? p.arc_emission[q.w] : 0;
                const float    w  = __int_as_float(q.z);
                const float    e  = in ? arc_scaled(p.scale, rows[(long long)f * p.ld + em]) : 0.f;
                float          mine = 0.f;
                const int      n    = T - f0 < 64 ? T - f0 : 64;
                for (int i = 0; i < n; ++i) {
                    const float ei   = __shfl(e, i, 64);
                    const float next = (prev + __shfl(w, i, 64)) + ei;
                    if (lane == i)
                        mine = next - prev;   // :438
                    prev = next;
                    es   = es + ei;
                }
                if (in) {
                    label[f] = p.arc_label[q.w], emis[f] = em;
                    if (arcsc)
                        arcsc[f] = mine;
                }
            }
        }
        if (lane == 0) {
            ArcSummary r;
            r.score          = reached ? pass_score : kAlignF32Max;
            r.reached        = reached;
            r.n_iterations   = n_iter;
            r.last_threshold = t;
            r.average        = nan ? 0.0 : avg;
            r.sum            = nan ? 0 : sum;
            r.nan = nan, r.pad = 0;
            r.passes_run = passes_run, r.passes_counted = passes_counted;
            p.summary[key.out]      = r;
            p.key_score[key.out]    = r.score;
            p.key_emission[key.out] = reached ? es : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void arcalign_gather_kernel(const float* __restrict__ key_score, const int* __restrict__ arc_key, int n_arcs,
                                                             float* __restrict__ out) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a < n_arcs)
        out[a] = arc_key[a] < 0 ? 0.f : key_score[arc_key[a]];   // an arc the rescorers give one()
}

template<int NS>
static int arcalign_launch(amx_ctx* ctx, ArcArgs a) {
    const int blocks = std::min(ceil_div(a.n_keys, kArcWaves), std::max(ctx->n_cu, 1) * kArcBlocksPerCu<NS>);
    ScopedKernelTimer timer(ctx, "arcalign_search");
    hipLaunchKernelGGL(arcalign_search_kernel<NS>, dim3((unsigned)blocks), dim3(kArcThreads), 0, ctx->stream, a);
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

}  // namespace amx

struct amx_arcalign {
    amx_ctx*       ctx = nullptr;
    amx_align_cfg  cfg{};
    long long      bp_cap = amx::kArcBpCapBytes;
    amx::AlignPlan plan;   // of the last call's graphs: the uploads read it until the call's synchronisation
    std::vector<amx::ArcKey>     keys;
    std::vector<int2>            arc2;
    std::vector<int>             arc_key;
    std::vector<amx::ArcSummary> summary;
    amx::DevBuf<amx::AlignSeg>   d_graph;
    amx::DevBuf<amx::ArcKey>     d_key;
    amx::DevBuf<int>             d_cols, d_in_off, d_arc_label, d_arc_emission, d_arc_key;
    amx::DevBuf<amx::AlignArc>   d_in_arc;
    amx::DevBuf<int2>            d_arc2;
    amx::DevBuf<unsigned char>   d_is_final, d_bp;
    amx::DevBuf<float>           d_final_w, d_key_score;   // d_key_score: [2][n_keys] alignment | emission, of the last run
    amx::DevBuf<amx::ArcSummary> d_summary;
    int                          n_keys = -1;   // of the last run; -1: none
    int                          last_launches = 0;
};

extern "C" {

int amx_arcalign_create(amx_ctx* ctx, const amx_align_cfg* cfg, amx_arcalign** out) {
    const char* who = "amx_arcalign_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(cfg, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(cfg->mode == AMX_ALIGN_VITERBI || cfg->mode == AMX_ALIGN_BAUM_WELCH, AMX_ERR_INVALID, "%s: mode %d is none", who, cfg->mode);
    AMX_REQUIRE(cfg->mode == AMX_ALIGN_VITERBI, AMX_ERR_UNSUPPORTED, "%s: mode baum-welch: arc alignments are built in mode viterbi only", who);
    AMX_TRY(amx::align_check_search_cfg(who, cfg->min_acoustic_pruning, cfg->max_acoustic_pruning, cfg->increment_factor,
                                        cfg->min_average_number_of_states, cfg->n_best_pruning, cfg->score_scale));
    std::unique_ptr<amx_arcalign> h(new amx_arcalign);
    h->ctx = ctx;
    h->cfg = *cfg;
    *out   = h.release();
    return AMX_OK;
}

void amx_arcalign_destroy(amx_arcalign* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

void amx_arcalign_kernel_shape(int wide, int* states_per_lane, int* keys_per_workgroup, int* lds_bytes_per_wave, int* lds_arcs) {
    if (states_per_lane)
        *states_per_lane = wide ? 4 : 1;
    if (keys_per_workgroup)
        *keys_per_workgroup = amx::kArcWaves;
    if (lds_bytes_per_wave)
        *lds_bytes_per_wave = (int)(wide ? sizeof(amx::ArcSlice<4>) : sizeof(amx::ArcSlice<1>));
    if (lds_arcs)
        *lds_arcs = wide ? amx::kArcLdsArcs<4> : amx::kArcLdsArcs<1>;
}

int amx_arcalign_set_workspace_cap(amx_arcalign* h, long long bytes) {
    AMX_REQUIRE(h && bytes >= 0, AMX_ERR_INVALID, "amx_arcalign_set_workspace_cap: NULL handle or a negative size");
    h->bp_cap = bytes ? bytes : amx::kArcBpCapBytes;
    return AMX_OK;
}

int amx_arcalign_last_launches(const amx_arcalign* h) {
    return h ? h->last_launches : 0;
}

int amx_arcalign_run_dev(amx_arcalign* h, int n_graphs, const amx_align_graphs* graphs, int n_keys, const int* key_graph, const int* key_segment,
                         const int* key_tbeg, const int* key_tend, int n_seg, const long* frame_offsets, const float* scores_dev, int scores_ld,
                         int n_columns, long* slot_offsets, int32_t* item_label_dev, int32_t* item_emission_dev, float* item_arc_score_dev,
                         float* key_score_dev, float* key_emission_score_dev, amx_align_result* result, unsigned long long counters[3]) {
    const char* who = "amx_arcalign_run_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_graphs >= 0 && n_keys >= 0 && n_seg >= 0 && n_columns >= 1 && scores_ld >= n_columns, AMX_ERR_INVALID,
                "%s: n_graphs %d, n_keys %d, n_seg %d, scores_ld %d with %d columns", who, n_graphs, n_keys, n_seg, scores_ld, n_columns);
    if (n_keys == 0) {
        if (counters)
            counters[0] = counters[1] = counters[2] = 0;
        if (slot_offsets)
            slot_offsets[0] = 0;
        h->n_keys = 0, h->last_launches = 0;
        return AMX_OK;
    }
    AMX_REQUIRE(key_graph && key_segment && key_tbeg && key_tend && frame_offsets && slot_offsets && result, AMX_ERR_INVALID, "%s: NULL key table, segment list, slot_offsets or result", who);
    // the graphs: align_plan's checks and tables, every graph a segment without frames (its messages say "segment g" for graph g)
    amx::AlignPlan& p = h->plan;
    p                 = amx::AlignPlan();
    if (n_graphs) {
        const std::vector<long> none((size_t)n_graphs + 1, 0);
        AMX_TRY(amx::align_plan(n_graphs, none.data(), graphs, n_columns, "amx_arcalign_run_dev: graphs (graph g is segment g here)", &p));
    }
    for (int g = 0; g < n_graphs; ++g) {
        const amx::AlignSeg& sg = p.seg[g];
        AMX_REQUIRE(sg.n_states <= amx::kArcMaxStates, AMX_ERR_UNSUPPORTED,
                    "%s: graph %d has %d states, more than the limit of %d states per arc alignment (amx_align_viterbi_dev takes it on its own rows)", who, g,
                    sg.n_states, amx::kArcMaxStates);
        AMX_REQUIRE(sg.n_cols <= amx::kArcMaxStates, AMX_ERR_UNSUPPORTED,
                    "%s: graph %d uses %d emission indices, more than the limit of %d per arc alignment (amx_align_viterbi_dev takes it on its own rows)", who,
                    g, sg.n_cols, amx::kArcMaxStates);
        for (int s = 0; s < sg.n_states; ++s) {
            const int n_in = p.in_off[(size_t)sg.state0 + s + 1] - p.in_off[(size_t)sg.state0 + s];
            AMX_REQUIRE(n_in <= amx::kArcMaxIn, AMX_ERR_UNSUPPORTED, "%s: graph %d: %d arcs into state %d, more than the limit of %d arcs into a state", who, g,
                        n_in, s, amx::kArcMaxIn);
        }
    }
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: negative frame offset", who);
    for (int s = 0; s < n_seg; ++s)
        AMX_REQUIRE(frame_offsets[s] <= frame_offsets[s + 1], AMX_ERR_INVALID, "%s: frame offsets decrease at segment %d", who, s);
    long long slots = 0;
    for (int k = 0; k < n_keys; ++k) {
        AMX_REQUIRE(key_graph[k] >= 0 && key_graph[k] < n_graphs, AMX_ERR_INVALID, "%s: key %d: graph %d outside the %d graphs", who, k, key_graph[k], n_graphs);
        AMX_REQUIRE(key_segment[k] >= 0 && key_segment[k] < n_seg, AMX_ERR_INVALID, "%s: key %d: segment %d outside the %d segments", who, k, key_segment[k],
                    n_seg);
        const long len = frame_offsets[key_segment[k] + 1] - frame_offsets[key_segment[k]];
        AMX_REQUIRE(key_tbeg[k] < key_tend[k], AMX_ERR_INVALID, "%s: key %d: begin time %d is not below end time %d (such an arc has no alignment: its key is -1)",
                    who, k, key_tbeg[k], key_tend[k]);
        AMX_REQUIRE(key_tbeg[k] >= 0 && key_tend[k] <= len, AMX_ERR_INVALID, "%s: key %d: frames [%d, %d) outside segment %d of %ld frames", who, k, key_tbeg[k],
                    key_tend[k], key_segment[k], len);
        AMX_REQUIRE(key_tend[k] - key_tbeg[k] <= amx::kArcMaxFrames, AMX_ERR_UNSUPPORTED, "%s: key %d has %d frames, more than the limit of %d frames per arc alignment",
                    who, k, key_tend[k] - key_tbeg[k], amx::kArcMaxFrames);
        slots += key_tend[k] - key_tbeg[k];
    }
    AMX_REQUIRE(slots < (1ll << 31), AMX_ERR_UNSUPPORTED, "%s: %lld frames over all keys are more than one call takes", who, slots);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(scores_dev && item_label_dev && item_emission_dev && key_score_dev && key_emission_score_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    if (counters)
        counters[0] = counters[1] = counters[2] = 0;
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    // the keys: narrow graphs first, each class by descending frames x states (the index breaks ties, so a call's dealing is a function of its input)
    slot_offsets[0] = 0;
    for (int k = 0; k < n_keys; ++k)
        slot_offsets[k + 1] = slot_offsets[k] + (key_tend[k] - key_tbeg[k]);
    auto wide = [&](int k) { return p.seg[key_graph[k]].n_states > 64 || p.seg[key_graph[k]].n_cols > 64; };
    auto work = [&](int k) { return (long long)(key_tend[k] - key_tbeg[k]) * p.seg[key_graph[k]].n_states; };
    std::vector<int> order(n_keys);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        if (wide(a) != wide(b))
            return wide(b);
        return work(a) != work(b) ? work(a) > work(b) : a < b;
    });
    // launches: a class's keys in order until the back-pointers would pass the cap (a key above the cap goes alone)
    struct Launch {
        int       first, n;
        bool      wide;
        long long bytes;
    };
    std::vector<Launch> launches;
    h->keys.resize(n_keys);
    long long most = 1;
    for (int i = 0; i < n_keys; ++i) {
        const int       k     = order[i];
        const long long bytes = work(k);
        if (launches.empty() || launches.back().wide != wide(k) || launches.back().bytes + bytes > h->bp_cap)
            launches.push_back(Launch{i, 0, wide(k), 0});
        amx::ArcKey& d = h->keys[i];
        d.row0 = frame_offsets[key_segment[k]] + key_tbeg[k], d.bp0 = launches.back().bytes, d.slot0 = (int)slot_offsets[k];
        d.frames = key_tend[k] - key_tbeg[k], d.graph = key_graph[k], d.out = k;
        ++launches.back().n, launches.back().bytes += bytes;
        most = std::max(most, launches.back().bytes);
    }
    h->arc2.resize(p.in_arc.size());
    for (size_t a = 0; a < p.in_arc.size(); ++a)
        h->arc2[a] = make_int2((p.in_arc[a].x & 0xffff) | ((p.in_arc[a].x >> 16) << 8) | (p.in_arc[a].y << 16), p.in_arc[a].z);
    AMX_TRY(amx::align_upload(ctx, h->d_graph, p.seg));
    AMX_TRY(amx::align_upload(ctx, h->d_key, h->keys));
    AMX_TRY(amx::align_upload(ctx, h->d_cols, p.cols));
    AMX_TRY(amx::align_upload(ctx, h->d_in_off, p.in_off));
    AMX_TRY(amx::align_upload(ctx, h->d_in_arc, p.in_arc));
    AMX_TRY(amx::align_upload(ctx, h->d_arc2, h->arc2));
    AMX_TRY(amx::align_upload(ctx, h->d_is_final, p.is_final));
    AMX_TRY(amx::align_upload(ctx, h->d_final_w, p.final_w));
    AMX_TRY(amx::align_upload(ctx, h->d_arc_label, p.arc_label));
    AMX_TRY(amx::align_upload(ctx, h->d_arc_emission, p.arc_emission));
    AMX_TRY(h->d_bp.reserve((size_t)most));
    AMX_TRY(h->d_summary.reserve(n_keys));
    AMX_TRY(h->d_key_score.reserve((size_t)2 * n_keys));
    h->n_keys = -1;   // until this run has ended
    amx::ArcArgs a{};
    a.graph = h->d_graph.get(), a.in_off = h->d_in_off.get(), a.arc2 = h->d_arc2.get(), a.in_arc = h->d_in_arc.get(), a.cols = h->d_cols.get();
    a.is_final = h->d_is_final.get(), a.final_w = h->d_final_w.get(), a.arc_label = h->d_arc_label.get(), a.arc_emission = h->d_arc_emission.get();
    a.scores = scores_dev, a.ld = scores_ld, a.scale = h->cfg.score_scale, a.bp = h->d_bp.get();
    a.label = item_label_dev, a.emission = item_emission_dev, a.arc_score = item_arc_score_dev;
    a.key_score = h->d_key_score.get(), a.key_emission = h->d_key_score.get() + n_keys, a.summary = h->d_summary.get();
    a.loop = amx::AlignLoop{h->cfg.min_acoustic_pruning, h->cfg.max_acoustic_pruning, h->cfg.increment_factor, h->cfg.min_average_number_of_states,
                            h->cfg.increase_until_no_score_difference ? 1 : 0};
    for (const Launch& l : launches) {   // in stream order: each launch has the workspace to itself
        a.key = h->d_key.get() + l.first, a.n_keys = l.n;
        AMX_TRY(l.wide ? amx::arcalign_launch<4>(ctx, a) : amx::arcalign_launch<1>(ctx, a));
    }
    h->last_launches = (int)launches.size();
    AMX_HIP(hipMemcpyAsync(key_score_dev, a.key_score, (size_t)n_keys * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(key_emission_score_dev, a.key_emission, (size_t)n_keys * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    h->summary.resize(n_keys);
    AMX_HIP(hipMemcpyAsync(h->summary.data(), h->d_summary.get(), (size_t)n_keys * sizeof(amx::ArcSummary), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n_keys; ++k) {
        const amx::ArcSummary& r = h->summary[k];
        result[k].score = r.score, result[k].reached_final = r.reached, result[k].n_iterations = r.n_iterations;
        result[k].last_threshold = r.last_threshold, result[k].average_states = r.average, result[k].state_sum = r.sum;
        if (counters)
            counters[0] += r.nan ? 1 : 0, counters[1] += r.passes_run, counters[2] += r.passes_counted;
    }
    h->n_keys = n_keys;
    return AMX_OK;
}

int amx_arcalign_arc_scores_dev(amx_arcalign* h, int n_arcs, const int32_t* arc_key, int which, float* arc_score_dev) {
    const char* who = "amx_arcalign_arc_scores_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_arcs >= 0 && (which == AMX_ARCALIGN_ALIGNMENT_SCORE || which == AMX_ARCALIGN_EMISSION_SCORE), AMX_ERR_INVALID, "%s: n_arcs %d, which %d", who,
                n_arcs, which);
    AMX_REQUIRE(h->n_keys >= 0, AMX_ERR_STATE, "%s: no amx_arcalign_run_dev has ended on this handle", who);
    if (n_arcs == 0)
        return AMX_OK;
    AMX_REQUIRE(arc_key, AMX_ERR_INVALID, "%s: NULL arc_key", who);
    for (int a = 0; a < n_arcs; ++a)
        AMX_REQUIRE(arc_key[a] >= -1 && arc_key[a] < h->n_keys, AMX_ERR_INVALID, "%s: arc %d: key %d outside the %d keys of the last run", who, a, arc_key[a],
                    h->n_keys);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(arc_score_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    h->arc_key.assign(arc_key, arc_key + n_arcs);   // the upload reads it until the synchronisation below
    AMX_TRY(amx::align_upload(ctx, h->d_arc_key, h->arc_key));
    {
        amx::ScopedKernelTimer timer(ctx, "arcalign_gather");
        hipLaunchKernelGGL(amx::arcalign_gather_kernel, dim3((unsigned)amx::ceil_div(n_arcs, 256)), dim3(256), 0, ctx->stream,
                           h->d_key_score.get() + (which == AMX_ARCALIGN_EMISSION_SCORE ? h->n_keys : 0), h->d_arc_key.get(), n_arcs, arc_score_dev);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    return AMX_OK;
}

long amx_arcalign_expand(int n_keys, const int* key_segment, const int* key_tbeg, const int* key_tend, const long* slot_offsets,
                         const int32_t* slot_emission, int n_seg, const long* arc_offsets, const int32_t* arc_key, long* item_offsets,
                         int32_t* item_frame, int32_t* item_emission) {
    const char* who = "amx_arcalign_expand";
    AMX_REQUIRE(n_keys >= 0 && n_seg >= 0 && arc_offsets && arc_offsets[0] == 0, AMX_ERR_INVALID, "%s: n_keys %d, n_seg %d, or arc_offsets that do not start at 0",
                who, n_keys, n_seg);
    for (int s = 0; s < n_seg; ++s)
        AMX_REQUIRE(arc_offsets[s] <= arc_offsets[s + 1], AMX_ERR_INVALID, "%s: arc offsets decrease at segment %d", who, s);
    const long n_arcs = arc_offsets[n_seg];
    AMX_REQUIRE(n_arcs == 0 || arc_key, AMX_ERR_INVALID, "%s: NULL arc_key", who);
    AMX_REQUIRE(n_keys == 0 || (key_segment && key_tbeg && key_tend && slot_offsets && slot_emission), AMX_ERR_INVALID, "%s: NULL key or slot table", who);
    const bool write = item_offsets && item_frame && item_emission;
    AMX_REQUIRE(write || (!item_offsets && !item_frame && !item_emission), AMX_ERR_INVALID, "%s: the three output tables are given together or not at all", who);
    long n = 0;
    for (int s = 0; s < n_seg; ++s)
        for (long a = arc_offsets[s]; a < arc_offsets[s + 1]; ++a) {
            const int k = arc_key[a];
            AMX_REQUIRE(k >= -1 && k < n_keys, AMX_ERR_INVALID, "%s: arc %ld: key %d outside the %d keys", who, a, k, n_keys);
            AMX_REQUIRE(k < 0 || key_segment[k] == s, AMX_ERR_INVALID, "%s: arc %ld of segment %d has key %d of segment %d", who, a, s, k, k < 0 ? 0 : key_segment[k]);
            if (write)
                item_offsets[a] = n;
            if (k < 0 || key_tbeg[k] >= key_tend[k] || slot_emission[slot_offsets[k]] < 0)   // the rescorers' one(), or no final state reached
                continue;
            const int T = key_tend[k] - key_tbeg[k];
            if (write)
                for (int i = 0; i < T; ++i)
                    item_frame[n + i] = key_tbeg[k] + i, item_emission[n + i] = slot_emission[slot_offsets[k] + i];
            n += T;
        }
    if (write)
        item_offsets[n_arcs] = n;
    return n;
}

}  // extern "C"
