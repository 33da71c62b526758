// latbest.hip -- lattice best path and forward-backward pruning on the device: Fsa::bestscore / Fsa::best (Fsa/tBest.cc:30-123) and
// Fsa::prunePosterior (Fsa/tPrune.cc:28-146) in the tropical semiring of tolerance 1, for a batch of lattices.
//
// Nothing here is a max-reduction: a potential, a best arc and the pruning minimum are each ONE chain of tolerant comparisons
// (latbest_plan.hpp: latbest_less) in the order the reference meets the candidates; an exact minimum gives other bits.
//
// latbest_potentials_kernel  one workgroup per (segment, direction) climbs the plan's levels with one barrier between them.  A lane takes
//                            a state and runs its chain over the arcs the plan lists (latbest_host.cpp: by the topological queue's order);
//                            a state of kLatWaveArcs arcs or more is shared by a wave: 64 lanes load one arc each and compute ext, then
//                            the chain is resolved by ballot (lat_chain_wave).  f32 potentials in LDS while the states fit
//                            (kLatBestLdsStates), in global memory otherwise, the same bits.
// latbest_arc_kernel / latbest_arc_wide_kernel   the best arc per state (lane / wave with the same ballot chain).
// latbest_path_kernel        one lane per segment follows best_arc from the initial state.
// latbest_min_kernel         one wave per segment: the single discover-order chain of minWeight over all arcs.
// latbest_keep_kernel        one lane per arc: compare(w(a), minWeight) <= 0.
// latbest_trim_kernel        two Boolean sweeps over the same levels: reached from the initial state / reaching a final state over kept arcs.
// latbest_scan_kernel        one workgroup per segment: applies the trim, scans keep into kept_index, counts.
// No floating-point atomics; a segment's bits depend on the segment alone.
#include <cfloat>
#include <chrono>

#include "common.hpp"
#include "latbest_plan.hpp"

namespace amx {

constexpr int   kLatBestThreads   = 256;
constexpr int   kLatBestLdsStates = 8192;   // x 4 bytes: 32 KB of LDS, the budget of latpost's 4096 f64 potentials
constexpr float kLatBestZero      = FLT_MAX;   // Zero and max() of the semiring (Fsa/tRealSemiring.cc:91-103)

struct LatBestArgs {
    const LatWalk*    walk;
    const LatBestSeg* seg;
    const int32_t *node_arcs, *node_final, *warc_peer, *warc_arc, *order, *levels, *arc_source, *arc_target, *state_seg, *disc_arc, *wide_state, *reached;
    const float *  node_fw, *warc_weight, *arc_weight, *final_weight;
    const uint8_t* final_flag;
    const long*    arc_offsets;
    float*         pot;      // [n_nodes]
    float*         ends;     // [3 x n_seg]: the best score, minWeight before and after the threshold
    int32_t*       counts;   // [2 x n_seg]: path length, kept arcs
    int32_t*       reach;    // [n_nodes]: the trim's flags
    int32_t *      best_arc, *path, *kept_index;
    uint8_t*       keep;
    long           n_arcs, n_states;
    int            n_seg, n_wide, relative, trim, prune, force_global;
    float          threshold;
};

// One trip of a chain shared by a wave: lane j holds candidate j (ext, valid).  Serially, candidate j replaces d when latbest_less(ext_j, d)
// with the d that the candidates before it have left.  By ballot: every lane votes against the current d; the lowest voter is the next
// replacement (nothing before it has changed d), its value is read, and only the lanes behind it vote again.  Rounds = replacements.
// Returns the new d; *winner is the last replacing lane (unchanged without one).
__device__ __forceinline__ float lat_chain_wave(float d, float ext, bool valid, int* winner) {
    unsigned long long behind = ~0ull;
    for (;;) {
        const unsigned long long votes = __ballot(valid && latbest_less(ext, d)) & behind;
        if (!votes)
            break;
        const int l = __ffsll((long long)votes) - 1;
        d           = __shfl(ext, l);
        *winner     = l;
        behind      = l == 63 ? 0ull : ~0ull << (l + 1);
    }
    return d;
}

__global__ __launch_bounds__(kLatBestThreads) void latbest_potentials_kernel(LatBestArgs a) {
    __shared__ float lds[kLatBestLdsStates];
    const LatWalk    w      = a.walk[blockIdx.x];
    const LatBestSeg g      = a.seg[blockIdx.x >> 1];
    const bool       fwd    = (blockIdx.x & 1) == 0;
    const bool       in_lds = !a.force_global && w.n_nodes <= kLatBestLdsStates;
    float*           pot    = in_lds ? lds : a.pot + w.node_base;
    const int        tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < w.n_nodes; i += kLatBestThreads)
        pot[i] = (fwd && i == g.initial) ? 0.f : kLatBestZero;   // d(maxStateId + 1, zero), d[start] = one
    __syncthreads();
    const int32_t* order  = a.order + w.order_base;
    const int32_t* levels = a.levels + w.level_base;
    const int32_t* narcs  = a.node_arcs + w.node_base;
    for (int l = 0; l < w.n_levels; ++l) {
        const int b = levels[2 * l], wb = levels[2 * l + 1], e = levels[2 * l + 2];
        for (int i = b + tid; i < wb; i += kLatBestThreads) {
            const int v = order[i];
            float     d = pot[v];
            if (a.node_final[w.node_base + v]) {   // the new initial state is dequeued first: extend(one, final weight)
                const float ext = 0.f + a.node_fw[w.node_base + v];
                if (latbest_less(ext, d))
                    d = ext;
            }
            for (int k = narcs[v]; k < narcs[v + 1]; ++k) {
                const float ds = pot[a.warc_peer[k]];
                if (ds == kLatBestZero)
                    continue;   // never replaced, so never queued: it relaxes nothing
                const float ext = ds + a.warc_weight[k];
                if (latbest_less(ext, d))
                    d = ext;
            }
            pot[v] = d;
        }
        for (int i = wb + wave; i < e; i += kLatBestThreads / 64) {
            const int v = order[i];
            float     d = pot[v];
            int       winner;
            if (a.node_final[w.node_base + v]) {
                const float ext = 0.f + a.node_fw[w.node_base + v];
                if (latbest_less(ext, d))
                    d = ext;
            }
            const int a0 = narcs[v], a1 = narcs[v + 1];
            for (int c = a0; c < a1; c += 64) {
                const int k     = c + lane;
                float     ext   = 0.f;
                bool      valid = false;
                if (k < a1) {
                    const float ds = pot[a.warc_peer[k]];
                    valid          = ds != kLatBestZero;
                    ext            = ds + a.warc_weight[k];
                }
                d = lat_chain_wave(d, ext, valid, &winner);
            }
            if (lane == 0)
                pot[v] = d;
        }
        __syncthreads();   // a level's potentials (LDS or global, written by this workgroup) before the next level reads them
    }
    if (in_lds)
        for (int i = tid; i < w.n_nodes; i += kLatBestThreads)
            a.pot[w.node_base + i] = pot[i];
}

// BestAutomaton::getState (tBest.cc:70-95) for every reached state with fewer than kLatWaveArcs arcs; clears path
__global__ __launch_bounds__(256) void latbest_arc_kernel(LatBestArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_states)
        return;
    a.path[i]          = -1;
    const LatBestSeg g = a.seg[a.state_seg[i]];
    const long       a0 = a.arc_offsets[i], a1 = a.arc_offsets[i + 1];
    if (a1 - a0 >= kLatWaveArcs && !g.dead && a.reached[i] >= 0)
        return;   // latbest_arc_wide_kernel's
    int best = -1;
    if (!g.dead && a.reached[i] >= 0) {
        const float* bw = a.pot + g.node_bwd;
        float        mn = kLatBestZero;
        for (long k = a0; k < a1; ++k) {
            const float w = a.arc_weight[k] + bw[a.arc_target[k]];
            if (latbest_less(w, mn))
                mn = w, best = (int)k;
        }
        if (a.final_flag[i] && latbest_less(a.final_weight[i], mn))
            best = -1;
    }
    a.best_arc[i] = best;
}

__global__ __launch_bounds__(64) void latbest_arc_wide_kernel(LatBestArgs a) {
    const int        i    = a.wide_state[blockIdx.x];
    const int        lane = threadIdx.x;
    const LatBestSeg g    = a.seg[a.state_seg[i]];
    const float*     bw   = a.pot + g.node_bwd;
    const long       a0 = a.arc_offsets[i], a1 = a.arc_offsets[i + 1];
    float            mn   = kLatBestZero;
    long             best = -1;
    for (long c = a0; c < a1; c += 64) {
        const long k      = c + lane;
        const float w     = k < a1 ? a.arc_weight[k] + bw[a.arc_target[k]] : 0.f;
        int         winner = -1;
        mn                = lat_chain_wave(mn, w, k < a1, &winner);
        if (winner >= 0)
            best = c + winner;
    }
    if (a.final_flag[i] && latbest_less(a.final_weight[i], mn))
        best = -1;
    if (lane == 0)
        a.best_arc[i] = (int)best;
}

__global__ __launch_bounds__(64) void latbest_path_kernel(LatBestArgs a) {
    const int gi = blockIdx.x * 64 + threadIdx.x;
    if (gi >= a.n_seg)
        return;
    const LatBestSeg g   = a.seg[gi];
    int              len = 0;
    if (!g.dead)
        for (int s = g.initial; len < g.n_states;) {   // acyclic: at most n_states - 1 arcs
            const int arc = a.best_arc[g.state0 + s];
            if (arc < 0)
                break;
            a.path[g.state0 + len++] = arc;
            s                        = a.arc_target[arc];
        }
    a.counts[2 * gi] = len;
    a.ends[3 * gi]   = g.dead ? -FLT_MAX : a.pot[g.node_bwd + g.initial];   // bestscore: semiring()->invalid() = Core::Type<f32>::min
}

// w(a) = extend(forward[s], extend(weight, backward[target])) (tPrune.cc:104-105, :116-117)
__device__ __forceinline__ float lat_arc_score(const LatBestArgs& a, const LatBestSeg& g, long k) {
    const float w = a.arc_weight[k] + a.pot[g.node_bwd + a.arc_target[k]];
    return a.pot[g.node_fwd + (a.arc_source[k] - g.state0)] + w;
}

// setMinWeight (tPrune.cc:49-58): relative, one chain over the arcs of the discovered states in discover order
__global__ __launch_bounds__(64) void latbest_min_kernel(LatBestArgs a) {
    const int        gi   = blockIdx.x;
    const int        lane = threadIdx.x;
    const LatBestSeg g    = a.seg[gi];
    float            mn = kLatBestZero, after = kLatBestZero;
    if (a.prune && !g.dead) {
        if (a.relative) {
            int winner;
            for (int c = 0; c < g.n_disc; c += 64) {
                const int   k = c + lane;
                const float w = k < g.n_disc ? lat_arc_score(a, g, a.disc_arc[g.disc_base + k]) : 0.f;
                mn            = lat_chain_wave(mn, w, k < g.n_disc, &winner);
            }
        }
        else
            mn = a.pot[g.node_bwd + g.initial];
        after = mn + a.threshold;
    }
    if (lane == 0)
        a.ends[3 * gi + 1] = mn, a.ends[3 * gi + 2] = after;
}

// PosteriorPruneAutomaton::getState (tPrune.cc:110-125)
__global__ __launch_bounds__(256) void latbest_keep_kernel(LatBestArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_arcs)
        return;
    const int s    = a.arc_source[i];
    const int gi   = a.state_seg[s];
    uint8_t   keep = 1;
    if (a.prune) {
        const LatBestSeg g = a.seg[gi];
        keep               = !g.dead && a.reached[s] >= 0 && latbest_compare(lat_arc_score(a, g, i), a.ends[3 * gi + 2]) <= 0;
    }
    a.keep[i] = keep;
}

__global__ __launch_bounds__(kLatBestThreads) void latbest_trim_kernel(LatBestArgs a) {
    const LatWalk    w     = a.walk[blockIdx.x];
    const LatBestSeg g     = a.seg[blockIdx.x >> 1];
    const bool       fwd   = (blockIdx.x & 1) == 0;
    int32_t*         reach = a.reach + w.node_base;
    const int        tid   = threadIdx.x;
    for (int i = tid; i < w.n_nodes; i += kLatBestThreads)
        reach[i] = 0;
    __syncthreads();
    const int32_t* order  = a.order + w.order_base;
    const int32_t* levels = a.levels + w.level_base;
    const int32_t* narcs  = a.node_arcs + w.node_base;
    for (int l = 0; l < w.n_levels; ++l) {
        for (int i = levels[2 * l] + tid; i < levels[2 * l + 2]; i += kLatBestThreads) {
            const int v = order[i];
            int       r = fwd ? v == g.initial : a.node_final[w.node_base + v] != 0;
            for (int k = narcs[v]; k < narcs[v + 1] && !r; ++k)
                r = a.keep[a.warc_arc[k]] && reach[a.warc_peer[k]];
            reach[v] = r;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kLatBestThreads) void latbest_scan_kernel(LatBestArgs a) {
    __shared__ int   wsum[kLatBestThreads / 64];
    const int        gi  = blockIdx.x;
    const LatBestSeg g   = a.seg[gi];
    const int        tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int              base = 0;
    for (int c = 0; c < g.n_arcs; c += kLatBestThreads) {
        const long k    = (long)g.arc0 + c + tid;
        bool       keep = false;
        if (c + tid < g.n_arcs) {
            keep = a.keep[k] != 0;
            if (a.trim) {
                keep = keep && a.reach[g.node_fwd + (a.arc_source[k] - g.state0)] && a.reach[g.node_bwd + a.arc_target[k]];
                a.keep[k] = keep;
            }
        }
        const unsigned long long votes = __ballot(keep);
        if (lane == 0)
            wsum[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, total = 0;
        for (int j = 0; j < kLatBestThreads / 64; ++j) {
            before += j < wave ? wsum[j] : 0;
            total += wsum[j];
        }
        if (c + tid < g.n_arcs)
            a.kept_index[k] = keep ? base + before + __popcll(votes & ((1ull << lane) - 1)) : -1;
        base += total;
        __syncthreads();
    }
    if (tid == 0)
        a.counts[2 * gi + 1] = base;
}

}  // namespace amx

struct amx_latbest {
    amx_ctx*        ctx = nullptr;
    amx_latbest_cfg cfg{};
    amx::DevBuf<int32_t> d_ints;
    amx::DevBuf<float>   d_floats;
    amx::DevBuf<long>    d_arc_offsets;
    amx::DevBuf<uint8_t> d_final_flag;
    amx::DevBuf<amx::LatWalk>    d_walk;
    amx::DevBuf<amx::LatBestSeg> d_seg;
    amx::DevBuf<float>           d_pot;    // [n_nodes + 3 x n_seg]: potentials, the segments' ends
    amx::DevBuf<int32_t>         d_work;   // [n_nodes + 2 x n_seg]: the trim's flags, the segments' counts
    std::vector<amx::LatBestSeg> last_seg;
    long                         last_nodes = 0, last_states = 0;
    double                       last_plan_ms = 0, last_upload_ms = 0;
};

extern "C" {

int amx_latbest_create(amx_ctx* ctx, const amx_latbest_cfg* cfg, amx_latbest** out) {
    const char* who = "amx_latbest_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    amx_latbest_cfg c;
    amx_latbest_cfg_default(&c);
    if (cfg)
        c = *cfg;
    AMX_REQUIRE(c.threshold == c.threshold, AMX_ERR_INVALID, "%s: threshold is not a number", who);
    AMX_REQUIRE(c.potentials == AMX_LATPOST_POTENTIALS_AUTO || c.potentials == AMX_LATPOST_POTENTIALS_GLOBAL, AMX_ERR_INVALID, "%s: potentials %d", who,
                c.potentials);
    std::unique_ptr<amx_latbest> h(new amx_latbest);
    h->ctx = ctx;
    h->cfg = c;
    *out   = h.release();
    return AMX_OK;
}

void amx_latbest_destroy(amx_latbest* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

void amx_latbest_kernel_shape(int* threads, int* lds_states, int* wave_arcs) {
    if (threads)
        *threads = amx::kLatBestThreads;
    if (lds_states)
        *lds_states = amx::kLatBestLdsStates;
    if (wave_arcs)
        *wave_arcs = amx::kLatWaveArcs;
}

int amx_latbest_run_dev(amx_latbest* h, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target, const float* arc_weight,
                        const int32_t* initial, const uint8_t* final_flag, const float* final_weight, int32_t* best_arc_dev, int32_t* path_dev,
                        uint8_t* keep_dev, int32_t* kept_index_dev, amx_latbest_info* info) {
    const char* who = "amx_latbest_run_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    amx::LatBestPlan p;
    const auto       t0 = std::chrono::steady_clock::now();
    AMX_TRY(amx::latbest_plan(n_seg, state_offsets, arc_offsets, arc_target, arc_weight, initial, final_flag, final_weight, who, &p));
    const auto t1 = std::chrono::steady_clock::now();
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(best_arc_dev && path_dev && (p.n_arcs == 0 || (keep_dev && kept_index_dev)), AMX_ERR_INVALID,
                "%s: NULL best_arc_dev, path_dev, keep_dev or kept_index_dev", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    h->last_seg.clear();

    // one table of 32-bit integers and one of floats, uploaded once per call; the host copies live until the call's one synchronisation
    std::vector<int32_t> ints;
    std::vector<float>   floats;
    auto put = [](auto& table, const auto* v, size_t n) {
        const size_t at = table.size();
        table.insert(table.end(), v, v + n);
        return at;
    };
    const size_t nA = (size_t)p.n_arcs, nS = (size_t)p.n_states, nN = (size_t)p.n_nodes;
    const size_t i_node_arcs = put(ints, p.node_arcs.data(), p.node_arcs.size()), i_node_final = put(ints, p.node_final.data(), nN);
    const size_t i_peer = put(ints, p.warc_peer.data(), p.warc_peer.size()), i_warc = put(ints, p.warc_arc.data(), p.warc_arc.size());
    const size_t i_order = put(ints, p.order.data(), p.order.size()), i_levels = put(ints, p.levels.data(), p.levels.size());
    const size_t i_src = put(ints, p.arc_source.data(), nA), i_tgt = put(ints, arc_target, nA), i_sseg = put(ints, p.state_seg.data(), nS);
    const size_t i_disc = put(ints, p.disc_arc.data(), p.disc_arc.size()), i_wide = put(ints, p.wide_state.data(), p.wide_state.size());
    const size_t i_reached = put(ints, p.discover_index.data(), nS);
    const size_t f_fw = put(floats, p.node_fw.data(), nN), f_ww = put(floats, p.warc_weight.data(), p.warc_weight.size());
    const size_t f_aw = put(floats, arc_weight, nA);
    std::vector<float> fin_w(nS, 0.f);   // read only where the flag is set: unset entries may be anything, NaN included
    for (size_t i = 0; i < nS; ++i)
        if (final_flag[i])
            fin_w[i] = final_weight[i];
    const size_t f_fiw = put(floats, fin_w.data(), nS);

    AMX_TRY(h->d_ints.reserve(ints.size() + 1));
    AMX_TRY(h->d_floats.reserve(floats.size() + 1));
    AMX_TRY(h->d_arc_offsets.reserve(nS + 1));
    AMX_TRY(h->d_final_flag.reserve(nS));
    AMX_TRY(h->d_walk.reserve(p.walk.size()));
    AMX_TRY(h->d_seg.reserve(p.seg.size()));
    AMX_TRY(h->d_pot.reserve(nN + 3 * (size_t)n_seg));
    AMX_TRY(h->d_work.reserve(nN + 2 * (size_t)n_seg));
    AMX_HIP(hipMemcpyAsync(h->d_ints.get(), ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_floats.get(), floats.data(), floats.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_arc_offsets.get(), arc_offsets, (nS + 1) * sizeof(long), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_final_flag.get(), final_flag, nS, hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_walk.get(), p.walk.data(), p.walk.size() * sizeof(amx::LatWalk), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_seg.get(), p.seg.data(), p.seg.size() * sizeof(amx::LatBestSeg), hipMemcpyHostToDevice, ctx->stream));
    h->last_plan_ms   = std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->last_upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();

    amx::LatBestArgs a{};
    a.walk = h->d_walk.get(), a.seg = h->d_seg.get();
    const int32_t* di = h->d_ints.get();
    const float*   df = h->d_floats.get();
    a.node_arcs = di + i_node_arcs, a.node_final = di + i_node_final, a.warc_peer = di + i_peer, a.warc_arc = di + i_warc, a.order = di + i_order;
    a.levels = di + i_levels, a.arc_source = di + i_src, a.arc_target = di + i_tgt, a.state_seg = di + i_sseg, a.disc_arc = di + i_disc;
    a.wide_state = di + i_wide, a.reached = di + i_reached;
    a.node_fw = df + f_fw, a.warc_weight = df + f_ww, a.arc_weight = df + f_aw, a.final_weight = df + f_fiw;
    a.final_flag = h->d_final_flag.get(), a.arc_offsets = h->d_arc_offsets.get();
    a.pot = h->d_pot.get(), a.ends = h->d_pot.get() + nN;
    a.reach = h->d_work.get(), a.counts = h->d_work.get() + nN;
    a.best_arc = best_arc_dev, a.path = path_dev, a.keep = keep_dev, a.kept_index = kept_index_dev;
    a.n_arcs = p.n_arcs, a.n_states = p.n_states, a.n_seg = n_seg, a.n_wide = (int)p.wide_state.size();
    a.relative = h->cfg.relative ? 1 : 0, a.trim = h->cfg.trim ? 1 : 0, a.threshold = h->cfg.threshold;
    a.prune        = h->cfg.threshold < FLT_MAX;   // Lattice::prune (Lattice/Posterior.cc:116)
    a.force_global = h->cfg.potentials == AMX_LATPOST_POTENTIALS_GLOBAL;
    const dim3 walks(2 * (unsigned)n_seg), segs((unsigned)n_seg);
    {
        amx::ScopedKernelTimer timer(ctx, "latbest_potentials");
        hipLaunchKernelGGL(amx::latbest_potentials_kernel, walks, dim3(amx::kLatBestThreads), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(ctx, "latbest_arc");
        hipLaunchKernelGGL(amx::latbest_arc_kernel, dim3((unsigned)amx::ceil_div(p.n_states, 256)), dim3(256), 0, ctx->stream, a);
        if (a.n_wide)
            hipLaunchKernelGGL(amx::latbest_arc_wide_kernel, dim3((unsigned)a.n_wide), dim3(64), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(ctx, "latbest_path");
        hipLaunchKernelGGL(amx::latbest_path_kernel, dim3((unsigned)amx::ceil_div(n_seg, 64)), dim3(64), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(ctx, "latbest_min");
        hipLaunchKernelGGL(amx::latbest_min_kernel, segs, dim3(64), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    if (p.n_arcs) {
        amx::ScopedKernelTimer timer(ctx, "latbest_keep");
        hipLaunchKernelGGL(amx::latbest_keep_kernel, dim3((unsigned)amx::ceil_div(p.n_arcs, 256)), dim3(256), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    if (a.trim) {
        amx::ScopedKernelTimer timer(ctx, "latbest_trim");
        hipLaunchKernelGGL(amx::latbest_trim_kernel, walks, dim3(amx::kLatBestThreads), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(ctx, "latbest_scan");
        hipLaunchKernelGGL(amx::latbest_scan_kernel, segs, dim3(amx::kLatBestThreads), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    std::vector<float>   ends(3 * (size_t)n_seg);
    std::vector<int32_t> counts(2 * (size_t)n_seg);
    AMX_HIP(hipMemcpyAsync(ends.data(), a.ends, ends.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipMemcpyAsync(counts.data(), a.counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));   // the call's one synchronisation: info, and the uploads' host copies go away
    if (info)
        for (int g = 0; g < n_seg; ++g) {
            info[g]                      = p.info[(size_t)g];
            info[g].best_score           = ends[3 * (size_t)g];
            info[g].min_weight           = ends[3 * (size_t)g + 1];
            info[g].min_weight_threshold = ends[3 * (size_t)g + 2];
            info[g].path_length          = counts[2 * (size_t)g];
            info[g].kept_arcs            = counts[2 * (size_t)g + 1];
        }
    h->last_seg    = std::move(p.seg);
    h->last_nodes  = p.n_nodes;
    h->last_states = p.n_states;
    return AMX_OK;
}

int amx_latbest_last_timing(const amx_latbest* h, double* plan_ms, double* upload_ms) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_latbest_last_timing: NULL handle");
    if (plan_ms)
        *plan_ms = h->last_plan_ms;
    if (upload_ms)
        *upload_ms = h->last_upload_ms;
    return AMX_OK;
}

int amx_latbest_last_potentials(const amx_latbest* h, long n_states, float* forward, float* backward) {
    const char* who = "amx_latbest_last_potentials";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(!h->last_seg.empty() && n_states == h->last_states, AMX_ERR_INVALID, "%s: %ld states, the last call had %ld", who, n_states, h->last_states);
    AMX_HIP(hipSetDevice(h->ctx->device));
    std::vector<float> pot((size_t)h->last_nodes);
    AMX_HIP(hipMemcpy(pot.data(), h->d_pot.get(), pot.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (const amx::LatBestSeg& g : h->last_seg)
        for (int s = 0; s < g.n_states; ++s) {
            const size_t i = (size_t)g.state0 + (size_t)s;
            if (forward)
                forward[i] = pot[(size_t)g.node_fwd + s];
            if (backward)
                backward[i] = pot[(size_t)g.node_bwd + s];
        }
    return AMX_OK;
}

}  // extern "C"
