// latpost.hip -- lattice arc posteriors on the device: Fsa::posterior64 / Fsa::posteriorE (Fsa/Sssp.cc:95-375) for a batch of lattices.
//
// latpost_potentials_kernel  one workgroup per (segment, direction): the backward pass walks the automaton, the forward pass its transpose
//                            (latpost_host.cpp has built both as lists of nodes by level).  Levels ascend with one barrier between them; a
//                            node's potential is ONE chain over its arcs in the reference's order: a lane takes a node, or a wave shares a
//                            node of kLatWaveArcs arcs or more -- its lanes compute the scores and the exp terms, the chain adds them in
//                            arc order.  The expectation pair (potential, generalized) rides in the same chain.  Potentials live in LDS
//                            while the walk's nodes fit (kLatLdsStates), in global memory otherwise; the arithmetic is the same.
// latpost_arcs_kernel        one thread per input arc and one per state: logPosterior, the f32 cap, expm or the risk product.
// No floating-point atomics, no tree sums: a segment's bits depend on the segment alone.
#include <cfloat>
#include <chrono>

#include "common.hpp"
#include "latpost_plan.hpp"

namespace amx {

constexpr int    kLatThreads   = 256;
constexpr int    kLatLdsStates = 4096;   // x 8 bytes (x 2 with the generalized potentials): 32 / 64 KB of LDS
constexpr double kLatZero      = DBL_MAX;   // Fsa/Sssp.cc:67

struct LatArgs {
    const LatWalk* walk;
    const LatSeg*  seg;
    const int32_t *node_arcs, *node_final, *warc_target, *order, *levels, *arc_source, *arc_target, *state_seg;
    const float *  node_fw, *node_fr, *warc_weight, *warc_risk, *arc_weight, *arc_risk, *final_weight, *final_risk;
    const uint8_t* final_flag;
    const long*    arc_offsets;
    double *       pot, *gen;   // [n_nodes] each
    double*        ends;        // [3 x n_seg]: bw[initial], fw[new initial], gbw[initial]
    float *        arc_out, *final_out;
    long           n_arcs, n_states;
    int            n_seg, mode, normalize, v_normalized, force_global;
};

__device__ __forceinline__ double lat_score(double potential, float w) {
    double s = potential + (double)w;
    return isinf(s) ? DBL_MAX : s;
}
// std::min(a, b) / std::max(a, b) as the reference calls them (a NaN in `a` stays)
__device__ __forceinline__ double lat_min(double a, double b) {
    return b < a ? b : a;
}
__device__ __forceinline__ double lat_max(double a, double b) {
    return a < b ? b : a;
}

// ---- a node taken by one lane

__device__ void lat_node_serial64(const LatArgs& a, int a0, int a1, bool fin, float fw, const double* pot, double* result) {
    double mn = fin ? (double)fw : kLatZero;
    int    mi = -1;
    for (int k = a0; k < a1; ++k) {
        const double score = lat_score(pot[a.warc_target[k]], a.warc_weight[k]);
        if (score <= mn)
            mn = score, mi = k;
    }
    double sum = (fin && mi >= 0) ? exp(mn - (double)fw) : 0.0;
    for (int k = a0; k < a1; ++k)
        if (k != mi)
            sum += exp(mn - lat_score(pot[a.warc_target[k]], a.warc_weight[k]));
    const double r = mn - log1p(sum);
    *result        = r < kLatZero ? r : kLatZero;
}

template<bool FMA>
__device__ void lat_node_serialE(const LatArgs& a, int a0, int a1, bool fin, float fw, float fr, const double* pot, const double* gen, double* rp, double* rg) {
    double mn = fin ? (double)fw : kLatZero;
    for (int k = a0; k < a1; ++k) {
        const double w = lat_score(pot[a.warc_target[k]], a.warc_weight[k]);
        if (mn > w)
            mn = w;
    }
    double den = fin ? exp(mn - (double)fw) : 0.0;
    double num = fin ? (double)fr * den : 0.0;
    for (int k = a0; k < a1; ++k) {
        const int    t = a.warc_target[k];
        const double p = exp(mn - lat_score(pot[t], a.warc_weight[k]));
        num            = mad<FMA>(p, (double)a.warc_risk[k] + gen[t], num);
        den += p;
    }
    if (den > 0) {
        *rp = lat_min(mn - log1p(den - 1), kLatZero);
        *rg = lat_max(lat_min(num / den, kLatZero), -kLatZero);
    }
}

// ---- a node shared by a wave: every lane ends with the same result

__device__ void lat_node_wave64(const LatArgs& a, int a0, int a1, bool fin, float fw, const double* pot, double* result) {
    const int lane = threadIdx.x & 63;
    // the last minimal arc: per lane over its own arcs, then across the lanes (comparisons only)
    double mn = INFINITY;   // above every score, which lat_score keeps at or below f64 max
    int    mi = -1;
    for (int k = a0 + lane; k < a1; k += 64) {
        const double score = lat_score(pot[a.warc_target[k]], a.warc_weight[k]);
        if (score <= mn)
            mn = score, mi = k;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double om = __shfl_xor(mn, d);
        const int    oi = __shfl_xor(mi, d);
        if (om < mn || (om == mn && oi > mi))
            mn = om, mi = oi;
    }
    const double start = fin ? (double)fw : kLatZero;
    if (!(mn <= start))
        mn = start, mi = -1;
    double sum = (fin && mi >= 0) ? exp(mn - (double)fw) : 0.0;
    for (int c = a0; c < a1; c += 64) {
        const int    k = c + lane;
        const double t = k < a1 ? exp(mn - lat_score(pot[a.warc_target[k]], a.warc_weight[k])) : 0.0;
        const int    m = a1 - c < 64 ? a1 - c : 64;
        for (int j = 0; j < m; ++j) {
            const double tj = __shfl(t, j);
            if (c + j != mi)
                sum += tj;
        }
    }
    const double r = mn - log1p(sum);
    *result        = r < kLatZero ? r : kLatZero;
}

template<bool FMA>
__device__ void lat_node_waveE(const LatArgs& a, int a0, int a1, bool fin, float fw, float fr, const double* pot, const double* gen, double* rp, double* rg,
                               bool* written) {
    const int lane = threadIdx.x & 63;
    double    mn   = INFINITY;
    for (int k = a0 + lane; k < a1; k += 64) {
        const double w = lat_score(pot[a.warc_target[k]], a.warc_weight[k]);
        if (mn > w)
            mn = w;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double om = __shfl_xor(mn, d);
        if (mn > om)
            mn = om;
    }
    const double start = fin ? (double)fw : kLatZero;
    if (!(start > mn))
        mn = start;
    double den = fin ? exp(mn - (double)fw) : 0.0;
    double num = fin ? (double)fr * den : 0.0;
    for (int c = a0; c < a1; c += 64) {
        const int k = c + lane;
        double    p = 0.0, rg_k = 0.0;
        if (k < a1) {
            const int t = a.warc_target[k];
            p           = exp(mn - lat_score(pot[t], a.warc_weight[k]));
            rg_k        = (double)a.warc_risk[k] + gen[t];
        }
        const int m = a1 - c < 64 ? a1 - c : 64;
        for (int j = 0; j < m; ++j) {
            const double pj = __shfl(p, j);
            num             = mad<FMA>(pj, __shfl(rg_k, j), num);
            den += pj;
        }
    }
    *written = den > 0;
    if (den > 0) {
        *rp = lat_min(mn - log1p(den - 1), kLatZero);
        *rg = lat_max(lat_min(num / den, kLatZero), -kLatZero);
    }
}

template<bool E, bool FMA>
__global__ __launch_bounds__(kLatThreads) void latpost_potentials_kernel(LatArgs a) {
    __shared__ double lds[(E ? 2 : 1) * kLatLdsStates];
    const LatWalk w      = a.walk[blockIdx.x];
    const bool    in_lds = !a.force_global && w.n_nodes <= kLatLdsStates;
    double*       pot    = in_lds ? lds : a.pot + w.node_base;
    double*       gen    = E ? (in_lds ? lds + kLatLdsStates : a.gen + w.node_base) : nullptr;
    const int     tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < w.n_nodes; i += kLatThreads) {
        pot[i] = kLatZero;   // where a walk does not come (and potentials_.grow(s, Zero))
        if (E)
            gen[i] = 0.0;    // generalized_.grow(s, 0)
    }
    __syncthreads();
    const int32_t* order  = a.order + w.order_base;
    const int32_t* levels = a.levels + w.level_base;
    const int32_t* narcs  = a.node_arcs + w.node_base;
    for (int l = 0; l < w.n_levels; ++l) {
        const int b = levels[2 * l], wb = levels[2 * l + 1], e = levels[2 * l + 2];
        for (int i = b + tid; i < wb; i += kLatThreads) {
            const int  v   = order[i];
            const bool fin = a.node_final[w.node_base + v] != 0;
            if (E) {
                double rp = pot[v], rg = gen[v];
                lat_node_serialE<FMA>(a, narcs[v], narcs[v + 1], fin, a.node_fw[w.node_base + v], a.node_fr[w.node_base + v], pot, gen, &rp, &rg);
                pot[v] = rp, gen[v] = rg;
            }
            else {
                double r;
                lat_node_serial64(a, narcs[v], narcs[v + 1], fin, a.node_fw[w.node_base + v], pot, &r);
                pot[v] = r;
            }
        }
        for (int i = wb + wave; i < e; i += kLatThreads / 64) {
            const int  v   = order[i];
            const bool fin = a.node_final[w.node_base + v] != 0;
            if (E) {
                double rp = 0, rg = 0;
                bool   written = false;
                lat_node_waveE<FMA>(a, narcs[v], narcs[v + 1], fin, a.node_fw[w.node_base + v], a.node_fr[w.node_base + v], pot, gen, &rp, &rg, &written);
                if (lane == 0 && written)
                    pot[v] = rp, gen[v] = rg;
            }
            else {
                double r;
                lat_node_wave64(a, narcs[v], narcs[v + 1], fin, a.node_fw[w.node_base + v], pot, &r);
                if (lane == 0)
                    pot[v] = r;
            }
        }
        __syncthreads();   // a level's potentials (LDS or global, written by this workgroup) before the next level reads them
    }
    if (in_lds)
        for (int i = tid; i < w.n_nodes; i += kLatThreads) {
            a.pot[w.node_base + i] = pot[i];
            if (E)
                a.gen[w.node_base + i] = gen[i];
        }
}

// the f32 cap of logPosterior, finalLogPosterior, risk and finalRisk (Sssp.cc:158, :164, :307, :313)
__device__ __forceinline__ float lat_cap(double v) {
    return v < (double)FLT_MAX ? (float)v : FLT_MAX;
}
// Fsa::expm (Fsa/Arithmetic.cc:47-50): exp resolves to the f64 overload, Weight(double) narrows
__device__ __forceinline__ float lat_expm(float w) {
    return isinf(w) ? 0.f : (float)exp(-(double)w);
}

__global__ __launch_bounds__(256) void latpost_arcs_kernel(LatArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_arcs) {
        const int     s   = a.arc_source[i];
        const LatSeg  g   = a.seg[a.state_seg[s]];
        const bool    e   = a.mode == AMX_LATPOST_EXPECTATION;
        const float   dead = a.mode == AMX_LATPOST_LOG ? FLT_MAX : 0.f;
        float         out = dead;
        if (!g.dead) {
            const int    ls = s - g.state0, t = a.arc_target[i];
            const double bw_initial = a.pot[g.node_bwd + g.initial];
            const double total_inv  = (e || a.normalize) ? -bw_initial : 0.0;
            const float  lp         = lat_cap(a.pot[g.node_fwd + ls] + (double)a.arc_weight[i] + a.pot[g.node_bwd + t] + total_inv);
            if (a.mode == AMX_LATPOST_LOG)
                out = lp;
            else if (a.mode == AMX_LATPOST_PROB)
                out = lat_expm(lp);
            else {
                const double normalization = a.v_normalized ? a.gen[g.node_bwd + g.initial] : 0.0;
                const float  risk          = lat_cap(a.gen[g.node_fwd + ls] + (double)a.arc_risk[i] + a.gen[g.node_bwd + t] - normalization);
                out                        = (float)(exp(-(double)lp) * (double)risk);
            }
        }
        a.arc_out[i] = out;
    }
    if (i < a.n_states) {
        const LatSeg g    = a.seg[a.state_seg[i]];
        const bool   e    = a.mode == AMX_LATPOST_EXPECTATION;
        const float  dead = a.mode == AMX_LATPOST_LOG ? FLT_MAX : 0.f;
        float        out  = dead;
        if (!g.dead && a.final_flag[i]) {
            const int    ls         = (int)i - g.state0;
            const bool   no_arcs    = a.arc_offsets[i + 1] == a.arc_offsets[i];
            const double bw_initial = a.pot[g.node_bwd + g.initial];
            const double total_inv  = (e || a.normalize) ? -bw_initial : 0.0;
            const float  lp         = no_arcs ? 0.f : lat_cap(a.pot[g.node_fwd + ls] + (double)a.final_weight[i] + total_inv);
            if (a.mode == AMX_LATPOST_LOG)
                out = lp;
            else if (a.mode == AMX_LATPOST_PROB)
                out = lat_expm(lp);
            else {
                const double normalization = a.v_normalized ? a.gen[g.node_bwd + g.initial] : 0.0;
                const float  risk          = no_arcs ? 0.f : lat_cap((double)a.final_risk[i] - normalization);
                out                        = (float)(exp(-(double)lp) * (double)risk);
            }
        }
        a.final_out[i] = out;
    }
    if (i < a.n_seg) {
        const LatSeg g    = a.seg[i];
        a.ends[3 * i]     = a.pot[g.node_bwd + g.initial];
        a.ends[3 * i + 1] = a.pot[g.node_fwd + g.n_states];
        a.ends[3 * i + 2] = a.mode == AMX_LATPOST_EXPECTATION ? a.gen[g.node_bwd + g.initial] : 0.0;
    }
}

}  // namespace amx

struct amx_latpost {
    amx_ctx*        ctx = nullptr;
    amx_latpost_cfg cfg{};
    amx::DevBuf<int32_t> d_ints;
    amx::DevBuf<float>   d_floats;
    amx::DevBuf<long>    d_arc_offsets;
    amx::DevBuf<uint8_t> d_final_flag;
    amx::DevBuf<amx::LatWalk> d_walk;
    amx::DevBuf<amx::LatSeg>  d_seg;
    amx::DevBuf<double>       d_pot;   // [2 x n_nodes + 3 x n_seg]: potentials, generalized potentials, the segments' ends
    std::vector<amx::LatSeg>  last_seg;
    long                      last_nodes = 0, last_states = 0;
    int                       last_mode  = 0;
    double                    last_plan_ms = 0, last_upload_ms = 0;   // host wall time of the last call's plan and of its uploads
};

namespace amx {
const amx_latpost_cfg& latpost_cfg_of(const amx_latpost* h) {
    return h->cfg;
}
}  // namespace amx

extern "C" {

int amx_latpost_create(amx_ctx* ctx, const amx_latpost_cfg* cfg, amx_latpost** out) {
    const char* who = "amx_latpost_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    amx_latpost_cfg c;
    amx_latpost_cfg_default(&c);
    if (cfg)
        c = *cfg;
    AMX_REQUIRE(c.mode == AMX_LATPOST_LOG || c.mode == AMX_LATPOST_PROB || c.mode == AMX_LATPOST_EXPECTATION, AMX_ERR_INVALID, "%s: mode %d", who, c.mode);
    // Core::isAlmostEqualUlp's own requirements (Core/Utility.hh:384-388)
    AMX_REQUIRE(c.tolerance > 0 && c.tolerance < 0x400000, AMX_ERR_INVALID, "%s: tolerance %d must lie in (0, 2^22)", who, c.tolerance);
    AMX_REQUIRE(c.potentials == AMX_LATPOST_POTENTIALS_AUTO || c.potentials == AMX_LATPOST_POTENTIALS_GLOBAL, AMX_ERR_INVALID, "%s: potentials %d", who,
                c.potentials);
    std::unique_ptr<amx_latpost> h(new amx_latpost);
    h->ctx = ctx;
    h->cfg = c;
    *out   = h.release();
    return AMX_OK;
}

void amx_latpost_destroy(amx_latpost* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

void amx_latpost_kernel_shape(int* threads, int* lds_states, int* wave_arcs) {
    if (threads)
        *threads = amx::kLatThreads;
    if (lds_states)
        *lds_states = amx::kLatLdsStates;
    if (wave_arcs)
        *wave_arcs = amx::kLatWaveArcs;
}

int amx_latpost_run_dev(amx_latpost* h, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target, const float* arc_weight,
                        const float* arc_risk, const int32_t* initial, const uint8_t* final_flag, const float* final_weight, const float* final_risk,
                        float* arc_out_dev, float* final_out_dev, amx_latpost_info* info) {
    const char* who = "amx_latpost_run_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    amx::LatPlan p;
    const auto   t0 = std::chrono::steady_clock::now();
    AMX_TRY(amx::latpost_plan(h->cfg.mode, n_seg, state_offsets, arc_offsets, arc_target, arc_weight, arc_risk, initial, final_flag, final_weight, final_risk,
                              who, &p));
    const auto t1 = std::chrono::steady_clock::now();
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(final_out_dev && (p.n_arcs == 0 || arc_out_dev), AMX_ERR_INVALID, "%s: NULL arc_out_dev or final_out_dev", who);
    amx_ctx*   ctx = h->ctx;
    const bool e   = h->cfg.mode == AMX_LATPOST_EXPECTATION;
    AMX_HIP(hipSetDevice(ctx->device));
    h->last_seg.clear();

    // one table of 32-bit integers and one of floats, uploaded once per call
    std::vector<int32_t> ints;
    std::vector<float>   floats;
    auto put = [](auto& table, const auto* v, size_t n) {
        const size_t at = table.size();
        table.insert(table.end(), v, v + n);
        return at;
    };
    const size_t nA = (size_t)p.n_arcs, nS = (size_t)p.n_states;
    const size_t i_node_arcs = put(ints, p.node_arcs.data(), p.node_arcs.size()), i_node_final = put(ints, p.node_final.data(), p.node_final.size());
    const size_t i_warc = put(ints, p.warc_target.data(), p.warc_target.size()), i_order = put(ints, p.order.data(), p.order.size());
    const size_t i_levels = put(ints, p.levels.data(), p.levels.size()), i_src = put(ints, p.arc_source.data(), nA);
    const size_t i_tgt = put(ints, arc_target, nA), i_sseg = put(ints, p.state_seg.data(), nS);
    const size_t f_fw = put(floats, p.node_fw.data(), p.node_fw.size()), f_fr = put(floats, p.node_fr.data(), p.node_fr.size());
    const size_t f_ww = put(floats, p.warc_weight.data(), p.warc_weight.size()), f_wr = put(floats, p.warc_risk.data(), p.warc_risk.size());
    const size_t f_aw = put(floats, arc_weight, nA), f_ar = e ? put(floats, arc_risk, nA) : 0;
    std::vector<float> fin_w(nS, 0.f), fin_r(nS, 0.f);   // read only where the flag is set: unset entries may be anything, NaN included
    for (size_t i = 0; i < nS; ++i)
        if (final_flag[i])
            fin_w[i] = final_weight[i], fin_r[i] = e ? final_risk[i] : 0.f;
    const size_t f_fiw = put(floats, fin_w.data(), nS), f_fir = put(floats, fin_r.data(), nS);

    const size_t nN = (size_t)p.n_nodes;
    AMX_TRY(h->d_ints.reserve(ints.size() + 1));
    AMX_TRY(h->d_floats.reserve(floats.size() + 1));
    AMX_TRY(h->d_arc_offsets.reserve(nS + 1));
    AMX_TRY(h->d_final_flag.reserve(nS));
    AMX_TRY(h->d_walk.reserve(p.walk.size()));
    AMX_TRY(h->d_seg.reserve(p.seg.size()));
    AMX_TRY(h->d_pot.reserve(2 * nN + 3 * (size_t)n_seg));
    AMX_HIP(hipMemcpyAsync(h->d_ints.get(), ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_floats.get(), floats.data(), floats.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_arc_offsets.get(), arc_offsets, (nS + 1) * sizeof(long), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_final_flag.get(), final_flag, nS, hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_walk.get(), p.walk.data(), p.walk.size() * sizeof(amx::LatWalk), hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->d_seg.get(), p.seg.data(), p.seg.size() * sizeof(amx::LatSeg), hipMemcpyHostToDevice, ctx->stream));
    // the uploads read pageable host memory of this call: wait before the vectors go away (the runtime stages them, but not all at once)
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    h->last_plan_ms   = std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->last_upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();

    amx::LatArgs a{};
    a.walk = h->d_walk.get(), a.seg = h->d_seg.get();
    const int32_t* di = h->d_ints.get();
    const float*   df = h->d_floats.get();
    a.node_arcs = di + i_node_arcs, a.node_final = di + i_node_final, a.warc_target = di + i_warc, a.order = di + i_order, a.levels = di + i_levels;
    a.arc_source = di + i_src, a.arc_target = di + i_tgt, a.state_seg = di + i_sseg;
    a.node_fw = df + f_fw, a.node_fr = df + f_fr, a.warc_weight = df + f_ww, a.warc_risk = df + f_wr, a.arc_weight = df + f_aw, a.arc_risk = df + f_ar;
    a.final_weight = df + f_fiw, a.final_risk = df + f_fir;
    a.final_flag = h->d_final_flag.get(), a.arc_offsets = h->d_arc_offsets.get();
    a.pot = h->d_pot.get(), a.gen = h->d_pot.get() + nN, a.ends = h->d_pot.get() + 2 * nN;
    a.arc_out = arc_out_dev, a.final_out = final_out_dev;
    a.n_arcs = p.n_arcs, a.n_states = p.n_states, a.n_seg = n_seg;
    a.mode = h->cfg.mode, a.normalize = h->cfg.normalize ? 1 : 0, a.v_normalized = h->cfg.v_normalized ? 1 : 0;
    a.force_global = h->cfg.potentials == AMX_LATPOST_POTENTIALS_GLOBAL;
    if (!e)
        AMX_HIP(hipMemsetAsync(a.gen, 0, nN * sizeof(double), ctx->stream));
    {
        amx::ScopedKernelTimer timer(ctx, "latpost_potentials");
        const dim3             grid(2 * (unsigned)n_seg), block(amx::kLatThreads);
        if (!e)
            hipLaunchKernelGGL((amx::latpost_potentials_kernel<false, false>), grid, block, 0, ctx->stream, a);
        else if (ctx->contract == AMX_CONTRACT_FMA)
            hipLaunchKernelGGL((amx::latpost_potentials_kernel<true, true>), grid, block, 0, ctx->stream, a);
        else
            hipLaunchKernelGGL((amx::latpost_potentials_kernel<true, false>), grid, block, 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(ctx, "latpost_arcs");
        long                   most = p.n_arcs > p.n_states ? p.n_arcs : p.n_states;
        if (most < n_seg)
            most = n_seg;
        hipLaunchKernelGGL(amx::latpost_arcs_kernel, dim3((unsigned)amx::ceil_div(most, 256)), dim3(256), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    std::vector<double> ends(3 * (size_t)n_seg);
    AMX_HIP(hipMemcpyAsync(ends.data(), a.ends, ends.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    if (info)
        for (int g = 0; g < n_seg; ++g) {
            info[g] = p.info[(size_t)g];
            amx::latpost_fill_info(h->cfg, ends[3 * (size_t)g], ends[3 * (size_t)g + 1], ends[3 * (size_t)g + 2], &info[g]);
        }
    h->last_seg    = std::move(p.seg);
    h->last_nodes  = p.n_nodes;
    h->last_states = p.n_states;
    h->last_mode   = h->cfg.mode;
    return AMX_OK;
}

int amx_latpost_last_timing(const amx_latpost* h, double* plan_ms, double* upload_ms) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_latpost_last_timing: NULL handle");
    if (plan_ms)
        *plan_ms = h->last_plan_ms;
    if (upload_ms)
        *upload_ms = h->last_upload_ms;
    return AMX_OK;
}

int amx_latpost_last_potentials(const amx_latpost* h, long n_states, double* forward, double* backward, double* generalized_forward,
                                double* generalized_backward) {
    const char* who = "amx_latpost_last_potentials";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(!h->last_seg.empty() && n_states == h->last_states, AMX_ERR_INVALID, "%s: %ld states, the last call had %ld", who, n_states, h->last_states);
    AMX_HIP(hipSetDevice(h->ctx->device));
    std::vector<double> all(2 * (size_t)h->last_nodes);
    AMX_HIP(hipMemcpy(all.data(), h->d_pot.get(), all.size() * sizeof(double), hipMemcpyDeviceToHost));
    const double* pot = all.data();
    const double* gen = all.data() + h->last_nodes;
    for (const amx::LatSeg& g : h->last_seg)
        for (int s = 0; s < g.n_states; ++s) {
            const size_t i = (size_t)g.state0 + (size_t)s;
            if (forward)
                forward[i] = pot[g.node_fwd + s];
            if (backward)
                backward[i] = pot[g.node_bwd + s];
            if (generalized_forward)
                generalized_forward[i] = gen[g.node_fwd + s];
            if (generalized_backward)
                generalized_backward[i] = gen[g.node_bwd + s];
        }
    return AMX_OK;
}

}  // extern "C"
