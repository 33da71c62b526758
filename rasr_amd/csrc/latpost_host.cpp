// latpost_host.cpp -- lattice arc posteriors, host side: the checks and the plan of a call (amx_latpost_plan_host needs no device).
//
// The plan restates what the reference's walks decide before any arithmetic happens (Fsa/tDfs.cc:21-68, Fsa/tRational.cc:594-689):
//   discover order  DfsState::dfs keeps a stack of state ids; the top is looked at: a white state turns gray, is DISCOVERED, and every
//                   target that is white at that moment is pushed, in arc order (a state can lie on the stack several times); a gray
//                   state turns black and is popped, a black one is popped.
//   transpose       discoverState appends, for every arc s -> t of the discovered state, an arc t -> s to t's list: a transposed state's
//                   arcs stand in discover order of their sources and, within a source, in the source's arc order.  The final states, in
//                   discover order, become the arcs of a new initial state; the old initial state becomes final with weight one.
//   levels          a state's potential needs its targets' (backward) or its sources' (forward): level = 1 + the largest level among
//                   them, 0 without any.  The order in which the reference's walk finishes states does not enter a value.
// Everything is linear in states + arcs.
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "latpost_plan.hpp"

namespace amx {

namespace {
constexpr float kF32Min = -3.40282347e+38F, kF32Epsilon = 1.19209290e-07F, kF32Delta = 1.17549435e-38F;

// Core::differenceUlp(f32, f32) (Core/Utility.cc:61-73), the s32 arithmetic wrapping as the reference's does on its hosts
int32_t difference_ulp(float af, float bf) {
    int32_t a, b;
    std::memcpy(&a, &af, 4), std::memcpy(&b, &bf, 4);
    if (a < 0)
        a = (int32_t)(0x80000000u - (uint32_t)a);
    if (b < 0)
        b = (int32_t)(0x80000000u - (uint32_t)b);
    const int32_t d = (int32_t)((uint32_t)a - (uint32_t)b);
    return d < 0 ? (int32_t)(0u - (uint32_t)d) : d;
}
bool almost_equal_ulp(float a, float b, int tolerance) {
    return difference_ulp(a, b) <= tolerance;
}
// Core::isAlmostEqual(f32, f32, f32) (Core/Utility.hh:316-321)
bool almost_equal(float a, float b, float tolerance) {
    const float d = std::fabs(a - b);
    const float e = (std::fabs(a) + std::fabs(b) + kF32Delta) * kF32Epsilon * tolerance;
    return d < e;
}
}  // namespace

void latpost_fill_info(const amx_latpost_cfg& cfg, double bw_initial, double fw_super, double gbw_initial, amx_latpost_info* info) {
    const bool e        = cfg.mode == AMX_LATPOST_EXPECTATION;
    info->total_inv     = -bw_initial;
    info->total_inv_f32 = e ? (float)info->total_inv : (info->total_inv > kF32Min ? (float)info->total_inv : kF32Min);
    info->expectation   = e ? (float)gbw_initial : 0.f;
    info->forward_flow  = (float)fw_super;
    info->backward_flow = (float)bw_initial;
    info->flows_agree   = e ? almost_equal_ulp(info->forward_flow, info->backward_flow, cfg.tolerance)
                            : almost_equal(info->forward_flow, info->backward_flow, (float)cfg.tolerance);
    info->vanishing_flow = almost_equal_ulp(info->total_inv_f32, kF32Min, cfg.tolerance);
}

int latpost_plan(int mode, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target, const float* arc_weight,
                 const float* arc_risk, const int32_t* initial, const uint8_t* final_flag, const float* final_weight, const float* final_risk,
                 const char* who, LatPlan* out) {
    const bool expectation = mode == AMX_LATPOST_EXPECTATION;
    AMX_REQUIRE(n_seg >= 0, AMX_ERR_INVALID, "%s: n_seg %d", who, n_seg);
    AMX_REQUIRE(state_offsets && arc_offsets, AMX_ERR_INVALID, "%s: NULL state_offsets or arc_offsets", who);
    AMX_REQUIRE(state_offsets[0] == 0 && arc_offsets[0] == 0, AMX_ERR_INVALID, "%s: state_offsets[0] and arc_offsets[0] must be 0", who);
    for (int g = 0; g < n_seg; ++g)
        AMX_REQUIRE(state_offsets[g + 1] >= state_offsets[g], AMX_ERR_INVALID, "%s: state_offsets descend at segment %d", who, g);
    const long n_states = state_offsets[n_seg];
    for (long i = 0; i < n_states; ++i)
        AMX_REQUIRE(arc_offsets[i + 1] >= arc_offsets[i], AMX_ERR_INVALID, "%s: arc_offsets descend at state %ld", who, i);
    const long n_arcs = arc_offsets[n_states];
    AMX_REQUIRE(2 * n_states + 2 * n_arcs + 2 * (long)n_seg < (1l << 30), AMX_ERR_UNSUPPORTED, "%s: %ld states and %ld arcs in one call are above the limit",
                who, n_states, n_arcs);
    AMX_REQUIRE(n_states == 0 || (initial && final_flag), AMX_ERR_INVALID, "%s: NULL initial or final_flag", who);
    AMX_REQUIRE(n_arcs == 0 || (arc_target && arc_weight), AMX_ERR_INVALID, "%s: NULL arc_target or arc_weight", who);
    AMX_REQUIRE(!expectation || ((n_arcs == 0 || arc_risk) && (n_states == 0 || final_risk)), AMX_ERR_INVALID,
                "%s: mode EXPECTATION needs arc_risk and final_risk", who);

    LatPlan& p = *out;
    p          = LatPlan();
    p.n_seg = n_seg, p.n_states = n_states, p.n_arcs = n_arcs;
    p.seg.resize((size_t)n_seg), p.walk.resize(2 * (size_t)n_seg), p.info.assign((size_t)n_seg, amx_latpost_info{});
    p.arc_source.resize((size_t)n_arcs), p.state_seg.resize((size_t)n_states);
    p.discover_index.assign((size_t)n_states, -1), p.level_backward.assign((size_t)n_states, -1), p.level_forward.assign((size_t)n_states, -1);
    p.level_super.assign((size_t)n_seg, -1), p.final_order.assign((size_t)n_states, -1);
    p.in_offsets.assign((size_t)n_states + 1, 0), p.in_arc.clear();
    p.node_arcs.push_back(0);

    std::vector<int32_t> stack, discover, topo, indegree, color, in_fill, bucket;
    std::vector<uint8_t> coreached;
    for (int g = 0; g < n_seg; ++g) {
        const long s0 = state_offsets[g];
        const int  n  = (int)(state_offsets[g + 1] - s0);
        // ---- checks, in the order the refusals are documented
        AMX_REQUIRE(n >= 1, AMX_ERR_INVALID, "%s: segment %d has no state", who, g);
        AMX_REQUIRE(initial[g] >= 0 && initial[g] < n, AMX_ERR_INVALID, "%s: segment %d: initial state %d outside its %d states", who, g, initial[g], n);
        for (int s = 0; s < n; ++s) {
            if (final_flag[s0 + s]) {
                AMX_REQUIRE(final_weight && final_weight[s0 + s] == final_weight[s0 + s], AMX_ERR_INVALID, "%s: segment %d: final weight of state %d is not a number",
                            who, g, s);
                AMX_REQUIRE(!expectation || final_risk[s0 + s] == final_risk[s0 + s], AMX_ERR_INVALID, "%s: segment %d: final risk of state %d is not a number", who,
                            g, s);
            }
            for (long a = arc_offsets[s0 + s]; a < arc_offsets[s0 + s + 1]; ++a) {
                AMX_REQUIRE(arc_target[a] >= 0 && arc_target[a] < n, AMX_ERR_INVALID, "%s: segment %d: arc %ld of state %d has target %d outside its %d states", who,
                            g, a - arc_offsets[s0 + s], s, arc_target[a], n);
                AMX_REQUIRE(arc_weight[a] == arc_weight[a], AMX_ERR_INVALID, "%s: segment %d: weight of arc %ld of state %d is not a number", who, g,
                            a - arc_offsets[s0 + s], s);
                AMX_REQUIRE(!expectation || arc_risk[a] == arc_risk[a], AMX_ERR_INVALID, "%s: segment %d: risk of arc %ld of state %d is not a number", who, g,
                            a - arc_offsets[s0 + s], s);
            }
        }
        // ---- a topological order of ALL states (sources first); what it cannot place lies on or behind a cycle
        indegree.assign((size_t)n, 0), topo.clear();
        for (long a = arc_offsets[s0]; a < arc_offsets[s0 + n]; ++a)
            ++indegree[(size_t)arc_target[a]];
        for (int s = 0; s < n; ++s)
            if (!indegree[(size_t)s])
                topo.push_back(s);
        for (size_t i = 0; i < topo.size(); ++i)
            for (long a = arc_offsets[s0 + topo[i]]; a < arc_offsets[s0 + topo[i] + 1]; ++a)
                if (--indegree[(size_t)arc_target[a]] == 0)
                    topo.push_back(arc_target[a]);
        if ((int)topo.size() != n) {
            // walk backwards among the unplaced states (each has an unplaced source) until one repeats: that one is on a cycle
            int s = 0;
            while (!indegree[(size_t)s])
                ++s;
            color.assign((size_t)n, 0);
            for (;;) {
                if (color[(size_t)s])
                    break;
                color[(size_t)s] = 1;
                int next         = -1;
                for (int u = 0; u < n && next < 0; ++u)
                    if (indegree[(size_t)u])
                        for (long a = arc_offsets[s0 + u]; a < arc_offsets[s0 + u + 1]; ++a)
                            if (arc_target[a] == s) {
                                next = u;
                                break;
                            }
                s = next;
            }
            set_error("%s: segment %d: state %d lies on a cycle (the lattice must be acyclic)", who, g, s);
            return AMX_ERR_INVALID;
        }
        // ---- DfsState::dfs, operation by operation: the discover order
        color.assign((size_t)n, 0), stack.clear(), discover.clear();
        stack.push_back(initial[g]);
        while (!stack.empty()) {
            const int s = stack.back();
            if (color[(size_t)s] == 0) {
                color[(size_t)s] = 1;
                p.discover_index[(size_t)(s0 + s)] = (int32_t)discover.size();
                discover.push_back(s);
                for (long a = arc_offsets[s0 + s]; a < arc_offsets[s0 + s + 1]; ++a)
                    if (color[(size_t)arc_target[a]] == 0)
                        stack.push_back(arc_target[a]);
            }
            else {
                if (color[(size_t)s] == 1)
                    color[(size_t)s] = 2;
                stack.pop_back();
            }
        }
        amx_latpost_info& info = p.info[(size_t)g];
        info.states_reached    = (int)discover.size();
        // ---- backward levels and co-reachability, targets first
        coreached.assign((size_t)n, 0);
        int max_back = -1, n_final = 0;
        for (int i = n - 1; i >= 0; --i) {
            const int s = topo[(size_t)i];
            if (!color[(size_t)s])
                continue;
            int  level = 0;
            bool co    = final_flag[s0 + s] != 0;
            for (long a = arc_offsets[s0 + s]; a < arc_offsets[s0 + s + 1]; ++a) {
                const int t = arc_target[a];
                if (p.level_backward[(size_t)(s0 + t)] + 1 > level)
                    level = p.level_backward[(size_t)(s0 + t)] + 1;
                co = co || coreached[(size_t)t];
            }
            p.level_backward[(size_t)(s0 + s)] = level;
            coreached[(size_t)s]               = co;
            if (level > max_back)
                max_back = level;
            info.arcs_reached += (int)(arc_offsets[s0 + s + 1] - arc_offsets[s0 + s]);
            info.states_coreached += co;
        }
        for (int s = 0; s < n; ++s)
            if (!coreached[(size_t)s]) {
                ++info.undefined_states;
                info.undefined_arcs += (int)(arc_offsets[s0 + s + 1] - arc_offsets[s0 + s]);
            }
        // ---- the transposed lists: sources in discover order, arcs in the source's order
        const size_t in_base = p.in_arc.size();
        in_fill.assign((size_t)n + 1, 0);
        for (int u : discover)
            for (long a = arc_offsets[s0 + u]; a < arc_offsets[s0 + u + 1]; ++a)
                ++in_fill[(size_t)arc_target[a] + 1];
        for (int s = 0; s < n; ++s)
            in_fill[(size_t)s + 1] += in_fill[(size_t)s];
        p.in_arc.resize(in_base + (size_t)in_fill[(size_t)n]);
        for (int s = 0; s < n; ++s)
            p.in_offsets[(size_t)(s0 + s)] = (long)in_base + in_fill[(size_t)s];
        p.in_offsets[(size_t)(s0 + n)] = (long)p.in_arc.size();
        for (int u : discover)
            for (long a = arc_offsets[s0 + u]; a < arc_offsets[s0 + u + 1]; ++a)
                p.in_arc[in_base + (size_t)in_fill[(size_t)arc_target[a]]++] = (int32_t)a;
        for (int u : discover)
            if (final_flag[s0 + u])
                p.final_order[(size_t)(s0 + n_final++)] = u;
        // ---- forward levels, sources first
        int super = -1;
        for (int s = 0; s < n; ++s) {
            p.state_seg[(size_t)(s0 + s)] = g;
            for (long a = arc_offsets[s0 + s]; a < arc_offsets[s0 + s + 1]; ++a)
                p.arc_source[(size_t)a] = (int32_t)(s0 + s);
        }
        for (int i = 0; i < n; ++i) {
            const int v = topo[(size_t)i];
            if (!coreached[(size_t)v])
                continue;
            int level = 0;
            for (long k = p.in_offsets[(size_t)(s0 + v)]; k < p.in_offsets[(size_t)(s0 + v + 1)]; ++k) {
                const int lu = p.level_forward[(size_t)p.arc_source[(size_t)p.in_arc[(size_t)k]]];
                if (lu + 1 > level)
                    level = lu + 1;
            }
            p.level_forward[(size_t)(s0 + v)] = level;
            if (final_flag[s0 + v] && level + 1 > super)
                super = level + 1;
        }
        const bool dead         = n_final == 0;
        p.level_super[(size_t)g] = dead ? -1 : super;
        info.reason             = dead ? AMX_LATPOST_NO_FINAL : AMX_LATPOST_OK;
        info.levels_forward     = dead ? 0 : super + 1;
        info.levels_backward    = max_back + 1;

        // ---- the two walks
        LatSeg& sg = p.seg[(size_t)g];
        sg.state0 = (int)s0, sg.initial = initial[g], sg.dead = dead, sg.n_states = n;
        for (int dir = 0; dir < 2; ++dir) {
            LatWalk& w   = p.walk[2 * (size_t)g + dir];
            w.node_base  = (int)p.node_final.size();
            w.n_nodes    = n + (dir == 0);
            w.order_base = (int)p.order.size();
            w.level_base = (int)p.levels.size();
            w.n_levels   = dir == 0 ? info.levels_forward : info.levels_backward;
            w.pad        = 0;
            (dir == 0 ? sg.node_fwd : sg.node_bwd) = w.node_base;
            if (w.n_nodes > p.max_nodes)
                p.max_nodes = w.n_nodes;
            for (int v = 0; v < w.n_nodes; ++v) {
                bool  fin = false;
                float fw = 0.f, fr = 0.f;
                if (dir == 1 && color[(size_t)v]) {
                    for (long a = arc_offsets[s0 + v]; a < arc_offsets[s0 + v + 1]; ++a) {
                        p.warc_target.push_back(arc_target[a]), p.warc_weight.push_back(arc_weight[a]);
                        p.warc_risk.push_back(expectation ? arc_risk[a] : 0.f);
                    }
                    if (final_flag[s0 + v])
                        fin = true, fw = final_weight[s0 + v], fr = expectation ? final_risk[s0 + v] : 0.f;
                }
                else if (dir == 0 && !dead && v == n) {
                    for (int k = 0; k < n_final; ++k) {
                        const int f = p.final_order[(size_t)(s0 + k)];
                        p.warc_target.push_back(f), p.warc_weight.push_back(final_weight[s0 + f]);
                        p.warc_risk.push_back(expectation ? final_risk[s0 + f] : 0.f);
                    }
                }
                else if (dir == 0 && !dead && v < n && coreached[(size_t)v]) {
                    for (long k = p.in_offsets[(size_t)(s0 + v)]; k < p.in_offsets[(size_t)(s0 + v + 1)]; ++k) {
                        const long a = p.in_arc[(size_t)k];
                        p.warc_target.push_back((int32_t)(p.arc_source[(size_t)a] - s0)), p.warc_weight.push_back(arc_weight[a]);
                        p.warc_risk.push_back(expectation ? arc_risk[a] : 0.f);
                    }
                    fin = v == initial[g];   // the semiring's one, in both automata
                }
                p.node_final.push_back(fin), p.node_fw.push_back(fw), p.node_fr.push_back(fr);
                p.node_arcs.push_back((int32_t)p.warc_target.size());
            }
            // nodes by level (a counting sort), a level's wave-shared nodes behind its lane-taken ones, each group by ascending id
            const int L = w.n_levels;
            bucket.assign(2 * (size_t)L + 1, 0);
            auto level_of = [&](int v) { return dir == 1 ? p.level_backward[(size_t)(s0 + v)] : (v == n ? (dead ? -1 : super) : (dead ? -1 : p.level_forward[(size_t)(s0 + v)])); };
            auto wide_of  = [&](int v) { return p.node_arcs[(size_t)w.node_base + v + 1] - p.node_arcs[(size_t)w.node_base + v] >= kLatWaveArcs; };
            for (int v = 0; v < w.n_nodes; ++v)
                if (level_of(v) >= 0)
                    ++bucket[2 * (size_t)level_of(v) + wide_of(v) + 1];
            for (size_t i = 0; i < 2 * (size_t)L; ++i)
                bucket[i + 1] += bucket[i];
            for (size_t i = 0; i <= 2 * (size_t)L; ++i)
                p.levels.push_back(bucket[i]);
            p.order.resize((size_t)w.order_base + (size_t)bucket[2 * (size_t)L]);
            for (int v = 0; v < w.n_nodes; ++v)
                if (level_of(v) >= 0)
                    p.order[(size_t)w.order_base + (size_t)bucket[2 * (size_t)level_of(v) + wide_of(v)]++] = v;
        }
    }
    p.n_nodes     = (long)p.node_final.size();
    p.n_walk_arcs = (long)p.warc_target.size();
    return AMX_OK;
}

}  // namespace amx

struct amx_latpost;
namespace amx {
const amx_latpost_cfg& latpost_cfg_of(const amx_latpost* h);
}

extern "C" {

void amx_latpost_cfg_default(amx_latpost_cfg* cfg) {
    if (!cfg)
        return;
    cfg->mode         = AMX_LATPOST_LOG;
    cfg->normalize    = 1;     // Fsa/Sssp.hh: posterior64(fsa, totalInv, tol) normalises
    cfg->v_normalized = 1;     // posteriorE's vNormalized
    cfg->tolerance    = 100;   // posterior-tolerance
    cfg->potentials   = AMX_LATPOST_POTENTIALS_AUTO;
}

int amx_latpost_plan_host(const amx_latpost* h, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target,
                          const float* arc_weight, const float* arc_risk, const int32_t* initial, const uint8_t* final_flag, const float* final_weight,
                          const float* final_risk, int32_t* discover_index, int32_t* level_backward, int32_t* level_forward, int32_t* level_super,
                          long* in_offsets, int32_t* in_arc, int32_t* final_order, amx_latpost_info* info) {
    const char* who = "amx_latpost_plan_host";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    amx::LatPlan p;
    AMX_TRY(amx::latpost_plan(amx::latpost_cfg_of(h).mode, n_seg, state_offsets, arc_offsets, arc_target, arc_weight, arc_risk, initial, final_flag,
                              final_weight, final_risk, who, &p));
    auto copy = [](auto* dst, const auto& v) {
        if (dst && !v.empty())
            std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
    };
    copy(discover_index, p.discover_index), copy(level_backward, p.level_backward), copy(level_forward, p.level_forward);
    copy(level_super, p.level_super), copy(in_offsets, p.in_offsets), copy(in_arc, p.in_arc), copy(final_order, p.final_order), copy(info, p.info);
    return AMX_OK;
}

}  // extern "C"
