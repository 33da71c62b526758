// latbest_host.cpp -- lattice best path and forward-backward pruning, host side: the plan of a call (amx_latbest_plan_host needs no
// device) and amx_latbest_compact.
//
// The checks, the discover order and the transposed arc lists are latpost_plan's.  What this plan adds is the ORDER of the tropical
// chains (Fsa/tSssp.cc:150-227, Fsa/tSort.cc:226-272):
//   topological order  topologicallySort runs DfsState::dfs (the stack walk latpost_host.cpp describes) and numbers the states by
//                      descending finishing time: a gray state on top of the stack turns black and FINISHES.  TopologicalSsspQueue hands
//                      out the queued state with the smallest number, so in an acyclic automaton every state is dequeued once, after all
//                      of its sources, and the arcs that reach a state relax it in the order (number of the source, arc order within it).
//   forward chains     per reached state, its incoming arcs from reached sources in that order.
//   backward chains    the same on transpose(f): the walk starts at the new initial state, whose arcs (the final weights) therefore relax
//                      the final states before anything else; a transposed state's arcs stand in latpost_plan's in_arc order.  Per state
//                      the chain is: its final weight (if final), then its outgoing arcs ordered by (transposed number of the target,
//                      the state's own arc order).
//   levels             a chain needs the potentials of its other ends: level = 1 + the largest level among them.
// Everything is linear in states + arcs.
#include <cfloat>

#include "common.hpp"
#include "latbest_plan.hpp"

namespace amx {

namespace {
// DfsState::dfs on `n` nodes from `start`; arcs(node, push) calls push(target) per arc in arc order.  finish[i] = i-th node to finish.
template<class Arcs>
void stack_walk(int n, int start, Arcs&& arcs, std::vector<int32_t>& color, std::vector<int32_t>& stack, std::vector<int32_t>& finish) {
    color.assign((size_t)n, 0), stack.clear(), finish.clear();
    stack.push_back(start);
    while (!stack.empty()) {
        const int s = stack.back();
        if (color[(size_t)s] == 0) {
            color[(size_t)s] = 1;
            arcs(s, [&](int t) {
                if (color[(size_t)t] == 0)
                    stack.push_back(t);
            });
        }
        else {
            if (color[(size_t)s] == 1)
                color[(size_t)s] = 2, finish.push_back(s);
            stack.pop_back();
        }
    }
}
}  // namespace

int latbest_plan(int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target, const float* arc_weight,
                 const int32_t* initial, const uint8_t* final_flag, const float* final_weight, const char* who, LatBestPlan* out) {
    LatPlan lp;
    AMX_TRY(latpost_plan(AMX_LATPOST_LOG, n_seg, state_offsets, arc_offsets, arc_target, arc_weight, nullptr, initial, final_flag, final_weight, nullptr,
                         who, &lp));
    LatBestPlan& p = *out;
    p              = LatBestPlan();
    p.n_seg = n_seg, p.n_states = lp.n_states, p.n_arcs = lp.n_arcs;
    const size_t nS = (size_t)p.n_states;
    p.seg.resize((size_t)n_seg), p.walk.resize(2 * (size_t)n_seg), p.info.assign((size_t)n_seg, amx_latbest_info{});
    p.arc_source = lp.arc_source, p.state_seg = lp.state_seg, p.discover_index = lp.discover_index;
    p.topo_forward.assign(nS, -1), p.topo_backward.assign(nS, -1), p.level_forward.assign(nS, -1), p.level_backward.assign(nS, -1);
    p.topo_super.assign((size_t)n_seg, -1);
    p.node_arcs.push_back(0);

    std::vector<int32_t> color, stack, finish, discover, fill, bucket;
    for (int g = 0; g < n_seg; ++g) {
        const long s0  = state_offsets[g];
        const int  n   = (int)(state_offsets[g + 1] - s0);
        const int  ini = initial[g];
        const long a0 = arc_offsets[s0], a1 = arc_offsets[s0 + n];
        const bool dead = lp.info[(size_t)g].reason == AMX_LATPOST_NO_FINAL;
        // ---- the discover order (latpost_plan's) as a list, and the arcs in that order
        discover.assign((size_t)lp.info[(size_t)g].states_reached, -1);
        for (int s = 0; s < n; ++s)
            if (lp.discover_index[(size_t)(s0 + s)] >= 0)
                discover[(size_t)lp.discover_index[(size_t)(s0 + s)]] = s;
        LatBestSeg& sg = p.seg[(size_t)g];
        sg.state0 = (int)s0, sg.n_states = n, sg.initial = ini, sg.dead = dead, sg.arc0 = (int)a0, sg.n_arcs = (int)(a1 - a0);
        sg.disc_base = (int)p.disc_arc.size();
        for (int u : discover)
            for (long a = arc_offsets[s0 + u]; a < arc_offsets[s0 + u + 1]; ++a)
                p.disc_arc.push_back((int32_t)a);
        sg.n_disc = (int)p.disc_arc.size() - sg.disc_base;
        // ---- topologicallySort(f): numbers by descending finishing time
        stack_walk(
                n, ini,
                [&](int s, auto push) {
                    for (long a = arc_offsets[s0 + s]; a < arc_offsets[s0 + s + 1]; ++a)
                        push(arc_target[a]);
                },
                color, stack, finish);
        const int n_reached = (int)finish.size();
        std::vector<int32_t> by_fwd((size_t)n_reached);
        for (int i = 0; i < n_reached; ++i) {
            p.topo_forward[(size_t)(s0 + finish[(size_t)i])] = n_reached - 1 - i;
            by_fwd[(size_t)(n_reached - 1 - i)]                = finish[(size_t)i];
        }
        // ---- topologicallySort(transpose(f)): node n is the new initial state
        std::vector<int32_t> by_bwd;
        if (!dead) {
            stack_walk(
                    n + 1, n,
                    [&](int t, auto push) {
                        if (t == n) {
                            for (int k = 0; k < n && lp.final_order[(size_t)(s0 + k)] >= 0; ++k)
                                push(lp.final_order[(size_t)(s0 + k)]);
                        }
                        else
                            for (long k = lp.in_offsets[(size_t)(s0 + t)]; k < lp.in_offsets[(size_t)(s0 + t + 1)]; ++k)
                                push((int)(lp.arc_source[(size_t)lp.in_arc[(size_t)k]] - s0));
                    },
                    color, stack, finish);
            const int m = (int)finish.size();
            by_bwd.resize((size_t)m);
            for (int i = 0; i < m; ++i) {
                const int v = finish[(size_t)i];
                by_bwd[(size_t)(m - 1 - i)] = v;
                (v == n ? p.topo_super[(size_t)g] : p.topo_backward[(size_t)(s0 + v)]) = m - 1 - i;
            }
        }
        amx_latbest_info& info = p.info[(size_t)g];
        info.reason            = dead ? AMX_LATBEST_NO_FINAL : AMX_LATBEST_OK;
        info.total_arcs        = sg.n_arcs;
        info.states_reached    = n_reached;
        info.states_coreached  = dead ? 0 : (int)by_bwd.size() - 1;

        // ---- the two walks
        for (int dir = 0; dir < 2; ++dir) {
            const std::vector<int32_t>& topo = dir == 0 ? by_fwd : by_bwd;
            std::vector<int32_t>&       lvl  = dir == 0 ? p.level_forward : p.level_backward;
            LatWalk&                    w    = p.walk[2 * (size_t)g + dir];
            w.node_base  = (int)p.node_final.size();
            w.n_nodes    = n;
            w.order_base = (int)p.order.size();
            w.level_base = (int)p.levels.size();
            w.pad        = 0;
            (dir == 0 ? sg.node_fwd : sg.node_bwd) = w.node_base;
            if (n > p.max_nodes)
                p.max_nodes = n;
            // a chain's arcs: walk the other ends in topological order, append each of their arcs to the chain of the state it relaxes
            fill.assign((size_t)n + 1, 0);
            auto each = [&](auto&& f) {
                for (int u : topo) {
                    if (u == n)
                        continue;   // the new initial state's arcs are node_final / node_fw
                    if (dir == 0)
                        for (long a = arc_offsets[s0 + u]; a < arc_offsets[s0 + u + 1]; ++a)
                            f(arc_target[a], u, a);
                    else
                        for (long k = lp.in_offsets[(size_t)(s0 + u)]; k < lp.in_offsets[(size_t)(s0 + u + 1)]; ++k) {
                            const long a = lp.in_arc[(size_t)k];
                            f((int)(lp.arc_source[(size_t)a] - s0), u, a);
                        }
                }
            };
            each([&](int v, int, long) { ++fill[(size_t)v + 1]; });
            for (int v = 0; v < n; ++v)
                fill[(size_t)v + 1] += fill[(size_t)v];
            const size_t base = p.warc_peer.size();
            p.warc_peer.resize(base + (size_t)fill[(size_t)n]), p.warc_arc.resize(base + (size_t)fill[(size_t)n]);
            p.warc_weight.resize(base + (size_t)fill[(size_t)n]);
            for (int v = 0; v < n; ++v) {
                const bool fin = dir == 1 && !dead && final_flag[s0 + v] && p.topo_backward[(size_t)(s0 + v)] >= 0;
                p.node_final.push_back(fin), p.node_fw.push_back(fin ? final_weight[s0 + v] : 0.f);
                p.node_arcs.push_back((int32_t)(base + (size_t)fill[(size_t)v + 1]));
            }
            // levels ride along: the other end's level is final when its arcs are appended
            for (int u : topo)
                if (u != n)
                    lvl[(size_t)(s0 + u)] = 0;
            int n_levels = topo.empty() ? 0 : 1;
            each([&](int v, int u, long a) {
                const size_t at = base + (size_t)fill[(size_t)v]++;
                p.warc_peer[at] = u, p.warc_arc[at] = (int32_t)a, p.warc_weight[at] = arc_weight[a];
                if (lvl[(size_t)(s0 + v)] < lvl[(size_t)(s0 + u)] + 1)
                    lvl[(size_t)(s0 + v)] = lvl[(size_t)(s0 + u)] + 1;
                if (lvl[(size_t)(s0 + v)] + 1 > n_levels)
                    n_levels = lvl[(size_t)(s0 + v)] + 1;
            });
            w.n_levels = n_levels;
            (dir == 0 ? info.levels_forward : info.levels_backward) = n_levels;
            // nodes by level (a counting sort), a level's wave-shared nodes behind its lane-taken ones, each group by ascending id
            const int L = n_levels;
            bucket.assign(2 * (size_t)L + 1, 0);
            auto wide_of = [&](int v) { return p.node_arcs[(size_t)w.node_base + v + 1] - p.node_arcs[(size_t)w.node_base + v] >= kLatWaveArcs; };
            for (int v = 0; v < n; ++v)
                if (lvl[(size_t)(s0 + v)] >= 0)
                    ++bucket[2 * (size_t)lvl[(size_t)(s0 + v)] + wide_of(v) + 1];
            for (size_t i = 0; i < 2 * (size_t)L; ++i)
                bucket[i + 1] += bucket[i];
            for (size_t i = 0; i <= 2 * (size_t)L; ++i)
                p.levels.push_back(bucket[i]);
            p.order.resize((size_t)w.order_base + (size_t)bucket[2 * (size_t)L]);
            for (int v = 0; v < n; ++v)
                if (lvl[(size_t)(s0 + v)] >= 0)
                    p.order[(size_t)w.order_base + (size_t)bucket[2 * (size_t)lvl[(size_t)(s0 + v)] + wide_of(v)]++] = v;
        }
        if (!dead)
            for (int u : discover)
                if (arc_offsets[s0 + u + 1] - arc_offsets[s0 + u] >= kLatWaveArcs)
                    p.wide_state.push_back((int32_t)(s0 + u));
    }
    p.n_nodes     = (long)p.node_final.size();
    p.n_walk_arcs = (long)p.warc_peer.size();
    return AMX_OK;
}

}  // namespace amx

extern "C" {

void amx_latbest_cfg_default(amx_latbest_cfg* cfg) {
    if (!cfg)
        return;
    cfg->threshold  = FLT_MAX;   // Lattice::prune: nothing is pruned
    cfg->relative   = 1;
    cfg->trim       = 0;
    cfg->potentials = AMX_LATPOST_POTENTIALS_AUTO;
}

int amx_latbest_plan_host(const amx_latbest* h, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target,
                          const float* arc_weight, const int32_t* initial, const uint8_t* final_flag, const float* final_weight,
                          int32_t* discover_index, int32_t* topo_forward, int32_t* topo_backward, int32_t* topo_super, int32_t* level_forward,
                          int32_t* level_backward, amx_latbest_info* info) {
    const char* who = "amx_latbest_plan_host";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    amx::LatBestPlan p;
    AMX_TRY(amx::latbest_plan(n_seg, state_offsets, arc_offsets, arc_target, arc_weight, initial, final_flag, final_weight, who, &p));
    auto copy = [](auto* dst, const auto& v) {
        if (dst && !v.empty())
            std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
    };
    copy(discover_index, p.discover_index), copy(topo_forward, p.topo_forward), copy(topo_backward, p.topo_backward), copy(topo_super, p.topo_super);
    copy(level_forward, p.level_forward), copy(level_backward, p.level_backward), copy(info, p.info);
    return AMX_OK;
}

int amx_latbest_compact(int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target, const float* arc_weight,
                        const uint8_t* keep, long* out_arc_offsets, int32_t* out_arc_target, float* out_arc_weight, int32_t* old_to_new,
                        long* n_kept) {
    const char* who = "amx_latbest_compact";
    AMX_REQUIRE(n_seg >= 0, AMX_ERR_INVALID, "%s: n_seg %d", who, n_seg);
    AMX_REQUIRE(state_offsets && arc_offsets && out_arc_offsets, AMX_ERR_INVALID, "%s: NULL state_offsets, arc_offsets or out_arc_offsets", who);
    AMX_REQUIRE(state_offsets[0] == 0 && arc_offsets[0] == 0, AMX_ERR_INVALID, "%s: state_offsets[0] and arc_offsets[0] must be 0", who);
    for (int g = 0; g < n_seg; ++g)
        AMX_REQUIRE(state_offsets[g + 1] >= state_offsets[g], AMX_ERR_INVALID, "%s: state_offsets descend at segment %d", who, g);
    const long n_states = state_offsets[n_seg];
    for (long i = 0; i < n_states; ++i)
        AMX_REQUIRE(arc_offsets[i + 1] >= arc_offsets[i], AMX_ERR_INVALID, "%s: arc_offsets descend at state %ld", who, i);
    const long n_arcs = arc_offsets[n_states];
    AMX_REQUIRE(n_arcs < (1l << 30), AMX_ERR_UNSUPPORTED, "%s: %ld arcs in one call are above the limit", who, n_arcs);
    AMX_REQUIRE(n_arcs == 0 || (arc_target && arc_weight && keep && out_arc_target && out_arc_weight), AMX_ERR_INVALID, "%s: NULL arc table, keep or output", who);
    long k = 0;
    out_arc_offsets[0] = 0;
    for (long i = 0; i < n_states; ++i) {
        for (long a = arc_offsets[i]; a < arc_offsets[i + 1]; ++a) {
            if (old_to_new)
                old_to_new[a] = keep[a] ? (int32_t)k : -1;
            if (keep[a])
                out_arc_target[k] = arc_target[a], out_arc_weight[k] = arc_weight[a], ++k;
        }
        out_arc_offsets[i + 1] = k;
    }
    if (n_kept)
        *n_kept = k;
    return AMX_OK;
}

}  // extern "C"
