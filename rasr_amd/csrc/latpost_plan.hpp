// latpost_plan.hpp -- the host plan of the lattice arc posteriors (amx_latpost_*): what latpost_host.cpp builds and latpost.hip uploads.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/amx.h"

namespace amx {

// One workgroup's walk: a segment's backward pass (the automaton itself) or its forward pass (the transposed automaton, whose last node
// is the new initial state).  Nodes are the segment's states by id; a node's arcs are [node_arcs[i], node_arcs[i + 1]) of the walk-arc tables.
struct LatWalk {
    int node_base;   // first node in the node tables and in the potentials
    int n_nodes;     // states (+ 1 for the forward walk)
    int order_base;  // first entry of `order`: the walked nodes by ascending level, within a level lane-taken nodes before wave-shared ones
    int level_base;  // first entry of `levels`: per level (begin, begin of the wave-shared nodes), then the end: 2 * n_levels + 1 entries
    int n_levels;
    int pad;
};

struct LatSeg {
    int state0;      // first state, counted over the call
    int initial;     // id within the segment
    int node_fwd;    // node_base of the forward walk
    int node_bwd;    // ... of the backward walk
    int dead;        // AMX_LATPOST_NO_FINAL: every output is dead
    int n_states;
};

struct LatPlan {
    long n_states = 0, n_arcs = 0, n_nodes = 0, n_walk_arcs = 0;
    int  n_seg = 0, max_nodes = 0;
    std::vector<LatSeg>  seg;        // [n_seg]
    std::vector<LatWalk> walk;       // [2 * n_seg]: forward, backward per segment
    std::vector<int32_t> node_arcs;  // [n_nodes + 1]
    std::vector<int32_t> node_final; // [n_nodes]
    std::vector<float>   node_fw, node_fr;            // final weight and risk of a node
    std::vector<int32_t> warc_target;                 // node id within the walk
    std::vector<float>   warc_weight, warc_risk;
    std::vector<int32_t> order, levels;
    std::vector<int32_t> arc_source;  // [n_arcs]: state counted over the call
    std::vector<int32_t> state_seg;   // [n_states]
    // what amx_latpost_plan_host hands out
    std::vector<int32_t> discover_index, level_backward, level_forward, level_super, in_arc, final_order;
    std::vector<long>    in_offsets;
    std::vector<amx_latpost_info> info;
};

// the number of arcs from which a node is shared by a wave (latpost.hip reads it; the plan sorts a level's nodes by it)
constexpr int kLatWaveArcs = 128;

// checks and plans a call; AMX_ERR_INVALID (error text set) names the first offender
int latpost_plan(int mode, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target, const float* arc_weight,
                 const float* arc_risk, const int32_t* initial, const uint8_t* final_flag, const float* final_weight, const float* final_risk,
                 const char* who, LatPlan* out);

// info's fields that follow from the three potentials a segment ends with (the reference's constructors, Sssp.cc:180-192, :333-350)
void latpost_fill_info(const amx_latpost_cfg& cfg, double bw_initial, double fw_super, double gbw_initial, amx_latpost_info* info);

}  // namespace amx
