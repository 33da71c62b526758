// latpost_plan.hpp -- the plan of the lattice arc posteriors (amx_latpost_*): what latpost_host.cpp builds and latpost.hip uploads, and
// what latplan.hip builds on the device instead (amx_latpost_cfg.plan).
#pragma once
#include <cstdint>
#include <vector>

#include "common.hpp"

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

// what the two kernels of latpost.hip read: the walk tables of a plan (the host's, uploaded, or the device's) and the call's own tables
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

// ---- the device plan (latplan.hip): a workgroup per lattice builds the same tables from the raw CSR tables.
// Bases follow from the offsets alone, so no segment waits for another: a segment of n states and m arcs whose first state is s0 and
// whose first arc is a0 owns 2n + 3 nodes (each walk keeps an end entry of its own in node_arcs), m + n forward and m backward walk
// arcs, and 2(n + 2) + 1 level entries per walk.
struct LatPlanBases {
    int node_fwd, node_bwd, warc_fwd, warc_bwd, level_fwd, level_bwd;
};
__host__ __device__ inline LatPlanBases latplan_bases(int g, long s0, int n, long a0, long m) {
    LatPlanBases b;
    b.node_fwd  = (int)(2 * s0 + 3 * (long)g);
    b.node_bwd  = b.node_fwd + n + 2;
    b.warc_fwd  = (int)(2 * a0 + s0);
    b.warc_bwd  = b.warc_fwd + (int)m + n;
    b.level_fwd = (int)(4 * s0 + 10 * (long)g);
    b.level_bwd = b.level_fwd + 2 * n + 5;
    return b;
}

// the buffers of a handle's device plans and what the last one read back
struct LatDevPlan {
    DevBuf<int32_t> ints;
    DevBuf<float>   floats;
    DevBuf<long>    offsets;      // state_offsets [n_seg + 1], arc_offsets [n_states + 1]
    DevBuf<uint8_t> final_flag;
    DevBuf<LatWalk> walk;
    DevBuf<LatSeg>  seg;
    long n_states = 0, n_arcs = 0, n_nodes = 0;
    int  n_seg = 0;
    std::vector<LatSeg>  h_seg;    // [n_seg]
    std::vector<int32_t> h_info;   // [8 x n_seg]: reason, states_reached, arcs_reached, states_coreached, undefined_states, undefined_arcs,
                                   // levels_forward, levels_backward
    // the plan's own outputs on the device, per state (in_off: n + 1 entries per segment from s0 + g, local to the segment; in_arc: from a0)
    int32_t *discover_index = nullptr, *level_backward = nullptr, *level_forward = nullptr, *level_super = nullptr, *final_order = nullptr,
            *in_off = nullptr, *in_arc = nullptr;
    double plan_ms = 0, upload_ms = 0;
};

// Uploads the raw tables, builds on the device every table LatArgs reads and sets those pointers and sizes in *args (pot, gen, ends, the
// outputs and the configuration's switches are the caller's).  One stream synchronisation.  Whatever the device refuses, the host plan
// refuses again with its own status and text; a loop that met its bound: AMX_ERR_DEVICE.
int latplan_run(amx_ctx* ctx, int mode, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target,
                const float* arc_weight, const float* arc_risk, const int32_t* initial, const uint8_t* final_flag, const float* final_weight,
                const float* final_risk, const char* who, LatDevPlan* plan, LatArgs* args);
// info's discrete fields of the last plan, the rest zero
void latplan_info(const LatDevPlan& plan, amx_latpost_info* info);
// amx_latpost_plan_dev's outputs from the last plan: copied back and laid out as the host plan lays them out (every output nullable)
int latplan_download(amx_ctx* ctx, const LatDevPlan& plan, const long* state_offsets, const long* arc_offsets, int32_t* discover_index,
                     int32_t* level_backward, int32_t* level_forward, int32_t* level_super, long* in_offsets, int32_t* in_arc, int32_t* final_order,
                     amx_latpost_info* info);

}  // namespace amx
