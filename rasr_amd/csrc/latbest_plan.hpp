// latbest_plan.hpp -- the host plan of the lattice best path and forward-backward pruning (amx_latbest_*): what latbest_host.cpp builds
// and latbest.hip uploads.  The checks, the discover order and the transposed arc order are latpost_plan.hpp's.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "latpost_plan.hpp"

namespace amx {

// A segment of the call.  Both walks have one node per state: node_fwd + s holds fw[s], node_bwd + s holds bw[s].
struct LatBestSeg {
    int state0, n_states, initial;
    int dead;        // AMX_LATBEST_NO_FINAL
    int node_fwd, node_bwd;
    int arc0, n_arcs;          // the segment's arcs, counted over the call
    int disc_base, n_disc;     // its part of `disc_arc`
};

struct LatBestPlan {
    long n_states = 0, n_arcs = 0, n_nodes = 0, n_walk_arcs = 0;
    int  n_seg = 0, max_nodes = 0;
    std::vector<LatBestSeg> seg;        // [n_seg]
    std::vector<LatWalk>    walk;       // [2 * n_seg]: forward, backward per segment (latpost's layout: order, levels, lane / wave split)
    std::vector<int32_t>    node_arcs;  // [n_nodes + 1]
    std::vector<int32_t>    node_final; // backward nodes: the state is final (the new initial state's arc comes first in its chain)
    std::vector<float>      node_fw;    // ... with this weight
    std::vector<int32_t>    warc_peer;  // the chain's arcs in the order the topological queue hands them out: the other end, id within the segment
    std::vector<int32_t>    warc_arc;   // ... and the input arc, counted over the call
    std::vector<float>      warc_weight;
    std::vector<int32_t>    order, levels;
    std::vector<int32_t>    arc_source;  // [n_arcs]: state counted over the call
    std::vector<int32_t>    state_seg;   // [n_states]
    std::vector<int32_t>    disc_arc;    // the arcs of the discovered states in discover order, within a state in arc order
    std::vector<int32_t>    wide_state;  // states (over the call) with kLatWaveArcs outgoing arcs or more: their best arc is a wave's
    // what amx_latbest_plan_host hands out, per state counted over the call
    std::vector<int32_t> discover_index, topo_forward, topo_backward, level_forward, level_backward;
    std::vector<int32_t> topo_super;   // [n_seg]: the new initial state's place in the transposed order (0), -1 with NO_FINAL
    std::vector<amx_latbest_info> info;
};

// checks (latpost_plan's, the same refusals in the same order) and plans a call
int latbest_plan(int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target, const float* arc_weight,
                 const int32_t* initial, const uint8_t* final_flag, const float* final_weight, const char* who, LatBestPlan* out);

// ---- Fsa::TropicalSemiring = TropicalSemiring_(1): the tolerant comparison, integer arithmetic on the bit patterns

// Core::differenceUlp(f32, f32) (Core/Utility.cc:61-73): negative patterns are mirrored (0x80000000 - i, so -0 meets +0), the s32
// difference and its absolute value wrap as they do on the reference's hosts; infinities are the patterns next to f32 max
__host__ __device__ __forceinline__ int32_t latbest_difference_ulp(float af, float bf) {
    int32_t a, b;
#if defined(__HIP_DEVICE_COMPILE__)
    a = __float_as_int(af), b = __float_as_int(bf);
#else
    std::memcpy(&a, &af, 4), std::memcpy(&b, &bf, 4);
#endif
    if (a < 0)
        a = (int32_t)(0x80000000u - (uint32_t)a);
    if (b < 0)
        b = (int32_t)(0x80000000u - (uint32_t)b);
    const int32_t d = (int32_t)((uint32_t)a - (uint32_t)b);
    return d < 0 ? (int32_t)(0u - (uint32_t)d) : d;
}
// LogSemiring::compare (Fsa/tRealSemiring.cc:207-215) with tolerance 1
__host__ __device__ __forceinline__ int latbest_compare(float a, float b) {
    if (a == b)
        return 0;
    if (latbest_difference_ulp(a, b) <= 1)
        return 0;
    return a < b ? -1 : 1;
}
// compare(a, b) < 0: what replaces a potential (ssspLoop: compare(d, min(d, ext)) != 0), a best arc and the pruning minimum
__host__ __device__ __forceinline__ bool latbest_less(float a, float b) {
    return a < b && latbest_difference_ulp(a, b) > 1;
}

}  // namespace amx
