// latword_plan.hpp -- the host plan of the lattice word measures (amx_latword_*): what latword_host.cpp builds and latword.hip uploads.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/amx.h"

namespace amx {

// frames a wave takes (one per lane) and records it stages per trip; the number of records from which a row's blocks get lists of the
// records that touch them; the duration from which an arc is taken by a wave instead of a lane.  Chosen, not tuned.
constexpr int kLwBlockFrames = 64;
constexpr int kLwListArcs    = 256;
constexpr int kLwWaveFrames  = 128;

// a reached arc with start < end, as the collector is fed with it
struct LwRec {
    int start, end, arc;   // arc: counted over the call
};
// a (segment, label): its records [rec0, rec0 + n_rec) in discover order, the frames [lo, hi) they span, and its row of the table:
// hi - lo + 1 cells from cell0
struct LwRow {
    int       rec0, n_rec, lo, hi, seg, label;
    long long cell0;
};
// a wave's work: the frames [f0, f0 + 64) of a row.  n_list < 0: it walks all of the row's records; otherwise the records
// rec0 + list[list0 + i], which a ballot pass has found to touch the block (the host only counts them)
struct LwUnit {
    int row, f0, list0, n_list;
};
// an interval of a segment's approximate-word table, sorted by (start, end, label); maxend: the largest end up to and including it
struct LwInterval {
    int start, end, label, maxend;
};

// the rows of one set of lattices (the hypotheses, or the correct lattices)
struct LwTable {
    std::vector<LwRec>     rec;
    std::vector<LwRow>     row;
    std::vector<int>       seg_row;    // [n_seg + 1]: a segment's rows, ascending by label
    std::vector<LwUnit>    unit;
    std::vector<int>       wide_unit;  // the units with a list
    long long              n_cells = 0, n_list = 0;
};

struct LwPlan {
    int  n_seg = 0;
    long n_states = 0, n_arcs = 0;
    LwTable               hyp, ref;    // ref: FRAME_WORD_ACCURACY only
    std::vector<int32_t>  arc_start, arc_end, arc_row;   // per arc of the hypotheses; arc_row: see latword.hip
    std::vector<int32_t>  long_arc;    // arcs of kLwWaveFrames frames and more
    std::vector<LwInterval> interval;  // APPROXIMATE_WORD
    std::vector<int>      seg_interval;   // [n_seg + 1]
    std::vector<int>      arc_seg;     // [n_arcs]
    std::vector<amx_latword_info> info;
};

enum { kLwArcUnreached = -2, kLwArcNoRow = -1 };

int latword_plan(const amx_latword_cfg& cfg, const amx_latword_lattices* lat, const amx_latword_lattices* correct, const int32_t* short_pause_label,
                 int n_short_pause, const char* who, LwPlan* out);

}  // namespace amx
