// nnseq_plan.hpp -- what nnseq.hip (device side) and nnseq_host.cpp (host side, no device) share: the row plan of a batch, the checks of
// a call's host tables, the layout of the collection's keys, the sizes of the sort's workspaces and the decoding of the device's refusal.
#pragma once
#include "common.hpp"

#include <vector>

namespace amx {

constexpr int kSeqThreads = 256;
constexpr int kSeqBlock   = 2048;              // elements of one workgroup of the sort and the scan: 8 chunks of 256
constexpr int kSeqArcs    = kSeqThreads / 64;  // arcs of one workgroup of the score kernel: one per wave
constexpr int kSeqStage   = 64;                // items a wave gathers at a time
constexpr int kSeqMaxPasses = 8;
constexpr long long kSeqMaxItems = 1ll << 27;  // arcs and items per table: positions and counts are 32-bit integers

// what went wrong first on the device: (stage << 48 | index << 3 | kind); stage 0 = labels and scores, p + 1 = pass p
enum { SEQ_BAD_FRAME = 1, SEQ_BAD_EMISSION = 2, SEQ_BAD_WEIGHT = 3, SEQ_BAD_LABEL = 4, SEQ_BAD_CELL = 5 };

// segment s owns the workspace rows [row0[s], row0[s] + len[s]); row0 a multiple of AMX_NNTRAIN_CHUNK; row_src[r]: the row of the
// features that workspace row r holds, -1 for the rows between two segments; row_seg[r]: the segment a row belongs to
struct SeqPlan {
    int                    rows = 0;
    long long              f0   = 0;
    std::vector<int>       row0, len, row_seg;
    std::vector<long long> row_src;
};
int nnseq_plan_rows(const char* who, int n_seg, const long* frame_offsets, SeqPlan* out);

// offsets of a pass's or a score call's tables: ascending from 0, one entry per segment / arc; *n_arcs, *n_items
int nnseq_check_tables(const char* who, int n_seg, const long* arc_off, const long* item_off, const int32_t* item_frame, const int32_t* item_emission,
                       long long* n_arcs, long long* n_items);

int nnseq_bit_length(long long v);  // bits that hold every value of [0, v]
// a key is row << out_bits | output; the sentinel (rows << out_bits) is larger than every key; `bits` of a code are sorted
void nnseq_key_layout(int rows, int n_outputs, int* out_bits, unsigned long long* sentinel, int* bits);
size_t nnseq_scan_ws(long long n);  // integers the scan of n integers needs for its block totals, every level
// chunk partials of the largest layer: n_chunks x Pin x Pout floats
size_t nnseq_part_size(int rows, int n_layers, const int* Pin, const int* Pout);
// AMX_OK for ~0, else the message naming the first offender and AMX_ERR_INVALID
int nnseq_report_bad(const char* who, unsigned long long bad);

}  // namespace amx
