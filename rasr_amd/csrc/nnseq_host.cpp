// nnseq_host.cpp -- sequence-discriminative NN training, host side (no device): the row plan of a batch of segments, the checks of a
// call's host tables, the key layout and the workspace sizes of the collection's sort, and the decoding of the device's refusal word.
// tests/host_nnseq_test.cc compiles this file into a program of its own.
#include "nnseq_plan.hpp"

#include <algorithm>

namespace amx {

int nnseq_plan_rows(const char* who, int n_seg, const long* frame_offsets, SeqPlan* out) {
    AMX_REQUIRE(frame_offsets && out, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(n_seg >= 1, AMX_ERR_INVALID, "%s: n_seg = %d", who, n_seg);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: frame_offsets[0] is negative", who);
    long long rows = 0;
    for (int s = 0; s < n_seg; ++s) {
        AMX_REQUIRE(frame_offsets[s + 1] >= frame_offsets[s], AMX_ERR_INVALID, "%s: frame_offsets do not ascend at segment %d", who, s);
        const long long len = (long long)frame_offsets[s + 1] - frame_offsets[s];
        AMX_REQUIRE(len <= AMX_NNTRAIN_MAX_FRAMES, AMX_ERR_INVALID, "%s: segment %d has %lld frames, more than the cap of %d frames per call", who, s, len,
                    AMX_NNTRAIN_MAX_FRAMES);
        rows += (len + AMX_NNTRAIN_CHUNK - 1) / AMX_NNTRAIN_CHUNK * AMX_NNTRAIN_CHUNK;
        AMX_REQUIRE(rows <= AMX_NNTRAIN_MAX_FRAMES, AMX_ERR_INVALID,
                    "%s: the segments' lengths, each padded to a multiple of %d, add up to more than the cap of %d frames per call at segment %d: split the batch",
                    who, AMX_NNTRAIN_CHUNK, AMX_NNTRAIN_MAX_FRAMES, s);
    }
    AMX_REQUIRE(frame_offsets[n_seg] < (1ll << 31), AMX_ERR_INVALID, "%s: frame_offsets[n_seg] = %ld (rows of feats_dev are 32-bit indices)", who, frame_offsets[n_seg]);
    out->rows = (int)rows, out->f0 = frame_offsets[0];
    out->row0.assign((size_t)n_seg + 1, 0);
    out->len.assign((size_t)n_seg, 0);
    out->row_src.assign((size_t)rows, -1);
    out->row_seg.assign((size_t)rows, 0);
    for (int s = 0, r = 0; s < n_seg; ++s) {
        const int len = (int)(frame_offsets[s + 1] - frame_offsets[s]);
        out->row0[s]  = r;
        out->len[s]   = len;
        for (int i = 0; i < len; ++i)
            out->row_src[(size_t)r + i] = frame_offsets[s] + i;
        const int padded = (len + AMX_NNTRAIN_CHUNK - 1) / AMX_NNTRAIN_CHUNK * AMX_NNTRAIN_CHUNK;
        for (int i = 0; i < padded; ++i)
            out->row_seg[(size_t)r + i] = s;
        r += padded;
        out->row0[s + 1] = r;
    }
    return AMX_OK;
}

int nnseq_check_tables(const char* who, int n_seg, const long* arc_off, const long* item_off, const int32_t* item_frame, const int32_t* item_emission,
                       long long* n_arcs, long long* n_items) {
    AMX_REQUIRE(arc_off && item_off, AMX_ERR_INVALID, "%s: arc_offsets or item_offsets is NULL", who);
    AMX_REQUIRE(arc_off[0] == 0, AMX_ERR_INVALID, "%s: arc_offsets[0] = %ld, must be 0", who, arc_off[0]);
    for (int s = 0; s < n_seg; ++s)
        AMX_REQUIRE(arc_off[s + 1] >= arc_off[s], AMX_ERR_INVALID, "%s: arc_offsets do not ascend at segment %d", who, s);
    *n_arcs = arc_off[n_seg];
    AMX_REQUIRE(*n_arcs < kSeqMaxItems, AMX_ERR_INVALID, "%s: %lld arcs (at most 2^27 - 1 per call)", who, *n_arcs);
    AMX_REQUIRE(item_off[0] == 0, AMX_ERR_INVALID, "%s: item_offsets[0] = %ld, must be 0", who, item_off[0]);
    for (long long a = 0; a < *n_arcs; ++a)
        AMX_REQUIRE(item_off[a + 1] >= item_off[a], AMX_ERR_INVALID, "%s: item_offsets do not ascend at arc %lld", who, a);
    *n_items = item_off[*n_arcs];
    AMX_REQUIRE(*n_items < kSeqMaxItems, AMX_ERR_INVALID, "%s: %lld items (at most 2^27 - 1 per call)", who, *n_items);
    AMX_REQUIRE(*n_items == 0 || (item_frame && item_emission), AMX_ERR_INVALID, "%s: item_frame or item_emission is NULL", who);
    return AMX_OK;
}

int nnseq_bit_length(long long v) {
    int b = 1;
    while ((v >> b) != 0)
        ++b;
    return b;
}

void nnseq_key_layout(int rows, int n_outputs, int* out_bits, unsigned long long* sentinel, int* bits) {
    *out_bits = nnseq_bit_length(n_outputs - 1);
    *sentinel = (unsigned long long)rows << *out_bits;
    *bits     = nnseq_bit_length((long long)*sentinel);
}

size_t nnseq_scan_ws(long long n) {
    size_t total = 0;
    while (n > 1) {
        n = (n + kSeqBlock - 1) / kSeqBlock;
        total += (size_t)n;
    }
    return total + 1;
}

size_t nnseq_part_size(int rows, int n_layers, const int* Pin, const int* Pout) {
    size_t part = 1;
    for (int l = 0; l < n_layers; ++l)
        part = std::max(part, (size_t)(rows / AMX_NNTRAIN_CHUNK) * Pin[l] * Pout[l]);
    return part;
}

namespace {
const char* bad_kind(int kind) {
    switch (kind) {
        case SEQ_BAD_FRAME: return "the frame lies outside its segment";
        case SEQ_BAD_EMISSION: return "the emission is no class of the network or a disregarded one";
        case SEQ_BAD_WEIGHT: return "the arc weight is not finite";
        case SEQ_BAD_LABEL: return "the label is out of range or of a disregarded class";
        case SEQ_BAD_CELL: return "the error signal at the alignment is negative under the frame rejection test";
    }
    return "unknown";
}
}  // namespace

int nnseq_report_bad(const char* who, unsigned long long bad) {
    if (bad == ~0ull)
        return AMX_OK;
    const int       stage = (int)(bad >> 48), kind = (int)(bad & 7);
    const long long index = (long long)((bad >> 3) & ((1ull << 45) - 1ull));
    const char*     what  = kind == SEQ_BAD_WEIGHT ? "arc" : kind == SEQ_BAD_LABEL ? "frame" : kind == SEQ_BAD_CELL ? "workspace row" : "item";
    if (stage == 0)
        set_error("%s: %s %lld: %s", who, what, index, bad_kind(kind));
    else
        set_error("%s: pass %d: %s %lld: %s", who, stage - 1, what, index, bad_kind(kind));
    return AMX_ERR_INVALID;
}

}  // namespace amx
