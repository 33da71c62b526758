// Stand-alone host program for the host side of the sequence-discriminative NN training (include/amx.h): it compiles nnseq_host.cpp into a
// program of its own (no device is touched), so that tests/test_nnseq.py can run it under the host sanitizers.
//   host_nnseq_test case.bin
// case.bin (written by the test): int32 n_seg | i64 frame_offsets [n_seg + 1] | i64 arc_offsets [n_seg + 1] | i64 item_offsets [n_arcs + 1] |
// i32 item_frame, item_emission [n_items] | the restatement's i32 rows, row0 [n_seg + 1], and i64 row_src [rows].  Every array is handed
// over in a heap block of exactly its size, so that a read past an end is seen.  Then the refusals, the key layout, the sizes of the
// sort's workspaces and the decoding of the device's refusal word.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/nnseq_host.cpp"

static std::string g_error;
namespace amx {
void set_error(const char* fmt, ...) {
    char    buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace amx

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) {                                                                                             \
            printf("host_nnseq_test: line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_error.c_str());    \
            return 1;                                                                                              \
        }                                                                                                          \
    } while (0)

template<class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    v.shrink_to_fit();
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static bool says(const char* word) {
    return g_error.find(word) != std::string::npos;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: host_nnseq_test case.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    CHECK(f);
    int32_t n_seg = 0, rows = 0;
    CHECK(fread(&n_seg, 4, 1, f) == 1 && n_seg >= 1);
    std::vector<long>      frame_off, arc_off, item_off;
    std::vector<int32_t>   item_frame, item_emission, row0;
    std::vector<long long> row_src;
    CHECK(take(f, frame_off, (size_t)n_seg + 1) && take(f, arc_off, (size_t)n_seg + 1));
    CHECK(take(f, item_off, (size_t)arc_off[n_seg] + 1));
    CHECK(take(f, item_frame, (size_t)item_off[arc_off[n_seg]]) && take(f, item_emission, (size_t)item_off[arc_off[n_seg]]));
    CHECK(fread(&rows, 4, 1, f) == 1);
    CHECK(take(f, row0, (size_t)n_seg + 1) && take(f, row_src, (size_t)rows));
    fclose(f);

    // the row plan against the restatement's
    amx::SeqPlan plan;
    CHECK(amx::nnseq_plan_rows("t", n_seg, frame_off.data(), &plan) == AMX_OK);
    CHECK(plan.rows == rows && plan.f0 == frame_off[0] && plan.row0.size() == (size_t)n_seg + 1 && plan.len.size() == (size_t)n_seg);
    CHECK(plan.row_src.size() == (size_t)rows && plan.row_seg.size() == (size_t)rows);
    for (int s = 0; s <= n_seg; ++s)
        CHECK(plan.row0[s] == row0[s] && plan.row0[s] % AMX_NNTRAIN_CHUNK == 0);
    for (int r = 0; r < rows; ++r)
        CHECK(plan.row_src[r] == row_src[r]);
    for (int s = 0; s < n_seg; ++s) {
        CHECK(plan.len[s] == frame_off[s + 1] - frame_off[s]);
        for (int r = plan.row0[s]; r < plan.row0[s + 1]; ++r)
            CHECK(plan.row_seg[r] == s && (plan.row_src[r] >= 0) == (r < plan.row0[s] + plan.len[s]));
    }
    // its refusals
    {
        std::vector<long> off(18);   // 17 segments of one frame: 17 x 256 rows
        for (int i = 0; i < 18; ++i)
            off[i] = i;
        CHECK(amx::nnseq_plan_rows("t", 17, off.data(), &plan) == AMX_ERR_INVALID && says("cap of 4096 frames"));
        CHECK(amx::nnseq_plan_rows("t", 16, off.data(), &plan) == AMX_OK && plan.rows == 4096);
        std::vector<long> one = {0, 4096};
        CHECK(amx::nnseq_plan_rows("t", 1, one.data(), &plan) == AMX_OK && plan.rows == 4096 && plan.row_src[4095] == 4095);
        one[1] = 4097;
        CHECK(amx::nnseq_plan_rows("t", 1, one.data(), &plan) == AMX_ERR_INVALID && says("cap of 4096 frames"));
        one[1] = 1l << 40;   // no overflow on the way to the refusal
        CHECK(amx::nnseq_plan_rows("t", 1, one.data(), &plan) == AMX_ERR_INVALID && says("cap of 4096 frames"));
        std::vector<long> down = {0, 5, 3};
        CHECK(amx::nnseq_plan_rows("t", 2, down.data(), &plan) == AMX_ERR_INVALID && says("do not ascend"));
        std::vector<long> neg = {-1, 3};
        CHECK(amx::nnseq_plan_rows("t", 1, neg.data(), &plan) == AMX_ERR_INVALID && says("negative"));
        std::vector<long> far = {(1l << 31) - 2, (1l << 31)};
        CHECK(amx::nnseq_plan_rows("t", 1, far.data(), &plan) == AMX_ERR_INVALID && says("32-bit"));
        std::vector<long> empty = {7, 7, 7};   // segments without frames: no rows
        CHECK(amx::nnseq_plan_rows("t", 2, empty.data(), &plan) == AMX_OK && plan.rows == 0 && plan.row_src.empty() && plan.row0[2] == 0);
        CHECK(amx::nnseq_plan_rows("t", 0, empty.data(), &plan) == AMX_ERR_INVALID);
        CHECK(amx::nnseq_plan_rows("t", 1, nullptr, &plan) == AMX_ERR_INVALID);
    }

    // the tables
    long long n_arcs = -1, n_items = -1;
    CHECK(amx::nnseq_check_tables("t", n_seg, arc_off.data(), item_off.data(), item_frame.data(), item_emission.data(), &n_arcs, &n_items) == AMX_OK);
    CHECK(n_arcs == arc_off[n_seg] && n_items == (long long)item_frame.size());
    {
        std::vector<long> a = arc_off, i = item_off;
        a[0] = 1;
        CHECK(amx::nnseq_check_tables("t", n_seg, a.data(), i.data(), item_frame.data(), item_emission.data(), &n_arcs, &n_items) == AMX_ERR_INVALID && says("arc_offsets[0]"));
        a = arc_off;
        if (n_seg >= 2 && a[2] > a[1]) {
            const long keep = a[1];
            a[1] = a[2] + 1;   // descends at segment 1; the last entry, which sizes item_offsets, is untouched
            CHECK(amx::nnseq_check_tables("t", n_seg, a.data(), i.data(), item_frame.data(), item_emission.data(), &n_arcs, &n_items) == AMX_ERR_INVALID && says("arc_offsets do not ascend"));
            a[1] = keep;
        }
        i[0] = 2;
        CHECK(amx::nnseq_check_tables("t", n_seg, a.data(), i.data(), item_frame.data(), item_emission.data(), &n_arcs, &n_items) == AMX_ERR_INVALID && says("item_offsets[0]"));
        i = item_off;
        if (i.size() > 3) {
            i[1] = i[2] + 1;
            CHECK(amx::nnseq_check_tables("t", n_seg, a.data(), i.data(), item_frame.data(), item_emission.data(), &n_arcs, &n_items) == AMX_ERR_INVALID && says("item_offsets do not ascend"));
        }
        CHECK(amx::nnseq_check_tables("t", n_seg, arc_off.data(), item_off.data(), nullptr, item_emission.data(), &n_arcs, &n_items) == AMX_ERR_INVALID && says("item_frame"));
        CHECK(amx::nnseq_check_tables("t", n_seg, nullptr, item_off.data(), item_frame.data(), item_emission.data(), &n_arcs, &n_items) == AMX_ERR_INVALID);
        std::vector<long> many = {0, 1l << 27};   // refused before item_offsets is read
        CHECK(amx::nnseq_check_tables("t", 1, many.data(), item_off.data(), item_frame.data(), item_emission.data(), &n_arcs, &n_items) == AMX_ERR_INVALID && says("2^27"));
        std::vector<long> a1 = {0, 1}, i1 = {0, 1l << 27};
        CHECK(amx::nnseq_check_tables("t", 1, a1.data(), i1.data(), item_frame.data(), item_emission.data(), &n_arcs, &n_items) == AMX_ERR_INVALID && says("items"));
        std::vector<long> a0 = {0, 0}, i0 = {0};   // no arcs at all: no item table is needed
        CHECK(amx::nnseq_check_tables("t", 1, a0.data(), i0.data(), nullptr, nullptr, &n_arcs, &n_items) == AMX_OK && n_arcs == 0 && n_items == 0);
    }

    // bits, keys, sizes
    CHECK(amx::nnseq_bit_length(0) == 1 && amx::nnseq_bit_length(1) == 1 && amx::nnseq_bit_length(2) == 2 && amx::nnseq_bit_length(255) == 8 &&
          amx::nnseq_bit_length(256) == 9 && amx::nnseq_bit_length((1ll << 40) - 1) == 40);
    int                out_bits = 0, bits = 0;
    unsigned long long sentinel = 0;
    amx::nnseq_key_layout(1280, 50, &out_bits, &sentinel, &bits);
    CHECK(out_bits == 6 && sentinel == (1280ull << 6) && bits == 17);
    amx::nnseq_key_layout(4096, 10000, &out_bits, &sentinel, &bits);
    CHECK(out_bits == 14 && sentinel == (4096ull << 14) && bits == 27 && ((4095ull << 14) | 9999ull) < sentinel);
    amx::nnseq_key_layout(256, 1, &out_bits, &sentinel, &bits);
    CHECK(out_bits == 1 && sentinel == 512 && bits == 10);
    CHECK(amx::nnseq_scan_ws(1) == 1 && amx::nnseq_scan_ws(2048) == 2 && amx::nnseq_scan_ws(2049) == 2 + 1 + 1 && amx::nnseq_scan_ws(256ll * 65536) == 8192 + 4 + 1 + 1);
    const int Pin[3] = {128, 2048, 2048}, Pout[3] = {2048, 2048, 10112};
    CHECK(amx::nnseq_part_size(4096, 3, Pin, Pout) == (size_t)16 * 2048 * 10112 && amx::nnseq_part_size(256, 1, Pin, Pout) == (size_t)128 * 2048);

    // the refusal word
    CHECK(amx::nnseq_report_bad("t", ~0ull) == AMX_OK);
    CHECK(amx::nnseq_report_bad("t", (0ull << 48) | (300ull << 3) | amx::SEQ_BAD_LABEL) == AMX_ERR_INVALID && says("t: frame 300: the label"));
    CHECK(amx::nnseq_report_bad("t", (1ull << 48) | (5ull << 3) | amx::SEQ_BAD_WEIGHT) == AMX_ERR_INVALID && says("pass 0: arc 5: the arc weight"));
    CHECK(amx::nnseq_report_bad("t", (8ull << 48) | (((1ull << 27) - 1) << 3) | amx::SEQ_BAD_FRAME) == AMX_ERR_INVALID && says("pass 7: item 134217727: the frame"));
    CHECK(amx::nnseq_report_bad("t", (2ull << 48) | (4095ull << 3) | amx::SEQ_BAD_CELL) == AMX_ERR_INVALID && says("pass 1: workspace row 4095"));
    CHECK(amx::nnseq_report_bad("t", (1ull << 48) | (7ull << 3) | amx::SEQ_BAD_EMISSION) == AMX_ERR_INVALID && says("item 7: the emission"));
    printf("host_nnseq_test: ok (%d segments, %d rows, %lld arcs, %lld items)\n", n_seg, rows, (long long)arc_off[n_seg], (long long)item_frame.size());
    return 0;
}
