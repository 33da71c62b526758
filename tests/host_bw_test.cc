// Stand-alone host program for the host side of the Baum-Welch alignment section of include/amx.h: it compiles
// rasr_amd/csrc/align_bw.hip's host side into itself (no librasr_amd.so, no Python), creates handles without a context, walks through the
// refusals and their messages, and checks what the host lays out for the kernels beyond the Viterbi plan: the arcs by source, the arcs by
// label in (target, source, ordinal) order, the label tables and the offsets of potentials and survivor bits.  No device call is made: a
// handle without a context refuses amx_bw_align_dev after its checks and before it touches HIP.  Meant to be built with the host
// sanitizers (tests/test_bw.py does):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -w -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/host_bw_test.cc -o host_bw_test && ./host_bw_test
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/align_bw.hip"

// what api.cpp gives the library
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

static int g_failed = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("%s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, g_error.c_str()); \
            ++g_failed;                                                                 \
        }                                                                               \
    } while (0)

static bool says(const char* what) { return g_error.find(what) != std::string::npos; }

struct Batch {
    std::vector<int>           state_offsets{0}, initial, arc_offsets{0}, target, emission, label;
    std::vector<unsigned char> is_final;
    std::vector<float>         final_weight, weight;
    void segment(int n_states, int init) {
        state_offsets.push_back(state_offsets.back() + n_states);
        initial.push_back(init);
        is_final.resize(state_offsets.back(), 0);
        final_weight.resize(state_offsets.back(), 0.f);
    }
    void final(int global_state, float w) { is_final[global_state] = 1, final_weight[global_state] = w; }
    void arc(int t, int e, int l, float w) { target.push_back(t), emission.push_back(e), label.push_back(l), weight.push_back(w); }
    void end_state() { arc_offsets.push_back((int)target.size()); }
    amx_align_graphs view() const {
        return amx_align_graphs{state_offsets.data(), initial.data(), is_final.data(), final_weight.data(), arc_offsets.data(),
                                target.data(),        emission.data(), label.data(),   weight.data()};
    }
};

// two segments: a diamond 0 -> {2, 1} -> 3 whose two arcs into state 3 carry one label, and a two-state loop of 70 states' width in bits
static Batch two_segments() {
    Batch b;
    b.segment(4, 0);
    b.arc(2, 7, 70, 1.f), b.arc(1, 5, 50, 2.f), b.end_state();
    b.arc(3, 9, 90, 3.f), b.end_state();
    b.arc(3, 9, 90, 4.f), b.arc(2, 7, 70, 5.f), b.end_state();
    b.end_state();
    b.final(3, 0.5f);
    b.segment(70, 1);
    b.arc(1, 2, 20, 1.f), b.end_state();
    b.arc(0, 3, 30, 1.f), b.arc(1, 2, 20, 2.f), b.end_state();
    for (int i = 2; i < 70; ++i)
        b.end_state();
    b.final(4 + 1, 0.f);
    return b;
}

static int create(amx_bw_cfg cfg, amx_bw** h) { return amx_bw_create(nullptr, &cfg, h); }

int main() {
    amx_bw_cfg d;
    amx_bw_default_cfg(&d);
    CHECK(d.min_acoustic_pruning == 50.f && d.max_acoustic_pruning == FLT_MAX && d.increment_factor == 2.f && d.n_best_pruning == INT_MAX);
    CHECK(d.min_weight == 0.f && d.use_partial_sums == 0 && d.score_scale == 1.f && d.increase_until_no_score_difference == 1);
    amx_bw* h = nullptr;
    {
        amx_bw_cfg c = d;
        c.use_partial_sums = 1;
        CHECK(create(c, &h) == AMX_ERR_UNSUPPORTED && !h && says("use_partial_sums 1"));
        c = d, c.min_weight = 0.5f;
        CHECK(create(c, &h) == AMX_ERR_UNSUPPORTED && !h && says("min_weight 0.5"));
        c = d, c.min_weight = FLT_MIN;
        CHECK(create(c, &h) == AMX_OK && h);
        amx_bw_destroy(h), h = nullptr;
        c = d, c.n_best_pruning = 7;
        CHECK(create(c, &h) == AMX_ERR_UNSUPPORTED && says("amx_bw_create") && says("n_best_pruning 7"));
        c = d, c.increment_factor = 1.f;
        CHECK(create(c, &h) == AMX_ERR_INVALID && says("Inconsistent"));
        CHECK(amx_bw_create(nullptr, nullptr, &h) == AMX_ERR_INVALID && amx_bw_create(nullptr, &d, nullptr) == AMX_ERR_INVALID);
    }
    CHECK(create(d, &h) == AMX_OK && h);
    const Batch            b = two_segments();
    const amx_align_graphs g = b.view();
    const long             off[3] = {2, 5, 9};
    amx_bw_result          res[2];
    unsigned long long     counters[3] = {9, 9, 9};
    // every check passes, then the missing context stops the call
    CHECK(amx_bw_align_dev(h, 2, off, &g, nullptr, 12, 10, nullptr, res, counters) == AMX_ERR_STATE && says("without a context"));
    CHECK(counters[0] == 0 && counters[1] == 0 && counters[2] == 0 && amx_bw_n_items(h) == 0);
    CHECK(amx_bw_align_dev(h, 0, off, &g, nullptr, 12, 10, nullptr, nullptr, nullptr) == AMX_OK);
    CHECK(amx_bw_align_dev(h, 2, off, &g, nullptr, 12, 9, nullptr, res, nullptr) == AMX_ERR_INVALID && says("arc_emission") && says("9 columns"));
    CHECK(amx_bw_items_dev(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == AMX_OK);
    CHECK(amx_bw_items_dev(h, -1, nullptr, nullptr, nullptr, nullptr, nullptr) == AMX_ERR_INVALID && says("capacity -1") && says("0 items"));
    {
        Batch c = b;
        c.emission[3] = 8;   // label 90 on emissions 9 and 8
        const amx_align_graphs gc = c.view();
        CHECK(amx_bw_align_dev(h, 2, off, &gc, nullptr, 12, 10, nullptr, res, nullptr) == AMX_ERR_INVALID && says("segment 0") && says("label 90") &&
              says("emission indices 9 and 8"));
    }
    CHECK(amx_gather_rows_dev(nullptr, nullptr, 4, 4, 0, nullptr, nullptr, 4) == AMX_ERR_INVALID && says("NULL context"));
    // the plans of the valid batch
    amx::AlignPlan p;
    amx::BwPlan    q;
    CHECK(amx::align_plan(2, off, &g, 10, "test", &p) == AMX_OK && amx::bw_plan(2, &g, p, "test", &q) == AMX_OK);
    CHECK(q.bseg.size() == 2 && q.bseg[0].n_labels == 3 && q.bseg[0].lab0 == 0 && q.bseg[1].n_labels == 2 && q.bseg[1].lab0 == 3);
    CHECK((q.lab_val == std::vector<int>{50, 70, 90, 20, 30}) && (q.lab_em == std::vector<int>{5, 7, 9, 2, 3}));
    CHECK((q.lab_off == std::vector<int>{0, 1, 3, 5, 7, 8}));
    CHECK(q.bseg[0].sw == 1 && q.bseg[1].sw == 2 && q.bseg[0].sv0 == 0 && q.bseg[1].sv0 == 3 && q.bseg[0].al0 == 0 && q.bseg[1].al0 == 4 * 4);
    CHECK(q.alpha_words == 16 + 5 * 70 && q.surv_words == 3 + 4 * 2 && q.max_labels == 3);
    CHECK((q.out_off == std::vector<int>(b.arc_offsets)));
    // by source: target, column, weight bits, label index
    const int cols0[] = {1, 0, 2, 2, 1};   // emissions 7, 5, 9, 9, 7 among {5, 7, 9}
    const int labs0[] = {1, 0, 2, 2, 1};
    for (int a = 0; a < 5; ++a) {
        float w;
        std::memcpy(&w, &q.out_arc[a].z, sizeof w);
        CHECK(q.out_arc[a].x == b.target[a] && q.out_arc[a].y == cols0[a] && w == b.weight[a] && q.out_arc[a].w == labs0[a]);
    }
    // by label, within a label by (target, source, ordinal): label 50: 0->1; label 70: 0->2, 2->2; label 90: 1->3, 2->3
    const int want[5][2] = {{0, 1}, {0, 2}, {2, 2}, {1, 3}, {2, 3}};
    const float ww[5]    = {2.f, 1.f, 5.f, 3.f, 4.f};
    for (int a = 0; a < 5; ++a) {
        float w;
        std::memcpy(&w, &q.lab_arc[a].w, sizeof w);
        CHECK(q.lab_arc[a].x == want[a][0] && q.lab_arc[a].y == want[a][1] && w == ww[a]);
    }
    // the second segment's lists start where the first one's end: label 20: 0->1 and 1->1 (targets equal: by source), label 30: 1->0
    CHECK(q.lab_arc[5].x == 0 && q.lab_arc[5].y == 1 && q.lab_arc[6].x == 1 && q.lab_arc[6].y == 1 && q.lab_arc[7].x == 1 && q.lab_arc[7].y == 0);
    amx_bw_destroy(h);
    amx_bw_destroy(nullptr);
    if (g_failed) {
        std::printf("host_bw_test: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("host_bw_test: ok\n");
    return 0;
}
