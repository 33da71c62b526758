// Stand-alone host program for the host side of the Viterbi alignment section of include/amx.h: it compiles rasr_amd/csrc/align.hip's host
// side into itself (no librasr_amd.so, no Python), creates handles without a context, walks through every refusal and its message,
// checks the transposition of a batch into by-target order, and holds the arithmetic count of the passes that are not run against a loop
// that runs them.  No device call is made: a handle without a context refuses amx_align_viterbi_dev after its checks and before it
// touches HIP.  Meant to be built with the host sanitizers (tests/test_align.py does):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -w -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/host_align_test.cc -o host_align_test && ./host_align_test
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/align.hip"

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

// a batch of graphs in the ABI's tables
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

// two segments: a diamond 0 -> {2, 1} -> 3 whose arcs leave state 0 towards state 2 first, and a two-state loop
static Batch two_segments() {
    Batch b;
    b.segment(4, 0);
    b.arc(2, 7, 70, 1.f), b.arc(1, 5, 50, 2.f), b.end_state();
    b.arc(3, 9, 90, 3.f), b.end_state();
    b.arc(3, 9, 91, 4.f), b.arc(2, 7, 71, 5.f), b.end_state();
    b.end_state();
    b.final(3, 0.5f);
    b.segment(2, 1);
    b.arc(1, 3, 30, 6.f), b.end_state();
    b.arc(1, 3, 31, 7.f), b.arc(0, 11, 110, 8.f), b.end_state();
    b.final(4, 0.f);
    return b;
}

static amx_align* handle() {
    amx_align_cfg c;
    amx_align_default_cfg(&c);
    amx_align* h = nullptr;
    CHECK(amx_align_create(nullptr, &c, &h) == AMX_OK && h);
    return h;
}

static int call(amx_align* h, const Batch& b, const std::vector<long>& off, int n_columns = 12) {
    const amx_align_graphs       g = b.view();
    std::vector<amx_align_result> r(off.size());
    unsigned long long           counters[3];
    return amx_align_viterbi_dev(h, (int)off.size() - 1, off.data(), &g, nullptr, n_columns, n_columns, nullptr, nullptr, nullptr, r.data(), counters);
}

// Aligner::feed(vector)'s loop (Aligner.cc:603-630) over passes that all give the same outcome, run one by one
static void brute(const amx::AlignLoop& c, bool reached, double avg, float score, float first_previous, int* n, float* last) {
    float previous = first_previous;
    *n             = 0;
    for (float t = c.lo; t <= c.hi; t *= c.factor) {
        ++*n;
        *last = t;
        if (c.factor <= 1)
            break;
        if (reached && avg >= c.min_avg) {
            if (!c.incr)
                break;
            if (t > c.lo && amx::align_almost_equal(score, previous))
                break;
        }
        previous = score;
    }
}

int main() {
    amx_align_cfg c;
    amx_align_default_cfg(&c);
    CHECK(c.min_acoustic_pruning == 50.f && c.max_acoustic_pruning == FLT_MAX && c.increment_factor == 2.f && c.min_average_number_of_states == 0.0);
    CHECK(c.increase_until_no_score_difference == 1 && c.n_best_pruning == INT_MAX && c.mode == AMX_ALIGN_VITERBI && c.score_scale == 1.f);
    amx_align_default_cfg(nullptr);
    amx_align* h = (amx_align*)0x1;
    CHECK(amx_align_create(nullptr, &c, nullptr) == AMX_ERR_INVALID);
    CHECK(amx_align_create(nullptr, nullptr, &h) == AMX_ERR_INVALID && h == nullptr);
    amx_align_cfg bad = c;
    bad.mode          = AMX_ALIGN_BAUM_WELCH;
    CHECK(amx_align_create(nullptr, &bad, &h) == AMX_ERR_UNSUPPORTED && h == nullptr && says("mode") && says("baum-welch"));
    bad = c, bad.n_best_pruning = 10;
    CHECK(amx_align_create(nullptr, &bad, &h) == AMX_ERR_UNSUPPORTED && says("n_best_pruning 10"));
    bad = c, bad.min_acoustic_pruning = 60.f, bad.max_acoustic_pruning = 50.f;
    CHECK(amx_align_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("min_acoustic_pruning=60") && says("max_acoustic_pruning=50"));
    bad = c, bad.increment_factor = 1.f;
    CHECK(amx_align_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("increment_factor=1"));
    bad = c, bad.min_acoustic_pruning = bad.max_acoustic_pruning = 70.f, bad.increment_factor = 1.f;
    CHECK(amx_align_create(nullptr, &bad, &h) == AMX_OK && h);
    amx_align_destroy(h);
    bad = c, bad.increment_factor = 1.0000001f;
    CHECK(amx_align_create(nullptr, &bad, &h) == AMX_ERR_UNSUPPORTED && says("limit of 4096 passes"));
    bad = c, bad.score_scale = NAN;
    CHECK(amx_align_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("score_scale"));
    amx_align_destroy(nullptr);

    // the plan of a valid batch: by-target order, compact columns, offsets of the scratch matrices
    {
        const Batch            b = two_segments();
        const amx_align_graphs g = b.view();
        const long             off[3] = {3, 8, 8};
        amx::AlignPlan         p;
        CHECK(amx::align_plan(2, off, &g, 12, "plan", &p) == AMX_OK);
        CHECK(p.frames == 5 && p.max_states == 4 && p.max_cols == 3 && p.max_in == 5 && p.cm_words == 15 && p.bp_words == 20);
        CHECK(p.cols == (std::vector<int>{5, 7, 9, 3, 11}));
        CHECK(p.in_off == (std::vector<int>{0, 0, 1, 3, 5, 6, 8}));
        CHECK(p.seg[0].frame0 == 3 && p.seg[0].frames == 5 && p.seg[1].frames == 0 && p.seg[1].state0 == 4 && p.seg[1].initial == 1);
        CHECK(p.seg[1].in0 == 5 && p.seg[1].n_in == 3 && p.seg[1].col0 == 3 && p.seg[1].n_cols == 2 && p.seg[1].cm0 == 15 && p.seg[1].bp0 == 20);
        // state 1 <- arc 1 (0, ordinal 1); state 2 <- arc 0 (0, ordinal 0), arc 4 (2, ordinal 1); state 3 <- arc 2 (1, 0), arc 3 (2, 0)
        const int want[8][4] = {{0 | 1 << 16, 0, 0, 1}, {0 | 0 << 16, 1, 0, 0}, {2 | 1 << 16, 1, 0, 4}, {1 | 0 << 16, 2, 0, 2}, {2 | 0 << 16, 2, 0, 3},
                                {1 | 1 << 16, 1, 0, 7}, {0 | 0 << 16, 0, 0, 5}, {1 | 0 << 16, 0, 0, 6}};
        for (int i = 0; i < 8; ++i) {
            float w;
            std::memcpy(&w, &p.in_arc[i].z, sizeof w);
            CHECK(p.in_arc[i].x == want[i][0] && p.in_arc[i].y == want[i][1] && p.in_arc[i].w == want[i][3] && w == b.weight[want[i][3]]);
        }
        CHECK(p.arc_src == (std::vector<int>{0, 0, 1, 2, 2, 0, 1, 1}) && p.arc_col == (std::vector<int>{1, 0, 2, 2, 1, 0, 0, 1}));
    }

    // refusals of a call: each names segment and index, and the call of a valid batch stops at the missing context
    h = handle();
    {
        Batch b = two_segments();
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_STATE && says("without a context"));
        CHECK(call(h, b, {0, 5, 4}) == AMX_ERR_INVALID && says("frame offsets decrease at segment 1"));
        CHECK(call(h, b, {-1, 5, 9}) == AMX_ERR_INVALID && says("negative frame offset"));
        b.target[3] = 4;
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_INVALID && says("segment 0") && says("arc_target[3] = 4"));
        b = two_segments(), b.target[7] = 2;
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_INVALID && says("segment 1") && says("arc_target[7] = 2"));
        b = two_segments(), b.emission[6] = 12;
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_INVALID && says("segment 1") && says("arc_emission[6] = 12") && says("12 columns"));
        b = two_segments(), b.emission[0] = -1;
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_INVALID && says("arc_emission[0] = -1"));
        b = two_segments(), b.initial[1] = 2;
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_INVALID && says("segment 1") && says("initial_state 2"));
        b = two_segments(), b.weight[2] = NAN;
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_INVALID && says("segment 0") && says("arc_weight[2]"));
        b = two_segments(), b.final_weight[3] = NAN;
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_INVALID && says("segment 0") && says("final_weight of state 3"));
        b = two_segments(), b.final_weight[0] = NAN;   // not final: not read
        CHECK(call(h, b, {0, 5, 9}) == AMX_ERR_STATE);
        const amx_align_graphs g = b.view();
        const long             off[3] = {0, 5, 9};
        amx_align_result       r[2];
        CHECK(amx_align_viterbi_dev(nullptr, 2, off, &g, nullptr, 12, 12, nullptr, nullptr, nullptr, r, nullptr) == AMX_ERR_INVALID);
        CHECK(amx_align_viterbi_dev(h, 2, off, &g, nullptr, 8, 12, nullptr, nullptr, nullptr, r, nullptr) == AMX_ERR_INVALID && says("scores_ld 8"));
        CHECK(amx_align_viterbi_dev(h, 2, off, &g, nullptr, 12, 12, nullptr, nullptr, nullptr, nullptr, nullptr) == AMX_ERR_INVALID && says("NULL result"));
        CHECK(amx_align_viterbi_dev(h, 2, off, nullptr, nullptr, 12, 12, nullptr, nullptr, nullptr, r, nullptr) == AMX_ERR_INVALID);
        CHECK(amx_align_viterbi_dev(h, 0, off, &g, nullptr, 12, 12, nullptr, nullptr, nullptr, nullptr, nullptr) == AMX_OK);
    }
    {   // the limits: states, arcs out of a state
        Batch b;
        b.segment(AMX_ALIGN_MAX_STATES + 1, 0);
        for (int i = 0; i <= AMX_ALIGN_MAX_STATES; ++i)
            b.arc(i, 0, 0, 1.f), b.end_state();
        CHECK(call(h, b, {0, 2}) == AMX_ERR_UNSUPPORTED && says("segment 0") && says("2049 states") && says("limit of 2048 states"));
        Batch f;
        f.segment(2, 0);
        for (int i = 0; i < AMX_ALIGN_MAX_OUT_ARCS + 1; ++i)
            f.arc(1, i % 12, i, 1.f);
        f.end_state(), f.end_state();
        CHECK(call(h, f, {0, 2}) == AMX_ERR_UNSUPPORTED && says("state 0 has 65 arcs") && says("limit of 64 arcs"));
        Batch ok;
        ok.segment(2, 0);
        for (int i = 0; i < AMX_ALIGN_MAX_OUT_ARCS; ++i)
            ok.arc(1, i % 12, i, 1.f);
        ok.end_state(), ok.end_state();
        CHECK(call(h, ok, {0, 2}) == AMX_ERR_STATE);
    }
    amx_align_destroy(h);

    // passes that repeat an outcome: counted, against the loop that runs them (the first pass is the one that was run)
    {
        const float los[] = {50.f, 1.f, 3e37f}, his[] = {FLT_MAX, 400.f, 50.f, 3.2e38f}, factors[] = {2.f, 1.5f, 10.f, 1.01f};
        const float scores[] = {123.5f, 0.f, FLT_MAX, INFINITY, -7.f};
        int         compared = 0;
        for (float lo : los)
            for (float hi : his)
                for (float factor : factors)
                    for (double min_avg : {0.0, 6.0})
                        for (int incr : {0, 1})
                            for (float score : scores)
                                for (double avg : {7.0, 2.0, (double)NAN}) {
                                    if (lo > hi || amx::align_steps(lo, hi, factor, AMX_ALIGN_MAX_PASSES) > AMX_ALIGN_MAX_PASSES)
                                        continue;
                                    const amx::AlignLoop c{lo, hi, factor, min_avg, incr};
                                    const bool           reached = score != FLT_MAX;
                                    int                  want_n;
                                    float                want_t = 0;
                                    brute(c, reached, avg, score, FLT_MAX, &want_n, &want_t);
                                    // what the kernel does after its first pass, which pruned nothing
                                    int                n = 1;
                                    float              t = lo;
                                    unsigned long long counted = 0;
                                    if (!amx::align_pass_ends(c, t, reached, avg, score, FLT_MAX))
                                        amx::align_count_repeats(c, &t, reached, avg, score, &n, &counted);
                                    CHECK(n == want_n && t == want_t && counted == (unsigned long long)(n - 1));
                                    ++compared;
                                }
        CHECK(compared > 1000);
        CHECK(amx::align_steps(50.f, FLT_MAX, 2.f, AMX_ALIGN_MAX_PASSES) == 123 && amx::align_steps(80.f, 80.f, 1.f, AMX_ALIGN_MAX_PASSES) == 1);
    }
    if (g_failed) {
        std::printf("host_align_test: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("host_align_test: ok\n");
    return 0;
}
