// Stand-alone host program for the host side of the linear-segmentation section of include/amx.h: it compiles rasr_amd/csrc/linseg.hip's host
// side into itself (no librasr_amd.so, no Python), creates handles without a context, walks through every refusal and its message, checks the
// segment table of a batch (reasons the host decides, places in the workspace) and holds the host instantiation of the kernel's two
// functions, logLikelihood and the spread's index, against values worked out by hand.  No device call is made: a handle without a
// context refuses amx_linseg_align_dev after its checks and before it touches HIP.  Meant to be built with the host sanitizers
// (tests/test_linseg.py does):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -w -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/host_linseg_test.cc -o host_linseg_test && ./host_linseg_test
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/linseg.hip"

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

// the flat models of a batch in the ABI's tables
struct Models {
    std::vector<int> offsets{0}, label, emission;
    int              silence_label = 900, silence_emission = 0;
    void segment(int n, int first) {
        for (int i = 0; i < n; ++i)
            label.push_back(first + i), emission.push_back(i % 7);
        offsets.push_back((int)label.size());
    }
    amx_linseg_models view() const { return amx_linseg_models{offsets.data(), label.data(), emission.data(), silence_label, silence_emission}; }
};

static Models three_segments() {
    Models m;
    m.segment(3, 10), m.segment(0, 0), m.segment(5, 20);
    return m;
}

static amx_linseg* handle(const amx_linseg_cfg* cfg = nullptr) {
    amx_linseg_cfg c;
    amx_linseg_default_cfg(&c);
    amx_linseg* h = nullptr;
    CHECK(amx_linseg_create(nullptr, cfg ? cfg : &c, &h) == AMX_OK && h);
    return h;
}

static int call(amx_linseg* h, const Models& m, const std::vector<long>& off, int ld = 1) {
    const amx_linseg_models        v = m.view();
    std::vector<amx_linseg_result> r(off.size());
    unsigned long long             counters[AMX_LINSEG_N_REASONS];
    return amx_linseg_align_dev(h, (int)off.size() - 1, off.data(), &v, nullptr, ld, nullptr, nullptr, r.data(), counters);
}

int main() {
    amx_linseg_cfg c;
    amx_linseg_default_cfg(&c);
    CHECK(c.number_of_iterations == 3 && c.penalty == 100.0 && c.minimum_speech_proportion == 0.7f && c.should_use_sietill == 0);
    CHECK(c.minimum_segment_length == 1 && c.maximum_segment_length == INT_MAX);
    amx_linseg_default_cfg(nullptr);
    amx_linseg* h = (amx_linseg*)0x1;
    CHECK(amx_linseg_create(nullptr, &c, nullptr) == AMX_ERR_INVALID);
    CHECK(amx_linseg_create(nullptr, nullptr, &h) == AMX_ERR_INVALID && h == nullptr);
    amx_linseg_cfg bad = c;
    bad.number_of_iterations = -1;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && h == nullptr && says("number_of_iterations -1"));
    bad = c, bad.number_of_iterations = AMX_LINSEG_MAX_ITERATIONS + 1;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_UNSUPPORTED && says("number_of_iterations 4097") && says("limit of 4096 iterations"));
    bad = c, bad.penalty = NAN;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("penalty is not a number"));
    bad = c, bad.penalty = -1.0;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("penalty -1"));
    bad = c, bad.penalty = INFINITY;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("penalty inf"));
    bad = c, bad.minimum_speech_proportion = NAN;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("minimum_speech_proportion is not a number"));
    bad = c, bad.minimum_speech_proportion = 1.5f;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("minimum_speech_proportion 1.5") && says("[0, 1]"));
    bad = c, bad.minimum_speech_proportion = -0.25f;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("minimum_speech_proportion -0.25"));
    bad = c, bad.minimum_segment_length = -2;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("minimum_segment_length -2"));
    bad = c, bad.maximum_segment_length = -3;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_ERR_INVALID && says("maximum_segment_length -3"));
    bad = c, bad.penalty = 0.0, bad.minimum_speech_proportion = 1.f, bad.number_of_iterations = 0, bad.should_use_sietill = 1;
    CHECK(amx_linseg_create(nullptr, &bad, &h) == AMX_OK && h);
    amx_linseg_destroy(h);
    amx_linseg_destroy(nullptr);

    // the segment table of a valid batch: the reasons the host decides and the places of the chains
    {
        amx_linseg_cfg lim = c;
        lim.minimum_segment_length = 4, lim.maximum_segment_length = 9;
        Models m;
        m.segment(3, 10), m.segment(0, 0), m.segment(5, 20), m.segment(2, 30), m.segment(1, 40), m.segment(2, 50);
        const amx_linseg_models v = m.view();
        const long              off[7] = {5, 9, 12, 12, 15, 25, 34};   // frames 4, 3, 0, 3, 10, 9
        amx::LinsegPlan         p;
        CHECK(amx::linseg_plan(lim, 6, off, &v, "plan", &p) == AMX_OK);
        CHECK(p.frames == 29 && p.chain_words == 35 && p.states == 13 && p.seg.size() == 6);
        const int       reasons[6] = {AMX_LINSEG_OK, AMX_LINSEG_NO_STATES, AMX_LINSEG_NO_STATES, AMX_LINSEG_TOO_SHORT, AMX_LINSEG_TOO_LONG, AMX_LINSEG_OK};
        const long long chain0[6]  = {0, 5, 9, 10, 14, 25};
        const int       state0[6]  = {0, 3, 3, 8, 10, 11};
        for (int s = 0; s < 6; ++s) {
            CHECK(p.seg[s].reason == reasons[s] && p.seg[s].chain0 == chain0[s] && p.seg[s].state0 == state0[s]);
            CHECK(p.seg[s].frame0 == off[s] && p.seg[s].frames == off[s + 1] - off[s] && p.seg[s].n_states == m.offsets[s + 1] - m.offsets[s]);
            // a segment's chains (frames + 1 doubles) end where the next one's begin
            CHECK(s == 5 || p.seg[s].chain0 + p.seg[s].frames + 1 == p.seg[s + 1].chain0);
        }
        CHECK(p.seg[5].chain0 + p.seg[5].frames + 1 == p.chain_words);
    }

    // refusals of a call: each names its field, and the call of a valid batch stops at the missing context
    h = handle();
    {
        Models m = three_segments();
        CHECK(call(h, m, {0, 5, 9, 20}) == AMX_ERR_STATE && says("without a context"));
        CHECK(call(h, m, {3, 3, 3, 3}) == AMX_ERR_STATE);
        CHECK(call(h, m, {0, 5, 4, 20}) == AMX_ERR_INVALID && says("frame offsets decrease at segment 1"));
        CHECK(call(h, m, {-1, 5, 9, 20}) == AMX_ERR_INVALID && says("negative frame offset"));
        CHECK(call(h, m, {0, 5, 9, 1l << 31}) == AMX_ERR_INVALID && says("2^31"));
        CHECK(call(h, m, {0, 5, 9, (1l << 31) - 1}) == AMX_ERR_STATE);
        CHECK(call(h, m, {0, 5, 9, 20}, 0) == AMX_ERR_INVALID && says("energy_ld 0"));
        m.label[1] = -1;
        CHECK(call(h, m, {0, 5, 9, 20}) == AMX_ERR_INVALID && says("segment 0") && says("state_label[1] = -1"));
        m = three_segments(), m.emission[5] = -4;
        CHECK(call(h, m, {0, 5, 9, 20}) == AMX_ERR_INVALID && says("segment 2") && says("state_emission[5] = -4"));
        m = three_segments(), m.silence_label = -1;
        CHECK(call(h, m, {0, 5, 9, 20}) == AMX_ERR_INVALID && says("silence_label -1"));
        m = three_segments(), m.silence_emission = -2;
        CHECK(call(h, m, {0, 5, 9, 20}) == AMX_ERR_INVALID && says("silence_emission -2"));
        m = three_segments(), m.offsets[0] = 1;
        CHECK(call(h, m, {0, 5, 9, 20}) == AMX_ERR_INVALID && says("state_offsets[0] is 1"));
        m = three_segments(), m.offsets[2] = 2;
        CHECK(call(h, m, {0, 5, 9, 20}) == AMX_ERR_INVALID && says("state_offsets decrease at segment 1"));
        m                         = three_segments();
        const amx_linseg_models v = m.view();
        const long              off[4] = {0, 5, 9, 20};
        amx_linseg_result       r[3];
        CHECK(amx_linseg_align_dev(nullptr, 3, off, &v, nullptr, 1, nullptr, nullptr, r, nullptr) == AMX_ERR_INVALID && says("NULL handle"));
        CHECK(amx_linseg_align_dev(h, -1, off, &v, nullptr, 1, nullptr, nullptr, r, nullptr) == AMX_ERR_INVALID && says("n_seg -1"));
        CHECK(amx_linseg_align_dev(h, 3, off, &v, nullptr, 1, nullptr, nullptr, nullptr, nullptr) == AMX_ERR_INVALID && says("NULL result"));
        CHECK(amx_linseg_align_dev(h, 3, nullptr, &v, nullptr, 1, nullptr, nullptr, r, nullptr) == AMX_ERR_INVALID && says("NULL frame_offsets"));
        CHECK(amx_linseg_align_dev(h, 3, off, nullptr, nullptr, 1, nullptr, nullptr, r, nullptr) == AMX_ERR_INVALID && says("NULL models"));
        amx_linseg_models w = v;
        w.state_label       = nullptr;
        CHECK(amx_linseg_align_dev(h, 3, off, &w, nullptr, 1, nullptr, nullptr, r, nullptr) == AMX_ERR_INVALID && says("NULL state_label"));
        unsigned long long counters[AMX_LINSEG_N_REASONS] = {9, 9, 9, 9, 9, 9, 9};
        CHECK(amx_linseg_align_dev(h, 0, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, counters) == AMX_OK && counters[0] == 0 && counters[6] == 0);
        double x;
        CHECK(amx_linseg_chains(h, 0, &x, &x) == AMX_ERR_STATE);
        CHECK(amx_linseg_chains(nullptr, 0, &x, &x) == AMX_ERR_INVALID);
    }
    amx_linseg_destroy(h);

    // logLikelihood's host instantiation on chains worked out by hand: energies 1, 1, 5, 7, 1 with penalty 0, so M_ and Q_ are integers
    {
        const double m[6] = {0, 1, 2, 7, 14, 15}, q[6] = {0, 1, 2, 27, 76, 77};
        // (ib, ie) = (3, 4): silence frames 1, 2, 5: s1 = 3, mean 1, variance 0 -> floored at 0.5; speech frames 3, 4: s2 = 2, mean 6, variance 1
        const double want = 3.0 * std::log(0.5) + 2.0 * std::log(1.0);
        CHECK(amx::linseg_likelihood<false>(m, q, 5u, 0.0, 0.7f * 5.f, 3u, 4u) == DBL_MAX);    // 1 frame apart: below 0.7 * 5
        CHECK(amx::linseg_likelihood<false>(m, q, 5u, 0.0, 0.2f * 5.f, 3u, 4u) == want);
        CHECK(amx::linseg_likelihood<true>(m, q, 5u, 0.0, 0.2f * 5.f, 3u, 4u) == want);         // the fused product is exact here
        CHECK(amx::linseg_likelihood<false>(m, q, 5u, 0.0, 0.f, 1u, 2u) == DBL_MAX);            // speech quieter than the rest: the mean gate
        CHECK(amx::linseg_likelihood<false>(m, q, 5u, 0.0, 0.f, 1u, 5u) == DBL_MAX);            // s1 = 0: 0 / 0 compares false
        // penalty 4: Q_ grows by (x * x + 2) / 4, the squared mean is divided by 4
        const double q4[6] = {0, 0.75, 1.5, 8.25, 21.0, 21.75};
        const double sil = 2.25 / 3 - (1.0 * 1.0) / 4, spe = 19.5 / 2 - (6.0 * 6.0) / 4;
        CHECK(amx::linseg_likelihood<false>(m, q4, 5u, 4.0, 0.f, 3u, 4u) == 3.0 * std::log(sil) + 2.0 * std::log(spe));
    }
    // the spread's index: round half away from zero of an f32 product
    {
        CHECK(amx::linseg_index(0.5f, 1) == 1 && amx::linseg_index(0.5f, 2) == 1 && amx::linseg_index(0.5f, 3) == 2 && amx::linseg_index(0.f, 77) == 0);
        const float slope = (float)(46 - 1) / (float)45;
        CHECK(amx::linseg_index(slope, 45) == 45 && amx::linseg_index(2.5f, 1) == 3 && amx::linseg_index(2.4999f, 1) == 2);
        for (int n = 2; n < 300; ++n)          // the last frame always reaches the last state when there is more than one frame
            for (int len = 1; len < 300; len += 7)
                CHECK(amx::linseg_index((float)(n - 1) / (float)len, (unsigned)len) == (unsigned)(n - 1));
    }
    if (g_failed) {
        std::printf("host_linseg_test: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("host_linseg_test: ok\n");
    return 0;
}
