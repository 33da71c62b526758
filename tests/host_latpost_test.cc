// Stand-alone host program for the host side of the lattice-posterior section of include/amx.h: it compiles latpost_host.cpp into a program
// of its own (no device is touched), so that tests/test_latpost.py can run it under the host sanitizers.
//   host_latpost_test case.bin
// case.bin (written by the test): int32 n_cases, then per lattice int32 n, n_arcs, initial | i64 arc_offsets [n + 1] | i32 arc_target |
// f32 arc_weight, arc_risk | u8 final_flag [n] | f32 final_weight, final_risk | the restatement's i32 discover_index, level_backward,
// level_forward [n] | i32 level_super, reason, undefined_arcs, states_coreached | i32 count, then the transposed lists, flattened, as arc
// indices of this lattice.  The lattices are planned one by one, all in one call, and in reversed order; then every refusal and an empty call.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/latpost_host.cpp"

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

struct amx_latpost {
    amx_latpost_cfg cfg;
};
namespace amx {
const amx_latpost_cfg& latpost_cfg_of(const amx_latpost* h) {
    return h->cfg;
}
}  // namespace amx

#define CHECK(cond)                                                                                                     \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            printf("host_latpost_test: line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_error.c_str());       \
            return 1;                                                                                                   \
        }                                                                                                               \
    } while (0)

struct Lattice {
    int                  n = 0, n_arcs = 0, initial = 0;
    std::vector<long>    off;
    std::vector<int32_t> target, discover, level_b, level_f, incoming;
    std::vector<float>   weight, risk, final_weight, final_risk;
    std::vector<uint8_t> final_flag;
    int32_t              tail[4] = {0, 0, 0, 0};
};

template<class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// a call over `lats` in the given order; the outputs against what the file says
static int plan_and_compare(const amx_latpost* h, const std::vector<const Lattice*>& lats) {
    std::vector<long>    state_off(1, 0), arc_off(1, 0);
    std::vector<int32_t> target, initial;
    std::vector<float>   weight, risk, fw, fr;
    std::vector<uint8_t> ff;
    for (const Lattice* l : lats) {
        const long a0 = arc_off.back();
        state_off.push_back(state_off.back() + l->n);
        for (int s = 0; s < l->n; ++s)
            arc_off.push_back(a0 + l->off[(size_t)s + 1]);
        target.insert(target.end(), l->target.begin(), l->target.end());
        weight.insert(weight.end(), l->weight.begin(), l->weight.end()), risk.insert(risk.end(), l->risk.begin(), l->risk.end());
        fw.insert(fw.end(), l->final_weight.begin(), l->final_weight.end()), fr.insert(fr.end(), l->final_risk.begin(), l->final_risk.end());
        ff.insert(ff.end(), l->final_flag.begin(), l->final_flag.end());
        initial.push_back(l->initial);
    }
    const size_t nS = (size_t)state_off.back(), nA = (size_t)arc_off.back(), nG = lats.size();
    std::vector<int32_t> disc(nS + 1), lb(nS + 1), lf(nS + 1), super(nG + 1), in_arc(nA + 1), final_order(nS + 1);
    std::vector<long>    in_off(nS + 2);
    std::vector<amx_latpost_info> info(nG + 1);
    CHECK(amx_latpost_plan_host(h, (int)nG, state_off.data(), arc_off.data(), target.data(), weight.data(), risk.data(), initial.data(), ff.data(), fw.data(),
                                fr.data(), disc.data(), lb.data(), lf.data(), super.data(), in_off.data(), in_arc.data(), final_order.data(), info.data()) == AMX_OK);
    for (size_t g = 0; g < nG; ++g) {
        const Lattice* l  = lats[g];
        const size_t   s0 = (size_t)state_off[g];
        const long     a0 = arc_off[s0];
        for (int s = 0; s < l->n; ++s) {
            CHECK(disc[s0 + s] == l->discover[(size_t)s]);
            CHECK(lb[s0 + s] == l->level_b[(size_t)s]);
            CHECK(lf[s0 + s] == l->level_f[(size_t)s]);
        }
        CHECK(super[g] == l->tail[0] && info[g].reason == l->tail[1] && info[g].undefined_arcs == l->tail[2] && info[g].states_coreached == l->tail[3]);
        CHECK((size_t)(in_off[s0 + l->n] - in_off[s0]) == l->incoming.size());
        for (size_t k = 0; k < l->incoming.size(); ++k)
            CHECK(in_arc[(size_t)in_off[s0] + k] - a0 == l->incoming[k]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: host_latpost_test case.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    CHECK(f);
    int32_t n_cases = 0;
    CHECK(fread(&n_cases, 4, 1, f) == 1 && n_cases > 0);
    std::vector<Lattice> lats((size_t)n_cases);
    for (Lattice& l : lats) {
        int32_t head[3];
        CHECK(fread(head, 4, 3, f) == 3);
        l.n = head[0], l.n_arcs = head[1], l.initial = head[2];
        std::vector<int64_t> off;
        CHECK(take(f, off, (size_t)l.n + 1));
        l.off.assign(off.begin(), off.end());
        CHECK(take(f, l.target, (size_t)l.n_arcs) && take(f, l.weight, (size_t)l.n_arcs) && take(f, l.risk, (size_t)l.n_arcs));
        CHECK(take(f, l.final_flag, (size_t)l.n) && take(f, l.final_weight, (size_t)l.n) && take(f, l.final_risk, (size_t)l.n));
        CHECK(take(f, l.discover, (size_t)l.n) && take(f, l.level_b, (size_t)l.n) && take(f, l.level_f, (size_t)l.n));
        CHECK(fread(l.tail, 4, 4, f) == 4);
        int32_t count = 0;
        CHECK(fread(&count, 4, 1, f) == 1 && count >= 0);
        CHECK(take(f, l.incoming, (size_t)count));
    }
    fclose(f);

    amx_latpost handle;
    amx_latpost_cfg_default(&handle.cfg);
    CHECK(handle.cfg.mode == AMX_LATPOST_LOG && handle.cfg.normalize == 1 && handle.cfg.v_normalized == 1 && handle.cfg.tolerance == 100);
    handle.cfg.mode = AMX_LATPOST_EXPECTATION;
    std::vector<const Lattice*> all, reversed;
    for (const Lattice& l : lats) {
        CHECK(plan_and_compare(&handle, {&l}) == 0);
        all.push_back(&l), reversed.insert(reversed.begin(), &l);
    }
    CHECK(plan_and_compare(&handle, all) == 0);
    CHECK(plan_and_compare(&handle, reversed) == 0);

    // an empty call, NULL outputs
    const long zero[1] = {0};
    CHECK(amx_latpost_plan_host(&handle, 0, zero, zero, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr) == AMX_OK);
    // the refusals, each on the second of three segments: 0 -> 1 -> 2, state 2 final
    auto refuse = [&](int what, const char* text) {
        long    so[4] = {0, 3, 6, 9}, ao[10] = {0, 1, 2, 2, 3, 4, 4, 5, 6, 6};
        int32_t tgt[6] = {1, 2, 1, 2, 1, 2}, ini[3] = {0, 0, 0};
        float   w[6] = {1, 2, 1, 2, 1, 2}, r[6] = {0, 0, 0, 0, 0, 0}, fw[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1}, fr[9] = {0};
        uint8_t ff[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
        const float* risk = r;
        switch (what) {
        case 0: tgt[3] = 1; break;             // 1 -> 1
        case 1: tgt[3] = 0; break;             // 0 -> 1 -> 0
        case 2: tgt[2] = 3; break;
        case 3: ini[1] = 3; break;
        case 4: w[3] = NAN; break;
        case 5: r[2] = NAN; break;
        case 6: fw[5] = NAN; break;
        case 7: risk = nullptr; break;
        case 8: so[2] = 2; break;
        case 9: ao[4] = 1; break;
        }
        int32_t out[9];
        for (int i = 0; i < 9; ++i)
            out[i] = 77;
        g_error.clear();
        const int rc = amx_latpost_plan_host(&handle, 3, so, ao, tgt, w, risk, ini, ff, fw, fr, out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        for (int i = 0; i < 9; ++i)
            if (out[i] != 77)
                return false;
        return rc == AMX_ERR_INVALID && g_error.find(text) != std::string::npos;
    };
    CHECK(refuse(0, "segment 1: state 1 lies on a cycle"));
    CHECK(refuse(1, "segment 1: state"));
    CHECK(refuse(2, "segment 1: arc 0 of state 0 has target 3"));
    CHECK(refuse(3, "segment 1: initial state 3"));
    CHECK(refuse(4, "segment 1: weight of arc 0 of state 1"));
    CHECK(refuse(5, "segment 1: risk of arc 0 of state 0"));
    CHECK(refuse(6, "segment 1: final weight of state 2"));
    CHECK(refuse(7, "needs arc_risk"));
    CHECK(refuse(8, "state_offsets descend"));
    CHECK(refuse(9, "arc_offsets descend"));
    CHECK(amx_latpost_plan_host(nullptr, 0, zero, zero, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr) == AMX_ERR_INVALID);

    // info's flags: the reference's two comparisons on chosen values
    amx_latpost_info info{};
    amx_latpost_cfg  cfg = handle.cfg;
    cfg.mode             = AMX_LATPOST_LOG;
    amx::latpost_fill_info(cfg, 12.5, 12.5, 0.0, &info);
    CHECK(info.flows_agree == 1 && info.vanishing_flow == 0 && info.total_inv == -12.5 && info.total_inv_f32 == -12.5f && info.expectation == 0.f);
    amx::latpost_fill_info(cfg, 12.5, 12.6, 0.0, &info);
    CHECK(info.flows_agree == 0);
    amx::latpost_fill_info(cfg, 1.7976931348623157e+308, 1.7976931348623157e+308, 0.0, &info);   // no path: totalInv clamps at f32 min
    CHECK(info.vanishing_flow == 1 && info.total_inv_f32 == -3.40282347e+38F);
    cfg.mode = AMX_LATPOST_EXPECTATION;
    amx::latpost_fill_info(cfg, 12.5, 12.5 + 100 * 9.5367431640625e-07, 0.75, &info);   // 100 f32 ulps apart: the limit of the ulp comparison
    CHECK(info.flows_agree == 1 && info.expectation == 0.75f);
    amx::latpost_fill_info(cfg, 12.5, 12.5 + 101 * 9.5367431640625e-07, 0.75, &info);
    CHECK(info.flows_agree == 0);
    printf("host_latpost_test: ok (%d lattices)\n", n_cases);
    return 0;
}
