// Stand-alone host program for the segment plan that the CMLLR and MLLR accumulations share (rasr_amd/csrc/key_plan.hpp): it calls
// amx::plan_keys alone (no device is touched), so that tests/test_keyplan.py can run it under the host sanitizers.  Every table lives in
// a heap block of exactly its size, so that a read past an end is seen.
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/key_plan.hpp"

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

#define CHECK(cond)                                                                                                  \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            printf("host_keyplan_test: line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_error.c_str());    \
            return 1;                                                                                                \
        }                                                                                                            \
    } while (0)

static bool segs_are(const amx::KeyPlan& p, std::vector<std::pair<long long, long long>> want) {
    if (p.segs.size() != want.size())
        return false;
    for (size_t i = 0; i < want.size(); ++i)
        if (p.segs[i].begin != want[i].first || p.segs[i].end != want[i].second)
            return false;
    return true;
}

int main() {
    // 5 segments on 3 keys: segment 1 is empty, key 1 has no segment, the two segments of key 0 and of key 2 are not adjacent
    const std::vector<long> off = {10, 14, 14, 20, 23, 30};
    const std::vector<int>  key = {2, 0, 0, 2, 0};
    amx::KeyPlan            p;
    CHECK(amx::plan_keys("who", 5, off.data(), key.data(), 3, true, &p) == AMX_OK);
    CHECK(p.t0 == 10 && p.n == 20);
    CHECK((p.key_tab == std::vector<int>{0, 2, 2, 4, /* key_base */ 0, 13, 13}));
    CHECK(segs_are(p, {{14, 20}, {23, 30}, {10, 14}, {20, 23}}));
    CHECK(amx::plan_keys("who", 5, off.data(), key.data(), 3, false, &p) == AMX_OK);
    CHECK((p.key_tab == std::vector<int>{0, 2, 2, 4}) && p.t0 == 10 && p.n == 20);
    CHECK(segs_are(p, {{14, 20}, {23, 30}, {10, 14}, {20, 23}}));

    // nothing to do: no segment (no table is read), no frame
    CHECK(amx::plan_keys("who", 0, nullptr, nullptr, 3, true, &p) == AMX_OK && p.n == 0 && p.segs.empty() && p.key_tab.empty());
    const std::vector<long> none = {7, 7, 7};
    CHECK(amx::plan_keys("who", 2, none.data(), key.data(), 3, true, &p) == AMX_OK && p.n == 0 && p.segs.empty());

    // the refusals: status and text, under the caller's name; a refused call leaves an empty plan
    std::vector<long> down = off;
    down[3] = 13;
    CHECK(amx::plan_keys("who", 5, down.data(), key.data(), 3, true, &p) == AMX_ERR_INVALID);
    CHECK(g_error == "who: frame_offsets decrease at segment 2 (13 after 14)" && p.n == 0 && p.segs.empty());
    std::vector<int> far = key;
    far[3]               = 3;
    CHECK(amx::plan_keys("who", 5, off.data(), far.data(), 3, true, &p) == AMX_ERR_INVALID && g_error == "who: segment 3: key 3 is outside [0, 3)");
    far[3] = -1;
    CHECK(amx::plan_keys("me", 5, off.data(), far.data(), 3, false, &p) == AMX_ERR_INVALID && g_error == "me: segment 3: key -1 is outside [0, 3)");
    std::vector<long> neg = off;
    neg[0]                = -1;
    CHECK(amx::plan_keys("who", 5, neg.data(), key.data(), 3, true, &p) == AMX_ERR_INVALID && g_error == "who: frame_offsets[0] = -1 is negative");
    const std::vector<long> cap = {5, 5 + (1l << 30)}, below = {5, 5 + (1l << 30) - 1};
    CHECK(amx::plan_keys("who", 1, cap.data(), key.data(), 3, true, &p) == AMX_ERR_INVALID);
    CHECK(g_error == "who: 1073741824 frames are more than one call takes" && p.n == 0);
    CHECK(amx::plan_keys("who", 1, below.data(), key.data(), 3, true, &p) == AMX_OK && p.n == (1ll << 30) - 1 && segs_are(p, {{5, 5 + (1ll << 30) - 1}}));
    CHECK((p.key_tab == std::vector<int>{0, 0, 0, 1, 0, 0, 0}));
    CHECK(amx::plan_keys("who", 5, nullptr, key.data(), 3, true, &p) == AMX_ERR_INVALID && g_error == "who: NULL frame_offsets or seg_key");
    CHECK(amx::plan_keys("who", 5, off.data(), nullptr, 3, true, &p) == AMX_ERR_INVALID && g_error == "who: NULL frame_offsets or seg_key");
    printf("host_keyplan_test: ok\n");
    return 0;
}
