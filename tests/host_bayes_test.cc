// Stand-alone host program for the argument checks of the Bayes classification section of include/amx.h: it compiles
// rasr_amd/csrc/bayes.hip's host side into itself (no librasr_amd.so, no Python), creates handles without a context, walks through every
// refusal and its message, and destroys what it created.  No device call is made: a handle without a context refuses every *_dev entry
// point before it touches HIP.  Meant to be built with the host sanitizers (tests/test_bayes.py does):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -w -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/host_bayes_test.cc -o host_bayes_test && ./host_bayes_test
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../rasr_amd/csrc/bayes.hip"

// what api.cpp and gmm.hip give the library
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
static int g_mixtures = 12;
extern "C" int amx_gmm_n_mixtures(const amx_gmm*) { return g_mixtures; }
extern "C" int amx_gmm_dimension(const amx_gmm*) { return 16; }
extern "C" int amx_gmm_score_dev(amx_gmm*, int, const float*, int, float*, uint32_t*) { return AMX_ERR_STATE; }

static int g_failed = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("%s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, g_error.c_str()); \
            ++g_failed;                                                                 \
        }                                                                               \
    } while (0)

static bool says(const char* what) { return g_error.find(what) != std::string::npos; }

static amx_bayes_cfg cfg_of(int n, long nof, long delay, int wl, int wr) {
    amx_bayes_cfg c;
    amx_bayes_default_cfg(&c);
    c.n_classes = n, c.number_of_features = nof, c.delay = delay, c.window_length = wl, c.window_right = wr;
    return c;
}

int main() {
    amx_bayes_cfg c;
    amx_bayes_default_cfg(&c);
    CHECK(c.n_classes == 0 && c.number_of_features == INT_MAX && c.delay == INT_MAX && c.window_length == -1 && c.window_right == 0 && c.single_frame == 0);
    amx_bayes_default_cfg(nullptr);

    amx_bayes* h = (amx_bayes*)0x1;
    CHECK(amx_bayes_create(nullptr, &c, nullptr) == AMX_ERR_INVALID);
    CHECK(amx_bayes_create(nullptr, nullptr, &h) == AMX_ERR_INVALID && h == nullptr);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_ERR_INVALID && h == nullptr && says("n_classes") && says("Class labels not defined"));
    c = cfg_of(-3, INT_MAX, INT_MAX, -1, 0);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_ERR_INVALID && says("n_classes"));
    c = cfg_of(3, INT_MAX, INT_MAX, 4, 4);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_ERR_INVALID && h == nullptr && says("window_right 4") && says("window_length 4"));
    c = cfg_of(3, INT_MAX, INT_MAX, 4, 9);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_ERR_INVALID && says("window_right"));
    c = cfg_of(3, INT_MAX, INT_MAX, 4, -1);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_ERR_INVALID && says("window_right"));
    c = cfg_of(3, 16, INT_MAX, 4, 0);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_ERR_INVALID && says("number_of_features 16") && says("window_length 4"));
    c = cfg_of(3, 16, 5, -1, 0);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_ERR_INVALID && says("number_of_features 16") && says("delay 5"));
    // window_right is not looked at without a window
    c = cfg_of(3, INT_MAX, INT_MAX, -1, 7);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_OK && h);
    amx_bayes_destroy(h);
    amx_bayes_destroy(nullptr);

    // a handle without a context: configuration and prior, every device entry point refuses
    float prior = 0.f;
    for (int n : {1, 2, 3, 13, 200}) {
        c = cfg_of(n, 0, -1, 0, 0);   // "unset" spelled with the other values the fields allow
        CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_OK && h);
        CHECK(amx_bayes_prior(h, &prior) == AMX_OK && prior == std::log((float)n));
        CHECK(amx_bayes_prior(h, nullptr) == AMX_ERR_INVALID && amx_bayes_prior(nullptr, &prior) == AMX_ERR_INVALID);
        long               off[2] = {0, 4};
        unsigned long long nw[2];
        int32_t            label = 77;
        CHECK(amx_bayes_classify_dev(h, 1, off, nullptr, n, nullptr, &label, nullptr, nullptr, nullptr, nw) == AMX_ERR_STATE && says("without a context"));
        CHECK(label == 77);
        CHECK(amx_bayes_scores_dev(h, 1, off, nullptr, n, nullptr, nullptr, n, nullptr) == AMX_ERR_STATE && says("without a context"));
        CHECK(amx_bayes_classify_gmm_dev(h, (amx_gmm*)0x1, 0, 1, off, nullptr, nullptr, &label, nullptr, nullptr, nullptr, nw) == AMX_ERR_STATE);
        CHECK(amx_bayes_classify_dev(nullptr, 1, off, nullptr, n, nullptr, &label, nullptr, nullptr, nullptr, nw) == AMX_ERR_INVALID);
        CHECK(amx_bayes_scores_dev(nullptr, 1, off, nullptr, n, nullptr, nullptr, n, nullptr) == AMX_ERR_INVALID);
        CHECK(amx_bayes_classify_gmm_dev(h, nullptr, 0, 1, off, nullptr, nullptr, &label, nullptr, nullptr, nullptr, nw) == AMX_ERR_INVALID);
        amx_bayes_destroy(h);
    }
    // windowed and continuous handles are created and destroyed as well
    c = cfg_of(13, INT_MAX, 7, 25, 24);
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_OK);
    amx_bayes_destroy(h);
    c = cfg_of(13, INT_MAX, 0, -1, 0);
    c.single_frame = 1;
    CHECK(amx_bayes_create(nullptr, &c, &h) == AMX_OK);
    amx_bayes_destroy(h);

    std::printf(g_failed ? "host_bayes_test: %d checks FAILED\n" : "host_bayes_test: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
