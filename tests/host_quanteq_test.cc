// Stand-alone host program for the host side of the quantile equalisation section of include/amx.h: it compiles
// rasr_amd/csrc/quanteq.hip's host side into itself (no librasr_amd.so, no Python), builds the grid tables, writes and reads quantile
// files (with and without pooling, short and missing files), walks through every refusal of create and of the *_dev entry points of a
// handle without a context, and destroys what it created.  No device call is made.  Meant to be built with the host sanitizers
// (tests/test_quanteq.py does):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -w -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/host_quanteq_test.cc -o host_quanteq_test && ./host_quanteq_test <directory>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/quanteq.hip"

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

static std::vector<float> grid_of(const amx_quanteq* h, int which) {
    int n = 0;
    CHECK(amx_quanteq_grid(h, which, &n, nullptr) == AMX_OK);
    std::vector<float> v((size_t)n);
    CHECK(amx_quanteq_grid(h, which, &n, v.data()) == AMX_OK);
    return v;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    const int         dim = 5, nq = 4;
    amx_quanteq_cfg   c;
    amx_quanteq_default_cfg(&c);
    CHECK(c.number_of_quantiles == 4 && c.pool_quantiles == 1 && c.length == INT_MAX && c.right == INT_MAX);
    std::vector<float> tq((size_t)(nq + 1) * dim, 1.f);
    amx_quanteq*       h = nullptr;

    // grid tables: 201 x 201 and 101 points, the last values those of an accumulating f32 loop variable
    CHECK(amx_quanteq_create(nullptr, dim, &c, tq.data(), &h) == AMX_OK && h);
    const std::vector<float> ga = grid_of(h, 0), gg = grid_of(h, 1), gl = grid_of(h, 2);
    CHECK(ga.size() == 201 && gg.size() == 201 && gl.size() == 101);
    CHECK(ga.front() == 0.f && gg.front() == 1.f && gl.front() == 0.f);
    CHECK(ga.back() == 0.9999992f && gg.back() == 2.999998f);
    CHECK(ga[1] == 0.005f && gg[1] == (float)(1.0 + (double)0.01f));
    int n = 0;
    CHECK(amx_quanteq_grid(h, 3, &n, nullptr) == AMX_ERR_INVALID && says("grid 3"));
    CHECK(amx_quanteq_grid(nullptr, 0, &n, nullptr) == AMX_ERR_INVALID);

    // a handle without a context refuses to run, before it looks at its buffers
    const long off[2] = {0, 4};
    CHECK(amx_quanteq_apply_dev(h, 1, off, nullptr, dim, nullptr, dim, nullptr) == AMX_ERR_STATE && says("without a context"));
    CHECK(amx_quanteq_estimate_dev(h, 1, off, nullptr, dim) == AMX_ERR_STATE);
    double             sums[(nq + 1) * dim];
    unsigned long long count = 7;
    CHECK(amx_quanteq_estimate_result(h, sums, &count) == AMX_ERR_STATE && says("estimate = 1"));
    amx_quanteq_destroy(h);
    amx_quanteq_destroy(nullptr);

    // refusals of create, each naming its parameter
    struct { const char* word; void (*set)(amx_quanteq_cfg&); } bad[] = {
        {"length", [](amx_quanteq_cfg& k) { k.length = 100; }},
        {"right", [](amx_quanteq_cfg& k) { k.right = 0; }},
        {"piecewise_linear", [](amx_quanteq_cfg& k) { k.piecewise_linear = 1; }},
        {"delta_alpha", [](amx_quanteq_cfg& k) { k.delta_alpha = 0.f; }},
        {"delta_alpha", [](amx_quanteq_cfg& k) { k.delta_alpha = 1e-6f; }},
        {"delta_gamma", [](amx_quanteq_cfg& k) { k.delta_gamma = -1.f; }},
        {"delta_lambda_and_rho", [](amx_quanteq_cfg& k) { k.delta_lambda_and_rho = 0.f; }},
        {"number_of_quantiles", [](amx_quanteq_cfg& k) { k.number_of_quantiles = 0; }},
        {"number_of_quantiles", [](amx_quanteq_cfg& k) { k.number_of_quantiles = AMX_QUANTEQ_MAX_QUANTILES + 1; }},
    };
    for (const auto& b : bad) {
        amx_quanteq_cfg k = c;
        b.set(k);
        h = (amx_quanteq*)1;
        CHECK(amx_quanteq_create(nullptr, dim, &k, tq.data(), &h) == AMX_ERR_UNSUPPORTED && says(b.word) && h == nullptr);
    }
    CHECK(amx_quanteq_create(nullptr, 0, &c, tq.data(), &h) == AMX_ERR_INVALID && says("dim"));
    CHECK(amx_quanteq_create(nullptr, dim, &c, nullptr, &h) == AMX_ERR_INVALID && says("training_quantiles"));
    CHECK(amx_quanteq_create(nullptr, dim, nullptr, tq.data(), &h) == AMX_ERR_INVALID);
    CHECK(amx_quanteq_create(nullptr, dim, &c, tq.data(), nullptr) == AMX_ERR_INVALID);
    {
        amx_quanteq_cfg k = c;
        k.delta_alpha = 0.25f, k.delta_gamma = 0.5f, k.delta_lambda_and_rho = 0.25f;   // exact steps reach the upper end
        CHECK(amx_quanteq_create(nullptr, dim, &k, tq.data(), &h) == AMX_OK);
        CHECK(grid_of(h, 0).size() == 5 && grid_of(h, 1).size() == 5 && grid_of(h, 2).size() == 3 && grid_of(h, 1).back() == 3.f);
        amx_quanteq_destroy(h);
        k = c;
        k.estimate = 1;
        CHECK(amx_quanteq_create(nullptr, dim, &k, nullptr, &h) == AMX_OK);
        CHECK(amx_quanteq_estimate_result(h, sums, &count) == AMX_OK && count == 0 && sums[0] == 0.0);
        CHECK(amx_quanteq_apply_dev(h, 1, off, nullptr, dim, nullptr, dim, nullptr) == AMX_ERR_STATE);
        amx_quanteq_destroy(h);
    }

    // files: the writer's text, the reader, pooling in f32 in channel order, short and missing files
    for (int i = 0; i <= nq; ++i)
        for (int d = 0; d < dim; ++d)
            sums[i * dim + d] = 3.0 * (0.1 + i + 0.37 * d);
    const std::string path = dir + "/host_quanteq_test_quantiles.txt";
    CHECK(amx_quanteq_quantiles_write(path.c_str(), dim, nq, sums, 3) == AMX_OK);
    {
        FILE* f = fopen(path.c_str(), "rb");
        CHECK(f != nullptr);
        char        text[4096] = {0};
        const size_t got = f ? fread(text, 1, sizeof text - 1, f) : 0;
        if (f)
            fclose(f);
        std::string want;
        for (int d = 0; d < dim; ++d) {
            char line[256];
            int  k = snprintf(line, sizeof line, "%i ", d);
            for (int i = 0; i <= nq; ++i)
                k += snprintf(line + k, sizeof line - k, "%f ", sums[i * dim + d] / 3u);
            want += line;
            want += "\n";
        }
        CHECK(std::string(text, got) == want);
    }
    std::vector<float> plain((size_t)(nq + 1) * dim, -1.f), pooled(plain);
    CHECK(amx_quanteq_quantiles_read(path.c_str(), dim, nq, 0, plain.data()) == AMX_OK);
    CHECK(amx_quanteq_quantiles_read(path.c_str(), dim, nq, 1, pooled.data()) == AMX_OK);
    for (int i = 0; i <= nq; ++i) {
        float average = 0.f;
        for (int d = 0; d < dim; ++d) {
            char text[64];
            snprintf(text, sizeof text, "%f", sums[i * dim + d] / 3u);
            CHECK(plain[i * dim + d] == strtof(text, nullptr));
            average += plain[i * dim + d];
        }
        average /= (float)dim;
        for (int d = 0; d < dim; ++d)
            CHECK(pooled[i * dim + d] == average);
    }
    std::vector<float> wider((size_t)(nq + 1) * (dim + 1));
    CHECK(amx_quanteq_quantiles_read(path.c_str(), dim + 1, nq, 1, wider.data()) == AMX_ERR_INVALID && says("does not hold"));   // a short file
    CHECK(amx_quanteq_quantiles_read((dir + "/no_such_file.txt").c_str(), dim, nq, 1, plain.data()) == AMX_ERR_INVALID && says("Can't open"));
    CHECK(amx_quanteq_quantiles_write((dir + "/no_such_directory/q.txt").c_str(), dim, nq, sums, 3) == AMX_ERR_INVALID && says("Can't open"));
    CHECK(amx_quanteq_quantiles_write(path.c_str(), dim, nq, sums, 1ull << 32) == AMX_ERR_INVALID && says("u32"));
    CHECK(amx_quanteq_quantiles_read(nullptr, dim, nq, 1, plain.data()) == AMX_ERR_INVALID);
    remove(path.c_str());

    if (g_failed) {
        std::printf("host_quanteq_test: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("host_quanteq_test: ok\n");
    return 0;
}
