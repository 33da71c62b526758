// Stand-alone host program for the host side of the constrained MLLR section of include/amx.h: it compiles cmllr_host.cpp into a
// program of its own (no device is touched), so that tests/test_cmllr.py can run it under the host sanitizers.
//   host_cmllr_test cases.bin directory bar_abs bar_rel min_obs
// cases.bin (written by the test from tests/golden/ref_cmllr.npz), per case: int32 F, M, pooled, iterations, initial columns (0: none) |
// f32 variance [M] when pooled | f64 key 0 | f64 key 2 | f32 initial [M x columns] | f64 the reference's mmi-prime transform [M x (F + 1)];
// directory/key0_<F>.acc holds the reference's accumulator file of key 0.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/cmllr_host.cpp"

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

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            printf("host_cmllr_test: line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_error.c_str()); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

static std::vector<unsigned char> slurp(const std::string& path) {
    std::vector<unsigned char> out;
    FILE*                      f = fopen(path.c_str(), "rb");
    if (!f)
        return out;
    unsigned char buf[4096];
    size_t        n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0)
        out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

static bool spill(const std::string& path, const unsigned char* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f)
        return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        printf("usage: host_cmllr_test cases.bin directory bar_abs bar_rel min_obs\n");
        return 2;
    }
    const std::string dir = argv[2];
    const double      bar_abs = atof(argv[3]), bar_rel = atof(argv[4]), min_obs = atof(argv[5]);
    FILE*             in = fopen(argv[1], "rb");
    CHECK(in);
    int               n_cases = 0;
    amx_cmllr_shape   full{}, pooled{};
    std::vector<float>  pooled_var;
    std::vector<double> full_acc, pooled_acc;
    for (;;) {
        int32_t head[5];
        if (fread(head, 4, 5, in) != 5)
            break;
        ++n_cases;
        amx_cmllr_shape s{head[0], head[1], 3, head[2]};
        const int       F = s.feature_dim, M = s.model_dim, R = F + 1, iterations = head[3], cols = head[4];
        const long      size = amx_cmllr_key_size(&s);
        CHECK(size > 0);
        std::vector<float> var((size_t)M), initial((size_t)M * cols);
        if (s.pooled)
            CHECK(fread(var.data(), 4, (size_t)M, in) == (size_t)M);
        const float*        v = s.pooled ? var.data() : nullptr;
        std::vector<double> key0((size_t)size), key2((size_t)size), ref((size_t)M * R);
        CHECK(fread(key0.data(), 8, (size_t)size, in) == (size_t)size && fread(key2.data(), 8, (size_t)size, in) == (size_t)size);
        if (cols)
            CHECK(fread(initial.data(), 4, initial.size(), in) == initial.size());
        CHECK(fread(ref.data(), 8, ref.size(), in) == ref.size());

        // files: the reference's bytes, read back to the same bits; truncations and a wrong tag are refused and leave `back` alone
        const std::string path = dir + "/host_test.acc";
        CHECK(amx_cmllr_accumulator_write(&s, v, key0.data(), path.c_str()) == AMX_OK);
        const std::vector<unsigned char> bytes = slurp(path), want = slurp(dir + "/key0_" + std::to_string(F) + ".acc");
        CHECK(!bytes.empty() && bytes == want);
        std::vector<double> back((size_t)size, -1.0);
        CHECK(amx_cmllr_accumulator_read(&s, v, path.c_str(), back.data()) == AMX_OK);
        CHECK(memcmp(back.data(), key0.data(), (size_t)size * 8) == 0);
        const size_t cuts[] = {0, 3, 39, 40, 52, bytes.size() / 3, bytes.size() / 2, bytes.size() - 9, bytes.size() - 1};
        for (size_t cut : cuts) {
            CHECK(spill(path, bytes.data(), cut));
            std::fill(back.begin(), back.end(), -1.0);
            CHECK(amx_cmllr_accumulator_read(&s, v, path.c_str(), back.data()) == AMX_ERR_INVALID);
            CHECK(back[0] == -1.0 && back[(size_t)size - 1] == -1.0);
        }
        std::vector<unsigned char> bad = bytes;
        bad[10] ^= 1;
        CHECK(spill(path, bad.data(), bad.size()));
        CHECK(amx_cmllr_accumulator_read(&s, v, path.c_str(), back.data()) == AMX_ERR_INVALID && g_error.find("type tag") != std::string::npos);
        amx_cmllr_shape other = s;
        other.feature_dim += 1;
        CHECK(spill(path, bytes.data(), bytes.size()));
        std::vector<double> big((size_t)amx_cmllr_key_size(&other));
        CHECK(amx_cmllr_accumulator_read(&other, v, path.c_str(), big.data()) == AMX_ERR_INVALID);
        CHECK(amx_cmllr_accumulator_read(&s, v, (dir + "/missing.acc").c_str(), back.data()) == AMX_ERR_INVALID);

        // combine: member by member, the product rounded first
        std::vector<double> sum = key0;
        CHECK(amx_cmllr_combine(&s, v, sum.data(), &s, v, key2.data(), 0.5) == AMX_OK);
        for (long c = 0; c < size; ++c) {
            const double p = key2[(size_t)c] * 0.5;
            CHECK(sum[(size_t)c] == key0[(size_t)c] + p);
        }
        CHECK(amx_cmllr_combine(&s, v, sum.data(), &other, v, big.data(), 1.0) == AMX_ERR_INVALID);

        // estimate: within the measured bar of the reference's text; the early return below min-observation-weight
        std::vector<float>  t32((size_t)M * R);
        std::vector<double> t64((size_t)M * R), its((size_t)iterations * M * R);
        int                 estimated = -1;
        const float*        ini = cols ? initial.data() : nullptr;
        CHECK(amx_cmllr_estimate(&s, v, key0.data(), iterations, min_obs, AMX_CMLLR_MMI_PRIME, ini, cols, t32.data(), t64.data(), its.data(), &estimated) ==
              AMX_OK);
        CHECK(estimated == 1);
        double d = 0, scale = 0;
        for (size_t e = 0; e < ref.size(); ++e) {
            d     = std::fmax(d, std::fabs(t64[e] - ref[e]));
            scale = std::fmax(scale, std::fabs(ref[e]));
            CHECK(t32[e] == (float)t64[e] && its[(size_t)(iterations - 1) * M * R + e] == t64[e]);
        }
        CHECK(d <= bar_abs && d <= bar_rel * scale);
        CHECK(amx_cmllr_estimate(&s, v, key2.data(), iterations, min_obs, AMX_CMLLR_MMI_PRIME, ini, cols, t32.data(), nullptr, nullptr, &estimated) == AMX_OK);
        CHECK(estimated == 0);
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < R; ++j) {
                const float w = cols == 0 ? (j == i + 1 ? 1.f : 0.f) : (cols == F ? (j == 0 ? 0.f : initial[(size_t)i * cols + j - 1]) : initial[(size_t)i * cols + j]);
                CHECK(t32[(size_t)i * R + j] == w);
            }
        double score = 0, score2 = 0;
        CHECK(amx_cmllr_estimate(&s, v, key0.data(), 1, 0.0, AMX_CMLLR_NAIVE, nullptr, 0, t32.data(), nullptr, nullptr, nullptr) == AMX_OK);
        CHECK(amx_cmllr_score(&s, v, key0.data(), t32.data(), AMX_CMLLR_NAIVE, &score) == AMX_OK && std::isfinite(score));
        CHECK(amx_cmllr_score(&s, v, key0.data(), t32.data(), AMX_CMLLR_MMI_PRIME, &score2) == AMX_OK && std::isfinite(score2));

        // the transform file: written, read back to the file's values, a truncation refused
        const std::string tpath = dir + "/host_test.matrix";
        CHECK(amx_cmllr_transform_write(tpath.c_str(), M, R, t32.data()) == AMX_OK);
        int    tr = 0, tc = 0;
        float* tback = nullptr;
        CHECK(amx_cmllr_transform_read(tpath.c_str(), &tr, &tc, &tback) == AMX_OK && tr == M && tc == R && tback);
        for (size_t e = 0; e < t32.size(); ++e) {
            char text[32];
            snprintf(text, sizeof text, "%e", (double)t32[e]);
            CHECK(tback[e] == strtof(text, nullptr));
        }
        free(tback);
        const std::vector<unsigned char> tbytes = slurp(tpath);
        CHECK(spill(tpath, tbytes.data(), tbytes.size() - 5));
        tback = (float*)1;
        CHECK(amx_cmllr_transform_read(tpath.c_str(), &tr, &tc, &tback) == AMX_ERR_INVALID && tback == nullptr);
        t32[1] = INFINITY;
        CHECK(amx_cmllr_transform_write(tpath.c_str(), M, R, t32.data()) == AMX_ERR_INVALID);
        t32[1] = 0.f;

        // refusals
        CHECK(amx_cmllr_estimate(&s, v, key0.data(), 1, 0.0, AMX_CMLLR_HLDA, nullptr, 0, t32.data(), nullptr, nullptr, nullptr) == AMX_ERR_UNSUPPORTED);
        CHECK(g_error.find("hlda") != std::string::npos);
        CHECK(amx_cmllr_score(&s, v, key0.data(), t32.data(), AMX_CMLLR_HLDA, &score) == AMX_ERR_UNSUPPORTED);
        CHECK(amx_cmllr_estimate(&s, v, key0.data(), 1, 0.0, 7, nullptr, 0, t32.data(), nullptr, nullptr, nullptr) == AMX_ERR_INVALID);
        CHECK(amx_cmllr_estimate(&s, v, key0.data(), 1, 0.0, AMX_CMLLR_NAIVE, t32.data(), F - 1, t32.data(), nullptr, nullptr, nullptr) == AMX_ERR_INVALID);
        CHECK(amx_cmllr_estimate(&s, v, nullptr, 1, 0.0, AMX_CMLLR_NAIVE, nullptr, 0, t32.data(), nullptr, nullptr, nullptr) == AMX_ERR_INVALID);
        std::vector<double> zeros((size_t)size, 0.0);
        CHECK(amx_cmllr_estimate(&s, v, zeros.data(), 1, 0.0, AMX_CMLLR_NAIVE, nullptr, 0, t32.data(), nullptr, nullptr, nullptr) == AMX_ERR_INVALID);
        CHECK(g_error.find("singular") != std::string::npos);
        amx_cmllr_shape small = s;
        small.feature_dim     = M - 1;
        CHECK(amx_cmllr_key_size(&small) == 0);
        CHECK(amx_cmllr_score(&small, v, key0.data(), t32.data(), AMX_CMLLR_NAIVE, &score) == AMX_ERR_INVALID && g_error.find("smaller than model_dim") != std::string::npos);
        if (s.pooled)
            CHECK(amx_cmllr_score(&s, nullptr, key0.data(), t32.data(), AMX_CMLLR_NAIVE, &score) == AMX_ERR_INVALID);
        (s.pooled ? pooled : full)         = s;
        (s.pooled ? pooled_acc : full_acc) = key0;
        if (s.pooled)
            pooled_var = var;
    }
    fclose(in);
    CHECK(n_cases == 2 && full.model_dim > 0 && pooled.model_dim > 0);
    // combine of a pooled with a non-pooled accumulator, and of unequal variance vectors
    amx_cmllr_shape as_full = pooled;
    as_full.pooled          = 0;
    std::vector<double> wide((size_t)amx_cmllr_key_size(&as_full), 0.0);
    CHECK(amx_cmllr_combine(&pooled, pooled_var.data(), pooled_acc.data(), &as_full, nullptr, wide.data(), 1.0) == AMX_ERR_INVALID);
    CHECK(g_error.find("non-pooled") != std::string::npos);
    std::vector<float> other_var = pooled_var;
    other_var[0] *= 2.f;
    std::vector<double> copy = pooled_acc;
    CHECK(amx_cmllr_combine(&pooled, pooled_var.data(), copy.data(), &pooled, other_var.data(), pooled_acc.data(), 1.0) == AMX_ERR_INVALID);
    CHECK(g_error.find("variances differ") != std::string::npos && copy == pooled_acc);
    printf("host_cmllr_test: ok (%d cases)\n", n_cases);
    return 0;
}
