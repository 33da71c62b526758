// Stand-alone host program for the host side of the EBW section of include/amx.h: it compiles ebw_host.cpp into a program of its own (no
// device is touched), so that tests/test_ebw.py can run it under the host sanitizers.
//   host_ebw_test case.bin directory
// case.bin (written by the test): int32 dim, n_mix, n_dens, n_mean, n_cov | u32 mix_offsets [n_mix + 1], dens_index, dens_mean, dens_cov |
// f64 accumulator, a second accumulator, their sum; directory/want.acc holds the restatement's bytes of the first accumulator's file.
// The estimate runs on statistics made here (both contracts, with and without i-smoothing, every refusal, removal to one density).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/ebw_host.cpp"

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
            printf("host_ebw_test: line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_error.c_str());        \
            return 1;                                                                                                \
        }                                                                                                            \
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
    const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

template<class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        printf("usage: host_ebw_test case.bin directory\n");
        return 2;
    }
    const std::string dir = argv[2];
    FILE*             f   = fopen(argv[1], "rb");
    CHECK(f);
    std::vector<int> head;
    CHECK(take(f, head, 5));
    const int             dim = head[0], n_mix = head[1], n_dens = head[2], n_mean = head[3], n_cov = head[4];
    std::vector<uint32_t> mix_off, dens_index, dens_mean, dens_cov;
    CHECK(take(f, mix_off, (size_t)n_mix + 1));
    CHECK(take(f, dens_index, (size_t)mix_off[(size_t)n_mix]));
    CHECK(take(f, dens_mean, (size_t)n_dens));
    CHECK(take(f, dens_cov, (size_t)n_dens));
    amx_gmm_model t{};
    t.dim = dim, t.n_mix = n_mix, t.n_dens = n_dens, t.n_mean = n_mean, t.n_cov = n_cov;
    t.mix_offsets = mix_off.data(), t.dens_index = dens_index.data(), t.dens_mean = dens_mean.data(), t.dens_cov = dens_cov.data();
    const long size = amx_ebw_topology_accumulator_size(&t);
    CHECK(size == 2 * ((long)mix_off[(size_t)n_mix] + (long)(n_mean + n_cov) * (1 + dim)) + 1);
    std::vector<double> acc, add, sum;
    CHECK(take(f, acc, (size_t)size) && take(f, add, (size_t)size) && take(f, sum, (size_t)size));
    fclose(f);

    // the file: the restatement's bytes, and back
    const std::string path = dir + "/got.acc";
    CHECK(amx_ebw_accumulator_write(&t, acc.data(), path.c_str()) == AMX_OK);
    const std::vector<unsigned char> want = slurp(dir + "/want.acc"), got = slurp(path);
    CHECK(!want.empty() && want == got);
    std::vector<double> back((size_t)size, -1.0);
    CHECK(amx_ebw_accumulator_read(&t, path.c_str(), back.data()) == AMX_OK && same_bits(back, acc));

    // every truncation is refused and leaves the buffer as it was; so does a byte too many
    const std::vector<double> mark((size_t)size, 3.25);
    const std::string         cut = dir + "/cut.acc";
    for (size_t n = 0; n < got.size(); ++n) {
        std::vector<double> buf = mark;
        CHECK(spill(cut, got.data(), n));
        CHECK(amx_ebw_accumulator_read(&t, cut.c_str(), buf.data()) == AMX_ERR_INVALID && same_bits(buf, mark));
    }
    {
        std::vector<unsigned char> more = got;
        more.push_back(0);
        std::vector<double> buf = mark;
        CHECK(spill(cut, more.data(), more.size()));
        CHECK(amx_ebw_accumulator_read(&t, cut.c_str(), buf.data()) == AMX_ERR_INVALID && same_bits(buf, mark));
        CHECK(g_error.find("bytes behind the objective") != std::string::npos);
    }

    // mismatched topologies: another dimension, another count of every kind, another index, a density outside the model
    {
        std::vector<double> big((size_t)size * 2 + 64, 3.25);
        amx_gmm_model       o = t;
        o.dim                 = dim + 1;
        CHECK(amx_ebw_accumulator_read(&o, path.c_str(), big.data()) == AMX_ERR_INVALID && g_error.find("dimension differs") != std::string::npos);
        o = t, o.n_mean = n_mean + 1;
        std::vector<uint32_t> none;
        CHECK(amx_ebw_accumulator_read(&o, path.c_str(), big.data()) == AMX_ERR_INVALID);
        o = t, o.n_cov = n_cov + 1;
        CHECK(amx_ebw_accumulator_read(&o, path.c_str(), big.data()) == AMX_ERR_INVALID);
        std::vector<uint32_t> dm = dens_mean;
        if (n_mean > 1) {
            dm[0] = dm[0] == 0 ? 1 : 0;
            o = t, o.dens_mean = dm.data();
            CHECK(amx_ebw_accumulator_read(&o, path.c_str(), big.data()) == AMX_ERR_INVALID && g_error.find("topology differs") != std::string::npos);
        }
        std::vector<uint32_t> di = dens_index;
        di[0]                    = (uint32_t)n_dens;
        o = t, o.dens_index = di.data();
        CHECK(amx_ebw_accumulator_read(&o, path.c_str(), big.data()) == AMX_ERR_INVALID && g_error.find("entry 0") != std::string::npos);
        CHECK(amx_ebw_accumulator_write(&o, acc.data(), cut.c_str()) == AMX_ERR_INVALID);
        std::vector<uint32_t> mo = mix_off;
        if (n_mix > 1) {
            mo[1] = mo[2] + 1;
            o = t, o.mix_offsets = mo.data();
            CHECK(amx_ebw_accumulator_write(&o, acc.data(), cut.c_str()) == AMX_ERR_INVALID && g_error.find("mix_offsets decrease") != std::string::npos);
        }
        for (double v : big)
            CHECK(v == 3.25);
        CHECK(amx_ebw_topology_accumulator_size(nullptr) == 0);
        CHECK(amx_ebw_accumulator_read(&t, (dir + "/missing").c_str(), big.data()) == AMX_ERR_INVALID);
        CHECK(amx_ebw_accumulator_write(&t, nullptr, cut.c_str()) == AMX_ERR_INVALID);
    }

    // combine
    {
        std::vector<double> a = acc;
        CHECK(amx_ebw_accumulator_combine(&t, a.data(), add.data()) == AMX_OK && same_bits(a, sum));
        std::vector<double> bad = add;
        bad.back()              = NAN;
        a                       = acc;
        CHECK(amx_ebw_accumulator_combine(&t, a.data(), bad.data()) == AMX_ERR_INVALID && same_bits(a, acc));
        CHECK(amx_ebw_accumulator_combine(&t, a.data(), nullptr) == AMX_ERR_INVALID);
    }
    // the estimate: statistics of 10 numerator and 4 denominator observations per density around previous means, every refusal, and
    // removal down to one density per mixture
    {
        const long nk = mix_off[(size_t)n_mix], block = nk + (long)(n_mean + n_cov) * (1 + dim);
        std::vector<float>  pmeans((size_t)n_mean * dim), pvars((size_t)n_cov * dim, 1.5f);
        std::vector<double> plogw((size_t)nk), st((size_t)size, 0.0);
        for (size_t i = 0; i < pmeans.size(); ++i)
            pmeans[i] = 0.25f * (float)(i % 7) - 0.5f;
        for (int m = 0; m < n_mix; ++m)
            for (uint32_t k = mix_off[(size_t)m]; k < mix_off[(size_t)m + 1]; ++k)
                plogw[k] = -std::log((double)(mix_off[(size_t)m + 1] - mix_off[(size_t)m]));
        for (long k = 0; k < nk; ++k) {
            const uint32_t d = dens_index[(size_t)k], j = dens_mean[d], c = dens_cov[d];
            for (int side = 0; side < 2; ++side) {
                double*      b = st.data() + side * block;
                const double w = side ? 4.0 : 10.0 + (double)k, shift = side ? 0.3 : 0.05;
                b[k] += w, b[nk + j] += w, b[nk + (long)n_mean * (1 + dim) + c] += w;
                for (int i = 0; i < dim; ++i) {
                    const double x = (double)pmeans[(size_t)j * dim + i] + shift;
                    b[nk + n_mean + (long)j * dim + i] += w * x;
                    b[nk + (long)n_mean * (1 + dim) + n_cov + (long)c * dim + i] += w * (x * x + 1.2);
                }
            }
        }
        amx_gmm_model prev = t;
        prev.log_weight = plogw.data(), prev.means = pmeans.data(), prev.variances = pvars.data();
        amx_ebw_estimate_cfg cfg;
        amx_ebw_estimate_cfg_default(&cfg);
        amx_ebw_estimate_info info;
        std::vector<double>   icd((size_t)n_mean, -1.0);
        amx_mixture_set*      ms = nullptr;
        for (int contract = 0; contract < 2; ++contract)
            for (int with_i = 0; with_i < 2; ++with_i) {
                cfg.contract = contract, cfg.i_smoothing_means = 2.0, cfg.i_smoothing_weights = 1.0;
                CHECK(amx_ebw_estimate(&t, st.data(), &prev, with_i ? &prev : nullptr, &cfg, &ms, &info, icd.data()) == AMX_OK && ms);
                CHECK((int)ms->mix_off.size() == n_mix + 1 && ms->means.size() == ms->dens_mean.size() * (size_t)dim && ms->dim == dim);
                CHECK(ms->log_weight.size() == ms->dens_index.size() && info.sigma_minimum > 0);
                for (float v : ms->variances)
                    CHECK(v > 0);
                delete ms, ms = nullptr;
            }
        cfg.min_observation_weight = 1e9;   // every density but the heaviest of its mixture goes
        CHECK(amx_ebw_estimate(&t, st.data(), &prev, nullptr, &cfg, &ms, &info, nullptr) == AMX_OK && ms);
        CHECK((int)ms->dens_index.size() == n_mix && info.n_removed == (int)nk - n_mix);
        for (int m = 0; m < n_mix; ++m)
            CHECK(ms->mix_off[(size_t)m + 1] - ms->mix_off[(size_t)m] == 1 && ms->log_weight[(size_t)m] == 0.0);
        delete ms, ms = nullptr;
        amx_ebw_estimate_cfg_default(&cfg);
        cfg.iteration_constants = AMX_EBW_IC_CAMBRIDGE;
        CHECK(amx_ebw_estimate(&t, st.data(), &prev, nullptr, &cfg, &ms, nullptr, nullptr) == AMX_ERR_UNSUPPORTED && !ms && g_error.find("cambridge") != std::string::npos);
        amx_ebw_estimate_cfg_default(&cfg);
        cfg.estimator = AMX_EBW_ESTIMATOR_RPROP;
        CHECK(amx_ebw_estimate(&t, st.data(), &prev, nullptr, &cfg, &ms, nullptr, nullptr) == AMX_ERR_UNSUPPORTED && !ms);
        amx_ebw_estimate_cfg_default(&cfg);
        amx_gmm_model other = prev;
        other.n_cov         = n_cov + 1;
        CHECK(amx_ebw_estimate(&t, st.data(), &other, nullptr, &cfg, &ms, nullptr, nullptr) == AMX_ERR_INVALID && !ms && g_error.find("differs in topology") != std::string::npos);
        CHECK(amx_ebw_estimate(&t, st.data(), nullptr, nullptr, &cfg, &ms, nullptr, nullptr) == AMX_ERR_INVALID && !ms);
        std::vector<double> nan = st;
        nan[3]                  = NAN;
        CHECK(amx_ebw_estimate(&t, nan.data(), &prev, nullptr, &cfg, &ms, nullptr, nullptr) == AMX_ERR_INVALID && !ms && g_error.find("entry 3") != std::string::npos);
        // the random accumulators of the file test carry negative weights: whatever the estimate says, it hands out a set or nothing
        const int r = amx_ebw_estimate(&t, acc.data(), &prev, nullptr, &cfg, &ms, nullptr, nullptr);
        CHECK((r == AMX_OK) == (ms != nullptr) && (r == AMX_OK || r == AMX_ERR_INVALID));
        delete ms;
    }
    printf("host_ebw_test: ok\n");
    return 0;
}
