// Stand-alone host program for the host side of the "NN training statistics" section of include/amx.h: it compiles
// rasr_amd/csrc/nntrain.hip's host side into itself (no librasr_amd.so, no Python), creates handles without a context, walks through
// every create-time refusal and its message, checks the layout of the flat buffer under every statistics mask, and sends a buffer
// through write, read and combine, a truncated file included.  No device call is made: a handle without a context refuses
// amx_nntrain_accumulate_dev before it touches HIP.  Meant to be built with the host sanitizers (tests/test_nntrain.py does):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -w -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/host_nntrain_test.cc -o host_nntrain_test && ./host_nntrain_test <tmpdir>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/nntrain.hip"

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

// a network 5-4-3 whose arrays outlive the model struct
struct Net {
    int                 in[2] = {5, 4}, out[2] = {4, 3}, act[2] = {AMX_ACT_SIGMOID, AMX_ACT_NONE};
    std::vector<float>  W0 = std::vector<float>(20, 0.25f), W1 = std::vector<float>(12, -0.5f), b0 = std::vector<float>(4, 0.f), b1 = std::vector<float>(3, 0.f);
    const float*        W[2];
    const float*        b[2];
    amx_ffnn_model      m{};
    Net() {
        W[0] = W0.data(), W[1] = W1.data(), b[0] = b0.data(), b[1] = b1.data();
        m.n_layers = 2, m.in_dim = in, m.out_dim = out, m.W = W, m.bias = b, m.activation = act, m.precision = AMX_PREC_FP32;
    }
};

static int create(const amx_ffnn_model* m, const amx_ffnn_layers* ext, const amx_nntrain_cfg& cfg, amx_nntrain** h) {
    g_error.clear();
    return amx_nntrain_create(nullptr, m, ext, &cfg, h);
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    amx_nntrain_cfg   cfg;
    amx_nntrain_default_cfg(&cfg);
    CHECK(cfg.statistics == (AMX_NNSTAT_BASE | AMX_NNSTAT_GRADIENT) && cfg.error_signal_clip == FLT_MAX && cfg.class_weights == nullptr);
    amx_nntrain* h = nullptr;

    // ---- refusals
    {
        Net n;
        CHECK(amx_nntrain_create(nullptr, &n.m, nullptr, nullptr, &h) == AMX_ERR_INVALID);
        amx_nntrain_cfg c = cfg;
        c.statistics      = 0;
        CHECK(create(&n.m, nullptr, c, &h) == AMX_ERR_INVALID && says("statistics"));
        c.statistics = 16;
        CHECK(create(&n.m, nullptr, c, &h) == AMX_ERR_INVALID);
        c                   = cfg;
        c.error_signal_clip = 0.f;
        CHECK(create(&n.m, nullptr, c, &h) == AMX_ERR_INVALID && says("error_signal_clip"));
        c.error_signal_clip = NAN;
        CHECK(create(&n.m, nullptr, c, &h) == AMX_ERR_INVALID);
        CHECK(create(nullptr, nullptr, cfg, &h) == AMX_ERR_INVALID && says("need a network"));
    }
    for (int prec : {AMX_PREC_BF16, AMX_PREC_BF16X3, AMX_PREC_F16MX}) {
        Net n;
        n.m.precision = prec;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_UNSUPPORTED && says("precision") && h == nullptr);
    }
    {
        Net n;
        n.act[0] = AMX_ACT_ELU;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_UNSUPPORTED && says("layer 0") && says("elu"));
        n.act[0] = 9;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID && says("layer 0"));
        n.act[0] = AMX_ACT_TANH, n.act[1] = AMX_ACT_SIGMOID;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID && says("layer 1") && says("output layer must be linear"));
        n.act[1] = AMX_ACT_NONE, n.in[1] = 7;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID && says("layer 1") && says("does not follow"));
        n.in[1] = 4, n.out[0] = 0;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID && says("layer 0"));
        n.out[0] = 4, n.m.n_layers = 0;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID);
        n.m.n_layers = AMX_NNTRAIN_MAX_LAYERS + 1;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID);
    }
    {   // maxout behind layer 0; bad preprocessing descriptors
        Net             n;
        int             groups[2] = {2, 0};
        amx_ffnn_layers ext{};
        ext.maxout_groups = groups;
        CHECK(create(&n.m, &ext, cfg, &h) == AMX_ERR_UNSUPPORTED && says("layer 0") && says("maxout"));
        ext.maxout_groups = nullptr;
        int types[1]      = {7};
        ext.n_pre = 1, ext.pre_type = types;
        CHECK(create(&n.m, &ext, cfg, &h) == AMX_ERR_INVALID && says("preprocessing layer 0"));
        types[0] = AMX_NN_PRE_MEAN_AND_VARIANCE;
        CHECK(create(&n.m, &ext, cfg, &h) == AMX_ERR_INVALID && says("needs a mean"));
        ext.n_pre = AMX_NN_MAX_PRE + 1;
        CHECK(create(&n.m, &ext, cfg, &h) == AMX_ERR_INVALID);
        types[0] = AMX_NN_PRE_LOGARITHM, ext.n_pre = 1;
        CHECK(create(&n.m, &ext, cfg, &h) == AMX_OK && h != nullptr);
        amx_nntrain_destroy(h);
    }
    {   // class mappings
        Net n;
        int map_bad[4] = {0, 1, 3, -1}, map_twice[4] = {0, 1, 1, -1}, map_ok[5] = {2, -1, 0, 1, -1};
        n.m.class_to_output = map_bad, n.m.n_classes = 4;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID && says("class_to_output[2]"));
        n.m.class_to_output = map_twice;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID && says("one-to-one"));
        n.m.class_to_output = map_ok, n.m.n_classes = 0;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_ERR_INVALID);
        n.m.n_classes = 5;
        CHECK(create(&n.m, nullptr, cfg, &h) == AMX_OK);
        amx_nntrain_destroy(h);
    }
    {   // without a network
        amx_nntrain_cfg c = cfg;
        c.statistics      = AMX_NNSTAT_MEAN_AND_VARIANCE;
        CHECK(create(nullptr, nullptr, c, &h) == AMX_ERR_INVALID && says("feature_dim"));
        c.statistics = AMX_NNSTAT_CLASS_COUNTS;
        CHECK(create(nullptr, nullptr, c, &h) == AMX_ERR_INVALID && says("n_outputs"));
        c.statistics = AMX_NNSTAT_CLASS_COUNTS | AMX_NNSTAT_MEAN_AND_VARIANCE, c.feature_dim = 6, c.n_outputs = 9;
        CHECK(create(nullptr, nullptr, c, &h) == AMX_OK);
        amx_nntrain_layout_info y;
        CHECK(amx_nntrain_layout(h, &y) == AMX_OK && y.n_layers == 0 && y.feature_sum == 0 && y.feature_square_sum == 6 && y.class_counts == 12 && y.tail == 21 &&
              y.size == 25 && amx_nntrain_accumulator_size(h) == 25 && y.gradient_weights[0] == -1);
        double acc[25] = {0};
        float  x[4]    = {0};
        CHECK(amx_nntrain_accumulate_dev(h, x, 6, 1, nullptr, nullptr, acc) == AMX_ERR_STATE && says("without a context"));
        amx_nntrain_destroy(h);
    }

    // ---- the layout under every mask, and the files
    for (int mask = 1; mask < 16; ++mask) {
        Net             n;
        amx_nntrain_cfg c = cfg;
        c.statistics      = mask;
        CHECK(create(&n.m, nullptr, c, &h) == AMX_OK);
        if (!h)
            continue;
        amx_nntrain_layout_info y;
        CHECK(amx_nntrain_layout(h, &y) == AMX_OK);
        long off = 0;
        for (int l = 0; l < 2; ++l) {
            if (mask & AMX_NNSTAT_GRADIENT) {
                CHECK(y.gradient_weights[l] == off);
                off += n.in[l] * n.out[l];
                CHECK(y.gradient_bias[l] == off);
                off += n.out[l];
            }
            else
                CHECK(y.gradient_weights[l] == -1 && y.gradient_bias[l] == -1);
        }
        if (mask & AMX_NNSTAT_MEAN_AND_VARIANCE) {
            CHECK(y.feature_sum == off && y.feature_square_sum == off + 5);
            off += 10;
        }
        else
            CHECK(y.feature_sum == -1 && y.feature_square_sum == -1);
        if (mask & AMX_NNSTAT_CLASS_COUNTS) {
            CHECK(y.class_counts == off);
            off += 3;
        }
        else
            CHECK(y.class_counts == -1);
        CHECK(y.tail == off && y.size == off + 4 && amx_nntrain_accumulator_size(h) == off + 4 && y.n_layers == 2 && y.feature_dim == 5 && y.n_outputs == 3);

        std::vector<double> a((size_t)y.size), b((size_t)y.size, -1.0), s((size_t)y.size, -1.0);
        for (long i = 0; i < y.size; ++i)
            a[i] = 0.125 * (double)(i + 1);      // exact in f32
        a[y.tail] = 40, a[y.tail + 1] = (mask & AMX_NNSTAT_BASE) ? 7 : 0, a[y.tail + 3] = (mask & AMX_NNSTAT_BASE) ? 2.5 : 0;
        if (y.class_counts >= 0)
            a[y.class_counts] = 3, a[y.class_counts + 1] = 0, a[y.class_counts + 2] = 37;
        const std::string path = dir + "/host_nntrain_" + std::to_string(mask) + ".stat";
        CHECK(amx_nnstat_write(h, a.data(), path.c_str()) == AMX_OK);
        CHECK(amx_nnstat_read(h, path.c_str(), b.data()) == AMX_OK);
        CHECK(a == b);
        const char* two[2] = {path.c_str(), path.c_str()};
        CHECK(amx_nnstat_combine(h, two, 2, s.data()) == AMX_OK);
        for (long i = 0; i < y.size; ++i)
            CHECK(s[i] == 2 * a[i]);
        CHECK(amx_nnstat_combine(h, two, 0, s.data()) == AMX_ERR_INVALID);
        // every proper prefix of the file is refused, and nothing is read past a buffer
        FILE* f = fopen(path.c_str(), "rb");
        std::vector<char> bytes(1 << 16);
        const size_t len = fread(bytes.data(), 1, bytes.size(), f);
        fclose(f);
        const std::string cut = dir + "/host_nntrain_cut.stat";
        for (size_t keep = 0; keep < len; keep += (keep < 40 ? 1 : 7)) {
            f = fopen(cut.c_str(), "wb");
            fwrite(bytes.data(), 1, keep, f);
            fclose(f);
            CHECK(amx_nnstat_read(h, cut.c_str(), b.data()) == AMX_ERR_INVALID);
        }
        // another mask's file
        amx_nntrain* other = nullptr;
        c.statistics       = mask == 15 ? 14 : mask + 1;
        CHECK(create(&n.m, nullptr, c, &other) == AMX_OK);
        std::vector<double> ob((size_t)amx_nntrain_accumulator_size(other));
        CHECK(amx_nnstat_read(other, path.c_str(), ob.data()) == AMX_ERR_INVALID && says("magic"));
        amx_nntrain_destroy(other);
        // prior and mean and deviation need their statistics
        float lp[3], mean[5], dev[5];
        CHECK(amx_prior_from_class_counts(h, a.data(), 1.f, lp) == ((mask & AMX_NNSTAT_CLASS_COUNTS) ? AMX_OK : AMX_ERR_STATE));
        CHECK(amx_prior_from_class_counts(h, a.data(), 1.5f, lp) != AMX_OK);
        CHECK(amx_nnstat_mean_and_deviation(h, a.data(), mean, dev) == ((mask & AMX_NNSTAT_MEAN_AND_VARIANCE) ? AMX_OK : AMX_ERR_STATE));
        amx_nntrain_destroy(h);
    }
    if (g_failed)
        std::printf("host_nntrain_test: %d checks failed\n", g_failed);
    else
        std::printf("host_nntrain_test: ok\n");
    return g_failed ? 1 : 0;
}
