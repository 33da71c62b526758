// Stand-alone host program for the host side of the "NN mini-batch training" section of include/amx.h: it compiles
// rasr_amd/csrc/nntrain.hip's and nnstep.hip's host side into itself (no librasr_amd.so, no Python), creates handles without a context
// and walks through amx_nnstep_default_cfg, every refusal of amx_nntrain_set_estimator and its message, a configuration set twice, the
// read-back of a host-only handle, the narrowing of a flat buffer that amx_nntrain_estimate starts from, and the info struct.  No
// device call is made: a handle without a context refuses every stepping entry point before it touches HIP.  Meant to be built with the
// host sanitizers (tests/test_nnstep.py does):
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -w -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/host_nnstep_test.cc -o host_nnstep_test && ./host_nnstep_test
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/nntrain.hip"
#include "../rasr_amd/csrc/nnstep.hip"

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
    std::vector<float>  W0 = std::vector<float>(20), W1 = std::vector<float>(12), b0 = std::vector<float>(4), b1 = std::vector<float>(3);
    const float*        W[2];
    const float*        b[2];
    amx_ffnn_model      m{};
    Net() {
        for (size_t i = 0; i < W0.size(); ++i) W0[i] = 0.25f * (float)i - 1.f;
        for (size_t i = 0; i < W1.size(); ++i) W1[i] = -0.5f * (float)i;
        for (size_t i = 0; i < b0.size(); ++i) b0[i] = 0.125f * (float)i;
        for (size_t i = 0; i < b1.size(); ++i) b1[i] = 3.f - (float)i;
        W[0] = W0.data(), W[1] = W1.data(), b[0] = b0.data(), b[1] = b1.data();
        m.n_layers = 2, m.in_dim = in, m.out_dim = out, m.W = W, m.bias = b, m.activation = act, m.precision = AMX_PREC_FP32;
    }
};

static int set(amx_nntrain* h, const amx_nnstep_cfg& c) {
    g_error.clear();
    return amx_nntrain_set_estimator(h, &c);
}

int main() {
    Net             n;
    amx_nntrain_cfg tc;
    amx_nntrain_default_cfg(&tc);
    amx_nntrain* h = nullptr;
    CHECK(amx_nntrain_create(nullptr, &n.m, nullptr, &tc, &h) == AMX_OK && h);

    amx_nnstep_cfg cfg;
    memset(&cfg, 0xff, sizeof cfg);
    amx_nnstep_default_cfg(&cfg);
    amx_nnstep_default_cfg(nullptr);
    CHECK(cfg.learning_rate == 1.f && cfg.bias_learning_rate == 1.f && !cfg.layer_learning_rate && !cfg.regularization_constant && !cfg.trainable);
    CHECK(cfg.regularizer == AMX_NNSTEP_REG_NONE && !cfg.center_W && !cfg.center_bias && !cfg.center_in_dim && !cfg.center_out_dim);
    CHECK(cfg.estimator == AMX_NNSTEP_MEAN_NORMALIZED_SGD && cfg.accumulate_multiple_batches == 1 && cfg.normalize_by_observations == 1 &&
          cfg.log_step_size == 0 && cfg.update_input_layer_weights == 1);
    CHECK(!cfg.statistics_smoothing && !cfg.trace_factor && !cfg.initial_activation_mean && !cfg.initial_activation_stddev &&
          cfg.input_smoothing == AMX_NNSTEP_STAT_NO_STATISTICS && cfg.input_trace_factor == 0.5f && !cfg.input_initial_mean && !cfg.input_initial_stddev);
    {   // activation statistics: the output layer keeps none; a mean comes with its deviation; unknown methods
        amx_nnstep_cfg c = cfg;
        int mode[2] = {AMX_NNSTEP_STAT_EXPONENTIAL_TRACE, AMX_NNSTEP_STAT_NONE};
        c.statistics_smoothing = mode;
        CHECK(amx_nntrain_set_estimator(h, &c) == AMX_ERR_UNSUPPORTED && says("output layer"));
        mode[1] = AMX_NNSTEP_STAT_NO_STATISTICS;
        CHECK(amx_nntrain_set_estimator(h, &c) == AMX_OK && h->step.stat_mode[1] == AMX_NNSTEP_STAT_EXPONENTIAL_TRACE && h->step.stat_mode[0] == 0 && h->step.stat_f[1] == 0.5f);
        const float  m[4] = {0.f, 1.f, 2.f, 3.f};
        const float* means[2] = {m, nullptr};
        c.initial_activation_mean = means;
        CHECK(amx_nntrain_set_estimator(h, &c) == AMX_ERR_INVALID && says("come together"));
        c.initial_activation_stddev = means;
        CHECK(amx_nntrain_set_estimator(h, &c) == AMX_OK && h->step.stat_has_initial[1] == 1);
        mode[0] = 3;
        CHECK(amx_nntrain_set_estimator(h, &c) == AMX_ERR_INVALID && says("statistics_smoothing = 3"));
        CHECK(amx_nntrain_get_activation_statistics(h, 0, nullptr, nullptr) == AMX_ERR_STATE);
        float one_row[5] = {0};
        CHECK(amx_nntrain_get_layer_input(h, 0, 1, one_row) == AMX_ERR_STATE);
    }

    // ---- stepping before an estimator is set, and on a handle without a context
    amx_nnstep_info info;
    float           x[5] = {0};
    uint32_t        e[1] = {0};
    CHECK(amx_nntrain_step_dev(h, x, 5, 1, e, nullptr, &info) == AMX_ERR_STATE && says("without a context"));
    CHECK(amx_nntrain_step_accumulate_dev(nullptr, x, 5, 1, e, nullptr) == AMX_ERR_INVALID);
    CHECK(amx_nntrain_step_estimate_dev(nullptr) == AMX_ERR_INVALID);

    // ---- refusals
    CHECK(amx_nntrain_set_estimator(h, nullptr) == AMX_ERR_INVALID && amx_nntrain_set_estimator(nullptr, &cfg) == AMX_ERR_INVALID);
    {
        amx_nnstep_cfg c = cfg;
        c.accumulate_multiple_batches = 0;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("accumulate_multiple_batches = 0"));
        c = cfg;
        const float neg[2] = {0.5f, -1e-3f};
        c.regularization_constant = neg;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("regularization_constant[1]"));
        c = cfg;
        const float rate[2] = {NAN, 1.f};
        c.layer_learning_rate = rate;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("layer_learning_rate[0]"));
        c = cfg;
        c.learning_rate = INFINITY;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("learning_rate"));
        c = cfg;
        c.regularizer = 4;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("regularizer = 4"));
        c = cfg;
        c.estimator = -1;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("estimator = -1"));
        c = cfg;
        c.regularizer = AMX_NNSTEP_REG_CENTERED_L2;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("center_W"));
        int          cin[2] = {5, 4}, cout[2] = {4, 2};
        const float* cb[2]  = {n.b0.data(), n.b1.data()};
        c.center_W = n.W, c.center_bias = cb, c.center_in_dim = cin, c.center_out_dim = cout;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("layer 1") && says("4 -> 2"));
        cout[1] = 3;
        cb[0]   = nullptr;
        CHECK(set(h, c) == AMX_ERR_INVALID && says("layer 0") && says("NULL"));
        cb[0] = n.b0.data();
        CHECK(set(h, c) == AMX_OK);  // the centre is copied: the arrays above may go
    }
    {   // no network / other statistics
        amx_nntrain_cfg t2 = tc;
        t2.statistics      = AMX_NNSTAT_CLASS_COUNTS;
        t2.n_outputs       = 3;
        amx_nntrain* bare  = nullptr;
        CHECK(amx_nntrain_create(nullptr, nullptr, nullptr, &t2, &bare) == AMX_OK);
        CHECK(set(bare, cfg) == AMX_ERR_INVALID && says("no network"));
        CHECK(amx_nntrain_get_parameters(bare, 0, 0, nullptr, nullptr) == AMX_ERR_STATE);
        amx_nntrain_destroy(bare);
        t2            = tc;
        t2.statistics = AMX_NNSTAT_BASE | AMX_NNSTAT_GRADIENT | AMX_NNSTAT_MEAN_AND_VARIANCE;
        CHECK(amx_nntrain_create(nullptr, &n.m, nullptr, &t2, &bare) == AMX_OK);
        CHECK(set(bare, cfg) == AMX_ERR_INVALID && says("nothing else"));
        amx_nntrain_destroy(bare);
    }

    // ---- a configuration set twice (the first one's copies are released), per-layer arrays copied
    {
        std::vector<float> rate = {1.f, 0.5f}, c = {0.f, 0.25f};
        std::vector<int>   tr   = {1, 0};
        amx_nnstep_cfg     k    = cfg;
        k.layer_learning_rate = rate.data(), k.regularization_constant = c.data(), k.trainable = tr.data();
        k.regularizer = AMX_NNSTEP_REG_L1, k.estimator = AMX_NNSTEP_MEAN_NORMALIZED_SGD_L1_CLIPPING, k.accumulate_multiple_batches = 3;
        CHECK(set(h, k) == AMX_OK);
        CHECK(set(h, k) == AMX_OK);
    }
    CHECK(h->step.set && h->step.A == 3 && h->step.n == 0 && h->step.eta_l[1] == 0.5f && h->step.c[1] == 0.25f && h->step.trainable[1] == 0);
    CHECK(h->step.center_W.empty());
    CHECK(!layer_regularized(h->step, 0) && !layer_regularized(h->step, 1));  // c == 0; not trainable
    CHECK(updates_weights(h, 0) && !updates_weights(h, 1));
    h->step.update_input = 0;
    CHECK(!updates_weights(h, 0));  // no preprocessing layer: layer 0 has no predecessor
    CHECK(amx_nntrain_step_dev(h, x, 5, 1, e, nullptr, &info) == AMX_ERR_STATE && says("without a context"));
    CHECK(amx_nntrain_step_estimate_dev(h) == AMX_ERR_STATE && amx_nntrain_step_info(h, &info) == AMX_ERR_STATE);
    CHECK(amx_nntrain_get_step_statistics(h, 0, nullptr, nullptr) == AMX_ERR_STATE);

    // ---- read-back on the host-only handle
    {
        std::vector<float> W(20, -9.f), b(4, -9.f);
        for (int image = 0; image < 2; ++image) {
            CHECK(amx_nntrain_get_parameters(h, 0, image, W.data(), b.data()) == AMX_OK);
            CHECK(W == n.W0 && b == n.b0);
        }
        CHECK(amx_nntrain_get_parameters(h, 1, 0, nullptr, b.data()) == AMX_OK && b[0] == 3.f && b[2] == 1.f && b[3] == n.b0[3]);
        CHECK(amx_nntrain_get_parameters(h, 2, 0, W.data(), b.data()) == AMX_ERR_INVALID && says("layer = 2"));
        CHECK(amx_nntrain_get_parameters(h, 0, 2, W.data(), b.data()) == AMX_ERR_INVALID && says("image = 2"));
    }

    // ---- the narrowing amx_nntrain_estimate starts from: the file's f32 (u32 for the counts), in the layout's order
    {
        amx_nntrain_layout_info y;
        CHECK(amx_nntrain_layout(h, &y) == AMX_OK && y.size == 20 + 4 + 12 + 3 + 4);
        std::vector<double> acc((size_t)y.size);
        for (long i = 0; i < y.size; ++i)
            acc[i] = 1.0 / 3.0 + (double)i;
        acc[y.tail + 0] = 129.0, acc[y.tail + 1] = 7.0;
        std::vector<std::vector<float>> gw, gb;
        uint32_t n_obs = 0, n_err = 0;
        float    tw = 0.f, obj = 0.f;
        CHECK(amx::nntrain_narrow_gradient(h, acc.data(), &gw, &gb, &n_obs, &n_err, &tw, &obj, "test") == AMX_OK);
        CHECK(n_obs == 129 && n_err == 7 && tw == (float)acc[y.tail + 2] && obj == (float)acc[y.tail + 3]);
        CHECK(gw.size() == 2 && gw[0].size() == 20 && gw[1].size() == 12 && gb[0].size() == 4 && gb[1].size() == 3);
        CHECK(gw[0][7] == (float)acc[y.gradient_weights[0] + 7] && gw[1][11] == (float)acc[y.gradient_weights[1] + 11] && gb[1][2] == (float)acc[y.gradient_bias[1] + 2]);
        acc[y.tail + 0] = -1.0;
        CHECK(amx::nntrain_narrow_gradient(h, acc.data(), &gw, &gb, &n_obs, &n_err, &tw, &obj, "test") == AMX_ERR_INVALID && says("test:"));
        CHECK(amx_nntrain_estimate(h, acc.data(), &info) == AMX_ERR_STATE);  // a handle without a context
    }

    // ---- the info struct from a group block
    {
        double g[amx::GRP_SIZE] = {0};
        g[amx::GRP_OBS] = 258, g[amx::GRP_ERR] = 31, g[amx::GRP_TOTAL_WEIGHT] = 250.5, g[amx::GRP_OBJECTIVE] = 4.25, g[amx::GRP_CRITERION] = 4.0;
        g[amx::GRP_STEP + 0] = 0.5, g[amx::GRP_STEP + 1] = 0.25, g[amx::GRP_STEP + 2] = 9.0;  // beyond the network's layers: not reported
        h->step.n = 6;
        memset(&info, 0xff, sizeof info);
        fill_info(h, g, 1, &info);
        CHECK(info.minibatch == 6 && info.updated == 1 && info.n_observations == 258 && info.n_classification_errors == 31);
        CHECK(info.total_weight == 250.5f && info.objective == 4.25f && info.criterion_objective == 4.f);
        CHECK(info.step_size[0] == 0.5f && info.step_size[1] == 0.25f && info.step_size[2] == 0.f && info.step_size[AMX_NNTRAIN_MAX_LAYERS - 1] == 0.f);
    }

    amx_nntrain_destroy(h);
    if (g_failed) {
        std::printf("host_nnstep_test: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("host_nnstep_test: ok\n");
    return 0;
}
