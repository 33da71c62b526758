// nntrain.hpp -- the handle that nntrain.hip (statistics pass, files) and nnstep.hip (mini-batch training) share.
#pragma once
#include "common.hpp"
#include "ffnn_f32.hpp"

#include <cfloat>
#include <vector>

namespace amx {

// Where the pass of nntrain.hip puts a call's results in mini-batch training (nnstep.hip) instead of the caller's f64 buffer: the
// call's tail, and the call's gradient added into the group's f32 statistic with the regulariser's axpy behind it.
struct StepSink {
    double*       call_tail  = nullptr;  // [4], zeroed by the caller: observations, errors, sum |w|, objective of this call
    const double* group_tail = nullptr;  // [0] = the group's observations before this call
    int           reset      = 0;        // the first call of a group: the statistic counts as zero, and the pass clears the group block
                                         // (group_block, group_bytes) once the labels have passed their check
    double*       group_block = nullptr;
    size_t        group_bytes = 0;
    int           regularizer = 0;       // AMX_NNSTEP_REG_*
    float*        G[AMX_NNTRAIN_MAX_LAYERS]  = {};  // [Pin x Pout], zero padded
    float*        g[AMX_NNTRAIN_MAX_LAYERS]  = {};  // [Pout]
    float         c[AMX_NNTRAIN_MAX_LAYERS]  = {};  // regularisation constant; 0 = the layer takes no regulariser
    const float*  WTc[AMX_NNTRAIN_MAX_LAYERS] = {};  // centre, transposed image [Pin x Pout]
    const float*  bc[AMX_NNTRAIN_MAX_LAYERS]  = {};
};

// amx_nntrain_set_estimator's copy of the configuration and what it allocates
struct NnStep {
    bool  set = false;
    float eta = 1.f, eta_bias = 1.f;
    std::vector<float> eta_l, c;
    std::vector<int>   trainable;
    int   regularizer = 0, estimator = 0, A = 1, normalize = 1, log_step = 0, update_input = 1;
    long  n = 0;  // mini-batches since set_estimator
    std::vector<std::vector<float>> center_W, center_b;  // host copies (a host-only handle keeps them for nothing but the checks)
    std::vector<DevBuf<float>> d_G, d_g, d_WTc, d_bc;
    DevBuf<double>       d_group, d_call, d_norm_part;  // group block (nnstep.hip: GRP_*), the call's tail, the segment sums of a norm
    DevBuf<float>        d_norm, d_abs_part;            // [2 x L] narrowed norms (bias, weights); tile sums of |G|
    DevBuf<double, true> h_group;
    // activation statistics, indexed by the layer they feed: p = 0 the last preprocessing layer, p = l the output of layer l - 1
    std::vector<int>   stat_mode;  // AMX_NNSTEP_STAT_*
    std::vector<float> stat_f;
    std::vector<char>  stat_need_init, stat_has_initial;
    std::vector<DevBuf<float>> d_act, d_act_initial;  // [2 x Pin]: sum, sum of squares; initial mean, initial deviation
    DevBuf<double>     d_act_nobs;                    // [L]
    DevBuf<float>      d_colpart;                     // [Pin / 32 x Pout] of the largest layer: the tile rows' parts of G^T m
};

}  // namespace amx

struct amx_nntrain {
    amx_ctx* ctx  = nullptr;
    int      mask = 0;
    float    clip = FLT_MAX;
    int      L = 0, feature_dim = 0, n_outputs = 0, n_classes = 0;
    std::vector<int>   in, out, act, Pin, Pout;
    std::vector<int>   class_to_output;  // empty = identity
    std::vector<float> class_weights;    // [n_outputs]
    amx_nntrain_layout_info lay{};
    std::vector<std::vector<float>> host_W, host_bias;  // a host-only handle keeps the parameters it was created with
    // device images
    std::vector<amx::DevBuf<float>> d_W, d_WT, d_bias;  // [Pout x Pin], [Pin x Pout], [Pout], zero padded
    amx::DevBuf<int>   d_c2o;
    amx::DevBuf<float> d_cw;
    amx::PreOps        pre{};
    std::vector<amx::DevBuf<float>> d_pre_mean, d_pre_rstd;
    // workspace of a call, grown to the largest call so far
    std::vector<amx::DevBuf<float>> d_x, d_E;  // layer inputs [Tpad x Pin], error signals [Tpad x Pout]
    amx::DevBuf<float>    d_top, d_rowstat, d_w, d_obj, d_part;
    amx::DevBuf<int>      d_label;
    amx::DevBuf<unsigned> d_err, d_bad;
    amx::DevBuf<unsigned, true> h_bad;
    amx::NnStep           step;
    unsigned long         workspace_epoch = 0;  // counts the calls that fill the workspace: nnseq.hip sees whether its batch is still there
};

namespace amx {

// One statistics pass (nntrain.hip).  sink == nullptr: into the caller's flat f64 buffer acc (amx_nntrain_accumulate_dev); otherwise
// acc is not read and the results go where the sink says.  who: the entry point's name for the messages.
int nntrain_pass(amx_nntrain* h, const float* feats, int ldf, int T, const uint32_t* emission, const double* weight, double* acc,
                 const StepSink* sink, const char* who);

// The launches of a pass on the handle's workspace, for the segment-wise trainer (nnseq.hip), which fills d_x[0], d_E[top], d_label
// and d_w itself; nntrain_pass goes through the same functions.  forward: every layer from d_x[0] [Tpad x Pin], the negated top
// output into d_top [T x n_outputs]; softmax: d_top in place (d_rowstat holds 2 T floats); backward: d_E[l - 1] from d_E[l], clip ==
// FLT_MAX: none; gemm_tn: the chunk partials of X_l E_l^T into d_part; bias_sums: the chunk partials of E_l's column sums into d_part.
void nntrain_launch_forward(amx_nntrain* h, int Tpad, int T, hipStream_t st);
void nntrain_launch_softmax(amx_nntrain* h, int T, hipStream_t st);
void nntrain_launch_backward(amx_nntrain* h, int Tpad, float clip, hipStream_t st);
void nntrain_launch_gemm_tn(amx_nntrain* h, int l, int Tpad, int tn_chunks, hipStream_t st);
void nntrain_launch_bias_sums(amx_nntrain* h, int l, int T, int n_chunks, hipStream_t st);

// the regulariser's axpy alone on the sink's statistic as it stands (amx_nntrain_estimate): factor = group_tail[0] + call_tail[0]
int nntrain_add_regularizer(amx_nntrain* h, const StepSink* sink);

// the buffer narrowed as the Nn::Statistics<f32> file narrows it (nntrain.hip): per layer G [in x out] and g [out], and the tail
int nntrain_narrow_gradient(const amx_nntrain* h, const double* acc, std::vector<std::vector<float>>* gw, std::vector<std::vector<float>>* gb,
                            uint32_t* n_obs, uint32_t* n_err, float* total_weight, float* objective, const char* who);

}  // namespace amx
