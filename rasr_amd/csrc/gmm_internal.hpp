// gmm_internal.hpp -- the entry points the GMM scorer's translation units call in one another (internal to librasr_amd.so, not part
// of the ABI).  gmm.hip and every file that defines one of them include it, so the compiler checks definition against declaration.
#pragma once
#include "common.hpp"

// the dimensions with kernel instances of their own (every other dimension runs the D = 0 instance, rows re-read from memory)
#define AMX_GMM_DIMS(X) X(16) X(24) X(32) X(33) X(39) X(40) X(45) X(48) X(64)

extern "C" {

// gmm_presel.hip: preselection-batch-float
int  amx_internal_gmm_presel_create(amx_ctx* ctx, int dim, size_t nk, const uint32_t* k_mean_host, const float* smeans_host, const float* d_smeans,
                                    const uint32_t* d_k_mean, int n_clusters, int n_select, int iterations, float backoff, int contract_fma,
                                    void** out);
void amx_internal_gmm_presel_destroy(void* p);
int  amx_internal_gmm_presel_info(const void* p, int* n_clusters, uint32_t* cluster_of, float* cluster_means);
int  amx_internal_gmm_presel_score(void* p, amx_ctx* ctx, const float* feats_dev, int T, float* scores_dev, const uint32_t* d_mix_off,
                                   const uint32_t* d_k_mean, const float* d_k_const, const float* d_smeans, const float* d_isr0, int n_mix);

// gmm_simd.hip: SIMD-diagonal-maximum, batch-int, preselection-batch-int
int   amx_internal_gmm_simd_create(const amx_gmm_model* m, int contract_fma, void** out, float* scaling_out);
void  amx_internal_gmm_simd_destroy(void* p);
float amx_internal_gmm_simd_scaling(const void* p);
int   amx_internal_gmm_simd_score(void* p, amx_ctx* ctx, int variant, const float* feats_dev, int T, float* scores_dev, uint32_t* best_dev);
int   amx_internal_gmm_simd_presel_build(void* p, amx_ctx* ctx, int n_clusters, int n_select, int iterations);
int   amx_internal_gmm_simd_presel_info(const void* p, int* n_clusters, uint32_t* cluster_of, float* cluster_means);
int   amx_internal_gmm_simd_presel_score(void* p, amx_ctx* ctx, const float* feats_dev, int T, float* scores_dev);

// gmm_tied.hip: the pruned path of a shared-list tied model
int    amx_internal_gmm_tied_create(int K, int n_mix, int mix_pad, const float* ahat_t_host, amx::DevBuf<float>& amin,
                                    amx::DevBuf<unsigned short>& aup);
size_t amx_internal_gmm_tied_workspace(int K, int T, int mix_pad);
int    amx_internal_gmm_tied_score(amx_ctx* ctx, const float* dist_dev, const uint32_t* k_dens_dev, int K, int T, int Tpad, int n_mix, int mix_pad,
                                   const unsigned short* aup, const float* amax, const float* m2lw_t, const float* ahat_t, const double* ln64,
                                   const float* ln32, const float* amin, void* workspace, float* scores, uint32_t* best,
                                   unsigned long long* survivors_dev, int dt_written, int near_written);
float* amx_internal_gmm_tied_dt(void* workspace, int K, int T, int have_positions);
unsigned long long* amx_internal_gmm_tied_near(void* workspace);
int                 amx_internal_gmm_tied_near_init(amx_ctx* ctx, void* workspace);

// gmm_fused.hip: screen and exact evaluation in one kernel
int amx_internal_gmm_fused_supported(int dim, int pooled, int Kp);
int amx_internal_gmm_fused_create(int dim, int n_mix, int n_tiles, const void* A2_host, const uint32_t* mix_off, const uint32_t* k_mean,
                                  const double* c64, const float* means, const float* p1, const float* p2, amx::DevBuf<char>& rec);
int amx_internal_gmm_fused_split(int n_cu, int Tpad, int n_tiles, int forced_waves);
int amx_internal_gmm_fused_score(amx_ctx* ctx, int dim, const void* rec_dev, const float* isr_dev, const float* feats, const void* X,
                                 const float* nx, const float* q, int T, int Tpad, int n_mix, int n_tiles, int split, float* scores, uint32_t* best,
                                 float* pmin, unsigned* pidx, int part_ld, unsigned long long* survivors, int forced_waves, int best_bytes,
                                 int contract_fma, float na_all);
int amx_internal_gmm_fused_waves(int Tpad, int forced_waves);

// gmm.hip: what an estimator built on a scorer handle reads of it (cmllr.hip).  The pointers live as long as the handle; the device ones
// and h_vars ([n_cov x dim], host) are NULL for a host-only handle
struct amx_internal_gmm_view {
    amx_ctx*        ctx;
    int             dim, n_mix, n_dens, n_mean, n_cov;
    const uint32_t *d_mix_off, *d_k_dens, *d_d_mean, *d_d_cov;
    const float*    d_means;   // [n_mean x dim]
    const float*    h_vars;
};
int amx_internal_gmm_view_get(const amx_gmm* h, amx_internal_gmm_view* out);

// ffnn.hip: combine per-tile arg-min partials [n_tiles x part_ld] (shared with the NN scorer's fused statistics)
int amx_internal_best_state_reduce(amx_ctx* ctx, const float* part_min, const unsigned* part_idx, int n_tiles, int part_ld, int T,
                                   uint32_t* best_state_dev, unsigned long long* counts_dev, double* score_sum_dev);

}  // extern "C"
