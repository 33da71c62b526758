// key_frames.hpp -- the front half of a corpus pass per key that cmllr.hip and mllr.hip share, device side: the upload of key_plan.hpp's
// plan and the resolver that maps every frame's emission and best density to its (mean, covariance [, leaf]) and checks it, before
// anything is written.  The kernel is a template, so each of the two files instantiates its own.
#pragma once
#include <optional>

#include "common.hpp"
#include "gmm_internal.hpp"
#include "key_plan.hpp"

namespace amx {

constexpr int kResolveThreads = 256;

inline int upload_plan(hipStream_t st, const KeyPlan& plan, DevBuf<int>& d_key, DevBuf<KeySeg>& d_segs) {
    AMX_TRY(d_key.reserve(plan.key_tab.size()));
    AMX_TRY(d_segs.reserve(plan.segs.size()));
    AMX_HIP(hipMemcpyAsync(d_key.get(), plan.key_tab.data(), plan.key_tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(d_segs.get(), plan.segs.data(), plan.segs.size() * sizeof(KeySeg), hipMemcpyHostToDevice, st));
    return AMX_OK;
}

// ---- every frame's (mean, covariance [, leaf]) and the checks.  bad = min over the offending frames of (frame << 3 | kind):
// 1 emission outside the model, 2 density outside the mixture, 3 non-finite feature, 4 non-finite weight
template<bool LEAF>
__global__ __launch_bounds__(kResolveThreads) void frame_resolve_kernel(const float* __restrict__ feats, long long ld, int F, long long t0, long long n,
                                                                        const int32_t* __restrict__ emission, const uint32_t* __restrict__ best, int best_ld,
                                                                        const double* __restrict__ weight, int n_mix, const uint32_t* __restrict__ mix_off,
                                                                        const uint32_t* __restrict__ k_dens, const uint32_t* __restrict__ d_mean,
                                                                        const uint32_t* __restrict__ d_cov, const int* __restrict__ leaf_of_mix,
                                                                        int* __restrict__ frame_mean, int* __restrict__ frame_cov, int* __restrict__ frame_leaf,
                                                                        unsigned long long* bad) {
    const long long i = (long long)blockIdx.x * kResolveThreads + threadIdx.x;
    if (i >= n)
        return;
    const long long t = t0 + i;
    const int32_t   e = emission[t];
    int             mi = -1, ci = -1, leaf = -1, kind = 0;
    if (e != -1) {
        if (e < 0 || e >= n_mix)
            kind = 1;
        else {
            const uint32_t kk = best_ld > 0 ? best[t * best_ld + e] : best[t];
            if (kk >= mix_off[e + 1] - mix_off[e])
                kind = 2;
            else {
                const uint32_t d = k_dens[mix_off[e] + kk];
                mi = (int)d_mean[d], ci = (int)d_cov[d];
                if (LEAF)
                    leaf = leaf_of_mix[e];
                for (int c = 0; c < F; ++c)
                    if (!isfinite(feats[t * ld + c]))
                        kind = 3;
                if (weight && !isfinite(weight[t]))
                    kind = kind ? kind : 4;
            }
        }
    }
    frame_mean[i] = kind ? -1 : mi;
    frame_cov[i]  = kind ? -1 : ci;
    if (LEAF)
        frame_leaf[i] = kind ? -1 : leaf;
    if (kind)
        atomicMin(bad, ((unsigned long long)i << 3) | (unsigned long long)kind);
}

// Resets the refusal word, runs the resolver over the call's n frames from t0 (under `timer` where it is not NULL), fetches the word
// and names the first offending frame.  frame_leaf and leaf_of_mix are read where LEAF.
template<bool LEAF>
int resolve_frames(const char* who, amx_ctx* ctx, const char* timer, const amx_internal_gmm_view& gmm, const float* feats, int ld, int F, long long t0,
                   long long n, const int32_t* emission, const uint32_t* best, int best_ld, const double* weight, const int* leaf_of_mix,
                   int* frame_mean, int* frame_cov, int* frame_leaf, unsigned long long* d_bad) {
    hipStream_t st = ctx->stream;
    AMX_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), st));
    {
        std::optional<ScopedKernelTimer> timed;
        if (timer)
            timed.emplace(ctx, timer);
        hipLaunchKernelGGL(frame_resolve_kernel<LEAF>, dim3((unsigned)((n + kResolveThreads - 1) / kResolveThreads)), dim3(kResolveThreads), 0, st, feats,
                           (long long)ld, F, t0, n, emission, best, best_ld, weight, gmm.n_mix, gmm.d_mix_off, gmm.d_k_dens, gmm.d_d_mean, gmm.d_d_cov,
                           leaf_of_mix, frame_mean, frame_cov, frame_leaf, d_bad);
        AMX_HIP(hipGetLastError());
    }
    unsigned long long bad = 0;
    AMX_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    if (bad == ~0ull)
        return AMX_OK;
    const long long t    = t0 + (long long)(bad >> 3);
    const int       kind = (int)(bad & 7);
    int32_t         e    = 0;
    AMX_HIP(hipMemcpy(&e, emission + t, sizeof(e), hipMemcpyDeviceToHost));
    if (kind == 1)
        set_error("%s: frame %lld: emission index %d is outside [0, %d) and is not -1", who, t, e, gmm.n_mix);
    else if (kind == 2)
        set_error("%s: frame %lld: the density of emission %d is outside its mixture", who, t, e);
    else
        set_error("%s: frame %lld: non-finite %s", who, t, kind == 3 ? "feature" : "weight");
    return AMX_ERR_INVALID;
}

}  // namespace amx
