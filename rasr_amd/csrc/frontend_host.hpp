// frontend_host.hpp -- host code the front ends share (mfcc_tables.cpp, gammatone.hip, voicedness.hip): the frame-count rule, the
// segment table of the batched entry points and the staging of the one-segment host entry points.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace amx {

// Signal/WindowBuffer.cc:84-125 (and TimeWindowBuffer on top of it): get() while >= 2*max(len,shift) buffered, then flush() every
// `shift` samples until the rest fits into one window; the last frame is short.
inline long window_frames(long n, int len, int shift) {
    if (n <= 0)
        return 0;
    const long reach = std::max(len, shift);
    if (n <= reach)
        return 1;
    return (n - reach + shift - 1) / shift + 1;
}

// The [2][n_seg + 1] sample / frame offset table of a batch (n_seg >= 1), checked, built and copied into d_off on the context's
// stream.  *frames is the batch's frame count; when it is 0 nothing is copied and no HIP call is made.
template<class Frames>
int upload_segment_table(amx_ctx* ctx, DevBuf<long long>& d_off, int n_seg, const long* sample_offsets, Frames&& n_frames, const char* who,
                         long long* frames) {
    std::vector<long long> off(2 * ((size_t)n_seg + 1));
    long long*             so = off.data();
    long long*             fo = off.data() + n_seg + 1;
    so[0] = sample_offsets[0];
    fo[0] = 0;
    for (int u = 0; u < n_seg; ++u) {
        const long len = sample_offsets[u + 1] - sample_offsets[u];
        AMX_REQUIRE(len >= 0 && len <= 0x7fffffffL, AMX_ERR_INVALID, "%s: segment %d has invalid length %ld", who, u, len);
        so[u + 1] = sample_offsets[u + 1];
        fo[u + 1] = fo[u] + n_frames(len);
    }
    *frames = fo[n_seg];
    if (*frames == 0)
        return AMX_OK;
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_TRY(d_off.reserve(off.size()));
    AMX_HIP(hipMemcpyAsync(d_off.get(), off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));  // `off` is a local
    return AMX_OK;
}

// One segment from host memory (n_in >= 1 samples, n_out >= 1 results): the handle's two staging buffers grow as needed, the
// samples go up, run(pcm_dev, out_dev) is the batched device entry point, the results come back and the stream is waited for.
template<class Run>
int run_staged(amx_ctx* ctx, DevBuf<float>& d_pcm, DevBuf<float>& d_out, const float* pcm_host, size_t n_in, float* out_host, size_t n_out,
               Run&& run) {
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_TRY(d_pcm.reserve(n_in));
    AMX_TRY(d_out.reserve(n_out));
    AMX_HIP(hipMemcpyAsync(d_pcm.get(), pcm_host, n_in * 4, hipMemcpyHostToDevice, ctx->stream));
    AMX_TRY(run(d_pcm.get(), d_out.get()));
    AMX_HIP(hipMemcpyAsync(out_host, d_out.get(), n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    return AMX_OK;
}

}  // namespace amx
