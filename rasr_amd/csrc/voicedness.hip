// voicedness.hip -- RASR's voicedness measure on gfx950 (Tools/FeatureExtraction/share/voicedness.flow) and the amx_voicedness_* part of
// the C ABI.
//
//   signal-window (rectangular)        Signal/TimeWindowBuffer.cc:52-125: frames of `length` every `shift`, short last frame included
//   signal-vector-f32-resize           Signal/VectorResize.hh:93-113: the short last frame is extended by zeros to `new-size`
//   signal-vector-f32-mean-energy-normalization   Signal/VectorNormalization.hh:44-49: f32 products added to a double in index order,
//                                      r = (f32)1 / (f32)sqrt(sum / size), every element times r
//   signal-cross-correlation, x = y    Signal/CrossCorrelation.cc:31-64: real FFT of length next-pow-2(size + K) (no scale: its sample
//                                      rate is 1), X conj(X), real inverse FFT times 2 / (f32)length (Signal/FastFourierTransform.cc:
//                                      125-132), lags [0, end), then :121-122 with CrossCorrelation.hh:43-48: R[m] / (f32)(size - m)
//   signal-peak-detection              Signal/PeakDetection.cc:42-68, 92-98: maximal-peak-value
//
// One kernel, one wave per frame.  A frame is NC = fft_len / 2 complex points (1024 at 16 kHz, 512 at 8 kHz), NC / 64 per lane:
//   * the lane loads its points (samples 2c, 2c + 1, zero behind the frame), the wave forms the energy sum and scales;
//   * forward complex transform: in-LDS Stockham radix-4 (+ one radix-2 stage for NC = 512), first stage from and last stage into
//     registers, twiddles from an LDS table shared by the workgroup's four waves; only wave-level ordering is needed;
//   * one pass over the bin pairs (i, NC - i) does the reference's split step (Math/FastFourierTransform.cc:113-145), the power
//     spectrum and the split step of the inverse transform, whose input has zero imaginary parts;
//   * inverse complex transform, scale, unbiased-estimate division; the lags go to LDS (and to acf_dev when a caller asks);
//   * peak detection: every lane scans its share of the lags for qualifying peaks exactly as the reference's loop would meet them,
//     then the wave keeps the largest value, the first one among equals (the reference's comparison is strict).
// Nothing but the samples (shift * 4 B per frame, overlaps from L2) and one f32 per frame crosses HBM.
//
// Numerics: the energy sum has the reference's bits (see energy_sum); the butterflies and the split are f32 with explicit fmaf and
// table twiddles, where the reference runs f64 recurrences narrowed per butterfly: graded by tolerance like the MFCC chain.
#include "frontend_host.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

struct amx_voicedness {
    amx_ctx*            ctx = nullptr;
    amx_voicedness_cfg  cfg;
    int                 frame_len = 0, frame_shift = 0, fft_len = 0, n_lags = 0, min_pos = 0, max_pos = 0;
    amx::DevBuf<float2> d_tw, d_stw;
    // per-call scratch
    amx::DevBuf<long long> d_off;         // [2][n_seg + 1] sample / frame offsets
    amx::DevBuf<float>     d_pcm, d_out;  // staging of the host entry point
};

namespace amx {

constexpr int kVcWaves = 4;  // frames in flight per workgroup: 4 x NC x 8 B of work buffers + the NC x 8 B twiddle table = 40 KB at NC = 1024

struct VcParams {
    const void*      pcm;         // f32 or s16 (widened without scaling, Flow/TypeConverter.hh:35-43)
    const long long* sample_off;  // [n_seg + 1]
    const long long* frame_off;   // [n_seg + 1]
    const float2*    tw;          // [NC]      e^{+2 pi i k / NC}
    const float2*    stw;         // [NC / 2]  e^{+pi i k / NC}
    float*           out;         // [total_frames][out_ld], column 0
    float*           acf;         // nullable [total_frames][n_lags]
    long long        total_frames;
    int              n_seg, out_ld, frame_len, frame_shift, n_lags, unbiased, min_pos, max_pos;
};

__device__ __forceinline__ void vc_wave_sync() {
    // order this wave's LDS traffic for the compiler; the hardware keeps DS operations of a wave in order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// work buffer index swizzle (a bijection inside every 16-point block): spreads the stride-4 / stride-16 Stockham writes over the banks
__device__ __forceinline__ int vc_zp(int i) { return i ^ (5 * ((i >> 4) & 3)); }

__device__ __forceinline__ float2 vc_cmul(float2 a, float2 w) {
    return make_float2(fmaf(a.x, w.x, -(a.y * w.y)), fmaf(a.x, w.y, a.y * w.x));
}

// 4-point DFT with kernel (s i)^(r k), s = +1 forwards (the reference's forward transform has the positive exponent), -1 backwards
template<bool INV>
__device__ __forceinline__ void vc_bf4(float2& a, float2& b, float2& c, float2& d) {
    const float2 t0 = make_float2(a.x + c.x, a.y + c.y), t1 = make_float2(a.x - c.x, a.y - c.y);
    const float2 t2 = make_float2(b.x + d.x, b.y + d.y), t3 = make_float2(b.x - d.x, b.y - d.y);
    const float2 j3 = INV ? make_float2(t3.y, -t3.x) : make_float2(-t3.y, t3.x);
    a               = make_float2(t0.x + t2.x, t0.y + t2.y);
    c               = make_float2(t0.x - t2.x, t0.y - t2.y);
    b               = make_float2(t1.x + j3.x, t1.y + j3.y);
    d               = make_float2(t1.x - j3.x, t1.y - j3.y);
}

// NC-point complex transform of one wave's frame.  In and out: z[b] = point lane + 64 b.  s_z is the wave's work buffer, free on
// entry (the caller has ordered its earlier readers) and free again on return.
template<int NC, bool INV>
__device__ __forceinline__ void vc_fft(float2 (&z)[NC / 64], float2* s_z, const float2* s_tw, int lane) {
    constexpr int P = NC / 64, Q = P / 4;
    constexpr int L = NC == 1024 ? 10 : 9, S4 = L / 2;
    constexpr bool R2 = (L & 1) != 0;
#pragma unroll
    for (int b = 0; b < Q; ++b)
        vc_bf4<INV>(z[b], z[b + Q], z[b + 2 * Q], z[b + 3 * Q]);
#pragma unroll
    for (int b = 0; b < Q; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            s_z[vc_zp(4 * (lane + 64 * b) + r)] = z[b + r * Q];
    vc_wave_sync();
#pragma unroll
    for (int s = 1; s < S4; ++s) {
        const int Ns = 1 << (2 * s);
#pragma unroll
        for (int b = 0; b < Q; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                z[b + r * Q] = s_z[vc_zp(lane + 64 * b + r * (NC / 4))];
#pragma unroll
        for (int b = 0; b < Q; ++b) {
            const int k = (lane + 64 * b) & (Ns - 1), idx = k * (NC / (4 * Ns));
#pragma unroll
            for (int r = 1; r < 4; ++r) {
                float2 w = s_tw[r * idx];
                if (INV)
                    w.y = -w.y;
                z[b + r * Q] = vc_cmul(z[b + r * Q], w);
            }
            vc_bf4<INV>(z[b], z[b + Q], z[b + 2 * Q], z[b + 3 * Q]);
        }
        if (s == S4 - 1 && !R2)
            break;  // the last stage's outputs are already in the register layout
        vc_wave_sync();
#pragma unroll
        for (int b = 0; b < Q; ++b) {
            const int j = lane + 64 * b, k = j & (Ns - 1), j0 = (j - k) * 4 + k;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                s_z[vc_zp(j0 + r * Ns)] = z[b + r * Q];
        }
        vc_wave_sync();
    }
    if (R2) {
#pragma unroll
        for (int b = 0; b < P / 2; ++b) {
            const int    j = lane + 64 * b;
            const float2 a = s_z[vc_zp(j)];
            float2       w = s_tw[j];
            if (INV)
                w.y = -w.y;
            const float2 t = vc_cmul(s_z[vc_zp(j + NC / 2)], w);
            z[b]           = make_float2(a.x + t.x, a.y + t.y);
            z[b + P / 2]   = make_float2(a.x - t.x, a.y - t.y);
        }
    }
    vc_wave_sync();  // every lane has its last reads before the caller reuses the buffer
}

__device__ __forceinline__ int vc_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, __shfl_xor(v, o));
    return v;
}

// std::inner_product(v.begin(), v.end(), v.begin(), 0.0) over the frame: f32-rounded products added to a double in index order.
// A double sum is exact, whatever its order, when every term is a multiple of 2^lo and all partial sums stay below 2^(lo + 53).
// The wave finds lo (lowest set bit of any product) and hi (largest exponent) and then adds in lane order -- sample values that came
// from 16-bit audio, scaled or not, always pass --; any other frame is added by one lane in index order through the work buffer.
template<int NC>
__device__ __forceinline__ double vc_energy_sum(const float2 (&z)[NC / 64], float2* s_z, int lane, int frame_len, bool* ordered = nullptr) {
    constexpr int P = NC / 64;
    int           hi = -1000, nlo = -1000;  // nlo = -lo, so that one max reduction serves both
    bool          odd = false;              // inf / NaN
    double        part = 0.0;
#pragma unroll
    for (int b = 0; b < P; ++b) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float    x = h ? z[b].y : z[b].x, p = x * x;
            const unsigned u = __float_as_uint(p), e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
            if (e == 255u)
                odd = true;
            else if (e != 0u || m != 0u) {
                const int ee = e ? (int)e - 127 : -126;
                hi           = max(hi, ee);
                nlo          = max(nlo, -(ee - 23 + (int)__builtin_ctz(e ? (m | 0x800000u) : m)));
            }
            part += (double)p;
        }
    }
    hi  = vc_wave_max(hi);
    nlo = vc_wave_max(nlo);
    odd = __any(odd);
    // at most 2 NC = 2^11 terms below 2^(hi + 1)
    const bool exact = !odd && (hi == -1000 || hi + 12 + nlo <= 53);
    if (ordered)
        *ordered = !exact;
    if (exact) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            part += __shfl_xor(part, o);
        return part;
    }
#pragma unroll
    for (int b = 0; b < P; ++b)
        s_z[vc_zp(lane + 64 * b)] = z[b];
    vc_wave_sync();
    double inner = 0.0;
    if (lane == 0)
        for (int n = 0; n < frame_len; ++n) {
            const float2 v = s_z[vc_zp(n >> 1)];
            const float  x = (n & 1) ? v.y : v.x, p = x * x;
            inner          = inner + (double)p;
        }
    vc_wave_sync();
    return __shfl(inner, 0);
}

// the samples of frame g as NC / 64 points per lane (point lane + 64 b = samples 2c, 2c + 1), zero behind the frame's samples
template<int NC, bool S16>
__device__ __forceinline__ void vc_load_frame(const VcParams& p, long long g, int lane, float2 (&z)[NC / 64]) {
    using Sample = typename std::conditional<S16, short, float>::type;
    // the frame's segment: the last u with frame_off[u] <= g
    int lo = 0, hi = p.n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.frame_off[mid] <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int       u     = __builtin_amdgcn_readfirstlane(lo);
    const long long s0    = p.sample_off[u], fstart = (g - p.frame_off[u]) * p.frame_shift;
    const long long rest  = p.sample_off[u + 1] - s0 - fstart;
    const int       valid = (int)(rest < p.frame_len ? rest : p.frame_len);  // signal-vector-f32-resize: zeros behind it
    const Sample*   fr    = (const Sample*)p.pcm + s0 + fstart;
#pragma unroll
    for (int b = 0; b < NC / 64; ++b) {
        const int n = 2 * (lane + 64 * b);
        z[b].x      = n < valid ? (float)fr[n] : 0.f;
        z[b].y      = n + 1 < valid ? (float)fr[n + 1] : 0.f;
    }
}

// test-only: the energy sum of every frame and which way it was added (amx_voicedness_energy_dev)
template<int NC, bool S16>
__global__ __launch_bounds__(kVcWaves * 64) void voicedness_energy_kernel(VcParams p, double* sum, int* ordered) {
    extern __shared__ __attribute__((aligned(16))) float2 vc_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2*   s_z  = vc_smem + wave * NC;
    for (long long g = (long long)blockIdx.x * kVcWaves + wave; g < p.total_frames; g += (long long)gridDim.x * kVcWaves) {
        float2 z[NC / 64];
        vc_load_frame<NC, S16>(p, g, lane, z);
        bool         ord   = false;
        const double inner = vc_energy_sum<NC>(z, s_z, lane, p.frame_len, &ord);
        if (lane == 0) {
            sum[g]     = inner;
            ordered[g] = ord ? 1 : 0;
        }
    }
}

template<int NC, bool S16>
__global__ __launch_bounds__(kVcWaves * 64) void voicedness_kernel(VcParams p) {
    constexpr int P = NC / 64;
    extern __shared__ __attribute__((aligned(16))) float2 vc_smem[];
    float2*   s_tw = vc_smem;                                  // [NC]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2*   s_z   = vc_smem + NC + wave * NC;                // this wave's work buffer
    float*    s_acf = (float*)s_z;                             // the lags, once the inverse transform is back in registers
    for (int i = threadIdx.x; i < NC; i += kVcWaves * 64)
        s_tw[i] = p.tw[i];
    __syncthreads();
    // split twiddles of the bin pairs (i, NC - i) this lane owns, i = lane + 64 q
    float2 stw[P / 2];
#pragma unroll
    for (int q = 0; q < P / 2; ++q)
        stw[q] = p.stw[lane + 64 * q];
    const float inv_nc = 2.0f / (float)(2 * NC);  // RealInverseFastFourierTransform::estimateContinuous with sampleRate_ = fft length

    for (long long g = (long long)blockIdx.x * kVcWaves + wave; g < p.total_frames; g += (long long)gridDim.x * kVcWaves) {
        float2 z[P];
        vc_load_frame<NC, S16>(p, g, lane, z);
        // mean-energy normalisation over the resized vector
        const double inner = vc_energy_sum<NC>(z, s_z, lane, p.frame_len);
        const float  r     = (float)1 / (float)sqrt(inner / (double)(size_t)p.frame_len);
#pragma unroll
        for (int b = 0; b < P; ++b) {
            const int n = 2 * (lane + 64 * b);  // the FFT's own padding behind the resized vector stays zero (0 * inf is NaN)
            z[b].x      = n < p.frame_len ? z[b].x * r : 0.f;
            z[b].y      = n + 1 < p.frame_len ? z[b].y * r : 0.f;
        }
        vc_fft<NC, false>(z, s_z, s_tw, lane);
#pragma unroll
        for (int b = 0; b < P; ++b)
            s_z[vc_zp(lane + 64 * b)] = z[b];
        vc_wave_sync();
        // split, |X|^2, split of the inverse: in place per bin pair
#pragma unroll
        for (int q = 0; q < P / 2; ++q) {
            const int    i  = lane + 64 * q, j = (NC - i) & (NC - 1);
            const float2 za = s_z[vc_zp(i)], zb = s_z[vc_zp(j)];
            const float2 w  = stw[q];
            const float  h1r = 0.5f * (za.x + zb.x), h1i = 0.5f * (za.y - zb.y);
            const float  h2r = 0.5f * (za.y + zb.y), h2i = -0.5f * (za.x - zb.x);
            const float  ar = fmaf(-w.y, h2i, fmaf(w.x, h2r, h1r)), ai = fmaf(w.y, h2r, fmaf(w.x, h2i, h1i));
            const float  br = fmaf(w.y, h2i, fmaf(-w.x, h2r, h1r)), bi = fmaf(w.y, h2r, fmaf(w.x, h2i, -h1i));
            const float  pa = fmaf(ar, ar, ai * ai), pb = fmaf(br, br, bi * bi);
            const float  g1 = 0.5f * (pa + pb), g2 = 0.5f * (pa - pb);
            float2       oa = make_float2(fmaf(w.y, g2, g1), w.x * g2), ob = make_float2(fmaf(-w.y, g2, g1), w.x * g2);
            if (i == 0) {  // DC and Nyquist bins, packed; the middle bin passes through both split steps untouched
                const float  x0 = za.x + za.y, xn = za.x - za.y, p0 = x0 * x0, pn = xn * xn;
                const float2 zm = s_z[vc_zp(NC / 2)];
                oa              = make_float2(0.5f * (p0 + pn), 0.5f * (p0 - pn));
                s_z[vc_zp(NC / 2)] = make_float2(fmaf(zm.x, zm.x, zm.y * zm.y), 0.f);
            }
            else
                s_z[vc_zp(j)] = ob;
            s_z[vc_zp(i)] = oa;
        }
        vc_wave_sync();
#pragma unroll
        for (int b = 0; b < P; ++b)
            z[b] = s_z[vc_zp(lane + 64 * b)];
        vc_wave_sync();
        vc_fft<NC, true>(z, s_z, s_tw, lane);
        // scale, lags [0, n_lags), unbiased estimate
        float* acf = p.acf ? p.acf + g * p.n_lags : nullptr;
#pragma unroll
        for (int b = 0; b < P; ++b) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int m = 2 * (lane + 64 * b) + h;
                float     v = (h ? z[b].y : z[b].x) * inv_nc;
                if (p.unbiased) {
                    const int N = p.frame_len - m;
                    v           = N > 0 ? v / (float)N : 0.f;
                }
                if (m < p.n_lags) {
                    s_acf[m] = v;
                    if (acf)
                        acf[m] = v;
                }
            }
        }
        vc_wave_sync();
        // PeakDetection::getMaximalPeakIndex: the loop's candidates are the indices with a strict rise in front and no rise behind
        // (an index inside a plateau never has the strict rise, so skipping over plateaus changes nothing)
        const int n = p.n_lags, chunk = (n + 63) / 64;
        bool      have = false;
        float     bv   = -FLT_MAX;  // Core::Type<f32>::min
        int       bp = 0x7fffffff, be = 0;
        const int pb = max(1, lane * chunk), pe = min(n - 1, (lane + 1) * chunk);
        for (int q = pb; q < pe; ++q) {
            if (s_acf[q - 1] < s_acf[q] && s_acf[q] >= s_acf[q + 1]) {
                int e = q;
                while (e + 1 < n && s_acf[e] == s_acf[e + 1])
                    ++e;
                if (e + 1 < n && s_acf[e] > s_acf[e + 1] && s_acf[e] > bv && q <= p.max_pos && e >= p.min_pos) {
                    bv   = s_acf[e];
                    bp   = q;
                    be   = e;
                    have = true;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int   op = __shfl_xor(bp, o), oe = __shfl_xor(be, o);
            const bool  oh = __shfl_xor((int)have, o) != 0;
            if (oh && (!have || ov > bv || (ov == bv && op < bp))) {
                bv   = ov;
                bp   = op;
                be   = oe;
                have = true;
            }
        }
        if (lane == 0) {
            float v = 0.f;
            if (have) {
                const unsigned pos = min(max((unsigned)(bp + be) / 2u, (unsigned)p.min_pos), (unsigned)p.max_pos);
                v                  = s_acf[pos];
            }
            p.out[g * p.out_ld] = v;
        }
        vc_wave_sync();  // the lags are read before the next frame's transform writes the buffer
    }
}

}  // namespace amx

extern "C" {

void amx_voicedness_default_cfg(amx_voicedness_cfg* c) {
    if (!c)
        return;
    c->sample_rate    = 16000.0;
    c->win_len_s      = 0.040;  // voicedness.flow: window length = padded-window new-size
    c->win_shift_s    = 0.010;
    c->corr_begin_s   = 0.0;
    c->corr_end_s     = 0.040;
    c->normalization  = AMX_XCORR_UNBIASED_ESTIMATE;
    c->min_position_s = 0.0025;
    c->max_position_s = 0.0167;
    c->tuning         = nullptr;
}

int amx_voicedness_create(amx_ctx* ctx, const amx_voicedness_cfg* c, amx_voicedness** out) {
    AMX_REQUIRE(c && out, AMX_ERR_INVALID, "amx_voicedness_create: NULL argument");
    *out = nullptr;
    AMX_REQUIRE(c->sample_rate > 0, AMX_ERR_INVALID, "voicedness: sample rate (%f) is not positive", c->sample_rate);
    AMX_REQUIRE(c->win_len_s > 0 && c->win_shift_s > 0, AMX_ERR_INVALID, "voicedness: window length / shift must be positive");
    {
        amx::Tuning              tune;
        static const char* const keys[] = {nullptr};  // no kernel choices yet; the string is still checked
        if (!tune.parse(c->tuning, keys, "amx_voicedness_create"))
            return AMX_ERR_INVALID;
    }
    // CrossCorrelationNode::init and PeakDetection::init: seconds to indices with rint
    const long begin = (long)std::rint(c->corr_begin_s * c->sample_rate), end = (long)std::rint(c->corr_end_s * c->sample_rate);
    AMX_REQUIRE(begin <= end, AMX_ERR_INVALID, "voicedness: Discrete begin time (%ld) is larger then Discrete end time (%ld).", begin, end);
    AMX_REQUIRE(begin == 0, AMX_ERR_UNSUPPORTED, "voicedness: begin (%g s = lag %ld) is not supported: only begin = 0 (no negative or skipped lags)",
                c->corr_begin_s, begin);
    AMX_REQUIRE(c->normalization != AMX_XCORR_UPPER_BOUND, AMX_ERR_UNSUPPORTED,
                "voicedness: normalization upper-bound is not supported (none | unbiased-estimate)");
    AMX_REQUIRE(c->normalization == AMX_XCORR_NONE || c->normalization == AMX_XCORR_UNBIASED_ESTIMATE, AMX_ERR_INVALID,
                "voicedness: unknown normalization %d", c->normalization);
    AMX_REQUIRE(c->min_position_s >= 0 && c->min_position_s < c->max_position_s, AMX_ERR_INVALID,
                "voicedness: min-position (%f) is larger or equal to max-position (%f).", c->min_position_s, c->max_position_s);
    std::unique_ptr<amx_voicedness> h(new amx_voicedness);
    h->ctx            = ctx;
    h->cfg            = *c;
    h->cfg.tuning     = nullptr;
    h->frame_len      = (int)(unsigned)std::rint(c->win_len_s * c->sample_rate);
    h->frame_shift    = (int)(unsigned)std::rint(c->win_shift_s * c->sample_rate);
    h->n_lags         = (int)end;
    // PeakDetection::init: the continuous positions are f32 members (PeakDetection.hh:33-36), the product with the sample rate is f64
    h->min_pos        = (int)(unsigned)std::rint((float)c->min_position_s * c->sample_rate);
    h->max_pos        = (int)(unsigned)std::rint((float)c->max_position_s * c->sample_rate);
    AMX_REQUIRE(h->frame_len >= 2 && h->frame_shift >= 1 && h->n_lags >= 1, AMX_ERR_INVALID,
                "voicedness: window of %d samples / shift of %d samples / %d lags", h->frame_len, h->frame_shift, h->n_lags);
    AMX_REQUIRE(h->n_lags > h->max_pos, AMX_ERR_INVALID,  // PeakDetectionNode::work
                "voicedness: Input size (%d) is smaller or equal to max-position (%d).", h->n_lags, h->max_pos);
    // RealFastFourierTransform fft(size + K), K = max(|begin|, |end - 1|); FastFourierTransform::setLength
    const unsigned len = (unsigned)h->frame_len + (unsigned)std::max(std::labs(begin), std::labs(end - 1));
    unsigned       n   = 1;
    while (n < len)
        n <<= 1;
    h->fft_len = (int)n;
    AMX_REQUIRE(h->fft_len == 1024 || h->fft_len == 2048, AMX_ERR_UNSUPPORTED,
                "voicedness: a window of %d samples with %d lags needs a %d-point transform; 1024 and 2048 are built "
                "(40 ms windows at 8 and 16 kHz)", h->frame_len, h->n_lags, h->fft_len);
    if (ctx) {
        const int           nc = h->fft_len / 2;
        std::vector<float2> tw(nc), stw(nc / 2);
        for (int k = 0; k < nc; ++k)
            tw[k] = make_float2((float)std::cos(2.0 * M_PI * k / nc), (float)std::sin(2.0 * M_PI * k / nc));
        for (int k = 0; k < nc / 2; ++k)
            stw[k] = make_float2((float)std::cos(M_PI * k / nc), (float)std::sin(M_PI * k / nc));
        AMX_REQUIRE(hipSetDevice(ctx->device) == hipSuccess && h->d_tw.upload(tw.data(), tw.size()) == AMX_OK &&
                            h->d_stw.upload(stw.data(), stw.size()) == AMX_OK,
                    AMX_ERR_DEVICE, "amx_voicedness_create: uploading the twiddle tables failed");
    }
    *out = h.release();
    return AMX_OK;
}

void amx_voicedness_destroy(amx_voicedness* h) {
    if (h && h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_voicedness_describe(const amx_voicedness* h, amx_voicedness_info* info) {
    AMX_REQUIRE(h && info, AMX_ERR_INVALID, "amx_voicedness_describe: NULL argument");
    info->frame_len    = h->frame_len;
    info->frame_shift  = h->frame_shift;
    info->fft_len      = h->fft_len;
    info->n_lags       = h->n_lags;
    info->min_position = h->min_pos;
    info->max_position = h->max_pos;
    return AMX_OK;
}

long amx_voicedness_n_frames(const amx_voicedness* h, long n) {
    return h ? amx::window_frames(n, h->frame_len, h->frame_shift) : 0;
}

static int voicedness_run_batch_dev(amx_voicedness* h, int n_seg, const long* sample_offsets, const void* pcm_dev, bool s16, float* out_dev,
                                    int out_ld, float* acf_dev, const char* who, double* sum_dev = nullptr, int* ordered_dev = nullptr) {
    using namespace amx;
    AMX_REQUIRE(h && n_seg >= 0 && (n_seg == 0 || (sample_offsets && pcm_dev && (out_dev || (sum_dev && ordered_dev)))), AMX_ERR_INVALID,
                "%s: bad argument", who);
    AMX_REQUIRE(out_ld >= 1, AMX_ERR_INVALID, "%s: out_ld (%d) must be at least 1", who, out_ld);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: host-only handle (created without a context)", who);
    if (n_seg == 0)
        return AMX_OK;
    long long frames = 0;
    AMX_TRY(upload_segment_table(h->ctx, h->d_off, n_seg, sample_offsets, [h](long len) { return amx_voicedness_n_frames(h, len); }, who, &frames));
    if (frames == 0)
        return AMX_OK;
    VcParams p;
    p.pcm          = pcm_dev;
    p.sample_off   = h->d_off.get();
    p.frame_off    = h->d_off.get() + n_seg + 1;
    p.tw           = h->d_tw.get();
    p.stw          = h->d_stw.get();
    p.out          = out_dev;
    p.acf          = acf_dev;
    p.total_frames = frames;
    p.n_seg        = n_seg;
    p.out_ld       = out_ld;
    p.frame_len    = h->frame_len;
    p.frame_shift  = h->frame_shift;
    p.n_lags       = h->n_lags;
    p.unbiased     = h->cfg.normalization == AMX_XCORR_UNBIASED_ESTIMATE;
    p.min_pos      = h->min_pos;
    p.max_pos      = h->max_pos;
    {
        ScopedKernelTimer timer(h->ctx, "voicedness");
        const int         nc   = h->fft_len / 2;
        const size_t      lds  = (size_t)(kVcWaves + 1) * nc * 8;
        const long long   wgs  = (frames + kVcWaves - 1) / kVcWaves;
        const long long   cap  = (long long)std::max(h->ctx->n_cu, 1) * 4;  // workgroups stride over the frames; at most four are resident per CU
                                                                            // (LDS), one at NC = 1024 (registers), the others queue behind them
        const dim3        grid((unsigned)std::min(wgs, cap));
        if (sum_dev) {  // test-only: the normalisation's energy sums
            const size_t elds = (size_t)kVcWaves * nc * 8;
            if (nc == 1024)
                hipLaunchKernelGGL((voicedness_energy_kernel<1024, false>), grid, dim3(kVcWaves * 64), elds, h->ctx->stream, p, sum_dev, ordered_dev);
            else
                hipLaunchKernelGGL((voicedness_energy_kernel<512, false>), grid, dim3(kVcWaves * 64), elds, h->ctx->stream, p, sum_dev, ordered_dev);
        }
        else if (nc == 1024) {
            if (s16)
                hipLaunchKernelGGL((voicedness_kernel<1024, true>), grid, dim3(kVcWaves * 64), lds, h->ctx->stream, p);
            else
                hipLaunchKernelGGL((voicedness_kernel<1024, false>), grid, dim3(kVcWaves * 64), lds, h->ctx->stream, p);
        }
        else {
            if (s16)
                hipLaunchKernelGGL((voicedness_kernel<512, true>), grid, dim3(kVcWaves * 64), lds, h->ctx->stream, p);
            else
                hipLaunchKernelGGL((voicedness_kernel<512, false>), grid, dim3(kVcWaves * 64), lds, h->ctx->stream, p);
        }
    }
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

int amx_voicedness_run_batch_dev(amx_voicedness* h, int n_seg, const long* sample_offsets, const float* pcm_dev, float* out_dev, int out_ld,
                                 float* acf_dev) {
    return voicedness_run_batch_dev(h, n_seg, sample_offsets, pcm_dev, false, out_dev, out_ld, acf_dev, "amx_voicedness_run_batch_dev");
}

int amx_voicedness_run_batch_dev_s16(amx_voicedness* h, int n_seg, const long* sample_offsets, const int16_t* pcm_dev, float* out_dev,
                                     int out_ld, float* acf_dev) {
    return voicedness_run_batch_dev(h, n_seg, sample_offsets, pcm_dev, true, out_dev, out_ld, acf_dev, "amx_voicedness_run_batch_dev_s16");
}

int amx_voicedness_energy_dev(amx_voicedness* h, int n_seg, const long* sample_offsets, const float* pcm_dev, double* sum_dev, int* ordered_dev) {
    AMX_REQUIRE(sum_dev && ordered_dev, AMX_ERR_INVALID, "amx_voicedness_energy_dev: NULL argument");
    return voicedness_run_batch_dev(h, n_seg, sample_offsets, pcm_dev, false, nullptr, 1, nullptr, "amx_voicedness_energy_dev", sum_dev, ordered_dev);
}

int amx_voicedness_run(amx_voicedness* h, const float* pcm_host, long n_samples, float* out_host) {
    AMX_REQUIRE(h && n_samples >= 0 && (n_samples == 0 || (pcm_host && out_host)), AMX_ERR_INVALID, "amx_voicedness_run: bad argument");
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "amx_voicedness_run: host-only handle (created without a context)");
    const long T = amx_voicedness_n_frames(h, n_samples);
    if (T == 0)
        return AMX_OK;
    const long off[2] = {0, n_samples};
    return amx::run_staged(h->ctx, h->d_pcm, h->d_out, pcm_host, (size_t)n_samples, out_host, (size_t)T, [&](const float* pcm_dev, float* out_dev) {
        return amx_voicedness_run_batch_dev(h, 1, off, pcm_dev, out_dev, 1, nullptr);
    });
}

}  // extern "C"
