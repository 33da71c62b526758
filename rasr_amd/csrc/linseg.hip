// linseg.hip -- Speech::LinearSegmenter on the device (include/amx.h, section "Linear-segmentation alignment"): the node
// speech-linear-segmentation for a batch of segments whose energy is a column of a feature matrix that is already on the device.
//
// One workgroup per segment, the segment is the parallel axis of the batch.  Inside a segment:
//   chains      Delimiter::feed's M_ and Q_ (AlignmentWithLinearSegmentation.cc:61-71) are two sequential f64 chains in frame order: the lanes
//               widen the energies into the handle's workspace (and look for values that are not finite), then ONE lane adds them up in
//               order, eight loads ahead of the chain.  No scan: a reassociated sum has other bits.
//   searches    every loop of getDelimitation (:155-169, :207-232) evaluates logLikelihood for candidates that do not depend on each other;
//               only the carried minimum does.  The lanes share the candidates, each keeps the first one of its own that is strictly below
//               what it holds (starting from the carried x_min), and one reduction per loop takes the smallest score, the lowest candidate
//               among equal scores.  That is the sequential loop's winner: the first candidate that reaches the loop's minimum, if that is
//               below the carried value.  A NaN compares false and never wins.
//   spread      (:325-347) every lane writes the labels of its frames; the jump test compares a frame's index with its predecessor's.
// No atomics on floating-point values and nothing that depends on occupancy, the batch or earlier calls: a segment's bits are its own.
// The library is compiled with -ffp-contract=off; mad<FMA> marks the one site where the reference's -march=native build holds a fused
// multiply-add that can change a bit (xsil + xspe with s2 * log(.) fused, :118).  feed's xx * xx + f / 2 is fused there as well, but xx is
// a widened f32 whose square is exact in f64: both forms round the same sum once.
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.hpp"

#define AMX_LINSEG_MAX_ITERATIONS 4096

namespace amx {

constexpr int      kLinsegThreads = 256;
constexpr int      kLinsegAhead   = 8;
constexpr unsigned kLinsegNone    = 0xffffffffu;

// one segment of a call, as the kernel takes it
struct LinsegSeg {
    long long frame0;    // absolute row of its first frame
    long long chain0;    // where its M_ starts in the workspace's M half (and its Q_ in the Q half): frames before it + segments before it
    int       frames;
    int       state0, n_states;
    int       reason;    // what the host's checks decided: OK (the kernel goes on), NO_STATES, TOO_SHORT, TOO_LONG
};

struct LinsegPlan {
    std::vector<LinsegSeg> seg;
    long long              frames = 0;       // frame_offsets[n_seg] - frame_offsets[0]
    long long              chain_words = 0;  // doubles in each half of the workspace: frames + n_seg
    int                    states = 0;
};

struct LinsegArgs {
    const LinsegSeg* seg;
    const float*     energy;
    long long        energy_ld;
    const int*       state_label;
    const int*       state_emission;
    int              silence_label, silence_emission;
    double*          m;   // [chain_words]
    double*          q;   // [chain_words]
    int32_t*         label;
    int32_t*         emission;
    amx_linseg_result* result;
    double           penalty;
    float            proportion;
    int              iterations, sietill;
};

// the checked segment table of a call: AlignmentWithLinearSegmentationNode::work's isAlignmentValid (:311-313, :413) and getAlignment's
// length tests (:316-319), which need no frame's value
static int linseg_plan(const amx_linseg_cfg& cfg, int n_seg, const long* frame_offsets, const amx_linseg_models* models, const char* who, LinsegPlan* p) {
    AMX_REQUIRE(frame_offsets, AMX_ERR_INVALID, "%s: NULL frame_offsets", who);
    AMX_REQUIRE(models && models->state_offsets, AMX_ERR_INVALID, "%s: NULL models or state_offsets", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: negative frame offset", who);
    AMX_REQUIRE(models->state_offsets[0] == 0, AMX_ERR_INVALID, "%s: state_offsets[0] is %d, not 0", who, models->state_offsets[0]);
    AMX_REQUIRE(models->silence_label >= 0 && models->silence_emission >= 0, AMX_ERR_INVALID, "%s: silence_label %d, silence_emission %d: negative", who,
                models->silence_label, models->silence_emission);
    p->seg.resize((size_t)n_seg);
    for (int s = 0; s < n_seg; ++s) {
        AMX_REQUIRE(frame_offsets[s] <= frame_offsets[s + 1], AMX_ERR_INVALID, "%s: frame offsets decrease at segment %d", who, s);
        AMX_REQUIRE(models->state_offsets[s] <= models->state_offsets[s + 1], AMX_ERR_INVALID, "%s: state_offsets decrease at segment %d", who, s);
    }
    AMX_REQUIRE(frame_offsets[n_seg] < (1ll << 31), AMX_ERR_INVALID, "%s: frame_offsets[%d] = %ld: a call takes rows below 2^31", who, n_seg, frame_offsets[n_seg]);
    p->states = models->state_offsets[n_seg];
    AMX_REQUIRE(p->states == 0 || (models->state_label && models->state_emission), AMX_ERR_INVALID, "%s: NULL state_label or state_emission", who);
    for (int s = 0; s < n_seg; ++s)
        for (int i = models->state_offsets[s]; i < models->state_offsets[s + 1]; ++i) {
            AMX_REQUIRE(models->state_label[i] >= 0, AMX_ERR_INVALID, "%s: segment %d: state_label[%d] = %d", who, s, i, models->state_label[i]);
            AMX_REQUIRE(models->state_emission[i] >= 0, AMX_ERR_INVALID, "%s: segment %d: state_emission[%d] = %d", who, s, i, models->state_emission[i]);
        }
    for (int s = 0; s < n_seg; ++s) {
        LinsegSeg& g = p->seg[s];
        g.frame0     = frame_offsets[s];
        g.chain0     = frame_offsets[s] - frame_offsets[0] + s;
        g.frames     = (int)(frame_offsets[s + 1] - frame_offsets[s]);
        g.state0     = models->state_offsets[s];
        g.n_states   = models->state_offsets[s + 1] - g.state0;
        g.reason     = AMX_LINSEG_OK;
        if (g.n_states == 0 || g.frames == 0)
            g.reason = AMX_LINSEG_NO_STATES;
        else if (g.frames < cfg.minimum_segment_length)
            g.reason = AMX_LINSEG_TOO_SHORT;
        else if (g.frames > cfg.maximum_segment_length)
            g.reason = AMX_LINSEG_TOO_LONG;
    }
    p->frames      = frame_offsets[n_seg] - frame_offsets[0];
    p->chain_words = p->frames + n_seg;
    return AMX_OK;
}

// Delimiter::logLikelihood (:103-120), every operation in its place.  m, q: the segment's chains; n: nFeatures()
template<bool FMA>
__host__ __device__ inline double linseg_likelihood(const double* m, const double* q, unsigned n, double f, float gate, unsigned ib,
                                                    unsigned ie) {
    const double e    = 0.5;
    const double d    = f > 0 ? f : 1;
    const double s1   = (double)(ib - 1u + n - ie);                      // u32 arithmetic, then widened (:106)
    const double m1   = m[ib - 1] + m[n] - m[ie];
    double       qq   = q[ib - 1] + q[n] - q[ie];
    const double a1   = m1 / s1;
    double       xx   = qq / s1 - (a1 * a1) / d;
    const double xsil = s1 * log(xx < e ? e : xx);                      // std::max(xx, e)
    const double s2   = (double)(ie - ib + 1u);
    const double m2   = m[ie] - m[ib - 1];
    qq                = q[ie] - q[ib - 1];
    const double a2   = m2 / s2;
    xx                = qq / s2 - (a2 * a2) / d;
    const double l2   = log(xx < e ? e : xx);
    if (a1 < a2 && (float)(ie - ib) >= gate)                            // gate = minimumSpeechProportion_ * nFeatures(), an f32 product (:117)
        return mad<FMA>(s2, l2, xsil);                                   // xsil + xspe; the native build fuses xspe's product (:118)
    return DBL_MAX;
}

// the index of frame t of the speech part [begin, end] (:328-332); d = t - begin
__host__ __device__ inline unsigned linseg_index(float slope, unsigned d) {
    return (unsigned)roundf(slope * (float)d);
}

struct LinsegBest {
    double   x;
    unsigned c;
};

// the smallest x of the workgroup, the lowest c among equal x; every lane returns it.  red: kLinsegThreads / 64 slots
__device__ inline LinsegBest linseg_reduce(LinsegBest b, LinsegBest* red) {
    for (int o = 32; o > 0; o >>= 1) {
        const double   x = __shfl_xor(b.x, o);
        const unsigned c = __shfl_xor(b.c, o);
        if (x < b.x || (x == b.x && c < b.c))
            b.x = x, b.c = c;
    }
    __syncthreads();   // red may still be read from the loop before
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = b;
    __syncthreads();
    b = red[0];
    for (int w = 1; w < kLinsegThreads / 64; ++w) {
        const LinsegBest o = red[w];
        if (o.x < b.x || (o.x == b.x && o.c < b.c))
            b = o;
    }
    return b;
}

template<bool FMA>
__global__ __launch_bounds__(kLinsegThreads) void linseg_kernel(LinsegArgs p) {
    __shared__ LinsegBest red[kLinsegThreads / 64];
    __shared__ int        nonfinite, jumped;   // set by whoever finds one, read behind a barrier
    const LinsegSeg g   = p.seg[blockIdx.x];
    const int       tid = threadIdx.x;
    const unsigned  n   = (unsigned)g.frames;
    int32_t*        lab = p.label + g.frame0;
    int32_t*        emi = p.emission + g.frame0;
    int             reason = g.reason;
    int             begin = -1, end = -1;
    double          x_min = DBL_MAX;
    if (reason == AMX_LINSEG_OK) {
        double* m = p.m + g.chain0;
        double* q = p.q + g.chain0;
        if (tid == 0)
            nonfinite = 0, jumped = 0;
        __syncthreads();
        // the energies, widened, into the places of Q_[1 ..]; a value that is not finite is remembered
        bool bad = false;
        for (unsigned t = tid; t < n; t += kLinsegThreads) {
            const float x = p.energy[(g.frame0 + t) * p.energy_ld];
            bad |= !(fabsf(x) <= FLT_MAX);
            q[t + 1] = (double)x;
        }
        if (bad)
            nonfinite = 1;
        __syncthreads();
        if (tid == 0) {   // feed (:61-71), in frame order
            const double f = p.penalty, half = f / 2.0;
            double       ms = 0, qs = 0;
            m[0] = 0, q[0] = 0;
            for (unsigned t0 = 0; t0 < n; t0 += kLinsegAhead) {
                double x[kLinsegAhead];
#pragma unroll
                for (int i = 0; i < kLinsegAhead; ++i)
                    x[i] = t0 + i < n ? q[t0 + i + 1] : 0.0;
#pragma unroll
                for (int i = 0; i < kLinsegAhead; ++i) {
                    if (t0 + i >= n)
                        break;
                    ms += x[i];
                    qs += f > 0 ? (x[i] * x[i] + half) / f : x[i] * x[i];
                    m[t0 + i + 1] = ms, q[t0 + i + 1] = qs;
                }
            }
            if (!(fabs(ms) <= DBL_MAX) || !(fabs(qs) <= DBL_MAX))   // Q_ only grows: its last value tells; M_ is bounded by n * FLT_MAX
                nonfinite = 1;
        }
        __syncthreads();
        if (nonfinite)
            reason = AMX_LINSEG_NONFINITE;
        else {
            unsigned i_beg = 1, i_end = p.sietill ? n : n - 1;
            if (p.proportion == 1.0f)
                i_beg = 1, i_end = n;                 // (0, nFeatures() - 1) (:146-147, :202-203)
            else if (!p.sietill && n == 1)
                i_beg = 1, i_end = 1;                 // (0, 0) (:149-150)
            else {
                const float  gate = p.proportion * (float)n;
                const double f    = p.penalty;
                for (int it = 0; it < p.iterations; ++it) {
                    const unsigned b0 = i_beg, e0 = i_end;
                    const double   x0 = x_min;
                    if (p.sietill)
                        x_min = DBL_MAX;              // per iteration (:208)
                    for (int which = 0; which < 2; ++which) {
                        // Delimiter: ib over [2, iEnd - 1) against iEnd, then ie over [iBeg + 1, n - 1) against iBeg (:156-169);
                        // Sietill: both over [2, n) except the other index, the pair ordered for the call (:209-226)
                        const unsigned other = which == 0 ? i_end : i_beg;
                        const unsigned lo    = p.sietill || which == 0 ? 2u : i_beg + 1u;
                        const unsigned hi    = p.sietill ? n : which == 0 ? i_end - 1u : n - 1u;
                        LinsegBest     best{x_min, kLinsegNone};
                        for (unsigned long long c64 = (unsigned long long)lo + tid; c64 < hi; c64 += kLinsegThreads) {
                            const unsigned c = (unsigned)c64;
                            double         x;
                            if (p.sietill) {
                                if (c == other)
                                    continue;
                                x = linseg_likelihood<FMA>(m, q, n, f, gate, c < other ? c : other, c < other ? other : c);
                            }
                            else
                                x = which == 0 ? linseg_likelihood<FMA>(m, q, n, f, gate, c, other) : linseg_likelihood<FMA>(m, q, n, f, gate, other, c);
                            if (x < best.x)
                                best.x = x, best.c = c;
                        }
                        best = linseg_reduce(best, red);
                        if (best.c != kLinsegNone) {
                            x_min = best.x;
                            if (which == 0)
                                i_beg = best.c;
                            else
                                i_end = best.c;
                        }
                    }
                    if (p.sietill && i_end < i_beg) {
                        const unsigned tmp = i_beg;
                        i_beg = i_end, i_end = tmp;
                    }
                    // an iteration is a function of what it starts from (Sietill: of the pair alone): one that changes nothing is a fixed point
                    if (i_beg == b0 && i_end == e0 && (p.sietill || x_min == x0))
                        break;
                }
            }
            begin = (int)(i_beg - 1), end = (int)(i_end - 1);
            // the spread: first the jump test over the speech part, then the labels
            const unsigned len   = (unsigned)(end - begin);
            const float    slope = (float)(g.n_states - 1) / (float)(len > 1u ? len : 1u);
            bool           jump  = false;
            for (unsigned d = 1 + tid; d <= len; d += kLinsegThreads)
                jump |= linseg_index(slope, d) - linseg_index(slope, d - 1) > 2u;
            if (jump)
                jumped = 1;
            __syncthreads();
            if (jumped)
                reason = AMX_LINSEG_JUMP;
            else if (linseg_index(slope, len) != (unsigned)(g.n_states - 1))
                reason = AMX_LINSEG_MISMATCH;
            else {
                const int* sl = p.state_label + g.state0;
                const int* se = p.state_emission + g.state0;
                for (unsigned t = tid; t < n; t += kLinsegThreads) {
                    int l = p.silence_label, e = p.silence_emission;
                    if (t >= (unsigned)begin && t <= (unsigned)end) {
                        unsigned i = linseg_index(slope, t - (unsigned)begin);
                        i          = i < (unsigned)g.n_states ? i : (unsigned)g.n_states - 1u;   // never past the table
                        l = sl[i], e = se[i];
                    }
                    lab[t] = l, emi[t] = e;
                }
            }
        }
    }
    if (reason != AMX_LINSEG_OK)
        for (unsigned t = tid; t < n; t += kLinsegThreads)
            lab[t] = -1, emi[t] = -1;
    if (tid == 0) {
        amx_linseg_result r;
        r.reason = reason, r.speech_begin = begin, r.speech_end = end, r.score = x_min;
        p.result[blockIdx.x] = r;
    }
}

}  // namespace amx

struct amx_linseg {
    amx_ctx*       ctx = nullptr;
    amx_linseg_cfg cfg{};
    amx::DevBuf<amx::LinsegSeg>     d_seg;
    amx::DevBuf<int>                d_states;   // [2 x states]: labels, then emission indices
    amx::DevBuf<double>             d_chains;   // [2 x (frames + n_seg)]: every segment's M_, then every segment's Q_
    amx::DevBuf<amx_linseg_result>  d_result;
    amx::LinsegPlan                 last;       // the last call's segments: amx_linseg_chains
};

extern "C" {

void amx_linseg_default_cfg(amx_linseg_cfg* cfg) {
    if (!cfg)
        return;
    cfg->number_of_iterations      = 3;         // AlignmentWithLinearSegmentation.cc:81-84
    cfg->penalty                   = 100.0;     // :86-89
    cfg->minimum_speech_proportion = 0.7f;      // :91-94
    cfg->should_use_sietill        = 0;         // :259-262
    cfg->minimum_segment_length    = 1;         // :254-257
    cfg->maximum_segment_length    = INT_MAX;   // :249-252
}

int amx_linseg_create(amx_ctx* ctx, const amx_linseg_cfg* cfg, amx_linseg** out) {
    const char* who = "amx_linseg_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(cfg, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(cfg->number_of_iterations >= 0, AMX_ERR_INVALID, "%s: number_of_iterations %d is negative", who, cfg->number_of_iterations);
    AMX_REQUIRE(cfg->number_of_iterations <= AMX_LINSEG_MAX_ITERATIONS, AMX_ERR_UNSUPPORTED, "%s: number_of_iterations %d is above the limit of %d iterations",
                who, cfg->number_of_iterations, AMX_LINSEG_MAX_ITERATIONS);
    AMX_REQUIRE(cfg->penalty == cfg->penalty, AMX_ERR_INVALID, "%s: penalty is not a number", who);
    AMX_REQUIRE(cfg->penalty >= 0 && cfg->penalty <= DBL_MAX, AMX_ERR_INVALID, "%s: penalty %g must be at least 0 and finite", who, cfg->penalty);
    AMX_REQUIRE(cfg->minimum_speech_proportion == cfg->minimum_speech_proportion, AMX_ERR_INVALID, "%s: minimum_speech_proportion is not a number", who);
    AMX_REQUIRE(cfg->minimum_speech_proportion >= 0.f && cfg->minimum_speech_proportion <= 1.f, AMX_ERR_INVALID,
                "%s: minimum_speech_proportion %g is outside [0, 1]", who, (double)cfg->minimum_speech_proportion);
    AMX_REQUIRE(cfg->minimum_segment_length >= 0, AMX_ERR_INVALID, "%s: minimum_segment_length %d is negative", who, cfg->minimum_segment_length);
    AMX_REQUIRE(cfg->maximum_segment_length >= 0, AMX_ERR_INVALID, "%s: maximum_segment_length %d is negative", who, cfg->maximum_segment_length);
    std::unique_ptr<amx_linseg> h(new amx_linseg);
    h->ctx = ctx;
    h->cfg = *cfg;
    *out   = h.release();
    return AMX_OK;
}

void amx_linseg_destroy(amx_linseg* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_linseg_align_dev(amx_linseg* h, int n_seg, const long* frame_offsets, const amx_linseg_models* models, const float* energy_dev, int energy_ld,
                         int32_t* label_dev, int32_t* emission_dev, amx_linseg_result* result, unsigned long long* counters) {
    const char* who = "amx_linseg_align_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_seg >= 0, AMX_ERR_INVALID, "%s: n_seg %d", who, n_seg);
    AMX_REQUIRE(energy_ld >= 1, AMX_ERR_INVALID, "%s: energy_ld %d must be at least 1", who, energy_ld);
    if (n_seg == 0) {
        if (counters)
            for (int r = 0; r < AMX_LINSEG_N_REASONS; ++r)
                counters[r] = 0;
        return AMX_OK;
    }
    AMX_REQUIRE(result, AMX_ERR_INVALID, "%s: NULL result", who);
    amx::LinsegPlan plan;
    AMX_TRY(amx::linseg_plan(h->cfg, n_seg, frame_offsets, models, who, &plan));
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(plan.frames == 0 || (energy_dev && label_dev && emission_dev), AMX_ERR_INVALID, "%s: NULL energy_dev, label_dev or emission_dev", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    h->last = amx::LinsegPlan();
    AMX_TRY(h->d_seg.reserve((size_t)n_seg));
    AMX_TRY(h->d_states.reserve(2 * (size_t)plan.states + 1));
    AMX_TRY(h->d_chains.reserve(2 * (size_t)plan.chain_words));
    AMX_TRY(h->d_result.reserve((size_t)n_seg));
    AMX_HIP(hipMemcpyAsync(h->d_seg.get(), plan.seg.data(), (size_t)n_seg * sizeof(amx::LinsegSeg), hipMemcpyHostToDevice, ctx->stream));
    if (plan.states) {
        AMX_HIP(hipMemcpyAsync(h->d_states.get(), models->state_label, (size_t)plan.states * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        AMX_HIP(hipMemcpyAsync(h->d_states.get() + plan.states, models->state_emission, (size_t)plan.states * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    }
    amx::LinsegArgs a{};
    a.seg = h->d_seg.get(), a.energy = energy_dev, a.energy_ld = energy_ld;
    a.state_label = h->d_states.get(), a.state_emission = h->d_states.get() + plan.states;
    a.silence_label = models->silence_label, a.silence_emission = models->silence_emission;
    a.m = h->d_chains.get(), a.q = h->d_chains.get() + plan.chain_words;
    a.label = label_dev, a.emission = emission_dev, a.result = h->d_result.get();
    a.penalty = h->cfg.penalty, a.proportion = h->cfg.minimum_speech_proportion;
    a.iterations = h->cfg.number_of_iterations, a.sietill = h->cfg.should_use_sietill ? 1 : 0;
    {
        amx::ScopedKernelTimer timer(ctx, "linseg");
        if (ctx->contract == AMX_CONTRACT_FMA)
            hipLaunchKernelGGL(amx::linseg_kernel<true>, dim3((unsigned)n_seg), dim3(amx::kLinsegThreads), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL(amx::linseg_kernel<false>, dim3((unsigned)n_seg), dim3(amx::kLinsegThreads), 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipMemcpyAsync(result, h->d_result.get(), (size_t)n_seg * sizeof(amx_linseg_result), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    if (counters) {
        for (int r = 0; r < AMX_LINSEG_N_REASONS; ++r)
            counters[r] = 0;
        for (int s = 0; s < n_seg; ++s)
            if (result[s].reason >= 0 && result[s].reason < AMX_LINSEG_N_REASONS)
                ++counters[result[s].reason];
    }
    h->last = std::move(plan);
    return AMX_OK;
}

int amx_linseg_chains(amx_linseg* h, int segment, double* m, double* q) {
    const char* who = "amx_linseg_chains";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(segment >= 0 && (size_t)segment < h->last.seg.size(), AMX_ERR_INVALID, "%s: segment %d of a call of %zu", who, segment, h->last.seg.size());
    const amx::LinsegSeg& g = h->last.seg[(size_t)segment];
    AMX_REQUIRE(g.reason == AMX_LINSEG_OK, AMX_ERR_STATE, "%s: segment %d was turned away before its chains were formed", who, segment);
    AMX_HIP(hipSetDevice(h->ctx->device));
    const size_t bytes = ((size_t)g.frames + 1) * sizeof(double);
    if (m)
        AMX_HIP(hipMemcpy(m, h->d_chains.get() + g.chain0, bytes, hipMemcpyDeviceToHost));
    if (q)
        AMX_HIP(hipMemcpy(q, h->d_chains.get() + h->last.chain_words + g.chain0, bytes, hipMemcpyDeviceToHost));
    return AMX_OK;
}

}  // extern "C"
