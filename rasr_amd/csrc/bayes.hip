// bayes.hip -- Signal::BayesClassification on a [frames x classes] score matrix that is already on the device (include/amx.h, section
// "Bayes classification"): the nodes signal-bayes-classification and signal-bayes-classification-score for a batch of segments.
//
// The f32 sum over frames is one dependent chain whose order the reference fixes (LikelihoodFunction.cc:76-81), so bayes_sum_kernel is
// parallel over (segment, class) only: no tree, no split over time.  The window of windowed mode is added up anew for every label
// (BayesClassification.cc:144-147), so every (frame, class) of bayes_window_kernel is independent.  Both kernels only form the rows
// logN + sum; bayes_argmin_kernel takes the decision of every row that leaves (strict <, lowest index on ties, -1 without a winner).
// The library is compiled with -ffp-contract=off: w * s is rounded before it is added, in every place.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"

struct amx_bayes {
    amx_ctx*      ctx = nullptr;
    amx_bayes_cfg cfg{};
    long long     n_used = INT_MAX;   // INT_MAX: all frames
    long long     delay  = INT_MAX;   // INT_MAX: no continuous output
    int           window = 0;         // 0: no window
    float         log_n  = 0.f;
    amx::DevBuf<long long>          d_off;     // [n_seg + 1] absolute frame offsets
    amx::DevBuf<float>              d_rows;    // [frames x n_classes] logN + sum of the frames that emit (continuous, windowed)
    amx::DevBuf<float>              d_seg;     // [n_seg x n_classes] when the caller takes no segment scores
    amx::DevBuf<float>              d_gmm;     // amx_bayes_classify_gmm_dev: the score matrix
    amx::DevBuf<unsigned char>      d_emit;    // [frames] frame labels that leave, then [n_seg] segment labels that leave
    amx::DevBuf<unsigned long long> d_count;   // [0], [1]: labels without a winner (segments, frames); [2]: first refused weight
};

namespace amx {

constexpr int kBayesThreads  = 256;
constexpr int kBayesAhead    = 8;      // rows loaded ahead of the chain
constexpr int kBayesLdsWords = 8192;   // 32 KB of staged products per workgroup
constexpr unsigned long long kBayesNoFrame = ~0ull;

enum BayesKind { kSegment = 0, kContinuous = 1, kScores = 2 };

struct BayesSumArgs {
    const float*     scores;
    const float*     weights;   // WEIGHTED only
    const long long* off;       // [n_seg + 1]
    long long        base;      // off[0]: scratch rows are relative to it
    int              n_seg, n_classes, cpad;
    long long        scores_ld;
    long long        n_used, delay;
    int              single_frame;
    float            log_n;
    float*           rows;       // kContinuous: scratch [frames x n_classes]; kScores: out_dev
    long long        rows_ld;
    unsigned char*   emit;       // kContinuous: scratch [frames] (relative); kScores: emitted_dev (absolute)
    float*           seg_rows;   // [n_seg x n_classes]
    unsigned char*   seg_emit;   // [n_seg]
    float*           sum_of_weights;  // nullable
};

// the first frame (absolute row) of a scored range whose weight is not >= 0
__global__ void bayes_weights_kernel(const float* __restrict__ weights, const long long* __restrict__ off, long long n_used,
                                     unsigned long long* first_bad) {
    const long long a = off[blockIdx.x];
    long long       n = off[blockIdx.x + 1] - a;
    n                 = n < n_used ? n : n_used;
    unsigned long long bad = kBayesNoFrame;
    for (long long t = threadIdx.x; t < n; t += blockDim.x)
        if (!(weights[a + t] >= 0.f)) {
            bad = (unsigned long long)(a + t);
            break;   // this lane's frames only grow
        }
    if (bad != kBayesNoFrame)
        atomicMin(first_bad, bad);
}

// one lane per (segment, class): consecutive lanes take consecutive classes of one segment (cpad of them, a power of two up to 256 or a
// multiple of 256), a wave is filled up with further segments
template<int KIND, bool WEIGHTED>
__global__ __launch_bounds__(kBayesThreads) void bayes_sum_kernel(BayesSumArgs p) {
    const long long gid = (long long)blockIdx.x * kBayesThreads + threadIdx.x;
    const long long seg = gid / p.cpad;
    const int       c   = (int)(gid % p.cpad);
    if (seg >= p.n_seg || c >= p.n_classes)
        return;
    const long long a  = p.off[seg];
    long long       n  = p.off[seg + 1] - a;
    if (KIND == kSegment && n > p.n_used)
        n = p.n_used;
    const float* s  = p.scores + a * p.scores_ld + c;
    const float* w  = WEIGHTED ? p.weights + a : nullptr;
    float        sum = 0.f, sw = 0.f;
    long long    since = 0;       // kScores: frames since the sums were reset
    bool         pending = false; // frames came after the last vector / label
    for (long long t0 = 0; t0 < n; t0 += kBayesAhead) {
        float x[kBayesAhead], wt[kBayesAhead];
        // the loads do not depend on the chain: all of a block are issued before its adds
#pragma unroll
        for (int i = 0; i < kBayesAhead; ++i) {
            const bool in = t0 + i < n;
            x[i]  = in ? s[(t0 + i) * p.scores_ld] : 0.f;
            wt[i] = WEIGHTED ? (in ? w[t0 + i] : 0.f) : 1.f;
        }
#pragma unroll
        for (int i = 0; i < kBayesAhead; ++i) {
            const long long t = t0 + i;
            if (t >= n)
                break;
            const float prod = WEIGHTED ? wt[i] * x[i] : x[i];   // LikelihoodFunction.cc:77, rounded (the library is built without contraction)
            sum += prod;                                         // :80
            sw += wt[i];                                         // LikelihoodFunction.hh:55
            pending = true;
            if (KIND == kContinuous) {
                if (t >= p.delay) {   // nFeatures_ > delay_ (:108)
                    p.rows[(a - p.base + t) * p.rows_ld + c] = p.log_n + sum;
                    if (c == 0)
                        p.emit[a - p.base + t] = 1;
                    pending = false;
                }
            }
            if (KIND == kScores) {
                ++since;
                const bool leaves = since > p.delay;   // :186
                if (leaves) {
                    p.rows[(a + t) * p.rows_ld + c] = p.log_n + sum;
                    pending                         = false;
                    if (p.single_frame) {               // reset() after each vector (:440-441)
                        sum   = 0.f;
                        since = 0;
                    }
                }
                if (c == 0)
                    p.emit[a + t] = leaves ? 1 : 0;
            }
        }
    }
    if (KIND == kScores) {
        if (pending) {   // getScores() at the end of the stream (:434-437): into the row of the last frame
            p.rows[(a + n - 1) * p.rows_ld + c] = p.log_n + sum;
            if (c == 0)
                p.emit[a + n - 1] = 2;
        }
        return;
    }
    if (pending) {   // classify() at the end of the stream (:388-394), or the label of first-N mode after frame N - 1
        p.seg_rows[seg * p.n_classes + c] = p.log_n + sum;
        if (c == 0)
            p.seg_emit[seg] = 1;
    }
    if (c == 0 && p.sum_of_weights)
        p.sum_of_weights[seg] = sw;
}

struct BayesWindowArgs {
    const float*     scores;
    const float*     weights;
    const long long* off;
    long long        base, frames;
    int              n_seg, n_classes, cw, fpb;   // cw classes and fpb frames per workgroup
    long long        scores_ld;
    int              window;
    long long        delay;
    float            log_n;
    float*           rows;       // [frames x n_classes], relative
    unsigned char*   emit;       // [frames], relative
    float*           seg_rows;
    unsigned char*   seg_emit;
};

// one lane per (output frame, class).  STAGED: the products w * s of the workgroup's frames and the window - 1 frames before them are
// rounded once into LDS and every lane adds its window from there, newest frame first; otherwise (a window too long for LDS) each lane
// forms the same products from memory.
template<bool WEIGHTED, bool STAGED>
__global__ __launch_bounds__(kBayesThreads) void bayes_window_kernel(BayesWindowArgs p) {
    extern __shared__ float lds[];
    const long long f0 = (long long)blockIdx.x * p.fpb;             // first frame of the workgroup, relative to base
    const int       c0 = blockIdx.y * p.cw;
    long long       lo = f0 - (p.window - 1);
    lo                 = lo < 0 ? 0 : lo;
    long long hi       = f0 + p.fpb;
    hi                 = hi < p.frames ? hi : p.frames;
    if (STAGED) {
        const long long words = (hi - lo) * p.cw;
        for (long long i = threadIdx.x; i < words; i += kBayesThreads) {
            const long long r = lo + i / p.cw;
            const int       c = c0 + (int)(i % p.cw);
            float           v = 0.f;
            if (c < p.n_classes) {
                v = p.scores[(p.base + r) * p.scores_ld + c];
                if (WEIGHTED)
                    v = p.weights[p.base + r] * v;
            }
            lds[i] = v;
        }
        __syncthreads();
    }
    const long long outs = (hi - f0) * p.cw;
    for (long long i = threadIdx.x; i < outs; i += kBayesThreads) {
        const long long r = f0 + i / p.cw;
        const int       c = c0 + (int)(i % p.cw);
        if (c >= p.n_classes)
            continue;
        // the segment of frame base + r: the last one that starts at or before it (empty segments start where the next one does)
        const long long t = p.base + r;
        int             b = 0, e = p.n_seg;   // off[b] <= t < off[e]
        while (e - b > 1) {
            const int m = (b + e) / 2;
            if (p.off[m] <= t)
                b = m;
            else
                e = m;
        }
        const long long a  = p.off[b];
        const long long tl = t - a;                      // frame within the segment
        const bool      last = t + 1 == p.off[b + 1];
        // a label leaves once the window is full and, with a delay, d frames came since the last one (:110-113; nFeaturesBuffered_ counts
        // from 0): first after frame max(L, d) - 1, then every max(d, 1) frames
        bool leaves = tl >= p.window - 1;
        if (leaves && p.delay < INT_MAX) {
            const long long first = (p.delay > p.window ? p.delay : p.window) - 1;
            const long long step  = p.delay > 1 ? p.delay : 1;
            leaves                = tl >= first && (tl - first) % step == 0;
        }
        if (!leaves && !last)
            continue;
        const long long depth = tl + 1 < p.window ? tl + 1 : p.window;   // what the window holds
        float           score = p.log_n;
        for (long long j = 0; j < depth; ++j) {   // from the newest frame to the oldest (SlidingWindow.hh:369-371)
            float v;
            if (STAGED)
                v = lds[(r - j - lo) * p.cw + (c - c0)];
            else {
                v = p.scores[(t - j) * p.scores_ld + c];
                if (WEIGHTED)
                    v = p.weights[t - j] * v;
            }
            score += v;
        }
        if (leaves) {
            p.rows[r * p.n_classes + c] = score;
            if (c == 0)
                p.emit[r] = 1;
        }
        else {   // frames came after the last label, or the window never filled: the label at the end of the stream
            p.seg_rows[(long long)b * p.n_classes + c] = score;
            if (c == 0)
                p.seg_emit[b] = 1;
        }
    }
}

// sumOfWeights() of windowed mode: one lane per segment, in frame order
__global__ void bayes_weight_sum_kernel(const float* __restrict__ weights, const long long* __restrict__ off, int n_seg, float* out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg)
        return;
    float sw = 0.f;
    for (long long t = off[s]; t < off[s + 1]; ++t)
        sw += weights ? weights[t] : 1.f;
    out[s] = sw;
}

// argMin (:138-157) of every row that leaves: one lane per row, classes in order
__global__ void bayes_argmin_kernel(const float* __restrict__ rows, long long ld, long long n_rows, int n_classes, const unsigned char* __restrict__ emit,
                                    int32_t* label, unsigned long long* no_winner) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows)
        return;
    int32_t best = -1;
    if (emit[r]) {
        float        min_score = 3.402823466e+38f;   // Core::Type<f32>::max
        const float* row       = rows + r * ld;
        for (int c = 0; c < n_classes; ++c) {
            const float v = row[c];
            if (v < min_score) {
                min_score = v;
                best      = c;
            }
        }
        if (best < 0)
            atomicAdd(no_winner, 1ull);
    }
    label[r] = best;
}

static int pad_classes(int n) {
    if (n > 256)
        return (n + 255) / 256 * 256;
    int p = 1;
    while (p < n)
        p *= 2;
    return p;
}

// the checked segment table of a call, on the device; *frames = 0: nothing to do
static int bayes_segments(int n_seg, const long* frame_offsets, const char* who, std::vector<long long>* off, long long* frames) {
    AMX_REQUIRE(frame_offsets, AMX_ERR_INVALID, "%s: NULL segment list", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: negative frame offset", who);
    off->resize((size_t)n_seg + 1);
    for (int s = 0; s <= n_seg; ++s) {
        AMX_REQUIRE(s == 0 || frame_offsets[s - 1] <= frame_offsets[s], AMX_ERR_INVALID, "%s: frame offsets decrease at segment %d", who, s - 1);
        (*off)[s] = frame_offsets[s];
    }
    *frames = (*off)[n_seg] - (*off)[0];
    return AMX_OK;
}

static int bayes_check_weights(amx_bayes* h, int n_seg, const float* weights_dev, long long n_used, const char* who) {
    amx_ctx*                 ctx = h->ctx;
    const unsigned long long none = kBayesNoFrame;
    unsigned long long       bad  = none;
    AMX_HIP(hipMemcpyAsync(h->d_count.get() + 2, &none, sizeof(none), hipMemcpyHostToDevice, ctx->stream));
    {
        ScopedKernelTimer timer(ctx, "bayes_weights");
        hipLaunchKernelGGL(bayes_weights_kernel, dim3((unsigned)n_seg), dim3(kBayesThreads), 0, ctx->stream, weights_dev, h->d_off.get(), n_used,
                           h->d_count.get() + 2);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipMemcpyAsync(&bad, h->d_count.get() + 2, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    AMX_REQUIRE(bad == none, AMX_ERR_INVALID, "%s: Weight of frame %llu is smaller then zero or not a number; nothing was written", who, bad);
    return AMX_OK;
}

template<int KIND>
static int launch_sum(amx_ctx* ctx, const BayesSumArgs& a, const char* name) {
    const long long lanes  = (long long)a.n_seg * a.cpad;
    const long long groups = (lanes + kBayesThreads - 1) / kBayesThreads;
    AMX_REQUIRE(groups < (1ll << 31), AMX_ERR_INVALID, "%s: %d segments of %d classes are more than one call takes", name, a.n_seg, a.n_classes);
    ScopedKernelTimer timer(ctx, "bayes_sum");
    if (a.weights)
        hipLaunchKernelGGL((bayes_sum_kernel<KIND, true>), dim3((unsigned)groups), dim3(kBayesThreads), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((bayes_sum_kernel<KIND, false>), dim3((unsigned)groups), dim3(kBayesThreads), 0, ctx->stream, a);
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

static int launch_argmin(amx_ctx* ctx, const float* rows, long long ld, long long n_rows, int n_classes, const unsigned char* emit, int32_t* label,
                         unsigned long long* counter) {
    const long long groups = (n_rows + kBayesThreads - 1) / kBayesThreads;
    AMX_REQUIRE(groups < (1ll << 31), AMX_ERR_INVALID, "amx_bayes_classify_dev: %lld rows are more than one call takes", n_rows);
    ScopedKernelTimer timer(ctx, "bayes_argmin");
    hipLaunchKernelGGL(bayes_argmin_kernel, dim3((unsigned)groups), dim3(kBayesThreads), 0, ctx->stream, rows, ld, n_rows, n_classes, emit, label, counter);
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

}  // namespace amx

extern "C" {

void amx_bayes_default_cfg(amx_bayes_cfg* cfg) {
    if (!cfg)
        return;
    cfg->n_classes          = 0;
    cfg->number_of_features = INT_MAX;   // paramNumUsedFeatures (BayesClassification.cc:297-298)
    cfg->delay              = INT_MAX;   // paramDelay (:294-295)
    cfg->window_length      = -1;        // paramWindowLength (:300-301)
    cfg->window_right       = 0;         // paramWindowRight (:302-303)
    cfg->single_frame       = 0;         // paramSingleFrameClassification (:418-419)
}

int amx_bayes_create(amx_ctx* ctx, const amx_bayes_cfg* cfg, amx_bayes** out) {
    AMX_REQUIRE(out, AMX_ERR_INVALID, "amx_bayes_create: NULL argument");
    *out = nullptr;
    AMX_REQUIRE(cfg, AMX_ERR_INVALID, "amx_bayes_create: NULL argument");
    AMX_REQUIRE(cfg->n_classes >= 1, AMX_ERR_INVALID, "amx_bayes_create: n_classes is %d: Class labels not defined.", cfg->n_classes);
    std::unique_ptr<amx_bayes> h(new amx_bayes);
    h->ctx    = ctx;
    h->cfg    = *cfg;
    h->n_used = cfg->number_of_features <= 0 || cfg->number_of_features >= INT_MAX ? INT_MAX : cfg->number_of_features;
    h->delay  = cfg->delay < 0 || cfg->delay >= INT_MAX ? INT_MAX : cfg->delay;
    h->window = cfg->window_length > 0 ? cfg->window_length : 0;
    if (h->window) {
        // SlidingWindow::init (SlidingWindow.hh:401-412) returns false for maxSize <= right; a negative right is a huge size_t there
        AMX_REQUIRE(cfg->window_right >= 0 && cfg->window_right < cfg->window_length, AMX_ERR_INVALID,
                    "amx_bayes_create: window_right %d must be at least 0 and smaller than window_length %d", cfg->window_right, cfg->window_length);
        AMX_REQUIRE(h->n_used == INT_MAX, AMX_ERR_INVALID, "amx_bayes_create: number_of_features %ld cannot be combined with window_length %d",
                    cfg->number_of_features, cfg->window_length);
    }
    AMX_REQUIRE(h->n_used == INT_MAX || h->delay == INT_MAX, AMX_ERR_INVALID, "amx_bayes_create: number_of_features %ld cannot be combined with delay %ld",
                cfg->number_of_features, cfg->delay);
    h->log_n = std::log((float)cfg->n_classes);   // AprioriProbability.cc:20: the float overload
    *out     = h.release();
    return AMX_OK;
}

void amx_bayes_destroy(amx_bayes* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_bayes_prior(const amx_bayes* h, float* log_n_classes) {
    AMX_REQUIRE(h && log_n_classes, AMX_ERR_INVALID, "amx_bayes_prior: NULL argument");
    *log_n_classes = h->log_n;
    return AMX_OK;
}

int amx_bayes_classify_dev(amx_bayes* h, int n_seg, const long* frame_offsets, const float* scores_dev, int scores_ld, const float* weights_dev,
                           int32_t* segment_label_dev, float* segment_score_dev, int32_t* frame_label_dev, float* sum_of_weights_dev,
                           unsigned long long no_winner[2]) {
    const char* who = "amx_bayes_classify_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    const int C = h->cfg.n_classes;
    AMX_REQUIRE(n_seg >= 0 && scores_ld >= C, AMX_ERR_INVALID, "%s: n_seg %d, scores_ld %d with %d classes", who, n_seg, scores_ld, C);
    if (no_winner)
        no_winner[0] = no_winner[1] = 0;
    if (n_seg == 0)
        return AMX_OK;
    const bool per_frame = h->window > 0 || h->delay < INT_MAX;
    std::vector<long long> off;
    long long              T = 0;
    AMX_TRY(amx::bayes_segments(n_seg, frame_offsets, who, &off, &T));
    AMX_REQUIRE(segment_label_dev, AMX_ERR_INVALID, "%s: NULL segment_label_dev", who);
    AMX_REQUIRE(T == 0 || scores_dev, AMX_ERR_INVALID, "%s: NULL scores_dev", who);
    AMX_REQUIRE(T == 0 || !per_frame || frame_label_dev, AMX_ERR_INVALID, "%s: continuous and windowed mode need frame_label_dev", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_TRY(h->d_off.reserve(off.size()));
    AMX_HIP(hipMemcpyAsync(h->d_off.get(), off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    AMX_TRY(h->d_count.reserve(3));
    if (weights_dev && T)
        AMX_TRY(amx::bayes_check_weights(h, n_seg, weights_dev, h->n_used, who));
    const size_t n_emit = (size_t)(per_frame ? T : 0) + (size_t)n_seg;
    AMX_TRY(h->d_emit.reserve(n_emit));
    AMX_HIP(hipMemsetAsync(h->d_emit.get(), 0, n_emit, ctx->stream));
    AMX_HIP(hipMemsetAsync(h->d_count.get(), 0, 2 * sizeof(unsigned long long), ctx->stream));
    unsigned char* frame_emit = h->d_emit.get();
    unsigned char* seg_emit   = h->d_emit.get() + (per_frame ? T : 0);
    float*         seg_rows   = segment_score_dev;
    if (!seg_rows) {
        AMX_TRY(h->d_seg.reserve((size_t)n_seg * C));
        seg_rows = h->d_seg.get();
    }
    if (per_frame && T)
        AMX_TRY(h->d_rows.reserve((size_t)T * C));
    if (h->window == 0) {
        amx::BayesSumArgs a{};
        a.scores = scores_dev, a.weights = weights_dev, a.off = h->d_off.get(), a.base = off[0];
        a.n_seg = n_seg, a.n_classes = C, a.cpad = amx::pad_classes(C);
        a.scores_ld = scores_ld, a.n_used = h->n_used, a.delay = h->delay, a.single_frame = 0, a.log_n = h->log_n;
        a.rows = h->d_rows.get(), a.rows_ld = C, a.emit = frame_emit, a.seg_rows = seg_rows, a.seg_emit = seg_emit;
        a.sum_of_weights = sum_of_weights_dev;
        if (per_frame)
            AMX_TRY(amx::launch_sum<amx::kContinuous>(ctx, a, who));
        else
            AMX_TRY(amx::launch_sum<amx::kSegment>(ctx, a, who));
    }
    else {
        if (T) {
            amx::BayesWindowArgs a{};
            a.scores = scores_dev, a.weights = weights_dev, a.off = h->d_off.get(), a.base = off[0], a.frames = T;
            a.n_seg = n_seg, a.n_classes = C, a.cw = std::min(amx::pad_classes(C), amx::kBayesThreads);
            a.scores_ld = scores_ld, a.window = h->window, a.delay = h->delay, a.log_n = h->log_n;
            a.rows = h->d_rows.get(), a.emit = frame_emit, a.seg_rows = seg_rows, a.seg_emit = seg_emit;
            // frames per workgroup: what LDS holds besides the window - 1 frames in front, at most eight outputs per lane; a window that
            // leaves no room for one output per lane is read from memory instead
            const int       per_pass = amx::kBayesThreads / a.cw;
            const long long room     = amx::kBayesLdsWords / a.cw - (h->window - 1);
            const bool      staged   = room >= per_pass;
            a.fpb                    = staged ? (int)std::min<long long>(room, 8 * per_pass) : per_pass;
            const long long gx = (T + a.fpb - 1) / a.fpb;
            const int       gy = (C + a.cw - 1) / a.cw;
            AMX_REQUIRE(gx < (1ll << 31) && gy < 65536, AMX_ERR_INVALID, "%s: %lld frames of %d classes are more than one call takes", who, T, C);
            const size_t lds = staged ? (size_t)(a.fpb + h->window - 1) * a.cw * sizeof(float) : 0;
            amx::ScopedKernelTimer timer(ctx, "bayes_window");
            const dim3 grid((unsigned)gx, (unsigned)gy), block(amx::kBayesThreads);
            if (staged && weights_dev)
                hipLaunchKernelGGL((amx::bayes_window_kernel<true, true>), grid, block, lds, ctx->stream, a);
            else if (staged)
                hipLaunchKernelGGL((amx::bayes_window_kernel<false, true>), grid, block, lds, ctx->stream, a);
            else if (weights_dev)
                hipLaunchKernelGGL((amx::bayes_window_kernel<true, false>), grid, block, lds, ctx->stream, a);
            else
                hipLaunchKernelGGL((amx::bayes_window_kernel<false, false>), grid, block, lds, ctx->stream, a);
            AMX_HIP(hipGetLastError());
        }
        if (sum_of_weights_dev) {
            hipLaunchKernelGGL(amx::bayes_weight_sum_kernel, dim3((unsigned)amx::ceil_div(n_seg, amx::kBayesThreads)), dim3(amx::kBayesThreads), 0, ctx->stream,
                               weights_dev, h->d_off.get(), n_seg, sum_of_weights_dev);
            AMX_HIP(hipGetLastError());
        }
    }
    AMX_TRY(amx::launch_argmin(ctx, seg_rows, C, n_seg, C, seg_emit, segment_label_dev, h->d_count.get()));
    if (per_frame && T)
        AMX_TRY(amx::launch_argmin(ctx, h->d_rows.get(), C, T, C, frame_emit, frame_label_dev + off[0], h->d_count.get() + 1));
    if (no_winner) {
        AMX_HIP(hipMemcpyAsync(no_winner, h->d_count.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return AMX_OK;
}

int amx_bayes_scores_dev(amx_bayes* h, int n_seg, const long* frame_offsets, const float* scores_dev, int scores_ld, const float* weights_dev,
                         float* out_dev, int out_ld, uint8_t* emitted_dev) {
    const char* who = "amx_bayes_scores_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    const int C = h->cfg.n_classes;
    AMX_REQUIRE(n_seg >= 0 && scores_ld >= C && out_ld >= C, AMX_ERR_INVALID, "%s: n_seg %d, scores_ld %d, out_ld %d with %d classes", who, n_seg, scores_ld,
                out_ld, C);
    if (n_seg == 0)
        return AMX_OK;
    std::vector<long long> off;
    long long              T = 0;
    AMX_TRY(amx::bayes_segments(n_seg, frame_offsets, who, &off, &T));
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(scores_dev && out_dev && emitted_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_TRY(h->d_off.reserve(off.size()));
    AMX_HIP(hipMemcpyAsync(h->d_off.get(), off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    AMX_TRY(h->d_count.reserve(3));
    if (weights_dev)
        AMX_TRY(amx::bayes_check_weights(h, n_seg, weights_dev, INT_MAX, who));
    amx::BayesSumArgs a{};
    a.scores = scores_dev, a.weights = weights_dev, a.off = h->d_off.get(), a.base = off[0];
    a.n_seg = n_seg, a.n_classes = C, a.cpad = amx::pad_classes(C);
    a.scores_ld = scores_ld, a.n_used = INT_MAX, a.delay = h->delay, a.single_frame = h->cfg.single_frame ? 1 : 0, a.log_n = h->log_n;
    a.rows = out_dev, a.rows_ld = out_ld, a.emit = emitted_dev;
    return amx::launch_sum<amx::kScores>(ctx, a, who);
}

int amx_bayes_classify_gmm_dev(amx_bayes* h, amx_gmm* gmm, int mode, int n_seg, const long* frame_offsets, const float* feats_dev, const float* weights_dev,
                               int32_t* segment_label_dev, float* segment_score_dev, int32_t* frame_label_dev, float* sum_of_weights_dev,
                               unsigned long long no_winner[2]) {
    const char* who = "amx_bayes_classify_gmm_dev";
    AMX_REQUIRE(h && gmm, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    const int C = h->cfg.n_classes;
    AMX_REQUIRE(amx_gmm_n_mixtures(gmm) == C, AMX_ERR_INVALID, "%s: Number of mixtures (%d) does not match to the number of classes (%d).", who,
                amx_gmm_n_mixtures(gmm), C);
    AMX_REQUIRE(n_seg >= 0, AMX_ERR_INVALID, "%s: n_seg %d", who, n_seg);
    if (n_seg == 0) {
        if (no_winner)
            no_winner[0] = no_winner[1] = 0;
        return AMX_OK;
    }
    std::vector<long long> off;
    long long              T = 0;
    AMX_TRY(amx::bayes_segments(n_seg, frame_offsets, who, &off, &T));
    AMX_REQUIRE(T <= INT_MAX, AMX_ERR_INVALID, "%s: %lld frames are more than one call takes", who, T);
    std::vector<long> rel((size_t)n_seg + 1);   // the handle's score matrix starts at the call's first frame
    for (int s = 0; s <= n_seg; ++s)
        rel[s] = (long)(off[s] - off[0]);
    if (T) {
        AMX_REQUIRE(feats_dev, AMX_ERR_INVALID, "%s: NULL feats_dev", who);
        AMX_HIP(hipSetDevice(h->ctx->device));
        AMX_TRY(h->d_gmm.reserve((size_t)T * C));
        AMX_TRY(amx_gmm_score_dev(gmm, mode, feats_dev + off[0] * amx_gmm_dimension(gmm), (int)T, h->d_gmm.get(), nullptr));
    }
    return amx_bayes_classify_dev(h, n_seg, rel.data(), h->d_gmm.get(), C, weights_dev ? weights_dev + off[0] : nullptr, segment_label_dev, segment_score_dev,
                                  frame_label_dev ? frame_label_dev + off[0] : nullptr, sum_of_weights_dev, no_winner);
}

}  // extern "C"
