// accuracy.hip -- the accuracies of a word lattice's arcs (include/amx.h, section "Lattice arc accuracies"): what Lattice/Accuracy.cc
// computes per arc for MPE (getApproximatePhoneAccuracy), the frame-phone variant (getFramePhoneAccuracy) and state-level MBR
// (getFrameStateAccuracy), from the aligned labels or emission indices amx_arcalign_run_dev has left in device memory.  An arc's value
// depends only on its key and on the segment's reference, so the unit of work is the key and a gather puts the values into arc order.
//
// Four kernels.  accuracy_check_kernel (a wave per key) refuses items outside the tables before anything is written.
// accuracy_runs_kernel (a wave per reference key) cuts the key's tokens into runs, 64 frames per trip, a ballot and a popcount prefix
// giving each run its place in the segment's slice of a run buffer; places come from integer counters, so their order is free and the
// sort removes it.  accuracy_table_kernel (a workgroup per segment) sorts the slice by (start, end, token) with a bitonic network --
// in LDS, or in a global workspace when the slice is larger than LDS holds: the same code on another pointer, so the bits are the same
// -- drops duplicates and writes the table with a running maximum of `end`, which makes the intervals that can overlap a run one
// window between two binary searches.  In state mode every frame of a reference key is a run of its own, so the same table is the
// sorted unique (frame, token) list.  accuracy_key_kernel (four waves per workgroup, all on keys of one segment) stages the table
// into LDS once and then loops over keys without a workgroup barrier: runs are extracted in registers, a run that crosses a trip is
// carried in wave-uniform scalars, the lanes stride over a run's window (approximate), stand for the run's frames (frame-phone) or for
// the key's frames (frame-state), and lane 0's chain is the key's value.  The arithmetic is integer but for one f32 division per
// interval or run and the chain; there are no floating-point atomics and no sum whose order depends on the batch.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <numeric>

#include "common.hpp"

namespace amx {

constexpr int kAccWaves        = 4;      // waves per workgroup of the check, runs and key kernels
constexpr int kAccThreads      = 64 * kAccWaves;
constexpr int kAccTripFrames   = 64;     // frames a wave takes per trip: one per lane
// Keys a workgroup of the key kernel takes (16 per wave) and intervals a workgroup keeps in LDS.  Chosen, not tuned: 64 keys spread
// the staging of a table over enough work, 2048 intervals are 24 KB in the sort and 32 KB in the key kernel, four workgroups per CU.
constexpr int kAccGroupKeys    = 64;
constexpr int kAccLdsIntervals = 2048;
static_assert((kAccLdsIntervals & (kAccLdsIntervals - 1)) == 0 && kAccLdsIntervals * 16 * 4 <= 160 * 1024, "a power of two, four workgroups per CU");

struct AccKey {
    int slot0, tbeg, frames, seg, out;   // out: the key's index in the caller's order
};
struct AccGroup {
    int seg, first, n;   // keys [first, first + n) of the segment-ordered list
};
enum { kAccBad = 0, kAccRuns = 1, kAccNoAlignment = 2, kAccIntervals = 3, kAccCounters = 4 };

struct AccArgs {
    const AccKey*         key;          // ordered by segment
    int                   n_keys;
    const AccGroup*       group;
    const int*            ref;          // the reference keys, as indices into key
    int                   n_ref;
    const int32_t*        item;
    const int32_t*        label_token;  // nullable: the item is the token
    int                   item_limit;   // items are in [-1, item_limit)
    const unsigned char*  short_pause;  // by token
    const int*            seg_off;      // [n_seg + 1]: the segments' slices of the run buffer and of the table
    const long long*      seg_sort_off; // [n_seg]: a segment's place in the global sort workspace
    int*                  seg_runs;     // [n_seg] runs written; seg_n: [n_seg] intervals of the table
    int*                  seg_n;
    unsigned long long*   run_key;      // start << 32 | end
    int*                  run_tok;
    unsigned long long*   sort_key;
    int*                  sort_tok;
    int *                 tab_start, *tab_end, *tab_tok, *tab_maxend;
    int                   lds_cap;
    int                   per_frame;    // state mode: every frame is a run
    float                 normalization;
    float*                key_acc;
    unsigned long long*   counters;     // [kAccCounters]
};

__device__ __forceinline__ int acc_token(const AccArgs& p, int item) {
    return p.label_token ? p.label_token[item] : item;
}

// Items outside [-1, limit) and keys that mix -1 with labels; the first offender by slot wins (slot << 32 | item).
__global__ __launch_bounds__(kAccThreads) void accuracy_check_kernel(AccArgs p) {
    const int k = blockIdx.x * kAccWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= p.n_keys)
        return;
    const AccKey   key   = p.key[k];
    const int32_t* item  = p.item + key.slot0;
    const int      first = item[0];
    for (int f = lane; f < key.frames; f += 64) {
        const int v = item[f];
        if (v < -1 || v >= p.item_limit || (v < 0) != (first < 0))
            atomicMin(&p.counters[kAccBad], ((unsigned long long)(unsigned)(key.slot0 + f) << 32) | (unsigned)v);
    }
    if (lane == 0 && first == -1)
        atomicAdd(&p.counters[kAccNoAlignment], 1ull);
}

// One trip of a key's run extraction.  Lane l looks at frame f0 + l; frame T is a sentinel that closes the last run.  A lane whose bit
// is set in `closed` ends a run there: [hs, f0 + l) with token tok, frames relative to the key.  carry_*: the open run, wave-uniform.
struct AccTrip {
    unsigned long long closed;
    int                hs, tok;
};
__device__ __forceinline__ AccTrip acc_trip(const AccArgs& p, const int32_t* item, int T, int f0, int lane, bool per_frame, int& carry_start,
                                            int& carry_tok) {
    const int  f    = f0 + lane;
    const int  tok  = f < T ? acc_token(p, item[f]) : -2;
    const int  up   = __shfl_up(tok, 1, 64);
    const int  prev = lane == 0 ? carry_tok : up;
    const bool flag = f <= T && (per_frame || tok != prev);
    const unsigned long long m     = __ballot(flag);
    const unsigned long long below = m & ((1ull << lane) - 1ull);
    const int  pl   = below ? 63 - __clzll((long long)below) : -1;
    const int  ptok = __shfl(tok, pl < 0 ? 0 : pl, 64);
    AccTrip    r;
    r.hs     = pl >= 0 ? f0 + pl : carry_start;
    r.tok    = pl >= 0 ? ptok : carry_tok;
    r.closed = __ballot(flag && r.hs >= 0);
    if (m) {
        const int last = 63 - __clzll((long long)m);
        carry_start    = f0 + last;
        carry_tok      = __shfl(tok, last, 64);
    }
    return r;
}

__global__ __launch_bounds__(kAccThreads) void accuracy_runs_kernel(AccArgs p) {
    const int ri = blockIdx.x * kAccWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ri >= p.n_ref)
        return;
    const AccKey   key  = p.key[p.ref[ri]];
    const int32_t* item = p.item + key.slot0;
    if (item[0] < 0)   // no final state reached: no runs
        return;
    const int off         = p.seg_off[key.seg];
    int       carry_start = -1, carry_tok = -2;
    for (int f0 = 0; f0 <= key.frames; f0 += kAccTripFrames) {
        const AccTrip t = acc_trip(p, item, key.frames, f0, lane, p.per_frame != 0, carry_start, carry_tok);
        const int     n = __popcll(t.closed);
        int           base = 0;
        if (lane == 0 && n)
            base = atomicAdd(&p.seg_runs[key.seg], n);
        base = __shfl(base, 0, 64);
        if ((t.closed >> lane) & 1ull) {
            const int pos  = off + base + __popcll(t.closed & ((1ull << lane) - 1ull));
            p.run_key[pos] = ((unsigned long long)(unsigned)(key.tbeg + t.hs) << 32) | (unsigned)(key.tbeg + f0 + lane);
            p.run_tok[pos] = t.tok;
        }
    }
}

// One workgroup per segment: sort, drop duplicates, running maximum of end.
__global__ __launch_bounds__(kAccThreads) void accuracy_table_kernel(AccArgs p) {
    __shared__ unsigned long long skey[kAccLdsIntervals];
    __shared__ int                stok[kAccLdsIntervals];
    __shared__ int                wsum[kAccWaves], wmax[kAccWaves];
    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = p.seg_runs[seg], off = p.seg_off[seg];
    int       npad = 1;
    while (npad < n)
        npad <<= 1;
    unsigned long long* K  = skey;   // generic: LDS when the slice fits
    int*                Tk = stok;
    if (npad > p.lds_cap)
        K = p.sort_key + p.seg_sort_off[seg], Tk = p.sort_tok + p.seg_sort_off[seg];
    for (int i = tid; i < npad; i += kAccThreads) {
        K[i]  = i < n ? p.run_key[off + i] : ~0ull;
        Tk[i] = i < n ? p.run_tok[off + i] : INT_MAX;
    }
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += kAccThreads) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = K[i], b = K[x];
                    const int                ta = Tk[i], tb = Tk[x];
                    const bool               gt = a > b || (a == b && ta > tb);
                    if (gt == ((i & k) == 0))
                        K[i] = b, K[x] = a, Tk[i] = tb, Tk[x] = ta;
                }
            }
            __syncthreads();
        }
    int base = 0, carry_max = 0;   // every end is >= 1
    for (int i0 = 0; i0 < n; i0 += kAccThreads) {
        const int                i   = i0 + tid;
        const bool               in  = i < n;
        const unsigned long long key = in ? K[i] : 0;
        const int                tok = in ? Tk[i] : 0;
        // the element before, by an index that never goes below 0: K may be a flat pointer to the start of LDS, and an address formed
        // below an aperture's base is refused by the hardware even where the instruction's offset brings it back inside
        const int                ib   = i > 0 ? i - 1 : 0;
        const bool               uniq = in && (i == 0 || K[ib] != key || Tk[ib] != tok);
        const int                end  = in ? (int)(unsigned)key : 0;
        int                      s = uniq ? 1 : 0, mx = end;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int us = __shfl_up(s, o, 64), um = __shfl_up(mx, o, 64);
            if (lane >= o)
                s += us, mx = um > mx ? um : mx;
        }
        if (lane == 63)
            wsum[w] = s, wmax[w] = mx;
        __syncthreads();
        int pre = 0, pmx = carry_max, tot = 0, tmx = carry_max;
        for (int j = 0; j < kAccWaves; ++j) {
            if (j < w)
                pre += wsum[j], pmx = wmax[j] > pmx ? wmax[j] : pmx;
            tot += wsum[j], tmx = wmax[j] > tmx ? wmax[j] : tmx;
        }
        if (uniq) {
            const int pos     = off + base + pre + s - 1;
            p.tab_start[pos]  = (int)(key >> 32);
            p.tab_end[pos]    = end;
            p.tab_tok[pos]    = tok;
            p.tab_maxend[pos] = mx > pmx ? mx : pmx;
        }
        base += tot, carry_max = tmx;
        __syncthreads();
    }
    if (tid == 0) {
        p.seg_n[seg] = base;
        atomicAdd(&p.counters[kAccIntervals], (unsigned long long)base);
    }
}

__device__ __forceinline__ float acc_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v             = u > v ? u : v;
    }
    return v;
}

// first i in [0, n) with a[i] > v (GT) or a[i] >= v; a ascending
template<bool GT>
__device__ __forceinline__ int acc_bound(const int* a, int n, int v) {
    int b = 0, e = n;
    while (b < e) {
        const int m = (b + e) >> 1;
        if (GT ? a[m] > v : a[m] >= v)
            e = m;
        else
            b = m + 1;
    }
    return b;
}

// Every value that steers control flow outside the per-lane code is the same in all lanes of the wave: it comes from the key, the
// table's size, a ballot or a broadcast.
template<int MODE, bool FMA>
__global__ __launch_bounds__(kAccThreads) void accuracy_key_kernel(AccArgs p) {
    __shared__ int  ls[kAccLdsIntervals], le[kAccLdsIntervals], lt[kAccLdsIntervals], lm[kAccLdsIntervals];
    const AccGroup  grp  = p.group[blockIdx.x];
    const int       lane = threadIdx.x & 63, n = p.seg_n[grp.seg], off = p.seg_off[grp.seg];
    const int *     S = p.tab_start + off, *E = p.tab_end + off, *K = p.tab_tok + off, *M = p.tab_maxend + off;   // generic
    if (n <= p.lds_cap) {
        for (int i = threadIdx.x; i < n; i += kAccThreads)
            ls[i] = S[i], le[i] = E[i], lt[i] = K[i], lm[i] = M[i];
        S = ls, E = le, K = lt, M = lm;
    }
    __syncthreads();
    for (int ki = grp.first + (threadIdx.x >> 6); ki < grp.first + grp.n; ki += kAccWaves) {
        const AccKey   key  = p.key[ki];
        const int32_t* item = p.item + key.slot0;
        const int      T    = key.frames;
        float          chain = 0.f;
        int            n_runs = 0;
        if (item[0] >= 0) {
            if (MODE == AMX_ACCURACY_FRAME_STATE) {
                int cnt = 0;
                for (int f0 = 0; f0 < T; f0 += kAccTripFrames) {
                    const int f   = f0 + lane;
                    bool      hit = false;
                    if (f < T) {
                        const int tok = acc_token(p, item[f]);
                        if (!p.short_pause[tok]) {
                            const int sf = key.tbeg + f;
                            for (int i = acc_bound<false>(S, n, sf); i < n && S[i] == sf && !hit; ++i)   // the frame's short list
                                hit = K[i] == tok;
                        }
                    }
                    cnt += __popcll(__ballot(hit));
                }
                chain  = (float)cnt;   // a chain of + 1.f from 0: exact
                n_runs = T;
            }
            else {
                int carry_start = -1, carry_tok = -2;
                for (int f0 = 0; f0 <= T; f0 += kAccTripFrames) {
                    const AccTrip      t = acc_trip(p, item, T, f0, lane, false, carry_start, carry_tok);
                    unsigned long long c = t.closed;
                    n_runs += __popcll(c);
                    while (c) {   // the trip's runs in frame order
                        const int j = __ffsll((long long)c) - 1;
                        c &= c - 1;
                        const int hs = key.tbeg + __shfl(t.hs, j, 64), he = key.tbeg + f0 + j, tk = __shfl(t.tok, j, 64);
                        if (p.short_pause[tk])
                            continue;
                        const int lo = acc_bound<true>(M, n, hs), hi = acc_bound<false>(S, n, he);   // rs < he holds below hi
                        float     v;
                        if (MODE == AMX_ACCURACY_APPROXIMATE_PHONE) {
                            float best = -3.40282347e+38f;
                            bool  any  = false;
                            for (int i = lo + lane; i < hi; i += 64) {
                                const int rs = S[i], re = E[i];
                                if (re > hs) {
                                    const float o = (float)((he < re ? he : re) - (hs > rs ? hs : rs)) / (float)(re - rs);
                                    const float a = -1.f + (K[i] == tk ? 2.f : 1.f) * o;
                                    best = a > best ? a : best, any = true;
                                }
                            }
                            best = acc_wave_max(best);
                            v    = __any(any) ? best : 0.f;
                        }
                        else {
                            int count = 0;
                            for (int c0 = hs; c0 < he; c0 += 64) {
                                const int f   = c0 + lane;
                                bool      cov = false;
                                if (f < he)
                                    for (int i = lo; i < hi && !cov; ++i)
                                        cov = K[i] == tk && S[i] <= f && f < E[i];
                                count += __popcll(__ballot(cov));
                            }
                            v = (float)count / mad<FMA>(p.normalization, (float)(unsigned)(he - hs - 1), 1.f);
                        }
                        chain = chain + v;
                    }
                }
            }
        }
        if (lane == 0) {
            p.key_acc[key.out] = chain;
            atomicAdd(&p.counters[kAccRuns], (unsigned long long)n_runs);
        }
    }
}

__global__ __launch_bounds__(256) void accuracy_gather_kernel(const float* __restrict__ key_acc, const int* __restrict__ arc_key, int n_arcs,
                                                             float* __restrict__ out) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a < n_arcs)
        out[a] = arc_key[a] < 0 ? 0.f : key_acc[arc_key[a]];   // no pronunciation: weight 0 (Accuracy.cc:604-606)
}

template<class T>
static int acc_upload(amx_ctx* ctx, DevBuf<T>& d, const std::vector<T>& v) {
    AMX_TRY(d.reserve(v.size() ? v.size() : 1));
    if (!v.empty())
        AMX_HIP(hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return AMX_OK;
}

}  // namespace amx

struct amx_accuracy {
    amx_ctx*                   ctx = nullptr;
    int                        mode = 0, n_labels = 0, n_tokens = 0, lds_cap = amx::kAccLdsIntervals;
    float                      normalization = 0.f;
    bool                       has_table = false, tables_on_device = false;
    std::vector<int32_t>       label_token;
    std::vector<unsigned char> short_pause;
    // of the last call: the uploads read the host tables until the call's synchronisation
    std::vector<amx::AccKey>   keys;
    std::vector<amx::AccGroup> groups;
    std::vector<int>           ref, seg_off, arc_key;
    std::vector<long long>     seg_sort_off;
    amx::DevBuf<amx::AccKey>   d_key;
    amx::DevBuf<amx::AccGroup> d_group;
    amx::DevBuf<int>           d_ref, d_seg_off, d_seg_count, d_run_tok, d_sort_tok, d_tab, d_arc_key;
    amx::DevBuf<int32_t>       d_label_token;
    amx::DevBuf<unsigned char> d_short_pause;
    amx::DevBuf<long long>     d_seg_sort_off;
    amx::DevBuf<unsigned long long> d_run_key, d_sort_key, d_counters;
    amx::DevBuf<float>         d_key_acc;
    int                        n_keys = -1, n_seg = 0;   // of the last run; -1: none
};

extern "C" {

int amx_accuracy_create(amx_ctx* ctx, const amx_accuracy_cfg* cfg, amx_accuracy** out) {
    const char* who = "amx_accuracy_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(cfg, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(cfg->mode == AMX_ACCURACY_APPROXIMATE_PHONE || cfg->mode == AMX_ACCURACY_FRAME_PHONE || cfg->mode == AMX_ACCURACY_FRAME_STATE, AMX_ERR_INVALID,
                "%s: mode %d is none (approximate word accuracy, the mask, soft and weighted variants and the exact accuracies are not built)", who, cfg->mode);
    AMX_REQUIRE(std::isfinite(cfg->normalization), AMX_ERR_INVALID, "%s: normalization %g is not finite", who, (double)cfg->normalization);
    AMX_REQUIRE(cfg->n_tokens >= 1 && cfg->n_labels >= 0, AMX_ERR_INVALID, "%s: n_tokens %d, n_labels %d", who, cfg->n_tokens, cfg->n_labels);
    AMX_REQUIRE(!cfg->label_token || cfg->n_labels >= 1, AMX_ERR_INVALID, "%s: a label_token table of %d labels", who, cfg->n_labels);
    for (int l = 0; cfg->label_token && l < cfg->n_labels; ++l)
        AMX_REQUIRE(cfg->label_token[l] >= 0 && cfg->label_token[l] < cfg->n_tokens, AMX_ERR_INVALID, "%s: label_token[%d] = %d outside the %d tokens", who, l,
                    cfg->label_token[l], cfg->n_tokens);
    std::unique_ptr<amx_accuracy> h(new amx_accuracy);
    h->ctx = ctx, h->mode = cfg->mode, h->normalization = cfg->normalization, h->n_labels = cfg->n_labels, h->n_tokens = cfg->n_tokens;
    h->has_table = cfg->label_token != nullptr;
    if (h->has_table)
        h->label_token.assign(cfg->label_token, cfg->label_token + cfg->n_labels);
    h->short_pause.assign((size_t)cfg->n_tokens, 0);
    for (int t = 0; cfg->short_pause && t < cfg->n_tokens; ++t)
        h->short_pause[t] = cfg->short_pause[t] ? 1 : 0;
    *out = h.release();
    return AMX_OK;
}

void amx_accuracy_destroy(amx_accuracy* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

void amx_accuracy_kernel_shape(int* keys_per_workgroup, int* frames_per_trip, int* lds_intervals) {
    if (keys_per_workgroup)
        *keys_per_workgroup = amx::kAccGroupKeys;
    if (frames_per_trip)
        *frames_per_trip = amx::kAccTripFrames;
    if (lds_intervals)
        *lds_intervals = amx::kAccLdsIntervals;
}

int amx_accuracy_set_lds_intervals(amx_accuracy* h, int n) {
    AMX_REQUIRE(h && n >= 0 && n <= amx::kAccLdsIntervals, AMX_ERR_INVALID, "amx_accuracy_set_lds_intervals: NULL handle or %d outside [0, %d]", n,
                amx::kAccLdsIntervals);
    h->lds_cap = n ? n : amx::kAccLdsIntervals;
    return AMX_OK;
}

int amx_accuracy_run_dev(amx_accuracy* h, int n_keys, const int* key_segment, const int* key_tbeg, const int* key_tend, const long* slot_offsets,
                         const unsigned char* key_is_reference, const int32_t* item_dev, int n_seg, float* key_accuracy_dev, amx_accuracy_info* info) {
    const char* who = "amx_accuracy_run_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_keys >= 0 && n_seg >= 0, AMX_ERR_INVALID, "%s: n_keys %d, n_seg %d", who, n_keys, n_seg);
    if (info)
        *info = amx_accuracy_info{0, 0, 0};
    if (n_keys == 0)
        return AMX_OK;
    AMX_REQUIRE(key_segment && key_tbeg && key_tend && slot_offsets && key_is_reference, AMX_ERR_INVALID, "%s: NULL key table", who);
    AMX_REQUIRE(slot_offsets[0] == 0, AMX_ERR_INVALID, "%s: slot_offsets start at %ld, not at 0", who, slot_offsets[0]);
    for (int k = 0; k < n_keys; ++k) {
        AMX_REQUIRE(key_segment[k] >= 0 && key_segment[k] < n_seg, AMX_ERR_INVALID, "%s: key %d: segment %d outside the %d segments", who, k, key_segment[k], n_seg);
        AMX_REQUIRE(key_tbeg[k] < key_tend[k], AMX_ERR_INVALID, "%s: key %d: begin time %d is not below end time %d (such an arc has key -1)", who, k, key_tbeg[k],
                    key_tend[k]);
        AMX_REQUIRE(key_tbeg[k] >= 0, AMX_ERR_INVALID, "%s: key %d: begin time %d is negative", who, k, key_tbeg[k]);
        AMX_REQUIRE(slot_offsets[k + 1] - slot_offsets[k] == (long)key_tend[k] - key_tbeg[k], AMX_ERR_INVALID,
                    "%s: key %d: slot_offsets give it %ld slots, its window [%d, %d) has %d frames", who, k, slot_offsets[k + 1] - slot_offsets[k], key_tbeg[k],
                    key_tend[k], key_tend[k] - key_tbeg[k]);
        AMX_REQUIRE(slot_offsets[k + 1] < (1l << 31), AMX_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 frames over all keys (at key %d)", who, k);
    }
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(item_dev && key_accuracy_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    // the keys by segment (the index breaks ties, so a call's dealing is a function of its input), groups of one segment's keys, the
    // reference keys and the segments' slices: a slice holds one run per frame of the segment's reference keys at the most
    std::vector<int> order(n_keys);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key_segment[a] < key_segment[b]; });
    h->keys.resize(n_keys), h->groups.clear(), h->ref.clear();
    h->seg_off.assign((size_t)n_seg + 1, 0);
    long long cap = 0;
    for (int i = 0; i < n_keys; ++i) {
        const int k = order[i];
        h->keys[i]  = amx::AccKey{(int)slot_offsets[k], key_tbeg[k], key_tend[k] - key_tbeg[k], key_segment[k], k};
        if (h->groups.empty() || h->groups.back().seg != key_segment[k] || h->groups.back().n == amx::kAccGroupKeys)
            h->groups.push_back(amx::AccGroup{key_segment[k], i, 0});
        ++h->groups.back().n;
        if (key_is_reference[k]) {
            h->ref.push_back(i);
            h->seg_off[(size_t)key_segment[k] + 1] += key_tend[k] - key_tbeg[k];
            cap += key_tend[k] - key_tbeg[k];
        }
    }
    AMX_REQUIRE(cap < (1ll << 30), AMX_ERR_UNSUPPORTED, "%s: %lld frames in reference keys are more than one call takes", who, cap);
    h->seg_sort_off.assign((size_t)n_seg, 0);
    long long sort_total = 0;
    for (int s = 0; s < n_seg; ++s) {
        long long pad = 1;
        while (pad < h->seg_off[(size_t)s + 1])
            pad <<= 1;
        if (pad > h->lds_cap)
            h->seg_sort_off[s] = sort_total, sort_total += pad;
        h->seg_off[(size_t)s + 1] += h->seg_off[s];
    }
    if (!h->tables_on_device) {
        AMX_TRY(h->d_label_token.upload(h->label_token.data(), h->label_token.size()));
        AMX_TRY(h->d_short_pause.upload(h->short_pause.data(), h->short_pause.size()));
        h->tables_on_device = true;
    }
    AMX_TRY(amx::acc_upload(ctx, h->d_key, h->keys));
    AMX_TRY(amx::acc_upload(ctx, h->d_group, h->groups));
    AMX_TRY(amx::acc_upload(ctx, h->d_ref, h->ref));
    AMX_TRY(amx::acc_upload(ctx, h->d_seg_off, h->seg_off));
    AMX_TRY(amx::acc_upload(ctx, h->d_seg_sort_off, h->seg_sort_off));
    const size_t slice = (size_t)std::max(cap, 1ll);
    AMX_TRY(h->d_seg_count.reserve((size_t)2 * n_seg));
    AMX_TRY(h->d_run_key.reserve(slice));
    AMX_TRY(h->d_run_tok.reserve(slice));
    AMX_TRY(h->d_tab.reserve(4 * slice));
    AMX_TRY(h->d_sort_key.reserve((size_t)std::max(sort_total, 1ll)));
    AMX_TRY(h->d_sort_tok.reserve((size_t)std::max(sort_total, 1ll)));
    AMX_TRY(h->d_counters.reserve(amx::kAccCounters));
    AMX_TRY(h->d_key_acc.reserve(n_keys));
    h->n_keys = -1;   // until this run has ended
    AMX_HIP(hipMemsetAsync(h->d_seg_count.get(), 0, (size_t)2 * n_seg * sizeof(int), ctx->stream));
    AMX_HIP(hipMemsetAsync(h->d_counters.get(), 0, amx::kAccCounters * sizeof(unsigned long long), ctx->stream));
    AMX_HIP(hipMemsetAsync(h->d_counters.get() + amx::kAccBad, 0xff, sizeof(unsigned long long), ctx->stream));
    amx::AccArgs a{};
    a.key = h->d_key.get(), a.n_keys = n_keys, a.group = h->d_group.get(), a.ref = h->d_ref.get(), a.n_ref = (int)h->ref.size();
    a.item = item_dev, a.label_token = h->has_table ? h->d_label_token.get() : nullptr, a.item_limit = h->has_table ? h->n_labels : h->n_tokens;
    a.short_pause = h->d_short_pause.get(), a.seg_off = h->d_seg_off.get(), a.seg_sort_off = h->d_seg_sort_off.get();
    a.seg_runs = h->d_seg_count.get(), a.seg_n = h->d_seg_count.get() + n_seg;
    a.run_key = h->d_run_key.get(), a.run_tok = h->d_run_tok.get(), a.sort_key = h->d_sort_key.get(), a.sort_tok = h->d_sort_tok.get();
    a.tab_start = h->d_tab.get(), a.tab_end = a.tab_start + slice, a.tab_tok = a.tab_end + slice, a.tab_maxend = a.tab_tok + slice;
    a.lds_cap = h->lds_cap, a.per_frame = h->mode == AMX_ACCURACY_FRAME_STATE, a.normalization = h->normalization;
    a.key_acc = h->d_key_acc.get(), a.counters = h->d_counters.get();
    const dim3         threads(amx::kAccThreads);
    unsigned long long counters[amx::kAccCounters];
    {
        amx::ScopedKernelTimer timer(ctx, "accuracy_check");
        hipLaunchKernelGGL(amx::accuracy_check_kernel, dim3((unsigned)amx::ceil_div(n_keys, amx::kAccWaves)), threads, 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipMemcpyAsync(counters, a.counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    if (counters[amx::kAccBad] != ~0ull) {
        const long slot = (long)(counters[amx::kAccBad] >> 32);
        const int  k    = (int)(std::upper_bound(slot_offsets, slot_offsets + n_keys + 1, slot) - slot_offsets) - 1;
        amx::set_error("%s: key %d, slot %ld: item %d is outside [0, %d) or the key mixes -1 with %s", who, k, slot - slot_offsets[k], (int)(unsigned)counters[amx::kAccBad],
                       a.item_limit, h->has_table ? "labels" : "emission indices");
        return AMX_ERR_INVALID;
    }
    if (!h->ref.empty()) {
        amx::ScopedKernelTimer timer(ctx, "accuracy_runs");
        hipLaunchKernelGGL(amx::accuracy_runs_kernel, dim3((unsigned)amx::ceil_div((long)h->ref.size(), amx::kAccWaves)), threads, 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    if (n_seg) {
        amx::ScopedKernelTimer timer(ctx, "accuracy_table");
        hipLaunchKernelGGL(amx::accuracy_table_kernel, dim3((unsigned)n_seg), threads, 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(ctx, "accuracy_key");
        const dim3 grid((unsigned)h->groups.size());
        const bool fma = ctx->contract == AMX_CONTRACT_FMA;
        if (h->mode == AMX_ACCURACY_APPROXIMATE_PHONE)
            hipLaunchKernelGGL((amx::accuracy_key_kernel<AMX_ACCURACY_APPROXIMATE_PHONE, false>), grid, threads, 0, ctx->stream, a);
        else if (h->mode == AMX_ACCURACY_FRAME_STATE)
            hipLaunchKernelGGL((amx::accuracy_key_kernel<AMX_ACCURACY_FRAME_STATE, false>), grid, threads, 0, ctx->stream, a);
        else if (fma)
            hipLaunchKernelGGL((amx::accuracy_key_kernel<AMX_ACCURACY_FRAME_PHONE, true>), grid, threads, 0, ctx->stream, a);
        else
            hipLaunchKernelGGL((amx::accuracy_key_kernel<AMX_ACCURACY_FRAME_PHONE, false>), grid, threads, 0, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipMemcpyAsync(key_accuracy_dev, a.key_acc, (size_t)n_keys * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(counters, a.counters, sizeof counters, hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    if (info)
        info->runs = counters[amx::kAccRuns], info->reference_intervals = counters[amx::kAccIntervals], info->keys_without_alignment = counters[amx::kAccNoAlignment];
    h->n_keys = n_keys, h->n_seg = n_seg;
    return AMX_OK;
}

int amx_accuracy_arc_dev(amx_accuracy* h, int n_arcs, const int32_t* arc_key, float* arc_accuracy_dev) {
    const char* who = "amx_accuracy_arc_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_arcs >= 0, AMX_ERR_INVALID, "%s: n_arcs %d", who, n_arcs);
    AMX_REQUIRE(h->n_keys >= 0, AMX_ERR_STATE, "%s: no amx_accuracy_run_dev has ended on this handle", who);
    if (n_arcs == 0)
        return AMX_OK;
    AMX_REQUIRE(arc_key, AMX_ERR_INVALID, "%s: NULL arc_key", who);
    for (int a = 0; a < n_arcs; ++a)
        AMX_REQUIRE(arc_key[a] >= -1 && arc_key[a] < h->n_keys, AMX_ERR_INVALID, "%s: arc %d: key %d outside the %d keys of the last run", who, a, arc_key[a],
                    h->n_keys);
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(arc_accuracy_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    h->arc_key.assign(arc_key, arc_key + n_arcs);   // the upload reads it until the synchronisation below
    AMX_TRY(amx::acc_upload(ctx, h->d_arc_key, h->arc_key));
    {
        amx::ScopedKernelTimer timer(ctx, "accuracy_gather");
        hipLaunchKernelGGL(amx::accuracy_gather_kernel, dim3((unsigned)amx::ceil_div(n_arcs, 256)), dim3(256), 0, ctx->stream, h->d_key_acc.get(), h->d_arc_key.get(),
                           n_arcs, arc_accuracy_dev);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    return AMX_OK;
}

int amx_accuracy_last_reference(amx_accuracy* h, int segment, int capacity, int32_t* token, int32_t* start, int32_t* end) {
    const char* who = "amx_accuracy_last_reference";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(h->n_keys >= 0 && h->ctx, AMX_ERR_STATE, "%s: no amx_accuracy_run_dev has ended on this handle", who);
    AMX_REQUIRE(segment >= 0 && segment < h->n_seg && capacity >= 0, AMX_ERR_INVALID, "%s: segment %d outside the %d segments of the last run, or capacity %d", who,
                segment, h->n_seg, capacity);
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    int n = 0;
    AMX_HIP(hipMemcpyAsync(&n, h->d_seg_count.get() + h->n_seg + segment, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    if (token && start && end && n) {
        AMX_REQUIRE(capacity >= n, AMX_ERR_INVALID, "%s: segment %d has %d intervals, the tables hold %d", who, segment, n, capacity);
        const size_t slice = (size_t)std::max(h->seg_off[h->n_seg], 1);
        const int*   tab   = h->d_tab.get() + h->seg_off[segment];
        AMX_HIP(hipMemcpyAsync(start, tab, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipMemcpyAsync(end, tab + slice, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipMemcpyAsync(token, tab + 2 * slice, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        AMX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return n;
}

}  // extern "C"
