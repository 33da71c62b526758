// nnseq.hip -- sequence-discriminative NN training from lattices: Nn::SegmentwiseNnTrainer (criteria MMI and ME) in full-batch mode on
// the handle of nntrain.hip.  include/amx.h ("NN sequence-discriminative training") states the arithmetic with the reference's
// file:line; this file holds the handle, the kernels between the forward pass and the backpropagation, and the host side of a call.
//
// A batch of segments shares the nntrain handle's workspace: segment s owns the rows [row0[s], row0[s] + len[s]), row0 a multiple of
// AMX_NNTRAIN_CHUNK, so that a chunk of the X E^T partial sums never holds frames of two segments.  Rows between two segments: zero
// layer inputs, zero error signal, label -1, weight 0.
// Kernels and their bounds ("NN sequence-discriminative training"):
//   scores    nnseq_score_kernel: one wave per arc, 64 gathered outputs at a time, ONE f32 chain in item order; latency bound gathers
//   collect   nnseq_resolve_kernel (item -> key (row, output), f32 weight), a stable 8-bit radix sort of the keys (the algorithm of
//             ebw.hip: count, scan, place), nnseq_collect_kernel: one f64 chain per key over its run, one write of E per key
//   reject    nnseq_reject_kernel: one cell per frame
//   smooth    nnseq_smooth_kernel: one workgroup per frame, one read and one write of E's row: scale, fmaf, delta, weight; argMax and
//             the CE term of the row ride along; HBM bound
//   sums      nnseq_reduce_kernel: per element and segment the chunk partials in ascending order in f32, widened, added in segment
//             order; nnseq_tail_kernel: ONE workgroup, nntrain_tail_kernel's order per segment
// Forward, softmax, E W and X E^T are nntrain.hip's launches (nntrain.hpp).
#include "nntrain.hpp"
#include "nnseq_plan.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

static_assert(sizeof(long) == sizeof(long long), "the host tables are uploaded as they are");

namespace amx {

__device__ __forceinline__ void seq_bad(unsigned long long* bad, int stage, long long index, int kind) {
    atomicMin(bad, ((unsigned long long)stage << 48) | ((unsigned long long)index << 3) | (unsigned long long)kind);
}

__device__ __forceinline__ long long seq_upper(const long long* __restrict__ off, long long n, long long v) {
    long long lo = 0, hi = n;  // first index with off[index] > v
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (off[mid] > v)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// ---- the network input: row r of the workspace is frame row_src[r] of the features, or zero (row_src < 0)
__global__ __launch_bounds__(kSeqThreads) void nnseq_pack_kernel(FeatSrc f, const long long* __restrict__ row_src, int rows, int K, float* __restrict__ out,
                                                               int Kpad) {
    const long long n = (long long)rows * Kpad;
    for (long long i = (long long)blockIdx.x * kSeqThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kSeqThreads) {
        const int       r = (int)(i / Kpad), k = (int)(i - (long long)r * Kpad);
        const long long s = row_src[r];
        out[i]            = (s >= 0 && k < K) ? f((int)s, k) : 0.f;
    }
}

// the rows between two segments of a hidden layer's input (the forward GEMM left f(bias) there)
__global__ __launch_bounds__(kSeqThreads) void nnseq_zero_rows_kernel(float* __restrict__ x, int ld, const long long* __restrict__ row_src, int rows) {
    const long long n = (long long)rows * ld;
    for (long long i = (long long)blockIdx.x * kSeqThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kSeqThreads)
        if (row_src[i / ld] < 0)
            x[i] = 0.f;
}

// ---- arc scores: one wave per arc; score -= out[o, t] in item order (top holds -out: a - b and a + (-b) are the same f32)
__global__ __launch_bounds__(kSeqThreads) void nnseq_score_kernel(long long n_arcs, int n_seg, const long long* __restrict__ arc_off,
                                                                const long long* __restrict__ item_off, const int32_t* __restrict__ item_frame,
                                                                const int32_t* __restrict__ item_emission, const int* __restrict__ seg_row0,
                                                                const int* __restrict__ seg_len, const int* __restrict__ c2o, int n_classes, int n_out,
                                                                const float* __restrict__ top, float* __restrict__ score_out, unsigned long long* bad) {
    const int       lane = threadIdx.x & 63;
    const long long arc  = (long long)blockIdx.x * kSeqArcs + (threadIdx.x >> 6);
    if (arc >= n_arcs)  // uniform over the wave
        return;
    const int       seg = (int)(seq_upper(arc_off, (long long)n_seg + 1, arc) - 1);
    const long long b = item_off[arc], e = item_off[arc + 1];
    const int       row0 = seg_row0[seg], len = seg_len[seg];
    float           score = 0.f;  // the semiring's one
    for (long long base = b; base < e; base += kSeqStage) {
        const long long i = base + lane;
        float           v = 0.f;
        if (i < e) {
            const int f = item_frame[i], em = item_emission[i];
            if (f < 0 || f >= len)
                seq_bad(bad, 0, i, SEQ_BAD_FRAME);
            else if (em < 0 || em >= n_classes)
                seq_bad(bad, 0, i, SEQ_BAD_EMISSION);
            else {
                const int o = c2o ? c2o[em] : em;
                if (o < 0 || o >= n_out)
                    seq_bad(bad, 0, i, SEQ_BAD_EMISSION);
                else
                    v = top[(size_t)(row0 + f) * n_out + o];
            }
        }
        const int cnt = (int)min((long long)kSeqStage, e - base);
        for (int j = 0; j < cnt; ++j)
            score = score + __shfl(v, j, 64);
    }
    if (lane == 0)
        score_out[arc] = score;
}

// ---- a frame of the best path that holds 0xffffffff marks its segment (state |= 2): "alignment vector failed"; runs before the labels
// are checked, so that nothing of such a segment is
__global__ __launch_bounds__(kSeqThreads) void nnseq_alignment_kernel(int rows, const long long* __restrict__ row_src, const int* __restrict__ row_seg, long long f0,
                                                                    const uint32_t* __restrict__ emission, int* __restrict__ seg_state) {
    const int r = blockIdx.x * kSeqThreads + threadIdx.x;
    if (r >= rows)
        return;
    const long long s = row_src[r];
    if (s >= 0 && !(seg_state[row_seg[r]] & AMX_NNSEQ_SEG_SKIPPED) && emission[s - f0] == 0xffffffffu)
        atomicOr(&seg_state[row_seg[r]], AMX_NNSEQ_SEG_NO_ALIGNMENT);
}

// ---- alignment: label[r] = class_to_output[emission], w[r] = class_weights[label]
__global__ __launch_bounds__(kSeqThreads) void nnseq_label_kernel(int rows, const long long* __restrict__ row_src, const int* __restrict__ row_seg, long long f0,
                                                                const uint32_t* __restrict__ emission, const int* __restrict__ c2o,
                                                                const float* __restrict__ class_weight, int n_classes, int n_out, const int* __restrict__ seg_state,
                                                                int* __restrict__ label, float* __restrict__ w, unsigned long long* bad) {
    const int r = blockIdx.x * kSeqThreads + threadIdx.x;
    if (r >= rows)
        return;
    int             o  = -1;
    float           wt = 0.f;
    const long long s  = row_src[r];
    if (s >= 0 && seg_state[row_seg[r]] == 0) {  // a skipped segment and one without an alignment are not checked
        const uint32_t e = emission[s - f0];
        if (e >= (uint32_t)n_classes)
            seq_bad(bad, 0, s - f0, SEQ_BAD_LABEL);
        else {
            const int m = c2o ? c2o[e] : (int)e;
            if (m < 0 || m >= n_out)
                seq_bad(bad, 0, s - f0, SEQ_BAD_LABEL);
            else {
                o  = m;
                wt = class_weight[m];
            }
        }
    }
    label[r] = o;
    w[r]     = wt;
}

// ---- items of one pass -> (code, val): code = row << out_bits | output, val = the f32 arc weight; what does not count gets the sentinel
__global__ __launch_bounds__(kSeqThreads) void nnseq_resolve_kernel(int stage, long long n_items, long long n_arcs, int n_seg, const long long* __restrict__ arc_off,
                                                                  const float* __restrict__ arc_w, const long long* __restrict__ item_off,
                                                                  const int32_t* __restrict__ item_frame, const int32_t* __restrict__ item_emission,
                                                                  const int* __restrict__ seg_row0, const int* __restrict__ seg_len,
                                                                  const int* __restrict__ seg_state, const int* __restrict__ c2o, int n_classes, int n_out,
                                                                  int negate, double threshold, int out_bits, unsigned long long sentinel,
                                                                  unsigned long long* __restrict__ code, uint32_t* __restrict__ val, unsigned long long* bad) {
    const long long i = (long long)blockIdx.x * kSeqThreads + threadIdx.x;
    if (i < n_arcs) {
        const int seg = (int)(seq_upper(arc_off, (long long)n_seg + 1, i) - 1);
        if (seg_state[seg] == 0 && !isfinite(arc_w[i]))
            seq_bad(bad, stage, i, SEQ_BAD_WEIGHT);
    }
    if (i >= n_items)
        return;
    const long long    arc = seq_upper(item_off, n_arcs + 1, i) - 1;
    const int          seg = (int)(seq_upper(arc_off, (long long)n_seg + 1, arc) - 1);
    unsigned long long c   = sentinel;
    uint32_t           v   = 0;
    if (seg_state[seg] == 0) {
        float w = arc_w[arc];
        if (negate)
            w = w * -1.f;  // Fsa::multiply(fsa, Weight(-1.0)): an f32 product
        const int f = item_frame[i], e = item_emission[i];
        if (f < 0 || f >= seg_len[seg])
            seq_bad(bad, stage, i, SEQ_BAD_FRAME);
        else if (e < 0 || e >= n_classes)
            seq_bad(bad, stage, i, SEQ_BAD_EMISSION);
        else {
            const int o = c2o ? c2o[e] : e;
            if (o < 0 || o >= n_out)
                seq_bad(bad, stage, i, SEQ_BAD_EMISSION);
            else if (isfinite(w) && (double)w > threshold) {  // f32 weight = f32(a->weight()); weight > weightThreshold_ (an f64), strict
                c = ((unsigned long long)(seg_row0[seg] + f) << out_bits) | (unsigned long long)o;
                v = __float_as_uint(w);
            }
        }
    }
    code[i] = c;
    val[i]  = v;
}

// ---- exclusive scan of 32-bit integers in place: a workgroup scans kSeqBlock of them and leaves its total in sums[block]
__global__ __launch_bounds__(kSeqThreads) void nnseq_scan_block_kernel(int* __restrict__ data, long long n, int* __restrict__ sums) {
    __shared__ int  s[kSeqThreads];
    const int       tid  = threadIdx.x;
    const long long base = (long long)blockIdx.x * kSeqBlock + (long long)tid * 8;
    int             v[8], total = 0;
    for (int j = 0; j < 8; ++j) {
        v[j] = base + j < n ? data[base + j] : 0;
        total += v[j];
    }
    s[tid] = total;
    __syncthreads();
    for (int o = 1; o < kSeqThreads; o <<= 1) {
        const int add = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    int run = s[tid] - total;
    for (int j = 0; j < 8; ++j) {
        if (base + j < n)
            data[base + j] = run;
        run += v[j];
    }
    if (tid == kSeqThreads - 1)
        sums[blockIdx.x] = s[tid];
}

__global__ __launch_bounds__(kSeqThreads) void nnseq_scan_add_kernel(int* __restrict__ data, long long n, const int* __restrict__ sums) {
    const long long i = (long long)blockIdx.x * kSeqThreads + threadIdx.x;
    if (i < n)
        data[i] += sums[i / kSeqBlock];
}

// ---- one pass of the stable sort over the 8 bits at `shift`.  table[digit * n_blocks + block]: counts, then (scanned) places
__global__ __launch_bounds__(kSeqThreads) void nnseq_sort_count_kernel(const unsigned long long* __restrict__ code, long long n, int shift, int n_blocks,
                                                                     int* __restrict__ table) {
    __shared__ int s_cnt[256];
    const int      tid = threadIdx.x;
    s_cnt[tid]         = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kSeqBlock;
    for (int c = 0; c < kSeqBlock; c += kSeqThreads) {
        const long long i = base + c + tid;
        if (i < n)
            atomicAdd(&s_cnt[(int)((code[i] >> shift) & 255)], 1);  // an integer count: the sum does not depend on the order
    }
    __syncthreads();
    table[(long long)tid * n_blocks + blockIdx.x] = s_cnt[tid];
}

__global__ __launch_bounds__(kSeqThreads) void nnseq_sort_place_kernel(const unsigned long long* __restrict__ code, const uint32_t* __restrict__ val, long long n,
                                                                     int shift, int n_blocks, const int* __restrict__ table,
                                                                     unsigned long long* __restrict__ code_out, uint32_t* __restrict__ val_out) {
    __shared__ int s_place[256];
    __shared__ int s_digit[kSeqThreads];
    const int      tid = threadIdx.x;
    s_place[tid]       = table[(long long)tid * n_blocks + blockIdx.x];
    __syncthreads();
    const long long base = (long long)blockIdx.x * kSeqBlock;
    for (int c = 0; c < kSeqBlock; c += kSeqThreads) {  // all lanes run every chunk
        const long long          i  = base + c + tid;
        const bool               in = i < n;
        const unsigned long long k  = in ? code[i] : 0ull;
        const int                d  = in ? (int)((k >> shift) & 255) : -1;
        s_digit[tid]                = d;
        __syncthreads();
        if (in) {
            int rank = 0;
            for (int j = 0; j < tid; ++j)
                rank += s_digit[j] == d;
            const int pos = s_place[d] + rank;  // < n: the places of a digit's blocks partition [0, n)
            code_out[pos] = k;
            val_out[pos]  = val[i];
        }
        __syncthreads();
        if (in)
            atomicAdd(&s_place[d], 1);
        __syncthreads();
    }
}

// ---- one chain per key: Collector::collect starts at the first weight's 0 + w and adds in the order the arcs were walked; then
// ErrorSignalAccumulator::accumulate: E (f32) += factor * collected (f64), narrowed once.  One write per key.
__global__ __launch_bounds__(kSeqThreads) void nnseq_collect_kernel(const unsigned long long* __restrict__ code, const uint32_t* __restrict__ val, long long n,
                                                                  unsigned long long sentinel, int out_bits, double factor, float* __restrict__ E, int ldE) {
    const long long i = (long long)blockIdx.x * kSeqThreads + threadIdx.x;
    if (i >= n)
        return;
    const unsigned long long c = code[i];
    if (c >= sentinel || (i > 0 && code[i - 1] == c))
        return;
    double sum = 0.0;
    for (long long q = i; q < n && code[q] == c; ++q)
        sum += (double)__uint_as_float(val[q]);
    float* cell = E + (size_t)(c >> out_bits) * ldE + (size_t)(c & ((1ull << out_bits) - 1ull));
    *cell       = (float)((double)*cell + factor * sum);
}

// ---- frame rejection: w[t] = 0 where E[alignment[t], t] < threshold; verify_ge(cell, 0) becomes a refusal
__global__ __launch_bounds__(kSeqThreads) void nnseq_reject_kernel(int stage, int rows, const int* __restrict__ row_seg, const int* __restrict__ seg_state,
                                                                 const int* __restrict__ label, const float* __restrict__ E, int ldE, float threshold,
                                                                 float* __restrict__ w, unsigned* __restrict__ seg_rejected, unsigned long long* bad) {
    const int r = blockIdx.x * kSeqThreads + threadIdx.x;
    if (r >= rows)
        return;
    const int o = label[r];
    if (o < 0 || seg_state[row_seg[r]] != 0)
        return;
    const float c = E[(size_t)r * ldE + o];
    if (!(c >= 0.f))
        seq_bad(bad, stage, r, SEQ_BAD_CELL);
    else if (c < threshold) {
        w[r] = 0.f;
        atomicAdd(&seg_rejected[row_seg[r]], 1u);
    }
}

// top (scores = -output) += prior_scale * log_prior on the output: addToAllColumns = axpy, one fused multiply-add per element
__global__ __launch_bounds__(kSeqThreads) void nnseq_prior_kernel(float* __restrict__ top, long long total, int n, const float* __restrict__ prior, float scale) {
    for (long long i = (long long)blockIdx.x * kSeqThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kSeqThreads)
        top[i] = fmaf(-scale, prior[i % n], top[i]);  // -(fma(s, p, a)) == fma(-s, p, -a)
}

// ---- one workgroup per frame over the top row: the smoothing's three steps and the weight on E, argMax and the CE term
// softmaxed: row holds p; otherwise the negated linear output.  E nullable (no gradient).
__global__ __launch_bounds__(kSeqThreads) void nnseq_smooth_kernel(const float* __restrict__ top, int n, int softmaxed, float lambda, float keep,
                                                                 const int* __restrict__ row_seg, const int* __restrict__ seg_state,
                                                                 const int* __restrict__ label, const float* __restrict__ w, float* __restrict__ E, int ldE,
                                                                 unsigned* __restrict__ err, float* __restrict__ term) {
    __shared__ float    s_val[4];
    __shared__ unsigned s_idx[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int o = label[r];
    if (o < 0 || seg_state[row_seg[r]] != 0) {  // uniform over the workgroup; E's row is zero and stays so
        if (tid == 0) {
            err[r]  = 0;
            term[r] = 0.f;
        }
        return;
    }
    const float* row = top + (size_t)r * n;
    float*       e   = E ? E + (size_t)r * ldE : nullptr;
    const float  wt  = w[r];
    float        best = -FLT_MAX;
    unsigned     bi   = 0xffffffffu;
    for (int i = tid; i < n; i += kSeqThreads) {
        const float x = row[i], v = softmaxed ? x : -x;
        if (v > best) {
            best = v;
            bi   = (unsigned)i;
        }
        if (e) {
            float d = e[i];
            if (softmaxed) {
                d = d * keep;           // scale((f32)(1.0 - lambda))
                d = fmaf(lambda, x, d);  // add(p, lambda): axpy
                if (i == o)
                    d = d + -lambda;     // addKroneckerDelta(alignment, -lambda)
            }
            d    = d * wt;  // multiplyColumnsByScalars(weights)
            e[i] = d;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float    ob = __shfl_xor(best, off, 64);
        const unsigned oi = (unsigned)__shfl_xor((int)bi, off, 64);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi   = oi;
        }
    }
    if ((tid & 63) == 0) {
        s_val[tid >> 6] = best;
        s_idx[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k)
            if (s_val[k] > best || (s_val[k] == best && s_idx[k] < bi)) {
                best = s_val[k];
                bi   = s_idx[k];
            }
        const unsigned arg = bi == 0xffffffffu ? 0u : bi;
        err[r]             = arg != (unsigned)o ? 1u : 0u;
        term[r]            = softmaxed ? logf(row[o]) * wt : 0.f;
    }
}

// ---- acc[r * cols + c] += per segment, in segment order: (f64)(((0 + part[c0]) + part[c0 + 1]) + ...), the segment's chunks in f32
__global__ __launch_bounds__(kSeqThreads) void nnseq_reduce_kernel(const float* __restrict__ part, size_t chunk_stride, int rows, int cols, int ld, int n_seg,
                                                                 const int* __restrict__ seg_row0, const int* __restrict__ seg_len,
                                                                 const int* __restrict__ seg_state, double* __restrict__ acc) {
    const long long total = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * kSeqThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kSeqThreads) {
        const int r = (int)(i / cols), c = (int)(i - (long long)r * cols);
        double    a = acc[i];
        for (int g = 0; g < n_seg; ++g) {
            if (seg_state[g] != 0 || seg_len[g] == 0)
                continue;
            const int q0 = seg_row0[g] / AMX_NNTRAIN_CHUNK, q1 = q0 + (seg_len[g] + AMX_NNTRAIN_CHUNK - 1) / AMX_NNTRAIN_CHUNK;
            float     s  = 0.f;
            for (int q = q0; q < q1; ++q)
                s = s + part[(size_t)q * chunk_stride + (size_t)r * ld + c];
            a += (double)s;
        }
        acc[i] = a;
    }
}

// ---- the tail, ONE workgroup: per segment nntrain_tail_kernel's sums in its order, then objective[s]; the CE objective of a
// segment is the reference's sequential f32 chain
__global__ __launch_bounds__(256) void nnseq_tail_kernel(int n_seg, const int* __restrict__ seg_row0, const int* __restrict__ seg_len,
                                                       const int* __restrict__ seg_state, const int* __restrict__ label, const float* __restrict__ w,
                                                       const unsigned* __restrict__ err, const float* __restrict__ term, const float* __restrict__ objective,
                                                       unsigned* __restrict__ seg_err, float* __restrict__ seg_ce, double* __restrict__ tail) {
    __shared__ double s_red[3][256];
    const int tid = threadIdx.x;
    for (int g = 0; g < n_seg; ++g) {  // uniform
        if (tid == 0) {
            seg_err[g] = 0;
            seg_ce[g]  = 0.f;
        }
        if (seg_state[g] != 0 || seg_len[g] == 0)
            continue;
        const int base = seg_row0[g], T = seg_len[g];
        double    n_obs = 0.0, n_err = 0.0, sum_w = 0.0;
        for (int t = tid; t < T; t += 256)
            if (label[base + t] >= 0) {
                n_obs += 1.0;
                sum_w += (double)fabsf(w[base + t]);
                n_err += (double)err[base + t];
            }
        s_red[0][tid] = n_obs;
        s_red[1][tid] = n_err;
        s_red[2][tid] = sum_w;
        __syncthreads();
        for (int half = 128; half > 0; half >>= 1) {
            if (tid < half)
                for (int q = 0; q < 3; ++q)
                    s_red[q][tid] += s_red[q][tid + half];
            __syncthreads();
        }
        if (tid == 0) {
            tail[0] += s_red[0][0];
            tail[2] += s_red[2][0];
            tail[1] += s_red[1][0];
            tail[3] += (double)objective[g];
            float ce = 0.f;
            for (int t = 0; t < T; ++t)
                ce = ce - term[base + t];
            seg_err[g] = (unsigned)s_red[1][0];
            seg_ce[g]  = ce;
        }
        __syncthreads();
    }
}

}  // namespace amx

struct amx_nnseq {
    amx_nntrain*       t = nullptr;
    amx_nnseq_cfg      cfg{};
    std::vector<float> prior;
    amx::DevBuf<float> d_prior;
    // the last forward
    bool              forwarded = false, top_softmax = false, accumulated = false;
    int               n_seg = 0, rows = 0;
    unsigned long     epoch = 0;  // the nntrain handle's workspace_epoch after the last forward
    long long         f0 = 0;
    std::vector<int>  row0, len;
    amx::DevBuf<long long> d_row_src;
    amx::DevBuf<int>       d_row_seg, d_seg_row0, d_seg_len, d_seg_state;
    amx::DevBuf<unsigned>  d_seg_err, d_seg_rej;
    amx::DevBuf<float>     d_seg_ce, d_term, d_objective, d_E_lattice;
    amx::DevBuf<unsigned long long>       d_bad;
    amx::DevBuf<unsigned long long, true> h_bad;
    // the tables of a pass and the sort
    amx::DevBuf<long long>          d_arc_off, d_item_off;
    amx::DevBuf<int32_t>            d_item_frame, d_item_emission;
    amx::DevBuf<unsigned long long> d_code[2];
    amx::DevBuf<uint32_t>           d_val[2];
    amx::DevBuf<int>                d_table, d_scan_ws;
    int last_passes = 0, last_blocks = 0;
};

namespace {

int seq_scan(hipStream_t st, int* data, long long n, int* ws) {
    const long long nb = (n + amx::kSeqBlock - 1) / amx::kSeqBlock;
    hipLaunchKernelGGL(amx::nnseq_scan_block_kernel, dim3((unsigned)nb), dim3(amx::kSeqThreads), 0, st, data, n, ws);
    AMX_HIP(hipGetLastError());
    if (nb > 1) {
        AMX_TRY(seq_scan(st, ws, nb, ws + nb));
        hipLaunchKernelGGL(amx::nnseq_scan_add_kernel, dim3((unsigned)((n + amx::kSeqThreads - 1) / amx::kSeqThreads)), dim3(amx::kSeqThreads), 0, st, data, n,
                           (const int*)ws);
        AMX_HIP(hipGetLastError());
    }
    return AMX_OK;
}

// stable sort of (code, val) by the low `bits` bits of code; *side: which of the two buffers holds the result
int seq_sort(amx_nnseq* h, hipStream_t st, long long n, int bits, int* side) {
    const int nb = (int)((n + amx::kSeqBlock - 1) / amx::kSeqBlock);
    AMX_TRY(h->d_table.reserve((size_t)256 * nb));
    AMX_TRY(h->d_scan_ws.reserve(amx::nnseq_scan_ws(256ll * nb)));
    int cur        = 0;
    h->last_passes = 0, h->last_blocks = nb;
    for (int shift = 0; shift < bits; shift += 8, cur ^= 1) {
        hipLaunchKernelGGL(amx::nnseq_sort_count_kernel, dim3((unsigned)nb), dim3(amx::kSeqThreads), 0, st, (const unsigned long long*)h->d_code[cur].get(), n,
                           shift, nb, h->d_table.get());
        AMX_HIP(hipGetLastError());
        AMX_TRY(seq_scan(st, h->d_table.get(), 256ll * nb, h->d_scan_ws.get()));
        hipLaunchKernelGGL(amx::nnseq_sort_place_kernel, dim3((unsigned)nb), dim3(amx::kSeqThreads), 0, st, (const unsigned long long*)h->d_code[cur].get(),
                           (const uint32_t*)h->d_val[cur].get(), n, shift, nb, (const int*)h->d_table.get(), h->d_code[cur ^ 1].get(), h->d_val[cur ^ 1].get());
        AMX_HIP(hipGetLastError());
        ++h->last_passes;
    }
    *side = cur;
    return AMX_OK;
}

int upload_tables(amx_nnseq* h, hipStream_t st, int n_seg, const long* arc_off, const long* item_off, const int32_t* item_frame, const int32_t* item_emission,
                  long long n_arcs, long long n_items) {
    AMX_HIP(hipStreamSynchronize(st));  // a table that grows is freed first: nothing in flight may still read it
    AMX_TRY(h->d_arc_off.reserve((size_t)n_seg + 1));
    AMX_TRY(h->d_item_off.reserve((size_t)n_arcs + 1));
    AMX_TRY(h->d_item_frame.reserve((size_t)std::max<long long>(n_items, 1)));
    AMX_TRY(h->d_item_emission.reserve((size_t)std::max<long long>(n_items, 1)));
    AMX_HIP(hipMemcpyAsync(h->d_arc_off.get(), arc_off, sizeof(long long) * ((size_t)n_seg + 1), hipMemcpyHostToDevice, st));
    AMX_HIP(hipMemcpyAsync(h->d_item_off.get(), item_off, sizeof(long long) * ((size_t)n_arcs + 1), hipMemcpyHostToDevice, st));
    if (n_items) {
        AMX_HIP(hipMemcpyAsync(h->d_item_frame.get(), item_frame, sizeof(int32_t) * (size_t)n_items, hipMemcpyHostToDevice, st));
        AMX_HIP(hipMemcpyAsync(h->d_item_emission.get(), item_emission, sizeof(int32_t) * (size_t)n_items, hipMemcpyHostToDevice, st));
    }
    AMX_HIP(hipStreamSynchronize(st));  // the caller's tables are not read after this returns, whatever ends the call
    return AMX_OK;
}

int fetch_bad(amx_nnseq* h, hipStream_t st, unsigned long long* out) {
    AMX_HIP(hipMemcpyAsync(h->h_bad.get(), h->d_bad.get(), 8, hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    *out = *h->h_bad.get();
    return AMX_OK;
}

int blocks_for(long long n) {
    return (int)std::min<long long>(16384, std::max<long long>(1, (n + amx::kSeqThreads - 1) / amx::kSeqThreads));
}

}  // namespace

extern "C" {

void amx_nnseq_default_cfg(amx_nnseq_cfg* cfg) {
    if (!cfg)
        return;
    memset(cfg, 0, sizeof *cfg);
    cfg->weight_threshold = (double)1.1920928955078125e-07f;  // Core::Type<f32>::epsilon
    cfg->full_batch       = 1;
}

void amx_nnseq_kernel_shape(int* sort_block_items, int* score_block_arcs, int* score_stage_items, int* threads) {
    if (sort_block_items)
        *sort_block_items = amx::kSeqBlock;
    if (score_block_arcs)
        *score_block_arcs = amx::kSeqArcs;
    if (score_stage_items)
        *score_stage_items = amx::kSeqStage;
    if (threads)
        *threads = amx::kSeqThreads;
}

void amx_nnseq_destroy(amx_nnseq* h) {
    delete h;
}

int amx_nnseq_create(amx_nntrain* train, const amx_nnseq_cfg* cfg, amx_nnseq** out) {
    AMX_REQUIRE(train && out, AMX_ERR_INVALID, "amx_nnseq_create: NULL argument");
    *out = nullptr;
    amx_nnseq_cfg c;
    amx_nnseq_default_cfg(&c);
    if (cfg)
        c = *cfg;
    AMX_REQUIRE(train->mask & AMX_NNSTAT_BASE, AMX_ERR_INVALID, "amx_nnseq_create: the nntrain handle's statistics need the base statistics (the segment-wise trainer always has them)");
    AMX_REQUIRE(!(train->mask & (AMX_NNSTAT_MEAN_AND_VARIANCE | AMX_NNSTAT_CLASS_COUNTS)), AMX_ERR_INVALID,
                "amx_nnseq_create: the nntrain handle's statistics may be the base statistics and the gradient only (mask %d)", train->mask);
    AMX_REQUIRE(train->L >= 1, AMX_ERR_INVALID, "amx_nnseq_create: the nntrain handle has no network");
    AMX_REQUIRE(c.full_batch != 0, AMX_ERR_UNSUPPORTED, "amx_nnseq_create: full_batch = 0: the stochastic per-segment update is not implemented");
    AMX_REQUIRE(c.accumulate_prior == 0, AMX_ERR_UNSUPPORTED,
                "amx_nnseq_create: accumulate_prior: count the classes of emission_dev with the class-counts statistics of amx_nntrain_accumulate_dev instead");
    AMX_REQUIRE(c.label_type == 0, AMX_ERR_UNSUPPORTED, "amx_nnseq_create: label_type = %d: allophone-state labels are not implemented, map them to emission indices", c.label_type);
    AMX_REQUIRE(c.weight_threshold == c.weight_threshold, AMX_ERR_INVALID, "amx_nnseq_create: weight_threshold is not a number");
    AMX_REQUIRE(c.ce_smoothing_weight >= 0.f && c.ce_smoothing_weight <= 1.f, AMX_ERR_INVALID, "amx_nnseq_create: ce_smoothing_weight = %g (0..1)", (double)c.ce_smoothing_weight);
    AMX_REQUIRE(c.frame_rejection_threshold >= 0.f && c.frame_rejection_threshold <= 1.f, AMX_ERR_INVALID, "amx_nnseq_create: frame_rejection_threshold = %g (0..1)",
                (double)c.frame_rejection_threshold);
    AMX_REQUIRE(std::isfinite(c.prior_scale), AMX_ERR_INVALID, "amx_nnseq_create: prior_scale is not finite");
    AMX_REQUIRE(!(c.prior_scale > 0.f && c.ce_smoothing_weight > 0.f && !c.log_prior), AMX_ERR_INVALID, "amx_nnseq_create: prior_scale > 0 without log_prior");
    std::unique_ptr<amx_nnseq> h(new amx_nnseq);
    h->t   = train;
    h->cfg = c;
    if (c.log_prior)
        h->prior.assign(c.log_prior, c.log_prior + train->n_outputs);
    h->cfg.log_prior = nullptr;
    if (train->ctx) {
        AMX_HIP(hipSetDevice(train->ctx->device));
        if (!h->prior.empty())
            AMX_TRY(h->d_prior.upload(h->prior.data(), h->prior.size()));
        AMX_TRY(h->d_bad.reserve(1));
        AMX_TRY(h->h_bad.reserve(1));
    }
    *out = h.release();
    return AMX_OK;
}

int amx_nnseq_forward_dev(amx_nnseq* h, const float* feats, int ldf, int n_seg, const long* frame_offsets) {
    const char* who = "amx_nnseq_forward_dev";
    AMX_REQUIRE(h && frame_offsets, AMX_ERR_INVALID, "%s: NULL argument", who);
    amx_nntrain* t = h->t;
    amx::SeqPlan plan;
    AMX_TRY(amx::nnseq_plan_rows(who, n_seg, frame_offsets, &plan));
    AMX_REQUIRE(t->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(feats && ldf >= t->feature_dim, AMX_ERR_INVALID, "%s: feats_dev is NULL or feats_stride %d < %d", who, ldf, t->feature_dim);
    h->forwarded = false;
    h->n_seg = n_seg, h->rows = plan.rows, h->f0 = plan.f0;
    h->row0 = plan.row0, h->len = plan.len;
    const long long               rows    = plan.rows;
    const std::vector<long long>& row_src = plan.row_src;
    const std::vector<int>&       row_seg = plan.row_seg;
    if (rows == 0) {
        h->forwarded = true, h->top_softmax = false, h->accumulated = false;
        h->epoch = ++t->workspace_epoch;
        return AMX_OK;
    }
    hipStream_t st = t->ctx->stream;
    AMX_HIP(hipSetDevice(t->ctx->device));
    AMX_HIP(hipStreamSynchronize(st));  // workspaces that grow are freed first
    const int  R = (int)rows, L = t->L, n_out = t->n_outputs, n_chunks = R / AMX_NNTRAIN_CHUNK;
    (void)n_chunks;
    const bool grad = (t->mask & AMX_NNSTAT_GRADIENT) != 0;
    AMX_TRY(t->d_label.reserve(R));
    AMX_TRY(t->d_w.reserve(R));
    AMX_TRY(t->d_err.reserve(R));
    AMX_TRY(t->d_obj.reserve(R));
    AMX_TRY(h->d_term.reserve(R));
    AMX_TRY(t->d_top.reserve((size_t)R * n_out));
    AMX_TRY(t->d_rowstat.reserve((size_t)2 * R));
    for (int l = 0; l < L; ++l) {
        AMX_TRY(t->d_x[l].reserve((size_t)R * t->Pin[l]));
        if (grad)
            AMX_TRY(t->d_E[l].reserve((size_t)R * t->Pout[l]));
    }
    const size_t part = grad ? amx::nnseq_part_size(R, L, t->Pin.data(), t->Pout.data()) : 1;
    AMX_TRY(t->d_part.reserve(part));
    AMX_TRY(h->d_row_src.reserve(R));
    AMX_TRY(h->d_row_seg.reserve(R));
    AMX_TRY(h->d_seg_row0.reserve((size_t)n_seg + 1));
    AMX_TRY(h->d_seg_len.reserve(n_seg));
    AMX_TRY(h->d_seg_state.reserve(n_seg));
    AMX_TRY(h->d_seg_err.reserve(n_seg));
    AMX_TRY(h->d_seg_rej.reserve(n_seg));
    AMX_TRY(h->d_seg_ce.reserve(n_seg));
    AMX_TRY(h->d_objective.reserve(n_seg));
    AMX_HIP(hipMemcpy(h->d_row_src.get(), row_src.data(), sizeof(long long) * R, hipMemcpyHostToDevice));
    AMX_HIP(hipMemcpy(h->d_row_seg.get(), row_seg.data(), sizeof(int) * R, hipMemcpyHostToDevice));
    AMX_HIP(hipMemcpy(h->d_seg_row0.get(), h->row0.data(), sizeof(int) * ((size_t)n_seg + 1), hipMemcpyHostToDevice));
    AMX_HIP(hipMemcpy(h->d_seg_len.get(), h->len.data(), sizeof(int) * (size_t)n_seg, hipMemcpyHostToDevice));
    {
        amx::ScopedKernelTimer timer(t->ctx, "nnseq_pack");
        const amx::FeatSrc src{feats, ldf, t->pre};
        hipLaunchKernelGGL(amx::nnseq_pack_kernel, dim3(std::min(4096, blocks_for((long long)R * t->Pin[0]))), dim3(amx::kSeqThreads), 0, st, src,
                           (const long long*)h->d_row_src.get(), R, t->in[0], t->d_x[0].get(), t->Pin[0]);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(t->ctx, "nnseq_gemm_forward");
        amx::nntrain_launch_forward(t, R, R, st);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(t->ctx, "nnseq_pack");
        for (int l = 1; l < L; ++l)
            hipLaunchKernelGGL(amx::nnseq_zero_rows_kernel, dim3(std::min(4096, blocks_for((long long)R * t->Pin[l]))), dim3(amx::kSeqThreads), 0, st,
                               t->d_x[l].get(), t->Pin[l], (const long long*)h->d_row_src.get(), R);
        AMX_HIP(hipGetLastError());
    }
    h->forwarded = true, h->top_softmax = false, h->accumulated = false;
    h->epoch = ++t->workspace_epoch;
    return AMX_OK;
}

int amx_nnseq_arc_scores_dev(amx_nnseq* h, const long* arc_offsets, const long* item_offsets, const int32_t* item_frame, const int32_t* item_emission,
                             float* arc_score_dev) {
    const char* who = "amx_nnseq_arc_scores_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL argument", who);
    amx_nntrain* t = h->t;
    AMX_REQUIRE(t->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(h->forwarded, AMX_ERR_STATE, "%s: no forward pass has run (amx_nnseq_forward_dev)", who);
    AMX_REQUIRE(h->epoch == t->workspace_epoch, AMX_ERR_STATE, "%s: another call has used the nntrain handle's workspace since the forward pass: run it again", who);
    AMX_REQUIRE(!h->top_softmax, AMX_ERR_STATE, "%s: the smoothing of amx_nnseq_accumulate_dev has replaced the linear top output by its softmax: run the forward pass again", who);
    long long n_arcs = 0, n_items = 0;
    AMX_TRY(amx::nnseq_check_tables(who, h->n_seg, arc_offsets, item_offsets, item_frame, item_emission, &n_arcs, &n_items));
    if (n_arcs == 0)
        return AMX_OK;
    AMX_REQUIRE(arc_score_dev, AMX_ERR_INVALID, "%s: arc_score_dev is NULL", who);
    hipStream_t st = t->ctx->stream;
    AMX_HIP(hipSetDevice(t->ctx->device));
    AMX_TRY(upload_tables(h, st, h->n_seg, arc_offsets, item_offsets, item_frame, item_emission, n_arcs, n_items));
    AMX_HIP(hipMemsetAsync(h->d_bad.get(), 0xff, 8, st));
    {
        amx::ScopedKernelTimer timer(t->ctx, "nnseq_scores");
        hipLaunchKernelGGL(amx::nnseq_score_kernel, dim3((unsigned)((n_arcs + amx::kSeqArcs - 1) / amx::kSeqArcs)), dim3(amx::kSeqThreads), 0, st, n_arcs, h->n_seg,
                           (const long long*)h->d_arc_off.get(), (const long long*)h->d_item_off.get(), (const int32_t*)h->d_item_frame.get(),
                           (const int32_t*)h->d_item_emission.get(), (const int*)h->d_seg_row0.get(), (const int*)h->d_seg_len.get(),
                           (const int*)(t->class_to_output.empty() ? nullptr : t->d_c2o.get()), t->n_classes, t->n_outputs, (const float*)t->d_top.get(), arc_score_dev,
                           h->d_bad.get());
        AMX_HIP(hipGetLastError());
    }
    unsigned long long bad = 0;
    AMX_TRY(fetch_bad(h, st, &bad));
    return amx::nnseq_report_bad(who, bad);
}

int amx_nnseq_accumulate_dev(amx_nnseq* h, int n_pass, const amx_nnseq_pass* passes, const uint32_t* emission, const uint8_t* skip, const float* objective,
                             double* acc, amx_nnseq_info* info) {
    const char* who = "amx_nnseq_accumulate_dev";
    AMX_REQUIRE(h && acc && objective && emission, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(n_pass >= 0 && n_pass <= amx::kSeqMaxPasses && (n_pass == 0 || passes), AMX_ERR_INVALID, "%s: n_pass = %d (0..%d passes)", who, n_pass, amx::kSeqMaxPasses);
    for (int p = 0; p < n_pass; ++p) {
        AMX_REQUIRE(passes[p].role >= AMX_NNSEQ_ADD && passes[p].role <= AMX_NNSEQ_ADD_REJECT_CLEAR, AMX_ERR_INVALID, "%s: pass %d: unknown role %d", who, p, passes[p].role);
        AMX_REQUIRE(std::isfinite(passes[p].factor), AMX_ERR_INVALID, "%s: pass %d: factor is not finite", who, p);
    }
    amx_nntrain* t = h->t;
    AMX_REQUIRE(t->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(h->forwarded, AMX_ERR_STATE, "%s: no forward pass has run (amx_nnseq_forward_dev)", who);
    AMX_REQUIRE(h->epoch == t->workspace_epoch, AMX_ERR_STATE, "%s: another call has used the nntrain handle's workspace since the forward pass: run it again", who);
    AMX_REQUIRE(!h->accumulated, AMX_ERR_STATE, "%s: the batch of the last forward pass has been accumulated already", who);
    const int   n_seg = h->n_seg, R = h->rows, L = t->L, n_out = t->n_outputs, ldE = t->Pout[L - 1];
    const bool  grad = (t->mask & AMX_NNSTAT_GRADIENT) != 0;
    const float lambda = h->cfg.ce_smoothing_weight;
    const bool  lattice = grad && lambda < 1.f;  // objectiveFunctionOnly without a gradient; lambda == 1: E starts from zero
    std::vector<long long> n_arcs((size_t)n_pass, 0), n_items((size_t)n_pass, 0);
    if (lattice)
        for (int p = 0; p < n_pass; ++p) {
            AMX_TRY(amx::nnseq_check_tables(who, n_seg, passes[p].arc_offsets, passes[p].item_offsets, passes[p].item_frame, passes[p].item_emission, &n_arcs[p], &n_items[p]));
            AMX_REQUIRE(n_arcs[p] == 0 || passes[p].arc_weight_dev, AMX_ERR_INVALID, "%s: pass %d: arc_weight_dev is NULL", who, p);
        }
    std::vector<int> state((size_t)n_seg, 0);
    for (int s = 0; s < n_seg; ++s)
        state[s] = (skip && skip[s]) ? AMX_NNSEQ_SEG_SKIPPED : AMX_NNSEQ_SEG_OK;
    std::vector<unsigned> seg_err((size_t)n_seg, 0), seg_rej((size_t)n_seg, 0);
    std::vector<float>    seg_ce((size_t)n_seg, 0.f);
    if (R > 0) {
        hipStream_t st = t->ctx->stream;
        AMX_HIP(hipSetDevice(t->ctx->device));
        const int* c2o   = t->class_to_output.empty() ? nullptr : t->d_c2o.get();
        const int* row0  = h->d_seg_row0.get();
        const int* len   = h->d_seg_len.get();
        int*       sst   = h->d_seg_state.get();
        AMX_HIP(hipMemcpyAsync(sst, state.data(), sizeof(int) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        AMX_HIP(hipMemcpyAsync(h->d_objective.get(), objective, sizeof(float) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        AMX_HIP(hipStreamSynchronize(st));  // the two host arrays may be pageable
        AMX_HIP(hipMemsetAsync(h->d_seg_rej.get(), 0, sizeof(unsigned) * (size_t)n_seg, st));
        AMX_HIP(hipMemsetAsync(h->d_bad.get(), 0xff, 8, st));
        hipLaunchKernelGGL(amx::nnseq_alignment_kernel, dim3((R + amx::kSeqThreads - 1) / amx::kSeqThreads), dim3(amx::kSeqThreads), 0, st, R,
                           (const long long*)h->d_row_src.get(), (const int*)h->d_row_seg.get(), h->f0, emission, sst);
        hipLaunchKernelGGL(amx::nnseq_label_kernel, dim3((R + amx::kSeqThreads - 1) / amx::kSeqThreads), dim3(amx::kSeqThreads), 0, st, R,
                           (const long long*)h->d_row_src.get(), (const int*)h->d_row_seg.get(), h->f0, emission, c2o, (const float*)t->d_cw.get(), t->n_classes, n_out,
                           (const int*)sst, t->d_label.get(), t->d_w.get(), h->d_bad.get());
        AMX_HIP(hipGetLastError());
        float* Etop = grad ? t->d_E[L - 1].get() : nullptr;
        if (grad)
            AMX_HIP(hipMemsetAsync(Etop, 0, sizeof(float) * (size_t)R * ldE, st));
        h->last_passes = h->last_blocks = 0;
        if (lattice) {
            int                out_bits = 0, bits = 0;
            unsigned long long sentinel = 0;
            amx::nnseq_key_layout(R, n_out, &out_bits, &sentinel, &bits);
            for (int p = 0; p < n_pass; ++p) {
                const amx_nnseq_pass& ps = passes[p];
                const long long       na = n_arcs[p], ni = n_items[p], nt = std::max(na, ni);
                if (nt > 0) {
                    AMX_TRY(upload_tables(h, st, n_seg, ps.arc_offsets, ps.item_offsets, ps.item_frame, ps.item_emission, na, ni));
                    for (int b = 0; b < 2; ++b) {
                        AMX_TRY(h->d_code[b].reserve((size_t)std::max<long long>(ni, 1)));
                        AMX_TRY(h->d_val[b].reserve((size_t)std::max<long long>(ni, 1)));
                    }
                    int side = 0;
                    {
                        amx::ScopedKernelTimer timer(t->ctx, "nnseq_sort");
                        hipLaunchKernelGGL(amx::nnseq_resolve_kernel, dim3((unsigned)((nt + amx::kSeqThreads - 1) / amx::kSeqThreads)), dim3(amx::kSeqThreads), 0, st,
                                           p + 1, ni, na, n_seg, (const long long*)h->d_arc_off.get(), ps.arc_weight_dev, (const long long*)h->d_item_off.get(),
                                           (const int32_t*)h->d_item_frame.get(), (const int32_t*)h->d_item_emission.get(), row0, len, (const int*)sst, c2o,
                                           t->n_classes, n_out, ps.negate ? 1 : 0, h->cfg.weight_threshold, out_bits, sentinel, h->d_code[0].get(), h->d_val[0].get(),
                                           h->d_bad.get());
                        AMX_HIP(hipGetLastError());
                        if (ni > 0)
                            AMX_TRY(seq_sort(h, st, ni, bits, &side));
                    }
                    if (ni > 0) {
                        amx::ScopedKernelTimer timer(t->ctx, "nnseq_collect");
                        hipLaunchKernelGGL(amx::nnseq_collect_kernel, dim3((unsigned)((ni + amx::kSeqThreads - 1) / amx::kSeqThreads)), dim3(amx::kSeqThreads), 0, st,
                                           (const unsigned long long*)h->d_code[side].get(), (const uint32_t*)h->d_val[side].get(), ni, sentinel, out_bits, ps.factor,
                                           Etop, ldE);
                        AMX_HIP(hipGetLastError());
                    }
                }
                if (ps.role != AMX_NNSEQ_ADD) {
                    amx::ScopedKernelTimer timer(t->ctx, "nnseq_reject");
                    if (h->cfg.frame_rejection_threshold > 0.f)
                        hipLaunchKernelGGL(amx::nnseq_reject_kernel, dim3((R + amx::kSeqThreads - 1) / amx::kSeqThreads), dim3(amx::kSeqThreads), 0, st, p + 1, R,
                                           (const int*)h->d_row_seg.get(), (const int*)sst, (const int*)t->d_label.get(), (const float*)Etop, ldE,
                                           h->cfg.frame_rejection_threshold, t->d_w.get(), h->d_seg_rej.get(), h->d_bad.get());
                    if (ps.role == AMX_NNSEQ_ADD_REJECT_CLEAR)
                        AMX_HIP(hipMemsetAsync(Etop, 0, sizeof(float) * (size_t)R * ldE, st));
                    AMX_HIP(hipGetLastError());
                }
            }
        }
        unsigned long long bad = 0;
        AMX_TRY(fetch_bad(h, st, &bad));
        AMX_TRY(amx::nnseq_report_bad(who, bad));  // nothing of acc_dev has been touched
        if (grad && h->cfg.keep_lattice_error) {
            AMX_TRY(h->d_E_lattice.reserve((size_t)R * ldE));
            AMX_HIP(hipMemcpyAsync(h->d_E_lattice.get(), Etop, sizeof(float) * (size_t)R * ldE, hipMemcpyDeviceToDevice, st));
        }
        {
            amx::ScopedKernelTimer timer(t->ctx, "nnseq_smooth");
            if (lambda > 0.f) {
                if (h->cfg.prior_scale > 0.f && h->d_prior.get())
                    hipLaunchKernelGGL(amx::nnseq_prior_kernel, dim3(blocks_for((long long)R * n_out)), dim3(amx::kSeqThreads), 0, st, t->d_top.get(), (long long)R * n_out,
                                       n_out, (const float*)h->d_prior.get(), h->cfg.prior_scale);
                amx::nntrain_launch_softmax(t, R, st);
                h->top_softmax = true;
            }
            hipLaunchKernelGGL(amx::nnseq_smooth_kernel, dim3(R), dim3(amx::kSeqThreads), 0, st, (const float*)t->d_top.get(), n_out, lambda > 0.f ? 1 : 0, lambda,
                               (float)(1.0 - (double)lambda), (const int*)h->d_row_seg.get(), (const int*)sst, (const int*)t->d_label.get(), (const float*)t->d_w.get(),
                               Etop, ldE, t->d_err.get(), h->d_term.get());
            AMX_HIP(hipGetLastError());
        }
        const amx_nntrain_layout_info& y = t->lay;
        if (grad) {
            {
                amx::ScopedKernelTimer timer(t->ctx, "nnseq_gemm_backward");
                amx::nntrain_launch_backward(t, R, FLT_MAX, st);  // the segment-wise trainer has no error-signal-clip
                AMX_HIP(hipGetLastError());
            }
            const int n_chunks = R / AMX_NNTRAIN_CHUNK;
            for (int l = L - 1; l >= 0; --l) {
                const int Kp = t->Pin[l], Np = t->Pout[l];
                {
                    amx::ScopedKernelTimer timer(t->ctx, "nnseq_gemm_tn");
                    amx::nntrain_launch_gemm_tn(t, l, R, n_chunks, st);
                }
                amx::ScopedKernelTimer timer(t->ctx, "nnseq_gradient_sums");
                hipLaunchKernelGGL(amx::nnseq_reduce_kernel, dim3(blocks_for((long long)t->in[l] * t->out[l])), dim3(amx::kSeqThreads), 0, st,
                                   (const float*)t->d_part.get(), (size_t)Kp * Np, t->in[l], t->out[l], Np, n_seg, row0, len, (const int*)sst, acc + y.gradient_weights[l]);
                amx::nntrain_launch_bias_sums(t, l, R, n_chunks, st);
                hipLaunchKernelGGL(amx::nnseq_reduce_kernel, dim3(std::min(1024, blocks_for(t->out[l]))), dim3(amx::kSeqThreads), 0, st, (const float*)t->d_part.get(),
                                   (size_t)t->out[l], 1, t->out[l], t->out[l], n_seg, row0, len, (const int*)sst, acc + y.gradient_bias[l]);
                AMX_HIP(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(amx::nnseq_tail_kernel, dim3(1), dim3(256), 0, st, n_seg, row0, len, (const int*)sst, (const int*)t->d_label.get(), (const float*)t->d_w.get(),
                           (const unsigned*)t->d_err.get(), (const float*)h->d_term.get(), (const float*)h->d_objective.get(), h->d_seg_err.get(), h->d_seg_ce.get(),
                           acc + y.tail);
        AMX_HIP(hipGetLastError());
        AMX_HIP(hipMemcpyAsync(state.data(), sst, sizeof(int) * (size_t)n_seg, hipMemcpyDeviceToHost, st));
        AMX_HIP(hipMemcpyAsync(seg_err.data(), h->d_seg_err.get(), sizeof(unsigned) * (size_t)n_seg, hipMemcpyDeviceToHost, st));
        AMX_HIP(hipMemcpyAsync(seg_rej.data(), h->d_seg_rej.get(), sizeof(unsigned) * (size_t)n_seg, hipMemcpyDeviceToHost, st));
        AMX_HIP(hipMemcpyAsync(seg_ce.data(), h->d_seg_ce.get(), sizeof(float) * (size_t)n_seg, hipMemcpyDeviceToHost, st));
        AMX_HIP(hipStreamSynchronize(st));
    }
    h->accumulated = true;
    if (info) {
        info->segments_processed = info->segments_skipped = info->segments_without_alignment = 0;
        info->observations = info->rejected_observations = 0;
        info->ce_objective = 0.f;
        for (int s = 0; s < n_seg; ++s) {
            const int reason = (state[s] & AMX_NNSEQ_SEG_SKIPPED) ? AMX_NNSEQ_SEG_SKIPPED : state[s] ? AMX_NNSEQ_SEG_NO_ALIGNMENT : AMX_NNSEQ_SEG_OK;
            if (reason == AMX_NNSEQ_SEG_OK && h->len[s] > 0) {
                ++info->segments_processed;
                info->observations += h->len[s];
                info->rejected_observations += seg_rej[s];
                info->ce_objective = info->ce_objective + seg_ce[s];
            }
            else if (reason == AMX_NNSEQ_SEG_SKIPPED)
                ++info->segments_skipped;
            else if (reason == AMX_NNSEQ_SEG_NO_ALIGNMENT)
                ++info->segments_without_alignment;
            const bool ok = reason == AMX_NNSEQ_SEG_OK;
            if (info->seg_reason)
                info->seg_reason[s] = reason;
            if (info->seg_errors)
                info->seg_errors[s] = ok ? seg_err[s] : 0;
            if (info->seg_rejected)
                info->seg_rejected[s] = ok ? seg_rej[s] : 0;
            if (info->seg_ce_objective)
                info->seg_ce_objective[s] = ok ? seg_ce[s] : 0.f;
        }
    }
    return AMX_OK;
}

int amx_nnseq_workspace_row(const amx_nnseq* h, int segment, int* row) {
    AMX_REQUIRE(h && row, AMX_ERR_INVALID, "amx_nnseq_workspace_row: NULL argument");
    AMX_REQUIRE(h->forwarded, AMX_ERR_STATE, "amx_nnseq_workspace_row: no forward pass has run");
    AMX_REQUIRE(segment >= 0 && segment <= h->n_seg, AMX_ERR_INVALID, "amx_nnseq_workspace_row: segment %d of %d", segment, h->n_seg);
    *row = h->row0[segment];
    return AMX_OK;
}

static int get_rows(amx_nnseq* h, const char* who, const float* src, int ld, int cols, int row, int n, float* out) {
    AMX_REQUIRE(row >= 0 && n >= 0 && row + n <= h->rows, AMX_ERR_INVALID, "%s: rows [%d, %d) of %d", who, row, row + n, h->rows);
    if (n == 0)
        return AMX_OK;
    AMX_REQUIRE(out && src, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_HIP(hipSetDevice(h->t->ctx->device));
    AMX_HIP(hipStreamSynchronize(h->t->ctx->stream));
    if (ld == cols)
        AMX_HIP(hipMemcpy(out, src + (size_t)row * ld, sizeof(float) * (size_t)n * cols, hipMemcpyDeviceToHost));
    else
        AMX_HIP(hipMemcpy2D(out, sizeof(float) * (size_t)cols, src + (size_t)row * ld, sizeof(float) * (size_t)ld, sizeof(float) * (size_t)cols, (size_t)n, hipMemcpyDeviceToHost));
    return AMX_OK;
}

int amx_nnseq_get_top(amx_nnseq* h, int which, int row, int n, float* out) {
    const char* who = "amx_nnseq_get_top";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(h->t->ctx && h->forwarded, AMX_ERR_STATE, "%s: no forward pass has run on a device", who);
    AMX_REQUIRE(which == 0 || which == 1, AMX_ERR_INVALID, "%s: which = %d", who, which);
    AMX_REQUIRE((which == 1) == h->top_softmax, AMX_ERR_STATE, "%s: the workspace holds the %s", who, h->top_softmax ? "softmax" : "linear top output");
    const int n_out = h->t->n_outputs;
    AMX_TRY(get_rows(h, who, h->t->d_top.get(), n_out, n_out, row, n, out));
    if (which == 0)  // the workspace keeps the negated output, as the scorers do
        for (size_t i = 0; i < (size_t)n * n_out; ++i)
            out[i] = -out[i];
    return AMX_OK;
}

int amx_nnseq_get_error_signal(amx_nnseq* h, int layer, int row, int n, float* out) {
    const char* who = "amx_nnseq_get_error_signal";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(h->t->ctx && h->accumulated, AMX_ERR_STATE, "%s: no accumulate has run on a device", who);
    AMX_REQUIRE(h->t->mask & AMX_NNSTAT_GRADIENT, AMX_ERR_STATE, "%s: the handle's statistics have no gradient, so there is no error signal", who);
    const int L = h->t->L;
    AMX_REQUIRE(layer >= -1 && layer < L, AMX_ERR_INVALID, "%s: layer %d of %d", who, layer, L);
    if (layer == -1) {
        AMX_REQUIRE(h->cfg.keep_lattice_error, AMX_ERR_STATE, "%s: cfg.keep_lattice_error was not set", who);
        return get_rows(h, who, h->d_E_lattice.get(), h->t->Pout[L - 1], h->t->n_outputs, row, n, out);
    }
    return get_rows(h, who, h->t->d_E[layer].get(), h->t->Pout[layer], h->t->out[layer], row, n, out);
}

int amx_nnseq_get_weights(amx_nnseq* h, int row, int n, float* out) {
    const char* who = "amx_nnseq_get_weights";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(h->t->ctx && h->accumulated, AMX_ERR_STATE, "%s: no accumulate has run on a device", who);
    return get_rows(h, who, h->t->d_w.get(), 1, 1, row, n, out);
}

int amx_nnseq_last_shape(const amx_nnseq* h, int* sort_passes, int* sort_blocks) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_nnseq_last_shape: NULL argument");
    if (sort_passes)
        *sort_passes = h->last_passes;
    if (sort_blocks)
        *sort_blocks = h->last_blocks;
    return AMX_OK;
}

}  // extern "C"
