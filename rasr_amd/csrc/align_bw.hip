// align_bw.hip -- Search::Aligner in mode baum-welch on a [frames x emissions] score matrix that is already on the device (include/amx.h,
// section "Baum-Welch alignment"): forward search with pruning, f64 forward and backward potentials over the last pass's survivors, and
// the per-frame item list (label, emission index, posterior weight) that amx_gmm_accumulate_weighted_dev takes.
//
// One workgroup per segment in every kernel, the segment's states in LDS; the host plan, the compact score matrix and the pass loop are
// the Viterbi entry's (align_plan.hpp).
//   bw_search_kernel    all pruning passes.  A state walks its incoming arcs in the static by-target order; its candidates
//                       score + (weight + emission) are f32, their log-sum min - log1p(sum exp(min - c)) is f64 and is rounded to f32 once.
//                       The last pass leaves a survivor bit per (frame, state).
//   bw_forward_kernel   one f64 sweep over those survivors, the potentials per (frame, state) go to memory
//   bw_backward_kernel  frames descend, beta double-buffered in LDS.  Per frame a LABEL walks its arcs (the host sorted them by label, then
//                       by target) and sums exp(-(fw + w + bw - total)); the frame's sum is a fixed tree over lanes and waves; weights > 0
//                       become items.  Run twice: counting, then (after bw_scan_kernel) writing into the handle's store, each frame's
//                       items sorted by (decreasing weight, label) in LDS.  `total` is the forward sweep's total flow: it cancels in the
//                       per-frame normalisation and only keeps exp() in range; bw[initial] is reported as log_total.
// Every sum has one order that depends on the segment's graph alone.  The only atomics are integer ones (the append position of a
// frame's items before their sort).
#include <cstdint>

#include "align_plan.hpp"

namespace amx {

constexpr double kBwDead      = 1.7976931348623157e308;   // Fsa/Sssp.cc:67 "Zero": the potential of a state no path goes through
constexpr int    kBwMaxLabels = AMX_BW_MAX_LABELS;
static_assert((kBwMaxLabels & (kBwMaxLabels - 1)) == 0, "the sort pads to a power of two");

struct BwSeg {
    long long al0;   // first word of the potentials, [frames + 1][states]
    long long sv0;   // first word of the survivor bits, [frames][sw]
    int       sw;    // 64-bit words per frame
    int       lab0, n_labels;
};

struct BwSummary {
    float              score;
    int                reached, n_iterations;
    float              last_threshold;
    double             average;
    unsigned long long sum;
    int                nan, pad;
    unsigned long long passes_run, passes_counted;
};

struct BwTotals {
    double    log_total;
    long long n_items;
};

struct BwSearchArgs {
    const AlignSeg*      seg;
    const BwSeg*         bseg;
    const int*           in_off;
    const AlignArc*      in_arc;
    const unsigned char* is_final;
    const float*         final_w;
    const float*         cm;
    unsigned long long*  surv;
    BwSummary*           summary;
    AlignLoop            loop;
    int                  lds_states, lds_cols;
};

// min - log1p(sum over the others of exp(min - x)): `m` the minimum, `sum` over all candidates but the first minimal one
__device__ __forceinline__ double bw_logsum(double m, double sum) { return m - log1p(sum); }

__global__ __launch_bounds__(kAlignThreads) void bw_search_kernel(BwSearchArgs p) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ float s_min[kAlignWaves], s_final;
    __shared__ int   s_cnt[kAlignWaves], s_new[kAlignWaves], s_nan;
    const int      tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AlignSeg sg  = p.seg[blockIdx.x];
    const BwSeg    bs  = p.bseg[blockIdx.x];
    const int      S = sg.n_states, E = sg.n_cols, T = sg.frames;
    const int      KS = (S + kAlignThreads - 1) / kAlignThreads;
    // LDS: scores[2] | alive[2] | incoming offsets | row
    float*          score  = (float*)lds_raw;
    int*            alive  = (int*)(score + 2 * p.lds_states);
    int*            in_off = alive + 2 * p.lds_states;
    float*          row    = (float*)(in_off + p.lds_states + 1);
    const AlignArc* arcs   = p.in_arc + sg.in0;
    for (int s = tid; s <= S; s += kAlignThreads)
        in_off[s] = p.in_off[sg.state0 + s] - sg.in0;
    if (tid == 0)
        s_nan = 0;
    const float*       cm   = p.cm + sg.cm0;
    unsigned long long* sv  = p.surv + bs.sv0;
    const AlignLoop    lp   = p.loop;
    float              t    = lp.lo, previous = kAlignF32Max, pass_score = kAlignF32Max;
    int                n_iter = 0;
    unsigned long long sum = 0, passes_run = 0, passes_counted = 0;
    double             avg = 0;
    bool               nan = false;
    __syncthreads();
    while (t <= lp.hi) {
        ++n_iter, ++passes_run;
        for (int s = tid; s < S; s += kAlignThreads) {
            alive[s] = s == sg.initial;
            score[s] = 0.f;
        }
        int  cur    = 0;
        bool pruned = false;
        sum         = 0;
        __syncthreads();
        for (int f = 0; f < T; ++f) {
            const int    nxt = cur ^ 1;
            const float* sc  = score + cur * p.lds_states;
            const int*   ac  = alive + cur * p.lds_states;
            float*       sn  = score + nxt * p.lds_states;
            int*         an  = alive + nxt * p.lds_states;
            for (int j = tid; j < E; j += kAlignThreads)
                row[j] = cm[(long long)f * E + j];
            __syncthreads();
            // expansion and recombination, one target state at a time (:215-252, :169-196)
            float m       = kAlignF32Max;
            int   n_new   = 0;
            bool  met_nan = false;
            for (int s = tid; s < S; s += kAlignThreads) {
                int   n = 0, first = -1;
                float best = 0.f;
                for (int a = in_off[s]; a < in_off[s + 1]; ++a) {
                    const AlignArc q   = arcs[a];
                    const int      src = q.x & 0xffff;
                    if (!ac[src])
                        continue;
                    const float arc = __int_as_float(q.z) + row[q.y];   // :238
                    const float c   = sc[src] + arc;                    // :239
                    met_nan         = met_nan || c != c;
                    if (n == 0 || c < best)
                        best = c, first = a;
                    ++n;
                }
                float v = best;
                if (n > 1) {
                    double acc = 0.0;
                    for (int a = in_off[s]; a < in_off[s + 1]; ++a) {
                        const AlignArc q   = arcs[a];
                        const int      src = q.x & 0xffff;
                        if (!ac[src] || a == first)
                            continue;
                        const float arc = __int_as_float(q.z) + row[q.y];
                        const float c   = sc[src] + arc;
                        acc += exp((double)best - (double)c);
                    }
                    v       = (float)bw_logsum((double)best, acc);
                    met_nan = met_nan || v != v;
                }
                sn[s] = v;
                an[s] = n > 0;
                if (n > 0) {
                    ++n_new;
                    m = v < m ? v : m;   // minimumScore (:254-261)
                }
            }
            if (met_nan)
                s_nan = 1;
            m     = wave_min(m);
            n_new = wave_sum(n_new);
            if (lane == 0)
                s_min[wave] = m, s_new[wave] = n_new;
            __syncthreads();
            m = kAlignF32Max, n_new = 0;
#pragma unroll
            for (int w = 0; w < kAlignWaves; ++w) {
                m = s_min[w] < m ? s_min[w] : m;
                n_new += s_new[w];
            }
            const float limit = m + t;   // :597
            int         kept  = 0;
            for (int k = 0; k < KS; ++k) {
                const int  s    = k * kAlignThreads + tid;
                const bool keep = s < S && an[s] && sn[s] <= limit;   // :305
                if (s < S)
                    an[s] = keep;
                kept += keep;
                const unsigned long long b = __ballot(keep);
                if (lane == 0 && k * kAlignWaves + wave < bs.sw)
                    sv[(long long)f * bs.sw + k * kAlignWaves + wave] = b;
            }
            kept = wave_sum(kept);
            if (lane == 0)
                s_cnt[wave] = kept;
            __syncthreads();
            kept = 0;
#pragma unroll
            for (int w = 0; w < kAlignWaves; ++w)
                kept += s_cnt[w];
            sum += (unsigned)kept;
            pruned = pruned || kept < n_new;
            cur    = nxt;
            if (s_nan)   // set before the frame's second barrier, read behind its third by every lane alike: the pass ends here
                break;
        }
        // finalStatePotential (:385-405): the final hypotheses collected like a state's candidates, in state order
        if (tid == 0) {
            const float* sc = score + cur * p.lds_states;
            const int*   ac = alive + cur * p.lds_states;
            int          n = 0, first = -1;
            float        best = 0.f;
            bool         bad  = false;
            for (int s = 0; s < S; ++s)
                if (ac[s] && p.is_final[sg.state0 + s]) {
                    const float v = p.final_w[sg.state0 + s] + sc[s];
                    bad           = bad || v != v;
                    if (!(v < kAlignF32Max))
                        continue;
                    if (n == 0 || v < best)
                        best = v, first = s;
                    ++n;
                }
            float r = n ? best : kAlignF32Max;
            if (n > 1) {
                double acc = 0.0;
                for (int s = 0; s < S; ++s)
                    if (ac[s] && p.is_final[sg.state0 + s] && s != first) {
                        const float v = p.final_w[sg.state0 + s] + sc[s];
                        if (v < kAlignF32Max)
                            acc += exp((double)best - (double)v);
                    }
                r   = (float)bw_logsum((double)best, acc);
                bad = bad || r != r;
            }
            s_final = r;
            if (bad)
                s_nan = 1;
        }
        __syncthreads();
        pass_score = s_final;
        nan        = s_nan != 0;
        __syncthreads();   // s_final and the state buffers are free for the next pass
        if (nan)
            break;
        avg                = (double)(unsigned)sum / (double)(unsigned)T;
        const bool reached = pass_score != kAlignF32Max;
        if (align_pass_ends(lp, t, reached, avg, pass_score, previous))
            break;
        previous = pass_score;
        if (!pruned) {
            align_count_repeats(lp, &t, reached, avg, pass_score, &n_iter, &passes_counted);
            break;
        }
        const float next = t * lp.factor;
        if (!(next <= lp.hi))
            break;
        t = next;
    }
    if (tid == 0) {
        BwSummary r;
        r.score          = nan ? kAlignF32Max : pass_score;
        r.reached        = !nan && pass_score != kAlignF32Max;
        r.n_iterations   = n_iter;
        r.last_threshold = t;
        r.average        = nan ? 0.0 : avg;
        r.sum            = nan ? 0 : sum;
        r.nan = nan, r.pad = 0;
        r.passes_run = passes_run, r.passes_counted = passes_counted;
        p.summary[blockIdx.x] = r;
    }
}

struct BwForwardArgs {
    const AlignSeg*           seg;
    const BwSeg*              bseg;
    const int*                in_off;
    const AlignArc*           in_arc;
    const unsigned char*      is_final;
    const float*              final_w;
    const float*              cm;
    const unsigned long long* surv;
    const BwSummary*          summary;
    double*                   alpha;
    double*                   fw_total;   // [n_seg]
    int                       lds_states, lds_cols;
};

__global__ __launch_bounds__(kAlignThreads) void bw_forward_kernel(BwForwardArgs p) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int      tid = threadIdx.x;
    const AlignSeg sg  = p.seg[blockIdx.x];
    const BwSeg    bs  = p.bseg[blockIdx.x];
    const int      S = sg.n_states, E = sg.n_cols, T = sg.frames;
    if (!p.summary[blockIdx.x].reached) {   // the same in every lane
        if (tid == 0)
            p.fw_total[blockIdx.x] = kBwDead;
        return;
    }
    // LDS: potentials[2] | incoming offsets | row
    double*         al     = (double*)lds_raw;
    int*            in_off = (int*)(al + 2 * p.lds_states);
    float*          row    = (float*)(in_off + p.lds_states + 1);
    const AlignArc* arcs   = p.in_arc + sg.in0;
    const float*    cm     = p.cm + sg.cm0;
    double*         ag     = p.alpha + bs.al0;
    const unsigned long long* sv = p.surv + bs.sv0;
    for (int s = tid; s <= S; s += kAlignThreads)
        in_off[s] = p.in_off[sg.state0 + s] - sg.in0;
    for (int s = tid; s < S; s += kAlignThreads) {
        const double v = s == sg.initial ? 0.0 : kBwDead;
        al[s]          = v;
        ag[s]          = v;
    }
    int cur = 0;
    __syncthreads();
    for (int f = 0; f < T; ++f) {
        const double* ac = al + cur * p.lds_states;
        double*       an = al + (cur ^ 1) * p.lds_states;
        for (int j = tid; j < E; j += kAlignThreads)
            row[j] = cm[(long long)f * E + j];
        __syncthreads();
        for (int s = tid; s < S; s += kAlignThreads) {
            double v = kBwDead;
            if ((sv[(long long)f * bs.sw + (s >> 6)] >> (s & 63)) & 1ull) {
                int    n = 0, first = -1;
                double best = 0.0;
                for (int a = in_off[s]; a < in_off[s + 1]; ++a) {
                    const AlignArc q = arcs[a];
                    const double   x = ac[q.x & 0xffff] + (double)(__int_as_float(q.z) + row[q.y]);
                    if (!(x < kBwDead))
                        continue;
                    if (n == 0 || x < best)
                        best = x, first = a;
                    ++n;
                }
                if (n == 1)
                    v = best;
                else if (n > 1) {
                    double acc = 0.0;
                    for (int a = in_off[s]; a < in_off[s + 1]; ++a) {
                        const AlignArc q = arcs[a];
                        const double   x = ac[q.x & 0xffff] + (double)(__int_as_float(q.z) + row[q.y]);
                        if (x < kBwDead && a != first)
                            acc += exp(best - x);
                    }
                    v = bw_logsum(best, acc);
                }
                if (!(v < kBwDead))
                    v = kBwDead;
            }
            an[s]                          = v;
            ag[(long long)(f + 1) * S + s] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (tid == 0) {
        const double* ac = al + cur * p.lds_states;
        int           n = 0, first = -1;
        double        best = 0.0;
        for (int s = 0; s < S; ++s)
            if (p.is_final[sg.state0 + s] && p.final_w[sg.state0 + s] < kAlignF32Max) {
                const double x = ac[s] + (double)p.final_w[sg.state0 + s];
                if (!(x < kBwDead))
                    continue;
                if (n == 0 || x < best)
                    best = x, first = s;
                ++n;
            }
        double v = n ? best : kBwDead;
        if (n > 1) {
            double acc = 0.0;
            for (int s = 0; s < S; ++s)
                if (p.is_final[sg.state0 + s] && p.final_w[sg.state0 + s] < kAlignF32Max && s != first) {
                    const double x = ac[s] + (double)p.final_w[sg.state0 + s];
                    if (x < kBwDead)
                        acc += exp(best - x);
                }
            v = bw_logsum(best, acc);
        }
        p.fw_total[blockIdx.x] = v < kBwDead ? v : kBwDead;
    }
}

// arcs by source: x = target, y = column of the compact matrix, z = weight bits, w = index of the label
// arcs by label:  x = source, y = target, z = column, w = weight bits
typedef int4 BwArc;

struct BwBackwardArgs {
    const AlignSeg*      seg;
    const BwSeg*         bseg;
    const int*           out_off;   // [states + 1] by source, global
    const BwArc*         out_arc;
    const int*           lab_off;   // [labels + 1], global
    const BwArc*         lab_arc;
    const int*           lab_val;   // [labels]
    const int*           lab_em;
    const unsigned char* is_final;
    const float*         final_w;
    const float*         cm;
    const double*        alpha;
    const BwSummary*     summary;
    const double*        fw_total;
    BwTotals*            totals;
    int*                 count;      // [rows of the call]
    const long long*     item_off;   // absolute rows
    const long long*     n_total;
    long long            capacity, base;
    int32_t *            o_frame, *o_label, *o_emission;
    float*               o_weight;
    double*              o_weight64;
    int                  lds_states, lds_cols, lds_labels;
};

template<bool WRITE>
__global__ __launch_bounds__(kAlignThreads) void bw_backward_kernel(BwBackwardArgs p) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ double s_red[kAlignWaves];
    __shared__ int    s_c[kAlignWaves], s_n;
    const int      tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AlignSeg sg  = p.seg[blockIdx.x];
    const BwSeg    bs  = p.bseg[blockIdx.x];
    const int      S = sg.n_states, E = sg.n_cols, T = sg.frames, L = bs.n_labels;
    const double   tot = p.fw_total[blockIdx.x];
    // every condition of an early return is the same in every lane
    if (!p.summary[blockIdx.x].reached || !(tot < kBwDead)) {
        if (!WRITE && tid == 0)
            p.totals[blockIdx.x].log_total = kBwDead;
        return;
    }
    if (WRITE && *p.n_total > p.capacity)
        return;
    // LDS: alpha of the frame | beta[2] | label sums | sort keys | row
    double*             alf  = (double*)lds_raw;
    double*             be   = alf + p.lds_states;
    double*             P    = be + 2 * p.lds_states;
    unsigned long long* keys = (unsigned long long*)(P + p.lds_labels);
    float*              row  = (float*)(keys + (WRITE ? p.lds_labels : 0));
    const float*        cm   = p.cm + sg.cm0;
    const double*       ag   = p.alpha + bs.al0;
    const int*          ooff = p.out_off + sg.state0;
    const int*          loff = p.lab_off + bs.lab0;
    {
        double* bT = be + (T & 1) * p.lds_states;
        for (int s = tid; s < S; s += kAlignThreads) {
            const float fw = p.final_w[sg.state0 + s];
            bT[s]          = p.is_final[sg.state0 + s] && fw < kAlignF32Max && ag[(long long)T * S + s] < kBwDead ? (double)fw : kBwDead;
        }
    }
    __syncthreads();
    for (int f = T - 1; f >= 0; --f) {
        const double* bn = be + ((f + 1) & 1) * p.lds_states;
        double*       bc = be + (f & 1) * p.lds_states;
        for (int s = tid; s < S; s += kAlignThreads)
            alf[s] = ag[(long long)f * S + s];
        for (int j = tid; j < E; j += kAlignThreads)
            row[j] = cm[(long long)f * E + j];
        if (tid == 0)
            s_n = 0;
        __syncthreads();
        // a label's arcs, sorted by target, then source, then ordinal
        double part = 0.0;
        for (int l = tid; l < L; l += kAlignThreads) {
            double acc = 0.0;
            for (int a = loff[l]; a < loff[l + 1]; ++a) {
                const BwArc  q  = p.lab_arc[a];
                const double fa = alf[q.x], bb = bn[q.y];
                if (fa < kBwDead && bb < kBwDead) {
                    const double lp = ((fa + (double)(__int_as_float(q.w) + row[q.z])) + bb) - tot;   // Sssp.cc:156-159
                    if (lp < (double)kAlignF32Max)
                        acc += exp(-lp);
                }
            }
            P[l] = acc;
            part += acc;
        }
        // beta of the frame: a state's outgoing arcs in the graph's order
        for (int s = tid; s < S; s += kAlignThreads) {
            double v = kBwDead;
            if (alf[s] < kBwDead) {
                int    n = 0, first = -1;
                double best = 0.0;
                for (int a = ooff[s]; a < ooff[s + 1]; ++a) {
                    const BwArc  q = p.out_arc[a];
                    const double x = bn[q.x] + (double)(__int_as_float(q.z) + row[q.y]);
                    if (!(x < kBwDead))
                        continue;
                    if (n == 0 || x < best)
                        best = x, first = a;
                    ++n;
                }
                if (n == 1)
                    v = best;
                else if (n > 1) {
                    double acc = 0.0;
                    for (int a = ooff[s]; a < ooff[s + 1]; ++a) {
                        const BwArc  q = p.out_arc[a];
                        const double x = bn[q.x] + (double)(__int_as_float(q.z) + row[q.y]);
                        if (x < kBwDead && a != first)
                            acc += exp(best - x);
                    }
                    v = bw_logsum(best, acc);
                }
                if (!(v < kBwDead))
                    v = kBwDead;
            }
            bc[s] = v;
        }
        // the frame's sum: a lane's labels in order, lanes by a fixed tree, waves in order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            part += __shfl_down(part, o, 64);
        if (lane == 0)
            s_red[wave] = part;
        __syncthreads();
        const double Z = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        int          cnt = 0;
        for (int l = tid; l < L; l += kAlignThreads) {
            const float w = (float)(P[l] / Z);
            if (w > 0.f) {
                if (WRITE)
                    keys[atomicAdd(&s_n, 1)] = ((unsigned long long)(~__float_as_uint(w)) << 32) | (unsigned)l;
                else
                    ++cnt;
            }
        }
        if (!WRITE) {
            cnt = wave_sum(cnt);
            if (lane == 0)
                s_c[wave] = cnt;
            __syncthreads();
            if (tid == 0)
                p.count[sg.frame0 - p.base + f] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        } else {
            __syncthreads();
            const int n  = s_n;   // at most L <= lds_labels
            int       n2 = 1;
            while (n2 < n)
                n2 <<= 1;
            for (int i = n + tid; i < n2; i += kAlignThreads)
                keys[i] = ~0ull;
            __syncthreads();
            // bitonic sort, ascending: the keys are distinct (a label appears once), so the order they were appended in leaves no trace
            for (int k = 2; k <= n2; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < n2; i += kAlignThreads) {
                        const int x = i ^ j;
                        if (x > i) {
                            const unsigned long long a = keys[i], b = keys[x];
                            if (((i & k) == 0) == (a > b))
                                keys[i] = b, keys[x] = a;
                        }
                    }
                    __syncthreads();
                }
            const long long at = p.item_off[sg.frame0 + f];
            for (int i = tid; i < n; i += kAlignThreads) {
                const unsigned long long key = keys[i];
                const int                l   = (int)(key & 0xffffffffull);
                const float              w   = __uint_as_float(~(unsigned)(key >> 32));
                p.o_frame[at + i]    = (int32_t)(sg.frame0 + f);
                p.o_label[at + i]    = p.lab_val[bs.lab0 + l];
                p.o_emission[at + i] = p.lab_em[bs.lab0 + l];
                p.o_weight[at + i]   = w;
                p.o_weight64[at + i] = (double)w;
            }
        }
        __syncthreads();
    }
    if (!WRITE && tid == 0)
        p.totals[blockIdx.x].log_total = be[sg.initial];   // beta of frame 0 lies in the first buffer
}

// One workgroup: the exclusive scan of the per-row item counts into item_off (absolute rows; rows below `base` have none), the total and
// the items per segment.
__global__ __launch_bounds__(kAlignThreads) void bw_scan_kernel(const int* __restrict__ count, long long n, long long base, long long* __restrict__ item_off,
                                                                long long* __restrict__ n_total, const long long* __restrict__ off, int n_seg,
                                                                BwTotals* __restrict__ totals) {
    __shared__ long long s_w[kAlignWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long t = tid; t < base; t += kAlignThreads)
        item_off[t] = 0;
    long long carry = 0;
    for (long long c0 = 0; c0 < n; c0 += kAlignThreads) {
        const long long i    = c0 + tid;
        const long long v    = i < n ? count[i] : 0;
        long long       incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long u = __shfl_up(incl, o, 64);
            incl += lane >= o ? u : 0;
        }
        if (lane == 63)
            s_w[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kAlignWaves; ++w) {
            before += w < wave ? s_w[w] : 0;
            all += s_w[w];
        }
        if (i < n)
            item_off[base + i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        item_off[base + n] = carry;
        *n_total           = carry;
    }
    __syncthreads();
    for (int s = tid; s < n_seg; s += kAlignThreads)
        totals[s].n_items = item_off[off[s + 1]] - item_off[off[s]];
}

__global__ __launch_bounds__(64) void gather_rows_kernel(const float* __restrict__ src, long long src_ld, int dim, long long n, const int32_t* __restrict__ rows,
                                                         float* __restrict__ dst, long long dst_ld) {
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {
        const float* from = src + (long long)rows[i] * src_ld;
        float*       to   = dst + i * dst_ld;
        for (int d = threadIdx.x; d < dim; d += 64)
            to[d] = from[d];
    }
}

// what the Baum-Welch kernels need beyond the Viterbi plan: arcs by source and by label, and the segments' label tables
struct BwPlan {
    std::vector<BwSeg> bseg;
    std::vector<int>   out_off, lab_off, lab_val, lab_em;
    std::vector<BwArc> out_arc, lab_arc;
    long long          alpha_words = 0, surv_words = 0;
    int                max_labels  = 0;
};

inline int bw_plan(int n_seg, const amx_align_graphs* g, const AlignPlan& p, const char* who, BwPlan* b) {
    const int n_states = g->state_offsets[n_seg], n_arcs = g->arc_offsets[n_states];
    b->bseg.resize(n_seg);
    b->out_off.assign(g->arc_offsets, g->arc_offsets + n_states + 1);
    b->out_arc.resize(n_arcs), b->lab_arc.resize(n_arcs);
    b->lab_off.assign(1, 0);
    std::vector<int> labels, fill;
    for (int s = 0; s < n_seg; ++s) {
        const AlignSeg& sg = p.seg[s];
        const int       a0 = sg.in0, a1 = sg.in0 + sg.n_in;
        labels.assign(g->arc_label + a0, g->arc_label + a1);
        std::sort(labels.begin(), labels.end());
        labels.erase(std::unique(labels.begin(), labels.end()), labels.end());
        AMX_REQUIRE((int)labels.size() <= kBwMaxLabels, AMX_ERR_UNSUPPORTED, "%s: segment %d has %zu distinct labels, more than the limit of %d labels per segment",
                    who, s, labels.size(), kBwMaxLabels);
        BwSeg& bs   = b->bseg[s];
        bs.lab0     = (int)b->lab_val.size();
        bs.n_labels = (int)labels.size();
        bs.sw       = (sg.n_states + 63) / 64;
        bs.al0 = b->alpha_words, bs.sv0 = b->surv_words;
        b->alpha_words += ((long long)sg.frames + 1) * sg.n_states;
        b->surv_words += (long long)sg.frames * bs.sw;
        b->max_labels = std::max(b->max_labels, bs.n_labels);
        b->lab_val.insert(b->lab_val.end(), labels.begin(), labels.end());
        b->lab_em.resize(b->lab_val.size(), -1);
        fill.assign(labels.size() + 1, 0);
        for (int a = a0; a < a1; ++a) {
            const int l  = (int)(std::lower_bound(labels.begin(), labels.end(), g->arc_label[a]) - labels.begin());
            int&      em = b->lab_em[(size_t)bs.lab0 + l];
            AMX_REQUIRE(em < 0 || em == g->arc_emission[a], AMX_ERR_INVALID, "%s: segment %d: label %d has the emission indices %d and %d (arc_emission[%d])", who, s,
                        g->arc_label[a], em, g->arc_emission[a], a);
            em = g->arc_emission[a];
            int wbits;
            std::memcpy(&wbits, &g->arc_weight[a], sizeof wbits);
            b->out_arc[a] = make_int4(g->arc_target[a], p.arc_col[a], wbits, l);
            ++fill[l + 1];
        }
        // by label, within a label the by-target order of the plan
        const int base = a0;
        for (size_t l = 0; l < labels.size(); ++l) {
            fill[l + 1] += fill[l];
            b->lab_off.push_back(base + fill[l + 1]);
        }
        for (int i = 0; i < sg.n_states; ++i)
            for (int k = p.in_off[(size_t)sg.state0 + i]; k < p.in_off[(size_t)sg.state0 + i + 1]; ++k) {
                const AlignArc q = p.in_arc[k];
                const int      l = b->out_arc[q.w].w;
                b->lab_arc[(size_t)base + fill[l]++] = make_int4(q.x & 0xffff, i, q.y, q.z);
            }
    }
    return AMX_OK;
}

}  // namespace amx

struct amx_bw {
    amx_ctx*       ctx = nullptr;
    amx_bw_cfg     cfg{};
    amx::AlignPlan plan;   // of the last call: the uploads read them until the call's synchronisation
    amx::BwPlan    bplan;
    amx::DevBuf<amx::AlignSeg>       d_seg;
    amx::DevBuf<amx::BwSeg>          d_bseg;
    amx::DevBuf<long long>           d_off, d_n_total;
    amx::DevBuf<int>                 d_cols, d_in_off, d_out_off, d_lab_off, d_lab_val, d_lab_em, d_count;
    amx::DevBuf<amx::AlignArc>       d_in_arc;
    amx::DevBuf<amx::BwArc>          d_out_arc, d_lab_arc;
    amx::DevBuf<unsigned char>       d_is_final;
    amx::DevBuf<float>               d_final_w, d_cm;
    amx::DevBuf<unsigned long long>  d_surv;
    amx::DevBuf<double>              d_alpha, d_fw_total;
    amx::DevBuf<amx::BwSummary>      d_summary;
    amx::DevBuf<amx::BwTotals>       d_totals;
    std::vector<amx::BwSummary>      summary;
    std::vector<amx::BwTotals>       totals;
    // the item store
    amx::DevBuf<int32_t> s_frame, s_label, s_emission;
    amx::DevBuf<float>   s_weight;
    amx::DevBuf<double>  s_weight64;
    long long            capacity = 0, n_items = 0;
    bool                 lds_raised = false;
};

namespace amx {

static int bw_reserve_store(amx_bw* h, long long n) {
    if (n <= h->capacity)
        return AMX_OK;
    h->capacity = 0;
    AMX_TRY(h->s_frame.reserve((size_t)n));
    AMX_TRY(h->s_label.reserve((size_t)n));
    AMX_TRY(h->s_emission.reserve((size_t)n));
    AMX_TRY(h->s_weight.reserve((size_t)n));
    AMX_TRY(h->s_weight64.reserve((size_t)n));
    h->capacity = n;
    return AMX_OK;
}

}  // namespace amx

extern "C" {

void amx_bw_default_cfg(amx_bw_cfg* cfg) {
    if (!cfg)
        return;
    cfg->min_acoustic_pruning               = 50.f;      // Aligner.cc:473-496, as amx_align_default_cfg
    cfg->max_acoustic_pruning               = FLT_MAX;
    cfg->increment_factor                   = 2.f;
    cfg->min_average_number_of_states       = 0.0;
    cfg->increase_until_no_score_difference = 1;
    cfg->n_best_pruning                     = INT_MAX;
    cfg->score_scale                        = 1.f;
    cfg->min_weight                         = 0.f;   // paramMinWeight
    cfg->use_partial_sums                   = 0;     // paramUsePartialSums
}

int amx_bw_create(amx_ctx* ctx, const amx_bw_cfg* cfg, amx_bw** out) {
    const char* who = "amx_bw_create";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_REQUIRE(cfg, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_TRY(amx::align_check_search_cfg(who, cfg->min_acoustic_pruning, cfg->max_acoustic_pruning, cfg->increment_factor, cfg->min_average_number_of_states,
                                        cfg->n_best_pruning, cfg->score_scale));
    AMX_REQUIRE(cfg->use_partial_sums == 0 || cfg->use_partial_sums == 1, AMX_ERR_INVALID, "%s: use_partial_sums %d is neither 0 nor 1", who, cfg->use_partial_sums);
    AMX_REQUIRE(!cfg->use_partial_sums, AMX_ERR_UNSUPPORTED,
                "%s: use_partial_sums 1: weights that are not normalised over a frame are not built (the reference adds the total flow twice there)", who);
    AMX_REQUIRE(!std::isnan(cfg->min_weight) && cfg->min_weight >= 0.f, AMX_ERR_INVALID, "%s: min_weight %g must be a number that is not negative", who,
                (double)cfg->min_weight);
    AMX_REQUIRE(cfg->min_weight <= FLT_MIN, AMX_ERR_UNSUPPORTED,
                "%s: min_weight %g: pruning the posterior automaton (prunePosterior's f32 second stage) is not built; only 0 (off) is", who, (double)cfg->min_weight);
    std::unique_ptr<amx_bw> h(new amx_bw);
    h->ctx = ctx;
    h->cfg = *cfg;
    *out   = h.release();
    return AMX_OK;
}

void amx_bw_destroy(amx_bw* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

long long amx_bw_n_items(const amx_bw* h) { return h ? h->n_items : 0; }

int amx_bw_align_dev(amx_bw* h, int n_seg, const long* frame_offsets, const amx_align_graphs* graphs, const float* scores_dev, int scores_ld, int n_columns,
                     int64_t* item_offsets_dev, amx_bw_result* result, unsigned long long counters[3]) {
    const char* who = "amx_bw_align_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(n_seg >= 0 && n_columns >= 1 && scores_ld >= n_columns, AMX_ERR_INVALID, "%s: n_seg %d, scores_ld %d with %d columns", who, n_seg, scores_ld,
                n_columns);
    if (counters)
        counters[0] = counters[1] = counters[2] = 0;
    h->n_items = 0;
    if (n_seg == 0)
        return AMX_OK;
    AMX_REQUIRE(result, AMX_ERR_INVALID, "%s: NULL result", who);
    amx::AlignPlan& p = h->plan;
    amx::BwPlan&    b = h->bplan;
    p                 = amx::AlignPlan();
    b                 = amx::BwPlan();
    AMX_TRY(amx::align_plan(n_seg, frame_offsets, graphs, n_columns, who, &p));
    AMX_TRY(amx::bw_plan(n_seg, graphs, p, who, &b));
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(item_offsets_dev && (p.frames == 0 || scores_dev), AMX_ERR_INVALID, "%s: NULL buffer", who);
    AMX_REQUIRE(p.frames < (1ll << 31), AMX_ERR_UNSUPPORTED, "%s: %lld frames are more than one call takes", who, p.frames);
    // LDS of the three kernels, at the sizes of this batch
    const int    ls = p.max_states, lc = std::max(p.max_cols, 1), ll = std::max(b.max_labels, 1);
    int          lp2 = 1;
    while (lp2 < ll)
        lp2 <<= 1;
    const size_t lds_search   = ((size_t)ls * 16 + ((size_t)ls + 1) * 4 + (size_t)lc * 4 + 15) / 16 * 16;
    const size_t lds_forward  = ((size_t)ls * 16 + ((size_t)ls + 1) * 4 + (size_t)lc * 4 + 15) / 16 * 16;
    const size_t lds_count    = ((size_t)ls * 24 + (size_t)lp2 * 8 + (size_t)lc * 4 + 15) / 16 * 16;
    const size_t lds_write    = lds_count + (size_t)lp2 * 8;
    static_assert((size_t)amx::kAlignMaxStates * 24 + (size_t)amx::kBwMaxLabels * 16 + (size_t)amx::kAlignMaxCols * 4 <= amx::kAlignLdsBytes, "the limits fit into LDS");
    amx_ctx* ctx = h->ctx;
    AMX_HIP(hipSetDevice(ctx->device));
    if (lds_write > 48 * 1024 && !h->lds_raised) {
        AMX_HIP(hipFuncSetAttribute((const void*)amx::bw_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)amx::kAlignLdsBytes));
        AMX_HIP(hipFuncSetAttribute((const void*)amx::bw_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)amx::kAlignLdsBytes));
        AMX_HIP(hipFuncSetAttribute((const void*)amx::bw_backward_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)amx::kAlignLdsBytes));
        AMX_HIP(hipFuncSetAttribute((const void*)amx::bw_backward_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)amx::kAlignLdsBytes));
        h->lds_raised = true;
    }
    AMX_TRY(amx::align_upload(ctx, h->d_seg, p.seg));
    AMX_TRY(amx::align_upload(ctx, h->d_bseg, b.bseg));
    AMX_TRY(amx::align_upload(ctx, h->d_off, p.off));
    AMX_TRY(amx::align_upload(ctx, h->d_cols, p.cols));
    AMX_TRY(amx::align_upload(ctx, h->d_in_off, p.in_off));
    AMX_TRY(amx::align_upload(ctx, h->d_in_arc, p.in_arc));
    AMX_TRY(amx::align_upload(ctx, h->d_is_final, p.is_final));
    AMX_TRY(amx::align_upload(ctx, h->d_final_w, p.final_w));
    AMX_TRY(amx::align_upload(ctx, h->d_out_off, b.out_off));
    AMX_TRY(amx::align_upload(ctx, h->d_out_arc, b.out_arc));
    AMX_TRY(amx::align_upload(ctx, h->d_lab_off, b.lab_off));
    AMX_TRY(amx::align_upload(ctx, h->d_lab_arc, b.lab_arc));
    AMX_TRY(amx::align_upload(ctx, h->d_lab_val, b.lab_val));
    AMX_TRY(amx::align_upload(ctx, h->d_lab_em, b.lab_em));
    AMX_TRY(h->d_cm.reserve((size_t)std::max<long long>(p.cm_words, 1)));
    AMX_TRY(h->d_surv.reserve((size_t)std::max<long long>(b.surv_words, 1)));
    AMX_TRY(h->d_alpha.reserve((size_t)std::max<long long>(b.alpha_words, 1)));
    AMX_TRY(h->d_fw_total.reserve(n_seg));
    AMX_TRY(h->d_summary.reserve(n_seg));
    AMX_TRY(h->d_totals.reserve(n_seg));
    AMX_TRY(h->d_n_total.reserve(1));
    AMX_TRY(h->d_count.reserve((size_t)std::max<long long>(p.frames, 1)));
    AMX_TRY(amx::bw_reserve_store(h, std::max<long long>(h->capacity, 4 * p.frames + 64)));
    AMX_HIP(hipMemsetAsync(h->d_count.get(), 0, (size_t)std::max<long long>(p.frames, 1) * sizeof(int), ctx->stream));
    AMX_HIP(hipMemsetAsync(h->d_totals.get(), 0, (size_t)n_seg * sizeof(amx::BwTotals), ctx->stream));
    if (p.frames) {
        amx::ScopedKernelTimer timer(ctx, "bw_gather");
        hipLaunchKernelGGL(amx::align_gather_kernel, dim3((unsigned)p.frames), dim3(amx::kAlignThreads), 0, ctx->stream, scores_dev, (long long)scores_ld,
                           h->d_off.get(), n_seg, h->d_seg.get(), h->d_cols.get(), h->cfg.score_scale, h->d_cm.get());
        AMX_HIP(hipGetLastError());
    }
    {
        amx::BwSearchArgs a{};
        a.seg = h->d_seg.get(), a.bseg = h->d_bseg.get(), a.in_off = h->d_in_off.get(), a.in_arc = h->d_in_arc.get(), a.is_final = h->d_is_final.get();
        a.final_w = h->d_final_w.get(), a.cm = h->d_cm.get(), a.surv = h->d_surv.get(), a.summary = h->d_summary.get();
        a.loop = amx::AlignLoop{h->cfg.min_acoustic_pruning, h->cfg.max_acoustic_pruning, h->cfg.increment_factor, h->cfg.min_average_number_of_states,
                                h->cfg.increase_until_no_score_difference ? 1 : 0};
        a.lds_states = ls, a.lds_cols = lc;
        amx::ScopedKernelTimer timer(ctx, "bw_search");
        hipLaunchKernelGGL(amx::bw_search_kernel, dim3((unsigned)n_seg), dim3(amx::kAlignThreads), lds_search, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::BwForwardArgs a{};
        a.seg = h->d_seg.get(), a.bseg = h->d_bseg.get(), a.in_off = h->d_in_off.get(), a.in_arc = h->d_in_arc.get(), a.is_final = h->d_is_final.get();
        a.final_w = h->d_final_w.get(), a.cm = h->d_cm.get(), a.surv = h->d_surv.get(), a.summary = h->d_summary.get(), a.alpha = h->d_alpha.get();
        a.fw_total = h->d_fw_total.get(), a.lds_states = ls, a.lds_cols = lc;
        amx::ScopedKernelTimer timer(ctx, "bw_forward");
        hipLaunchKernelGGL(amx::bw_forward_kernel, dim3((unsigned)n_seg), dim3(amx::kAlignThreads), lds_forward, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    amx::BwBackwardArgs a{};
    a.seg = h->d_seg.get(), a.bseg = h->d_bseg.get(), a.out_off = h->d_out_off.get(), a.out_arc = h->d_out_arc.get(), a.lab_off = h->d_lab_off.get();
    a.lab_arc = h->d_lab_arc.get(), a.lab_val = h->d_lab_val.get(), a.lab_em = h->d_lab_em.get(), a.is_final = h->d_is_final.get(), a.final_w = h->d_final_w.get();
    a.cm = h->d_cm.get(), a.alpha = h->d_alpha.get(), a.summary = h->d_summary.get(), a.fw_total = h->d_fw_total.get(), a.totals = h->d_totals.get();
    a.count = h->d_count.get(), a.item_off = (const long long*)item_offsets_dev, a.n_total = h->d_n_total.get(), a.base = p.off[0];
    a.lds_states = ls, a.lds_cols = lc, a.lds_labels = lp2;
    {
        amx::ScopedKernelTimer timer(ctx, "bw_backward_count");
        hipLaunchKernelGGL(amx::bw_backward_kernel<false>, dim3((unsigned)n_seg), dim3(amx::kAlignThreads), lds_count, ctx->stream, a);
        AMX_HIP(hipGetLastError());
    }
    {
        amx::ScopedKernelTimer timer(ctx, "bw_scan");
        hipLaunchKernelGGL(amx::bw_scan_kernel, dim3(1), dim3(amx::kAlignThreads), 0, ctx->stream, h->d_count.get(), p.frames, p.off[0], (long long*)item_offsets_dev,
                           h->d_n_total.get(), h->d_off.get(), n_seg, h->d_totals.get());
        AMX_HIP(hipGetLastError());
    }
    auto write = [&]() -> int {
        a.capacity = h->capacity;
        a.o_frame = h->s_frame.get(), a.o_label = h->s_label.get(), a.o_emission = h->s_emission.get(), a.o_weight = h->s_weight.get();
        a.o_weight64 = h->s_weight64.get();
        amx::ScopedKernelTimer timer(ctx, "bw_backward_write");
        hipLaunchKernelGGL(amx::bw_backward_kernel<true>, dim3((unsigned)n_seg), dim3(amx::kAlignThreads), lds_write, ctx->stream, a);
        AMX_HIP(hipGetLastError());
        return AMX_OK;
    };
    AMX_TRY(write());
    h->summary.resize(n_seg), h->totals.resize(n_seg);
    long long n_total = 0;
    AMX_HIP(hipMemcpyAsync(h->summary.data(), h->d_summary.get(), (size_t)n_seg * sizeof(amx::BwSummary), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipMemcpyAsync(h->totals.data(), h->d_totals.get(), (size_t)n_seg * sizeof(amx::BwTotals), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipMemcpyAsync(&n_total, h->d_n_total.get(), sizeof n_total, hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    if (n_total > h->capacity) {   // the store was too small and nothing was written: grow it and write again
        AMX_TRY(amx::bw_reserve_store(h, n_total + n_total / 4));
        AMX_TRY(write());
        AMX_HIP(hipStreamSynchronize(ctx->stream));
    }
    h->n_items = n_total;
    for (int s = 0; s < n_seg; ++s) {
        const amx::BwSummary& r = h->summary[s];
        result[s].score = r.score, result[s].reached_final = r.reached, result[s].n_iterations = r.n_iterations;
        result[s].last_threshold = r.last_threshold, result[s].average_states = r.average, result[s].state_sum = r.sum;
        result[s].n_items   = h->totals[s].n_items;
        result[s].log_total = r.reached ? h->totals[s].log_total : amx::kBwDead;
        if (counters)
            counters[0] += r.nan ? 1 : 0, counters[1] += r.passes_run, counters[2] += r.passes_counted;
    }
    return AMX_OK;
}

int amx_bw_items_dev(amx_bw* h, long long capacity, int32_t* frame_dev, int32_t* label_dev, int32_t* emission_dev, float* weight_dev, double* weight_f64_dev) {
    const char* who = "amx_bw_items_dev";
    AMX_REQUIRE(h, AMX_ERR_INVALID, "%s: NULL handle", who);
    AMX_REQUIRE(capacity >= h->n_items, AMX_ERR_INVALID, "%s: capacity %lld is too small: the last call left %lld items", who, capacity, h->n_items);
    if (h->n_items == 0)
        return AMX_OK;
    AMX_REQUIRE(h->ctx, AMX_ERR_STATE, "%s: the handle was created without a context", who);
    AMX_REQUIRE(frame_dev && label_dev && emission_dev && weight_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    amx_ctx*     ctx = h->ctx;
    const size_t n   = (size_t)h->n_items;
    AMX_HIP(hipSetDevice(ctx->device));
    AMX_HIP(hipMemcpyAsync(frame_dev, h->s_frame.get(), n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(label_dev, h->s_label.get(), n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(emission_dev, h->s_emission.get(), n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    AMX_HIP(hipMemcpyAsync(weight_dev, h->s_weight.get(), n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    if (weight_f64_dev)
        AMX_HIP(hipMemcpyAsync(weight_f64_dev, h->s_weight64.get(), n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return AMX_OK;
}

int amx_gather_rows_dev(amx_ctx* ctx, const float* src_dev, int src_ld, int dim, long long n, const int32_t* row_dev, float* dst_dev, int dst_ld) {
    const char* who = "amx_gather_rows_dev";
    AMX_REQUIRE(ctx, AMX_ERR_INVALID, "%s: NULL context", who);
    AMX_REQUIRE(n >= 0 && dim >= 1 && src_ld >= dim && dst_ld >= dim, AMX_ERR_INVALID, "%s: n %lld, dim %d, src_ld %d, dst_ld %d", who, n, dim, src_ld, dst_ld);
    if (n == 0)
        return AMX_OK;
    AMX_REQUIRE(src_dev && row_dev && dst_dev, AMX_ERR_INVALID, "%s: NULL buffer", who);
    AMX_HIP(hipSetDevice(ctx->device));
    amx::ScopedKernelTimer timer(ctx, "gather_rows");
    hipLaunchKernelGGL(amx::gather_rows_kernel, dim3((unsigned)std::min<long long>(n, 1 << 20)), dim3(64), 0, ctx->stream, src_dev, (long long)src_ld, dim, n, row_dev,
                       dst_dev, (long long)dst_ld);
    AMX_HIP(hipGetLastError());
    return AMX_OK;
}

}  // extern "C"
