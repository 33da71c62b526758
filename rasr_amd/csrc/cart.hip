// cart.hip -- decision-tree state tying (include/amx.h, section "Decision-tree state tying"): Speech::FeatureAccumulator's examples on the
// device (Speech/DecisionTreeTrainer.cc:54-90) and Cart::DecisionTreeTrainer's Training (Cart/DecisionTreeTrainer.cc:353-801) with
// StateTyingDecisionTreeTrainer::LogLikelihoodGain (Speech/DecisionTreeTrainer.cc:134-250) as the scorer.
//
// Accumulation.  Per (label, component) the reference adds the frames in corpus order into an f64.  The frames of a call are ordered by
// label without any floating-point atomic: count per label (integer atomics), scan, then ONE workgroup walks the frames in order and
// gives every frame its place behind the earlier frames of its label (a rank among the 256 frames of its step plus a per-label cursor).
// The list of a label is therefore ascending by construction.  One wave per label then runs the chains, lane = component, continuing
// from what the buffer holds, four frames' loads ahead of the adds.
//
// Training.  The tree logic (node lists, question-id lists, the one-slot hypothesis manager, Core::PriorityQueue's heap moves, the leaf
// limit, rollback, numbering) runs on the host exactly as the reference writes it.  What the reference spends its time on -- per node
// and question the two f64 sums over the node's examples -- is cart_eval_kernel: a workgroup owns one node and a tile of questions,
// stages the node's example rows in LDS, and each lane keeps a left and a right accumulator for one (question, component), adding
// `bit ? v : +0.0` and `bit ? +0.0 : v` in list order.  An accumulator starts at +0.0 and can never become -0.0 (a sum is -0.0 only
// when both operands are), so adding +0.0 returns its own bits: the masked add equals skipping the example.  The same pass carries the
// u32 observation counts, truncated after every addition as the reference's `u32 += f64` does.
// The device's f64 log is not glibc's, so the kernel's gain is a screen: a question goes through the host's ::log (on the DEVICE's
// sums, never re-summed) unless the screen decides it by more than the margin; exact_all sends all.
// The library is compiled with -ffp-contract=off; mad<FMA> marks the sites the reference's -march=native build contracts.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <deque>

#include "common.hpp"

namespace amx {

constexpr int    kCartThreads   = 256;
constexpr int    kCartStageMax  = 64;          // example rows staged in LDS at most
constexpr int    kCartStageBytes = 32768;      // ... and their bytes
constexpr int    kCartMaxDim    = 1024;
constexpr int    kCartAhead     = 4;
constexpr double kCartLog2Pi    = 1.8378770664093453;   // ::log(PI + PI) of Speech/DecisionTreeTrainer.cc:106, :231: the f64 nearest to log(2 pi)
constexpr double kCartLogUlps   = 4.0;          // what the screen grants the device's log (documented: 1 ulp)
constexpr double kCartEps       = 2.220446049250313e-16;

// ---------------------------------------------------------------------------------------------------------------- accumulation

__global__ void cart_count_kernel(const int32_t* label, const double* weight, int T, int n_labels, int* count, unsigned* bad) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T)
        return;
    const int id = label[t];
    if (id == -1)
        return;
    if (id < 0 || id >= n_labels) {
        atomicMin(bad, (unsigned)t);
        return;
    }
    if (weight && weight[t] == 0.0)
        return;
    atomicAdd(&count[id], 1);
}

// start[l] = frames of the labels below l; cursor = start.  One workgroup.
__global__ __launch_bounds__(kCartThreads) void cart_scan_kernel(const int* count, int n_labels, int* start, int* cursor) {
    __shared__ int part[kCartThreads];
    const int tid = threadIdx.x;
    const int per = (n_labels + kCartThreads - 1) / kCartThreads;
    const int lo = tid * per < n_labels ? tid * per : n_labels, hi = lo + per < n_labels ? lo + per : n_labels;
    int       s  = 0;
    for (int l = lo; l < hi; ++l)
        s += count[l];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < kCartThreads; ++i) {
            const int v = part[i];
            part[i]     = run;
            run += v;
        }
    }
    __syncthreads();
    s = part[tid];
    for (int l = lo; l < hi; ++l) {
        start[l] = s, cursor[l] = s;
        s += count[l];
    }
    if (tid == kCartThreads - 1)
        start[n_labels] = s;
}

// One workgroup walks the frames in order, 256 per step: a frame's place is its label's cursor plus the number of earlier frames of the
// step with the same label; the last frame of a label in the step moves the cursor.  order[] is ascending within every label.
__global__ __launch_bounds__(kCartThreads) void cart_place_kernel(const int32_t* label, const double* weight, int T, int* cursor, int* order) {
    __shared__ int lab[kCartThreads];
    const int tid = threadIdx.x;
    for (int t0 = 0; t0 < T; t0 += kCartThreads) {
        const int t  = t0 + tid;
        int       id = -1;
        if (t < T) {
            id = label[t];
            if (id >= 0 && weight && weight[t] == 0.0)
                id = -1;
        }
        __syncthreads();   // the cursors of the step before are written, lab[] is free
        lab[tid] = id;
        __syncthreads();
        int  at   = -1;
        bool last = true;
        if (id >= 0) {
            int rank = 0;
            for (int j = 0; j < tid; ++j)
                rank += lab[j] == id;
            for (int j = tid + 1; j < kCartThreads; ++j)
                if (lab[j] == id) {
                    last = false;
                    break;
                }
            at = cursor[id] + rank;
        }
        __syncthreads();   // every frame of the step has read its cursor
        if (id >= 0) {
            order[at] = t;
            if (last)
                cursor[id] = at + 1;   // nobody else of this step writes it
        }
    }
}

// one wave per label, lane = component of the row [nObs, sum[dim], sumSq[dim]] (Speech/DecisionTreeTrainer.cc:74-89)
template<bool FMA>
__global__ __launch_bounds__(64) void cart_chain_kernel(const float* feats, long long stride, int dim, const double* weight, const int* start, const int* order,
                                                        double* acc) {
    const int l  = blockIdx.x;
    const int lo = start[l], hi = start[l + 1];
    if (lo == hi)
        return;
    const int R   = 1 + 2 * dim;
    double*   row = acc + (size_t)l * R;
    for (int c = threadIdx.x; c < R; c += 64) {
        const int  col = c == 0 ? 0 : (c - 1) % dim;
        const bool sq  = c > dim;
        double     a   = row[c];
        for (int i0 = lo; i0 < hi; i0 += kCartAhead) {
            float  x[kCartAhead];
            double w[kCartAhead];
#pragma unroll
            for (int k = 0; k < kCartAhead; ++k) {
                const int i = i0 + k < hi ? i0 + k : hi - 1;
                const int t = order[i];
                x[k]        = feats[(long long)t * stride + col];
                w[k]        = weight ? weight[t] : 1.0;
            }
#pragma unroll
            for (int k = 0; k < kCartAhead; ++k) {
                if (i0 + k >= hi)
                    break;
                if (c == 0)
                    a += w[k];                                     // example.nObs += w (:89)
                else if (!sq)
                    a = mad<FMA>((double)x[k], w[k], a);           // *itSum += (*itFeature) * w (:86)
                else
                    a = mad<FMA>((double)(x[k] * x[k]), w[k], a);  // the square is an f32 product (:87)
            }
        }
        row[c] = a;
    }
}

// ---------------------------------------------------------------------------------------------------------------- split search

struct CartTask {
    int       list0, n_ex;   // the node's examples: list[list0, list0 + n_ex)
    int       q0, n_q;       // the questions to evaluate: rows of the answer matrix qrows[q0, q0 + n_q)
    long long out0;          // item of the first of them
    double    father;        // node->score
};
struct CartBlock {
    int task, tile;
};
struct CartCount {
    unsigned l_obs, r_obs;   // SplitHypothesis::nLeftObs / nRightObs
    unsigned l_ex, r_ex;     // nLeftExamples / nRightExamples
};
struct CartEvalArgs {
    const CartTask*  tasks;
    const CartBlock* blocks;
    const int*       list;
    const int*       qrows;
    const double*    rows;      // [E x R]
    const uint32_t*  answers;   // [Q x words]
    int              words, R, dim, stage, tq;
    double           clip;
    CartCount*       cnt;       // [items]
    double*          screen;    // [items x 2]: the device's gain and its margin (nullable)
    double*          sums;      // [items x 2 x R]: left row, right row (nullable)
};

// LogLikelihoodGain::logLikelihood from the sums of a side (Speech/DecisionTreeTrainer.cc:219-232): s = [count, sum[dim], sumSq[dim]].
// abs_log (nullable): the sum of |log| over the components, what the screen's margin is made from.
// log of component d's clipped variance from a side's sums s = [count, sum[dim], sumSq[dim]] (Speech/DecisionTreeTrainer.cc:223-228)
template<bool FMA>
__host__ __device__ inline double cart_log_variance(const double* s, int d, int dim, double clip) {
    const double n   = s[0];
    const double mu  = s[1 + d] / n;                    // *itMu /= n
    double       var = s[1 + dim + d] / n;              // *itSigmaSquare /= n
    var              = mad<FMA>(-mu, mu, var);          // *itSigmaSquare -= (*itMu) * (*itMu)
    if (var < clip)
        var = clip;
    return log(var);
}

// (0.5 * n) * (d + d * ::log(PI + PI) + ll) (:231)
template<bool FMA>
__host__ __device__ inline double cart_close(double n, int dim, double ll) {
    const double D = (double)dim;
    return (0.5 * n) * (mad<FMA>(D, kCartLog2Pi, D) + ll);
}

template<bool FMA>
__host__ __device__ inline double cart_likelihood(const double* s, unsigned n_examples, int dim, double clip, double* abs_log) {
    if (abs_log)
        *abs_log = 0;
    if (n_examples == 0)
        return 0.0;                                         // begin == end (:137-138)
    double ll = 0.0, al = 0.0;
    for (int d = 0; d < dim; ++d) {
        const double lg = cart_log_variance<FMA>(s, d, dim, clip);
        ll += lg;                                           // ll += ::log(*itSigmaSquare), ascending
        al += fabs(lg);
    }
    if (abs_log)
        *abs_log = al;
    return cart_close<FMA>(s[0], dim, ll);
}

// what the screen grants a side: the two logs differ by at most kCartLogUlps ulps per component, the two chains round alike except where
// their inputs differ (one ulp of the running sum per step), and the closing product rounds twice
__host__ __device__ inline double cart_side_margin(double n, int dim, double abs_log, double value) {
    const double D = (double)dim;
    return 0.5 * fabs(n) * (kCartLogUlps + D + 4.0) * kCartEps * (abs_log + D * (1.0 + kCartLog2Pi)) + 4.0 * kCartEps * fabs(value);
}

template<bool FMA>
__global__ __launch_bounds__(kCartThreads) void cart_eval_kernel(CartEvalArgs p) {
    extern __shared__ double lds[];
    const CartBlock blk  = p.blocks[blockIdx.x];
    const CartTask  task = p.tasks[blk.task];
    const int       R = p.R, S = p.stage, TQ = p.tq, tid = threadIdx.x;
    double*         rows = lds;                          // [S x R]
    double*         sc   = lds + (size_t)S * R;          // [TQ x 2 x R]
    int*            sidx = (int*)(sc + (size_t)TQ * 2 * R);   // [S]
    unsigned*       sex  = (unsigned*)(sidx + S);             // [TQ x 2]: examples on the left, on the right
    for (int w0 = 0; w0 < TQ * R; w0 += kCartThreads) {  // one round unless a row is longer than the workgroup
        const int  w    = w0 + tid;
        const int  ql   = w / R, c = w % R;
        const int  qpos = blk.tile * TQ + ql;
        const bool active = w < TQ * R && qpos < task.n_q;
        const uint32_t* bits = p.answers + (size_t)(active ? p.qrows[task.q0 + qpos] : 0) * p.words;
        double   acc_l = 0.0, acc_r = 0.0;
        unsigned obs_l = 0, obs_r = 0, ex_l = 0, ex_r = 0;
        for (int s0 = 0; s0 < task.n_ex; s0 += S) {
            const int ns = task.n_ex - s0 < S ? task.n_ex - s0 : S;
            __syncthreads();   // the stage before has been read
            for (int i = tid; i < ns; i += kCartThreads)
                sidx[i] = p.list[task.list0 + s0 + i];
            __syncthreads();
            for (int i = tid; i < ns * R; i += kCartThreads)
                rows[i] = p.rows[(size_t)sidx[i / R] * R + i % R];
            __syncthreads();
            if (active)
                for (int e = 0; e < ns; ++e) {
                    const int    idx = sidx[e];
                    const bool   bit = (bits[idx >> 5] >> (idx & 31)) & 1u;
                    const double v   = rows[e * R + c];
                    acc_l += bit ? v : 0.0;
                    acc_r += bit ? 0.0 : v;
                    if (c == 0) {   // splitHyp.nLeftObs += nObs: a u32 that takes an f64 addition (Cart/DecisionTreeTrainer.cc:458, :462)
                        if (bit)
                            obs_l = (unsigned)((double)obs_l + v), ++ex_l;
                        else
                            obs_r = (unsigned)((double)obs_r + v), ++ex_r;
                    }
                }
        }
        if (active) {
            const long long item = task.out0 + qpos;
            if (p.sums) {
                p.sums[(size_t)item * 2 * R + c]     = acc_l;
                p.sums[(size_t)item * 2 * R + R + c] = acc_r;
            }
            sc[(size_t)ql * 2 * R + c]     = acc_l;
            sc[(size_t)ql * 2 * R + R + c] = acc_r;
            if (c == 0) {
                CartCount k;
                k.l_obs = obs_l, k.r_obs = obs_r, k.l_ex = ex_l, k.r_ex = ex_r;
                p.cnt[item] = k;
                sex[2 * ql] = ex_l, sex[2 * ql + 1] = ex_r;
            }
        }
    }
    __syncthreads();
    // the screen, on the sums the tile has just left in sc: every lane takes logarithms (question, side, component), then one lane per
    // question adds them up in ascending order
    if (!p.screen)
        return;
    const int nq = task.n_q - blk.tile * TQ < TQ ? task.n_q - blk.tile * TQ : TQ;
    double*   lg = rows;   // [TQ x 2 x dim]: the stage is no longer needed (TQ * 2 * dim < S * R for every dim)
    for (int w = tid; w < nq * 2 * p.dim; w += kCartThreads) {
        const int ql = w / (2 * p.dim), side = w / p.dim % 2, d = w % p.dim;
        lg[w]        = sex[2 * ql + side] ? cart_log_variance<FMA>(sc + ((size_t)ql * 2 + side) * R, d, p.dim, p.clip) : 0.0;
    }
    __syncthreads();
    if (tid < nq) {
        const double*   sl   = sc + (size_t)tid * 2 * R;
        const long long item = task.out0 + blk.tile * TQ + tid;
        double          v[2], m[2];
        for (int side = 0; side < 2; ++side) {
            const double* x  = lg + ((size_t)tid * 2 + side) * p.dim;
            double        ll = 0.0, al = 0.0;
            for (int d = 0; d < p.dim; ++d)
                ll += x[d], al += fabs(x[d]);
            v[side] = sex[2 * tid + side] ? cart_close<FMA>(sl[side * R], p.dim, ll) : 0.0;
            m[side] = cart_side_margin(sl[side * R], p.dim, al, v[side]);
        }
        p.screen[2 * item]     = task.father - (v[0] + v[1]);
        p.screen[2 * item + 1] = 2.0 * (m[0] + m[1]) + 8.0 * kCartEps * (fabs(v[0]) + fabs(v[1]) + fabs(task.father));
    }
}

// the shape of a launch for rows of R doubles
inline void cart_shape(int dim, int* stage, int* tq) {
    const int R = 1 + 2 * dim;
    int       s = kCartStageBytes / (R * (int)sizeof(double));
    *stage      = s < 1 ? 1 : s > kCartStageMax ? kCartStageMax : s;
    *tq         = kCartThreads / R < 1 ? 1 : kCartThreads / R;
}

// ---------------------------------------------------------------------------------------------------------------- the host's tree

constexpr unsigned kCartNoOrder = 0xffffffffu;

struct CartNode {   // Training::Node (Cart/DecisionTreeTrainer.cc:162-185)
    unsigned         depth = 0;
    double           score = 0;
    unsigned         n_obs = 0;
    std::vector<int> ex;
    int              question = -1;   // id among the questions of all steps run so far
    unsigned         order    = kCartNoOrder;
    CartNode *       left = nullptr, *right = nullptr;
};

struct CartSuggestion {   // what splitNode(node, questionIds, strict) finds: the hypothesis manager's one slot
    bool     done = false, has = false;
    size_t   qidid = 0;
    double   gain = 0, l_score = 0, r_score = 0;
    unsigned l_obs = 0, r_obs = 0, l_ex = 0, r_ex = 0;
    unsigned long long errors = 0;   // negative gains the reference reports while it looks
};

struct CartSplit {   // Training::Split (:298-319) and what has been looked up ahead of the queue for its children
    CartNode*        node;
    std::vector<int> qids;
    size_t           qidid;
    double           gain;
    bool             ahead = false;
    CartSuggestion   left_s, right_s;
    int question() const { return qids[qidid]; }
};

struct CartRequest {
    const CartNode*         node;
    const std::vector<int>* qids;
    CartSuggestion*         out;
};

// Core::PriorityQueue<Split*, SplitPtrGreaterThan> (Core/PriorityQueue.hh:55-108), move by move
struct CartQueue {
    std::vector<CartSplit*> heap{nullptr};
    static bool precedes(const CartSplit* a, const CartSplit* b) { return a->gain > b->gain; }
    size_t size() const { return heap.size() - 1; }
    bool   empty() const { return heap.size() == 1; }
    CartSplit* top() const { return heap[1]; }
    void insert(CartSplit* e) {
        heap.push_back(e);
        size_t i = size();
        while (i > 1 && !precedes(heap[i / 2], e)) {
            heap[i] = heap[i / 2];
            i /= 2;
        }
        heap[i] = e;
    }
    void pop() {
        heap[1] = heap[size()];
        heap.pop_back();
        if (size() > 0) {
            size_t     i = 1, j;
            CartSplit* e = heap[1];
            while (i <= size() / 2) {
                j = 2 * i;
                if (j < size() && precedes(heap[j + 1], heap[j]))
                    j = j + 1;
                if (!precedes(heap[j], e))
                    break;
                heap[i] = heap[j];
                i       = j;
            }
            heap[i] = e;
        }
    }
};

// Core::isAlmostEqualUlp(f32(gain), f32(0.0), 20) (Core/Utility.cc:61-73) for a negative gain
inline bool cart_almost_zero(double gain) {
    const float f = (float)gain;
    int32_t     i;
    std::memcpy(&i, &f, 4);
    if (i < 0)
        i = (int32_t)(0x80000000u - (uint32_t)i);
    const int64_t d = i < 0 ? -(int64_t)i : (int64_t)i;
    return d <= 20;
}

}  // namespace amx

struct amx_cart_tree {
    std::vector<amx_cart_node>   nodes;
    std::vector<int32_t>         classes;
    std::vector<amx_cart_commit> log;
    std::vector<amx_cart_qstat>  qstats;
    amx_cart_info                info{};
};

namespace amx {

struct CartTraining {
    amx_ctx*                ctx;
    const amx_cart_problem& pb;
    const amx_cart_plan&    plan;
    const bool              fma;
    const int               R, words;
    int                     stage, tq;
    std::vector<double>     rows;   // [E x R]
    DevBuf<double>          d_rows, d_screen, d_sums;
    DevBuf<uint32_t>        d_answers;
    DevBuf<int>             d_list, d_qrows;
    DevBuf<CartTask>        d_tasks;
    DevBuf<CartBlock>       d_blocks;
    DevBuf<CartCount>       d_cnt;

    std::deque<CartNode*>        nodes_;
    CartQueue                    splits_;
    std::vector<std::pair<int, int>> question_of;   // id -> (step, row)
    std::vector<amx_cart_qstat>  qstats;
    std::vector<amx_cart_commit> log;
    const amx_cart_step*         step_ = nullptr;
    double                       score_ = 0, gain_ = 0;
    unsigned                     n_obs_ = 0, n_number_ = 0, n_leaf_ = 0;
    unsigned long long           errors = 0, screened = 0, reevaluated = 0, launches = 0;
    std::vector<CartNode*>       all_nodes;   // owned
    std::vector<CartSplit*>      all_splits;  // owned

    CartTraining(amx_ctx* c, const amx_cart_problem& p, const amx_cart_plan& pl, bool fused)
            : ctx(c), pb(p), plan(pl), fma(fused), R(1 + 2 * p.dim), words((p.n_examples + 31) / 32) {
        cart_shape(p.dim, &stage, &tq);
    }
    virtual ~CartTraining() {
        for (CartNode* n : all_nodes)
            delete n;
        for (CartSplit* s : all_splits)
            delete s;
    }
    CartNode* new_node(unsigned depth, double score, unsigned n_obs) {
        CartNode* n = new CartNode;
        n->depth = depth, n->score = score, n->n_obs = n_obs;
        all_nodes.push_back(n);
        return n;
    }
    bool answer(int id, int example) const {
        const uint32_t* bits = pb.answers + (size_t)question_of[(size_t)id].second * words;
        return (bits[example >> 5] >> (example & 31)) & 1u;
    }
    double likelihood(const double* s, unsigned n_ex) const {
        return fma ? cart_likelihood<true>(s, n_ex, pb.dim, plan.variance_clipping, nullptr) : cart_likelihood<false>(s, n_ex, pb.dim, plan.variance_clipping, nullptr);
    }

    int upload() {
        rows.resize((size_t)pb.n_examples * R);
        for (int e = 0; e < pb.n_examples; ++e) {
            rows[(size_t)e * R] = pb.n_obs[e];
            std::memcpy(&rows[(size_t)e * R + 1], pb.values + (size_t)e * 2 * pb.dim, (size_t)2 * pb.dim * sizeof(double));
        }
        return upload_device();
    }
    // the two device-side seams (tests/host_cart_test.cc replaces them by plain loops to run the host's tree under the sanitizers)
    virtual int upload_device() {
        AMX_TRY(d_rows.upload(rows.data(), rows.size()));
        AMX_TRY(d_answers.upload(pb.answers, (size_t)pb.n_questions * words));
        return AMX_OK;
    }
    // counts, screen (nullable) and sums (nullable) of the listed (node, questions) pairs: one launch and its readback
    virtual int compute(const std::vector<CartTask>& tasks, const std::vector<int>& list, const std::vector<int>& qrows, long long items, CartCount* cnt,
                        double* screen, double* sums) {
        hipStream_t st = ctx->stream;
        AMX_TRY(launch(tasks, list, qrows, items, screen != nullptr, sums != nullptr));
        AMX_HIP(hipMemcpyAsync(cnt, d_cnt.get(), (size_t)items * sizeof(CartCount), hipMemcpyDeviceToHost, st));
        if (screen)
            AMX_HIP(hipMemcpyAsync(screen, d_screen.get(), (size_t)items * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (sums)
            AMX_HIP(hipMemcpyAsync(sums, d_sums.get(), (size_t)items * 2 * R * sizeof(double), hipMemcpyDeviceToHost, st));
        AMX_HIP(hipStreamSynchronize(st));
        return AMX_OK;
    }

    // one launch over the listed (node, questions) pairs
    int launch(const std::vector<CartTask>& tasks, const std::vector<int>& list, const std::vector<int>& qrows, long long items, bool want_screen, bool want_sums) {
        std::vector<CartBlock> blocks;
        for (size_t t = 0; t < tasks.size(); ++t)
            for (int tile = 0; tile * tq < tasks[t].n_q; ++tile)
                blocks.push_back(CartBlock{(int)t, tile});
        if (blocks.empty())
            return AMX_OK;
        hipStream_t st = ctx->stream;
        AMX_TRY(d_tasks.reserve(tasks.size()));
        AMX_TRY(d_blocks.reserve(blocks.size()));
        AMX_TRY(d_list.reserve(list.size()));
        AMX_TRY(d_qrows.reserve(qrows.size()));
        AMX_TRY(d_cnt.reserve((size_t)items));
        if (want_screen)
            AMX_TRY(d_screen.reserve((size_t)items * 2));
        if (want_sums)
            AMX_TRY(d_sums.reserve((size_t)items * 2 * R));
        AMX_HIP(hipMemcpyAsync(d_tasks.get(), tasks.data(), tasks.size() * sizeof(CartTask), hipMemcpyHostToDevice, st));
        AMX_HIP(hipMemcpyAsync(d_blocks.get(), blocks.data(), blocks.size() * sizeof(CartBlock), hipMemcpyHostToDevice, st));
        AMX_HIP(hipMemcpyAsync(d_list.get(), list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, st));
        AMX_HIP(hipMemcpyAsync(d_qrows.get(), qrows.data(), qrows.size() * sizeof(int), hipMemcpyHostToDevice, st));
        CartEvalArgs a{};
        a.tasks = d_tasks.get(), a.blocks = d_blocks.get(), a.list = d_list.get(), a.qrows = d_qrows.get();
        a.rows = d_rows.get(), a.answers = d_answers.get();
        a.words = words, a.R = R, a.dim = pb.dim, a.stage = stage, a.tq = tq, a.clip = plan.variance_clipping;
        a.cnt = d_cnt.get(), a.screen = want_screen ? d_screen.get() : nullptr, a.sums = want_sums ? d_sums.get() : nullptr;
        const size_t lds = ((size_t)stage * R + (size_t)tq * 2 * R) * sizeof(double) + ((size_t)stage + 2 * (size_t)tq) * sizeof(int);
        {
            ScopedKernelTimer timer(ctx, "cart_eval");
            if (fma)
                hipLaunchKernelGGL(cart_eval_kernel<true>, dim3((unsigned)blocks.size()), dim3(kCartThreads), lds, st, a);
            else
                hipLaunchKernelGGL(cart_eval_kernel<false>, dim3((unsigned)blocks.size()), dim3(kCartThreads), lds, st, a);
            AMX_HIP(hipGetLastError());
        }
        return AMX_OK;
    }

    // splitNode for every request (Cart/DecisionTreeTrainer.cc:397-524, strict): the sums on the device, the decisions here
    int evaluate(std::vector<CartRequest>& reqs) {
        const size_t cap_screen = (size_t)1 << 20, cap_sums = ((size_t)256 << 20) / ((size_t)2 * R * sizeof(double));
        size_t       r0 = 0;
        while (r0 < reqs.size()) {
            // a group of requests whose items fit a launch
            std::vector<size_t> group;
            size_t              items = 0;
            const size_t        cap = plan.exact_all ? cap_sums : cap_screen;
            while (r0 < reqs.size()) {
                CartRequest& q = reqs[r0];
                *q.out      = CartSuggestion();
                q.out->done = true;
                if (q.node->n_obs < (unsigned)(2u * step_->min_obs) || q.qids->empty()) {   // :398-399
                    ++r0;
                    continue;
                }
                if (!group.empty() && items + q.qids->size() > cap)
                    break;
                group.push_back(r0), items += q.qids->size();
                ++r0;
            }
            if (group.empty())
                continue;
            AMX_TRY(evaluate_group(reqs, group));
        }
        return AMX_OK;
    }

    int evaluate_group(std::vector<CartRequest>& reqs, const std::vector<size_t>& group) {
        std::vector<CartTask>  tasks;
        std::vector<int>       list, qrows;
        std::vector<CartCount> cnt;
        std::vector<double>    screen;
        std::vector<std::vector<int>> chosen(group.size());   // positions that go through the host's log, ascending
        std::vector<size_t>    first(group.size());           // a request's first item of the screen launch
        const double           thr = step_->min_gain > 0.0 ? step_->min_gain : 0.0;
        auto counts_pass = [&](const CartCount& k) {
            if (k.l_obs < step_->min_obs || k.r_obs < step_->min_obs)   // :471-472
                return false;
            return !(k.l_obs == 0 || k.r_obs == 0);                     // strict (:473-474)
        };
        if (!plan.exact_all) {
            long long items = 0;
            for (size_t g = 0; g < group.size(); ++g) {
                const CartRequest& q = reqs[group[g]];
                CartTask           t{};
                t.list0 = (int)list.size(), t.n_ex = (int)q.node->ex.size(), t.q0 = (int)qrows.size(), t.n_q = (int)q.qids->size();
                t.out0 = items, t.father = q.node->score;
                first[g] = (size_t)items;
                list.insert(list.end(), q.node->ex.begin(), q.node->ex.end());
                for (int id : *q.qids)
                    qrows.push_back(question_of[(size_t)id].second);
                items += t.n_q;
                tasks.push_back(t);
            }
            cnt.resize((size_t)items), screen.resize((size_t)items * 2);
            AMX_TRY(compute(tasks, list, qrows, items, cnt.data(), screen.data(), nullptr));
            ++launches;
            screened += (unsigned long long)items;
            // the contenders: every question the screen does not decide, and every one that may still be the largest
            for (size_t g = 0; g < group.size(); ++g) {
                const size_t nq = reqs[group[g]].qids->size();
                double       floor_best = -DBL_MAX;   // an exact gain that some question certainly reaches
                bool         any = false;
                for (size_t i = 0; i < nq; ++i) {
                    const size_t it = first[g] + i;
                    if (!counts_pass(cnt[it]))
                        continue;
                    const double gn = screen[2 * it], m = screen[2 * it + 1] > 1e-30 ? screen[2 * it + 1] : 1e-30;
                    if (gn - m > thr && gn - m > floor_best)
                        floor_best = gn - m, any = true;
                }
                for (size_t i = 0; i < nq; ++i) {
                    const size_t it = first[g] + i;
                    if (!counts_pass(cnt[it]))
                        continue;
                    const double gn = screen[2 * it], m = screen[2 * it + 1] > 1e-30 ? screen[2 * it + 1] : 1e-30;
                    const bool   negative = gn + m < 0.0;                          // fails, and the reference reports it
                    const bool   fails    = gn - m > 0.0 && gn + m < thr;          // fails silently
                    const bool   passes   = gn - m > thr;
                    const bool   beaten   = passes && any && gn + m < floor_best;  // passes, but another one is certainly larger
                    if (!(negative || fails || beaten))
                        chosen[g].push_back((int)i);
                }
            }
        }
        else
            for (size_t g = 0; g < group.size(); ++g) {
                chosen[g].resize(reqs[group[g]].qids->size());
                for (size_t i = 0; i < chosen[g].size(); ++i)
                    chosen[g][i] = (int)i;
            }
        // the listed pairs once more (exact_all: for the first time), this time for their sums
        std::vector<CartTask>  tasks2;
        std::vector<int>       list2, qrows2;
        std::vector<size_t>    first2(group.size());
        long long              items2 = 0;
        for (size_t g = 0; g < group.size(); ++g) {
            first2[g] = (size_t)items2;
            if (chosen[g].empty())
                continue;
            const CartRequest& q = reqs[group[g]];
            CartTask           t{};
            t.list0 = (int)list2.size(), t.n_ex = (int)q.node->ex.size(), t.q0 = (int)qrows2.size(), t.n_q = (int)chosen[g].size();
            t.out0 = items2, t.father = q.node->score;
            list2.insert(list2.end(), q.node->ex.begin(), q.node->ex.end());
            for (int i : chosen[g])
                qrows2.push_back(question_of[(size_t)(*q.qids)[(size_t)i]].second);
            items2 += t.n_q;
            tasks2.push_back(t);
        }
        std::vector<double>    sums;
        std::vector<CartCount> cnt2;
        if (items2) {
            // in pieces that fit the workspace
            const size_t cap_sums = ((size_t)256 << 20) / ((size_t)2 * R * sizeof(double));
            sums.resize((size_t)items2 * 2 * R), cnt2.resize((size_t)items2);
            size_t t0 = 0;
            while (t0 < tasks2.size()) {
                std::vector<CartTask> piece;
                long long             n = 0;
                const long long       base = tasks2[t0].out0;
                while (t0 < tasks2.size() && (piece.empty() || (size_t)(n + tasks2[t0].n_q) <= cap_sums)) {
                    CartTask t = tasks2[t0++];
                    t.out0 -= base;
                    n += t.n_q;
                    piece.push_back(t);
                }
                AMX_TRY(compute(piece, list2, qrows2, n, cnt2.data() + base, nullptr, sums.data() + (size_t)base * 2 * R));
                ++launches;
            }
            reevaluated += (unsigned long long)items2;
        }
        // the reference's loop over the questions of each node, in their order
        for (size_t g = 0; g < group.size(); ++g) {
            const CartRequest& q  = reqs[group[g]];
            CartSuggestion&    s  = *q.out;
            const size_t       nq = q.qids->size();
            size_t             k  = 0;   // next of chosen[g]
            for (size_t i = 0; i < nq; ++i) {
                const bool exact = k < chosen[g].size() && (size_t)chosen[g][k] == i;
                if (!exact) {
                    if (plan.exact_all)
                        continue;
                    const size_t it = first[g] + i;
                    if (counts_pass(cnt[it])) {
                        const double m = screen[2 * it + 1] > 1e-30 ? screen[2 * it + 1] : 1e-30;
                        if (screen[2 * it] + m < 0.0)
                            ++s.errors;
                    }
                    continue;
                }
                const size_t     it = first2[g] + k++;
                const CartCount& c  = cnt2[it];
                if (!counts_pass(c))
                    continue;
                const double* sl = &sums[it * 2 * R];
                const double  l  = likelihood(sl, c.l_ex), r = likelihood(sl + R, c.r_ex);
                const double  gain = q.node->score - (l + r);   // Speech/DecisionTreeTrainer.cc:246-249
                if (gain < 0.0) {                               // Cart/DecisionTreeTrainer.cc:479-483
                    if (!cart_almost_zero(gain))
                        ++s.errors;
                    continue;
                }
                if (gain < step_->min_gain)
                    continue;
                if (gain == 0.0)
                    continue;
                if (s.has && gain <= s.gain)                    // SplitHypothesesManager::push with one slot (:249-258)
                    continue;
                s.has = true, s.qidid = i, s.gain = gain, s.l_score = l, s.r_score = r;
                s.l_obs = c.l_obs, s.r_obs = c.r_obs, s.l_ex = c.l_ex, s.r_ex = c.r_ex;
            }
        }
        return AMX_OK;
    }

    // suggestSplit (:556-565); `pre` is the suggestion when it was looked up ahead
    int suggest(CartNode* node, std::vector<int>&& qids, const CartSuggestion* pre) {
        CartSuggestion s;
        if (pre && pre->done)
            s = *pre;
        else {
            std::vector<CartRequest> one{CartRequest{node, &qids, &s}};
            AMX_TRY(evaluate(one));
        }
        errors += s.errors;
        if (!s.has) {
            nodes_.push_back(node);
            return AMX_OK;
        }
        node->left  = new_node(node->depth + 1, s.l_score, s.l_obs);     // :494-516
        node->right = new_node(node->depth + 1, s.r_score, s.r_obs);
        node->left->ex.reserve(s.l_ex), node->right->ex.reserve(s.r_ex);
        const int id = qids[s.qidid];
        for (int e : node->ex)
            (answer(id, e) ? node->left : node->right)->ex.push_back(e);
        std::vector<int>().swap(node->ex);
        CartSplit* sp = new CartSplit{node, std::move(qids), s.qidid, s.gain};
        all_splits.push_back(sp);
        splits_.insert(sp);
        return AMX_OK;
    }

    void insert_split(CartSplit* sp) {   // :529-551
        gain_ += sp->gain;
        CartNode* node     = sp->node;
        node->question     = sp->question();
        node->left->order  = n_number_++;
        node->right->order = n_number_++;
        amx_cart_commit c{};
        c.node = (int)node->order, c.step = question_of[(size_t)node->question].first, c.row = question_of[(size_t)node->question].second;
        c.depth = node->depth, c.gain = sp->gain, c.total_gain = gain_;
        log.push_back(c);
        amx_cart_qstat& q = qstats[(size_t)node->question];
        ++q.count;
        q.sum_gain += sp->gain;
        q.min_gain = std::min(q.min_gain, sp->gain);
        q.max_gain = std::max(q.max_gain, sp->gain);
        q.sum_depth += node->depth;
        q.min_depth = std::min(q.min_depth, node->depth);
        q.max_depth = std::max(q.max_depth, node->depth);
    }

    // splitNode depends on the node's list, its question list and the step alone: the children of every queued split are looked up in
    // one launch, ahead of the queue (half splits: the right child only, the left one waits for the next step)
    int look_ahead(CartSplit* now, bool half) {
        std::vector<CartSplit*>       todo;
        std::vector<std::vector<int>> lists;
        if (!now->ahead)
            todo.push_back(now);
        for (size_t i = 1; i < splits_.heap.size(); ++i)
            if (!splits_.heap[i]->ahead)
                todo.push_back(splits_.heap[i]);
        lists.reserve(todo.size());
        std::vector<CartRequest> reqs;
        for (CartSplit* sp : todo) {
            std::vector<int> q = sp->qids;   // commitSplit's swap with the back (:575-576)
            q[sp->qidid]       = q.back();
            q.pop_back();
            lists.push_back(std::move(q));
        }
        for (size_t i = 0; i < todo.size(); ++i) {
            if (!half)
                reqs.push_back(CartRequest{todo[i]->node->left, &lists[i], &todo[i]->left_s});
            reqs.push_back(CartRequest{todo[i]->node->right, &lists[i], &todo[i]->right_s});
        }
        AMX_TRY(evaluate(reqs));
        for (CartSplit* sp : todo)
            sp->ahead = true;
        return AMX_OK;
    }

    int run_step(int step_index) {   // split() / halfSplit() (:622-676)
        const amx_cart_step& s = *step_;
        const int            base = (int)question_of.size();
        std::vector<int>     ids((size_t)s.n_questions);
        for (int i = 0; i < s.n_questions; ++i) {
            question_of.push_back({step_index, s.questions[i]});
            amx_cart_qstat q{};
            q.step = step_index, q.row = s.questions[i];
            q.min_gain = DBL_MAX, q.max_gain = -DBL_MAX;                 // Core::Type<f64>::max / ::min (:150-152)
            q.min_depth = 0xffffffffu, q.max_depth = 0;
            qstats.push_back(q);
            ids[(size_t)i] = base + i;
        }
        {   // every node of the step's start in one launch
            std::vector<CartSuggestion> pre(nodes_.size());
            std::vector<CartRequest>    reqs;
            for (size_t i = 0; i < nodes_.size(); ++i)
                reqs.push_back(CartRequest{nodes_[i], &ids, &pre[i]});
            AMX_TRY(evaluate(reqs));
            for (size_t i = nodes_.size(), k = 0; i > 0; --i, ++k) {
                CartNode* n = nodes_.front();
                nodes_.pop_front();
                AMX_TRY(suggest(n, std::vector<int>(ids), &pre[k]));
            }
        }
        const bool half = s.action != AMX_CART_SPLIT;
        while (!splits_.empty() && (unsigned long long)n_leaf_ + nodes_.size() + splits_.size() < (unsigned long long)plan.max_leaves) {
            CartSplit* sp = splits_.top();
            splits_.pop();
            if (!sp->ahead)
                AMX_TRY(look_ahead(sp, half));
            insert_split(sp);
            CartNode* node          = sp->node;
            sp->qids[sp->qidid]     = sp->qids.back();
            sp->qids.pop_back();
            if (!half) {   // commitSplit (:571-579)
                AMX_TRY(suggest(node->left, std::vector<int>(sp->qids), &sp->left_s));
                AMX_TRY(suggest(node->right, std::move(sp->qids), &sp->right_s));
            }
            else {         // commitHalfSplit (:586-594)
                AMX_TRY(suggest(node->right, std::move(sp->qids), &sp->right_s));
                if (s.action == AMX_CART_CLUSTER)
                    ++n_leaf_;
                else
                    nodes_.push_back(node->left);
            }
        }
        while (!splits_.empty()) {   // rollbackSplit (:599-614)
            CartSplit* sp = splits_.top();
            splits_.pop();
            CartNode* node = sp->node;
            node->ex       = std::move(node->left->ex);
            node->ex.insert(node->ex.end(), node->right->ex.begin(), node->right->ex.end());
            node->left = node->right = nullptr;
            nodes_.push_back(node);
        }
        return AMX_OK;
    }

    void commit_node(const CartNode* node, amx_cart_tree* tree, unsigned* n_cluster) {   // commitNode (:706-726)
        amx_cart_node& o = tree->nodes[node->order];
        o.depth = node->depth, o.n_obs = node->n_obs, o.score = node->score;
        if (node->left && node->right) {
            o.step = question_of[(size_t)node->question].first, o.row = question_of[(size_t)node->question].second;
            o.left = (int)node->left->order, o.right = (int)node->right->order, o.class_id = -1;
            // setChilds(commitNode(node->left), commitNode(node->right)): the order of the two calls is the compiler's, and the reference's
            // build (GCC) evaluates arguments from the right -- tests/golden/ref_cart.npz holds its class ids
            commit_node(node->right, tree, n_cluster);
            commit_node(node->left, tree, n_cluster);
        }
        else {
            o.step = o.row = o.left = o.right = -1;
            o.class_id = (int)(*n_cluster)++;
            for (int e : node->ex)
                tree->classes[(size_t)e] = o.class_id;
        }
    }

    int train(amx_cart_tree* tree) {
        AMX_TRY(upload());
        // init (:353-369)
        std::vector<double> total((size_t)R, 0.0);
        CartNode*           root = new_node(0, 0.0, 0);
        root->ex.resize((size_t)pb.n_examples);
        for (int e = 0; e < pb.n_examples; ++e) {
            root->ex[(size_t)e] = e;
            n_obs_              = (unsigned)((double)n_obs_ + pb.n_obs[e]);
            for (int c = 0; c < R; ++c)
                total[(size_t)c] += rows[(size_t)e * R + c];
        }
        score_      = likelihood(total.data(), (unsigned)pb.n_examples);
        root->score = score_, root->n_obs = n_obs_;
        root->order = n_number_++;
        // start (:678-704)
        nodes_.push_back(root);
        for (int i = 0; i < plan.n_steps && (unsigned long long)n_leaf_ + nodes_.size() < (unsigned long long)plan.max_leaves; ++i) {
            step_ = &plan.steps[i];
            AMX_TRY(run_step(i));
        }
        n_leaf_ += (unsigned)nodes_.size();
        nodes_.clear();
        // finish (:728-766)
        tree->nodes.assign((size_t)n_number_, amx_cart_node{});
        tree->classes.assign((size_t)pb.n_examples, -1);
        unsigned n_cluster = 0;
        commit_node(root, tree, &n_cluster);
        tree->log = std::move(log), tree->qstats = std::move(qstats);
        amx_cart_info& f = tree->info;
        f.n_nodes = (int)n_number_, f.n_leaves = (int)n_cluster, f.n_commits = (int)tree->log.size(), f.n_question_stats = (int)tree->qstats.size();
        f.n_examples = pb.n_examples, f.n_obs = n_obs_, f.initial_score = score_, f.total_gain = gain_;
        f.negative_gain_errors = errors, f.items_screened = screened, f.items_reevaluated = reevaluated, f.launches = launches;
        AMX_REQUIRE(n_cluster == n_leaf_, AMX_ERR_STATE, "amx_cart_train: %u leaves counted but %u numbered", n_leaf_, n_cluster);
        return AMX_OK;
    }
};

// the checks of amx_cart_train that need no device
static int cart_check(const amx_cart_problem* pb, const amx_cart_plan* plan, const char* who) {
    AMX_REQUIRE(pb && plan, AMX_ERR_INVALID, "%s: NULL problem or plan", who);
    AMX_REQUIRE(pb->n_examples >= 1, AMX_ERR_INVALID, "%s: n_examples %d must be at least 1", who, pb->n_examples);
    AMX_REQUIRE(pb->dim >= 1, AMX_ERR_INVALID, "%s: dim %d must be at least 1", who, pb->dim);
    AMX_REQUIRE(pb->dim <= kCartMaxDim, AMX_ERR_UNSUPPORTED, "%s: dim %d is above the limit of %d components", who, pb->dim, kCartMaxDim);
    AMX_REQUIRE(pb->n_questions >= 0, AMX_ERR_INVALID, "%s: n_questions %d is negative", who, pb->n_questions);
    AMX_REQUIRE(pb->n_obs && pb->values, AMX_ERR_INVALID, "%s: NULL n_obs or values", who);
    AMX_REQUIRE(pb->n_questions == 0 || pb->answers, AMX_ERR_INVALID, "%s: NULL answers", who);
    AMX_REQUIRE(plan->n_steps >= 0 && (plan->n_steps == 0 || plan->steps), AMX_ERR_INVALID, "%s: n_steps %d or NULL steps", who, plan->n_steps);
    AMX_REQUIRE(plan->variance_clipping == plan->variance_clipping, AMX_ERR_INVALID, "%s: variance_clipping is not a number", who);
    double total = 0;
    for (int e = 0; e < pb->n_examples; ++e) {
        AMX_REQUIRE(pb->n_obs[e] >= 0 && pb->n_obs[e] <= DBL_MAX, AMX_ERR_INVALID, "%s: n_obs[%d] = %g must be at least 0 and finite", who, e, pb->n_obs[e]);
        total += pb->n_obs[e];
    }
    AMX_REQUIRE(total < 4294967296.0, AMX_ERR_UNSUPPORTED, "%s: %g observations in all: the reference counts them in 32 bits", who, total);
    for (int i = 0; i < plan->n_steps; ++i) {
        const amx_cart_step& s = plan->steps[i];
        AMX_REQUIRE(s.action == AMX_CART_SPLIT || s.action == AMX_CART_PARTITION || s.action == AMX_CART_CLUSTER, AMX_ERR_INVALID,
                    "%s: step %d: unknown action %d", who, i, s.action);
        AMX_REQUIRE(s.randomize >= 1, AMX_ERR_INVALID, "%s: step %d: randomize %d must be at least 1", who, i, s.randomize);
        AMX_REQUIRE(s.randomize == 1, AMX_ERR_UNSUPPORTED, "%s: step %d: randomize %d: the reference seeds the choice with the time of day", who, i, s.randomize);
        AMX_REQUIRE(s.min_gain == s.min_gain, AMX_ERR_INVALID, "%s: step %d: min_gain is not a number", who, i);
        AMX_REQUIRE(s.n_questions >= 0 && (s.n_questions == 0 || s.questions), AMX_ERR_INVALID, "%s: step %d: n_questions %d or NULL questions", who, i, s.n_questions);
        for (int k = 0; k < s.n_questions; ++k)
            AMX_REQUIRE(s.questions[k] >= 0 && s.questions[k] < pb->n_questions, AMX_ERR_INVALID, "%s: step %d: questions[%d] = %d of %d rows", who, i, k,
                        s.questions[k], pb->n_questions);
    }
    return AMX_OK;
}

}  // namespace amx

extern "C" {

size_t amx_cart_accumulator_size(int n_labels, int dim) {
    if (n_labels < 0 || dim < 1)
        return 0;
    return (size_t)n_labels * (1 + 2 * (size_t)dim);
}

int amx_cart_accumulate_dev(amx_ctx* ctx, const float* feats_dev, int feats_stride, int dim, int T, const int32_t* label_dev, const double* weight_dev,
                            int n_labels, double* acc_dev) {
    const char* who = "amx_cart_accumulate_dev";
    AMX_REQUIRE(ctx, AMX_ERR_INVALID, "%s: NULL context", who);
    AMX_REQUIRE(dim >= 1 && feats_stride >= dim, AMX_ERR_INVALID, "%s: dim %d, feats_stride %d", who, dim, feats_stride);
    AMX_REQUIRE(T >= 0 && n_labels >= 1, AMX_ERR_INVALID, "%s: T %d, n_labels %d", who, T, n_labels);
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(feats_dev && label_dev && acc_dev, AMX_ERR_INVALID, "%s: NULL feats_dev, label_dev or acc_dev", who);
    AMX_HIP(hipSetDevice(ctx->device));
    hipStream_t  st    = ctx->stream;
    // workspace: count[n_labels] start[n_labels + 1] cursor[n_labels] order[T] bad[1]
    const size_t words = 3 * (size_t)n_labels + 1 + (size_t)T + 1;
    AMX_TRY(ctx->scratch.reserve(words * sizeof(int)));
    int*      count  = (int*)ctx->scratch.get();
    int*      start  = count + n_labels;
    int*      cursor = start + n_labels + 1;
    int*      order  = cursor + n_labels;
    unsigned* bad    = (unsigned*)(order + T);
    AMX_HIP(hipMemsetAsync(count, 0, (size_t)n_labels * sizeof(int), st));
    AMX_HIP(hipMemsetAsync(bad, 0xff, sizeof(unsigned), st));
    // 1. labels, checked before anything is written
    hipLaunchKernelGGL(amx::cart_count_kernel, dim3((unsigned)amx::ceil_div(T, 256)), dim3(256), 0, st, label_dev, weight_dev, T, n_labels, count, bad);
    AMX_HIP(hipGetLastError());
    unsigned h_bad = 0;
    AMX_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    AMX_HIP(hipStreamSynchronize(st));
    if (h_bad != 0xffffffffu) {
        int32_t id = 0;
        AMX_HIP(hipMemcpy(&id, label_dev + h_bad, sizeof(id), hipMemcpyDeviceToHost));
        amx::set_error("%s: frame %u: label %d is outside [0, %d) and is not -1", who, h_bad, id, n_labels);
        return AMX_ERR_INVALID;
    }
    // 2. every label's frames in ascending order, 3. the chains
    hipLaunchKernelGGL(amx::cart_scan_kernel, dim3(1), dim3(amx::kCartThreads), 0, st, (const int*)count, n_labels, start, cursor);
    hipLaunchKernelGGL(amx::cart_place_kernel, dim3(1), dim3(amx::kCartThreads), 0, st, label_dev, weight_dev, T, cursor, order);
    AMX_HIP(hipGetLastError());
    {
        amx::ScopedKernelTimer timer(ctx, "cart_accumulate");
        if (ctx->contract == AMX_CONTRACT_FMA)
            hipLaunchKernelGGL(amx::cart_chain_kernel<true>, dim3((unsigned)n_labels), dim3(64), 0, st, feats_dev, (long long)feats_stride, dim, weight_dev,
                               (const int*)start, (const int*)order, acc_dev);
        else
            hipLaunchKernelGGL(amx::cart_chain_kernel<false>, dim3((unsigned)n_labels), dim3(64), 0, st, feats_dev, (long long)feats_stride, dim, weight_dev,
                               (const int*)start, (const int*)order, acc_dev);
        AMX_HIP(hipGetLastError());
    }
    AMX_HIP(hipStreamSynchronize(st));   // the workspace is the context's
    return AMX_OK;
}

void amx_cart_kernel_shape(int dim, int* stage_examples, int* tile_questions) {
    int s = 0, q = 0;
    if (dim >= 1 && dim <= amx::kCartMaxDim)
        amx::cart_shape(dim, &s, &q);
    if (stage_examples)
        *stage_examples = s;
    if (tile_questions)
        *tile_questions = q;
}

int amx_cart_train(amx_ctx* ctx, const amx_cart_problem* problem, const amx_cart_plan* plan, amx_cart_tree** out) {
    const char* who = "amx_cart_train";
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    AMX_TRY(amx::cart_check(problem, plan, who));
    AMX_REQUIRE(ctx, AMX_ERR_STATE, "%s: no context: the checks passed, the search needs a device", who);
    AMX_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<amx_cart_tree> tree(new amx_cart_tree);
    amx::CartTraining              t(ctx, *problem, *plan, ctx->contract == AMX_CONTRACT_FMA);
    AMX_TRY(t.train(tree.get()));
    *out = tree.release();
    return AMX_OK;
}

void amx_cart_tree_destroy(amx_cart_tree* tree) {
    delete tree;
}

int amx_cart_tree_info(const amx_cart_tree* tree, amx_cart_info* info) {
    AMX_REQUIRE(tree && info, AMX_ERR_INVALID, "amx_cart_tree_info: NULL argument");
    *info = tree->info;
    return AMX_OK;
}

int amx_cart_tree_get(const amx_cart_tree* tree, amx_cart_node* nodes, int32_t* classes, amx_cart_commit* log, amx_cart_qstat* question_stats) {
    AMX_REQUIRE(tree, AMX_ERR_INVALID, "amx_cart_tree_get: NULL tree");
    if (nodes)
        std::copy(tree->nodes.begin(), tree->nodes.end(), nodes);
    if (classes)
        std::copy(tree->classes.begin(), tree->classes.end(), classes);
    if (log)
        std::copy(tree->log.begin(), tree->log.end(), log);
    if (question_stats)
        std::copy(tree->qstats.begin(), tree->qstats.end(), question_stats);
    return AMX_OK;
}

}  // extern "C"
