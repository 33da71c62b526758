// latplan.hip -- the plan of the lattice arc posteriors on the device (amx_latpost_cfg.plan = device, amx_latpost_plan_dev): what
// latpost_host.cpp's latpost_plan computes on one host thread, lattice after lattice, computed by one workgroup per lattice.
//
// latplan_kernel  one workgroup of kPlanThreads per lattice, ONE launch per call.  The steps are separated by workgroup barriers:
//   checks      all threads, over states and arcs; nothing below indexes with a value that has not passed them
//   peel        in-degrees by atomics, then a work list: what the list never reaches lies on or behind a cycle
//   discover    DfsState::dfs, the plan's one sequential chain, by wave 0: the discovered state's arcs 64 at a time, a ballot over "target
//               is white" and a popcount prefix give every pushed target its stack slot in arc order; a ballot over the top 64 stack
//               entries pops a whole run of black ones in one step
//   transpose   in-list lengths by atomics, a scan, and a STABLE placement: the arcs are enumerated discover-major (a scan of the discovered
//               states' degrees, a binary search per arc), 256 at a time; an arc's slot is its list's cursor plus the number of arcs
//               with the same target in front of it in its 256
//   levels      backward then forward, each a work list walked by wave 0: a state whose counter (targets / incoming arcs not yet done) falls
//               to zero is appended; a lane takes a listed state, PULLS its level from its finished neighbours and counts its
//               other neighbours down.  No workgroup barrier per level: a lattice has a few states per level and thousands of levels
//   tables      all threads: node_arcs by a scan, the walk arcs in the chain order of latpost_host.cpp, the nodes bucketed by level
// The per-state work arrays (colour / counters, cursors, the work list) live in LDS while the segment has at most kPlanLdsStates states,
// the stack while it has at most kPlanLdsStack entries (arcs + 1); above that they live in a global workspace.  The results are the same.
// Every loop has a bound that follows from the sizes; a loop that meets its bound stores a status and the workgroup returns.
#include <algorithm>
#include <chrono>

#include "common.hpp"
#include "latpost_plan.hpp"

namespace amx {

constexpr int kPlanThreads   = 256;
constexpr int kPlanLdsStates = 2048;   // x 3 arrays x 4 bytes: 24 KB of LDS
constexpr int kPlanLdsStack  = 8192;   // x 4 bytes: 32 KB of LDS
enum { kPlanRefused = 1, kPlanBound = 2 };

struct LatPlanArgs {
    // the call's raw tables
    const long *   state_offsets, *arc_offsets;
    const int32_t *arc_target, *initial;
    const float *  arc_weight, *arc_risk, *final_weight, *final_risk;
    const uint8_t* final_flag;
    // the walk tables
    LatWalk* walk;
    LatSeg*  seg;
    int32_t *node_arcs, *node_final, *warc_target, *order, *levels, *arc_source, *state_seg;
    float *  node_fw, *node_fr, *warc_weight, *warc_risk;
    // the plan's own outputs
    int32_t *discover_index, *level_backward, *level_forward, *level_super, *final_order, *in_off, *in_arc;
    // work: the discover list and the co-reached flags per state; per segment 3 n + m + 1 entries for what does not fit LDS
    int32_t *disc, *co, *work;
    int32_t *info, *status;
    long     n_arcs;
    int      expectation, has_final_weight;
};

// an exclusive scan over get(0 .. n) by the whole workgroup: put(i, sum of get(j < i)); returns the total.  part: kPlanThreads entries of LDS
template<class Get, class Put>
__device__ int plan_scan(int n, int* part, Get get, Put put) {
    const int tid = threadIdx.x, per = (n + kPlanThreads - 1) / kPlanThreads;
    const int b = tid * per < n ? tid * per : n, e = b + per < n ? b + per : n;
    int       sum = 0;
    for (int i = b; i < e; ++i)
        sum += get(i);
    part[tid] = sum;
    __syncthreads();
    int base = 0, total = 0;
    for (int j = 0; j < kPlanThreads; ++j) {
        const int v = part[j];
        base += j < tid ? v : 0;
        total += v;
    }
    __syncthreads();
    for (int i = b; i < e; ++i) {
        const int v = get(i);
        put(i, base);
        base += v;
    }
    return total;
}

// Wave 0 walks a work list: the entries [head, tail) that stand in the list at the start of a step are independent of each other (an entry
// is appended when its last neighbour has been visited), a lane takes one; visit(s) may append.  At most n entries, so at most n steps.
// Returns the number of entries visited, -1 when the bound was met.
template<class Visit>
__device__ int plan_walk(const int* queue, int* tail_p, int n, Visit visit) {
    const int lane = threadIdx.x & 63;
    int       head = 0;
    for (int step = 0; step <= n; ++step) {
        __threadfence_block();   // the last step's appends, levels and counters
        int tail = *(volatile int*)tail_p;
        tail     = tail < n ? tail : n;
        if (head >= tail)
            return head;
        if (head + lane < tail)
            visit(queue[head + lane]);
        head = head + 64 < tail ? head + 64 : tail;
    }
    return -1;
}

__global__ __launch_bounds__(kPlanThreads) void latplan_kernel(LatPlanArgs a) {
    __shared__ int32_t lds_state[3 * kPlanLdsStates];
    __shared__ int32_t lds_stack[kPlanLdsStack];
    __shared__ int32_t part[kPlanThreads];
    __shared__ int32_t keys[kPlanThreads];
    // tail of the work list, discovered states, their arcs, reached finals, largest backward level, the new initial state's level,
    // co-reached states, undefined arcs, the status that ends the workgroup
    __shared__ int32_t sh_tail, sh_ndisc, sh_reached_arcs, sh_nfinal, sh_maxback, sh_super, sh_co, sh_undef_arcs, sh_stop;

    const int  g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const bool wave0 = tid < 64, e = a.expectation != 0;
    const long s0 = a.state_offsets[g];   // the host has checked the state offsets: ascending, every segment with a state
    const int  n  = (int)(a.state_offsets[g + 1] - s0);

    // ---- checks: the segment's arc offsets, its initial state and its final weights; then, inside the checked range, its arcs
    const int ini = a.initial[g];
    int       bad = ini < 0 || ini >= n;
    for (int s = tid; s < n; s += kPlanThreads) {
        const long o0 = a.arc_offsets[s0 + s], o1 = a.arc_offsets[s0 + s + 1];
        bad |= o0 < 0 || o1 < o0 || o1 > a.n_arcs;
        if (a.final_flag[s0 + s]) {
            bad |= !a.has_final_weight || a.final_weight[s0 + s] != a.final_weight[s0 + s];
            bad |= e && a.final_risk[s0 + s] != a.final_risk[s0 + s];
        }
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0)
            atomicOr(a.status, kPlanRefused);
        return;
    }
    const long     a0  = a.arc_offsets[s0];
    const int      m   = (int)(a.arc_offsets[s0 + n] - a0);
    const int32_t* tgt = a.arc_target + a0;
    for (int k = tid; k < m; k += kPlanThreads) {
        bad |= tgt[k] < 0 || tgt[k] >= n || a.arc_weight[a0 + k] != a.arc_weight[a0 + k];
        bad |= e && a.arc_risk[a0 + k] != a.arc_risk[a0 + k];
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0)
            atomicOr(a.status, kPlanRefused);
        return;
    }
    auto off = [&](int s) { return (int)(a.arc_offsets[s0 + s] - a0); };   // a state's first arc, counted within the segment

    const bool states_in_lds = n <= kPlanLdsStates, stack_in_lds = m + 1 <= kPlanLdsStack;
    int32_t*   gwork = a.work + 3 * s0 + a0 + g;
    int32_t*   color = states_in_lds ? lds_state : gwork;                           // the walk's colours; later the levels' counters
    int32_t*   aux   = states_in_lds ? lds_state + kPlanLdsStates : gwork + n;      // in-degrees; later the in-lists' cursors
    int32_t*   queue = states_in_lds ? lds_state + 2 * kPlanLdsStates : gwork + 2 * n;   // the work list; the discover-major arc ranks
    int32_t*   stack = stack_in_lds ? lds_stack : gwork + 3 * n;
    int32_t *  disc = a.disc + s0, *co = a.co + s0, *didx = a.discover_index + s0, *lb = a.level_backward + s0, *lf = a.level_forward + s0;
    int32_t *  in_off = a.in_off + s0 + g, *in_arc = a.in_arc + a0, *src = a.arc_source + a0;
    const LatPlanBases B = latplan_bases(g, s0, n, a0, m);

    for (int s = tid; s < n; s += kPlanThreads) {
        color[s] = 0, aux[s] = 0, co[s] = 0, didx[s] = -1, lb[s] = -1, lf[s] = -1;
        a.final_order[s0 + s] = -1, a.state_seg[s0 + s] = g;
        for (int k = off(s), end = off(s + 1); k < end; ++k)
            src[k] = (int32_t)(s0 + s);
    }
    if (tid == 0)
        sh_tail = 0, sh_ndisc = 0, sh_reached_arcs = 0, sh_nfinal = 0, sh_maxback = -1, sh_super = -1, sh_co = 0, sh_undef_arcs = 0, sh_stop = 0;
    __syncthreads();
    auto append = [&](int s) {
        const int q = atomicAdd(&sh_tail, 1);
        if (q < n)
            queue[q] = s;
    };
    // every thread of the workgroup, after a barrier: a stop set by wave 0 ends the workgroup
    auto stopped = [&]() {
        if (sh_stop && tid == 0)
            atomicOr(a.status, sh_stop);
        return sh_stop != 0;
    };

    // ---- the peel of in-degrees over ALL states: what it does not place lies on or behind a cycle
    for (int k = tid; k < m; k += kPlanThreads)
        atomicAdd(&aux[tgt[k]], 1);
    __syncthreads();
    for (int s = tid; s < n; s += kPlanThreads)
        if (__hip_atomic_load(&aux[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            append(s);
    __syncthreads();
    if (wave0) {
        const int placed = plan_walk(queue, &sh_tail, n, [&](int s) {
            for (int k = off(s), end = off(s + 1); k < end; ++k)
                if (atomicSub(&aux[tgt[k]], 1) == 1)
                    append(tgt[k]);
        });
        if (lane == 0 && placed != n)
            sh_stop = placed < 0 ? kPlanBound : kPlanRefused;
    }
    __syncthreads();
    if (stopped())
        return;

    // ---- DfsState::dfs by wave 0: the discover order.  Every in-degree is back at zero: aux serves as the in-lists' counters next
    if (wave0) {
        const long bound = 2 * ((long)m + 1) + n;   // a state turns gray once, an entry is pushed (at most m + 1) and popped once
        int        sp = 1, nd = 0, reached_arcs = 0, stop = 0;
        if (lane == 0)
            stack[0] = ini;
        for (long step = 0; sp > 0 && !stop; ++step) {
            if (step > bound) {
                stop = kPlanBound;
                break;
            }
            __threadfence_block();   // the last step's pushes and colours
            const int top = stack[sp - 1], c = color[top];
            if (c == 0) {
                if (lane == 0)
                    color[top] = 1, didx[top] = nd, disc[nd] = top;
                ++nd;
                const int b = off(top), end = off(top + 1);
                reached_arcs += end - b;
                __threadfence_block();
                for (int k0 = b; k0 < end; k0 += 64) {
                    const int k = k0 + lane;
                    const int t = k < end ? tgt[k] : 0;
                    const bool white = k < end && color[t] == 0;   // white at this moment: a target can be pushed several times
                    const unsigned long long mask = __ballot(white);
                    const int                cnt  = __popcll(mask);
                    if (sp + cnt > m + 1) {
                        stop = kPlanBound;
                        break;
                    }
                    if (white)
                        stack[sp + __popcll(mask & ((1ull << lane) - 1))] = t;
                    sp += cnt;
                }
            }
            else {
                if (c == 1) {
                    if (lane == 0)
                        color[top] = 2;
                    --sp;
                    __threadfence_block();
                }
                if (sp > 0) {   // the run of black entries on top goes in one step
                    const int  i     = sp - 1 - lane;
                    const bool black = i >= 0 && color[stack[i]] == 2;
                    const unsigned long long rest = ~__ballot(black);
                    sp -= rest ? __ffsll((long long)rest) - 1 : 64;
                }
            }
        }
        if (lane == 0)
            sh_ndisc = nd, sh_reached_arcs = reached_arcs, sh_stop = stop;
    }
    __syncthreads();
    if (stopped())
        return;
    const int ndisc = sh_ndisc, R = sh_reached_arcs;

    // ---- the transposed lists: lengths, offsets, then the arcs in discover-major order, placed stably
    for (int k = tid; k < m; k += kPlanThreads)
        if (didx[src[k] - s0] >= 0)
            atomicAdd(&aux[tgt[k]], 1);
    __syncthreads();
    plan_scan(n, part, [&](int s) { return __hip_atomic_load(&aux[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
              [&](int s, int x) { in_off[s] = x, aux[s] = x; });
    if (tid == 0)
        in_off[n] = R;
    plan_scan(ndisc, part, [&](int j) { return off(disc[j] + 1) - off(disc[j]); }, [&](int j, int x) { queue[j] = x; });
    const int n_final = plan_scan(ndisc, part, [&](int j) { return (int)(a.final_flag[s0 + disc[j]] != 0); }, [&](int j, int x) {
        if (a.final_flag[s0 + disc[j]])
            a.final_order[s0 + x] = disc[j];
    });
    __syncthreads();
    for (int r0 = 0; r0 < R; r0 += kPlanThreads) {
        const int r = r0 + tid;
        int       key = -1, k = 0;
        if (r < R) {
            int lo = 0, hi = ndisc - 1;   // the last discovered state whose first rank is at or below r
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (queue[mid] <= r)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            k   = off(disc[lo]) + r - queue[lo];
            key = tgt[k];
        }
        keys[tid] = key;
        __syncthreads();
        int before = 0, after = 0;
        if (r < R) {
            for (int j = 0; j < kPlanThreads; ++j) {
                const bool same = keys[j] == key;
                before += same && j < tid;
                after |= same && j > tid;
            }
            in_arc[aux[key] + before] = (int32_t)(a0 + k);
        }
        __syncthreads();
        if (r < R && !after)
            aux[key] += before + 1;
        __syncthreads();
    }

    // ---- backward levels and co-reachability over the reached states, targets first
    const bool dead = n_final == 0;
    if (tid == 0)
        sh_tail = 0, sh_nfinal = n_final;
    __syncthreads();
    for (int s = tid; s < n; s += kPlanThreads)
        if (didx[s] >= 0) {
            color[s] = off(s + 1) - off(s);
            if (color[s] == 0)
                append(s);
        }
    __syncthreads();
    if (wave0) {
        const int done = plan_walk(queue, &sh_tail, n, [&](int s) {
            int level = 0, c = a.final_flag[s0 + s] != 0;
            for (int k = off(s), end = off(s + 1); k < end; ++k) {
                const int t = tgt[k];
                level       = lb[t] + 1 > level ? lb[t] + 1 : level;
                c |= co[t];
            }
            lb[s] = level, co[s] = c;
            for (int i = in_off[s], end = in_off[s + 1]; i < end; ++i) {
                const int u = src[in_arc[i] - a0] - (int)s0;
                if (atomicSub(&color[u], 1) == 1)
                    append(u);
            }
        });
        if (lane == 0 && done != ndisc)
            sh_stop = kPlanBound;
    }
    __syncthreads();
    if (stopped())
        return;
    for (int s = tid; s < n; s += kPlanThreads) {
        if (co[s])
            atomicAdd(&sh_co, 1);
        else
            atomicAdd(&sh_undef_arcs, off(s + 1) - off(s));
        if (lb[s] >= 0)
            atomicMax(&sh_maxback, lb[s]);
    }
    if (tid == 0)
        sh_tail = 0;
    __syncthreads();
    const int n_co = sh_co;

    // ---- forward levels over the co-reached states, sources first, along the transposed lists
    for (int s = tid; s < n; s += kPlanThreads)
        if (co[s]) {
            color[s] = in_off[s + 1] - in_off[s];
            if (color[s] == 0)
                append(s);
        }
    __syncthreads();
    if (wave0) {
        const int done = plan_walk(queue, &sh_tail, n, [&](int s) {
            int level = 0;
            for (int i = in_off[s], end = in_off[s + 1]; i < end; ++i) {
                const int lu = lf[src[in_arc[i] - a0] - s0];
                level        = lu + 1 > level ? lu + 1 : level;
            }
            lf[s] = level;
            if (a.final_flag[s0 + s])
                atomicMax(&sh_super, level + 1);
            for (int k = off(s), end = off(s + 1); k < end; ++k)
                if (co[tgt[k]] && atomicSub(&color[tgt[k]], 1) == 1)
                    append(tgt[k]);
        });
        if (lane == 0 && done != n_co)
            sh_stop = kPlanBound;
    }
    __syncthreads();
    if (stopped())
        return;
    const int super = dead ? -1 : sh_super;

    // ---- the two walks' tables
    for (int dir = 0; dir < 2; ++dir) {
        const int nb = dir == 0 ? B.node_fwd : B.node_bwd, wb = dir == 0 ? B.warc_fwd : B.warc_bwd, nn = n + (dir == 0);
        const int L  = dir == 0 ? (dead ? 0 : super + 1) : sh_maxback + 1;
        auto n_arcs_of = [&](int v) {
            if (dir == 1)
                return didx[v] >= 0 ? off(v + 1) - off(v) : 0;
            if (dead)
                return 0;
            return v == n ? n_final : (co[v] ? in_off[v + 1] - in_off[v] : 0);
        };
        const int total = plan_scan(nn, part, n_arcs_of, [&](int v, int x) { a.node_arcs[nb + v] = wb + x; });
        if (tid == 0)
            a.node_arcs[nb + nn] = wb + total;
        __syncthreads();
        for (int v = tid; v < nn; v += kPlanThreads) {
            int   w   = a.node_arcs[nb + v];
            bool  fin = false;
            float fw = 0.f, fr = 0.f;
            if (dir == 1 && didx[v] >= 0) {
                for (int k = off(v), end = off(v + 1); k < end; ++k, ++w)
                    a.warc_target[w] = tgt[k], a.warc_weight[w] = a.arc_weight[a0 + k], a.warc_risk[w] = e ? a.arc_risk[a0 + k] : 0.f;
                if (a.final_flag[s0 + v])
                    fin = true, fw = a.final_weight[s0 + v], fr = e ? a.final_risk[s0 + v] : 0.f;
            }
            else if (dir == 0 && !dead && v == n) {
                for (int i = 0; i < n_final; ++i, ++w) {
                    const int f      = a.final_order[s0 + i];
                    a.warc_target[w] = f, a.warc_weight[w] = a.final_weight[s0 + f], a.warc_risk[w] = e ? a.final_risk[s0 + f] : 0.f;
                }
            }
            else if (dir == 0 && !dead && co[v]) {
                for (int i = in_off[v], end = in_off[v + 1]; i < end; ++i, ++w) {
                    const int k      = in_arc[i] - (int)a0;
                    a.warc_target[w] = src[k] - (int32_t)s0, a.warc_weight[w] = a.arc_weight[a0 + k], a.warc_risk[w] = e ? a.arc_risk[a0 + k] : 0.f;
                }
                fin = v == ini;   // the semiring's one, in both automata
            }
            a.node_final[nb + v] = fin, a.node_fw[nb + v] = fw, a.node_fr[nb + v] = fr;
        }
        // the nodes by level, a level's wave-shared nodes behind its lane-taken ones.  Counts go two entries up, so that after the
        // inclusive scan entry key + 1 is the first slot of `key`; placing moves it to the first slot of key + 1, where the table wants it
        int32_t* lv  = a.levels + (dir == 0 ? B.level_fwd : B.level_bwd);
        auto key_of = [&](int v) {
            const int level = dir == 1 ? lb[v] : (dead ? -1 : (v == n ? super : lf[v]));
            return level < 0 || level >= L ? -1 : 2 * level + (n_arcs_of(v) >= kLatWaveArcs);
        };
        for (int i = tid; i < 2 * L + 2; i += kPlanThreads)
            lv[i] = 0;
        __syncthreads();
        for (int v = tid; v < nn; v += kPlanThreads)
            if (key_of(v) >= 0)
                atomicAdd(&lv[key_of(v) + 2], 1);
        __syncthreads();
        plan_scan(2 * L + 2, part, [&](int i) { return __hip_atomic_load(&lv[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
                  [&](int i, int x) { lv[i] = x + __hip_atomic_load(&lv[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
        __syncthreads();
        for (int v = tid; v < nn; v += kPlanThreads)
            if (key_of(v) >= 0)
                a.order[nb + atomicAdd(&lv[key_of(v) + 1], 1)] = v;
        if (tid == 0) {
            LatWalk w;
            w.node_base = nb, w.n_nodes = nn, w.order_base = nb, w.level_base = dir == 0 ? B.level_fwd : B.level_bwd, w.n_levels = L, w.pad = 0;
            a.walk[2 * g + dir] = w;
        }
        __syncthreads();
    }
    if (tid == 0) {
        LatSeg sg;
        sg.state0 = (int)s0, sg.initial = ini, sg.node_fwd = B.node_fwd, sg.node_bwd = B.node_bwd, sg.dead = dead, sg.n_states = n;
        a.seg[g]         = sg;
        a.level_super[g] = super;
        int32_t* info    = a.info + 8 * g;
        info[0] = dead ? AMX_LATPOST_NO_FINAL : AMX_LATPOST_OK, info[1] = ndisc, info[2] = R, info[3] = n_co, info[4] = n - n_co;
        info[5] = sh_undef_arcs, info[6] = dead ? 0 : super + 1, info[7] = sh_maxback + 1;
    }
}

// what the host checks before anything is uploaded: linear in n_seg.  false: the host plan names the offender
static bool latplan_uploadable(int mode, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target, const float* arc_weight,
                               const float* arc_risk, const int32_t* initial, const uint8_t* final_flag, const float* final_risk) {
    if (n_seg < 1 || !state_offsets || !arc_offsets || state_offsets[0] != 0 || arc_offsets[0] != 0)
        return false;
    for (int g = 0; g < n_seg; ++g)
        if (state_offsets[g + 1] <= state_offsets[g])
            return false;
    const long n_states = state_offsets[n_seg], n_arcs = arc_offsets[n_states];
    if (n_arcs < 0 || 2 * n_states + 2 * n_arcs + 2 * (long)n_seg >= (1l << 30) || !initial || !final_flag || (n_arcs > 0 && (!arc_target || !arc_weight)))
        return false;
    return mode != AMX_LATPOST_EXPECTATION || ((n_arcs == 0 || arc_risk) && final_risk);
}

int latplan_run(amx_ctx* ctx, int mode, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target,
                const float* arc_weight, const float* arc_risk, const int32_t* initial, const uint8_t* final_flag, const float* final_weight,
                const float* final_risk, const char* who, LatDevPlan* plan, LatArgs* args) {
    // the refusals are the host plan's: its status, its first offender, its wording
    auto refuse = [&]() {
        LatPlan   p;
        const int r = latpost_plan(mode, n_seg, state_offsets, arc_offsets, arc_target, arc_weight, arc_risk, initial, final_flag, final_weight, final_risk,
                                   who, &p);
        if (r == AMX_OK)
            set_error("%s: the device plan refused tables that the host plan accepts", who);
        return r == AMX_OK ? (int)AMX_ERR_DEVICE : r;
    };
    if (!latplan_uploadable(mode, n_seg, state_offsets, arc_offsets, arc_target, arc_weight, arc_risk, initial, final_flag, final_risk))
        return refuse();
    const bool   e  = mode == AMX_LATPOST_EXPECTATION;
    const size_t nG = (size_t)n_seg, nS = (size_t)state_offsets[n_seg], nA = (size_t)arc_offsets[nS];
    const size_t nN = 2 * nS + 3 * nG, nW = 2 * nA + nS, nL = 4 * nS + 10 * nG;
    AMX_HIP(hipSetDevice(ctx->device));

    // one table of 32-bit integers and one of floats; what the host fills stands in front
    size_t n_int = 0, n_flt = 0;
    auto   take  = [](size_t& at, size_t n) {
        const size_t r = at;
        at += n;
        return r;
    };
    const size_t i_tgt = take(n_int, nA), i_ini = take(n_int, nG), i_node_arcs = take(n_int, nN), i_node_final = take(n_int, nN), i_warc = take(n_int, nW);
    const size_t i_order = take(n_int, nN), i_levels = take(n_int, nL), i_src = take(n_int, nA), i_sseg = take(n_int, nS), i_didx = take(n_int, nS);
    const size_t i_lb = take(n_int, nS), i_lf = take(n_int, nS), i_super = take(n_int, nG), i_forder = take(n_int, nS), i_inoff = take(n_int, nS + nG);
    const size_t i_inarc = take(n_int, nA), i_disc = take(n_int, nS), i_co = take(n_int, nS), i_work = take(n_int, 3 * nS + nA + nG);
    const size_t i_info = take(n_int, 8 * nG), i_status = take(n_int, 1);
    const size_t f_aw = take(n_flt, nA), f_ar = take(n_flt, e ? nA : 0), f_fiw = take(n_flt, nS), f_fir = take(n_flt, e ? nS : 0);
    const size_t f_fw = take(n_flt, nN), f_fr = take(n_flt, nN), f_ww = take(n_flt, nW), f_wr = take(n_flt, nW);
    AMX_TRY(plan->ints.reserve(n_int));
    AMX_TRY(plan->floats.reserve(n_flt + 1));
    AMX_TRY(plan->offsets.reserve(nG + 1 + nS + 1));
    AMX_TRY(plan->final_flag.reserve(nS));
    AMX_TRY(plan->walk.reserve(2 * nG));
    AMX_TRY(plan->seg.reserve(nG));
    int32_t* di = plan->ints.get();
    float*   df = plan->floats.get();
    long*    dl = plan->offsets.get();

    const auto t0 = std::chrono::steady_clock::now();
    auto       up = [&](void* dst, const void* host, size_t bytes) {
        return bytes && host ? hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
    };
    AMX_HIP(up(dl, state_offsets, (nG + 1) * sizeof(long)));
    AMX_HIP(up(dl + nG + 1, arc_offsets, (nS + 1) * sizeof(long)));
    AMX_HIP(up(di + i_tgt, arc_target, nA * sizeof(int32_t)));
    AMX_HIP(up(di + i_ini, initial, nG * sizeof(int32_t)));
    AMX_HIP(up(df + f_aw, arc_weight, nA * sizeof(float)));
    AMX_HIP(up(df + f_fiw, final_weight, nS * sizeof(float)));
    if (e) {
        AMX_HIP(up(df + f_ar, arc_risk, nA * sizeof(float)));
        AMX_HIP(up(df + f_fir, final_risk, nS * sizeof(float)));
    }
    AMX_HIP(up(plan->final_flag.get(), final_flag, nS));
    AMX_HIP(hipMemsetAsync(di + i_status, 0, sizeof(int32_t), ctx->stream));
    const auto t1 = std::chrono::steady_clock::now();

    LatPlanArgs k{};
    k.state_offsets = dl, k.arc_offsets = dl + nG + 1, k.arc_target = di + i_tgt, k.initial = di + i_ini;
    k.arc_weight = df + f_aw, k.arc_risk = df + f_ar, k.final_weight = df + f_fiw, k.final_risk = df + f_fir, k.final_flag = plan->final_flag.get();
    k.walk = plan->walk.get(), k.seg = plan->seg.get();
    k.node_arcs = di + i_node_arcs, k.node_final = di + i_node_final, k.warc_target = di + i_warc, k.order = di + i_order, k.levels = di + i_levels;
    k.arc_source = di + i_src, k.state_seg = di + i_sseg;
    k.node_fw = df + f_fw, k.node_fr = df + f_fr, k.warc_weight = df + f_ww, k.warc_risk = df + f_wr;
    k.discover_index = di + i_didx, k.level_backward = di + i_lb, k.level_forward = di + i_lf, k.level_super = di + i_super, k.final_order = di + i_forder;
    k.in_off = di + i_inoff, k.in_arc = di + i_inarc, k.disc = di + i_disc, k.co = di + i_co, k.work = di + i_work;
    k.info = di + i_info, k.status = di + i_status;
    k.n_arcs = (long)nA, k.expectation = e, k.has_final_weight = final_weight != nullptr;
    {
        ScopedKernelTimer timer(ctx, "latpost_plan");
        hipLaunchKernelGGL(latplan_kernel, dim3((unsigned)n_seg), dim3(kPlanThreads), 0, ctx->stream, k);
        AMX_HIP(hipGetLastError());
    }
    int32_t status = 0;
    plan->h_seg.resize(nG), plan->h_info.resize(8 * nG);
    AMX_HIP(hipMemcpyAsync(&status, k.status, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipMemcpyAsync(plan->h_info.data(), k.info, 8 * nG * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipMemcpyAsync(plan->h_seg.data(), k.seg, nG * sizeof(LatSeg), hipMemcpyDeviceToHost, ctx->stream));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    plan->upload_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    plan->plan_ms   = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (status & kPlanBound) {
        set_error("%s: a loop of the device plan met its bound", who);
        return AMX_ERR_DEVICE;
    }
    if (status)
        return refuse();

    plan->n_seg = n_seg, plan->n_states = (long)nS, plan->n_arcs = (long)nA, plan->n_nodes = (long)nN;
    plan->discover_index = k.discover_index, plan->level_backward = k.level_backward, plan->level_forward = k.level_forward;
    plan->level_super = k.level_super, plan->final_order = k.final_order, plan->in_off = k.in_off, plan->in_arc = k.in_arc;
    if (args) {
        args->walk = k.walk, args->seg = k.seg;
        args->node_arcs = k.node_arcs, args->node_final = k.node_final, args->warc_target = k.warc_target, args->order = k.order, args->levels = k.levels;
        args->arc_source = k.arc_source, args->arc_target = k.arc_target, args->state_seg = k.state_seg;
        args->node_fw = k.node_fw, args->node_fr = k.node_fr, args->warc_weight = k.warc_weight, args->warc_risk = k.warc_risk;
        args->arc_weight = k.arc_weight, args->arc_risk = k.arc_risk, args->final_weight = k.final_weight, args->final_risk = k.final_risk;
        args->final_flag = k.final_flag, args->arc_offsets = k.arc_offsets;
        args->n_arcs = (long)nA, args->n_states = (long)nS, args->n_seg = n_seg;
    }
    return AMX_OK;
}

void latplan_info(const LatDevPlan& plan, amx_latpost_info* info) {
    for (int g = 0; g < plan.n_seg; ++g) {
        const int32_t* c = plan.h_info.data() + 8 * (size_t)g;
        info[g]          = amx_latpost_info{};
        info[g].reason = c[0], info[g].states_reached = c[1], info[g].arcs_reached = c[2], info[g].states_coreached = c[3];
        info[g].undefined_states = c[4], info[g].undefined_arcs = c[5], info[g].levels_forward = c[6], info[g].levels_backward = c[7];
    }
}

int latplan_download(amx_ctx* ctx, const LatDevPlan& plan, const long* state_offsets, const long* arc_offsets, int32_t* discover_index,
                     int32_t* level_backward, int32_t* level_forward, int32_t* level_super, long* in_offsets, int32_t* in_arc, int32_t* final_order,
                     amx_latpost_info* info) {
    const size_t nS = (size_t)plan.n_states, nA = (size_t)plan.n_arcs, nG = (size_t)plan.n_seg;
    auto down = [&](void* host, const void* dev, size_t bytes) {
        return host && bytes ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
    };
    std::vector<int32_t> off(in_offsets || in_arc ? nS + nG : 0), arcs(in_arc ? nA : 0);
    AMX_HIP(down(discover_index, plan.discover_index, nS * sizeof(int32_t)));
    AMX_HIP(down(level_backward, plan.level_backward, nS * sizeof(int32_t)));
    AMX_HIP(down(level_forward, plan.level_forward, nS * sizeof(int32_t)));
    AMX_HIP(down(level_super, plan.level_super, nG * sizeof(int32_t)));
    AMX_HIP(down(final_order, plan.final_order, nS * sizeof(int32_t)));
    AMX_HIP(down(off.empty() ? nullptr : off.data(), plan.in_off, off.size() * sizeof(int32_t)));
    AMX_HIP(down(arcs.empty() ? nullptr : arcs.data(), plan.in_arc, arcs.size() * sizeof(int32_t)));
    AMX_HIP(hipStreamSynchronize(ctx->stream));
    // the host plan's lists stand one behind the other; the device's stand at their segments' first arcs
    long base = 0;
    for (size_t g = 0; g < nG && !off.empty(); ++g) {
        const long     s0 = state_offsets[g], n = state_offsets[g + 1] - s0, a0 = arc_offsets[s0];
        const int32_t* o  = off.data() + s0 + g;
        if (in_offsets)
            for (long s = 0; s < n; ++s)
                in_offsets[s0 + s] = base + o[s];
        if (in_arc)
            std::copy(arcs.begin() + a0, arcs.begin() + a0 + o[n], in_arc + base);
        base += o[n];
    }
    if (in_offsets)
        in_offsets[nS] = base;
    if (info)
        latplan_info(plan, info);
    return AMX_OK;
}

}  // namespace amx

extern "C" void amx_latpost_plan_shape(int* threads, int* lds_states, int* lds_stack) {
    if (threads)
        *threads = amx::kPlanThreads;
    if (lds_states)
        *lds_states = amx::kPlanLdsStates;
    if (lds_stack)
        *lds_stack = amx::kPlanLdsStack;
}
