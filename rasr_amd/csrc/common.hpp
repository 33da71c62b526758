// common.hpp -- internals shared by the librasr_amd.so translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/amx.h"

namespace amx {

void set_error(const char* fmt, ...);

#define AMX_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            amx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return AMX_ERR_DEVICE;                                                             \
        }                                                                                      \
    } while (0)

#define AMX_REQUIRE(cond, status, ...)   \
    do {                                 \
        if (!(cond)) {                   \
            amx::set_error(__VA_ARGS__); \
            return (status);             \
        }                                \
    } while (0)

#define AMX_TRY(expr)       \
    do {                    \
        int r__ = (expr);   \
        if (r__ != AMX_OK)  \
            return r__;     \
    } while (0)

// An owning device buffer: a pointer and its capacity in elements (Pinned: page-locked host memory instead).  Nothing is allocated
// until upload / reserve, and the destructor of an empty buffer makes no HIP call (host-only handles).
template<class T, bool Pinned = false>
class DevBuf {
    T*     p_   = nullptr;
    size_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&)            = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept
            : p_(o.p_), cap_(o.cap_) {
        o.p_   = nullptr;
        o.cap_ = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_, cap_ = o.cap_;
            o.p_   = nullptr;
            o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    T*     get() const { return p_; }
    size_t capacity() const { return cap_; }
    void   release() {
        if (p_)
            Pinned ? hipHostFree(p_) : hipFree(p_);
        p_   = nullptr;
        cap_ = 0;
    }
    // AMX_OK at once when the capacity suffices; otherwise the old memory is freed (its contents are not kept) and exactly n
    // elements are allocated -- the workspaces are sized to what a call needs.  On failure the buffer is empty.
    int reserve(size_t n) {
        if (n <= cap_)
            return AMX_OK;
        release();
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p_, n * sizeof(T)) : hipMalloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            amx::set_error("allocation of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
            return AMX_ERR_DEVICE;
        }
        cap_ = n;
        return AMX_OK;
    }
    // a fresh allocation of max(n, 1) elements holding host[0, n)
    int upload(const T* host, size_t n) {
        release();
        AMX_TRY(reserve(n > 1 ? n : 1));
        if (n)
            AMX_HIP(hipMemcpy(p_, host, n * sizeof(T), hipMemcpyHostToDevice));
        return AMX_OK;
    }
};

// Per-kernel event timing (amx_profile_*): pairs of events recorded around a launch on the
// context's current stream; resolved lazily in amx_profile_get.
struct ProfileSlot {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    double                                          total_ms = 0;
    long                                            n        = 0;
};

}  // namespace amx

struct amx_ctx {
    int                                      device     = 0;
    hipStream_t                              own_stream = nullptr;
    hipStream_t                              stream     = nullptr;
    bool                                     profiling  = false;
    std::map<std::string, amx::ProfileSlot>  prof;
    int                                      n_cu = 0;
    int                                      contract = AMX_CONTRACT_OFF;   // amx_set_contract: which build of the reference the f32 arithmetic follows
    amx::DevBuf<char> scratch;   // amx_gather_scores: index pairs up, scores down
};

namespace amx {

// RAII-less helper: records start/stop events around a launch when profiling is on.
struct ScopedKernelTimer {
    amx_ctx*    ctx;
    const char* name;
    hipEvent_t  a = nullptr, b = nullptr;
    ScopedKernelTimer(amx_ctx* c, const char* n)
            : ctx(c), name(n) {
        if (ctx->profiling) {
            hipEventCreate(&a);
            hipEventCreate(&b);
            hipEventRecord(a, ctx->stream);
        }
    }
    ~ScopedKernelTimer() {
        if (a) {
            hipEventRecord(b, ctx->stream);
            ctx->prof[name].events.emplace_back(a, b);
        }
    }
};

// Small-batch passes on unchanged device buffers (the decoder's ring buffer), recorded once and replayed as HIP graphs: the tuning
// option graph=1 of amx_gmm_model and amx_ffnn_model (default 0: every pass is launched plainly).  Key is what a handle's pass depends
// on (buffers, stream, sizes).  A recorded pass holds the addresses of the handle's workspaces, so whoever moves one of those calls
// clear() first.
template<class Key>
struct GraphCache {
    enum Ran { kPlain, kRecorded, kReplayed };
    std::map<Key, hipGraphExec_t> graphs;
    int                           use_graphs = 0;
    GraphCache() = default;
    GraphCache(const GraphCache&)            = delete;
    GraphCache& operator=(const GraphCache&) = delete;
    ~GraphCache() { clear(); }
    void clear() {
        for (auto& kv : graphs)
            if (kv.second)
                hipGraphExecDestroy(kv.second);
        graphs.clear();
    }
    // pass(capturing) enqueues the launches.  First call with a key: plain (it sizes the workspaces) and remembered; second call:
    // captured, instantiated and launched; later calls: launched.  A caller that never repeats a signature (64 of them) or a
    // stream that cannot capture switches graphs off.  *ran tells the caller which statistics the pass itself has kept.
    template<class Pass>
    int run(const Key& key, hipStream_t stream, Pass&& pass, Ran* ran) {
        *ran    = kPlain;
        auto it = graphs.find(key);
        if (it == graphs.end()) {
            if (graphs.size() >= 64) {
                clear();
                use_graphs = 0;
            }
            else
                graphs[key] = nullptr;
            return pass(false);
        }
        hipGraphExec_t ex = it->second;
        if (ex)
            *ran = kReplayed;
        else {
            hipGraph_t g = nullptr;
            if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
                (void)hipGetLastError();
                use_graphs = 0;
                return pass(false);
            }
            const int  r  = pass(true);
            const bool ok = hipStreamEndCapture(stream, &g) == hipSuccess && r == AMX_OK && g != nullptr;
            if (!ok || hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
                (void)hipGetLastError();
                if (g)
                    hipGraphDestroy(g);
                use_graphs = 0;
                return pass(false);
            }
            hipGraphDestroy(g);
            graphs[key] = ex;  // by key: a pass that had to grow a workspace has emptied the map
            *ran        = kRecorded;
        }
        AMX_HIP(hipGraphLaunch(ex, stream));
        return AMX_OK;
    }
};

// The `tuning` string of amx_mfcc_cfg / amx_gmm_model / amx_ffnn_model: "key=value,key=value".  A handle parses it once at
// creation against the list of keys it knows (an unknown key fails the creation: a typo must not silently select the default
// kernel) and keeps the values; nothing in the library reads kernel-selecting switches from the environment.  Lab builds
// (-DAMX_LAB, tools/ab_*.sh) append the AMX_TUNING environment variable to every handle's string, unknown keys ignored there.
struct Tuning {
    std::map<std::string, std::string> kv;
    // returns false (error text set) on a malformed string or a key that is not in `allowed` (NULL-terminated list)
    bool parse(const char* s, const char* const* allowed, const char* who);
    bool has(const char* key) const { return kv.count(key) != 0; }
    // Typed reads, checked at creation: false (error text set) unless the value is a whole decimal number within [lo, hi] /
    // one of `words` (NULL-terminated).  A value the key does not take fails the creation like an unknown key does.
    bool get_int(const char* key, int dflt, long lo, long hi, int* out, const char* who) const;
    bool get_word(const char* key, const char* dflt, const char* const* words, std::string* out, const char* who) const;
};

// keys of amx_gmm_model.tuning (gmm.hip and gmm_simd.hip parse the same string)
static const char* const gmm_tuning_keys[] = {"screen", "fused", "screen_all", "screen_kernel", "graph", "tied_prune", "chunk", "fused_waves", "fr",
                                              "simd_mfma", "contract", "dist_list", "near_fused", "fused_pack", nullptr};

// the ONE source of a fused multiply-add outside the GMM scorers (gmm_device.hpp has sq_acc<FMA>): a * b + c as the reference's
// default build computes it at a contracted site (FMA) or with two roundings (the library is compiled with -ffp-contract=off)
template<bool FMA>
__host__ __device__ __forceinline__ float mad(float a, float b, float c) {
    return FMA ? __builtin_fmaf(a, b, c) : a * b + c;
}
template<bool FMA>
__host__ __device__ __forceinline__ double mad(double a, double b, double c) {
    return FMA ? __builtin_fma(a, b, c) : a * b + c;
}

// streaming stores of the score / best-density matrices (written once, read by a later kernel or the host): non-temporal, so that
// gigabytes of results do not push the operand panels out of L2.  -DAMX_PLAIN_STORES (tools/energy_table.sh: a measurement build)
// turns them into plain stores for the energy / time comparison of profiles/r06/energy.json.
template<class V>
__device__ __forceinline__ void nt_store(V v, V* p) {
#ifdef AMX_PLAIN_STORES
    *p = v;
#else
    __builtin_nontemporal_store(v, p);
#endif
}

// whether the views in[T x in_w] (leading dimension in_ld) and out[T x out_w] share an element
inline bool views_alias(const float* in, int in_ld, int in_w, const float* out, int out_ld, int out_w, long long T) {
    if (T <= 0)
        return false;
    const float* in_end  = in + (T - 1) * (long long)in_ld + in_w;
    const float* out_end = out + (T - 1) * (long long)out_ld + out_w;
    if (in_end <= out || out_end <= in)
        return false;
    if (in_ld == out_ld) {
        const long long ld = in_ld, delta = out - in;
        const long long c  = ((delta % ld) + ld) % ld;  // column offset of `out` relative to `in`
        if (c >= in_w && c + out_w <= ld)
            return false;  // disjoint column ranges of the same matrix (also with a row shift)
    }
    return true;
}

inline int ceil_div(long a, long b) {
    return (int)((a + b - 1) / b);
}

}  // namespace amx
