// histogram.hpp -- the two handles of histogram normalisation, shared by histogram.hip (device) and histogram_host.cpp (files, tables).
#pragma once
#include <cstdint>
#include <vector>

#include "common.hpp"

namespace amx {

// Signal::LookupTable<f32, f32> (Signal/LookupTable.hh:50-66): bucketSize_, offset_, f_, grow_
struct LookupTable {
    float              bucket_size = 0.f;
    int32_t            offset      = 0;
    bool               grow        = true;
    std::vector<float> f;
};

// One dimension of a histogram that still counts: bucket b holds the frames with k = b - offset.  The reference adds 1.0f in f32, so its
// value stops at 2^24; the count goes on in u32 and is cut when it is exported.
struct HistCounts {
    int32_t               offset = 0;
    std::vector<uint32_t> c;  // empty: nothing seen yet
};

constexpr uint32_t kHistSaturation  = 1u << 24;  // the f32 value at which a + 1.0f == a
constexpr int      kHistLdsBuckets  = 512;       // a dimension whose window has at most this many buckets may count in LDS ...
constexpr int      kHistLdsCapacity = 8192;      // ... as long as the workgroup's table (u32 words, 32 KB) still has room, dimensions in order
constexpr int      kHistMaxDim      = 4096;      // the range kernel keeps min / max of every dimension in LDS (32 KB)
constexpr float    kHistMaxQuotient = 1073741824.f;  // |x / bucket_size| >= 2^30 is refused

struct HistDimMeta {  // one dimension of one count launch, device side
    long long off;      // first bucket in the flat count buffer
    int       kmin;     // k of bucket 0
    int       size;     // buckets in the window
    int       lds_off;  // first word in the workgroup's LDS table, -1: global atomics
    int       pad;
};

struct TableMeta {  // one lookup table on the device
    const float* values;
    float        bucket_size;
    int          offset;
    int          size;
    int          pad;
};

}  // namespace amx

struct amx_histogram {
    amx_ctx*                     ctx         = nullptr;
    int                          dim         = 0;
    float                        bucket_size = 0.f;
    bool                         frozen      = false;  // read from a file whose values are not counts: tables only
    std::vector<amx::LookupTable> tables;              // frozen handles
    std::vector<amx::HistCounts>  counts;              // counting handles; valid when host_valid
    unsigned long long           frames = 0;           // accumulated so far (a file: the largest sum of one dimension)
    bool                         host_valid = true, dev_valid = false;
    // device state of a counting handle: the windows as the device holds them and one flat buffer of counts
    std::vector<int32_t>         d_kmin, d_size;
    std::vector<long long>       d_off;                // [dim + 1]
    std::unique_ptr<amx::DevBuf<uint32_t>> d_counts;
    amx::DevBuf<int>             d_range;              // [2 dim + 1]
    amx::DevBuf<amx::HistDimMeta> d_meta;
    unsigned long long           n_lds = 0, n_global = 0, n_calls = 0;
};

struct amx_histnorm {
    amx_ctx*                                   ctx = nullptr;
    int                                        dim = 0;
    float                                      probability_bucket_size = 0.f;
    std::vector<std::vector<amx::LookupTable>> train;    // [n_train][dim] copies of the training histograms
    std::vector<amx::LookupTable>              inverse;  // [dim], empty until they can be built
    std::vector<std::vector<amx::LookupTable>> keys;     // [n_keys][dim] test CDFs
    // device copies
    amx::DevBuf<float>                              d_inverse;
    std::vector<std::unique_ptr<amx::DevBuf<float>>> d_keys;
    amx::DevBuf<amx::TableMeta>                     d_meta;  // [dim] inverse tables, then [n_keys][dim] test CDFs
    bool                                            meta_dirty = true;
    amx::DevBuf<long long>                          d_seg;   // [n_seg + 1] frame offsets, then n_seg keys (as long long)
    amx::DevBuf<unsigned long long>                 d_clamped;
};

namespace amx {
// host state of a handle, downloaded from the device if the device is ahead (histogram.hip)
int  hist_sync_host(const amx_histogram* h);
// one dimension as the reference's Histogram<f32>
int  hist_table(const amx_histogram* h, int d, LookupTable* out);
int  hist_cdf(const LookupTable& hist, LookupTable* cdf, const char* who);
int  histnorm_build_inverse(amx_histnorm* h, const float* scales);
// LookupTable::insert (LookupTable.hh:178-202): the bucket of `index`, the table grown if it may
size_t lookup_insert(LookupTable& t, float index, float init);
}  // namespace amx
