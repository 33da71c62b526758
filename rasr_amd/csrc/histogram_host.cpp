// histogram_host.cpp -- histogram normalisation on the host: the handles, the files of Signal::HistogramVector<f32>::write / read
// (Signal/Histogram.hh:122-135, Signal/LookupTable.hh:298-319), Histogram::getCdf / percentile (Histogram.hh:56-80), LookupTable::getInverse
// (LookupTable.hh:239-271) and the two forms of HistogramNormalization::setTrainingHistograms (Signal/HistogramNormalization.cc:24-60).
// Everything here is sequential f32 arithmetic in the reference's order; no multiply feeds an add, so both contracts of the reference
// compute the same bits (tests/golden/ref_histogram.npz records that) and amx_set_contract changes nothing here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "histogram.hpp"

namespace amx {

// LookupTable::bucket (LookupTable.hh:69-72) is (s32)round(index / bucketSize) + offset; the cast is undefined outside s32, so the
// rounded quotient is cut to what an s32 holds first -- such an index lies far outside every table and ends in the same end bucket
static long long lookup_bucket(const LookupTable& t, float index) {
    float r = roundf(index / t.bucket_size);
    r       = r < -2147483648.f ? -2147483648.f : (r > 2147483520.f ? 2147483520.f : r);
    return (long long)(int32_t)r + t.offset;
}
static float lookup_index(const LookupTable& t, int32_t b) {
    return (float)(b - t.offset) * t.bucket_size;
}

size_t lookup_insert(LookupTable& t, float index, float init) {
    long long b = lookup_bucket(t, index);
    if (!t.f.empty()) {
        if (b < 0) {
            if (t.grow) {
                t.f.insert(t.f.begin(), (size_t)(-b), init);
                t.offset -= (int32_t)b;
            }
            b = 0;
        }
        else if (b >= (long long)t.f.size()) {
            if (t.grow)
                t.f.insert(t.f.end(), (size_t)(b - (long long)t.f.size() + 1), init);
            b = (long long)t.f.size() - 1;
        }
    }
    else {
        t.f.push_back(init);
        t.offset -= (int32_t)b;
        b = 0;
    }
    return (size_t)b;
}

static float lookup_sum(const LookupTable& t) {  // std::accumulate(begin(), end(), (Value)0)
    float s = 0.f;
    for (float v : t.f)
        s = s + v;
    return s;
}

int hist_table(const amx_histogram* h, int d, LookupTable* out) {
    AMX_REQUIRE(h && d >= 0 && d < h->dim, AMX_ERR_INVALID, "histogram: dimension %d is outside [0, %d)", d, h ? h->dim : 0);
    if (h->frozen) {
        *out = h->tables[d];
        return AMX_OK;
    }
    AMX_TRY(hist_sync_host(h));
    const HistCounts& c = h->counts[d];
    out->bucket_size    = h->bucket_size;
    out->offset         = c.offset;
    out->grow           = true;
    out->f.resize(c.c.size());
    for (size_t b = 0; b < c.c.size(); ++b)
        out->f[b] = (float)std::min(c.c[b], kHistSaturation);
    return AMX_OK;
}

// Histogram::getCdf (Histogram.hh:73-80): std::partial_sum, then every entry divided by sum()
int hist_cdf(const LookupTable& hist, LookupTable* cdf, const char* who) {
    const float sum = lookup_sum(hist);
    AMX_REQUIRE(!hist.f.empty() && sum != 0, AMX_ERR_INVALID, "%s: the histogram is empty (its sum is 0)", who);
    for (float v : hist.f)
        AMX_REQUIRE(v >= 0, AMX_ERR_INVALID, "%s: the histogram holds a negative or undefined value, its CDF would not be monotonous", who);
    *cdf      = hist;
    float acc = 0.f;
    for (size_t b = 0; b < cdf->f.size(); ++b) {
        acc       = b ? acc + hist.f[b] : hist.f[b];
        cdf->f[b] = acc;
    }
    for (float& v : cdf->f)
        v = v / sum;
    return AMX_OK;
}

// LookupTable::getInverse (LookupTable.hh:239-262) with proposeBucketSizeForInverse (:264-271)
static int lookup_inverse(const LookupTable& t, float bucket_size, LookupTable* inverse, const char* who) {
    *inverse = LookupTable();
    if (bucket_size == 0) {
        bucket_size = (*std::max_element(t.f.begin(), t.f.end()) - *std::min_element(t.f.begin(), t.f.end())) / ((float)t.f.size() * 2.f);
        AMX_REQUIRE(bucket_size > 0, AMX_ERR_INVALID, "%s: no bucket size can be proposed for the inverse of a constant table", who);
    }
    inverse->bucket_size = bucket_size;
    size_t previous      = 0;
    for (int32_t b = 0; b < (int32_t)t.f.size(); ++b) {
        const size_t current = lookup_insert(*inverse, t.f[b], 0.f);
        // insert may have grown the table at the front: positions of earlier entries move by the same amount only in that case, and the
        // reference's previousIndex does not follow them either (it is an index, not an iterator)
        const float v       = lookup_index(t, b);
        inverse->f[current] = v;
        if (previous < current)
            std::fill(inverse->f.begin() + previous + 1, inverse->f.begin() + current, v);
        else if (current < previous)
            std::fill(inverse->f.begin() + current + 1, inverse->f.begin() + previous, v);
        previous = current;
    }
    return AMX_OK;
}

int histnorm_build_inverse(amx_histnorm* h, const float* scales) {
    const size_t               n = h->train.size();
    std::vector<LookupTable>   interpolated;
    const std::vector<LookupTable>* hist = &h->train[0];
    if (n > 1) {
        // normalizeScales (HistogramNormalization.cc:91-93): the first scale is 1 - sum of the others, the sum taken in f64
        std::vector<float> s(n);
        double             sum = 0.0;
        for (size_t i = 1; i < n; ++i) {
            s[i] = scales[i - 1];
            sum += (double)s[i];
        }
        s[0] = (float)((double)1.0f - sum);
        for (size_t i = 0; i < n; ++i)  // areScalesWellDefined (:77-84)
            AMX_REQUIRE(s[i] >= 0 && s[i] <= 1, AMX_ERR_INVALID,  // a NaN is refused too
                        "amx_histnorm_set_scales: One or more histogram scales are smaller than zero or larger than 1 (scale %zu is %g).", i, s[i]);
        float minimal = std::numeric_limits<float>::max();
        for (size_t i = 0; i < n; ++i)
            for (const LookupTable& t : h->train[i])
                minimal = std::min(minimal, t.bucket_size);
        interpolated.assign((size_t)h->dim, LookupTable());
        for (LookupTable& t : interpolated)
            t.bucket_size = minimal;
        for (size_t i = 0; i < n; ++i)
            for (int d = 0; d < h->dim; ++d) {
                LookupTable to_add = h->train[i][d];
                const float surface = lookup_sum(to_add) * to_add.bucket_size;  // normalizeSurface (LookupTable.hh:204-209)
                AMX_REQUIRE(surface != 0, AMX_ERR_INVALID, "amx_histnorm: training histogram %zu is empty in dimension %d", i, d);
                for (float& v : to_add.f)
                    v = v / surface;
                for (float& v : to_add.f)  // operator*= (:283-289)
                    v = v * s[i];
                for (int32_t b = 0; b < (int32_t)to_add.f.size(); ++b) {  // operator+= (:273-281)
                    const size_t at = lookup_insert(interpolated[d], lookup_index(to_add, b), 0.f);
                    interpolated[d].f[at] = interpolated[d].f[at] + to_add.f[b];
                }
            }
        hist = &interpolated;
    }
    std::vector<LookupTable> inverse((size_t)h->dim);
    for (int d = 0; d < h->dim; ++d) {
        LookupTable cdf;
        AMX_TRY(hist_cdf((*hist)[d], &cdf, "amx_histnorm (training histogram)"));
        AMX_TRY(lookup_inverse(cdf, h->probability_bucket_size, &inverse[d], "amx_histnorm (training CDF)"));
    }
    h->inverse.swap(inverse);
    h->meta_dirty = true;
    return AMX_OK;
}

static int copy_out(const LookupTable& t, float* bucket_size, int* offset, int* size, float* values) {
    if (bucket_size)
        *bucket_size = t.bucket_size;
    if (offset)
        *offset = t.offset;
    if (size)
        *size = (int)t.f.size();
    if (values && !t.f.empty())
        memcpy(values, t.f.data(), t.f.size() * sizeof(float));
    return AMX_OK;
}

// the range of k = (s32)round(x / bucket_size) per dimension over T frames; false (error text set) on a value the cast is undefined for
static bool host_range(const amx_histogram* h, const float* x, int in_ld, long T, std::vector<int32_t>& kmin, std::vector<int32_t>& kmax) {
    kmin.assign((size_t)h->dim, std::numeric_limits<int32_t>::max());
    kmax.assign((size_t)h->dim, std::numeric_limits<int32_t>::min());
    for (long t = 0; t < T; ++t)
        for (int d = 0; d < h->dim; ++d) {
            const float q = x[(size_t)t * in_ld + d] / h->bucket_size;
            if (!(fabsf(q) < kHistMaxQuotient)) {
                set_error("amx_histogram_accumulate: frame %ld, component %d is not finite or lies %g buckets from zero (2^30 and more are refused)",
                          t, d, (double)q);
                return false;
            }
            const int32_t k = (int32_t)roundf(q);
            kmin[d]         = std::min(kmin[d], k);
            kmax[d]         = std::max(kmax[d], k);
        }
    return true;
}

}  // namespace amx

using amx::LookupTable;

extern "C" {

int amx_histogram_create(amx_ctx* ctx, int dim, float bucket_size, amx_histogram** out) {
    AMX_REQUIRE(out, AMX_ERR_INVALID, "amx_histogram_create: NULL argument");
    *out = nullptr;
    AMX_REQUIRE(dim >= 1 && dim <= amx::kHistMaxDim, AMX_ERR_INVALID, "amx_histogram_create: dim %d is outside [1, %d]", dim, amx::kHistMaxDim);
    AMX_REQUIRE(bucket_size > 0 && std::isfinite(bucket_size), AMX_ERR_INVALID, "amx_histogram_create: Bucket size is %g, it must be positive.",
                (double)bucket_size);
    amx_histogram* h = new amx_histogram;
    h->ctx           = ctx;
    h->dim           = dim;
    h->bucket_size   = bucket_size;
    h->counts.resize((size_t)dim);
    *out = h;
    return AMX_OK;
}

void amx_histogram_destroy(amx_histogram* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_histogram_attach(amx_histogram* h, amx_ctx* ctx) {
    AMX_REQUIRE(h && ctx, AMX_ERR_INVALID, "amx_histogram_attach: NULL argument");
    AMX_REQUIRE(!h->ctx || h->ctx == ctx, AMX_ERR_STATE, "amx_histogram_attach: the handle already belongs to another context");
    h->ctx = ctx;
    return AMX_OK;
}

int amx_histogram_describe(const amx_histogram* h, amx_histogram_info* info) {
    AMX_REQUIRE(h && info, AMX_ERR_INVALID, "amx_histogram_describe: NULL argument");
    info->dim             = h->dim;
    info->bucket_size     = h->bucket_size;
    info->frozen          = h->frozen ? 1 : 0;
    info->lds_max_buckets = amx::kHistLdsBuckets;
    info->lds_capacity    = amx::kHistLdsCapacity;
    info->frames          = h->frames;
    info->n_lds           = h->n_lds;
    info->n_global        = h->n_global;
    info->n_device_calls  = h->n_calls;
    return AMX_OK;
}

int amx_histogram_accumulate(amx_histogram* h, const float* feats, int in_ld, long T) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_histogram_accumulate: NULL handle");
    AMX_REQUIRE(!h->frozen, AMX_ERR_STATE, "amx_histogram_accumulate: the handle was read from a file whose values are not counts; it only serves tables");
    AMX_REQUIRE(in_ld >= h->dim && T >= 0, AMX_ERR_INVALID, "amx_histogram_accumulate: in_ld %d < dim %d or negative frame count %ld", in_ld, h->dim, T);
    if (T == 0)
        return AMX_OK;
    AMX_REQUIRE(feats, AMX_ERR_INVALID, "amx_histogram_accumulate: NULL buffer");
    AMX_REQUIRE((unsigned long long)T <= 0xffffffffull - h->frames, AMX_ERR_INVALID,
                "amx_histogram_accumulate: %ld more frames would take the handle past 2^32 - 1 frames (it holds %llu)", T, h->frames);
    AMX_TRY(amx::hist_sync_host(h));
    std::vector<int32_t> kmin, kmax;
    if (!amx::host_range(h, feats, in_ld, T, kmin, kmax))
        return AMX_ERR_INVALID;
    for (int d = 0; d < h->dim; ++d) {
        amx::HistCounts& c = h->counts[d];
        if (c.c.empty()) {
            c.offset = -kmin[d];
            c.c.assign((size_t)((long long)kmax[d] - kmin[d] + 1), 0u);
        }
        else {
            const long long lo = std::min<long long>(-(long long)c.offset, kmin[d]), hi = std::max<long long>((long long)c.c.size() - 1 - c.offset, kmax[d]);
            c.c.insert(c.c.begin(), (size_t)(-(long long)c.offset - lo), 0u);
            c.offset = (int32_t)-lo;
            c.c.resize((size_t)(hi - lo + 1), 0u);
        }
    }
    for (long t = 0; t < T; ++t)
        for (int d = 0; d < h->dim; ++d) {
            const int32_t k = (int32_t)roundf(feats[(size_t)t * in_ld + d] / h->bucket_size);
            ++h->counts[d].c[(size_t)((long long)k + h->counts[d].offset)];
        }
    h->frames += (unsigned long long)T;
    h->dev_valid = false;
    return AMX_OK;
}

int amx_histogram_table(const amx_histogram* h, int d, float* bucket_size, int* offset, int* size, float* values) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_histogram_table: NULL handle");
    LookupTable t;
    AMX_TRY(amx::hist_table(h, d, &t));
    return amx::copy_out(t, bucket_size, offset, size, values);
}

int amx_histogram_cdf(const amx_histogram* h, int d, float* bucket_size, int* offset, int* size, float* values) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_histogram_cdf: NULL handle");
    LookupTable t, cdf;
    AMX_TRY(amx::hist_table(h, d, &t));
    AMX_TRY(amx::hist_cdf(t, &cdf, "amx_histogram_cdf"));
    return amx::copy_out(cdf, bucket_size, offset, size, values);
}

// Histogram::percentile (Histogram.hh:56-64)
int amx_histogram_percentile(const amx_histogram* h, int d, float percent, float* value) {
    AMX_REQUIRE(h && value, AMX_ERR_INVALID, "amx_histogram_percentile: NULL argument");
    LookupTable t;
    AMX_TRY(amx::hist_table(h, d, &t));
    float   p = percent * amx::lookup_sum(t);
    int32_t b = 0;
    for (; b < (int32_t)t.f.size() && p > 0; ++b)
        p = p - t.f[b];
    *value = amx::lookup_index(t, b);
    return AMX_OK;
}

// ---- files: u32 n | n x (f32 bucketSize, s32 offset, bool grow (one byte: 0xff or 0), u32 size, f32 values[size]), little endian
int amx_histogram_write(const amx_histogram* h, const char* path) {
    AMX_REQUIRE(h && path, AMX_ERR_INVALID, "amx_histogram_write: NULL argument");
    std::vector<LookupTable> t((size_t)h->dim);
    for (int d = 0; d < h->dim; ++d)
        AMX_TRY(amx::hist_table(h, d, &t[d]));
    FILE* f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "amx_histogram_write: cannot open '%s'", path);
    const uint32_t n  = (uint32_t)h->dim;
    bool           ok = fwrite(&n, 4, 1, f) == 1;
    for (int d = 0; d < h->dim && ok; ++d) {
        const uint32_t      size = (uint32_t)t[d].f.size();
        const unsigned char grow = t[d].grow ? 0xff : 0;  // BinaryOutputStream::write<bool> (Core/BinaryStream.cc:95-103)
        ok = fwrite(&t[d].bucket_size, 4, 1, f) == 1 && fwrite(&t[d].offset, 4, 1, f) == 1 && fwrite(&grow, 1, 1, f) == 1 && fwrite(&size, 4, 1, f) == 1 &&
             (size == 0 || fwrite(t[d].f.data(), 4, size, f) == size);
    }
    ok = (fclose(f) == 0) && ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "amx_histogram_write: write to '%s' failed", path);
    return AMX_OK;
}

int amx_histogram_read(const char* path, amx_histogram** out) {
    AMX_REQUIRE(path && out, AMX_ERR_INVALID, "amx_histogram_read: NULL argument");
    *out    = nullptr;
    FILE* f = fopen(path, "rb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "amx_histogram_read: cannot open '%s'", path);
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint32_t                 n = 0;
    bool                     ok = fread(&n, 4, 1, f) == 1 && n >= 1 && n <= (uint32_t)amx::kHistMaxDim;
    std::vector<LookupTable> t(ok ? n : 0);
    for (uint32_t d = 0; d < n && ok; ++d) {
        uint32_t      size = 0;
        unsigned char grow = 0;
        ok = fread(&t[d].bucket_size, 4, 1, f) == 1 && fread(&t[d].offset, 4, 1, f) == 1 && fread(&grow, 1, 1, f) == 1 && fread(&size, 4, 1, f) == 1 &&
             (long)size <= (bytes - ftell(f)) / 4 && t[d].bucket_size > 0;
        if (ok) {
            t[d].grow = grow != 0;
            t[d].f.resize(size);
            ok = size == 0 || fread(t[d].f.data(), 4, size, f) == size;
        }
    }
    fclose(f);
    if (!ok) {
        amx::set_error("amx_histogram_read: '%s' is not a histogram-vector file (1 to %d tables of positive bucket size) or is truncated", path, amx::kHistMaxDim);
        return AMX_ERR_INVALID;
    }
    amx_histogram* h = new amx_histogram;
    h->dim           = (int)n;
    h->bucket_size   = t[0].bucket_size;
    // a file resumes counting if it is what this library's estimator writes: one bucket size, tables that grow, whole counts up to 2^24
    // whose window fits the s32 arithmetic of the kernels
    bool counts = true;
    for (const LookupTable& lt : t) {
        counts = counts && lt.grow && lt.bucket_size == h->bucket_size && (long long)lt.f.size() < (1ll << 31) &&
                 std::llabs((long long)lt.offset) < (1ll << 30) && std::llabs((long long)lt.f.size() - lt.offset) <= (1ll << 30);
        for (float v : lt.f)
            counts = counts && v >= 0 && v <= (float)amx::kHistSaturation && v == floorf(v);
    }
    if (counts) {
        h->counts.resize(n);
        for (uint32_t d = 0; d < n; ++d) {
            h->counts[d].offset    = t[d].offset;
            unsigned long long sum = 0;
            for (float v : t[d].f) {
                h->counts[d].c.push_back((uint32_t)v);
                sum += (uint32_t)v;
            }
            h->frames = std::max(h->frames, sum);
        }
        if (h->frames > 0xffffffffull)
            counts = false;
    }
    if (!counts) {
        h->frozen = true;
        h->frames = 0;
        h->counts.clear();
        h->tables.swap(t);
    }
    *out = h;
    return AMX_OK;
}

// ---- the normaliser
int amx_histnorm_create(amx_ctx* ctx, int n_train, const amx_histogram* const* train, float probability_bucket_size, amx_histnorm** out) {
    AMX_REQUIRE(out, AMX_ERR_INVALID, "amx_histnorm_create: NULL argument");
    *out = nullptr;
    AMX_REQUIRE(n_train >= 1 && train, AMX_ERR_INVALID, "amx_histnorm_create: at least one training histogram is needed");
    AMX_REQUIRE(probability_bucket_size >= 0 && std::isfinite(probability_bucket_size), AMX_ERR_INVALID,
                "amx_histnorm_create: probability bucket size %g is negative", (double)probability_bucket_size);
    for (int i = 0; i < n_train; ++i) {
        AMX_REQUIRE(train[i], AMX_ERR_INVALID, "amx_histnorm_create: training histogram %d is NULL", i);
        AMX_REQUIRE(train[i]->dim == train[0]->dim, AMX_ERR_INVALID, "amx_histnorm_create: Mismatch between #training-histograms(%d) and feature dimension(%d).",
                    train[i]->dim, train[0]->dim);
    }
    std::unique_ptr<amx_histnorm> h(new amx_histnorm);
    h->ctx                     = ctx;
    h->dim                     = train[0]->dim;
    h->probability_bucket_size = probability_bucket_size;
    h->train.resize((size_t)n_train);
    for (int i = 0; i < n_train; ++i) {
        h->train[i].resize((size_t)h->dim);
        for (int d = 0; d < h->dim; ++d)
            AMX_TRY(amx::hist_table(train[i], d, &h->train[i][d]));
    }
    if (n_train == 1)
        AMX_TRY(amx::histnorm_build_inverse(h.get(), nullptr));
    *out = h.release();
    return AMX_OK;
}

void amx_histnorm_destroy(amx_histnorm* h) {
    if (!h)
        return;
    if (h->ctx)
        hipSetDevice(h->ctx->device);
    delete h;
}

int amx_histnorm_set_scales(amx_histnorm* h, const float* scales) {
    AMX_REQUIRE(h, AMX_ERR_INVALID, "amx_histnorm_set_scales: NULL handle");
    AMX_REQUIRE(h->train.size() > 1, AMX_ERR_STATE, "amx_histnorm_set_scales: one training histogram takes no scale");
    AMX_REQUIRE(scales, AMX_ERR_INVALID, "amx_histnorm_set_scales: NULL scales");
    return amx::histnorm_build_inverse(h, scales);
}

int amx_histnorm_add_key(amx_histnorm* h, const amx_histogram* test, int* key) {
    AMX_REQUIRE(h && test && key, AMX_ERR_INVALID, "amx_histnorm_add_key: NULL argument");
    AMX_REQUIRE(test->dim == h->dim, AMX_ERR_INVALID, "amx_histnorm_add_key: Mismatch between #test-histograms(%d) and feature dimension(%d).", test->dim, h->dim);
    std::vector<LookupTable> cdfs((size_t)h->dim);
    for (int d = 0; d < h->dim; ++d) {
        LookupTable t;
        AMX_TRY(amx::hist_table(test, d, &t));
        AMX_TRY(amx::hist_cdf(t, &cdfs[d], "amx_histnorm_add_key"));
    }
    h->keys.push_back(std::move(cdfs));
    h->meta_dirty = true;
    *key          = (int)h->keys.size() - 1;
    return AMX_OK;
}

int amx_histnorm_n_keys(const amx_histnorm* h) {
    return h ? (int)h->keys.size() : 0;
}

int amx_histnorm_inverse_cdf(const amx_histnorm* h, int d, float* bucket_size, int* offset, int* size, float* values) {
    AMX_REQUIRE(h && d >= 0 && d < h->dim, AMX_ERR_INVALID, "amx_histnorm_inverse_cdf: bad handle or dimension %d", d);
    AMX_REQUIRE(!h->inverse.empty(), AMX_ERR_STATE, "amx_histnorm_inverse_cdf: several training histograms need amx_histnorm_set_scales first");
    return amx::copy_out(h->inverse[d], bucket_size, offset, size, values);
}

int amx_histnorm_test_cdf(const amx_histnorm* h, int key, int d, float* bucket_size, int* offset, int* size, float* values) {
    AMX_REQUIRE(h && d >= 0 && d < h->dim && key >= 0 && key < (int)h->keys.size(), AMX_ERR_INVALID, "amx_histnorm_test_cdf: bad handle, key %d or dimension %d",
                key, d);
    return amx::copy_out(h->keys[key][d], bucket_size, offset, size, values);
}

}  // extern "C"
