// cmllr_host.cpp -- the host side of constrained MLLR (include/amx.h, section "constrained MLLR"): Mm::AffineFeatureTransformAccumulator's
// files, combine, finalize, estimate and score (Mm/AffineFeatureTransformAccumulator.cc:123-377) on ONE key's part of the flat accumulator
// that cmllr.hip fills.  Nothing here needs a device.
//
// estimate and score restate the reference operation by operation in f64, Math::Matrix / Math::Vector's loops included (a dot product
// starts at T() and adds a[i] * b[i] with i ascending; Matrix / scalar divides every element, Vector / scalar too).  Two things are not
// the reference's bits: the inverse (the reference calls dgetrf / dgetri of whatever LAPACK it is linked with; here an LU with partial
// pivoting and one triangular solve per unit vector), and the products' roundings where its -march=native build contracts a dot product
// into fused multiply-adds (this file is compiled with -ffp-contract=off and follows the other build).  Both are far inside the bar that
// tests/golden/make_cmllr_golden.py measures against the reference's text with OpenBLAS's LU in both builds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"

extern "C++" {
namespace {

constexpr const char* kCmllrTag = "affine-feature-transform-accumulator";   // AffineFeatureTransformAccumulator.hh:81-83
constexpr int         kCmllrMaxDim = 255;

struct CmllrLayout {
    int  F, M, R;
    long tri, off_k, off_mean, off_cov, off_g, size;
};

bool cmllr_shape_ok(const amx_cmllr_shape* s) {
    return s && s->model_dim >= 1 && s->feature_dim >= s->model_dim && s->feature_dim <= kCmllrMaxDim && s->n_keys >= 1;
}

CmllrLayout cmllr_layout(const amx_cmllr_shape* s) {
    CmllrLayout l;
    l.F = s->feature_dim, l.M = s->model_dim, l.R = l.F + 1;
    l.tri      = (long)l.R * (l.R + 1) / 2;
    l.off_k    = 1;
    l.off_mean = l.off_k + (long)l.M * l.R;
    l.off_cov  = l.off_mean + l.R;
    l.off_g    = l.off_cov + l.tri;
    l.size     = l.off_g + (s->pooled ? 0 : (long)l.M * l.tri);
    return l;
}

// cell (j, k), j <= k, of the row-major upper triangle of an R x R matrix
inline long tri_at(int R, int j, int k) {
    return (long)j * R - (long)j * (j - 1) / 2 + (k - j);
}

typedef std::vector<double> Vec;
struct Mat {   // row-major
    int r = 0, c = 0;
    Vec a;
    Mat() = default;
    Mat(int rows, int cols)
            : r(rows), c(cols), a((size_t)rows * cols, 0.0) {}
    double&       at(int i, int j) { return a[(size_t)i * c + j]; }
    const double& at(int i, int j) const { return a[(size_t)i * c + j]; }
};

// Vector::operator*(Vector), Math/Vector.hh:94-101
double dot(const double* a, const double* b, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i)
        s += a[i] * b[i];
    return s;
}
// Matrix::operator*(Vector), Math/Matrix.hh:486-494
Vec mat_vec(const Mat& m, const Vec& v) {
    Vec out((size_t)m.r);
    for (int n = 0; n < m.r; ++n)
        out[n] = dot(&m.a[(size_t)n * m.c], v.data(), m.c);
    return out;
}
// Matrix::operator*(Matrix), Math/Matrix.hh:496-508
Mat mat_mat(const Mat& l, const Mat& rs) {
    Mat out(l.r, rs.c);
    for (int n = 0; n < l.r; ++n)
        for (int m = 0; m < rs.c; ++m) {
            double s = 0;
            for (int k = 0; k < l.c; ++k)
                s += l.at(n, k) * rs.at(k, m);
            out.at(n, m) = s;
        }
    return out;
}
Mat transpose(const Mat& m) {
    Mat out(m.c, m.r);
    for (int i = 0; i < m.c; ++i)
        for (int j = 0; j < m.r; ++j)
            out.at(i, j) = m.at(j, i);
    return out;
}

// P A = L U with partial pivoting in place (the first largest |.| of the column is the pivot, as dgetf2's idamax takes it); false when a
// pivot is exactly zero
bool lu_factor(Mat& a, std::vector<int>& piv) {
    const int n = a.r;
    piv.resize((size_t)n);
    for (int c = 0; c < n; ++c) {
        int    p = c;
        double best = std::fabs(a.at(c, c));
        for (int i = c + 1; i < n; ++i)
            if (std::fabs(a.at(i, c)) > best)
                best = std::fabs(a.at(i, c)), p = i;
        piv[c] = p;
        if (!(best > 0.0) || !std::isfinite(best))
            return false;
        if (p != c)
            for (int j = 0; j < n; ++j)
                std::swap(a.at(c, j), a.at(p, j));
        const double d = a.at(c, c);
        for (int i = c + 1; i < n; ++i) {
            const double f = a.at(i, c) / d;
            a.at(i, c)     = f;
            for (int j = c + 1; j < n; ++j)
                a.at(i, j) -= f * a.at(c, j);
        }
    }
    return true;
}

// Math::Lapack::invert (Math/Lapack/MatrixTools.hh:29-99)
bool invert(Mat& m) {
    const int        n = m.r;
    Mat              lu = m;
    std::vector<int> piv;
    if (!lu_factor(lu, piv))
        return false;
    Vec x((size_t)n);
    for (int col = 0; col < n; ++col) {
        for (int i = 0; i < n; ++i)
            x[i] = i == col ? 1.0 : 0.0;
        for (int i = 0; i < n; ++i)
            if (piv[i] != i)
                std::swap(x[i], x[piv[i]]);
        for (int i = 1; i < n; ++i) {   // L y = P e
            double s = x[i];
            for (int j = 0; j < i; ++j)
                s -= lu.at(i, j) * x[j];
            x[i] = s;
        }
        for (int i = n - 1; i >= 0; --i) {   // U x = y
            double s = x[i];
            for (int j = i + 1; j < n; ++j)
                s -= lu.at(i, j) * x[j];
            x[i] = s / lu.at(i, i);
        }
        for (int i = 0; i < n; ++i)
            m.at(i, col) = x[i];
    }
    return true;
}

// Math::Lapack::logDeterminant (MatrixTools.hh:112-148): the sum of log |u_ii|
bool log_determinant(const Mat& m, double* out) {
    Mat              lu = m;
    std::vector<int> piv;
    if (!lu_factor(lu, piv))
        return false;
    double d = 0.0;
    for (int i = 0; i < m.r; ++i)
        d += std::log(std::fabs(lu.at(i, i)));
    *out = d;
    return true;
}

// the accumulator after finalize() (:123-143): G mirrored (derived from cov for a pooled model), cov mirrored
struct Finalized {
    double           beta = 0;
    std::vector<Mat> G;     // M of R x R
    std::vector<Vec> k;     // M of R
    Vec              mean;  // R
    Mat              cov;   // R x R
};

Finalized finalize(const CmllrLayout& l, bool pooled, const float* variance, const double* acc) {
    Finalized f;
    const int R = l.R;
    f.beta      = acc[0];
    f.k.resize((size_t)l.M);
    for (int i = 0; i < l.M; ++i)
        f.k[i].assign(acc + l.off_k + (long)i * R, acc + l.off_k + (long)(i + 1) * R);
    f.mean.assign(acc + l.off_mean, acc + l.off_mean + R);
    f.cov = Mat(R, R);
    f.G.assign((size_t)l.M, Mat(R, R));
    for (int i = 0; i < l.M; ++i)
        for (int j = 0; j < R; ++j)
            for (int k = j; k < R; ++k) {
                const double v = pooled ? acc[l.off_cov + tri_at(R, j, k)] / (double)variance[i]   // :129
                                        : acc[l.off_g + (long)i * l.tri + tri_at(R, j, k)];
                f.G[i].at(j, k) = v;
                f.G[i].at(k, j) = v;
            }
    for (int j = 0; j < R; ++j)
        for (int k = j; k < R; ++k)
            f.cov.at(j, k) = f.cov.at(k, j) = acc[l.off_cov + tri_at(R, j, k)];
    return f;
}

// the global covariance of :233-236 / :317-320: cov / beta - (mean / beta)(mean / beta)^T without row and column 0
Mat global_covariance(const Finalized& f, int R) {
    Vec a((size_t)R);
    for (int i = 0; i < R; ++i)
        a[i] = f.mean[i] / f.beta;
    Mat gc(R - 1, R - 1);
    for (int i = 1; i < R; ++i)
        for (int j = 1; j < R; ++j)
            gc.at(i - 1, j - 1) = f.cov.at(i, j) / f.beta - a[i] * a[j];
    return gc;
}

int check_host_args(const amx_cmllr_shape* shape, const float* variance, const double* acc, const char* who) {
    AMX_REQUIRE(shape, AMX_ERR_INVALID, "%s: NULL shape", who);
    AMX_REQUIRE(shape->feature_dim >= shape->model_dim, AMX_ERR_INVALID, "%s: feature_dim %d is smaller than model_dim %d", who,
                shape->feature_dim, shape->model_dim);
    AMX_REQUIRE(cmllr_shape_ok(shape), AMX_ERR_INVALID, "%s: bad shape (feature_dim %d in [model_dim, %d], model_dim %d, n_keys %d)", who,
                shape->feature_dim, kCmllrMaxDim, shape->model_dim, shape->n_keys);
    AMX_REQUIRE(acc, AMX_ERR_INVALID, "%s: NULL accumulator", who);
    AMX_REQUIRE(!shape->pooled || variance, AMX_ERR_INVALID, "%s: a pooled model needs its variance vector", who);
    return AMX_OK;
}

template<class T>
bool put(FILE* f, T v) {
    return fwrite(&v, sizeof(T), 1, f) == 1;   // little-endian host
}
template<class T>
bool get(FILE* f, T* v) {
    return fread(v, sizeof(T), 1, f) == 1;
}

}  // namespace
}  // extern "C++"

extern "C" {

long amx_cmllr_key_size(const amx_cmllr_shape* shape) {
    return cmllr_shape_ok(shape) ? cmllr_layout(shape).size : 0;
}

int amx_cmllr_accumulator_write(const amx_cmllr_shape* shape, const float* variance, const double* acc, const char* path) {
    const char* who = "amx_cmllr_accumulator_write";
    AMX_TRY(check_host_args(shape, variance, acc, who));
    AMX_REQUIRE(path, AMX_ERR_INVALID, "%s: NULL path", who);
    const CmllrLayout l = cmllr_layout(shape);
    const int         R = l.R;
    FILE*             f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    // a Math::Matrix<f64> with its upper triangle from `tri` (NULL: 0 x 0), Math/Matrix.hh:560-564
    auto matrix = [&](const double* tri) {
        if (!tri)
            return put(f, (uint32_t)0) && put(f, (uint32_t)0) && put(f, (uint32_t)0);
        bool ok = put(f, (uint32_t)R) && put(f, (uint32_t)R) && put(f, (uint32_t)R);
        for (int j = 0; ok && j < R; ++j) {
            ok = put(f, (uint32_t)R);
            for (int k = 0; ok && k < R; ++k)
                ok = put(f, k >= j ? tri[tri_at(R, j, k)] : 0.0);
        }
        return ok;
    };
    const uint32_t n_tag = (uint32_t)strlen(kCmllrTag);
    bool           ok = put(f, n_tag) && fwrite(kCmllrTag, 1, n_tag, f) == n_tag;   // Core::IoRef::write
    ok = ok && put(f, (uint32_t)l.F) && put(f, (uint32_t)l.M) && put(f, acc[0]);
    ok = ok && put(f, (uint32_t)l.M);
    for (int i = 0; ok && i < l.M; ++i)
        ok = matrix(shape->pooled ? nullptr : acc + l.off_g + (long)i * l.tri);
    ok = ok && put(f, (uint32_t)l.M);
    for (int i = 0; ok && i < l.M; ++i)
        ok = put(f, (uint32_t)R) && fwrite(acc + l.off_k + (long)i * R, 8, (size_t)R, f) == (size_t)R;
    ok = ok && put(f, (uint32_t)R) && fwrite(acc + l.off_mean, 8, (size_t)R, f) == (size_t)R;
    ok = ok && matrix(acc + l.off_cov);
    ok = ok && put(f, (uint32_t)(shape->pooled ? l.M : 0));
    if (ok && shape->pooled)
        ok = fwrite(variance, 4, (size_t)l.M, f) == (size_t)l.M;
    ok = ok && put(f, (uint8_t)(shape->pooled ? 0xff : 0));   // BinaryOutputStream::write<bool>
    ok = (fclose(f) == 0) && ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: write to '%s' failed", who, path);
    return AMX_OK;
}

int amx_cmllr_accumulator_read(const amx_cmllr_shape* shape, const float* variance, const char* path, double* acc) {
    const char* who = "amx_cmllr_accumulator_read";
    AMX_TRY(check_host_args(shape, variance, acc, who));
    AMX_REQUIRE(path, AMX_ERR_INVALID, "%s: NULL path", who);
    const CmllrLayout l = cmllr_layout(shape);
    const int         R = l.R;
    FILE*             f = fopen(path, "rb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    const char* why = nullptr;
    Vec         tmp((size_t)l.size, 0.0);
    // 0: bad, 1: read into tri, 2: a 0 x 0 matrix
    auto matrix = [&](double* tri) {
        uint32_t r = 0, c = 0, n = 0;
        if (!(get(f, &r) && get(f, &c) && get(f, &n)))
            return 0;
        if (r == 0 && c == 0 && n == 0)
            return 2;
        if ((int)r != R || (int)c != R || (int)n != R)
            return 0;
        for (int j = 0; j < R; ++j) {
            uint32_t m = 0;
            if (!get(f, &m) || (int)m != R)
                return 0;
            for (int k = 0; k < R; ++k) {
                double v = 0;
                if (!get(f, &v))
                    return 0;
                if (k >= j) {
                    if (tri)
                        tri[tri_at(R, j, k)] = v;
                }
                else if (v != 0.0) {
                    why = "a lower triangle is not zero (a finalized accumulator)";
                    return 0;
                }
            }
        }
        return 1;
    };
    uint32_t n_tag = 0, F = 0, M = 0, n = 0;
    char     tag[64] = {0};
    bool     ok = get(f, &n_tag);
    if (ok && (n_tag != strlen(kCmllrTag) || fread(tag, 1, n_tag, f) != n_tag || memcmp(tag, kCmllrTag, n_tag) != 0)) {
        why = "the type tag is not 'affine-feature-transform-accumulator'";
        ok  = false;
    }
    ok = ok && get(f, &F) && get(f, &M);
    if (ok && ((int)F != l.F || (int)M != l.M)) {
        why = "the dimensions differ from the shape's";
        ok  = false;
    }
    ok = ok && get(f, &tmp[0]) && get(f, &n) && (int)n == l.M;
    int g_kind = 0;
    for (int i = 0; ok && i < l.M; ++i) {
        const int kind = matrix(shape->pooled ? nullptr : &tmp[l.off_g + (long)i * l.tri]);
        ok             = kind != 0 && (i == 0 || kind == g_kind);
        g_kind         = kind;
    }
    ok = ok && get(f, &n) && (int)n == l.M;
    for (int i = 0; ok && i < l.M; ++i)
        ok = get(f, &n) && (int)n == R && fread(&tmp[l.off_k + (long)i * R], 8, (size_t)R, f) == (size_t)R;
    ok = ok && get(f, &n) && (int)n == R && fread(&tmp[l.off_mean], 8, (size_t)R, f) == (size_t)R;
    ok = ok && matrix(&tmp[l.off_cov]) == 1;
    std::vector<float> var;
    if (ok && (ok = get(f, &n) && n <= (uint32_t)kCmllrMaxDim)) {
        var.resize(n);
        ok = n == 0 || fread(var.data(), 4, n, f) == n;
    }
    uint8_t flag = 0;
    ok           = ok && get(f, &flag);
    fclose(f);
    if (ok && !why) {
        const bool pooled = flag != 0;
        if (pooled != (shape->pooled != 0) || (g_kind == 2) != pooled)
            why = "a pooled accumulator does not go with a non-pooled model (or the other way round)";
        else if (pooled && ((int)var.size() != l.M || memcmp(var.data(), variance, (size_t)l.M * 4) != 0))
            why = "the global model variance differs from the model's";
    }
    if (why) {
        amx::set_error("%s: '%s': %s", who, path, why);
        return AMX_ERR_INVALID;
    }
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: '%s' is truncated or is not an accumulator of this shape", who, path);
    std::copy(tmp.begin(), tmp.end(), acc);
    return AMX_OK;
}

int amx_cmllr_combine(const amx_cmllr_shape* shape, const float* variance, double* acc, const amx_cmllr_shape* other_shape,
                      const float* other_variance, const double* other_acc, double weight) {
    const char* who = "amx_cmllr_combine";
    AMX_TRY(check_host_args(shape, variance, acc, who));
    AMX_TRY(check_host_args(other_shape, other_variance, other_acc, who));
    AMX_REQUIRE(shape->feature_dim == other_shape->feature_dim, AMX_ERR_INVALID, "%s: feature dimensions %d and %d differ", who, shape->feature_dim,
                other_shape->feature_dim);
    AMX_REQUIRE(shape->model_dim == other_shape->model_dim, AMX_ERR_INVALID, "%s: model dimensions %d and %d differ", who, shape->model_dim,
                other_shape->model_dim);
    AMX_REQUIRE((shape->pooled != 0) == (other_shape->pooled != 0), AMX_ERR_INVALID,
                "%s: a pooled accumulator (global variance optimization) cannot be combined with a non-pooled one", who);
    if (shape->pooled)
        AMX_REQUIRE(memcmp(variance, other_variance, (size_t)shape->model_dim * sizeof(float)) == 0, AMX_ERR_INVALID,
                    "%s: the global model variances differ", who);
    // every member is `this += other * weight` with the product stored first (Vector / Matrix temporaries): two roundings in both builds
    const CmllrLayout l = cmllr_layout(shape);
    for (long c = 0; c < l.size; ++c) {
        const double p = other_acc[c] * weight;
        acc[c] += p;
    }
    return AMX_OK;
}

int amx_cmllr_estimate(const amx_cmllr_shape* shape, const float* variance, const double* acc, int iterations, double min_obs_weight, int criterion,
                       const float* initial, int initial_cols, float* transform_out, double* transform64_out, double* iterations_out,
                       int* estimated) {
    const char* who = "amx_cmllr_estimate";
    AMX_REQUIRE(criterion != AMX_CMLLR_HLDA, AMX_ERR_UNSUPPORTED,
                "%s: criterion hlda (optimization-criterion = hlda) is not supported: only naive and mmi-prime are", who);
    AMX_REQUIRE(criterion == AMX_CMLLR_NAIVE || criterion == AMX_CMLLR_MMI_PRIME, AMX_ERR_INVALID, "%s: unknown criterion %d", who, criterion);
    AMX_TRY(check_host_args(shape, variance, acc, who));
    AMX_REQUIRE(transform_out && iterations >= 0, AMX_ERR_INVALID, "%s: NULL transform_out or negative iterations", who);
    const CmllrLayout l = cmllr_layout(shape);
    const int         R = l.R, M = l.M, F = l.F;
    AMX_REQUIRE(!initial || initial_cols == F || initial_cols == R, AMX_ERR_INVALID, "%s: the initial transform has %d columns, neither %d nor %d", who,
                initial_cols, F, R);
    Mat T(M, R);   // :169-174 identity, or the initial transform widened, a zero column in front of an F-column one (:197-199)
    for (int i = 0; i < M; ++i) {
        if (!initial)
            T.at(i, i + 1) = 1.0;
        else
            for (int j = 0; j < initial_cols; ++j)
                T.at(i, j + (initial_cols == F ? 1 : 0)) = (double)initial[(size_t)i * initial_cols + j];
    }
    auto give = [&](int est) {
        for (size_t e = 0; e < T.a.size(); ++e) {
            transform_out[e] = (float)T.a[e];
            if (transform64_out)
                transform64_out[e] = T.a[e];
        }
        if (estimated)
            *estimated = est;
        return AMX_OK;
    };
    const Finalized f = finalize(l, shape->pooled != 0, variance, acc);
    if (criterion != AMX_CMLLR_NAIVE && f.beta < min_obs_weight)   // :204-205
        return give(0);
    std::vector<Mat> gInverse = f.G;
    for (int i = 0; i < M; ++i)
        AMX_REQUIRE(invert(gInverse[i]), AMX_ERR_INVALID, "%s: G of component %d is singular (beta %g)", who, i, f.beta);
    if (criterion == AMX_CMLLR_NAIVE) {   // :226-230
        for (int i = 0; i < M; ++i) {
            const Vec row = mat_vec(gInverse[i], f.k[i]);
            std::copy(row.begin(), row.end(), &T.at(i, 0));
        }
        return give(1);
    }
    AMX_REQUIRE(f.beta != 0, AMX_ERR_INVALID, "%s: beta is zero", who);
    const Mat gc = global_covariance(f, R);   // F x F
    auto      linear = [&]() {
        Mat lt(M, F);
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < F; ++j)
                lt.at(i, j) = T.at(i, j + 1);
        return lt;
    };
    Mat hct = mat_mat(linear(), gc);                  // halfCovarianceTransposed, M x F (:241)
    Mat tc  = mat_mat(linear(), transpose(hct));      // transformedCovariance, M x M (:242)
    for (int it = 0; it < iterations; ++it) {
        for (int row = 0; row < M; ++row) {
            Mat lt   = linear();
            Mat pinv = M < F ? tc : lt;   // :252-257
            AMX_REQUIRE(invert(pinv), AMX_ERR_INVALID, "%s: iteration %d, row %d: the %s is singular", who, it, row,
                        M < F ? "transformed covariance" : "linear transform");
            Vec col((size_t)M);
            for (int m = 0; m < M; ++m)
                col[m] = pinv.at(m, row);
            Vec cof((size_t)R, 0.0);   // :262-267
            if (M < F) {
                const Vec c = mat_vec(transpose(hct), col);
                std::copy(c.begin(), c.end(), cof.begin() + 1);
            }
            else
                std::copy(col.begin(), col.end(), cof.begin() + 1);
            double      e1 = 0.0, e2 = 0.0;   // :270-276
            const Mat&  gi = gInverse[row];
            const Vec&  kr = f.k[row];
            for (int j = 0; j < R; ++j)
                for (int k = 0; k < R; ++k) {
                    e1 += cof[j] * gi.at(j, k) * cof[k];
                    e2 += cof[j] * gi.at(j, k) * kr[k];
                }
            const double beta = f.beta;
            const double a1 = (-e2 + std::sqrt(e2 * e2 + 4 * e1 * beta)) / (2 * e1);   // :279-280
            const double a2 = (-e2 - std::sqrt(e2 * e2 + 4 * e1 * beta)) / (2 * e1);
            // :283-284: `1 / 2` is an integer division, the quadratic term is 0 * alpha * alpha * epsilon1
            const double l1 = beta * std::log(std::abs(a1 * e1 + e2)) - (1 / 2) * a1 * a1 * e1;
            const double l2 = beta * std::log(std::abs(a2 * e1 + e2)) - (1 / 2) * a2 * a2 * e1;
            const double alpha = l1 > l2 ? a1 : a2;
            Vec rhs((size_t)R);   // :288
            for (int j = 0; j < R; ++j) {
                const double p = cof[j] * alpha;
                rhs[j]         = p + kr[j];
            }
            const Vec new_row = mat_vec(gi, rhs);
            std::copy(new_row.begin(), new_row.end(), &T.at(row, 0));
            // :291-297
            const Vec nrl(new_row.begin() + 1, new_row.end());
            std::copy(nrl.begin(), nrl.end(), &lt.at(row, 0));
            const Vec nrhc = mat_vec(gc, nrl);
            std::copy(nrhc.begin(), nrhc.end(), &hct.at(row, 0));
            const Vec tr = mat_vec(hct, nrl);
            std::copy(tr.begin(), tr.end(), &tc.at(row, 0));
            const Vec tcol = mat_vec(lt, nrhc);
            for (int m = 0; m < M; ++m)
                tc.at(m, row) = tcol[m];
        }
        if (iterations_out)
            std::copy(T.a.begin(), T.a.end(), iterations_out + (size_t)it * M * R);
    }
    return give(1);
}

int amx_cmllr_score(const amx_cmllr_shape* shape, const float* variance, const double* acc, const float* transform, int criterion,
                    double* score_out) {
    const char* who = "amx_cmllr_score";
    AMX_REQUIRE(criterion != AMX_CMLLR_HLDA, AMX_ERR_UNSUPPORTED,
                "%s: criterion hlda (optimization-criterion = hlda) is not supported: only naive and mmi-prime are", who);
    AMX_REQUIRE(criterion == AMX_CMLLR_NAIVE || criterion == AMX_CMLLR_MMI_PRIME, AMX_ERR_INVALID, "%s: unknown criterion %d", who, criterion);
    AMX_TRY(check_host_args(shape, variance, acc, who));
    AMX_REQUIRE(transform && score_out, AMX_ERR_INVALID, "%s: NULL argument", who);
    const CmllrLayout l = cmllr_layout(shape);
    const int         R = l.R, M = l.M, F = l.F;
    const Finalized   f = finalize(l, shape->pooled != 0, variance, acc);
    AMX_REQUIRE(f.beta != 0, AMX_ERR_INVALID, "%s: beta is zero", who);
    double jacobian = 0;
    if (criterion == AMX_CMLLR_MMI_PRIME) {   // :330
        const Mat gc = global_covariance(f, R);
        Mat       lt(M, F);
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < F; ++j)
                lt.at(i, j) = (double)transform[(size_t)i * R + j + 1];
        double ld = 0;
        AMX_REQUIRE(log_determinant(mat_mat(mat_mat(lt, gc), transpose(lt)), &ld), AMX_ERR_INVALID, "%s: the transformed covariance is singular", who);
        jacobian = ld / 2;
    }
    double distance = 0;   // :336-340
    for (int i = 0; i < M; ++i) {
        Vec row((size_t)R);
        for (int j = 0; j < R; ++j)
            row[j] = (double)transform[(size_t)i * R + j];
        const Vec gr = mat_vec(f.G[i], row);
        distance += dot(gr.data(), row.data(), R) / 2 - dot(f.k[i].data(), row.data(), R);
    }
    *score_out = jacobian - distance / f.beta;
    return AMX_OK;
}

// ---- the transform file of AffineFeatureTransformEstimator::postProcess (Speech/AffineFeatureTransformEstimator.cc:124-132): `os <<
// transform` on a Core::XmlOutputStream = Math::Matrix<f32>::write(Core::XmlWriter&) (Math/Matrix.hh:641-647): the declaration the
// stream puts in front, the element with nRows / nColumns, print_raw's rows (every value in std::scientific with the stream's six
// digits, a space behind each, a line per row), the closing tag.  The text between the tags is not wrapped.
int amx_cmllr_transform_write(const char* path, int rows, int cols, const float* transform) {
    const char* who = "amx_cmllr_transform_write";
    AMX_REQUIRE(path && transform, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(rows >= 1 && cols >= 1, AMX_ERR_INVALID, "%s: bad shape %d x %d", who, rows, cols);
    for (size_t e = 0; e < (size_t)rows * cols; ++e)
        AMX_REQUIRE(std::isfinite(transform[e]), AMX_ERR_INVALID, "%s: element %zu is not finite", who, e);
    FILE* f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    bool ok = fprintf(f, "<?xml version=\"1.0\" encoding=\"ISO-8859-1\"?>\n<matrix-f32 nRows=\"%d\" nColumns=\"%d\">\n", rows, cols) > 0;
    for (int i = 0; ok && i < rows; ++i) {
        for (int j = 0; ok && j < cols; ++j)
            ok = fprintf(f, "%e ", (double)transform[(size_t)i * cols + j]) > 0;
        ok = ok && fputc('\n', f) != EOF;
    }
    ok = ok && fputs("</matrix-f32>\n", f) >= 0;
    ok = (fclose(f) == 0) && ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: write to '%s' failed", who, path);
    return AMX_OK;
}

// The reference reads the file through an XML parser: the declaration and comments in front are skipped, the attributes may come in
// either order and with either kind of quote, the values are separated by any white space.  *data: rows x cols floats, amx_free().
int amx_cmllr_transform_read(const char* path, int* rows, int* cols, float** data) {
    const char* who = "amx_cmllr_transform_read";
    AMX_REQUIRE(path && rows && cols && data, AMX_ERR_INVALID, "%s: NULL argument", who);
    *data = nullptr;
    FILE* f = fopen(path, "rb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    std::string text;
    char        buf[4096];
    size_t      n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0)
        text.append(buf, n);
    fclose(f);
    size_t at = 0;
    for (;;) {   // to the element, over the declaration and comments
        at = text.find('<', at);
        AMX_REQUIRE(at != std::string::npos, AMX_ERR_INVALID, "%s: '%s' holds no <matrix-f32> element", who, path);
        if (text.compare(at, 4, "<!--") == 0) {
            const size_t e = text.find("-->", at);
            AMX_REQUIRE(e != std::string::npos, AMX_ERR_INVALID, "%s: '%s': a comment does not end", who, path);
            at = e + 3;
        }
        else if (text.compare(at, 2, "<?") == 0)
            at += 2;
        else
            break;
    }
    const size_t close = text.find('>', at);
    AMX_REQUIRE(text.compare(at, 11, "<matrix-f32") == 0 && close != std::string::npos && strchr(" \t\r\n>", text[at + 11]), AMX_ERR_INVALID,
                "%s: '%s': the root element is not <matrix-f32>", who, path);
    const std::string head = text.substr(at, close - at);
    auto attribute = [&](const char* name, int* out) {
        size_t p = head.find(name);
        if (p == std::string::npos)
            return false;
        p = head.find_first_not_of(" \t\r\n", p + strlen(name));
        if (p == std::string::npos || head[p] != '=')
            return false;
        p = head.find_first_not_of(" \t\r\n", p + 1);
        if (p == std::string::npos || (head[p] != '"' && head[p] != '\''))
            return false;
        char*      end = nullptr;
        const long v   = strtol(head.c_str() + p + 1, &end, 10);
        if (end == head.c_str() + p + 1 || *end != head[p] || v < 1 || v > (1 << 20))
            return false;
        *out = (int)v;
        return true;
    };
    int r = 0, c = 0;
    AMX_REQUIRE(attribute("nRows", &r) && attribute("nColumns", &c), AMX_ERR_INVALID, "%s: '%s': nRows / nColumns are missing or not positive numbers", who,
                path);
    float* out = (float*)malloc((size_t)r * c * sizeof(float));
    AMX_REQUIRE(out, AMX_ERR_INVALID, "%s: out of memory", who);
    const char* p  = text.c_str() + close + 1;
    bool        ok = true;
    for (size_t e = 0; ok && e < (size_t)r * c; ++e) {
        char* end = nullptr;
        out[e]    = strtof(p, &end);
        ok        = end != p;
        p         = end;
    }
    if (ok) {
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')
            ++p;
        ok = strncmp(p, "</matrix-f32>", 13) == 0;
    }
    if (!ok) {
        free(out);
        amx::set_error("%s: '%s' does not hold %d x %d values between its tags (truncated, or more values than it declares)", who, path, r, c);
        return AMX_ERR_INVALID;
    }
    *rows = r, *cols = c, *data = out;
    return AMX_OK;
}

}  // extern "C"
