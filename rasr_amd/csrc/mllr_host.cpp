// mllr_host.cpp -- the host side of MLLR (include/amx.h, section "MLLR"): the accumulator and adaptor files of
// Mm::FullAdaptorViterbiEstimator / Mm::ShiftAdaptorViterbiEstimator and Mm::FullAdaptor / Mm::ShiftAdaptor, and adaptor()
// (Mm/MllrAdaptation.cc:444-531, :671-691, :741-827) on ONE key's part of the flat accumulator that mllr.hip fills.  Nothing here needs a
// device.
//
// estimate restates the reference operation by operation in f64: propagate's recursion (left, right, node = left, node += right),
// the strict threshold, Matrix * Matrix's loop, the walk up `previous`, the silence rule.  One thing is not the reference's bits: the
// pseudo-inverse.  The reference calls dgelsd (an SVD) on G against the identity with rcond = 1e-12; here G is symmetrised and
// decomposed by cyclic Jacobi rotations, pinv = V diag(1 / lambda) V^T over the eigenvalues with |lambda| > rcond * max |lambda|.
// This file is compiled with -ffp-contract=off and follows the reference's build without fused multiply-adds in W = Z * pinv(G).
// Both differences are inside the bar that tests/golden/make_mllr_golden.py measures against the reference's text with OpenBLAS's
// dgelsd in both builds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.hpp"

extern "C++" {
namespace {

constexpr const char* kFullTag       = "full-adaptor-viterbi-estimator";    // MllrAdaptation.hh:405-407
constexpr const char* kShiftTag      = "shift-adaptor-viterbi-estimator";   // :298-300
constexpr const char* kFullAdaptor   = "full-adaptor";                      // :146-148
constexpr const char* kShiftAdaptor  = "shift-adaptor";                     // :118-120
constexpr int         kMllrMaxDim    = 255;
constexpr int         kMllrMaxLeafs  = 4096;
constexpr int         kMllrMaxIds    = 65535;   // Core::BinaryTree::Id is u16 and 65535 its invalidId

bool mllr_shape_ok(const amx_mllr_shape* s) {
    return s && (s->mode == AMX_MLLR_FULL || s->mode == AMX_MLLR_SHIFT) && s->dim >= 1 && s->dim <= kMllrMaxDim && s->n_leafs >= 1 &&
           s->n_leafs <= kMllrMaxLeafs && s->n_keys >= 1;
}

long leaf_size(const amx_mllr_shape* s) {
    const long D = s->dim, R = D + 1;
    return s->mode == AMX_MLLR_SHIFT ? 1 + 2 * D : 2 + D * R + R * R;
}

int check_shape(const amx_mllr_shape* shape, const char* who) {
    AMX_REQUIRE(shape, AMX_ERR_INVALID, "%s: NULL shape", who);
    AMX_REQUIRE(shape->mode != AMX_MLLR_BAND && shape->mode != AMX_MLLR_SEMI_TIED, AMX_ERR_UNSUPPORTED,
                "%s: mode %s (mllr-adaptation, MODULE_ADAPT_ADVANCED) is not supported: only full and shift are", who,
                shape->mode == AMX_MLLR_BAND ? "band" : "semi-tied");
    AMX_REQUIRE(mllr_shape_ok(shape), AMX_ERR_INVALID, "%s: bad shape (mode %d, dim %d in [1, %d], n_leafs %d in [1, %d], n_keys %d)", who, shape->mode,
                shape->dim, kMllrMaxDim, shape->n_leafs, kMllrMaxLeafs, shape->n_keys);
    return AMX_OK;
}

typedef std::vector<double> Vec;

// ---- the pseudo-inverse of Math::Lapack::pseudoInvert (Math/Lapack/Svd.cc:21-99) for a (nearly) symmetric positive semi-definite g
// [n x n]: cyclic Jacobi on (g + g^T) / 2, eigenvalues with |lambda| <= rcond * max |lambda| dropped as dgelsd drops singular values
void pseudo_invert(const double* g, int n, double rcond, double* out) {
    Vec a((size_t)n * n), v((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j)
            a[(size_t)i * n + j] = 0.5 * (g[(size_t)i * n + j] + g[(size_t)j * n + i]);
        v[(size_t)i * n + i] = 1.0;
    }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                (i == j ? diag : off) += a[(size_t)i * n + j] * a[(size_t)i * n + j];
        if (!(off > 1e-60 * diag))   // converged (or not finite)
            break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                if (apq == 0.0)
                    continue;
                const double theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
                const double t     = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {   // columns p, q
                    const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * akp - s * akq;
                    a[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {   // rows p, q
                    const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
                    a[(size_t)p * n + k] = c * apk - s * aqk;
                    a[(size_t)q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * vkp - s * vkq;
                    v[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    double top = 0.0;
    for (int i = 0; i < n; ++i)
        top = std::max(top, std::fabs(a[(size_t)i * n + i]));
    Vec inv((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double l = a[(size_t)i * n + i];
        inv[i]         = std::fabs(l) > rcond * top ? 1.0 / l : 0.0;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k)
                s += v[(size_t)i * n + k] * inv[k] * v[(size_t)j * n + k];
            out[(size_t)i * n + j] = s;
        }
}

// w [D x R] = z [D x R] * pinv(g [R x R]): Matrix::operator*(Matrix), Math/Matrix.hh:496-508
void z_times_pinv(const double* z, const double* g, int D, double rcond, double* w) {
    const int R = D + 1;
    Vec       gi((size_t)R * R);
    pseudo_invert(g, R, rcond, gi.data());
    for (int n = 0; n < D; ++n)
        for (int m = 0; m < R; ++m) {
            double s = 0;
            for (int k = 0; k < R; ++k)
                s += z[(size_t)n * R + k] * gi[(size_t)k * R + m];
            w[(size_t)n * R + m] = s;
        }
}

struct Out {   // little-endian host
    FILE* f;
    bool  ok = true;
    template<class T>
    void put(T v) {
        ok = ok && fwrite(&v, sizeof(T), 1, f) == 1;
    }
    void str(const char* s) {   // BinaryOutputStream << std::string: u32 length, bytes
        const uint32_t n = (uint32_t)strlen(s);
        put(n);
        ok = ok && fwrite(s, 1, n, f) == n;
    }
    void vec(const double* v, int n) {   // Math::Vector<f64>::write (Math/Vector.hh:286-290)
        put((uint32_t)n);
        ok = ok && (n == 0 || fwrite(v, 8, (size_t)n, f) == (size_t)n);
    }
    void matrix(const double* m, int r, int c) {   // Math::Matrix<f64>::write (Math/Matrix.hh:560-564): nRows, nColumns, vector of rows
        put((uint32_t)r), put((uint32_t)c), put((uint32_t)r);
        for (int i = 0; i < r; ++i)
            vec(m ? m + (size_t)i * c : nullptr, c);
    }
};

struct In {
    FILE* f;
    template<class T>
    bool get(T* v) {
        return fread(v, sizeof(T), 1, f) == 1;
    }
    bool str(std::string* s) {
        uint32_t n = 0;
        if (!get(&n) || n > 4096)
            return false;
        s->resize(n);
        return n == 0 || fread(&(*s)[0], 1, n, f) == n;
    }
    bool vec(double* v, int n) {   // a vector of exactly n elements
        uint32_t m = 0;
        return get(&m) && (int)m == n && (n == 0 || fread(v, 8, (size_t)n, f) == (size_t)n);
    }
    bool matrix(double* m, int r, int c) {   // a matrix of exactly r x c
        uint32_t a = 0, b = 0, rows = 0;
        if (!(get(&a) && get(&b) && get(&rows)) || (int)a != r || (int)b != c || (int)rows != r)
            return false;
        for (int i = 0; i < r; ++i)
            if (!vec(m + (size_t)i * c, c))
                return false;
        return true;
    }
    bool skip_matrix() {   // any matrix
        uint32_t a = 0, b = 0, rows = 0;
        if (!(get(&a) && get(&b) && get(&rows)) || a > 65536 || b > 65536 || rows != a)
            return false;
        Vec row;
        for (uint32_t i = 0; i < rows; ++i) {
            uint32_t m = 0;
            if (!get(&m) || m != b)
                return false;
            row.resize(m);
            if (m && fread(row.data(), 8, m, f) != m)
                return false;
        }
        return true;
    }
};

}  // namespace
}  // extern "C++"

extern "C" {

long amx_mllr_leaf_size(const amx_mllr_shape* shape) {
    return mllr_shape_ok(shape) ? leaf_size(shape) : 0;
}

long amx_mllr_key_size(const amx_mllr_shape* shape) {
    return mllr_shape_ok(shape) ? leaf_size(shape) * shape->n_leafs : 0;
}

int amx_mllr_accumulator_write(const amx_mllr_shape* shape, const double* acc, const char* cluster_id, double min_observation,
                               double min_silence_observation, int n_count, const double* node_count, int n_map_ids, const int* map_ids,
                               const char* path) {
    const char* who = "amx_mllr_accumulator_write";
    AMX_TRY(check_shape(shape, who));
    AMX_REQUIRE(acc && cluster_id && path, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(n_count >= 0 && (n_count == 0 || node_count), AMX_ERR_INVALID, "%s: n_count %d without node_count", who, n_count);
    AMX_REQUIRE(n_map_ids >= 0 && (n_map_ids == 0 || map_ids), AMX_ERR_INVALID, "%s: n_map_ids %d without map_ids", who, n_map_ids);
    for (int i = 0; i < n_map_ids; ++i)
        AMX_REQUIRE(map_ids[i] >= 0 && map_ids[i] < kMllrMaxIds && (i == 0 || map_ids[i] > map_ids[i - 1]), AMX_ERR_INVALID,
                    "%s: map_ids[%d] = %d: the ids must ascend within [0, %d)", who, i, map_ids[i], kMllrMaxIds);
    const int  D = shape->dim, R = D + 1, L = shape->n_leafs;
    const long ls = leaf_size(shape);
    const bool shift = shape->mode == AMX_MLLR_SHIFT;
    FILE*      f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    Out o{f};
    o.str(shift ? kShiftTag : kFullTag);   // Core::IoRef::write
    o.str(cluster_id);                     // AdaptorEstimator::write :247-250
    o.put((uint32_t)D);
    o.vec(node_count, n_count);
    o.put(min_observation), o.put(min_silence_observation);
    if (shift) {   // :533-538
        o.put((uint32_t)L);
        for (int l = 0; l < L; ++l)
            o.put(acc[l * ls]);
        for (int part = 0; part < 2; ++part) {
            o.put((uint32_t)L);
            for (int l = 0; l < L; ++l)
                o.vec(acc + l * ls + 1 + (long)part * D, D);
        }
        const Vec zeros((size_t)D, 0.0);
        o.put((uint32_t)n_map_ids);
        for (int i = 0; i < n_map_ids; ++i) {
            o.put((uint16_t)map_ids[i]);
            o.matrix(zeros.data(), 1, D);   // init() leaves a 1 x D row of zeros (:339-342)
        }
    }
    else {   // :829-834, every accumulator :279-282
        o.put((uint32_t)L);
        for (int l = 0; l < L; ++l) {
            o.matrix(acc + l * ls + 1, D, R);
            o.put(acc[l * ls]);
        }
        o.put((uint32_t)L);
        for (int l = 0; l < L; ++l) {
            o.matrix(acc + l * ls + 2 + (long)D * R, R, R);
            o.put(acc[l * ls + 1 + (long)D * R]);
        }
        o.put((uint32_t)n_map_ids);
        for (int i = 0; i < n_map_ids; ++i) {
            o.put((uint16_t)map_ids[i]);
            o.matrix(nullptr, 0, 0);   // init() leaves Matrix() (:577)
        }
    }
    const bool ok = (fclose(f) == 0) && o.ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: write to '%s' failed", who, path);
    return AMX_OK;
}

int amx_mllr_accumulator_read(const amx_mllr_shape* shape, const char* path, double* acc, double* min_observation,
                              double* min_silence_observation) {
    const char* who = "amx_mllr_accumulator_read";
    AMX_TRY(check_shape(shape, who));
    AMX_REQUIRE(acc && path, AMX_ERR_INVALID, "%s: NULL argument", who);
    const int  D = shape->dim, R = D + 1, L = shape->n_leafs;
    const long ls = leaf_size(shape);
    const bool shift = shape->mode == AMX_MLLR_SHIFT;
    FILE*      f = fopen(path, "rb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    In          in{f};
    const char* why = nullptr;
    Vec         tmp((size_t)ls * L, 0.0);
    std::string tag, cluster;
    uint32_t    dim = 0, n = 0;
    double      mo = 0, ms = 0;
    bool        ok = in.str(&tag);
    if (ok && tag != (shift ? kShiftTag : kFullTag)) {
        why = shift ? "the type tag is not 'shift-adaptor-viterbi-estimator'" : "the type tag is not 'full-adaptor-viterbi-estimator'";
        ok  = false;
    }
    ok = ok && in.str(&cluster) && in.get(&dim);
    if (ok && (int)dim != D) {
        why = "the dimension differs from the shape's";
        ok  = false;
    }
    if (ok && (ok = in.get(&n) && n <= (uint32_t)kMllrMaxIds)) {   // count_
        Vec c(n);
        ok = n == 0 || fread(c.data(), 8, n, f) == n;
    }
    ok = ok && in.get(&mo) && in.get(&ms);
    for (int part = 0; ok && part < (shift ? 3 : 2); ++part) {
        ok = in.get(&n);
        if (ok && (int)n != L) {
            why = "the number of leaf accumulators differs from the shape's n_leafs";
            ok  = false;
        }
        for (int l = 0; ok && l < L; ++l) {
            double* a = &tmp[(size_t)l * ls];
            if (shift)
                ok = part == 0 ? in.get(a) : in.vec(a + 1 + (long)(part - 1) * D, D);
            else if (part == 0)
                ok = in.matrix(a + 1, D, R) && in.get(a);
            else
                ok = in.matrix(a + 2 + (long)D * R, R, R) && in.get(a + 1 + (long)D * R);
        }
    }
    if (ok && (ok = in.get(&n) && n <= (uint32_t)kMllrMaxIds))   // w_ / shift_
        for (uint32_t i = 0; ok && i < n; ++i) {
            uint16_t id = 0;
            ok          = in.get(&id) && in.skip_matrix();
        }
    fclose(f);
    if (why) {
        amx::set_error("%s: '%s': %s", who, path, why);
        return AMX_ERR_INVALID;
    }
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: '%s' is truncated or is not an accumulator of this shape", who, path);
    std::copy(tmp.begin(), tmp.end(), acc);
    if (min_observation)
        *min_observation = mo;
    if (min_silence_observation)
        *min_silence_observation = ms;
    return AMX_OK;
}

int amx_mllr_estimate(const amx_mllr_shape* shape, const double* acc, const amx_mllr_tree* tree, int n_mixtures, const int* leaf_of_mixture,
                      double min_observation, double min_silence_observation, double rcond, int* n_matrices, int* matrix_ids, double* matrices,
                      int* matrix_of_mixture, double* node_count, int* flags) {
    const char* who = "amx_mllr_estimate";
    AMX_TRY(check_shape(shape, who));
    AMX_REQUIRE(acc && tree && leaf_of_mixture && n_matrices && matrix_ids && matrices && matrix_of_mixture, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(n_mixtures >= 1, AMX_ERR_INVALID, "%s: n_mixtures %d is not positive", who, n_mixtures);
    AMX_REQUIRE(min_observation >= 0 && min_silence_observation >= 0, AMX_ERR_INVALID, "%s: a negative threshold", who);
    if (!(rcond > 0))
        rcond = 1e-12;   // Math/Lapack/Svd.hh:27
    const int  D = shape->dim, R = D + 1, L = shape->n_leafs, N = tree->n_ids;
    const long ls = leaf_size(shape);
    const bool shift = shape->mode == AMX_MLLR_SHIFT;
    const long per   = shift ? D : (long)D * R;
    // ---- the tree's arrays describe a tree
    AMX_REQUIRE(N >= 1 && tree->n_silence >= 0 && N + tree->n_silence <= kMllrMaxIds, AMX_ERR_INVALID,
                "%s: bad tree: %d ids and %d silence mixtures (ids are 16 bits wide, %d is invalidId)", who, N, tree->n_silence, kMllrMaxIds);
    AMX_REQUIRE(tree->left && tree->right && tree->previous && tree->leaf_number && (tree->n_leaf_list == 0 || tree->leaf_list) &&
                        (tree->n_silence == 0 || tree->silence_mixtures),
                AMX_ERR_INVALID, "%s: bad tree: a NULL array", who);
    AMX_REQUIRE(tree->root >= 0 && tree->root < N, AMX_ERR_INVALID, "%s: bad tree: root %d is outside [0, %d)", who, tree->root, N);
    AMX_REQUIRE(tree->n_leaf_list >= 0 && tree->n_leaf_list <= N, AMX_ERR_INVALID, "%s: bad tree: %d leaf-list entries for %d ids", who, tree->n_leaf_list, N);
    for (int m = 0; m < n_mixtures; ++m)
        AMX_REQUIRE(leaf_of_mixture[m] >= 0 && leaf_of_mixture[m] < L, AMX_ERR_INVALID, "%s: mixture %d: leaf %d is outside [0, %d)", who, m,
                    leaf_of_mixture[m], L);
    for (int s = 0; s < tree->n_silence; ++s)
        AMX_REQUIRE(tree->silence_mixtures[s] >= 0 && tree->silence_mixtures[s] < n_mixtures && (s == 0 || tree->silence_mixtures[s] > tree->silence_mixtures[s - 1]),
                    AMX_ERR_INVALID, "%s: silence mixture %d (entry %d) is outside [0, %d) or does not ascend", who, tree->silence_mixtures[s], s, n_mixtures);
    // propagate's recursion (:228-248) without the call stack: every id reached from the root in post-order, each exactly once
    std::vector<int>  order, stack{tree->root};
    std::vector<char> seen((size_t)N, 0), expanded((size_t)N, 0);
    seen[(size_t)tree->root] = 1;
    while (!stack.empty()) {
        const int id = stack.back();
        if (tree->leaf_number[id] >= 0) {
            AMX_REQUIRE(tree->leaf_number[id] < L, AMX_ERR_INVALID, "%s: bad tree: node %d: leaf number %d is outside [0, %d)", who, id, tree->leaf_number[id], L);
            order.push_back(id);
            stack.pop_back();
            continue;
        }
        if (expanded[(size_t)id]) {
            order.push_back(id);
            stack.pop_back();
            continue;
        }
        expanded[(size_t)id] = 1;
        const int l = tree->left[id], r = tree->right[id];
        AMX_REQUIRE(l >= 0 && l < N && r >= 0 && r < N && l != r, AMX_ERR_INVALID, "%s: bad tree: inner node %d has children %d and %d", who, id, l, r);
        AMX_REQUIRE(!seen[(size_t)l] && !seen[(size_t)r], AMX_ERR_INVALID, "%s: bad tree: a child of node %d is reached twice", who, id);
        seen[(size_t)l] = seen[(size_t)r] = 1;
        stack.push_back(r);   // left is finished first
        stack.push_back(l);
    }
    for (int p = 0; p < tree->n_leaf_list; ++p) {
        const int id = tree->leaf_list[p];
        AMX_REQUIRE(id >= 0 && id < N && seen[(size_t)id] && tree->leaf_number[id] >= 0, AMX_ERR_INVALID,
                    "%s: bad tree: leaf-list entry %d (node %d) is not a leaf below the root", who, p, id);
        int at = id, steps = 0;   // `previous` leads to the root
        while (at != tree->root) {
            at = tree->previous[at];
            AMX_REQUIRE(at >= 0 && at < N && ++steps <= N, AMX_ERR_INVALID, "%s: bad tree: `previous` of leaf node %d does not lead to the root", who, id);
        }
    }
    // ---- propagate: nodeData[id] = leafData[leafNumber(id)] | nodeData[left] += nodeData[right]
    std::vector<Vec> node((size_t)N);
    for (int id : order) {
        if (tree->leaf_number[id] >= 0)
            node[(size_t)id].assign(acc + (long)tree->leaf_number[id] * ls, acc + (long)(tree->leaf_number[id] + 1) * ls);
        else {
            node[(size_t)id] = node[(size_t)tree->left[id]];
            const Vec& r     = node[(size_t)tree->right[id]];
            for (long c = 0; c < ls; ++c)
                node[(size_t)id][(size_t)c] += r[(size_t)c];
        }
    }
    // count_[id] = g[id].count() | count[id]; an id that is not below the root keeps a fresh accumulator's 0
    Vec count((size_t)N, 0.0);
    for (int id : order)
        count[(size_t)id] = node[(size_t)id][shift ? 0 : (size_t)(1 + (long)D * R)];
    if (node_count)
        std::copy(count.begin(), count.end(), node_count);
    auto estimate_from = [&](const double* a, double* out) {   // :683-685 | :372-373
        if (shift)
            for (int d = 0; d < D; ++d)
                out[d] = a[1 + D + d] / a[1 + d];
        else
            z_times_pinv(a + 1, a + 2 + (long)D * R, D, rcond, out);
    };
    auto unit = [&](double* out) {   // adaptationUnitMatrix (:24-29) | a row of zeros
        std::fill(out, out + per, 0.0);
        if (!shift)
            for (int d = 0; d < D; ++d)
                out[(long)d * R + d + 1] = 1.0;
    };
    std::map<int, Vec> mats;
    std::vector<int>   matrix_id((size_t)L, 0);   // std::vector<NodeId> matrixId(nLeafs_)
    int                fl = 0;
    const int          root = tree->root;
    if (count[(size_t)root] <= min_observation) {   // :752-764
        fl |= AMX_MLLR_ROOT_FALLBACK;
        mats[root].resize((size_t)per);
        unit(mats[root].data());
        for (int p = 0; p < tree->n_leaf_list; ++p)
            matrix_id[(size_t)tree->leaf_number[tree->leaf_list[p]]] = root;
    }
    else
        for (int p = 0; p < tree->n_leaf_list; ++p) {   // :766-781
            int       id   = tree->leaf_list[p];
            const int leaf = tree->leaf_number[id];
            while (id != root && count[(size_t)id] <= min_observation)
                id = tree->previous[id];
            AMX_REQUIRE(count[(size_t)id] > min_observation && !node[(size_t)id].empty(), AMX_ERR_INVALID,
                        "%s: bad tree: `previous` of leaf %d leads to node %d, which is not above it", who, leaf, id);
            if (!mats.count(id)) {
                mats[id].resize((size_t)per);
                estimate_from(node[(size_t)id].data(), mats[id].data());
            }
            matrix_id[(size_t)leaf] = id;
        }
    int silence_id = N;   // numberOfNodes() + numberOfLeafs()
    for (int s = 0; s < tree->n_silence; ++s, ++silence_id) {   // :788-805
        const int     leaf = leaf_of_mixture[tree->silence_mixtures[s]];
        const double* a    = acc + (long)leaf * ls;
        mats[silence_id].resize((size_t)per);
        if (a[shift ? 0 : 1 + (long)D * R] > min_silence_observation)
            estimate_from(a, mats[silence_id].data());
        else {
            fl |= AMX_MLLR_SILENCE_FALLBACK;
            unit(mats[silence_id].data());
        }
        matrix_id[(size_t)leaf] = silence_id;
    }
    for (int m = 0; m < n_mixtures; ++m)   // :811-813
        matrix_of_mixture[m] = matrix_id[(size_t)leaf_of_mixture[m]];
    int n = 0;
    for (const auto& kv : mats) {
        matrix_ids[n] = kv.first;
        std::copy(kv.second.begin(), kv.second.end(), matrices + (long)n * per);
        ++n;
    }
    *n_matrices = n;
    if (flags)
        *flags = fl;
    return AMX_OK;
}

int amx_mllr_adaptor_write(const amx_mllr_shape* shape, const char* cluster_id, int n_matrices, const int* matrix_ids, const double* matrices,
                           int n_mixtures, const int* matrix_of_mixture, const char* path) {
    const char* who = "amx_mllr_adaptor_write";
    AMX_TRY(check_shape(shape, who));
    AMX_REQUIRE(cluster_id && matrix_ids && matrices && matrix_of_mixture && path, AMX_ERR_INVALID, "%s: NULL argument", who);
    AMX_REQUIRE(n_matrices >= 0 && n_mixtures >= 0, AMX_ERR_INVALID, "%s: negative count", who);
    for (int i = 0; i < n_matrices; ++i)
        AMX_REQUIRE(matrix_ids[i] >= 0 && matrix_ids[i] < kMllrMaxIds && (i == 0 || matrix_ids[i] > matrix_ids[i - 1]), AMX_ERR_INVALID,
                    "%s: matrix_ids[%d] = %d: the ids must ascend within [0, %d)", who, i, matrix_ids[i], kMllrMaxIds);
    for (int m = 0; m < n_mixtures; ++m)
        AMX_REQUIRE(matrix_of_mixture[m] >= 0 && matrix_of_mixture[m] < kMllrMaxIds, AMX_ERR_INVALID, "%s: mixture %d: matrix id %d", who, m, matrix_of_mixture[m]);
    const int  D = shape->dim, R = D + 1;
    const bool shift = shape->mode == AMX_MLLR_SHIFT;
    FILE*      f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    Out o{f};
    o.str(shift ? kShiftAdaptor : kFullAdaptor);
    o.str(cluster_id);   // Adaptor::write :38-41
    o.put((uint32_t)n_matrices);
    for (int i = 0; i < n_matrices; ++i) {
        o.put((uint16_t)matrix_ids[i]);
        if (shift)
            o.matrix(matrices + (long)i * D, 1, D);
        else
            o.matrix(matrices + (long)i * D * R, D, R);
    }
    o.put((uint32_t)n_mixtures);
    for (int m = 0; m < n_mixtures; ++m)
        o.put((uint16_t)matrix_of_mixture[m]);
    const bool ok = (fclose(f) == 0) && o.ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: write to '%s' failed", who, path);
    return AMX_OK;
}

int amx_mllr_adaptor_read(const amx_mllr_shape* shape, const char* path, int max_matrices, int* n_matrices, int* matrix_ids, double* matrices,
                          int n_mixtures, int* matrix_of_mixture) {
    const char* who = "amx_mllr_adaptor_read";
    AMX_TRY(check_shape(shape, who));
    AMX_REQUIRE(path && n_matrices && matrix_ids && matrices && matrix_of_mixture && max_matrices >= 0 && n_mixtures >= 0, AMX_ERR_INVALID,
                "%s: NULL argument or negative count", who);
    const int  D = shape->dim, R = D + 1;
    const bool shift = shape->mode == AMX_MLLR_SHIFT;
    FILE*      f = fopen(path, "rb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    In          in{f};
    const char* why = nullptr;
    std::string tag, cluster;
    uint32_t    n = 0, nm = 0;
    bool        ok = in.str(&tag);
    if (ok && tag != (shift ? kShiftAdaptor : kFullAdaptor)) {
        why = shift ? "the type tag is not 'shift-adaptor'" : "the type tag is not 'full-adaptor'";
        ok  = false;
    }
    ok = ok && in.str(&cluster) && in.get(&n);
    if (ok && n > (uint32_t)max_matrices) {
        why = "more matrices than the caller has room for";
        ok  = false;
    }
    Vec              mats((size_t)(ok ? n : 0) * (shift ? D : D * R));
    std::vector<int> ids(ok ? n : 0), index((size_t)n_mixtures);
    for (uint32_t i = 0; ok && i < n; ++i) {
        uint16_t id = 0;
        ok          = in.get(&id) && (shift ? in.matrix(&mats[(size_t)i * D], 1, D) : in.matrix(&mats[(size_t)i * D * R], D, R));
        ids[i]      = id;
        if (!ok && !feof(f))
            why = "a matrix does not have the shape's dimension";
    }
    ok = ok && in.get(&nm);
    if (ok && (int)nm != n_mixtures) {
        why = "the index vector's length differs from n_mixtures";
        ok  = false;
    }
    for (int m = 0; ok && m < n_mixtures; ++m) {
        uint16_t id = 0;
        ok          = in.get(&id);
        index[m]    = id;
    }
    fclose(f);
    if (why) {
        amx::set_error("%s: '%s': %s", who, path, why);
        return AMX_ERR_INVALID;
    }
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: '%s' is truncated or is not an adaptor of this shape", who, path);
    *n_matrices = (int)n;
    std::copy(ids.begin(), ids.end(), matrix_ids);
    std::copy(mats.begin(), mats.end(), matrices);
    std::copy(index.begin(), index.end(), matrix_of_mixture);
    return AMX_OK;
}

}  // extern "C"
