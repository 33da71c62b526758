// Stand-alone host program for the host side of the MLLR section of include/amx.h: it compiles mllr_host.cpp into a program of its own
// (no device is touched), so that tests/test_mllr.py can run it under the host sanitizers.
//   host_mllr_test case.bin directory bar_abs bar_rel
// case.bin (written by the test from tests/golden/ref_mllr.npz): int32 mode, D, n_leafs, n_mixtures, n_ids, root, n_leaf_list, n_silence,
// n_matrices | int32 left, right, previous, leaf_number [n_ids] | leaf_list | silence_mixtures | leaf_of_mixture | f64 min_obs, min_sil |
// f64 key 0 | int32 the reference's matrix ids, index vector | f64 its matrices; directory/key0.acc and directory/key0.adaptor hold the
// reference's accumulator and adaptor files of key 0.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rasr_amd/csrc/mllr_host.cpp"

static std::string g_error;
namespace amx {
void set_error(const char* fmt, ...) {
    char    buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace amx

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            printf("host_mllr_test: line %d: %s failed (last error: %s)\n", __LINE__, #cond, g_error.c_str()); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

static std::vector<unsigned char> slurp(const std::string& path) {
    std::vector<unsigned char> out;
    FILE*                      f = fopen(path.c_str(), "rb");
    if (!f)
        return out;
    unsigned char buf[4096];
    size_t        n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0)
        out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

static bool spill(const std::string& path, const unsigned char* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f)
        return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

static bool ints(FILE* f, std::vector<int>& v, int n) {
    v.resize((size_t)n);
    return n == 0 || fread(v.data(), 4, (size_t)n, f) == (size_t)n;
}

int main(int argc, char** argv) {
    if (argc != 5) {
        printf("usage: host_mllr_test case.bin directory bar_abs bar_rel\n");
        return 2;
    }
    const std::string dir = argv[2];
    const double      bar_abs = atof(argv[3]), bar_rel = atof(argv[4]);
    FILE*             in = fopen(argv[1], "rb");
    CHECK(in);
    int32_t head[9];
    CHECK(fread(head, 4, 9, in) == 9);
    const int mode = head[0], D = head[1], L = head[2], n_mix = head[3], n_ids = head[4], root = head[5], n_ll = head[6], n_sil = head[7], n_ref = head[8];
    std::vector<int> left, right, prev, leafno, llist, sil, lom, ref_ids, ref_index;
    CHECK(ints(in, left, n_ids) && ints(in, right, n_ids) && ints(in, prev, n_ids) && ints(in, leafno, n_ids) && ints(in, llist, n_ll) &&
          ints(in, sil, n_sil) && ints(in, lom, n_mix));
    double thr[2];
    CHECK(fread(thr, 8, 2, in) == 2);
    amx_mllr_shape shape{mode, D, L, 1};
    const long     size = amx_mllr_key_size(&shape), per = mode == AMX_MLLR_SHIFT ? D : (long)D * (D + 1);
    CHECK(size > 0);
    std::vector<double> acc((size_t)size), ref_mats((size_t)(per * n_ref));
    CHECK(fread(acc.data(), 8, (size_t)size, in) == (size_t)size);
    CHECK(ints(in, ref_ids, n_ref) && ints(in, ref_index, n_mix));
    CHECK(fread(ref_mats.data(), 8, ref_mats.size(), in) == ref_mats.size());
    fclose(in);
    amx_mllr_tree tree{n_ids, root, left.data(), right.data(), prev.data(), leafno.data(), n_ll, llist.data(), n_sil, sil.data()};

    // ---- the accumulator file: the reference's bytes, and back
    std::vector<int> map_ids;   // init() puts every id below the root into the map
    for (int i = 0; i < n_ids; ++i)
        if (i == root || prev[i] >= 0)
            map_ids.push_back(i);
    const std::string p = dir + "/mine.acc";
    CHECK(amx_mllr_accumulator_write(&shape, acc.data(), "key0", 1000.0, 500.0, 0, nullptr, (int)map_ids.size(), map_ids.data(), p.c_str()) == AMX_OK);
    const std::vector<unsigned char> ref_file = slurp(dir + "/key0.acc"), mine = slurp(p);
    CHECK(!ref_file.empty() && mine == ref_file);
    std::vector<double> back((size_t)size);
    double              mo = 0, ms = 0;
    CHECK(amx_mllr_accumulator_read(&shape, p.c_str(), back.data(), &mo, &ms) == AMX_OK);
    CHECK(memcmp(back.data(), acc.data(), (size_t)size * 8) == 0 && mo == 1000.0 && ms == 500.0);
    for (size_t cut : {(size_t)0, (size_t)3, (size_t)20, (size_t)60, mine.size() / 2, mine.size() - 1}) {   // every truncation is refused
        CHECK(spill(p, mine.data(), cut));
        CHECK(amx_mllr_accumulator_read(&shape, p.c_str(), back.data(), nullptr, nullptr) == AMX_ERR_INVALID);
    }
    {
        std::vector<unsigned char> bad = mine;
        bad[5] ^= 1;   // the tag
        CHECK(spill(p, bad.data(), bad.size()));
        CHECK(amx_mllr_accumulator_read(&shape, p.c_str(), back.data(), nullptr, nullptr) == AMX_ERR_INVALID && g_error.find("type tag") != std::string::npos);
        amx_mllr_shape other = shape;
        other.dim            = D + 1;
        std::vector<double> wide((size_t)amx_mllr_key_size(&other));
        CHECK(spill(p, mine.data(), mine.size()));
        CHECK(amx_mllr_accumulator_read(&other, p.c_str(), wide.data(), nullptr, nullptr) == AMX_ERR_INVALID && g_error.find("dimension") != std::string::npos);
        other         = shape;
        other.n_leafs = L + 1;
        wide.assign((size_t)amx_mllr_key_size(&other), 0.0);
        CHECK(amx_mllr_accumulator_read(&other, p.c_str(), wide.data(), nullptr, nullptr) == AMX_ERR_INVALID && g_error.find("leaf") != std::string::npos);
    }

    // ---- the estimate: ids, index vector and counts in every bit, W within the bar
    const int           cap = n_ll + n_sil + 1;
    std::vector<int>    ids((size_t)cap), index((size_t)n_mix);
    std::vector<double> mats((size_t)(per * cap)), count((size_t)n_ids);
    int                 n = 0, flags = -1;
    CHECK(amx_mllr_estimate(&shape, acc.data(), &tree, n_mix, lom.data(), thr[0], thr[1], 0.0, &n, ids.data(), mats.data(), index.data(), count.data(),
                            &flags) == AMX_OK);
    CHECK(n == n_ref && flags == 0);
    CHECK(memcmp(ids.data(), ref_ids.data(), (size_t)n * 4) == 0 && memcmp(index.data(), ref_index.data(), (size_t)n_mix * 4) == 0);
    for (int m = 0; m < n; ++m) {   // per matrix, against its largest element
        double worst = 0, scale = 0;
        for (long e = (long)m * per; e < (long)(m + 1) * per; ++e) {
            worst = std::max(worst, std::fabs(mats[(size_t)e] - ref_mats[(size_t)e]));
            scale = std::max(scale, std::fabs(ref_mats[(size_t)e]));
        }
        CHECK(worst <= bar_abs && worst <= bar_rel * scale);
    }
    // the default thresholds: the root-only fallback and the silence fallback
    CHECK(amx_mllr_estimate(&shape, acc.data(), &tree, n_mix, lom.data(), 1000.0, 500.0, 0.0, &n, ids.data(), mats.data(), index.data(), nullptr, &flags) ==
          AMX_OK);
    CHECK(flags == (AMX_MLLR_ROOT_FALLBACK | AMX_MLLR_SILENCE_FALLBACK) && n == 1 + n_sil && ids[0] == root);
    for (int d = 0; mode == AMX_MLLR_FULL && d < D; ++d)
        CHECK(mats[(size_t)d * (D + 1) + d + 1] == 1.0 && mats[(size_t)d * (D + 1)] == 0.0);

    // ---- the adaptor file: the reference's bytes from the reference's matrices, and back
    const std::string q = dir + "/mine.adaptor";
    CHECK(amx_mllr_adaptor_write(&shape, "key0", n_ref, ref_ids.data(), ref_mats.data(), n_mix, ref_index.data(), q.c_str()) == AMX_OK);
    const std::vector<unsigned char> ref_ad = slurp(dir + "/key0.adaptor"), mine_ad = slurp(q);
    CHECK(!ref_ad.empty() && mine_ad == ref_ad);
    int n_back = 0;
    CHECK(amx_mllr_adaptor_read(&shape, q.c_str(), cap, &n_back, ids.data(), mats.data(), n_mix, index.data()) == AMX_OK);
    CHECK(n_back == n_ref && memcmp(ids.data(), ref_ids.data(), (size_t)n_ref * 4) == 0 && memcmp(mats.data(), ref_mats.data(), ref_mats.size() * 8) == 0 &&
          memcmp(index.data(), ref_index.data(), (size_t)n_mix * 4) == 0);
    CHECK(amx_mllr_adaptor_read(&shape, q.c_str(), n_ref - 1, &n_back, ids.data(), mats.data(), n_mix, index.data()) == AMX_ERR_INVALID);
    for (size_t cut : {(size_t)0, (size_t)7, (size_t)30, mine_ad.size() / 2, mine_ad.size() - 1}) {
        CHECK(spill(q, mine_ad.data(), cut));
        CHECK(amx_mllr_adaptor_read(&shape, q.c_str(), cap, &n_back, ids.data(), mats.data(), n_mix, index.data()) == AMX_ERR_INVALID);
    }

    // ---- refusals: trees that are no trees, a leaf out of range, the unsupported modes
    {
        std::vector<int> l2 = left;
        l2[(size_t)root]    = root;   // a cycle
        amx_mllr_tree t     = tree;
        t.left              = l2.data();
        CHECK(amx_mllr_estimate(&shape, acc.data(), &t, n_mix, lom.data(), thr[0], thr[1], 0.0, &n, ids.data(), mats.data(), index.data(), nullptr, nullptr) ==
              AMX_ERR_INVALID);
        l2               = left;
        l2[(size_t)root] = n_ids;   // outside
        CHECK(amx_mllr_estimate(&shape, acc.data(), &t, n_mix, lom.data(), thr[0], thr[1], 0.0, &n, ids.data(), mats.data(), index.data(), nullptr, nullptr) ==
              AMX_ERR_INVALID);
        std::vector<int> ln = leafno;
        ln[(size_t)llist[0]] = L;   // a leaf number outside [0, n_leafs)
        t                    = tree;
        t.leaf_number        = ln.data();
        CHECK(amx_mllr_estimate(&shape, acc.data(), &t, n_mix, lom.data(), thr[0], thr[1], 0.0, &n, ids.data(), mats.data(), index.data(), nullptr, nullptr) ==
              AMX_ERR_INVALID);
        std::vector<int> pv = prev;
        pv[(size_t)llist[0]] = llist[0];   // `previous` does not lead to the root
        t                    = tree;
        t.previous           = pv.data();
        CHECK(amx_mllr_estimate(&shape, acc.data(), &t, n_mix, lom.data(), thr[0], thr[1], 0.0, &n, ids.data(), mats.data(), index.data(), nullptr, nullptr) ==
              AMX_ERR_INVALID);
        std::vector<int> lm = lom;
        lm[0]               = L;
        CHECK(amx_mllr_estimate(&shape, acc.data(), &tree, n_mix, lm.data(), thr[0], thr[1], 0.0, &n, ids.data(), mats.data(), index.data(), nullptr, nullptr) ==
              AMX_ERR_INVALID);
        amx_mllr_shape band = shape;
        band.mode           = AMX_MLLR_BAND;
        CHECK(amx_mllr_estimate(&band, acc.data(), &tree, n_mix, lom.data(), thr[0], thr[1], 0.0, &n, ids.data(), mats.data(), index.data(), nullptr, nullptr) ==
                      AMX_ERR_UNSUPPORTED &&
              g_error.find("band") != std::string::npos);
        band.mode = AMX_MLLR_SEMI_TIED;
        CHECK(amx_mllr_key_size(&band) == 0);
        band      = shape;
        band.dim  = 256;
        CHECK(amx_mllr_key_size(&band) == 0);
    }
    printf("host_mllr_test: ok\n");
    return 0;
}
