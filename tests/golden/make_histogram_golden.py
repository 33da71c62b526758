#!/usr/bin/env python3
"""tests/golden/make_histogram_golden.py -- writes tests/golden/ref_histogram.npz: histogram estimation and histogram normalisation as
the reference's own text computes them.

Run it where the reference tree is mounted and `oracle/_ref/` has been built (`__graft_entry__.build()`); tests read only the
fixture.  What it compiles, in both of the reference's arithmetics (the flag sets of oracle/ref/Makefile: -msse3 = contract=off,
-msse3 -march=native = contract=fma), taken by line range + SHA-256 into a temporary directory that is deleted afterwards:
  * Signal/LookupTable.hh:28-33, 50-319, 330-340 (the class, insert, normalizeSurface, isMonotonous, getInverse,
    proposeBucketSizeForInverse, += and *=, read, write and the binary stream operators; the XML operator<< is left out, a forward
    declaration of Core::XmlWriter suffices)
  * Signal/Histogram.hh:33-80, 85-135 (Histogram, HistogramVector; without dump)
  * Signal/HistogramNormalization.cc:24-93 (both setTrainingHistograms, setTestHistograms, apply, the three scale functions) behind a
    shell that declares the members of HistogramNormalization.hh:26-68
Core/BinaryStream.cc comes compiled and unmodified from oracle/_ref/libref.so / libref_native.so.  The text is compiled with
-fno-access-control so that the entry points of this file's own (hg_* / hn_*, no reference text) can read offset_ and call bucket().

Histogram::percentile (Histogram.hh:56-64) cannot be instantiated: it names `Precursor::ConstantIterator`, which LookupTable does not
have (its type is ConstIterator), and calls the base's index() unqualified.  hg_percentile below is that function with exactly these
two names put right and nothing else changed; the fixture's percentiles come from it.

Recorded: per histogram (ties at dim 2 and 5 with bucket size 0.25; Gaussian at dim 3 with bucket sizes 0.01, 0.02, 0.05; a second,
shifted speaker) the frames, the tables, the file's bytes, the tables read back from the file, the CDFs and percentiles; per
normaliser (one training histogram with explicit and proposed probability bucket size, two and three of different bucket sizes with
scales) the inverse CDFs, the test CDFs, and apply() on each test key's own frames with a mask of the elements whose two buckets lie
inside their tables (outside, the release build reads beyond a deque: those are not evaluated).  The contract=fma copies are kept only
where their bits differ from contract=off (expected: nowhere).

    python3 tests/golden/make_histogram_golden.py [out.npz]
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"

PIECES = {
    "lookup": [("Signal/LookupTable.hh", 28, 33), ("Signal/LookupTable.hh", 50, 319), ("Signal/LookupTable.hh", 330, 340)],
    "histogram": [("Signal/Histogram.hh", 33, 80), ("Signal/Histogram.hh", 85, 135)],
    "normalization": [("Signal/HistogramNormalization.cc", 24, 93)],
}
SHA = "f35b82124c852b9229044c865735621460b11f5506494d273fe6f74c48a25016"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/BinaryStream.hh>
#include <Core/Types.hh>
#include <Core/Utility.hh>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <functional>
#include <numeric>
#include <string>
#include <vector>
namespace Core { class XmlWriter; }
namespace Signal {
// ---- reference text: LookupTable ----
%(lookup)s
// ---- reference text: Histogram, HistogramVector ----
%(histogram)s
// ---- shell: the members of HistogramNormalization.hh:26-68
class HistogramNormalization {
public:
    typedef f32                           Value;
    typedef Histogram<Value>::Probability Probability;
    typedef Histogram<Value>::Weight      HistogramWeight;
    typedef LookupTable<Probability, Value> Cdf;
    typedef std::vector<Cdf>                Cdfs;
    typedef LookupTable<Value, Probability> InverseCdf;
    typedef std::vector<InverseCdf>         InverseCdfs;
    Cdfs        testCdfs_;
    InverseCdfs inverseTrainingCdfs_;
    HistogramNormalization() {}
    void apply(const std::vector<Value>& in, std::vector<Value>& out);
    void setTrainingHistograms(const std::vector<Histogram<Value>>& trainingHistograms, Probability probabilityBucketSize);
    void setTrainingHistograms(const std::vector<HistogramVector<Value>>& trainingHistograms, const std::vector<Value>& scales,
                               Probability probabilityBucketSize);
    void setTestHistograms(const std::vector<Histogram<Value>>& testHistograms);
    static bool areScalesWellDefined(const std::vector<HistogramWeight>& scales);
    static bool areScalesNormalized(const std::vector<HistogramWeight>& scales);
    static void normalizeScales(std::vector<HistogramWeight>& scales);
};
}  // namespace Signal
using namespace Signal;
// ---- reference text: HistogramNormalization ----
%(normalization)s
// ---- this generator's own entry points (no reference text) ----
static std::vector<HistogramVector<f32>*>   g_hist;
static std::vector<HistogramNormalization*> g_norm;
typedef LookupTable<f32, f32> Table;
static int dump(const Table& t, float* bs, int* off, int* grow, int cap, float* values) {
    *bs   = t.bucketSize_;
    *off  = t.offset_;
    *grow = t.grow_ ? 1 : 0;
    if ((int)t.f_.size() <= cap)
        std::copy(t.f_.begin(), t.f_.end(), values);
    return (int)t.f_.size();
}
extern "C" int hg_new(int dim, float bucket_size) {
    g_hist.push_back(new HistogramVector<f32>(dim, bucket_size));
    return (int)g_hist.size() - 1;
}
extern "C" void hg_accumulate(int id, int T, const float* feats) {
    const size_t   dim = g_hist[id]->size();
    std::vector<f32> v(dim);
    for (int t = 0; t < T; ++t) {
        std::copy(feats + (size_t)t * dim, feats + (size_t)(t + 1) * dim, v.begin());
        g_hist[id]->accumulate(v);   // Speech::HistogramEstimator::processFeature: weight 1
    }
}
extern "C" int hg_dim(int id) { return (int)g_hist[id]->size(); }
extern "C" int hg_table(int id, int d, float* bs, int* off, int* grow, int cap, float* values) {
    return dump((*g_hist[id])[d], bs, off, grow, cap, values);
}
extern "C" int hg_cdf(int id, int d, float* bs, int* off, int* grow, int cap, float* values) {
    Table cdf;
    (*g_hist[id])[d].getCdf(cdf);
    return dump(cdf, bs, off, grow, cap, values);
}
// Histogram.hh:56-64 with `ConstantIterator` -> `ConstIterator` and `index` -> `this->index` (see the docstring)
extern "C" float hg_percentile(int id, int d, float percent) {
    const Histogram<f32>& h = (*g_hist[id])[d];
    f32                   p = percent * h.sum();
    Table::ConstIterator  b;
    for (b = h.begin(); b != h.end() && p > 0; ++b)
        p -= *b;
    return h.index(b - h.begin());
}
extern "C" int hg_write(int id, const char* path) {
    Core::BinaryOutputStream bos(path);
    if (!bos)
        return -1;
    g_hist[id]->write(bos);
    return bos.good() ? 0 : -2;
}
extern "C" int hg_read(const char* path) {
    Core::BinaryInputStream bis(path);
    if (!bis)
        return -1;
    HistogramVector<f32>* h = new HistogramVector<f32>();
    h->read(bis);
    if (!bis.good())
        return -2;
    g_hist.push_back(h);
    return (int)g_hist.size() - 1;
}
extern "C" int hn_new() {
    g_norm.push_back(new HistogramNormalization());
    return (int)g_norm.size() - 1;
}
// HistogramNormalizationNode::init with one training histogram / updateTrainingHistograms with several (scales: n - 1 of them);
// all_scales [n] returns what normalizeScales made of them; -1 if areScalesWellDefined says no
extern "C" int hn_set_training(int nid, int n, const int* ids, const float* scales, float probability_bucket_size, float* all_scales) {
    if (n == 1) {
        g_norm[nid]->setTrainingHistograms(*g_hist[ids[0]], probability_bucket_size);
        return 0;
    }
    std::vector<f32> s(scales, scales + n - 1);
    HistogramNormalization::normalizeScales(s);
    std::copy(s.begin(), s.end(), all_scales);
    if (!HistogramNormalization::areScalesWellDefined(s))
        return -1;
    std::vector<HistogramVector<f32>> train;
    for (int i = 0; i < n; ++i)
        train.push_back(*g_hist[ids[i]]);
    g_norm[nid]->setTrainingHistograms(train, s, probability_bucket_size);
    return 0;
}
extern "C" void hn_set_test(int nid, int id) { g_norm[nid]->setTestHistograms(*g_hist[id]); }
extern "C" int hn_inverse(int nid, int d, float* bs, int* off, int* grow, int cap, float* values) {
    return dump(g_norm[nid]->inverseTrainingCdfs_[d], bs, off, grow, cap, values);
}
extern "C" int hn_test_cdf(int nid, int d, float* bs, int* off, int* grow, int cap, float* values) {
    return dump(g_norm[nid]->testCdfs_[d], bs, off, grow, cap, values);
}
// apply() frame by frame; a frame is evaluated only if every component's two buckets lie inside their tables (inside[t] = 1)
extern "C" void hn_apply(int nid, int T, const float* in, float* out, int* inside) {
    HistogramNormalization& n = *g_norm[nid];
    const size_t            dim = n.testCdfs_.size();
    std::vector<f32>        x(dim), y;
    for (int t = 0; t < T; ++t) {
        bool ok = true;
        for (size_t i = 0; i < dim && ok; ++i) {
            const f32 v = in[(size_t)t * dim + i];
            s32       b = n.testCdfs_[i].bucket(v);
            ok          = 0 <= b && b < (s32)n.testCdfs_[i].size();
            if (ok) {
                b  = n.inverseTrainingCdfs_[i].bucket(n.testCdfs_[i].f_[b]);
                ok = 0 <= b && b < (s32)n.inverseTrainingCdfs_[i].size();
            }
        }
        inside[t] = ok ? 1 : 0;
        if (!ok)
            continue;
        std::copy(in + (size_t)t * dim, in + (size_t)(t + 1) * dim, x.begin());
        n.apply(x, y);
        std::copy(y.begin(), y.end(), out + (size_t)t * dim);
    }
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-fno-access-control", "-D_GNU_SOURCE",
         "-DSPRINT_RELEASE_BUILD", "-I" + REF, "-I/usr/include/libxml2", "-w"]
PERCENTS = np.array([0.0, 0.1, 0.5, 0.9, 1.0], np.float32)


def reference_text():
    cache, parts, h = {}, {}, hashlib.sha256()
    for key, ranges in PIECES.items():
        out = []
        for fn, first, last in ranges:
            if fn not in cache:
                with open(os.path.join(REF, fn), encoding="utf-8", errors="replace") as f:
                    cache[fn] = f.readlines()
            out.append("".join(cache[fn][first - 1:last]))
        parts[key] = "\n".join(out)
        h.update(parts[key].encode())
    return parts, h.hexdigest()


def build(tmp, flavour, parts):
    gen = os.path.join(tmp, "histogram_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "histogram_%s.so" % flavour)
    lib = "ref" if flavour == "off" else "ref_native"
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen, "-L" + os.path.join(ROOT, "oracle", "_ref"), "-l" + lib,
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_ref")])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
    table = [C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p]
    for name, res, args in (("hg_new", C.c_int, [C.c_int, C.c_float]), ("hg_accumulate", None, [C.c_int, C.c_int, f32p]), ("hg_dim", C.c_int, [C.c_int]),
                            ("hg_table", C.c_int, [C.c_int, C.c_int] + table), ("hg_cdf", C.c_int, [C.c_int, C.c_int] + table),
                            ("hg_percentile", C.c_float, [C.c_int, C.c_int, C.c_float]), ("hg_write", C.c_int, [C.c_int, C.c_char_p]),
                            ("hg_read", C.c_int, [C.c_char_p]), ("hn_new", C.c_int, []),
                            ("hn_set_training", C.c_int, [C.c_int, C.c_int, i32p, C.c_void_p, C.c_float, f32p]), ("hn_set_test", None, [C.c_int, C.c_int]),
                            ("hn_inverse", C.c_int, [C.c_int, C.c_int] + table), ("hn_test_cdf", C.c_int, [C.c_int, C.c_int] + table),
                            ("hn_apply", None, [C.c_int, C.c_int, f32p, f32p, i32p])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L, int(fma or 0)


def get_table(fn, *head):
    """{bucket_size, offset, grow, values} through one of the dump entry points"""
    bs, off, grow = C.c_float(), C.c_int(), C.c_int()
    n = fn(*head, C.byref(bs), C.byref(off), C.byref(grow), 0, None)
    v = np.zeros(n, np.float32)
    assert fn(*head, C.byref(bs), C.byref(off), C.byref(grow), n, v.ctypes.data) == n
    return {"bucket_size": np.float32(bs.value), "offset": np.int32(off.value), "grow": np.int32(grow.value), "values": v}


def histograms():
    """name -> (bucket size, frames f32 [T, dim])"""
    out = {}
    for dim in (2, 5):
        rng = np.random.Generator(np.random.PCG64(40 + dim))
        T = 48
        k = rng.integers(-9, 10, (T, dim))
        sign = rng.choice([-1.0, 1.0], (T, dim))
        x = (k * 0.25 + sign * 0.125).astype(np.float32)          # exact ties k * 0.25 +- 0.125, both signs
        x[::7] = (rng.integers(-9, 10, x[::7].shape) * 0.25).astype(np.float32)   # bucket centres
        x[3, 0], x[5, dim - 1], x[8, 0] = -0.0, -0.0, 0.0
        x[11] = 0.125
        x[12] = -0.125
        out["ties%d" % dim] = (np.float32(0.25), x)
    rng = np.random.Generator(np.random.PCG64(7))
    out["gauss_a"] = (np.float32(0.01), (rng.standard_normal((200, 3)) * [0.3, 0.5, 0.2] + [0.0, 1.0, -0.5]).astype(np.float32))
    out["gauss_b"] = (np.float32(0.02), (rng.standard_normal((160, 3)) * [0.4, 0.3, 0.3] + [0.2, 0.8, -0.4]).astype(np.float32))
    out["gauss_c"] = (np.float32(0.05), (rng.standard_normal((120, 3)) * [0.2, 0.6, 0.25] + [-0.1, 1.2, -0.6]).astype(np.float32))
    out["speaker"] = (np.float32(0.01), (rng.standard_normal((150, 3)) * [0.45, 0.35, 0.3] + [0.6, 0.4, -0.1]).astype(np.float32))
    return out


# name -> (training histograms, scales of all but the first, probability bucket size, test keys)
NORMALIZERS = {
    "single_explicit": (["gauss_a"], [], 0.01, ["gauss_a", "speaker"]),
    "single_proposed": (["gauss_a"], [], 0.0, ["speaker"]),
    "ties": (["ties5"], [], 0.0, ["ties5"]),
    "two": (["gauss_a", "gauss_b"], [0.3], 0.0, ["speaker"]),
    "three": (["gauss_a", "gauss_b", "gauss_c"], [0.25, 0.5], 0.005, ["speaker", "gauss_a"]),
}


def run(L, tmp, fl):
    """every recorded array of one build"""
    a, ids = {}, {}
    for name, (bs, x) in histograms().items():
        T, dim = x.shape
        hid = L.hg_new(dim, float(bs))
        half = T // 3
        L.hg_accumulate(hid, half, np.ascontiguousarray(x[:half]))
        L.hg_accumulate(hid, T - half, np.ascontiguousarray(x[half:]))
        ids[name] = hid
        path = os.path.join(tmp, "%s_%s.hist" % (name, fl))
        assert L.hg_write(hid, path.encode()) == 0
        with open(path, "rb") as f:
            a["h/%s/file" % name] = np.frombuffer(f.read(), np.uint8).copy()
        rid = L.hg_read(path.encode())
        assert rid >= 0 and L.hg_dim(rid) == dim
        for d in range(dim):
            for what, t in (("table", get_table(L.hg_table, hid, d)), ("read", get_table(L.hg_table, rid, d)), ("cdf", get_table(L.hg_cdf, hid, d))):
                for k, v in t.items():
                    a["h/%s/%s/%d/%s" % (name, what, d, k)] = v
            a["h/%s/percentiles/%d" % (name, d)] = np.array([L.hg_percentile(hid, d, float(p)) for p in PERCENTS], np.float32)
    for name, (train, scales, pbs, tests) in NORMALIZERS.items():
        nid = L.hn_new()
        tid = np.array([ids[t] for t in train], np.int32)
        sc = np.array(scales, np.float32)
        all_scales = np.zeros(len(train), np.float32)
        assert L.hn_set_training(nid, len(train), tid, sc.ctypes.data if len(sc) else None, float(np.float32(pbs)), all_scales) == 0
        if len(train) > 1:
            a["n/%s/all_scales" % name] = all_scales
        dim = histograms()[train[0]][1].shape[1]
        for d in range(dim):
            for k, v in get_table(L.hn_inverse, nid, d).items():
                a["n/%s/inverse/%d/%s" % (name, d, k)] = v
        for key in tests:
            L.hn_set_test(nid, ids[key])
            for d in range(dim):
                for k, v in get_table(L.hn_test_cdf, nid, d).items():
                    a["n/%s/test/%s/cdf/%d/%s" % (name, key, d, k)] = v
            x = np.ascontiguousarray(histograms()[key][1])
            out, inside = np.zeros_like(x), np.zeros(len(x), np.int32)
            L.hn_apply(nid, len(x), x, out, inside)
            a["n/%s/test/%s/out" % (name, key)] = out
            a["n/%s/test/%s/inside" % (name, key)] = inside
    # a scale outside [0, 1]: areScalesWellDefined refuses (the first scale becomes 1 - 1.25 < 0; a negative one)
    nid = L.hn_new()
    tid = np.array([ids["gauss_a"], ids["gauss_b"]], np.int32)
    for k, s in (("too_large", 1.25), ("negative", -0.25)):
        sc = np.array([s], np.float32)
        a["scales_refused/" + k] = np.array(L.hn_set_training(nid, 2, tid, sc.ctypes.data, 0.0, np.zeros(2, np.float32)) == -1, np.int32)
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_histogram.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_histogram_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    arrays = {"percents": PERCENTS}
    for name, (bs, x) in histograms().items():
        arrays["h/%s/feats" % name], arrays["h/%s/bucket_size" % name] = x, bs
    for name, (train, scales, pbs, tests) in NORMALIZERS.items():
        arrays["n/%s/train" % name] = np.array(train)
        arrays["n/%s/scales" % name] = np.array(scales, np.float32)
        arrays["n/%s/probability_bucket_size" % name] = np.float32(pbs)
        arrays["n/%s/tests" % name] = np.array(tests)
    with tempfile.TemporaryDirectory() as tmp:
        got = {}
        for fl in ("off", "fma"):
            L, n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)   # fused multiply-adds in the generated object (objdump)
            got[fl] = run(L, tmp, fl)
    for k, v in got["off"].items():
        arrays["off/" + k] = v
    for k, v in got["fma"].items():
        if not same_bits(v, got["off"][k]):
            arrays["fma/" + k] = v
    arrays["fma_arrays_compared"] = np.array(len(got["fma"]))
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    print("  fma instructions: off %d, fma %d" % (int(arrays["fma_instructions/off"]), int(arrays["fma_instructions/fma"])))
    print("  fma copies that differ from off: %d of %d" % (sum(1 for k in arrays if k.startswith("fma/")), len(got["fma"])))
    inside = {k: "%d/%d" % (v.sum(), len(v)) for k, v in arrays.items() if k.endswith("/inside")}
    print("  frames evaluated by apply:", inside)


if __name__ == "__main__":
    main()
