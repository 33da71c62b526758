#!/usr/bin/env python3
"""tests/golden/make_quanteq_golden.py -- writes tests/golden/ref_quanteq.npz: what the `signal-quantile-equalization` node computes in
segment mode, as the reference's own text computes it.

Run it where the reference tree is mounted; tests read only the fixture.  What it compiles, in both of the reference's arithmetics (the
flag sets of oracle/ref/Makefile: -msse3 = contract=off, -msse3 -march=native = contract=fma), taken by line range + SHA-256 into a
temporary directory that is deleted afterwards:
  * Signal/SlidingWindow.hh:20-471 (everything between the two Flow includes and the include guard's end)
  * Signal/QuantileEqualization.hh:27-268 (the class)
  * Signal/QuantileEqualization.cc:28-339 (init, both file functions, update, updateTransformationParameters, applyTransformations)
behind a shell of this file's own that holds no reference text: Flow::Data / Vector / DataPtr stand-ins (DataPtr counts references;
makePrivate copies a shared vector, operator bool, a converting constructor) and the two AssertionsPrivate functions the text calls.

The driver replays QuantileEqualizationNode::work (QuantileEqualization.hh:364-378) per segment: update() per frame, flush() until it
fails, reset().  `firstcall` (QuantileEqualization.cc:29) is a function-local static, so only the first object of a process reads its
training file: every configuration gets ONE object in a copy of the shared object of its own (a fresh static), reset() per segment as the
node does.  Training quantiles go through a real file, which the object reads itself.

Recorded per configuration: its parameters, the training file's bytes, the training quantiles as the object read them (pooled or not),
and per segment the input, alpha, gamma, lambda, rho, mean, deviation, the current quantiles after the search (interior ones transformed)
and the output; for the estimating configurations the file the object wrote.  The segments of a configuration lie one after the other
along the first axis.  The fma/ copies are kept only where bits differ.  One one-frame segment (all quantiles coincide, the grid is full
of near-ties) is searched for on which the two builds choose different (alpha, gamma), and kept (configuration d20, last segment).

cpu_seconds_per_segment/<dim>/<combination>: wall time of one 1000-frame segment in the contract=off build on the CPU named in cpu_name.

    python3 tests/golden/make_quanteq_golden.py [out.npz]
"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"

PIECES = {
    "sliding_window": [("Signal/SlidingWindow.hh", 20, 471)],
    "quanteq_hh": [("Signal/QuantileEqualization.hh", 27, 268)],
    "quanteq_cc": [("Signal/QuantileEqualization.cc", 28, 339)],
}
SHA = "235fa3c1d04afc7f72ce91718fc32c1bee263f5915c0b29edba9ada1ef94c29b"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/Types.hh>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>
// ---- shell: stand-ins (no reference text) ----
namespace AssertionsPrivate {
void assertionFailed(const char* type, const char* expr, const char* function, const char* filename, unsigned int line) {
    fprintf(stderr, "%%s failed: %%s in %%s (%%s:%%u)\n", type, expr, function, filename, line);
    abort();
}
void hopeDisappointed(const char* expr, const char* function, const char* filename, unsigned int line) {
    fprintf(stderr, "hope disappointed: %%s in %%s (%%s:%%u)\n", expr, function, filename, line);
    abort();
}
}  // namespace AssertionsPrivate
namespace Flow {
class Data {
public:
    virtual ~Data() {}
};
template<class T> class Vector : public Data, public std::vector<T> {
public:
    Vector() {}
    Vector(size_t n) : std::vector<T>(n) {}
};
template<class T> class DataPtr {
public:
    std::shared_ptr<T> p_;
    DataPtr() {}
    DataPtr(T* p) : p_(p) {}
    template<class U> DataPtr(const DataPtr<U>& o) : p_(std::dynamic_pointer_cast<T>(o.p_)) {}
    T*   get() const { return p_.get(); }
    T*   operator->() const { return p_.get(); }
    T&   operator*() const { return *p_; }
    operator bool() const { return (bool)p_; }
    void makePrivate() {
        if (p_ && p_.use_count() > 1)
            p_ = std::shared_ptr<T>(new T(*p_));
    }
};
}  // namespace Flow
// ---- reference text: SlidingWindow (opens and closes namespace Signal itself) ----
%(sliding_window)s
namespace Signal {
// ---- reference text: QuantileEqualization ----
%(quanteq_hh)s
}  // namespace Signal
using namespace Signal;
using namespace Core;
using namespace Flow;
// ---- reference text: QuantileEqualization.cc ----
%(quanteq_cc)s
// ---- this generator's own driver (no reference text) ----
typedef Flow::DataPtr<Flow::Vector<f32>> QeFrame;
// QuantileEqualizationNode's constructor (QuantileEqualization.hh:293-312)
extern "C" void* qe_new(int quantiles, int combination, int estimate, int mean, int variance, int nq, float of, float delta_alpha,
                        float delta_gamma, float delta_lr, float beta, int pool, const char* filename) {
    QuantileEqualization* q = new QuantileEqualization;
    q->piecewiseLinear_ = false;   // the members the constructor leaves unset get the node's defaults through the setters below
    q->estimateQuantiles_ = false;
    q->poolQuantiles_ = true;
    q->setQuantileEqualization(quantiles);
    q->setCombineNeighbors(combination);
    q->setQuantileEstimation(estimate);
    q->setQuantileFile(filename);
    q->setPoolQuantiles(pool);
    q->setPiecewiseLinear(false);
    q->setNormalizeMean(mean);
    q->setNormalizeVariance(variance);
    q->setLength(Core::Type<s32>::max);
    q->setRight(Core::Type<s32>::max);
    q->setNumberOfQuantiles(nq);
    q->setOverestimationFactor(of);
    q->setDeltaAlpha(delta_alpha);
    q->setDeltaGamma(delta_gamma);
    q->setDeltaLambdaAndRho(delta_lr);
    q->setBeta(beta);
    q->reset();
    return q;
}
// QuantileEqualizationNode::work (:364-378) for one segment; params: alpha, gamma, lambda, rho, mean, deviation [6 x dim] after the
// first frame left
extern "C" int qe_segment(void* h, int dim, int T, const float* x, float* out, float* params, float* cq_after, float* tq_as_read) {
    QuantileEqualization* q = (QuantileEqualization*)h;
    int n_out = 0;
    QeFrame o;
    for (int t = 0; t < T; ++t) {
        Flow::Vector<f32>* v = new Flow::Vector<f32>(dim);
        std::copy(x + (size_t)t * dim, x + (size_t)(t + 1) * dim, v->begin());
        QeFrame in(v);
        if (q->update(in, o))
            return -1;   // segment mode emits nothing before the end of the stream
    }
    while (q->flush(o)) {
        if (n_out == 0) {
            for (int d = 0; d < dim; ++d) {
                params[0 * dim + d] = q->alpha_[d];
                params[1 * dim + d] = q->gamma_[d];
                params[2 * dim + d] = q->lambda_[d];
                params[3 * dim + d] = q->rho_[d];
                params[4 * dim + d] = q->mean_[d];
                params[5 * dim + d] = q->dev_[d];
            }
            std::copy(q->currentQuantile_.begin(), q->currentQuantile_.end(), cq_after);
            std::copy(q->trainingQuantile_.begin(), q->trainingQuantile_.end(), tq_as_read);
        }
        if (n_out >= T)
            return -2;
        std::copy(o->begin(), o->end(), out + (size_t)n_out * dim);
        ++n_out;
    }
    q->reset();
    return n_out;
}
extern "C" void qe_sums(void* h, double* sums, unsigned* count) {
    QuantileEqualization* q = (QuantileEqualization*)h;
    std::copy(q->quantileSum_.begin(), q->quantileSum_.end(), sums);
    *count = q->frameCounter_;
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-fno-access-control", "-D_GNU_SOURCE",
         "-DSPRINT_RELEASE_BUILD", "-I" + REF, "-I/usr/include/libxml2", "-w"]

DEFAULTS = dict(quantiles=1, combination=0, estimate=0, mean=1, variance=0, nq=4, of=1.0, delta_alpha=0.005, delta_gamma=0.01, delta_lr=0.005,
                beta=0.05, pool=1)
BASE_T = (1, 2, 3, 5, 63, 64, 65, 300)
# name -> (dim, parameters that differ from DEFAULTS, segments); a segment is (T, kind) with the kinds of segment_input()
CONFIGS = {
    "d20": (20, {}, [(t, "plain") for t in BASE_T] + [(50, "constant"), (200, "quantised"), (300, "below"), (300, "above"), (40, "signed"),
                    (40, "cancelling")]),
    "d20_cv": (20, dict(combination=1, variance=1), [(1, "plain"), (2, "plain"), (5, "plain"), (64, "plain"), (300, "plain"), (50, "constant")]),
    "d20_c": (20, dict(combination=1), [(3, "plain"), (65, "plain")]),
    "d20_v": (20, dict(variance=1), [(2, "plain"), (63, "plain"), (300, "plain")]),
    "d20_nomean_v": (20, dict(mean=0, variance=1), [(5, "plain"), (64, "plain")]),
    "d20_nomean_c": (20, dict(mean=0, combination=1), [(3, "plain"), (300, "plain")]),
    "d20_nomean": (20, dict(mean=0), [(65, "plain")]),
    "d20_nomean_cv": (20, dict(mean=0, combination=1, variance=1), [(63, "plain")]),
    "d20_of": (20, dict(of=1.2, combination=1, variance=1), [(1, "plain"), (64, "above"), (300, "plain")]),
    "d1": (1, dict(combination=1, variance=1), [(1, "plain"), (3, "plain"), (64, "plain"), (300, "plain")]),
    "d2_nq1": (2, dict(nq=1), [(1, "plain"), (2, "plain"), (65, "plain")]),
    "d2_nq2": (2, dict(nq=2, combination=1), [(1, "plain"), (5, "plain"), (300, "plain")]),
    # the sort's size boundaries: its network has a power-of-two size (1024 | 1025), its LDS ends at 16384 frames (16385 is refused)
    "d1_long": (1, dict(variance=1), [(1024, "plain"), (1025, "plain"), (16383, "plain"), (16384, "plain")]),
    "d40_nq10": (40, dict(nq=10, combination=1, variance=1, of=1.2), [(3, "plain"), (63, "plain"), (300, "plain")]),
    "d65": (65, dict(variance=1), [(2, "plain"), (64, "plain"), (65, "plain")]),
    "d20_unpooled": (20, dict(pool=0, combination=1, variance=1), [(5, "plain"), (300, "plain"), (30, "zero_channel")]),
    "d20_noq": (20, dict(quantiles=0, variance=1), [(1, "plain"), (5, "plain"), (300, "plain")]),
    "est_d20": (20, dict(estimate=1), [(300, "plain"), (1, "plain"), (64, "quantised"), (5, "plain")]),
    "est_d2_nq10": (2, dict(estimate=1, nq=10), [(65, "plain"), (2, "plain"), (3, "plain")]),
}
ZERO_CHANNEL = 3   # d20_unpooled: training quantiles of this channel are 0, and the zero_channel segment holds 0 there


def cfg_of(name):
    c = dict(DEFAULTS)
    c.update(CONFIGS[name][1])
    return c


def coarse(x):
    """f32 values on a grid of 2^-8 (they compress; the arithmetic does not care)"""
    return (np.round(np.asarray(x, np.float64) * 256.0) / 256.0).astype(np.float32)


def segment_input(name, index, dim, T, kind, seed=0):
    """filter-bank-like positive values, channel d around 4 + d / 4"""
    rng = np.random.Generator(np.random.PCG64([sum(name.encode()), index, seed]))
    level = 4.0 + np.arange(dim) / 4.0
    x = level * np.exp(rng.normal(0.0, 0.5, (T, dim)))
    if kind == "constant":
        x = np.tile(level, (T, 1))
    elif kind == "quantised":
        x = np.round(x / 2.0) * 2.0
    elif kind == "below":       # maximum below the training maximum
        x = x * 0.25
    elif kind == "above":       # and above
        x = x * 4.0
    elif kind == "signed":      # negative values: pow gives NaN for every gamma but 1
        x = x - level
    x = coarse(x)
    if kind == "cancelling":    # + 2^60 and - 2^60 as the last two frames: the f64 sum depends on the order of the frames
        x = coarse(level * np.exp(rng.normal(0.0, 0.5, (T, dim))) - level)
        x[T - 2], x[T - 1] = np.float32(2.0 ** 60), np.float32(-2.0 ** 60)
    if kind == "zero_channel":
        x[:, ZERO_CHANNEL] = 0.0
    return x


def training_file(name, dim, nq):
    """the text of a training quantile file: increasing quantiles per channel, different per channel"""
    rng = np.random.Generator(np.random.PCG64([sum(name.encode()), 77]))
    level = 4.5 + np.arange(dim) / 5.0
    q = np.sort(level * np.exp(rng.normal(0.0, 0.6, (nq + 1, dim))), axis=0) * np.linspace(0.5, 2.5, nq + 1)[:, None]
    if name == "d20_unpooled":
        q[:, ZERO_CHANNEL] = 0.0
    return "".join("%d " % d + "".join("%f " % q[i, d] for i in range(nq + 1)) + "\n" for d in range(dim))


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
    gen = os.path.join(tmp, "quanteq_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "quanteq_%s.so" % flavour)
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    return so, int(fma or 0)


_copies = [0]


def load(tmp, so):
    """a copy of the shared object of its own: a fresh `firstcall`"""
    _copies[0] += 1
    mine = os.path.join(tmp, "copy%d_%s" % (_copies[0], os.path.basename(so)))
    shutil.copy(so, mine)
    L = C.CDLL(mine)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    L.qe_new.restype = C.c_void_p
    L.qe_new.argtypes = [C.c_int] * 6 + [C.c_float] * 5 + [C.c_int, C.c_char_p]
    L.qe_segment.restype = C.c_int
    L.qe_segment.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, f32p, f32p, f32p, f32p]
    L.qe_sums.restype = None
    L.qe_sums.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float64, flags="C"), C.POINTER(C.c_uint)]
    return L


def new_object(tmp, so, name, dim):
    c = cfg_of(name)
    L = load(tmp, so)
    path = os.path.join(tmp, "quantiles_%s_%d.txt" % (name, _copies[0]))
    if not c["estimate"]:
        with open(path, "w") as f:
            f.write(training_file(name, dim, c["nq"]))
    h = L.qe_new(c["quantiles"], c["combination"], c["estimate"], c["mean"], c["variance"], c["nq"], c["of"], c["delta_alpha"], c["delta_gamma"],
                 c["delta_lr"], c["beta"], c["pool"], path.encode())
    return L, h, path


def run_segment(L, h, dim, nq, x):
    T = len(x)
    out = np.full((T, dim), np.nan, np.float32)
    par = np.full((6, dim), np.nan, np.float32)
    cq = np.full((nq + 1, dim), np.nan, np.float32)
    tq = np.full((nq + 1, dim), np.nan, np.float32)
    n = L.qe_segment(h, dim, T, np.ascontiguousarray(x), out, par, cq, tq)
    assert n == T, (n, T)
    return out, par, cq, tq


def run(tmp, so, extra_one_frame=None):
    """every recorded array of one build"""
    a = {}
    for name, (dim, _, segments) in CONFIGS.items():
        c = cfg_of(name)
        nq = c["nq"]
        L, h, path = new_object(tmp, so, name, dim)
        rec = {"out": [], "params": [], "cq_after": []}
        xs = [segment_input(name, i, dim, T, kind) for i, (T, kind) in enumerate(segments)]
        if name == "d20" and extra_one_frame is not None:
            xs.append(extra_one_frame)
        for x in xs:
            out, par, cq, tq = run_segment(L, h, dim, nq, x)
            if c["estimate"]:
                continue
            rec["out"].append(out)
            rec["params"].append(par[None])
            rec["cq_after"].append(cq[None])
            a[name + "/training_quantiles"] = tq
        if c["estimate"]:
            sums, count = np.zeros((nq + 1, dim), np.float64), C.c_uint()
            L.qe_sums(h, sums, C.byref(count))
            a[name + "/sums"], a[name + "/count"] = sums, np.array(count.value, np.uint64)
            with open(path, "rb") as f:
                a[name + "/file"] = np.frombuffer(f.read(), np.uint8)
        else:
            for k, v in rec.items():
                a[name + "/" + k] = np.concatenate(v)
    # the same training file read without pooling
    L, h, path = new_object(tmp, so, "d20_unpooled", 20)
    a["d20_unpooled/training_quantiles_check"] = run_segment(L, h, 20, 4, segment_input("d20_unpooled", 0, 20, 5, "plain"))[3]
    return a


def find_differing_one_frame(tmp, sos):
    """a one-frame segment of configuration d20 on which the two builds choose different (alpha, gamma)"""
    objs = {fl: new_object(tmp, so, "d20", 20) for fl, so in sos.items()}
    for seed in range(1, 200):
        x = segment_input("d20", 99, 20, 1, "plain", seed)
        par = {fl: run_segment(L, h, 20, 4, x)[1] for fl, (L, h, _) in objs.items()}
        if not same_bits(par["off"][:2], par["fma"][:2]):
            return x, seed
    sys.exit("make_quanteq_golden: no one-frame segment on which the builds differ")


def measure(tmp, so):
    out = {}
    for dim in (20, 40):
        for comb in (0, 1):
            name = "d20_c" if comb else "d20"
            L, h, _ = new_object(tmp, so, name, dim)
            x = segment_input("time", dim, dim, 1000, "plain")
            best = 1e9
            for _ in range(3):
                t0 = time.perf_counter()
                run_segment(L, h, dim, 4, x)
                best = min(best, time.perf_counter() - t0)
            out["cpu_seconds_per_segment/%d/%d" % (dim, comb)] = np.array(best)
    return out


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_quanteq.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_quanteq_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        sos = {}
        for fl in ("off", "fma"):
            sos[fl], n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)   # fused multiply-adds in the generated object (objdump)
        one_frame, seed = find_differing_one_frame(tmp, sos)
        arrays["one_frame_seed"] = np.array(seed)
        got = {fl: run(tmp, sos[fl], one_frame) for fl in ("off", "fma")}
        arrays.update(measure(tmp, sos["off"]))
        arrays["cpu_name"] = np.array(cpu_name())
    for name, (dim, _, segments) in CONFIGS.items():
        c = cfg_of(name)
        arrays["cfg/" + name] = np.array([dim] + [c[k] for k in DEFAULTS], np.float64)
        xs = [segment_input(name, i, dim, T, kind) for i, (T, kind) in enumerate(segments)]
        if name == "d20":
            xs.append(one_frame)
        arrays["in/" + name] = np.concatenate(xs)
        arrays["lengths/" + name] = np.array([len(x) for x in xs], np.int64)
        if not c["estimate"]:
            arrays["training_file/" + name] = np.frombuffer(training_file(name, dim, c["nq"]).encode(), np.uint8)
    arrays["cfg_fields"] = np.array(["dim"] + list(DEFAULTS))
    for k, v in got["off"].items():
        arrays["off/" + k] = v
    differ = [k for k, v in got["fma"].items() if not same_bits(v, got["off"][k])]
    for k in differ:
        arrays["fma/" + k] = got["fma"][k]
    arrays["fma_differs"] = np.array(differ if differ else [""])
    arrays["fma_arrays_compared"] = np.array(len(got["fma"]))
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    print("  fma instructions: off %d, fma %d" % (int(arrays["fma_instructions/off"]), int(arrays["fma_instructions/fma"])))
    print("  fma copies that differ from off: %d of %d %s" % (len(differ), len(got["fma"]), differ[:8]))
    print("  one-frame segment on which the builds differ: seed %d" % seed)
    for k in sorted(arrays):
        if k.startswith("cpu_seconds"):
            print("  %s = %.4f s (%s)" % (k, float(arrays[k]), cpu_name()))


if __name__ == "__main__":
    main()
