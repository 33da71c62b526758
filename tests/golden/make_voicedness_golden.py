#!/usr/bin/env python3
"""tests/golden/make_voicedness_golden.py -- writes tests/golden/ref_voicedness.npz: voicedness.flow's arithmetic as the reference's
own text computes it.

Run it where the reference tree is mounted and `oracle/_ref/` has been built (`__graft_entry__.build()`); tests read only the
fixture.  What it compiles, in both of the reference's arithmetics (the flag sets of oracle/ref/Makefile: -msse3 = contract=off,
-msse3 -march=native = contract=fma), taken by line range + SHA-256 into a temporary directory that is deleted afterwards:
  * Signal/FastFourierTransform.hh:24-219 and .cc:21-142: the classes FastFourierTransform, RealFastFourierTransform,
    RealInverseFastFourierTransform (padding, unpack / pack, the scaling by the sample rate) on Math::FastFourierTransform, which
    oracle/_ref/libref.so / libref_native.so hold compiled from Math/FastFourierTransform.cc unmodified;
  * Signal/CrossCorrelation.hh:33-49 (normalizeCrossCorrelationEstimate), :193-198 (normalize) and .cc:31-64
    (CrossCorrelation::crossCorrelation, with Math::conjugateMultiplies from Math/Complex.hh as it is) behind a class shell that
    declares the members the text uses (the real header pulls in Flow/Node.hh);
  * Signal/PeakDetection.cc:42-68, 92-98, 252-261 (getMaximalPeakIndex, getMaximalPeakValue, init) behind a shell with the members of
    PeakDetection.hh:33-44 in the reference's types (the continuous positions are f32);
  * the mean-energy normaliser through ref_vector_normalize of the same libraries (oracle/ref/extract_fn.py "vector_normalization").
An entry point of this file's own (ENTRY) drives them the way CrossCorrelation::apply and PeakDetectionNode::work do.

Recorded: s16-valued frames (voiced, noise, a short last frame padded by the resize node, digital silence, a constant), their
normalised autocorrelation in both builds (the contract=fma copy only where its bits differ), the forward spectrum of two frames,
the peak index / value on every recorded autocorrelation vector and on a few hundred short integer vectors with plateaus.

    python3 tests/golden/make_voicedness_golden.py [out.npz]
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
sys.path.insert(0, ROOT)

# (file, first line, last line): the reference text, in the order it is written out; SHA-256 of the concatenation below
PIECES = {
    "fft_hh": [("Signal/FastFourierTransform.hh", 24, 219)],
    "fft_cc": [("Signal/FastFourierTransform.cc", 21, 142)],
    "estimate": [("Signal/CrossCorrelation.hh", 33, 49)],
    "normalize": [("Signal/CrossCorrelation.hh", 193, 198)],
    "xcorr": [("Signal/CrossCorrelation.cc", 31, 64)],
    "peak": [("Signal/PeakDetection.cc", 42, 68), ("Signal/PeakDetection.cc", 92, 98), ("Signal/PeakDetection.cc", 252, 261)],
}
SHA = "0770f6c42528d15cf34ff197f61e4caebf7cd9333664c32603571fecb0498bc2"

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/StringUtilities.hh>
#include <Core/Types.hh>
#include <Core/Utility.hh>
#include <Math/Complex.hh>
#include <Math/FastFourierTransform.hh>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <numeric>
#include <string>
#include <vector>
namespace Signal {
// ---- reference text: Signal/FastFourierTransform.hh ----
%(fft_hh)s
// ---- reference text: CrossCorrelation.hh, the unbiased-estimate functor ----
%(estimate)s
// ---- shell: the members CrossCorrelation::crossCorrelation and normalize use (CrossCorrelation.hh:129-156)
class CrossCorrelation {
public:
    typedef f32 Data;
    std::vector<Data> X_;
    std::vector<Data> Y_;
    s32 begin_;
    s32 end_;
    void crossCorrelation(const std::vector<Data>& x, const std::vector<Data>& y, std::vector<Data>& Rxy);
// ---- reference text: CrossCorrelation.hh, normalize ----
%(normalize)s
};
// ---- shell: the members of PeakDetection.hh:33-44 in the reference's types
class PeakDetection {
public:
    typedef f32 Amplitude;
    f32  continuousMinPosition_;
    u32  minPosition_;
    f32  continuousMaxPosition_;
    u32  maxPosition_;
    f32  continuousMaxWidth_;
    u32  maxWidthHalf_;
    f32  continuousHeightAverageWidth_;
    u32  heightAverageWidthHalf_;
    f64  sampleRate_;
    bool needInit_;
    u32       getMaximalPeakIndex(const std::vector<Amplitude>& v) const;
    Amplitude getMaximalPeakValue(const std::vector<Amplitude>& v);
    void      init();
};
}  // namespace Signal
using namespace Signal;
// ---- reference text: Signal/FastFourierTransform.cc ----
%(fft_cc)s
using namespace Core;   // CrossCorrelation.cc:19, PeakDetection.cc:20
// ---- reference text: CrossCorrelation::crossCorrelation ----
%(xcorr)s
// ---- reference text: PeakDetection::getMaximalPeakIndex, getMaximalPeakValue, init ----
%(peak)s
// ---- this generator's own entry points (no reference text) ----
// CrossCorrelation::apply with x = y, similarity multiplication, use-fft, normalization none (0) | unbiased-estimate (1)
extern "C" void vc_autocorrelation(const float* x, int size, int begin, int end, int unbiased, float* out) {
    std::vector<f32> v(x, x + size), R;
    CrossCorrelation cc;
    cc.begin_ = begin;
    cc.end_   = end;
    cc.crossCorrelation(v, v, R);
    if (unbiased)
        cc.normalize(v, v, R, normalizeCrossCorrelationEstimate<f32>(v, v));
    std::memcpy(out, R.data(), R.size() * sizeof(f32));
}
// RealFastFourierTransform(length) with the default sample rate; out: fft length + 2 values; returns the fft length
extern "C" int vc_real_fft(const float* x, int size, int length, float* out) {
    std::vector<f32> v(x, x + size);
    RealFastFourierTransform fft(length);
    if (!fft.transform(v))
        return -1;
    std::memcpy(out, v.data(), v.size() * sizeof(f32));
    return (int)fft.length();
}
// PeakDetectionNode: continuous positions (f32 members) and the sample rate, maximal-peak-value; index_out: getMaximalPeakIndex
extern "C" float vc_peak(const float* a, int n, float min_position, float max_position, double sample_rate, unsigned* index_out,
                         unsigned* min_out, unsigned* max_out) {
    std::vector<f32> v(a, a + n);
    PeakDetection p;
    p.continuousMinPosition_ = min_position;
    p.continuousMaxPosition_ = max_position;
    p.continuousMaxWidth_ = p.continuousHeightAverageWidth_ = 0;
    p.sampleRate_ = sample_rate;
    p.needInit_   = true;
    const float value = p.getMaximalPeakValue(v);
    *index_out        = p.getMaximalPeakIndex(v);
    *min_out          = p.minPosition_;
    *max_out          = p.maxPosition_;
    return value;
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-D_GNU_SOURCE", "-DSPRINT_RELEASE_BUILD",
         "-I" + REF, "-I/usr/include/libxml2", "-w"]


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
    gen = os.path.join(tmp, "voicedness_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "voicedness_%s.so" % flavour)
    lib = "ref" if flavour == "off" else "ref_native"
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen, "-L" + os.path.join(ROOT, "oracle", "_ref"), "-l" + lib,
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_ref")])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    L.vc_autocorrelation.restype = None
    L.vc_autocorrelation.argtypes = [f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p]
    L.vc_real_fft.restype = C.c_int
    L.vc_real_fft.argtypes = [f32p, C.c_int, C.c_int, f32p]
    L.vc_peak.restype = C.c_float
    L.vc_peak.argtypes = [f32p, C.c_int, C.c_float, C.c_float, C.c_double] + [C.POINTER(C.c_uint)] * 3
    L.ref_vector_normalize.restype = None
    L.ref_vector_normalize.argtypes = [C.c_int, f32p, C.c_int, f32p]
    return L, int(fma or 0)


def frames_for(fs):
    """s16-valued frames of the resize node's output length"""
    from tests import voicedness_cases as cases
    n = int(round(0.040 * fs))
    k = 24 if fs == 16000.0 else 16
    v, u = cases.voiced(3 * n + 4 * k, fs, seed=51), cases.unvoiced(3 * n + 4 * k, fs, seed=52)
    p = cases.pulses(3 * n + 4 * k, fs, seed=53)
    rows = []
    for i in range(k - 4):
        src = (v, u, p)[i % 3]
        rows.append(src[37 * i:37 * i + n])
    short = np.zeros(n, np.float32)
    short[:n // 3] = v[:n // 3]           # a short last frame behind signal-vector-f32-resize
    rows += [short, np.zeros(n, np.float32), np.full(n, 250, np.float32), np.tile(np.array([500, 500, -500, -500], np.float32), n // 4)]
    return np.array(rows, np.float32)


def peak(L, a, mn, mx, fs):
    i, lo, hi = C.c_uint(), C.c_uint(), C.c_uint()
    v = L.vc_peak(np.ascontiguousarray(a, np.float32), len(a), mn, mx, fs, C.byref(i), C.byref(lo), C.byref(hi))
    return v, i.value, lo.value, hi.value


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_voicedness.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_voicedness_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        libs = {}
        for fl in ("off", "fma"):
            libs[fl], n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)   # fused multiply-adds in the generated object (objdump)
        for fs in (16000.0, 8000.0):
            tag = "%d" % fs
            raw = frames_for(fs)
            n = raw.shape[1]
            arrays[tag + "/frames"] = raw.astype(np.int16)
            got = {}
            for fl, L in libs.items():
                norm, acf, raw_acf = np.zeros_like(raw), np.zeros((len(raw), n), np.float32), np.zeros((2, n), np.float32)
                for r in range(len(raw)):
                    L.ref_vector_normalize(3, raw[r], n, norm[r])
                    L.vc_autocorrelation(norm[r], n, 0, n, 1, acf[r])
                for r in range(2):
                    L.vc_autocorrelation(norm[r], n, 0, n, 0, raw_acf[r])
                spec = np.zeros((2, 4 * n + 2), np.float32)
                lens = [L.vc_real_fft(norm[r], n, 2 * n - 1, spec[r]) for r in range(2)]
                spec = spec[:, :lens[0] + 2].copy()
                mn, mx = (0.0025, 0.0167)
                pk = [peak(L, a, mn, mx, fs) for a in acf]
                got[fl] = dict(normalized=norm, acf=acf, acf_none=raw_acf, spectrum=spec,
                               peak_value=np.array([p[0] for p in pk], np.float32), peak_index=np.array([p[1] for p in pk], np.uint32),
                               positions=np.array(pk[0][2:], np.uint32))
            for fl in got:
                for k, v in got[fl].items():
                    if k == "normalized":   # restated by the test from the frames; kept only as a statement about the two builds
                        arrays["%s/%s/normalized_same_as_off" % (tag, fl)] = np.array(int(same_bits(v, got["off"][k])))
                        continue
                    if fl == "fma" and same_bits(v, got["off"][k]):
                        arrays["%s/fma/%s_same_as_off" % (tag, k)] = np.array(1)
                        continue
                    arrays["%s/%s/%s" % (tag, fl, k)] = v
        # the peak scan on short integer vectors: plateaus, ties, monotone stretches; positions in samples at sample rate 1
        rng = np.random.Generator(np.random.PCG64(7))
        vecs = rng.integers(-3, 4, (400, 24)).astype(np.int8)
        rngs = np.array([(rng.integers(0, 10), 0) for _ in range(400)], np.int32)
        rngs[:, 1] = rngs[:, 0] + rng.integers(1, 12, 400)
        res = {}
        for fl, L in libs.items():
            pk = [peak(L, v.astype(np.float32), float(a), float(b), 1.0) for v, (a, b) in zip(vecs, rngs)]
            res[fl] = (np.array([p[0] for p in pk], np.float32), np.array([p[1] for p in pk], np.uint32))
        assert same_bits(res["off"][0], res["fma"][0]) and same_bits(res["off"][1], res["fma"][1])
        arrays["scan/vectors"], arrays["scan/ranges"] = vecs, rngs
        arrays["scan/value"], arrays["scan/index"] = res["off"]
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    for k in sorted(arrays):
        if "same_as_off" in k or "fma_instructions" in k:
            print("  %s = %d" % (k, int(arrays[k])))


if __name__ == "__main__":
    main()
