#!/usr/bin/env python3
"""tests/golden/make_vtln_golden.py -- writes tests/golden/ref_vtln.npz, the VTLN filter banks as the reference builds them.

Run it where the reference tree is mounted and `oracle/_ref/` has been built (`__graft_entry__.build()`); tests read only the
fixture.  What it compiles, in both of the reference's arithmetics (the flag sets of oracle/ref/Makefile: -msse3 = contract=off,
-msse3 -march=native = contract=fma):
  * the reference's own Math/PiecewiseLinearFunction.cc (add, normalize, invert; value and derive from its header), whole;
  * the filter builder and boundary function text of Signal/Filterbank.cc, taken by line range + SHA-256 through
    oracle/ref/extract_fn.py (imported, not changed), with that file's entry points ref_filter_boundary / Probe;
  * a small entry point of this file's own (ENTRY below) that composes them the way FilterBankNode::init and
    AnalyticFunctionFactory do: linear-2 built in the order of createTwoPieceLinearFunction (add(limit * max, factor),
    normalize(max), or the inverse of the function of 1 / factor), nest(mel | bark, linear-2), the maximum frequency through
    nest(warping, discrete-to-continuous), the boundary on that maximum and one FilterBuilder::create per centre.
The generated sources live in a temporary directory and are deleted with it; nothing of the reference's text is written here.

    python3 tests/golden/make_vtln_golden.py [out.npz]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/src"
REFDIR = os.path.join(ROOT, "oracle", "ref")
sys.path.insert(0, REFDIR)
import extract_fn  # noqa: E402  (oracle/ref/extract_fn.py: SPECS and the extraction by line range + SHA-256)

FACTORS = [0.80, 0.88, 0.94, 1.0, 1.06, 1.12, 1.20]
LIMITS = [0.875, 0.5]
# name -> the amx_mfcc_cfg fields the test sets, and the geometry the reference sees (fs, FFT length)
CONFIGS = [
    ("mfcc", dict(), 16000.0, 512),
    ("mfcc_nodiff", dict(warp_differential_unit=0), 16000.0, 512),
    ("plp16", dict(front_end=2, win_len_s=0.02, fft_max_input_s=0.02, preemph_alpha=0.0, mel_filter_width=3.8, mel_spacing=0.93853,
                   filter_type=1, boundary=1, warping=1, dct_normalize=1, n_autocorrelation=13, n_ceps=13), 16000.0, 512),
    ("plp16_nodiff", dict(front_end=2, win_len_s=0.02, fft_max_input_s=0.02, preemph_alpha=0.0, mel_filter_width=3.8, mel_spacing=0.93853,
                          filter_type=1, boundary=1, warping=1, dct_normalize=1, n_autocorrelation=13, n_ceps=13,
                          warp_differential_unit=0), 16000.0, 512),
    ("plp8", dict(front_end=2, sample_rate=8000.0, win_len_s=0.02, fft_max_input_s=0.02, preemph_alpha=0.0, mel_filter_width=3.8,
                  mel_spacing=0.973442, filter_type=1, boundary=1, warping=1, dct_normalize=1, n_autocorrelation=11, n_ceps=11), 8000.0, 256),
]
DEFAULT = dict(mel_filter_width=268.258, mel_spacing=0.0, filter_type=0, boundary=0, warping=0, warp_differential_unit=1)

ENTRY = r'''
// ---- this generator's own entry point (no reference text) ----
#include <Math/PiecewiseLinearFunction.hh>
extern "C" int vtln_bank(int type, int warping, int boundary, double factor, double limit, double width, double spacing, double ncp,
                         double bin_rate, int n_bins, int diff, double* fmax_out, int* start, int* end, int* offset, float* weights,
                         int cap) {
    Math::UnaryAnalyticFunctionRef d2c    = fb_scaling(1 / bin_rate);
    const double                   maxArg = d2c->value(n_bins - 1);
    Math::UnaryAnalyticFunctionRef plf;
    if (factor <= 1) {
        Math::PiecewiseLinearFunction* r = new Math::PiecewiseLinearFunction;
        r->add(limit * maxArg, factor);
        r->normalize(maxArg);
        plf = Math::UnaryAnalyticFunctionRef(r);
    }
    else {
        Math::PiecewiseLinearFunction inverse;
        inverse.add(limit * maxArg, 1 / factor);
        inverse.normalize(maxArg);
        plf = inverse.invert();
    }
    Math::UnaryAnalyticFunctionRef outer =
            warping == 0 ? Math::nest(fb_scaling(2595.0), Math::UnaryAnalyticFunctionRef(new Math::MelWarpingCore))
                         : Math::nest(fb_scaling(6.0), Math::nest(Math::UnaryAnalyticFunctionRef(new Math::Sinh)->invert(), fb_scaling(1.0 / 600.0)));
    Math::UnaryAnalyticFunctionRef warp = Math::nest(outer, plf);
    const double fmax = Math::nest(warp, d2c)->value(n_bins - 1);
    *fmax_out         = fmax;
    double w = 0, sp = 0, centres[256];
    const int nf = ref_filter_boundary(boundary, width, spacing, ncp, 0.0, fmax, &w, &sp, centres, 256);
    if (nf < 0 || nf > 256)
        return -1;
    int used = 0;
    for (int i = 0; i < nf; ++i) {
        int n = type == 0 ? Probe<Signal::SymmetricalTriangularFilterBuilder>().run(centres[i], w, 0.0, fmax, d2c, warp, diff != 0, start + i, end + i, weights + used, cap - used)
                          : Probe<Signal::TrapezeFilterBuilder>().run(centres[i], w, 0.0, fmax, d2c, warp, diff != 0, start + i, end + i, weights + used, cap - used);
        if (n < 0)
            return -2;
        offset[i] = used;
        used += n;
    }
    offset[nf] = used;
    return nf;
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-D_GNU_SOURCE", "-DSPRINT_RELEASE_BUILD",
         "-I" + REF, "-I/usr/include/libxml2", "-w"]


def build(tmp, flavour):
    assert "filter_build" in extract_fn.SPECS
    gen = os.path.join(tmp, "filter_build_%s.cc" % flavour)
    subprocess.check_call([sys.executable, os.path.join(REFDIR, "extract_fn.py"), "filter_build", gen], cwd=REFDIR)
    with open(gen, "a") as f:
        f.write(ENTRY)
    so = os.path.join(tmp, "vtln_%s.so" % flavour)
    lib = "ref" if flavour == "off" else "ref_native"
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen, os.path.join(REF, "Math", "PiecewiseLinearFunction.cc"),
                           "-L" + os.path.join(ROOT, "oracle", "_ref"), "-l" + lib, "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_ref")])
    L = C.CDLL(so)
    L.vtln_bank.restype = C.c_int
    L.vtln_bank.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_double] * 6 + [C.c_int, C.c_int, C.POINTER(C.c_double)] + [C.c_void_p] * 4 + [C.c_int]
    return L


def bank(L, cfg, fs, fft_len, factor, limit):
    c = dict(DEFAULT, **cfg)
    bin_rate = float("%g" % (fft_len / fs))   # the FFT node's "sample-rate" attribute, through its text form
    ncp = 2.5 / (1.3 - (-2.5)) if c["filter_type"] == 1 else 0.5
    width = c["mel_filter_width"]
    spacing = c["mel_spacing"] if c["mel_spacing"] != 0 else ncp * width
    cap = 20000
    st, en, off, w = np.zeros(256, np.int32), np.zeros(256, np.int32), np.zeros(257, np.int32), np.zeros(cap, np.float32)
    fmax = C.c_double(0)
    nf = L.vtln_bank(c["filter_type"], c["warping"], c["boundary"], factor, limit, width, spacing, ncp, bin_rate, fft_len // 2 + 1,
                     c["warp_differential_unit"], C.byref(fmax), st.ctypes.data, en.ctypes.data, off.ctypes.data, w.ctypes.data, cap)
    assert nf > 0, (cfg, factor, limit, nf)
    return st[:nf].copy(), en[:nf].copy(), off[:nf + 1].copy(), w[:off[nf]].copy(), fmax.value


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_vtln.npz")
    arrays = {"factors": np.array(FACTORS), "limits": np.array(LIMITS),
              "configs": np.array(json.dumps([[n, c] for n, c, _, _ in CONFIGS]))}
    with tempfile.TemporaryDirectory() as tmp:
        libs = {fl: build(tmp, fl) for fl in ("off", "fma")}
        for name, cfg, fs, fft_len in CONFIGS:
            for li, limit in enumerate(LIMITS):
                for fi, factor in enumerate(FACTORS):
                    got = {fl: bank(libs[fl], cfg, fs, fft_len, factor, limit) for fl in libs}
                    for fl, (st, en, off, w, fmax) in got.items():
                        key = "%s/%s/%d/%d" % (name, fl, li, fi)
                        if fl == "fma" and all(np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))
                                               for a, b in zip(got["off"], got["fma"])):
                            arrays[key + "/same_as_off"] = np.array(1)   # the two arithmetics agree: stored once
                            continue
                        arrays[key + "/start"], arrays[key + "/end"], arrays[key + "/offset"] = st.astype(np.int16), en.astype(np.int16), off
                        arrays[key + "/weights"], arrays[key + "/fmax"] = w, np.array(fmax)
    np.savez_compressed(out, **arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))


if __name__ == "__main__":
    main()
