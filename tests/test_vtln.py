"""CPU: VTLN filter banks (amx_mfcc_create_vtln / amx_mfcc_tables_vtln / amx_mfcc_plan_create_vtln) on host-only handles.

warping-function = nest(linear-2(factor, limit), mel | bark): factor 1 is the unwarped bank bit for bit, every factor keeps the
filter count and the descriptor and plan arguments are checked with named messages.  No kernel runs here."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

from rasr_amd import _lib

# plp.flow's parameter values (amx_plp_default_cfg), at 16 and 8 kHz
PLP16 = dict(front_end=2, win_len_s=0.02, fft_max_input_s=0.02, preemph_alpha=0.0, mel_filter_width=3.8, mel_spacing=0.93853,
             filter_type=1, boundary=1, warping=1, dct_normalize=1, n_autocorrelation=13, n_ceps=13)
PLP8 = dict(PLP16, sample_rate=8000.0, mel_spacing=0.973442, n_autocorrelation=11, n_ceps=11)
CONFIGS = {
    "mfcc": dict(),
    "mfcc40": dict(n_ceps=40, mel_filter_width=138.0),
    "mfcc_nodiff": dict(warp_differential_unit=0),
    "plp16": PLP16,
    "plp8": PLP8,
    "plp16_nodiff": dict(PLP16, warp_differential_unit=0),
}
FACTORS = [0.80, 0.88, 0.94, 1.0, 1.06, 1.12, 1.20]


def cfg_of(contract="off", **kw):
    L = _lib.lib()
    cfg = _lib.MfccCfg()
    L.amx_mfcc_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    cfg.tuning = ("contract=%s" % contract).encode()
    return cfg


class Handle:
    def __init__(self, cfg, factors=None, limit=0.875):
        self.L = _lib.lib()
        self.h = C.c_void_p()
        if factors is None:
            self.status = self.L.amx_mfcc_create(None, C.byref(cfg), C.byref(self.h))
        else:
            self.wf = np.ascontiguousarray(factors, np.float64)
            vt = _lib.MfccVtln(limit, len(self.wf), self.wf.ctypes.data if len(self.wf) else None)
            self.status = self.L.amx_mfcc_create_vtln(None, C.byref(cfg), C.byref(vt), C.byref(self.h))
        self.error = self.L.amx_last_error().decode() if self.status else ""

    def __del__(self):
        if self.h:
            self.L.amx_mfcc_destroy(self.h)

    def info(self):
        i = _lib.MfccInfo()
        _lib.check(self.L.amx_mfcc_describe(self.h, C.byref(i)))
        return i

    def tables(self, factor=None):
        i = self.info()
        win = np.zeros(i.frame_len, np.float32)
        fs, fe, fo = (np.zeros(i.n_filters, np.int32), np.zeros(i.n_filters, np.int32), np.zeros(i.n_filters + 1, np.int32))
        get = self.L.amx_mfcc_tables if factor is None else (lambda *a: self.L.amx_mfcc_tables_vtln(a[0], factor, *a[1:]))
        _lib.check(get(self.h, None, None, None, fo.ctypes.data, None, None))
        fw = np.zeros(int(fo[-1]), np.float32)
        dct = np.zeros((i.n_transform, i.n_transform_inputs), np.float32)
        _lib.check(get(self.h, win.ctypes.data, fs.ctypes.data, fe.ctypes.data, fo.ctypes.data, fw.ctypes.data, dct.ctypes.data))
        return dict(window=win, filter_start=fs, filter_end=fe, filter_offset=fo, filter_weights=fw, dct=dct)


def same_bits(a, b):
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                                    np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_factor_one_is_the_unwarped_bank_bit_for_bit(name, contract):
    cfg = cfg_of(contract, **CONFIGS[name])
    plain = Handle(cfg)
    assert plain.status == 0, plain.error
    want = plain.tables()
    for limit in (0.875, 0.5):
        v = Handle(cfg, FACTORS, limit)
        assert v.status == 0, v.error
        assert same_bits(v.tables(1.0), want)
        # a one-factor handle at 1.0 is the plain handle, through every entry point that takes no factor
        one = Handle(cfg, [1.0], limit)
        assert same_bits(one.tables(), want) and same_bits(one.tables(1.0), want)
        assert one.info().mel_max == plain.info().mel_max


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_every_factor_keeps_the_filter_count_and_factor_zero_is_the_default(name, contract):
    cfg = cfg_of(contract, **CONFIGS[name])
    n = Handle(cfg).info().n_filters
    for first in (0.88, 1.12):
        fac = [first] + [f for f in FACTORS if f != first]
        v = Handle(cfg, fac)
        assert v.status == 0, v.error
        assert v.info().n_filters == n
        assert same_bits(v.tables(), v.tables(first))
        unwarped = v.tables(1.0)
        for f in fac:
            t = v.tables(f)
            assert len(t["filter_start"]) == n
            assert np.array_equal(t["window"], unwarped["window"]) and np.array_equal(t["dct"], unwarped["dct"])
            if f != 1.0:  # the warping moves the filters' edges or weights
                assert not (np.array_equal(t["filter_start"], unwarped["filter_start"]) and
                            np.array_equal(t["filter_end"], unwarped["filter_end"]) and
                            np.array_equal(t["filter_weights"], unwarped["filter_weights"]))


def two_piece(factor, limit, mx):
    """linear-2 restated in Python (f64, contract=off): (limits, slopes, offsets), first limit >= x selects a segment"""
    def build(a1):
        lim, a, b = [limit * mx], [a1], [0.0]
        v = a1 * lim[0] + 0.0
        a2 = (mx - v) / (mx - lim[0])
        lim.append(sys.float_info.max), a.append(a2), b.append(v - a2 * lim[0])
        return lim, a, b

    def value(f, x):
        i = next((k for k, L in enumerate(f[0]) if L >= x), len(f[0]) - 1)
        return f[1][i] * x + f[2][i]

    def invert(f):
        return ([value(f, L) for L in f[0]], [1.0 / a for a in f[1]], [-b / a for a, b in zip(f[1], f[2])])
    return build(factor) if factor <= 1 else invert(build(1 / factor)), value, invert


@pytest.mark.parametrize("factor", FACTORS)
def test_filter_edges_against_a_python_restatement(factor):
    """mfcc.flow (mel, triangular, stretch-to-cover), contract=off: the filters' first and last bins follow plf^-1(mel^-1(edge))"""
    cfg = cfg_of("off")
    v = Handle(cfg, [factor])
    assert v.status == 0, v.error
    i = v.info()
    t = v.tables()
    rate = float("%g" % i.fft_output_sample_rate)
    d2c = lambda k: (1 / rate) * k  # noqa: E731
    mx = d2c(i.n_bins - 1)
    plf, value, invert = two_piece(factor, 0.875, mx)
    inv = invert(plf)
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)  # noqa: E731
    mel_inv = lambda m: (math.pow(10, (1 / 2595.0) * m) - 1.0) * 700.0  # noqa: E731
    f_max = mel(value(plf, mx))
    assert i.mel_max == f_max
    width, spacing = 268.258, 0.5 * 268.258
    nf = i.n_filters
    coverage = (spacing * (nf - 1) + width) / f_max
    width, spacing = width / coverage, spacing / coverage
    for k in range(nf):
        centre = 0.5 * width + (spacing * k + 0.0)
        first = (1 / (1 / rate)) * value(inv, mel_inv(max(-0.5 * width + centre, 0.0)))
        first = round(first) if abs(first - round(first)) < 1e-10 else math.ceil(first)
        last = (1 / (1 / rate)) * value(inv, mel_inv(min(0.5 * width + centre, f_max)))
        last = round(last) + 1 if abs(last - round(last)) < 1e-10 else math.ceil(last)
        assert (t["filter_start"][k], t["filter_end"][k]) == (first, last), k


@pytest.mark.parametrize("limit", [0.0, 1.0, 1.5, -0.2, float("nan")])
def test_limit_outside_the_open_unit_interval_is_refused(limit):
    v = Handle(cfg_of(), [1.0], limit)
    assert v.status == _lib.AMX_ERR_INVALID and "limit" in v.error


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_non_positive_or_non_finite_factor_is_refused(bad):
    v = Handle(cfg_of(), [1.0, bad])
    assert v.status == _lib.AMX_ERR_INVALID and "warping factor 1" in v.error, v.error


def test_duplicate_factor_and_factor_counts_are_refused():
    v = Handle(cfg_of(), [0.9, 1.0, 0.9])
    assert v.status == _lib.AMX_ERR_INVALID and "warping factors 0 and 2" in v.error, v.error
    v = Handle(cfg_of(), [])
    assert v.status == _lib.AMX_ERR_INVALID and "n_factors" in v.error
    ok = Handle(cfg_of(), list(np.linspace(0.8, 1.2, _lib.AMX_MFCC_MAX_WARPING_FACTORS)))
    assert ok.status == 0, ok.error
    v = Handle(cfg_of(), list(np.linspace(0.8, 1.2, _lib.AMX_MFCC_MAX_WARPING_FACTORS + 1)))
    assert v.status == _lib.AMX_ERR_INVALID and "n_factors" in v.error


def test_unknown_factor_is_refused_by_tables_and_plans():
    L = _lib.lib()
    v = Handle(cfg_of(), [0.9, 1.0, 1.1])
    assert v.status == 0, v.error
    fo = np.zeros(v.info().n_filters + 1, np.int32)
    assert L.amx_mfcc_tables_vtln(v.h, 0.95, None, None, None, fo.ctypes.data, None, None) == _lib.AMX_ERR_INVALID
    assert b"not one of the handle's" in L.amx_last_error()
    off = np.array([0, 100, 200, 300], np.int64)
    wf = np.array([0.9, 1.1, 1.05])
    p = C.c_void_p()
    assert L.amx_mfcc_plan_create_vtln(v.h, 3, off.ctypes.data, wf.ctypes.data, C.byref(p)) == _lib.AMX_ERR_INVALID
    assert b"segment 2" in L.amx_last_error()
    # a plain handle has the one factor 1
    plain = Handle(cfg_of())
    assert L.amx_mfcc_tables_vtln(plain.h, 1.0, None, None, None, fo.ctypes.data, None, None) == 0
    assert L.amx_mfcc_tables_vtln(plain.h, 0.9, None, None, None, fo.ctypes.data, None, None) == _lib.AMX_ERR_INVALID


def test_python_extractor_on_a_host_only_handle():
    import rasr_amd
    fe = rasr_amd.MfccExtractor(None, warping_factors=[1.1, 1.0], vtln_limit=0.875)
    assert fe.warping_factors == (1.1, 1.0)
    t = fe.tables()
    assert same_bits(t, fe.tables(1.1))
    plain = rasr_amd.MfccExtractor(None)
    assert same_bits(fe.tables(1.0), plain.tables())
    with pytest.raises(rasr_amd.AmxError, match="not one of the handle"):
        fe.tables(0.9)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vtln.npz")


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_tables_against_the_reference_fixture(contract):
    """every bank of the grid factors {0.80 .. 1.20} x limits {0.875, 0.5} on mfcc.flow, plp.flow at 16 and 8 kHz, with and without
    warp-differential-unit, against the reference's own PiecewiseLinearFunction and filter-builder text compiled in the build of
    that contract (tests/golden/make_vtln_golden.py): start, end, offset, weights and the warped maximum frequency, bit for bit;
    the window against the unwarped handle's"""
    z = np.load(GOLDEN)
    factors, limits = [float(f) for f in z["factors"]], [float(v) for v in z["limits"]]
    checked = 0
    for name, fields in json.loads(str(z["configs"])):
        cfg = cfg_of(contract, **fields)
        window = Handle(cfg).tables()["window"]
        for li, limit in enumerate(limits):
            v = Handle(cfg, factors, limit)
            assert v.status == 0, v.error
            for fi, f in enumerate(factors):
                key = "%s/%s/%d/%d" % (name, contract, li, fi)
                if key + "/same_as_off" in z.files:
                    key = "%s/off/%d/%d" % (name, li, fi)
                t = v.tables(f)
                assert np.array_equal(t["filter_start"], z[key + "/start"].astype(np.int32)), key
                assert np.array_equal(t["filter_end"], z[key + "/end"].astype(np.int32)), key
                assert np.array_equal(t["filter_offset"], z[key + "/offset"]), key
                assert np.array_equal(t["filter_weights"].view(np.uint32), z[key + "/weights"].view(np.uint32)), key
                assert np.array_equal(t["window"].view(np.uint32), window.view(np.uint32))
                one = Handle(cfg, [f], limit)
                assert one.info().mel_max == float(z[key + "/fmax"]), key
                checked += 1
    assert checked == 5 * 2 * 7
