"""CPU: the voicedness front end's restatement (tests/voicedness_reference.py) against the reference's own text
(tests/golden/ref_voicedness.npz, written by tests/golden/make_voicedness_golden.py from both builds of the reference), against the
nodes' definitions, the peak scan on cases written by hand, the excuse rule of the end-to-end GPU test, and the ABI surface (geometry,
refusals) without a device."""
import ctypes as C
import os

import numpy as np
import pytest

from rasr_amd import _lib
from tests import voicedness_cases as cases
from tests import voicedness_reference as V


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_voicedness.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def golden(g, tag, build, key):
    """the recorded array of a build; the contract=fma copy is stored only where its bits differ from contract=off"""
    name = "%s/%s/%s" % (tag, build, key)
    return g[name] if name in g.files else g["%s/off/%s" % (tag, key)]


@pytest.mark.parametrize("fs", [16000.0, 8000.0])
def test_restatement_against_the_references_own_text(fs):
    """the bar: autocorrelation within 1e-4 |ref| + 1e-4 R[0], peak index and value exact on the golden vectors.  Held with room:
    the restatement has the BITS of both builds (spectrum, plain and normalised autocorrelation), NaN frames included."""
    g = np.load(GOLDEN)
    tag = "%d" % fs
    geo = V.geometry(fs)
    frames = g[tag + "/frames"].astype(np.float32)
    assert frames.shape[1] == geo["frame_len"]
    assert tuple(g[tag + "/off/positions"]) == (geo["min_position"], geo["max_position"])
    assert int(g[tag + "/off/normalized_same_as_off"]) == 1 and int(g[tag + "/fma/normalized_same_as_off"]) == 1
    x = V.normalize(frames)
    spec = V.real_fft(x[:2], geo["fft_len"])
    for build in ("off", "fma"):
        want = golden(g, tag, build, "acf")
        mine = V.autocorrelation(x, geo["n_lags"], contract=build)
        assert np.array_equal(np.isnan(mine), np.isnan(want)) and np.isnan(want).any()
        fin = ~np.isnan(want)
        assert np.all(np.abs(mine[fin] - want[fin]) <= cases.acf_bar(np.where(fin, want, 1))[fin]), build
        assert np.array_equal(bits(mine)[fin], bits(want)[fin]), (build, int((bits(mine)[fin] != bits(want)[fin]).sum()))
        assert np.array_equal(bits(V.autocorrelation(x[:2], geo["n_lags"], "none", contract=build)), bits(golden(g, tag, build, "acf_none")))
        assert np.array_equal(bits(spec), bits(golden(g, tag, build, "spectrum")))
        # the peak scan on the golden vectors: index and value exact
        idx = [V.maximal_peak_index(a.tolist(), geo["min_position"], geo["max_position"]) for a in want]
        val = np.array([V.maximal_peak_value(a.tolist(), geo["min_position"], geo["max_position"]) for a in want], np.float32)
        assert idx == golden(g, tag, build, "peak_index").tolist(), build
        assert np.array_equal(bits(val), bits(golden(g, tag, build, "peak_value"))), build
    # the two builds do differ, in X conj(X) only (the restatement's contract switch): most lags by a last bit
    assert not np.array_equal(bits(g[tag + "/off/acf"]), bits(g[tag + "/fma/acf"]))
    assert int(g["fma_instructions/off"]) == 0 and int(g["fma_instructions/fma"]) > 0


def test_peak_scan_against_the_references_own_text():
    g = np.load(GOLDEN)
    for v, (mn, mx), value, index in zip(g["scan/vectors"], g["scan/ranges"], g["scan/value"], g["scan/index"]):
        got = peak(v, int(mn), int(mx))
        assert got[0] == int(index) and bits(np.float32(got[1])) == bits(value), (v, mn, mx, got, index, value)
    assert (g["scan/index"] == V.U32_MAX).sum() > 10 and (g["scan/index"] != V.U32_MAX).sum() > 100


def peak(v, mn, mx):
    v = np.asarray(v, np.float32).tolist()
    return V.maximal_peak_index(v, mn, mx), V.maximal_peak_value(v, mn, mx)


def test_peak_scan_hand_cases():
    none = V.U32_MAX
    # a plain peak inside the range
    assert peak([0, 1, 3, 1, 0, 0], 1, 4) == (2, 3)
    # plateau: begin 2, end 4, midpoint 3
    assert peak([0, 1, 5, 5, 5, 2, 0], 1, 5) == (3, 5)
    # even plateau: (2 + 3) / 2 = 2
    assert peak([0, 1, 5, 5, 2, 0], 1, 4) == (2, 5)
    # a plateau that never falls (rises again) is no peak; the later peak is taken
    assert peak([0, 1, 5, 5, 6, 2, 0], 1, 5) == (4, 6)
    # peak straddling min-position: begin 1 < min 3 <= end 4 qualifies; midpoint 2 is clamped to 3, the value is read THERE
    assert peak([0, 7, 7, 7, 7, 1, 0, 0], 3, 6) == (3, 7)
    # peak straddling max-position: begin 3 <= max 3 qualifies, midpoint 4 clamped to 3
    assert peak([0, 0, 1, 7, 7, 7, 1, 0], 1, 3) == (3, 7)
    # peak entirely in front of min-position / behind max-position does not qualify
    assert peak([0, 9, 0, 0, 1, 0, 0], 3, 5) == (4, 1)
    assert peak([0, 1, 0, 0, 0, 9, 0], 1, 3) == (1, 1)
    # clamping reads the value at the clamped index, which need not be the peak's: peak (begin 1, end 1) with min 1, max 1 is itself;
    # peak begin 4 > max: no; so take a peak whose midpoint lies left of min: begin 1, end 2 (qualifies by end >= min = 2), midpoint 1 -> 2
    assert peak([0, 4, 4, 1, 0, 0], 2, 4) == (2, 4)
    # monotone input: no peak, value 0
    assert peak([0, 1, 2, 3, 4, 5], 1, 4) == (none, 0)
    assert peak([5, 4, 3, 2, 1, 0], 1, 4) == (none, 0)
    assert peak([2, 2, 2, 2, 2], 1, 3) == (none, 0)
    # peak at the last index has no fall behind it: not a peak; at the last but one it is
    assert peak([0, 1, 0, 1, 2], 1, 3) == (1, 1)
    assert peak([0, 1, 0, 3, 2], 1, 3) == (3, 3)
    # a plateau running to the end never falls
    assert peak([0, 1, 0, 3, 3], 1, 3) == (1, 1)
    # equal maxima: the first wins (the comparison is strict)
    assert peak([0, 5, 0, 5, 0, 5, 0], 1, 5) == (1, 5)
    assert peak([0, 5, 0, 6, 0, 6, 0], 1, 5) == (3, 6)
    # NaNs compare false everywhere
    assert peak([np.nan] * 6, 1, 4) == (none, 0)
    # -0.0 == 0.0: a plateau of mixed zeros is walked
    i, v = peak([-1, 0.0, -0.0, -1, -2], 1, 3)
    assert i == 1 and v == 0


def test_geometry_follows_the_nodes_rounding():
    assert V.geometry(16000.0) == dict(frame_len=640, frame_shift=160, n_lags=640, min_position=40, max_position=267, fft_len=2048)
    assert V.geometry(8000.0) == dict(frame_len=320, frame_shift=80, n_lags=320, min_position=20, max_position=134, fft_len=1024)


@pytest.mark.parametrize("fs", [16000.0, 8000.0])
def test_restatement_against_an_independent_f64_autocorrelation(fs):
    """f32 reference arithmetic against numpy's f64 FFT on the same normalised frames: within the front-end bar; R[0] of a full frame
    is the mean energy, 1"""
    g = V.geometry(fs)
    for name, x in cases.end_to_end_inputs(fs).items():
        x = x[:int(fs) // 2 + 57]
        fr = V.normalize(V.frames(x, g["frame_len"], g["frame_shift"]))
        acf = V.autocorrelation(fr, g["n_lags"])
        F = np.fft.rfft(fr.astype(np.float64), g["fft_len"], axis=1)
        want = np.fft.irfft(np.abs(F) ** 2, g["fft_len"], axis=1)[:, :g["n_lags"]] / (g["frame_len"] - np.arange(g["n_lags"]))
        assert np.all(np.abs(acf - want) <= cases.acf_bar(want)), name
        assert np.allclose(acf[:-4, 0], 1, atol=1e-5)
        none = V.autocorrelation(fr, g["n_lags"], "none")
        assert np.allclose(none[:-4, 0], g["frame_len"], rtol=1e-5)


def test_definition_pulse_train_noise_constant():
    fs = 16000.0
    # NOT voicedness.flow's range: with max-position .0167 (lag 267) the peaks at lags 80, 160 and 240 of an exact pulse train are
    # equally high up to rounding and the scan takes 80 or 160 depending on the last bit; .0075 leaves one period inside [min, max]
    g = V.geometry(fs, max_position_s=0.0075)
    x = np.zeros(8000, np.float32)
    x[::80] = 1000
    out, acf = V.voicedness(x, fs, return_acf=True, max_position_s=0.0075)
    idx = [V.maximal_peak_index(a.tolist(), g["min_position"], g["max_position"]) for a in acf]
    assert all(i == 80 for i in idx[:-4]) and np.allclose(out[:-4], 1, atol=1e-5)
    rng = np.random.Generator(np.random.PCG64(5))
    noise = V.voicedness(np.rint(3000 * rng.standard_normal(16000)).astype(np.float32), fs)
    # "near 0": an autocorrelation estimate over 640 - m >= 373 independent products has a standard deviation of at most 1 / sqrt(373)
    # = 0.052 and the peak is the largest of about 230 lags: below 0.25 (4.8 sigma) for every frame
    assert np.all(np.abs(noise[:-4]) < 0.25) and abs(float(noise[:-4].mean())) < 0.15
    const = V.voicedness(np.full(4000, 123, np.float32), fs, return_acf=True)[1]
    # the unbiased estimate of a constant signal is constant: within the front-end bar (the last lags divide the transform pair's
    # f32 round-off, about 640 * 2^-24 absolute, by N = 1, 2, ...)
    assert np.all(np.abs(const[:-4] - 1) <= cases.acf_bar(np.ones_like(const[:-4])))
    silent, sacf = V.voicedness(np.zeros(2000, np.float32), fs, return_acf=True)
    assert np.all(np.isnan(sacf)) and np.all(silent == 0)   # 0 * (1 / 0): NaN everywhere, no peak


@pytest.mark.parametrize("fs", [16000.0, 8000.0])
def test_excuse_rule_stays_under_the_cap(fs):
    """the end-to-end test excuses a frame only for a near-tie in the reference autocorrelation; with the restatement's own
    autocorrelation perturbed by +- the bar, at most 1 % of an input's frames are excused and every other frame keeps its value"""
    g = V.geometry(fs)
    mn, mx = g["min_position"], g["max_position"]
    rng = np.random.Generator(np.random.PCG64(99))
    for name, x in cases.end_to_end_inputs(fs).items():
        out, acf = V.voicedness(x, fs, return_acf=True)
        pert = (acf + rng.choice([-1.0, 1.0], acf.shape) * cases.acf_bar(acf)).astype(np.float32)
        got = np.array([V.maximal_peak_value(a.tolist(), mn, mx) for a in pert], np.float32)
        excused = np.array([cases.near_tie(a, mn, mx) for a in acf])
        print(name, fs, "excused", int(excused.sum()), "of", len(out))
        assert excused.sum() <= 0.01 * len(out), (name, int(excused.sum()), len(out))
        # the perturbation itself moves a value by the bar, the comparison allows the bar on top
        ok = np.abs(got - out) <= 2 * (cases.RTOL * np.abs(out) + cases.ATOL)
        assert np.all(ok | excused), (name, np.flatnonzero(~(ok | excused)))


def host(**kw):
    L = _lib.lib()
    cfg = _lib.VoicednessCfg()
    L.amx_voicedness_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    st = L.amx_voicedness_create(None, C.byref(cfg), C.byref(h))
    return L, h, st


def test_abi_surface_geometry_and_refusals():
    L = _lib.lib()
    for name in ("amx_voicedness_default_cfg", "amx_voicedness_create", "amx_voicedness_destroy", "amx_voicedness_describe",
                 "amx_voicedness_n_frames", "amx_voicedness_run", "amx_voicedness_run_batch_dev", "amx_voicedness_run_batch_dev_s16"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    cfg = _lib.VoicednessCfg()
    L.amx_voicedness_default_cfg(C.byref(cfg))
    assert (cfg.sample_rate, cfg.win_len_s, cfg.win_shift_s, cfg.corr_begin_s, cfg.corr_end_s) == (16000.0, 0.040, 0.010, 0.0, 0.040)
    assert (cfg.normalization, cfg.min_position_s, cfg.max_position_s) == (_lib.AMX_XCORR_UNBIASED_ESTIMATE, 0.0025, 0.0167)
    for fs in (16000.0, 8000.0):
        L, h, st = host(sample_rate=fs)
        assert st == 0, L.amx_last_error()
        info = _lib.VoicednessInfo()
        assert L.amx_voicedness_describe(h, C.byref(info)) == 0
        g = V.geometry(fs)
        assert {k: getattr(info, k) for k in g} == g
        for n in (0, 1, g["frame_len"] - 1, g["frame_len"], g["frame_len"] + 1, g["frame_len"] + g["frame_shift"], 12345, 160000):
            assert L.amx_voicedness_n_frames(h, n) == V.n_frames(n, g["frame_len"], g["frame_shift"])
        # a host-only handle has no device entry points
        assert L.amx_voicedness_run(h, None, 0, None) == _lib.AMX_ERR_STATE
        L.amx_voicedness_destroy(h)
    # the 40 ms window flushes later than the 25 ms one: the frame counts differ
    L, h, st = host()
    mcfg = _lib.MfccCfg()
    L.amx_mfcc_default_cfg(C.byref(mcfg))
    mh = C.c_void_p()
    assert L.amx_mfcc_create(None, C.byref(mcfg), C.byref(mh)) == 0
    assert L.amx_voicedness_n_frames(h, 16000) == 97 and L.amx_mfcc_n_frames(mh, 16000) == 99
    L.amx_mfcc_destroy(mh)
    L.amx_voicedness_destroy(h)
    # refusals: unsupported, naming the parameter
    for kw, word in ((dict(corr_begin_s=-0.01), b"begin"), (dict(corr_begin_s=0.005), b"begin"),
                     (dict(normalization=_lib.AMX_XCORR_UPPER_BOUND), b"upper-bound"),
                     (dict(sample_rate=44100.0), b"transform"), (dict(win_len_s=0.1, corr_end_s=0.1), b"transform")):
        L, h, st = host(**kw)
        assert st == _lib.AMX_ERR_UNSUPPORTED and word in L.amx_last_error(), (kw, st, L.amx_last_error())
    # invalid
    for kw, word in ((dict(sample_rate=0.0), b"not positive"), (dict(normalization=7), b"unknown normalization"),
                     (dict(min_position_s=0.02), b"min-position"), (dict(max_position_s=0.05), b"max-position"),
                     (dict(win_shift_s=0.0), b"positive"), (dict(tuning=b"fft=r16"), b"fft")):
        L, h, st = host(**kw)
        assert st == _lib.AMX_ERR_INVALID and word in L.amx_last_error(), (kw, st, L.amx_last_error())
    L, h, st = host(normalization=_lib.AMX_XCORR_NONE)
    assert st == 0
    L.amx_voicedness_destroy(h)


def test_three_front_ends_count_frames_alike():
    """one WindowBuffer rule behind amx_mfcc_n_frames, amx_gammatone_n_frames and amx_voicedness_n_frames: on host-only handles with
    400-sample windows every 160 samples they agree with each other and with the closed form (frames start every `shift` samples
    until the rest fits into one window)"""
    import rasr_amd
    L, vh, st = host(win_len_s=0.025)
    assert st == 0, L.amx_last_error()
    mcfg = _lib.MfccCfg()
    L.amx_mfcc_default_cfg(C.byref(mcfg))
    mh = C.c_void_p()
    assert L.amx_mfcc_create(None, C.byref(mcfg), C.byref(mh)) == 0
    gt = rasr_amd.GammatoneExtractor(None)
    vi, mi = _lib.VoicednessInfo(), _lib.MfccInfo()
    assert L.amx_voicedness_describe(vh, C.byref(vi)) == 0 and L.amx_mfcc_describe(mh, C.byref(mi)) == 0
    assert (vi.frame_len, vi.frame_shift) == (mi.frame_len, mi.frame_shift) == (gt.info.frame_len, gt.info.frame_shift) == (400, 160)
    for n in (0, 1, 2, 159, 160, 399, 400, 401, 560, 561, 800, 801, 48077):
        want = 0 if n == 0 else 1 if n <= 400 else -(-(n - 400) // 160) + 1
        assert L.amx_mfcc_n_frames(mh, n) == gt.n_frames(n) == L.amx_voicedness_n_frames(vh, n) == want, n
    L.amx_mfcc_destroy(mh)
    L.amx_voicedness_destroy(vh)
