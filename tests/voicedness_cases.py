"""Inputs and the excuse rule shared by tests/test_voicedness.py (CPU self-check of the rule) and tests/test_voicedness_gpu.py."""
import numpy as np

from tests import synth

RTOL, ATOL = 1e-4, 1e-4   # the front-end bar (tests/test_mfcc_gpu.py)


def acf_bar(ref):
    """|dev - ref| <= 1e-4 |ref| + 1e-4 s, s = the frame's R[0]"""
    ref = np.asarray(ref, np.float64)
    return RTOL * np.abs(ref) + ATOL * np.abs(ref[..., :1])


def voiced(n, fs, seed):
    """harmonics of a gliding 90..150 Hz fundamental plus a little noise, s16-valued"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / fs
    phase = np.cumsum(2 * np.pi * (120 + 30 * np.sin(2 * np.pi * 1.5 * t)) / fs)
    x = 4000 * sum(np.sin(k * phase) / k for k in range(1, 8)) + 200 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.float32)


def unvoiced(n, fs, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.clip(np.rint(3000 * rng.standard_normal(n)), -32768, 32767).astype(np.float32)


def pulses(n, fs, seed):
    """a glottal-pulse-like train on a gliding 90..150 Hz fundamental through a three-tap filter, plus noise: sharp autocorrelation
    peaks whose height falls with the lag (the glide decorrelates later periods), s16-valued"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / fs
    phase = np.cumsum((120 + 30 * np.sin(2 * np.pi * 1.5 * t)) / fs)
    x = np.zeros(n)
    x[1:][np.diff(np.floor(phase)) > 0] = 8000
    x = np.convolve(x, [1, -0.6, 0.3])[:n] + 300 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.float32)


def end_to_end_inputs(fs):
    """name -> samples.  Beside each seed: frames the excuse rule (near_tie) takes / frames, counted on the CPU;
    tests/test_voicedness.py::test_excuse_rule_stays_under_the_cap asserts the 1 % cap and that the restatement run on its own
    autocorrelation perturbed by +- the bar keeps every other frame's value.  Not here on purpose: config-1 audio (its 440 Hz tone has
    equally high peaks at every multiple of the period, 12 / 298 real ties) and smooth harmonic sums at 16 kHz (flat-topped peaks,
    21 / 198); both are in the autocorrelation half and the bit-exact peak half."""
    n = 2 * int(fs) + 77
    return {
        "pulses": pulses(n, fs, seed=21),       # 16 kHz: 0 / 198, 8 kHz: 0 / 198
        "unvoiced": unvoiced(n, fs, seed=12),   # 16 kHz: 0 / 198, 8 kHz: 1 / 198
    }


def near_tie(ref, min_position, max_position):
    """May this frame be excused from the end-to-end value comparison?  Only if the REFERENCE autocorrelation has a near-tie within
    twice the bar: two separate peaks whose values both come within it of the best, or a best peak whose rise / fall comparison
    (which decides whether and where it qualifies) is that close."""
    v = np.asarray(ref, np.float64)
    if not np.all(np.isfinite(v)):
        return False
    tol = 2 * acf_bar(v)
    lo, hi = max(1, min_position - 1), min(len(v) - 2, max_position + 1)
    loose = [q for q in range(lo, hi + 1) if v[q] >= v[q - 1] - tol[q] and v[q] >= v[q + 1] - tol[q]]
    if not loose:
        return False
    top = max(v[q] for q in loose)
    near = [q for q in loose if v[q] >= top - tol[q]]
    groups = 1 + sum(1 for a, b in zip(near, near[1:]) if b != a + 1)
    if groups > 1:
        return True
    return any(abs(v[q] - v[q - 1]) <= tol[q] or abs(v[q] - v[q + 1]) <= tol[q] for q in near)
