"""GPU: the fused voicedness kernel (rasr_amd/csrc/voicedness.hip) in two halves and end to end.

  autocorrelation half   acf_dev against tests/voicedness_reference.py within the front-end bar |dev - ref| <= 1e-4 |ref| + 1e-4 R[0]
  peak half              the reference's scan, as a Python loop, over the device's OWN acf_dev: equal to out_dev bit for bit
  end to end             against the restatement; a frame is excused only for a near-tie in the REFERENCE autocorrelation
                         (tests/voicedness_cases.py), at most 1 % of the frames of an input
"""
import numpy as np
import pytest

from tests import synth
from tests import voicedness_cases as cases
from tests import voicedness_reference as V

pytestmark = pytest.mark.gpu

RATES = [16000.0, 8000.0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def extractor(ctx, fs, **kw):
    import rasr_amd
    return rasr_amd.VoicednessExtractor(ctx, sample_rate=fs, **kw)


def run_dev(fe, segs, s16=False, acf=True, out_ld=1, column=0):
    """the batch entry point on a list of segments: measures [T], autocorrelation [T x n_lags] (or None), the whole output matrix"""
    import torch
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    pcm = np.concatenate(segs) if len(segs) else np.zeros(0, np.float32)
    T = sum(fe.n_frames(len(s)) for s in segs)
    d = torch.from_numpy(pcm.astype(np.int16) if s16 else pcm.astype(np.float32)).cuda()
    out = torch.full((max(T, 1), out_ld), -7.0, dtype=torch.float32, device="cuda")
    a = torch.full((max(T, 1), fe.n_lags), -7.0, dtype=torch.float32, device="cuda") if acf else None
    fe.run_batch_dev(off, d, out[:, column], out_ld=out_ld, acf_dev=a)
    torch.cuda.synchronize()
    o = out.cpu().numpy()[:T]
    return o[:, column].copy(), (a.cpu().numpy()[:T] if acf else None), o


def reference(segs, fs, **kw):
    outs, acfs = zip(*[V.voicedness(s, fs, return_acf=True, **kw) for s in segs])
    return np.concatenate(outs), np.concatenate(acfs)


def segments(fs, seed=0):
    """config-1 audio, synthetic voiced / unvoiced / silent / constant segments, segments shorter than one window, and lengths that
    leave every residue class of short last frames the shift allows (one per multiple of shift / 8)"""
    g = V.geometry(fs)
    L, S = g["frame_len"], g["frame_shift"]
    n = int(fs)
    segs = [synth.waveform(n + 37, seed=1, fs=fs), cases.voiced(n // 2 + 5, fs, seed + 3), cases.unvoiced(n // 3, fs, seed + 4),
            np.zeros(L + 3 * S, np.float32), np.full(L + S + 1, 250, np.float32), cases.unvoiced(1, fs, 5), cases.unvoiced(L // 3, fs, 6),
            cases.unvoiced(L - 1, fs, 7), cases.voiced(L, fs, 8), cases.voiced(L + 1, fs, 9)]
    segs += [cases.voiced(L + 2 * S + r, fs, 20 + r) for r in range(0, S, max(1, S // 8))]
    return segs


def short_tails(fs):
    """every possible short last frame: segment lengths L + S + r, r = 1 .. S (the last frame holds L - S + r .. L samples), and the
    flush of a segment shorter than the window"""
    g = V.geometry(fs)
    L, S = g["frame_len"], g["frame_shift"]
    base = cases.voiced(L + 2 * S, fs, 31)
    return [base[:L + S + r] for r in range(1, S + 1)] + [base[:r] for r in (1, 2, 3, S, L - 1)]


@pytest.mark.parametrize("fs", RATES)
def test_autocorrelation_half(ctx, fs):
    fe = extractor(ctx, fs)
    worst = (0.0, None)
    for label, segs in (("mixed", segments(fs)), ("tails", short_tails(fs))):
        out, acf, _ = run_dev(fe, segs)
        ref_out, ref_acf = reference(segs, fs)
        assert acf.shape == ref_acf.shape
        assert np.array_equal(np.isnan(acf), np.isnan(ref_acf)), label   # digital silence: 0 * (1 / 0), NaN in the same places
        assert np.isnan(ref_acf).any() or label != "mixed"
        fin = ~np.isnan(ref_acf)
        ratio = np.where(fin, np.abs(np.where(fin, acf, 0) - np.where(fin, ref_acf, 0)) / np.maximum(cases.acf_bar(np.where(fin, ref_acf, 1)), 1e-300), 0)
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        print("fs %g %s: %d frames, worst |dev - ref| / bar = %.3f at frame %d lag %d" % (fs, label, len(acf), ratio[i], i[0], i[1]))
        if ratio[i] > worst[0]:
            worst = (float(ratio[i]), (label,) + tuple(int(k) for k in i))
        assert ratio[i] <= 1.0, (label, worst)


@pytest.mark.parametrize("fs", RATES)
def test_autocorrelation_without_normalization(ctx, fs):
    fe = extractor(ctx, fs, normalization="none")
    segs = [cases.voiced(int(fs) // 4 + 11, fs, 41), cases.unvoiced(int(fs) // 5, fs, 42)]
    out, acf, _ = run_dev(fe, segs)
    ref_out, ref_acf = reference(segs, fs, normalization="none")
    assert np.all(np.abs(acf - ref_acf) <= cases.acf_bar(ref_acf))


@pytest.mark.parametrize("fs", RATES)
def test_peak_half_is_bit_exact_on_the_devices_own_autocorrelation(ctx, fs):
    fe = extractor(ctx, fs)
    g = V.geometry(fs)
    plateaus = [np.zeros(3 * g["frame_len"], np.float32), np.full(2 * g["frame_len"] + 7, -1234, np.float32),
                np.tile(np.array([500, 500, -500, -500], np.float32), g["frame_len"])]   # silence, constants, a square wave
    n = 0
    for segs in (segments(fs), short_tails(fs), plateaus):
        out, acf, _ = run_dev(fe, segs)
        want = np.array([V.maximal_peak_value(a.tolist(), g["min_position"], g["max_position"]) for a in acf], np.float32)
        assert np.array_equal(bits(out), bits(want)), np.flatnonzero(bits(out) != bits(want))
        n += len(out)
    assert n > 300
    # other position ranges, the peak straddling them included
    for mn, mx in ((0.0005, 0.002), (0.006, 0.0061), (0.0025, 0.039)):
        fe2 = extractor(ctx, fs, min_position_s=mn, max_position_s=mx)
        g2 = V.geometry(fs, min_position_s=mn, max_position_s=mx)
        out, acf, _ = run_dev(fe2, segments(fs)[:3])
        want = np.array([V.maximal_peak_value(a.tolist(), g2["min_position"], g2["max_position"]) for a in acf], np.float32)
        assert np.array_equal(bits(out), bits(want)), (mn, mx)


@pytest.mark.parametrize("fs", RATES)
def test_end_to_end_against_the_restatement(ctx, fs):
    fe = extractor(ctx, fs)
    g = V.geometry(fs)
    for name, x in cases.end_to_end_inputs(fs).items():
        out, _, _ = run_dev(fe, [x], acf=False)
        ref_out, ref_acf = reference([x], fs)
        excused = np.array([cases.near_tie(a, g["min_position"], g["max_position"]) for a in ref_acf])
        diff = np.abs(out - ref_out)
        ok = diff <= cases.RTOL * np.abs(ref_out) + cases.ATOL
        print("fs %g %s: %d frames, %d excused, %d of the others over the bar, max diff %.3g" % (fs, name, len(out), excused.sum(),
                                                                                                 (~ok & ~excused).sum(), diff.max()))
        assert excused.sum() <= 0.01 * len(out), (name, int(excused.sum()), len(out))
        assert np.all(ok | excused), (name, np.flatnonzero(~ok & ~excused))


@pytest.mark.parametrize("fs", RATES)
def test_entry_points_agree(ctx, fs):
    fe = extractor(ctx, fs)
    segs = segments(fs)
    out, acf, _ = run_dev(fe, segs)
    # s16 samples: the same bits
    out16, acf16, _ = run_dev(fe, segs, s16=True)
    assert np.array_equal(bits(out), bits(out16)) and np.array_equal(bits(acf), bits(acf16))
    # acf_dev = NULL: the same measures
    plain, none, _ = run_dev(fe, segs, acf=False)
    assert none is None and np.array_equal(bits(out), bits(plain))
    # out_ld > 1 writes its column only
    col, _, wide = run_dev(fe, segs, acf=False, out_ld=5, column=3)
    assert np.array_equal(bits(col), bits(out))
    assert np.all(np.delete(wide, 3, axis=1) == -7.0)
    # the host entry point, segment by segment
    host = np.concatenate([fe.run(s) for s in segs])
    assert np.array_equal(bits(host), bits(out))
    # a segment's measures do not depend on the batch around it
    alone, _, _ = run_dev(fe, segs[1:2], acf=False)
    t0 = fe.n_frames(len(segs[0]))
    assert np.array_equal(bits(alone), bits(out[t0:t0 + len(alone)]))
    # empty batch, empty segments
    e, _, _ = run_dev(fe, [], acf=False)
    assert len(e) == 0
    z, _, _ = run_dev(fe, [np.zeros(0, np.float32), segs[1], np.zeros(0, np.float32)], acf=False)
    assert np.array_equal(bits(z), bits(alone))


def energy(fe, segs):
    import torch
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    T = sum(fe.n_frames(len(s)) for s in segs)
    d = torch.from_numpy(np.concatenate(segs).astype(np.float32)).cuda()
    total, ordered = torch.full((T,), -1.0, dtype=torch.float64, device="cuda"), torch.full((T,), -1, dtype=torch.int32, device="cuda")
    fe.energy_dev(off, d, total, ordered)
    torch.cuda.synchronize()
    return total.cpu().numpy(), ordered.cpu().numpy()


@pytest.mark.parametrize("fs", RATES)
def test_energy_sum_has_the_bits_of_the_index_order_sum_on_both_of_its_paths(ctx, fs):
    """the kernel adds a frame's squares in lane order when it can prove the double sum exact in any order, else one lane adds them
    in index order; either way the sum is std::inner_product's, bit for bit, and the test sees which way was taken"""
    g = V.geometry(fs)
    fe = extractor(ctx, fs)
    rng = np.random.Generator(np.random.PCG64(17))
    n = int(fs) // 3
    wide = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)      # squares span far more than 53 bits
    unit = (cases.unvoiced(n, fs, 18) / np.float32(32768)).astype(np.float32)                 # 16-bit audio scaled to [-1, 1)
    tiny = (cases.unvoiced(n, fs, 19) * np.float32(1e-22)).astype(np.float32)                 # squares are denormal
    odd = wide.copy()
    odd[n // 2] = np.inf
    huge = (cases.unvoiced(n, fs, 20) * np.float32(1e17)).astype(np.float32)                  # squares overflow to inf
    paths = {}
    for name, x in (("s16", cases.voiced(n, fs, 21)), ("unit", unit), ("wide", wide), ("tiny", tiny), ("inf", odd), ("huge", huge),
                    ("silence", np.zeros(n, np.float32))):
        got, ordered = energy(fe, [x])
        want = V.energy_sum(V.frames(x, g["frame_len"], g["frame_shift"]))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, np.flatnonzero(got.view(np.uint64) != want.view(np.uint64)))
        assert set(ordered.tolist()) <= {0, 1}
        paths[name] = ordered
    assert not paths["s16"].any() and not paths["unit"].any() and not paths["silence"].any()   # always provably exact
    assert paths["wide"].mean() > 0.9 and paths["huge"].all()                                 # the ordered path is taken and tested
    # and through the whole kernel: R[0] of such frames within the bar
    out, acf, _ = run_dev(fe, [wide])
    ref_out, ref_acf = reference([wide], fs)
    assert np.all(np.abs(acf - ref_acf) <= cases.acf_bar(ref_acf))


@pytest.mark.parametrize("fs", RATES)
def test_device_against_the_references_own_text_in_both_builds(ctx, fs):
    """tests/golden/ref_voicedness.npz: every recorded frame as a one-frame segment; the device autocorrelation within the bar of
    the reference's in either build, NaN frames in the same places"""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_voicedness.npz"))
    tag = "%d" % fs
    frames = g[tag + "/frames"].astype(np.float32)
    out, acf, _ = run_dev(extractor(ctx, fs), list(frames))
    for build in ("off", "fma"):
        want = g["%s/%s/acf" % (tag, build)]
        assert np.array_equal(np.isnan(acf), np.isnan(want))
        fin = ~np.isnan(want)
        ratio = np.abs(acf[fin] - want[fin]) / cases.acf_bar(np.where(fin, want, 1))[fin]
        print("fs %g contract=%s: worst |dev - ref| / bar = %.3f" % (fs, build, ratio.max()))
        assert ratio.max() <= 1.0, build


def test_reused_handle_gives_the_bits_of_a_fresh_one(ctx):
    fs = 16000.0
    probe = segments(fs)[:4]
    fresh, fresh_acf, _ = run_dev(extractor(ctx, fs), probe)
    fe = extractor(ctx, fs)
    run_dev(fe, short_tails(fs))                       # many short segments: larger offset tables
    run_dev(fe, [cases.unvoiced(50000, fs, 3)], s16=True, acf=False)
    fe.run(cases.voiced(30000, fs, 4))                 # the host path's staging buffers
    again, again_acf, _ = run_dev(fe, probe)
    assert np.array_equal(bits(fresh), bits(again)) and np.array_equal(bits(fresh_acf), bits(again_acf))
