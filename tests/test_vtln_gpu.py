"""GPU: VTLN filter banks in the fused MFCC kernel (bank per tile): a segment's cepstra do not depend on the other segments of the
batch or on their factors, factor 1 is the unwarped kernel bit for bit, every route gives the same bits, and the warped cepstra
follow a numpy chain built from the library's own host tables of the factor."""
import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-4   # tests/test_mfcc_gpu.py
FACTORS = [0.88, 1.0, 1.12, 0.94, 1.06, 0.80, 1.20]
GRID = [round(0.88 + 0.02 * k, 2) for k in range(13)]   # a warping-factor estimation grid, 0.88 .. 1.12


def close(a, b):
    return np.all(np.abs(a - b) <= RTOL * np.abs(b) + ATOL)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ragged(seed=0):
    """empty, one-frame and long segments with mixed factors"""
    lens = [48077, 0, 400, 1, 16000, 5281, 0, 12345, 560, 3999]
    pcms = [synth.waveform(n, seed=seed + 10 * i) for i, n in enumerate(lens)]
    facs = [FACTORS[i % len(FACTORS)] for i in range(len(lens))]
    return pcms, facs


def extractor(ctx, factors, **kw):
    import rasr_amd
    if kw.get("front_end") == "plp":
        kw = dict(kw)
        kw.pop("front_end")
        return rasr_amd.MfccExtractor.plp(ctx, warping_factors=factors, **kw)
    return rasr_amd.MfccExtractor(ctx, warping_factors=factors, **kw)


FRONT_ENDS = {
    "mfcc40": dict(nr_cepstrum_coefficients=40, filter_width=138.0),
    "mfplp": dict(front_end="mfplp", normalize=True, nr_autocorrelation_coefficients=13, nr_cepstrum_coefficients=13),
    "plp": dict(front_end="plp"),
}


@pytest.mark.parametrize("fe_name", sorted(FRONT_ENDS))
def test_batch_equals_single_factor_handles_and_uniform_plans(ctx, fe_name):
    kw = FRONT_ENDS[fe_name]
    pcms, facs = ragged()
    fe = extractor(ctx, FACTORS, **kw)
    got = fe.run_batch(pcms, warping_factors=facs)
    for f in sorted(set(facs)):
        single = extractor(ctx, [f], **kw)
        uniform = fe.run_batch(pcms, warping_factors=[f] * len(pcms))
        for u, p in enumerate(pcms):
            if facs[u] != f:
                continue
            alone = single.run(p)
            assert got[u].shape == alone.shape == (single.n_frames(len(p)), fe.n_ceps)
            assert np.array_equal(bits(got[u]), bits(alone)), (u, f)
            assert np.array_equal(bits(got[u]), bits(uniform[u])), (u, f)
            assert np.array_equal(bits(alone), bits(single.run(p, warping_factor=f)))


@pytest.mark.parametrize("fe_name", sorted(FRONT_ENDS))
def test_factor_one_is_the_unwarped_kernel(ctx, fe_name):
    import rasr_amd
    kw = FRONT_ENDS[fe_name]
    pcms, _ = ragged(seed=5)
    plain = extractor(ctx, None, **kw) if kw.get("front_end") == "plp" else rasr_amd.MfccExtractor(ctx, **kw)
    want = plain.run_batch(pcms)
    fe = extractor(ctx, [0.9, 1.0, 1.1], **kw)
    got = fe.run_batch(pcms, warping_factors=[1.0] * len(pcms))
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))
    one = extractor(ctx, [1.0], **kw)   # the entry points without a factor use factors[0]
    for a, b in zip(one.run_batch(pcms), want):
        assert np.array_equal(bits(a), bits(b))


def numpy_chain(pcm, fe, tables, front_end="mfcc", alpha=1.0, normalize=False, plp_power=0.33):
    """the front end in f64 numpy from the library's host tables: preemphasis, Hamming window, zero-padded FFT, |X| / fs, then
    mfcc.flow: filter bank, log10, DCT-II; mfplp.flow / plp.flow: |X|^2, filter bank (plp: first and last filter twice, times the
    equal-loudness factors), ^plp_power, the N-plus-one cosine transform (/ (N - 1) when normalized), Levinson-Durbin and the LPC
    cepstrum.  Only the frames that lie inside the segment (the short last frame is left to the kernel tests)."""
    n, L, S, N = len(pcm), fe.frame_len, fe.frame_shift, fe.fft_len
    x = pcm.astype(np.float64)
    y = x - alpha * np.concatenate([[x[0]], x[:-1]])
    T = 0 if n < L else (n - L) // S + 1
    fs, fe_, fo, fw = tables["filter_start"], tables["filter_end"], tables["filter_offset"], tables["filter_weights"].astype(np.float64)
    win = tables["window"].astype(np.float64)
    dct = tables["dct"].astype(np.float64)
    eql = fe.equal_loudness() if front_end == "plp" else None
    out = np.zeros((T, fe.n_ceps))
    for t in range(T):
        amp = np.abs(np.fft.rfft(y[t * S:t * S + L] * win, N)) * (fe.info.fft_output_sample_rate / N)   # x 1/fs
        if front_end != "mfcc":
            amp = amp * amp
        e = np.array([np.dot(amp[fs[k]:fe_[k]], fw[fo[k]:fo[k] + fe_[k] - fs[k]]) for k in range(len(fs))])
        if front_end == "mfcc":
            out[t] = dct @ np.log10(e)
            continue
        if eql is not None:
            e = np.concatenate([[e[0]], e, [e[-1]]]) * eql
        R = dct @ (e ** plp_power)
        if normalize:
            R = R / (len(e) - 1)
        out[t] = lpc_cepstrum(R, fe.n_ceps)
    return out


def lpc_cepstrum(R, n_ceps):
    """Levinson-Durbin on the autocorrelation R[0..p], then the cepstrum of the all-pole model (gain^2 / |A|^2)"""
    p = len(R) - 1
    a, E = np.zeros(p + 1), R[0]
    a[0] = 1.0
    for i in range(1, p + 1):
        k = -(R[i] + np.dot(a[1:i], R[i - 1:0:-1])) / E
        a[1:i + 1] = a[1:i + 1] + k * np.concatenate([a[i - 1:0:-1], [1.0]])
        E = (1 - k * k) * E
    c = np.zeros(n_ceps)
    c[0] = np.log(E)   # 2 log(gain), gain = sqrt(E)
    for m in range(1, n_ceps):
        c[m] = -(m * a[m] + sum((m - k) * c[m - k] * a[k] for k in range(1, m))) / m
    return c


# extractor keywords, numpy-chain keywords, the oracle's configuration (oracle.MfccCfg constructor and arguments)
NUMPY_FRONT_ENDS = {
    "mfcc40": (FRONT_ENDS["mfcc40"], dict(front_end="mfcc"), ("default", dict(n_ceps=40, filter_width=138.0))),
    "mfplp": (FRONT_ENDS["mfplp"], dict(front_end="mfplp", normalize=True), ("mfplp", dict(n_ceps=13, n_autocorrelation=13))),
    "plp": (FRONT_ENDS["plp"], dict(front_end="plp", normalize=True, alpha=0.0), ("plp", dict())),
}


@pytest.mark.parametrize("fe_name", sorted(NUMPY_FRONT_ENDS))
def test_numeric_parity_with_a_numpy_chain_on_the_factors_tables(ctx, fe_name):
    from oracle import MfccCfg, OracleMfcc
    kw, nkw, (ocfg, okw) = NUMPY_FRONT_ENDS[fe_name]
    pcm = synth.waveform(48077, seed=21)
    # the numpy chain itself, on unwarped tables, against the oracle
    plain = extractor(ctx, None, **kw)
    ref = numpy_chain(pcm, plain, plain.tables(), **nkw)
    orc = OracleMfcc(getattr(MfccCfg, ocfg)(**okw)).run(pcm)[:len(ref)]
    assert close(ref, orc), np.abs(ref - orc).max()
    fe = extractor(ctx, FACTORS, **kw)
    got = fe.run_batch([pcm] * len(FACTORS), warping_factors=FACTORS)
    for f, g in zip(FACTORS, got):
        want = numpy_chain(pcm, fe, fe.tables(f), **nkw)
        assert close(g[:len(want)], want), (f, np.abs(g[:len(want)] - want).max())
        if f != 1.0:  # the warping moves the cepstra well beyond the bar
            assert not close(g[:len(want)], got[FACTORS.index(1.0)][:len(want)])


ROUTES = [dict(fft="stockham", prefetch=1), dict(fft="stockham", prefetch=0), dict(fft="mfma"), dict(fft="r16")]


@pytest.mark.parametrize("fe_name", sorted(FRONT_ENDS))
def test_every_route(ctx, fe_name):
    """on every route (fft=stockham with and without the sample prefetch, fft=mfma, fft=r16; f32 and s16 samples) a mixed-factor
    batch gives, segment for segment, the bits of one-factor handles of the same route; s16 and f32 samples of whole-numbered audio
    give the same bits; the prefetch leaves the bits alone and the matrix-core and radix-16 transforms stay within the MFCC bar of
    the butterflies, as tests/test_mfcc_gpu.py requires of the unwarped kernel"""
    kw = dict(FRONT_ENDS[fe_name])
    if fe_name == "mfcc40":
        kw["alpha"] = 0.97
    pcms, facs = ragged(seed=9)
    s16 = [np.clip(np.round(p), -32768, 32767).astype(np.int16) for p in pcms]
    f32 = [p.astype(np.float32) for p in s16]
    ref = None
    for tuning in ROUTES:
        fe = extractor(ctx, FACTORS, tuning=tuning, **kw)
        got = fe.run_batch(s16, warping_factors=facs)
        for u, (a, b) in enumerate(zip(got, fe.run_batch(f32, warping_factors=facs))):
            assert np.array_equal(bits(a), bits(b)), (tuning, u)
        for f in sorted(set(facs)):
            single = extractor(ctx, [f], tuning=tuning, **kw)
            for u in (u for u in range(len(pcms)) if facs[u] == f):
                assert np.array_equal(bits(got[u]), bits(single.run(s16[u]))), (tuning, u)
        if ref is None:
            ref = got
        for u, (a, b) in enumerate(zip(got, ref)):
            if tuning.get("fft") == "stockham":
                assert np.array_equal(bits(a), bits(b)), (tuning, u)
            else:
                ok = np.isfinite(b)
                assert np.array_equal(np.isfinite(a), ok) and close(a[ok], b[ok]), (tuning, u)


def test_plan_of_another_handle_is_refused(ctx):
    import torch

    import rasr_amd
    a = rasr_amd.MfccExtractor(ctx, warping_factors=[0.9, 1.0])
    b = rasr_amd.MfccExtractor(ctx, warping_factors=[0.9, 1.0])
    plan = a.plan([0, 1600], warping_factors=[0.9])
    pcm = torch.zeros(1600, dtype=torch.float32, device="cuda")
    out = torch.zeros((plan.total_frames, a.n_ceps), dtype=torch.float32, device="cuda")
    with pytest.raises(rasr_amd.AmxError, match="another front-end handle"):
        b.run_plan(plan, pcm, out)
    with pytest.raises(rasr_amd.AmxError, match="segment 0"):
        a.plan([0, 1600], warping_factors=[1.1])


def test_full_size_thirteen_factors(ctx):
    """config 2 (1000 utterances, seed 3) with 13 factors dealt round the utterances: frame counts, finiteness, and every 97th
    utterance against a one-factor handle, bit for bit, and against the numpy chain"""
    import torch

    import rasr_amd
    fe = rasr_amd.MfccExtractor(ctx, nr_cepstrum_coefficients=40, filter_width=138.0, warping_factors=GRID)
    lens = synth.utterance_lengths(1000, seed=3)
    off = np.concatenate([[0], np.cumsum(lens)])
    base = synth.waveform(int(lens.max()), seed=4)
    pcm = np.concatenate([np.roll(base, u)[:n] for u, n in enumerate(lens)])
    facs = [GRID[u % len(GRID)] for u in range(1000)]
    ceps, fo = fe.run_batch_dev(off, torch.from_numpy(pcm).cuda(), facs)
    assert ceps.shape[0] == sum(fe.n_frames(int(n)) for n in lens)
    got = ceps.cpu().numpy()
    assert np.isfinite(got).all()
    for u in range(0, 1000, 97):
        seg = got[fo[u]:fo[u + 1]]
        single = rasr_amd.MfccExtractor(ctx, nr_cepstrum_coefficients=40, filter_width=138.0, warping_factors=[facs[u]])
        assert np.array_equal(bits(seg), bits(single.run(pcm[off[u]:off[u + 1]]))), u
        want = numpy_chain(pcm[off[u]:off[u + 1]], fe, fe.tables(facs[u]))
        assert close(seg[:len(want)], want), (u, np.abs(seg[:len(want)] - want).max())
