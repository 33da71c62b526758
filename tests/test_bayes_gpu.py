"""GPU parity: amx_bayes_classify_dev, amx_bayes_scores_dev and amx_bayes_classify_gmm_dev (bayes_sum_kernel, bayes_window_kernel,
bayes_argmin_kernel) through the Python class against the restatement of tests/bayes_reference.py, which tests/test_bayes.py holds against
the reference's own results.  Every comparison is equality of bits: labels, per-class scores, per-frame labels, emitted masks, sums of
weights.  The order of every f32 sum is fixed and nothing on the device is transcendental, so no tolerance exists.

Shapes.  bayes_sum_kernel gives a segment a group of lanes as wide as the next power of two of n_classes (a multiple of 256 above
256): 1, 2, 13, 63, 64, 65 and 200 classes are groups smaller than, equal to and larger than a wave.  It reads eight frames ahead of the
chain: segments of 0, 1, 2, 15, 16, 17 and 300 frames in one call (an empty one first, in the middle and last) are below, at and above
that block and diverge within a wave.  The score matrix is wider than n_classes, its other columns hold NaN.

Before a test touches the device it asserts on the CPU that it can fail: `order_matters`, `prior_ties`, the no-winner inputs.
"""
import numpy as np
import pytest

from tests import bayes_reference as br
from tests.test_bayes import bits, same

pytestmark = pytest.mark.gpu

CLASSES = (1, 2, 13, 63, 64, 65, 200)
LENGTHS = (0, 1, 2, 15, 0, 16, 17, 300, 0)
T_MAX = 300
PAD = 3                        # scores_ld = n_classes + 3
SENTINEL_I, SENTINEL_F = -77, np.float32(-12345.5)
INT_MAX = br.INT_MAX


def offsets(lengths=LENGTHS, first=0):
    return np.concatenate([[first], first + np.cumsum(lengths)]).astype(np.int64)


def mixed_scores(n_classes, lengths=LENGTHS, seed=0):
    """N(50, 30) with a few values near 1e4 (sums whose bits depend on the order), weights in [0, 2] with one exact 0 per segment"""
    rng = np.random.Generator(np.random.PCG64(977 * n_classes + seed))
    T = int(np.sum(lengths))
    s = rng.normal(50.0, 30.0, (T, n_classes)).astype(np.float32)
    hit = rng.random((T, n_classes)) < 0.03
    s[hit] = (1e4 + rng.normal(0.0, 50.0, (T, n_classes))).astype(np.float32)[hit]
    w = (rng.random(T) * 2.0).astype(np.float32)
    off = offsets(lengths)
    for a, e in zip(off[:-1], off[1:]):
        if e - a > 1:
            w[a + (e - a) // 2] = 0.0
    return s, w


def order_scores(n_classes, lengths=LENGTHS, seed=0):
    """windowed inputs whose labels depend on the order of the window's sum: class 1 repeats class 0 with neighbouring frames swapped (the
    same values in another order inside most windows), every other class is far above"""
    s, w = mixed_scores(n_classes, lengths, seed)
    if n_classes >= 2:
        s[:, 1] = s[:, 0]
        off = offsets(lengths)
        for a, e in zip(off[:-1], off[1:]):
            for t in range(a, e - 1, 2):
                s[t, 1], s[t + 1, 1] = s[t + 1, 0], s[t, 0]
        s[:, 2:] += np.float32(3e4)
    return s, w


def order_matters(n_classes, L):
    """condition 1 of the tests: newest-to-oldest against oldest-to-newest differs in a score bit AND a label (windowed inputs), and the
    sequential sum differs from a pairwise one in a bit (cumulative inputs)"""
    s, _ = order_scores(n_classes)
    off = offsets()
    a, e = int(off[7]), int(off[8])   # the 300-frame segment
    new = br.classify_segment(s[a:e], window_length=L)
    old = br.classify_segment(s[a:e], window_length=L, oldest_first=True)
    score_bit = not np.array_equal(bits(new["frame_scores"][L - 1:]), bits(old["frame_scores"][L - 1:]))
    label = bool(np.any(new["frame_label"] != old["frame_label"]))
    m, _ = mixed_scores(n_classes)
    seq = br.classify_segment(m[a:e])["eos_scores"]
    tree = np.array([np.float32(br.prior(n_classes) + br.pairwise_sum(m[a:e, c])) for c in range(n_classes)], np.float32)
    return score_bit, label, not np.array_equal(bits(seq), bits(tree))


def prior_ties(n_classes):
    """condition 2: one-frame scores for classes 0 and 1 whose sums differ (class 1 is SMALLER) while logN + sum is the same f32; the
    label must be 0.  Found by walking the floats below a power of two, where adding logN crosses into the coarser binade."""
    log_n = br.prior(n_classes)
    for top in (1024.0, 2048.0, 4096.0, 512.0):
        lo = np.float32(top - 0.5)
        for k in range(64):
            s1 = lo
            for _ in range(k):
                s1 = np.nextafter(s1, np.float32(np.inf), dtype=np.float32)
            s0 = np.nextafter(s1, np.float32(np.inf), dtype=np.float32)
            if np.float32(log_n + s0) == np.float32(log_n + s1) and s0 != s1 and np.float32(log_n + s0) >= np.float32(top):
                return s0, s1
    return None


class Device:
    """one call's buffers on the device, every output filled with a sentinel beforehand"""

    def __init__(self, scores, off, weights=None, first_row=0):
        import torch
        T, n = scores.shape
        self.n, self.T, self.n_seg, self.first = n, T, len(off) - 1, first_row
        wide = np.full((first_row + T, n + PAD), np.nan, np.float32)
        wide[first_row:, :n] = scores
        self.scores = torch.from_numpy(wide).cuda()
        self.ld = n + PAD
        self.weights = None
        if weights is not None:
            wv = np.full(first_row + T, np.nan, np.float32)
            wv[first_row:] = weights
            self.weights = torch.from_numpy(wv).cuda()
        self.seg_label = torch.full((self.n_seg,), SENTINEL_I, dtype=torch.int32, device="cuda")
        self.seg_score = torch.full((self.n_seg, n), float(SENTINEL_F), dtype=torch.float32, device="cuda")
        self.frame_label = torch.full((first_row + T,), SENTINEL_I, dtype=torch.int32, device="cuda")
        self.sum_w = torch.full((self.n_seg,), float(SENTINEL_F), dtype=torch.float32, device="cuda")
        self.out = torch.full((first_row + T, n + 1), float(SENTINEL_F), dtype=torch.float32, device="cuda")
        self.emitted = torch.full((first_row + T,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def outputs_untouched(self):
        import torch
        torch.cuda.synchronize()
        return (bool((self.seg_label == SENTINEL_I).all()) and bool((self.seg_score == float(SENTINEL_F)).all()) and
                bool((self.frame_label == SENTINEL_I).all()) and bool((self.sum_w == float(SENTINEL_F)).all()))


def classify_and_compare(ctx, scores, lengths, weights=None, first_row=0, handle=None, what=None, **cfg):
    """one amx_bayes_classify_dev call against the restatement; returns the restatement's result"""
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    off = offsets(lengths)
    want = br.classify_batch(scores, off, weights, **cfg)
    d = Device(scores, off, weights, first_row)
    b = handle or rasr_amd.BayesClassifier(ctx, scores.shape[1], **cfg)
    got_nw = b.classify(off + first_row, d.scores, d.ld, d.seg_label, weights_dev=d.weights, segment_score_dev=d.seg_score,
                        frame_label_dev=d.frame_label, sum_of_weights_dev=d.sum_w)
    torch.cuda.synchronize()
    assert np.array_equal(d.seg_label.cpu().numpy(), want["segment_label"]), what
    ss = d.seg_score.cpu().numpy()
    assert same(ss[want["written"]], want["segment_score"][want["written"]]), what
    assert np.all(ss[~want["written"]] == SENTINEL_F), what            # segments without a label keep what the buffer held
    assert same(d.sum_w.cpu().numpy(), want["sum_of_weights"]), what
    fl = d.frame_label.cpu().numpy()
    assert np.all(fl[:first_row] == SENTINEL_I), what
    if br.is_continuous(cfg):
        assert np.array_equal(fl[first_row:], want["frame_label"]), what
    else:
        assert np.all(fl == SENTINEL_I), what                          # ignored in segment mode
    assert got_nw == want["no_winner"], what
    if handle is None:
        b.close()
    return want


def weight_variants(w):
    return (("none", None), ("random", w))


# ------------------------------------------------------------------ modes, on every class-group width

@pytest.mark.parametrize("n", CLASSES)
def test_segment_mode_and_first_n_frames(ctx, n):
    s, w = mixed_scores(n)
    assert order_matters(n, 4)[2] or n == 1 and order_matters(13, 4)[2]     # a tree-shaped sum would give other bits
    none = classify_and_compare(ctx, s, LENGTHS, None, what=(n, "segment"))
    assert list(none["written"]) == [T > 0 for T in LENGTHS]
    ones = classify_and_compare(ctx, s, LENGTHS, np.ones(len(s), np.float32), what=(n, "ones"))
    assert same(ones["segment_score"], none["segment_score"])                # all weights 1: the bits of no weights
    classify_and_compare(ctx, s, LENGTHS, w, first_row=5, what=(n, "weighted"))
    for N in (1, 16, 17, T_MAX, T_MAX + 5):
        for wk, wv in weight_variants(w):
            r = classify_and_compare(ctx, s, LENGTHS, wv, number_of_features=N, what=(n, "first", N, wk))
            if wv is None:
                assert r["sum_of_weights"].tolist() == [float(min(T, N)) for T in LENGTHS]


@pytest.mark.parametrize("n", CLASSES)
def test_continuous_mode(ctx, n):
    s, w = mixed_scores(n, seed=1)
    for d in (0, 1, 16, T_MAX - 1, T_MAX + 5):
        for wk, wv in weight_variants(w):
            r = classify_and_compare(ctx, s, LENGTHS, wv, delay=d, what=(n, "continuous", d, wk))
            # a label at the end of the stream only where no frame reached the delay
            assert list(r["written"]) == [0 < T <= d for T in LENGTHS], d
            assert int((r["frame_label"] >= 0).sum()) == sum(max(0, T - d) for T in LENGTHS)


@pytest.mark.parametrize("n", CLASSES)
def test_windowed_mode(ctx, n):
    s, w = order_scores(n, seed=2)
    if n >= 2:
        score_bit, label, _ = order_matters(n, 4)
        assert score_bit and label                                           # oldest-to-newest would give other scores and other labels
    for L, d in ((1, INT_MAX), (4, INT_MAX), (25, INT_MAX), (4, 0), (4, 3), (25, 7)):
        for wk, wv in weight_variants(w):
            r = classify_and_compare(ctx, s, LENGTHS, wv, first_row=2 if L == 4 else 0, window_length=L, window_right=L - 1, delay=d,
                                     what=(n, "window", L, d, wk))
            short = [0 < T < L for T in LENGTHS]
            assert all(wr for wr, sh in zip(r["written"], short) if sh)      # a window that never filled: the label at the end of the stream
            if (L, d) == (4, 3):                                             # labels after frames 3, 6, 9, ...: 16 ends on one; 15, 17 and 300 do not
                assert list(r["written"]) == [False, True, True, True, False, False, True, True, False]
            if d == INT_MAX or d == 0:
                assert not any(wr for wr, T in zip(r["written"], LENGTHS) if T >= L)


def test_window_longer_than_the_staging_buffer(ctx):
    """a window whose products do not fit the workgroup's LDS takes the kernel's other path (memory); same bits"""
    s, w = order_scores(200, seed=3)
    classify_and_compare(ctx, s, LENGTHS, w, window_length=40, window_right=0, what="unstaged 200 x 40")
    s, w = order_scores(13, (700, 0, 30), seed=3)
    classify_and_compare(ctx, s, (700, 0, 30), w, window_length=600, window_right=3, delay=50, what="unstaged 13 x 600")


@pytest.mark.parametrize("n", CLASSES)
def test_score_node(ctx, n):
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    s, w = mixed_scores(n, seed=4)
    off = offsets()
    for single in (0, 1):
        for d in (0, 3):
            for wk, wv in weight_variants(w):
                want, em = br.scores_batch(s, off, wv, delay=d, single_frame=bool(single))
                dev = Device(s, off, wv, first_row=1)
                b = rasr_amd.BayesClassifier(ctx, n, delay=d, single_frame=single)
                b.scores(off + 1, dev.scores, dev.ld, dev.out, n + 1, dev.emitted, weights_dev=dev.weights)
                torch.cuda.synchronize()
                got, gem = dev.out.cpu().numpy(), dev.emitted.cpu().numpy()
                what = (n, single, d, wk)
                assert gem[0] == 9 and np.array_equal(gem[1:], em), what
                assert same(got[1:, :n][em > 0], want[em > 0]), what
                assert np.all(got[1:, :n][em == 0] == SENTINEL_F) and np.all(got[:, n] == SENTINEL_F) and np.all(got[0] == SENTINEL_F), what
                if d == 3:
                    assert 2 in em and 0 in em                               # a vector at the end of a stream, rows that emit nothing
                b.close()


# ------------------------------------------------------------------ ties, no winner, refused weights

@pytest.mark.parametrize("n", (2, 13, 65))
def test_the_prior_creates_ties_and_the_lower_index_wins(ctx, n):
    tie = prior_ties(n)
    assert tie is not None
    s0, s1 = tie
    assert s1 < s0 and np.float32(br.prior(n) + s0) == np.float32(br.prior(n) + s1)
    s = np.full((3, n), 9e3, np.float32)
    s[:, 0], s[:, 1] = s0, s1                                                # three one-frame segments
    for cfg in (dict(), dict(delay=0), dict(window_length=1)):
        r = classify_and_compare(ctx, s, (1, 1, 1), None, what=(n, cfg), **cfg)
        labels = r["frame_label"] if cfg else r["segment_label"]
        assert labels.tolist() == [0, 0, 0]                                  # without the prior class 1 would win


@pytest.mark.parametrize("cfg", (dict(), dict(delay=0), dict(window_length=2)), ids=("segment", "continuous", "window"))
def test_no_winner_is_minus_one_and_counted(ctx, cfg):
    n = 13
    lengths = (4, 4, 4, 4)
    s, _ = mixed_scores(n, lengths, seed=5)
    s[0:4] = np.nan                                                          # every class NaN
    s[4:8] = np.inf                                                          # every class +inf
    s[8:12] = np.nan
    s[8:12, 7] = 40.0                                                        # one finite class among NaNs
    r = classify_and_compare(ctx, s, lengths, None, what=cfg, **cfg)
    if not cfg:
        assert r["segment_label"].tolist()[:3] == [-1, -1, 7] and r["no_winner"] == (2, 0) and r["written"].all()
    elif "delay" in cfg:
        assert r["frame_label"][:12].tolist() == [-1] * 8 + [7] * 4 and r["no_winner"] == (0, 8)
    else:
        assert r["frame_label"][:12].tolist() == [-1] * 8 + [-1, 7, 7, 7] and r["no_winner"] == (0, 6)


def test_a_refused_weight_names_its_frame_and_writes_nothing(ctx):
    import rasr_amd
    ctx.use_torch_stream()
    n, k = 13, 21
    s, w = mixed_scores(n, seed=6)
    off = offsets()
    for cfg in (dict(), dict(delay=3), dict(window_length=4)):
        b = rasr_amd.BayesClassifier(ctx, n, **cfg)
        for bad_value in (-0.5, np.nan):
            bad = w.copy()
            bad[k], bad[k + 40] = bad_value, -1.0
            assert br.check_weights(bad) == k
            d = Device(s, off, bad)
            with pytest.raises(rasr_amd.AmxError, match="frame %d " % k) as e:
                b.classify(off, d.scores, d.ld, d.seg_label, weights_dev=d.weights, segment_score_dev=d.seg_score, frame_label_dev=d.frame_label,
                           sum_of_weights_dev=d.sum_w)
            assert e.value.status == -1 and d.outputs_untouched()
        classify_and_compare(ctx, s, LENGTHS, w, handle=b, what=("after the refusal", cfg), **cfg)    # the handle is as good as new
        b.close()
    # first-N mode reads no weight past frame N - 1 (the reference drains those frames without their weights)
    bad = w.copy()
    bad[int(off[7]) + 100] = -1.0
    classify_and_compare(ctx, s, LENGTHS, bad, number_of_features=16, what="first 16 with a bad weight behind")
    b = rasr_amd.BayesClassifier(ctx, n, delay=0)
    d = Device(s, off, bad)
    with pytest.raises(rasr_amd.AmxError, match="frame %d " % (int(off[7]) + 100)):
        b.scores(off, d.scores, d.ld, d.out, n + 1, d.emitted, weights_dev=d.weights)
    b.close()


def test_one_handle_over_calls_of_different_shapes(ctx):
    """scratch that grows and is reused: a large batch, a small one and the large one again give the bits of fresh handles"""
    import rasr_amd
    n = 13
    small, big = (3, 0, 9), LENGTHS
    for cfg in (dict(), dict(delay=1), dict(window_length=4, delay=3)):
        b = rasr_amd.BayesClassifier(ctx, n, **cfg)
        for lengths, seed in ((small, 7), (big, 8), (small, 9), (big, 8)):
            s, w = mixed_scores(n, lengths, seed)
            classify_and_compare(ctx, s, lengths, w, handle=b, what=(cfg, lengths), **cfg)     # the expectation never sees the handle
        b.close()


# ------------------------------------------------------------------ with the GMM scorer in front, and the fast-VTLN loop

def diagonal_model(n_mix, dim, seed):
    from tests import synth
    return synth.gmm_cart(n_mix, 1, 1, dim, seed=seed, pooled=False)


def test_classify_gmm_is_score_then_classify(ctx):
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    dim, n = 16, 13
    lengths = (0, 17, 40, 0, 5)
    off = offsets(lengths)
    T = int(off[-1])
    rng = np.random.Generator(np.random.PCG64(31))
    feats = torch.from_numpy(rng.standard_normal((T, dim)).astype(np.float32)).cuda()
    gmm = rasr_amd.GmmFeatureScorer(ctx, diagonal_model(n, dim, 3), "diagonal-maximum")
    sc = torch.zeros((T, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gmm.score_dev(feats, T, sc)
    torch.cuda.synchronize()
    for cfg in (dict(), dict(delay=2), dict(window_length=4)):
        b = rasr_amd.BayesClassifier(ctx, n, **cfg)
        outs = []
        for composed in (False, True):
            lab = torch.full((len(lengths),), SENTINEL_I, dtype=torch.int32, device="cuda")
            ssc = torch.full((len(lengths), n), float(SENTINEL_F), dtype=torch.float32, device="cuda")
            fl = torch.full((T,), SENTINEL_I, dtype=torch.int32, device="cuda")
            sw = torch.zeros(len(lengths), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if composed:
                nw = b.classify_gmm(gmm, off, feats, lab, segment_score_dev=ssc, frame_label_dev=fl, sum_of_weights_dev=sw)
            else:
                nw = b.classify(off, sc, n, lab, segment_score_dev=ssc, frame_label_dev=fl, sum_of_weights_dev=sw)
            torch.cuda.synchronize()
            outs.append((lab.cpu().numpy(), ssc.cpu().numpy(), fl.cpu().numpy(), sw.cpu().numpy(), nw))
        for x, y in zip(outs[0][:4], outs[1][:4]):
            assert same(x, y), cfg
        assert outs[0][4] == outs[1][4] == (0, 0)
        want = br.classify_batch(sc.cpu().numpy(), off, None, **cfg)            # and both are what the restatement makes of the matrix
        assert np.array_equal(outs[1][0], want["segment_label"]) and same(outs[1][1][want["written"]], want["segment_score"][want["written"]])
        b.close()
    b = rasr_amd.BayesClassifier(ctx, n)
    twelve = rasr_amd.GmmFeatureScorer(ctx, diagonal_model(12, dim, 4), "diagonal-maximum")
    lab = torch.full((len(lengths),), SENTINEL_I, dtype=torch.int32, device="cuda")
    with pytest.raises(rasr_amd.AmxError, match=r"Number of mixtures \(12\) does not match to the number of classes \(13\)") as e:
        b.classify_gmm(twelve, off, feats, lab)
    torch.cuda.synchronize()
    assert e.value.status == -1 and bool((lab == SENTINEL_I).all())
    b.close()


def test_fast_vtln_end_to_end(ctx):
    """unwarped MFCCs -> a 3-mixture GMM -> segment labels -> warping factors -> amx_mfcc_plan_create_vtln accepts them and the plan's
    output is that of a plan built from the same factors given by hand"""
    import rasr_amd
    import torch
    from tests import synth
    ctx.use_torch_stream()
    factors = [0.9, 1.0, 1.1]
    n_samples = 4800                                                             # 0.3 s
    pcm = np.concatenate([synth.waveform(n_samples, seed=40 + u) for u in range(4)]).astype(np.float32)
    sample_off = np.arange(5, dtype=np.int64) * n_samples
    fe = rasr_amd.MfccExtractor(ctx, warping_factors=factors)
    pcm_dev = torch.from_numpy(pcm).cuda()
    ceps, frame_off = fe.run_batch_dev(sample_off, pcm_dev, warping_factors=[1.0] * 4)   # unwarped
    T = int(frame_off[-1])
    # one mixture per factor, its mean near one segment's mean cepstrum so that the segments do not all take one class
    c = ceps.cpu().numpy()
    model = diagonal_model(3, fe.n_ceps, 5)
    for k, u in enumerate((0, 2, 3)):
        model["means"][model["dens_mean"][model["dens_index"][model["mix_offsets"][k]]]] = c[frame_off[u]:frame_off[u + 1]].mean(axis=0)
    gmm = rasr_amd.GmmFeatureScorer(ctx, model, "diagonal-maximum")
    b = rasr_amd.BayesClassifier(ctx, 3)
    lab = torch.full((4,), SENTINEL_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert b.classify_gmm(gmm, frame_off, ceps, lab) == (0, 0)
    torch.cuda.synchronize()
    labels = lab.cpu().numpy()
    sc = np.zeros((T, 3), np.float32)
    sc[:], _ = gmm.score(c)
    assert np.array_equal(labels, br.classify_batch(sc, frame_off)["segment_label"]) and len(set(labels.tolist())) >= 2
    chosen = rasr_amd.BayesClassifier.warping_factors(labels, factors)
    by_label, _ = fe.run_batch_dev(sample_off, pcm_dev, warping_factors=chosen)
    by_hand, _ = fe.run_batch_dev(sample_off, pcm_dev, warping_factors=[factors[int(l)] for l in labels])
    assert same(by_label.cpu().numpy(), by_hand.cpu().numpy())
    assert not same(by_label.cpu().numpy(), c)                                   # and some segment really was warped
    b.close()
