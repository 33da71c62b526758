"""Plain restatement of the GMM training statistics (Mm::AbstractMixtureSetEstimator::accumulate, Viterbi and weighted Viterbi) in
numpy, from the model dict alone: neither the oracle nor the library is called.

The accumulator is one flat f64 vector [nk | n_mean | n_mean*dim | n_cov | n_cov*dim]: the weight of every mixture entry, the weight
and the sum of x of every mean row, the weight and the sum of x*x of every covariance row.  Frame t, aligned to mixture m with density
j of that mixture, goes to entry k = mix_offsets[m] + j, to mean row dens_mean[dens_index[k]] and covariance row
dens_cov[dens_index[k]] with its weight w: w, w*x and (w*x)*x (the unweighted form is w = 1).  A frame is skipped when its mixture
lies outside the model, when its density is "none" (0xffffffff, or 0xff in the byte form) or lies behind its mixture's last density.

Exact inputs.  With features k/64 (integer |k| <= 512) and weights j/16 (integer 0 <= j <= 32) every product above is exact in f64
and every partial sum of up to 65 536 frames is an integer multiple of 2^-16 below 2^24: no f64 addition ever rounds, so the sums
have ONE right value whatever the order of addition.  `exact_features` / `exact_weights` draw such inputs, `accumulate_int` forms the
same sums in int64 (the proof that `accumulate` itself rounds nowhere on them).
"""
import numpy as np

NO_DENSITY = 0xFFFFFFFF
FEATURE_SCALE, WEIGHT_SCALE = 64, 16


def layout(model):
    """offsets of the five sections and the total length: (off_mw, off_ms, off_cw, off_cs, size)"""
    nk = int(model["mix_offsets"][-1])
    n_mean, n_cov, dim = model["means"].shape[0], model["variances"].shape[0], int(model["dim"])
    off_mw = nk
    off_ms = off_mw + n_mean
    off_cw = off_ms + n_mean * dim
    off_cs = off_cw + n_cov
    return off_mw, off_ms, off_cw, off_cs, off_cs + n_cov * dim


def chosen_density(mixture, density, n_mix):
    """the per-frame density (u32, NO_DENSITY for "none") from any input form: a per-frame list [T] or a matrix [T, ld >= n_mix] of
    which column mixture[t] counts; u32 (signed views allowed: -1 is 0xffffffff) or bytes (0xff is "none")"""
    mixture = np.asarray(mixture).astype(np.int64) & 0xFFFFFFFF
    d = np.asarray(density)
    is_bytes = d.dtype.itemsize == 1
    if d.ndim == 2:   # a frame whose mixture lies outside the model is skipped whatever is picked here
        d = d[np.arange(d.shape[0]), np.where(mixture < n_mix, mixture, 0)]
    d = d.astype(np.int64)
    if is_bytes:
        d = np.where((d & 0xFF) == 0xFF, NO_DENSITY, d & 0xFF)
    return mixture, (d & 0xFFFFFFFF)


def kept_frames(model, mixture, density):
    """(frames that count, their mixture entry k): the skip rules"""
    off = model["mix_offsets"].astype(np.int64)
    n_mix = len(off) - 1
    mixture, d = chosen_density(mixture, density, n_mix)
    inside = mixture < n_mix
    m = np.where(inside, mixture, 0)
    keep = inside & (d < off[m + 1] - off[m])      # NO_DENSITY is larger than any mixture
    t = np.nonzero(keep)[0]
    return t, off[m[t]] + d[t]


def accumulate(model, feats, mixture, density, weight=None, acc=None):
    """Viterbi statistics (weight None) or weighted Viterbi statistics (weight f64 [T]) added into acc (a new zero vector if None)"""
    off_mw, off_ms, off_cw, off_cs, size = layout(model)
    dim = int(model["dim"])
    if acc is None:
        acc = np.zeros(size, np.float64)
    assert acc.dtype == np.float64 and acc.shape == (size,)
    feats = np.asarray(feats, np.float32).reshape(-1, dim)
    t, k = kept_frames(model, mixture, density)
    dens = model["dens_index"].astype(np.int64)[k]
    mi, ci = model["dens_mean"].astype(np.int64)[dens], model["dens_cov"].astype(np.int64)[dens]
    w = np.ones(len(t), np.float64) if weight is None else np.asarray(weight, np.float64)[t]
    y = feats[t].astype(np.float64)
    wy = w[:, None] * y
    np.add.at(acc, k, w)
    np.add.at(acc, off_mw + mi, w)
    np.add.at(acc, off_cw + ci, w)
    np.add.at(acc[off_ms:off_cw].reshape(-1, dim), mi, wy)
    np.add.at(acc[off_cs:].reshape(-1, dim), ci, wy * y)
    return acc


def exact_features(T, dim, seed):
    """(f32 features [T, dim] = k / 64, the integers k) with |k| <= 512"""
    k = np.random.Generator(np.random.PCG64(seed)).integers(-512, 513, (T, dim))
    return (k / FEATURE_SCALE).astype(np.float32), k.astype(np.int64)


def exact_weights(T, seed):
    """(f64 weights [T] = j / 16, the integers j) with 0 <= j <= 32"""
    j = np.random.Generator(np.random.PCG64(seed)).integers(0, 33, T)
    return j / float(WEIGHT_SCALE), j.astype(np.int64)


def accumulate_int(model, k_feats, mixture, density, j_weight=None):
    """the statistics of exact inputs from their integers, summed in int64 and scaled once: features k_feats / 64, weights
    j_weight / 16 (None: 1).  Every scaled value is an integer below 2^53 over a power of two, so the division is exact."""
    off_mw, off_ms, off_cw, off_cs, size = layout(model)
    dim = int(model["dim"])
    t, k = kept_frames(model, mixture, density)
    dens = model["dens_index"].astype(np.int64)[k]
    mi, ci = model["dens_mean"].astype(np.int64)[dens], model["dens_cov"].astype(np.int64)[dens]
    kf = np.asarray(k_feats, np.int64).reshape(-1, dim)[t]
    j = np.full(len(t), WEIGHT_SCALE, np.int64) if j_weight is None else np.asarray(j_weight, np.int64)[t]
    acc = np.zeros(size, np.int64)
    np.add.at(acc, k, j)
    np.add.at(acc, off_mw + mi, j)
    np.add.at(acc, off_cw + ci, j)
    np.add.at(acc[off_ms:off_cw].reshape(-1, dim), mi, j[:, None] * kf)
    np.add.at(acc[off_cs:].reshape(-1, dim), ci, j[:, None] * kf * kf)
    assert np.abs(acc).max(initial=0) < 1 << 53
    scale = np.full(size, float(WEIGHT_SCALE))
    scale[off_ms:off_cw] *= FEATURE_SCALE
    scale[off_cs:] *= FEATURE_SCALE * FEATURE_SCALE
    return acc.astype(np.float64) / scale


# ---- the cases both test files build: models by tying, alignments by what they do to a block of 256 frames, skipped frames

MODEL_KINDS = ("cart", "tied", "tied-partial", "shared-means")
COV_KINDS = ("pooled", "grouped", "density")


def model(kind, cov, dim, seed):
    """a small model (at least 256 mixture entries) of one tying kind: "cart" (every mixture owns 4..12 densities), "tied" (every
    mixture lists all 48 densities), "tied-partial" (10 of 64), "shared-means" (CART whose densities share a third as many mean rows);
    cov "pooled" (one covariance), "density" (one each) or "grouped" (1 < n_cov < n_dens: one per mixture for the CART kinds, seven
    spread over the densities for the tied ones)"""
    from tests import synth
    pooled = cov == "pooled"
    if kind in ("cart", "shared-means"):
        m = synth.gmm_cart(48, 4, 12, dim, seed=seed, pooled=pooled)
        if cov == "grouped":
            m = synth.gmm_retie(m, seed + 1, cov="mixture")
        if kind == "shared-means":
            m = synth.gmm_retie(m, seed + 2, n_mean=len(m["dens_mean"]) // 3)
    else:
        m = synth.gmm_tied(12, 48, dim, seed=seed, pooled=pooled) if kind == "tied" else synth.gmm_tied(30, 64, dim, seed=seed, pooled=pooled, k_per_mix=10)
        if cov == "grouped":
            m = synth.gmm_retie(m, seed + 1, cov=7)
    n_dens, n_cov = len(m["dens_mean"]), m["variances"].shape[0]
    assert {"pooled": n_cov == 1, "grouped": 1 < n_cov < n_dens, "density": n_cov == n_dens}[cov] and int(m["mix_offsets"][-1]) >= 256
    return m


ALIGNMENTS = ("one", "distinct", "straddle", "bursty", "random")


def alignment(mdl, T, kind, seed):
    """(mixture i32 [T], density within the mixture u32 [T]):
      "one"       every frame to the same entry: one chain through all 256 frames of a block
      "distinct"  256 different entries in every block: every frame leads a chain of its own
      "straddle"  runs of 100 frames that begin 37 frames before the first block: every run but a few crosses a block edge
      "bursty"    runs of 7, like an aligned utterance;  "random": no runs"""
    off = mdl["mix_offsets"].astype(np.int64)
    nk = int(off[-1])
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(T)
    if kind == "one":
        k = np.full(T, nk // 2)
    elif kind == "distinct":
        assert nk >= 256
        k = (t % 256 + 11 * (t // 256)) % nk
    elif kind == "straddle":
        k = rng.integers(0, nk, T // 100 + 2)[(t + 37) // 100]
    elif kind == "bursty":
        k = np.repeat(rng.integers(0, nk, T // 7 + 1), 7)[:T]
    else:
        assert kind == "random"
        k = rng.integers(0, nk, T)
    m = np.searchsorted(off, k, side="right") - 1
    return m.astype(np.int32), (k - off[m]).astype(np.uint32)


def add_skips(mdl, mixture, density, feats, frames):
    """make `frames` contribute nothing, by the five ways in turn: a NaN feature (the scorers then write "none"), a mixture index
    == n_mix, a mixture index -1, a density index == the mixture's density count, "none" on a finite frame.  Returns the NaN frames."""
    n_of = np.diff(mdl["mix_offsets"].astype(np.int64))
    nan_frames = []
    for i, t in enumerate(frames):
        way = i % 5
        if way == 0:
            feats[t, t % feats.shape[1]] = np.nan
            density[t] = NO_DENSITY
            nan_frames.append(t)
        elif way == 1:
            mixture[t] = len(n_of)
        elif way == 2:
            mixture[t] = -1
        elif way == 3:
            density[t] = n_of[mixture[t]]
        else:
            density[t] = NO_DENSITY
    return np.asarray(nan_frames, np.int64)


def chain_breaks(T):
    """frames at the head (0), the middle (127, 128) and the tail (255) of every block of 256, and the last frame of all"""
    t = np.arange(T)
    return np.unique(np.concatenate([t[np.isin(t % 256, (0, 127, 128, 255))], [T - 1]]))
