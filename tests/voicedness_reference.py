"""NumPy restatement of voicedness.flow in the reference's operation order: f32 data, f64 where the reference uses f64.  All frames of
a segment are carried through each step together (arrays [frames x n]); the arithmetic per frame is the reference's.

  frames           Signal/WindowBuffer.cc:84-125 (framing, flush: the short last frame) + Signal/VectorResize.hh:93-113 (zeros to new-size)
  normalize        Signal/VectorNormalization.hh:44-49
  real_fft / real_ifft   Math/FastFourierTransform.cc:28-146 (bit reversal, Danielson-Lanczos with f64 recurrences, the split step)
  autocorrelation  Signal/CrossCorrelation.cc:31-64, 121-122; CrossCorrelation.hh:43-48; Signal/FastFourierTransform.cc:66-73, 125-132
  maximal_peak_index / _value   Signal/PeakDetection.cc:42-68, 92-98 as a plain loop
"""
import numpy as np

F32_MIN = np.float32(-3.40282347e+38)   # Core::Type<f32>::min (Core/Types.hh:147)
U32_MAX = 0xFFFFFFFF


def rint(x):
    return int(np.rint(x))


def geometry(sample_rate=16000.0, win_len_s=0.040, win_shift_s=0.010, corr_end_s=0.040, min_position_s=0.0025, max_position_s=0.0167):
    """the nodes' conversions of seconds to indices: rint(seconds * sample rate) everywhere"""
    g = dict(frame_len=rint(win_len_s * sample_rate), frame_shift=rint(win_shift_s * sample_rate), n_lags=rint(corr_end_s * sample_rate),
             # PeakDetection.hh:33-36: the continuous positions are f32 members, the product with the f64 sample rate is f64
             min_position=rint(float(np.float32(min_position_s)) * sample_rate),
             max_position=rint(float(np.float32(max_position_s)) * sample_rate))
    length = g["frame_len"] + max(0, abs(g["n_lags"] - 1))   # CrossCorrelation.cc:34-36, begin = 0
    n = 1
    while n < length:
        n <<= 1
    g["fft_len"] = n
    return g


def n_frames(n, frame_len, frame_shift):
    if n <= 0:
        return 0
    reach = max(frame_len, frame_shift)
    return 1 if n <= reach else (n - reach + frame_shift - 1) // frame_shift + 1


def frames(pcm, frame_len, frame_shift):
    """rectangular window (weights 1.0f: the product is the sample) and the resize to frame_len"""
    pcm = np.asarray(pcm, np.float32)
    T = n_frames(len(pcm), frame_len, frame_shift)
    out = np.zeros((T, frame_len), np.float32)
    for t in range(T):
        seg = pcm[t * frame_shift:t * frame_shift + frame_len]
        out[t, :len(seg)] = seg
    return out


def energy_sum(v):
    """std::inner_product(v.begin(), v.end(), v.begin(), 0.0): f32 products added to a double in index order"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        prod = (v * v).astype(np.float64)
        inner = np.zeros(v.shape[0], np.float64)
        for i in range(v.shape[1]):
            inner = inner + prod[:, i]
    return inner


def normalize(v):
    """sqrt(inner_product(v, v, 0.0) / v.size()) narrowed to f32; every element times (f32)1 / it"""
    v = np.asarray(v, np.float32)
    inner = energy_sum(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float32(1) / np.sqrt(inner / float(v.shape[1])).astype(np.float32)
        return v * r[:, None]


def _bit_reversal(v):
    size = v.shape[1]
    order = np.arange(size)
    j = 1
    for i in range(1, size, 2):
        if j > i:
            order[i - 1], order[i] = j - 1, j
        m = size // 2
        while m >= 2 and j > m:
            j -= m
            m >>= 1
        j += m
    for i in range(size):                       # std::swap(v[i], v[reording_[i]]) for every i in turn
        k = order[i]
        if k != i:
            v[:, [i, k]] = v[:, [k, i]]


def _transform(v, inverse):
    """FastFourierTransform::transform on [frames x size] f32, in place"""
    size = v.shape[1]
    theta_base = 6.28318530717959 * (-1.0 if inverse else 1.0)
    _bit_reversal(v)
    cur = 2
    while cur < size:
        step = cur << 1
        theta = theta_base / cur
        s = np.sin(0.5 * theta)
        wpR, wpI = -2.0 * s * s, np.sin(theta)
        wR, wI = 1.0, 0.0
        for m in range(1, cur, 2):
            i = np.arange(m, size + 1, step)
            j = i + cur
            a, b = v[:, j - 1].astype(np.float64), v[:, j].astype(np.float64)
            tmpR = (wR * a - wI * b).astype(np.float32)
            tmpI = (wR * b + wI * a).astype(np.float32)
            v[:, j - 1] = v[:, i - 1] - tmpR
            v[:, j] = v[:, i] - tmpI
            v[:, i - 1] += tmpR
            v[:, i] += tmpI
            wR, wI = wR * wpR - wI * wpI + wR, wI * wpR + wR * wpI + wI
        cur = step


def _transform_real(v, inverse):
    size = v.shape[1]
    theta = (3.141592653589793238 * (-1 if inverse else 1)) / (size >> 1)
    c = np.float32(0.5 if inverse else -0.5)
    if not inverse:
        _transform(v, False)
    s = np.sin(0.5 * theta)
    wpR, wpI = -2.0 * s * s, np.sin(theta)
    wR, wI = wpR + 1, wpI
    for i in range(1, size >> 2):
        i1, i2, i3, i4 = 2 * i, 2 * i + 1, size - 2 * i, size - 2 * i + 1
        h1R = 0.5 * (v[:, i1] + v[:, i3]).astype(np.float64)     # f32 sums, f64 products
        h1I = 0.5 * (v[:, i2] - v[:, i4]).astype(np.float64)
        h2R = (-c * (v[:, i2] + v[:, i4])).astype(np.float64)    # f32 products
        h2I = (c * (v[:, i1] - v[:, i3])).astype(np.float64)
        v[:, i1] = (h1R + wR * h2R - wI * h2I).astype(np.float32)
        v[:, i2] = (h1I + wR * h2I + wI * h2R).astype(np.float32)
        v[:, i3] = (h1R - wR * h2R + wI * h2I).astype(np.float32)
        v[:, i4] = (-h1I + wR * h2I + wI * h2R).astype(np.float32)
        wR, wI = wR * wpR - wI * wpI + wR, wI * wpR + wR * wpI + wI
    h = v[:, 0].copy()
    if inverse:
        v[:, 0] = (0.5 * (h + v[:, 1]).astype(np.float64)).astype(np.float32)
        v[:, 1] = (0.5 * (h - v[:, 1]).astype(np.float64)).astype(np.float32)
        _transform(v, True)
    else:
        v[:, 0] = h + v[:, 1]
        v[:, 1] = h - v[:, 1]


def real_fft(x, fft_len):
    """RealFastFourierTransform(length) with the default sample rate 1 (no scale): [frames x (fft_len + 2)] alternating complex"""
    x = np.asarray(x, np.float32)
    v = np.zeros((x.shape[0], fft_len), np.float32)
    v[:, :x.shape[1]] = x
    with np.errstate(invalid="ignore"):
        _transform_real(v, False)
    out = np.zeros((x.shape[0], fft_len + 2), np.float32)       # unpack
    out[:, :fft_len] = v
    out[:, fft_len] = v[:, 1]
    out[:, 1] = 0
    return out


def real_ifft(X, sample_rate):
    """RealInverseFastFourierTransform(length, sample_rate): pack, inverse transform, times 2 / (f32)sample_rate"""
    X = np.asarray(X, np.float32)
    v = X[:, :-2].copy()
    v[:, 1] = X[:, -2]
    with np.errstate(invalid="ignore"):
        _transform_real(v, True)
        if sample_rate != 2:
            v = v * (np.float32(2) / np.float32(sample_rate))
    return v


def autocorrelation(x, n_lags, normalization="unbiased-estimate", contract="off"):
    """CrossCorrelation::apply with x = y, begin = 0, end = n_lags on normalised frames [frames x size].
    contract: which build of the reference.  The two differ in bits at ONE place that reaches an f32 result: x * conj(x) of
    Math::conjugateMultiplies, where the -march=native build fuses re = fma(a, a, b b) and im = fma(b, a, -(a b)) (an imaginary part
    of rounding-error size instead of zero).  The f64 expressions of the transforms (Math/FastFourierTransform.cc:79-80, 125-128) are
    fused there too, but narrowed to f32 they gave the same bits on every recorded value (tests/golden/ref_voicedness.npz)."""
    x = np.asarray(x, np.float32)
    size = x.shape[1]
    fft_len = 1
    while fft_len < size + abs(n_lags - 1):
        fft_len <<= 1
    X = real_fft(x, fft_len)
    re, im = X[:, 0::2], X[:, 1::2]
    with np.errstate(invalid="ignore", over="ignore"):
        P = np.zeros_like(X)
        if contract == "fma":   # an f32 fma through f64: the product of two f32 is exact there
            a, b = re.astype(np.float64), im.astype(np.float64)
            P[:, 0::2] = (a * a + (im * im).astype(np.float64)).astype(np.float32)
            P[:, 1::2] = (b * a - (re * im).astype(np.float64)).astype(np.float32)
        else:
            P[:, 0::2] = re * re + im * im      # x * conj(x), real part a a - b (-b); the imaginary part a (-b) + b a is zero
    R = real_ifft(P, float(fft_len))[:, :n_lags].copy()   # fft.outputSampleRate() = length / 1
    if normalization == "unbiased-estimate":
        N = size - np.arange(n_lags)
        with np.errstate(invalid="ignore", divide="ignore"):
            R = np.where(N > 0, R / np.maximum(N, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return R


def maximal_peak_index(v, min_position, max_position):
    """PeakDetection::getMaximalPeakIndex, statement by statement"""
    n = len(v)
    best_value, best_position = F32_MIN, U32_MAX
    peak_begin = 1
    while peak_begin + 1 < n:
        if v[peak_begin - 1] < v[peak_begin] and v[peak_begin] >= v[peak_begin + 1]:
            peak_end = peak_begin
            while peak_end + 1 < n and v[peak_end] == v[peak_end + 1]:
                peak_end += 1
            if (peak_end + 1 < n and v[peak_end] > v[peak_end + 1] and v[peak_end] > best_value and
                    peak_begin <= max_position and peak_end >= min_position):
                best_value = v[peak_end]
                best_position = (peak_begin + peak_end) // 2
                best_position = min(max(best_position, min_position), max_position)
            peak_begin = peak_end
        peak_begin += 1
    return best_position


def maximal_peak_value(v, min_position, max_position):
    i = maximal_peak_index(v, min_position, max_position)
    return np.float32(v[i]) if i < U32_MAX else np.float32(0)


def voicedness(pcm, sample_rate=16000.0, normalization="unbiased-estimate", return_acf=False, contract="off", **kw):
    """the whole network on one segment: [frames] f32 (and the autocorrelation vectors)"""
    g = geometry(sample_rate, **kw)
    x = normalize(frames(pcm, g["frame_len"], g["frame_shift"]))
    acf = autocorrelation(x, g["n_lags"], normalization, contract) if len(x) else np.zeros((0, g["n_lags"]), np.float32)
    out = np.array([maximal_peak_value(a.tolist(), g["min_position"], g["max_position"]) for a in acf], np.float32)
    return (out, acf) if return_acf else out
