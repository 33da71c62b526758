"""Plain restatement (numpy, f64, no GPU) of the arithmetic that AMX_PREC_F16MX and AMX_PREC_BF16X3 promise for ONE layer, written from
the header of rasr_amd/csrc/ffnn_mx.hpp and the comment above pack_input_bf16x3 in ffnn.hip -- not from the kernels.

f16mx, operands x [T x K] and W [N x K] (f32), K padded with zeros to blocks of 32 consecutive k:
    h(v) = f16(v), round to nearest even
    E    = biased f32 exponent of the block's largest |v|, at least 14; a frame keeps its own, weight rows n and n ^ 32 share the larger
           of their two block maxima (a partner row beyond N counts as zero)
    r(v) = e2m3 of v - h(v) under the scale 2^(E - 13 - 127)
    q(v) = e2m3 of h(v)     under the scale 2^(E - 2 - 127)
    S    = sum_k h(x) h(w) + q(x) r(w) + r(x) q(w)
bf16x3: hi = bf16(v), lo = bf16(v - hi), S = sum_k xh wh + xh wl + xl wh.

restate() evaluates S twice: in f64 ("S64", the exact value of the promise) and in f32 in the documented order ("S32": K-tiles of 32
ascending; per tile the f16 product of k-slab 0, of k-slab 1, then the 64-deep scaled product -- split bf16: per slab of 16 k the
products hi.hi, lo.hi, hi.lo with the WEIGHTS' plane named first, as the kernels name them: wh xh, wl xh, wh xl -- each matrix instruction's own sum taken by an f32 matrix product, the accumulator updated in f32).
Their distance measures what f32 accumulation costs on the case's own operands; bar() forms the test's bound from it.  `defect=`
plants one deliberate deviation; tests/test_split_gemm_reference.py shows that every one of them leaves the bar on every case that
tests/test_ffnn_split_exact_gpu.py runs.  The cases (shapes, operand families) live here because both files walk them.
"""
import numpy as np

F16MX_DEFECTS = ("r_truncated", "w_exponent_unpaired", "x_exponent_paired", "last_tile_cross_dropped", "q_unsaturated",
                 "r_scale_off_by_one", "padding_k_counts", "exponent_unclamped")
BF16X3_DEFECTS = ("lo_truncated", "lo_lo_added", "lo_hi_dropped_last_tile")
DEFECTS = {"f16mx": F16MX_DEFECTS, "bf16x3": BF16X3_DEFECTS}

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_ELU = 0, 1, 2, 3, 4

# ------------------------------------------------------------------------------------------------ e2m3 (OCP MX fp6)
# code = sign (bit 5) | exponent (2 bits) | mantissa (3 bits); exponent 0: subnormal m / 8, else (1 + m / 8) 2^(e - 1); largest 7.5
E2M3_MAGNITUDES = np.array([(m / 8.0) if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1) for e in range(4) for m in range(8)])


def e2m3_decode(code):
    code = np.asarray(code)
    return np.where(code & 32, -1.0, 1.0) * E2M3_MAGNITUDES[code & 31]


def e2m3_encode(a, truncate=False):
    """code of the e2m3 value nearest to a (f64; ties to the even code; |a| >= 7.5 saturates; gradual underflow: the codes below 8 are
    the subnormals; the sign bit of a zero is kept), by search in the table of the 32 magnitudes.  truncate: toward zero instead."""
    a = np.asarray(a, np.float64)
    m = np.abs(a)
    up = np.minimum(np.searchsorted(E2M3_MAGNITUDES, m, side="left"), 31)   # first magnitude >= m (31: saturated)
    dn = np.maximum(up - 1, 0)
    exact = E2M3_MAGNITUDES[up] == m
    if truncate:
        code = np.where(exact | (m >= 7.5), up, dn)
    else:
        d_up, d_dn = E2M3_MAGNITUDES[up] - m, m - E2M3_MAGNITUDES[dn]
        code = np.where(d_up < d_dn, up, np.where(d_up > d_dn, dn, np.where(up % 2 == 0, up, dn)))
        code = np.where(exact | (m >= 7.5), up, code)
    return (code | np.where(np.signbit(a), 32, 0)).astype(np.int64)


def e2m3(a, truncate=False):
    return e2m3_decode(e2m3_encode(a, truncate))


# ------------------------------------------------------------------------------------------------ operands
def _pad_k(v, mult, wrap=False):
    """[rows x K] -> [rows x Kp]; the tail is zero, or (planted defect) what a read without the k < K check finds: the flat array's
    next values, wrapping at its end"""
    rows, K = v.shape
    Kp = -(-K // mult) * mult
    out = np.zeros((rows, Kp), np.float32)
    out[:, :K] = v
    if wrap and Kp > K:
        flat = v.reshape(-1)
        idx = (np.arange(rows)[:, None] * K + np.arange(K, Kp)[None, :]) % flat.size
        out[:, K:] = flat[idx]
    return out


def f16(v):
    return np.asarray(v, np.float32).astype(np.float16).astype(np.float32)


def block_exponent(max_abs, clamp=True):
    e = ((np.ascontiguousarray(max_abs, np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    return np.maximum(e, 14) if clamp else e


def split_f16mx(v, side, defect=None):
    """v [rows x K] f32, side "x" (frames) or "w" (weight rows) -> h, q, r as f64 [rows x Kp], exactly the values the products take"""
    vp = _pad_k(np.asarray(v, np.float32), 32, wrap=defect == "padding_k_counts")
    rows, Kp = vp.shape
    h = f16(vp)
    lo = (vp - h).astype(np.float64)          # exact in f32
    bmax = np.abs(vp).reshape(rows, Kp // 32, 32).max(axis=2)
    paired = (side == "w") != (defect == ("w_exponent_unpaired" if side == "w" else "x_exponent_paired"))
    if paired:
        rp = -(-rows // 64) * 64
        m = np.zeros((rp, Kp // 32), np.float32)
        m[:rows] = bmax
        partner = m[np.arange(rp) ^ 32]
        bmax = np.maximum(m, partner)[:rows]
    E = block_exponent(bmax, clamp=defect != "exponent_unclamped")
    E = np.repeat(E, 32, axis=1)
    sq = np.ldexp(1.0, E - 2 - 127)
    sr = np.ldexp(1.0, E - (12 if defect == "r_scale_off_by_one" else 13) - 127)
    r = e2m3(lo / sr, truncate=defect == "r_truncated") * sr
    q = h.astype(np.float64) if defect == "q_unsaturated" else e2m3(h.astype(np.float64) / sq) * sq
    return h.astype(np.float64), q, r


def bf16_round(v, truncate=False):
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    if not truncate:
        u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) << 16).astype(np.uint32).view(np.float32)


def split_bf16x3(v, defect=None):
    """-> hi, lo (f32 values that are bf16) [rows x Kp], K padded to the 32-k tile with zeros"""
    vp = _pad_k(np.asarray(v, np.float32), 32)
    hi = bf16_round(vp)
    lo = bf16_round(vp - hi, truncate=defect == "lo_truncated")
    return hi, lo


# ------------------------------------------------------------------------------------------------ one layer
def activate(z, act):
    """the activation on f64 (f32 input: the result is rounded to f32 by the caller)"""
    z = np.asarray(z, np.float64)
    if act == ACT_RELU:
        return np.where(z < 0, 0.0, z)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-z))
    if act == ACT_TANH:
        return np.tanh(z)
    if act == ACT_ELU:
        return np.where(z < 0, np.expm1(np.minimum(z, 0.0)), z)
    return z


def folded_bias(bias, n, last, log_prior=None, prior_scale=1.0):
    """the bias as the handle holds it (f32): the output layer's has prior_scale * log_prior removed, rounded after each step"""
    b = np.zeros(n, np.float32) if bias is None else np.asarray(bias, np.float32).copy()
    if last and log_prior is not None and prior_scale != 0.0:
        b = b - np.float32(prior_scale) * np.asarray(log_prior, np.float32)
    return b.astype(np.float32)


class Restated:
    """S64 / S32: the sum in f64 / in f32 in the documented order; z64 = S64 + bias; out64: the layer's exact output (-z, or act(z)),
    out32: the same through f32 (S32, bias added in f32, the activation rounded to f32)"""

    def __init__(self, S64, S32, bias, last, act):
        self.S64, self.S32, self.bias, self.last, self.act = S64, S32, bias.astype(np.float64)[None, :], last, act
        self.z64 = S64 + self.bias
        z32 = (S32 + bias[None, :]).astype(np.float32)
        if last:
            self.out64, self.out32 = -self.z64, -z32
        else:
            self.out64, self.out32 = activate(self.z64, act), activate(z32, act).astype(np.float32)


def _f32_groups(acc, groups):
    for a, b in groups:
        acc = (acc + np.matmul(a.astype(np.float32), b.astype(np.float32).T)).astype(np.float32)
    return acc


def restate(scheme, x, W, bias=None, act=ACT_NONE, last=True, log_prior=None, prior_scale=1.0, defect=None, x_split=None, exact_only=False):
    """one layer of `scheme` ("f16mx" | "bf16x3") on frames x [T x K] and weights W [N x K] (f32) -> Restated.
    x_split (bf16x3): the frames' (hi, lo) planes as a previous layer left them, instead of splitting x.
    exact_only: S32 is not evaluated (a copy of S64 rounded to f32 stands in)."""
    if defect is not None and defect not in DEFECTS[scheme]:
        raise ValueError("%s has no planted defect %r" % (scheme, defect))
    W = np.asarray(W, np.float32)
    N = W.shape[0]
    b = folded_bias(bias, N, last, log_prior, prior_scale)
    if scheme == "f16mx":
        hx, qx, rx = split_f16mx(x, "x", defect)
        hw, qw, rw = split_f16mx(W, "w", defect)
        KT = hx.shape[1] // 32
        cx, cw = np.concatenate([qx, rx], axis=1), np.concatenate([rw, qw], axis=1)   # [q(x) | r(x)] . [r(w) | q(w)]
        Kp = hx.shape[1]
        if defect == "last_tile_cross_dropped":
            cx = cx.copy()
            cx[:, Kp - 32:Kp] = 0.0
            cx[:, 2 * Kp - 32:] = 0.0
        S64 = hx @ hw.T + cx @ cw.T
        if exact_only:
            return Restated(S64, S64.astype(np.float32), b, last, act)
        acc = np.zeros(S64.shape, np.float32)
        for kt in range(KT):
            k0 = 32 * kt
            sl = np.r_[k0:k0 + 32, Kp + k0:Kp + k0 + 32]
            acc = _f32_groups(acc, [(hx[:, k0:k0 + 16], hw[:, k0:k0 + 16]), (hx[:, k0 + 16:k0 + 32], hw[:, k0 + 16:k0 + 32]), (cx[:, sl], cw[:, sl])])
        return Restated(S64, acc, b, last, act)
    if scheme != "bf16x3":
        raise ValueError(scheme)
    if x_split is None:
        xh, xl = split_bf16x3(x, defect)
    else:
        xh, xl = (_pad_k(np.asarray(p, np.float32), 32) for p in x_split)
    wh, wl = split_bf16x3(W, defect)
    Kp = xh.shape[1]
    xh64, xl64, wh64, wl64 = (a.astype(np.float64) for a in (xh, xl, wh, wl))
    xhc, xlc = xh64, xl64
    if defect == "lo_hi_dropped_last_tile":      # both cross products of the last 32-k tile
        keep = np.ones(Kp)
        keep[Kp - 32:] = 0.0
        xhc, xlc = xh64 * keep, xl64 * keep
    S64 = xh64 @ wh64.T + xhc @ wl64.T + xlc @ wh64.T
    if defect == "lo_lo_added":
        S64 = S64 + xl64 @ wl64.T
    if exact_only:
        return Restated(S64, S64.astype(np.float32), b, last, act)
    acc = np.zeros(S64.shape, np.float32)
    for k0 in range(0, Kp, 16):
        s = slice(k0, k0 + 16)
        groups = [(xh[:, s], wh[:, s]), (xhc[:, s], wl[:, s]), (xlc[:, s], wh[:, s])]     # wh xh, wl xh, wh xl (frames first here: a @ b.T)
        if defect == "lo_lo_added":
            groups.append((xl[:, s], wl[:, s]))
        acc = _f32_groups(acc, groups)
    return Restated(S64, acc, b, last, act)


# ------------------------------------------------------------------------------------------------ the bar
def ulp32(a):
    """spacing of f32 at |a| (f64 array)"""
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def bar(res):
    """elementwise bound on |kernel output - res.out64| for a kernel that keeps the promise:
        4 max|S32 - S64|                    f32 accumulation on these operands; 4: a matrix instruction's internal order is not ours to know
      + 2 ulp_f32(max(|z|, |bias|, |S64|))  the epilogue's two f32 roundings
    A hidden layer's activation has a slope of at most 1 (ReLU, sigmoid, tanh, ELU), so the bound carries over to its output; the
    sigmoid, tanh and ELU go through the device's expf / tanhf (documented at 1-2 ulp) and up to three more f32 roundings (negation is
    exact; 1 + e, the division, e - 1): 4 ulp_f32 of the output beside it.  Nothing here comes from a kernel."""
    b = 4.0 * np.abs(res.S32.astype(np.float64) - res.S64).max() + 2.0 * ulp32(np.maximum(np.maximum(np.abs(res.z64), np.abs(res.bias)), np.abs(res.S64)))
    if not res.last and res.act in (ACT_SIGMOID, ACT_TANH, ACT_ELU):
        b = b + 4.0 * ulp32(res.out64)
    return b


def accumulation_bar(res, x, W):
    """the bar for a case whose excess over bar() was found to be accumulation inside the matrix instructions (f16mx; scores): a derived
    worst case per element instead of the f32 distance measured on S32.  A matrix instruction adds its n_i products and the incoming
    accumulator after aligning them to the largest of them; an addend far below that one loses its low bits -- up to 2^-23 M_i each
    (f32 under truncation), M_i the largest of the products and of the accumulator before and behind the instruction -- and the result
    is rounded once: (n_i + 1) 2^-23 M_i per instruction, summed over the instructions in the documented order.  Never more than the
    coarser worst case 2 n 2^-24 sum_k |terms| over all n accumulated terms.  The epilogue's 2 ulp stay."""
    hx, qx, rx = split_f16mx(x, "x")
    hw, qw, rw = split_f16mx(W, "w")
    Kp = hx.shape[1]
    acc, bound = np.zeros_like(res.S64), np.zeros_like(res.S64)
    for k0 in range(0, Kp, 32):
        t = slice(k0, k0 + 32)
        for a, b in ((hx[:, k0:k0 + 16], hw[:, k0:k0 + 16]), (hx[:, k0 + 16:k0 + 32], hw[:, k0 + 16:k0 + 32]),
                     (np.concatenate([qx[:, t], rx[:, t]], axis=1), np.concatenate([rw[:, t], qw[:, t]], axis=1))):
            largest = np.abs(a[:, None, :] * b[None, :, :]).max(axis=2)
            new = acc + a @ b.T
            bound += (a.shape[1] + 1) * 2.0 ** -23 * np.maximum(np.maximum(np.abs(acc), np.abs(new)), largest)
            acc = new
    sum_abs = np.abs(hx) @ np.abs(hw).T + np.abs(qx) @ np.abs(rw).T + np.abs(rx) @ np.abs(qw).T
    bound = np.minimum(bound, 2.0 * (3 * Kp) * 2.0 ** -24 * sum_abs)
    return bound + 2.0 * ulp32(np.maximum(np.maximum(np.abs(res.z64), np.abs(res.bias)), np.abs(res.S64)))


def distance_over_bar(got, res, the_bar=None):
    """worst |got - out64| / bar over the matrix"""
    return float((np.abs(np.asarray(got, np.float64) - res.out64) / (bar(res) if the_bar is None else the_bar)).max())


# ------------------------------------------------------------------------------------------------ the cases both test files walk
K_AXIS = (1, 7, 31, 32, 33, 64, 96, 97, 130, 257, 288, 440)
N_AXIS = (1, 31, 32, 33, 64, 65, 130, 257)
T_AXIS = (1, 31, 33, 64, 65, 257)
# every value of an axis against ragged values of the other two, and a few corners: (T, K, N)
SHAPES = tuple([(33, k, 65) for k in K_AXIS] + [(65, 97, n) for n in N_AXIS] + [(t, 130, 33) for t in T_AXIS] +
               [(1, 1, 1), (31, 31, 31), (64, 64, 64), (257, 257, 257), (257, 440, 130), (65, 288, 257)])
FAMILIES = ("gaussian", "exact-f16", "q-saturates", "block-outlier", "zero-blocks", "tiny", "below-clamp", "f16-subnormal", "near-65504", "cancellation")
NO_PRIOR = ("tiny", "below-clamp", "f16-subnormal", "cancellation")
FAMILY_SHAPES = ((65, 97, 65), (65, 440, 130))
ACTIVATIONS = (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_ELU)
TWO_LAYER = (97, 130, 65)          # [in, hidden, out] of the ragged two-layer network, at T = 257
TWO_LAYER_T = 257
F16MX_TILES = ("0", "3", "6", "2", "4", "5", "7", "8", "9", "11", "12", "14")
BF16X3_TILES = ("0", "2", "3", "4", "6")
KSPLIT_DIMS = (64, 2048, 2048, 40)
KSPLIT_T = (100, 256)


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def _step_rows(a):
    """rows with bit 5 of their index set are twice as large: partners r and r ^ 32 then differ in their block exponents, so it
    matters who shares an exponent with whom (no more than twice: the bar's first term is a maximum over the output matrix, and a wide
    spread of magnitudes would loosen it for the small rows)"""
    a = a.copy()
    a[(np.arange(a.shape[0]) & 32) != 0] *= 2.0
    return a


def operands(family, T, K, N, seed):
    """-> x [T x K], W [N x K], bias [N] (f32) of one layer in the operand family"""
    g = _rng(seed, T, K, N)
    x = _step_rows(g.standard_normal((T, K))).astype(np.float32)
    W = _step_rows(g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * g.standard_normal(N)).astype(np.float32)
    if family == "gaussian":
        pass
    elif family == "exact-f16":      # r = 0 everywhere: the f16 product alone
        x, W = f16(x), f16(W)
    elif family == "q-saturates":    # every block maximum has a mantissa >= 1.9375: q = 7.5, not 7.75
        for a in (x, W):
            for b0 in range(0, K, 32):
                blk = a[:, b0:b0 + 32]
                j = np.abs(blk).argmax(axis=1)
                m = np.abs(blk[np.arange(len(blk)), j])
                e = np.floor(np.log2(m))
                blk[np.arange(len(blk)), j] = (np.sign(blk[np.arange(len(blk)), j]) * np.exp2(e) * g.uniform(1.9375, 1.9999, len(blk))).astype(np.float32)
    elif family == "block-outlier":  # one value of 2^8 .. 2^12 per block: the other 31 fall into q's subnormals
        for a in (x, W):
            rows = np.arange(a.shape[0])
            for b0 in range(0, K, 32):
                j = b0 + g.integers(0, min(32, K - b0), a.shape[0])
                a[rows, j] = (np.sign(a[rows, j]) * np.exp2(g.integers(8, 13, a.shape[0])) * g.uniform(1.0, 1.99, a.shape[0])).astype(np.float32)
    elif family == "zero-blocks":    # whole blocks and whole rows of zeros beside live ones
        for a in (x, W):
            for b0 in range(0, K, 64):
                a[::2, b0:b0 + 32] = 0.0
            a[3::7] = 0.0
    elif family == "tiny":           # 1e-30: biased exponent 27, still above the clamp
        x = (np.sign(x) * np.maximum(np.abs(x), 0.05) * 1e-30).astype(np.float32)
        bias[:] = 0.0
    elif family == "below-clamp":    # frames of 2^-126 .. 2^-121: every block exponent clamps at 14, h and q of a frame are zero and its
        #                              residual (the value itself, under the scale 2^-126) is all that is left; normal f32 numbers throughout
        x = (np.sign(x) * np.maximum(np.abs(x), 0.3) * 2.0 ** -124).astype(np.float32)
        W = (W * 1e4).astype(np.float32)
        bias[:] = 0.0
    elif family == "f16-subnormal":  # |v| about 1e-6: h has a spacing of 2^-24, r saturates
        x = (x * 1e-6).astype(np.float32)
        W[:, 1::3] *= np.float32(1e-5)
        bias[:] = 0.0
    elif family == "near-65504":     # the top of the f16 range: every value (so every block maximum lies in one binade), either sign;
        #                              64 .. 127 off a multiple of 256, so that split bf16's lo plane carries a residual of weight
        def top(a):
            return (np.sign(a) * (256.0 * g.integers(235, 256, a.shape) + g.choice([-1.0, 1.0], a.shape) * g.uniform(64.0, 127.0, a.shape))).astype(np.float32)
        x, W = top(x), top(W)
    elif family == "cancellation":   # neighbouring k cancel: S is near zero while the sum of |terms| is not
        x[:, 1::2] = x[:, 0:2 * (K // 2):2] * (1.0 + g.standard_normal((T, K // 2)) * 2.0 ** -10).astype(np.float32)
        W[:, 1::2] = -W[:, 0:2 * (K // 2):2] * (1.0 + g.standard_normal((N, K // 2)) * 2.0 ** -10).astype(np.float32)
        bias[:] = 0.0
    else:
        raise ValueError(family)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(W, np.float32), bias


def log_prior(N, seed):
    z = _rng(seed, N).standard_normal(N)
    return (z - (np.log(np.sum(np.exp(z - z.max()))) + z.max())).astype(np.float32)


def two_layer(dims, T, seed, act):
    """x, [W1, W2], [b1, b2], log prior of an [in, hidden, out] network"""
    x, W1, b1 = operands("gaussian", T, dims[0], dims[1], seed)
    _, W2, b2 = operands("gaussian", 1, dims[1], dims[2], seed + 1)
    return x, [W1, W2], [b1, b2], log_prior(dims[2], seed)


def exemption(scheme, defect, T, K, N, family="gaussian", fed_by_epilogue=False):
    """reason why `defect` cannot act on a case, or None"""
    if scheme == "bf16x3":
        if defect == "lo_truncated" and family == "exact-f16":
            return "v - hi has at most three significant bits: bf16 holds it exactly, rounded or truncated"
        return None
    if defect == "padding_k_counts":
        if K % 32 == 0:
            return "K is a whole number of K-tiles: there is no padded k"
        if fed_by_epilogue:
            return "the frames come as the previous layer's blocks, whose padded k the epilogue wrote"
    if defect == "w_exponent_unpaired" and N <= 32:
        return "no weight row has a partner n ^ 32 inside the layer"
    if defect == "x_exponent_paired" and T <= 32:
        return "no frame has a partner t ^ 32 inside the batch"
    if defect == "exponent_unclamped" and family != "below-clamp":
        return "no block maximum lies below 2^-113 (biased exponent 14) except all-zero blocks, whose products are zero either way"
    if family == "below-clamp" and defect == "x_exponent_paired":
        return "every block of every frame clamps to the exponent 14, shared or not"
    if family == "exact-f16" and defect != "padding_k_counts":
        return "every residual is zero, so both cross terms are zero whatever scale, rounding or q they are given"
    if family == "tiny" and defect == "r_truncated":
        return "every frame's residual saturates (h = 0, |v| > 500 scales), and q(x) = 0 takes the weights' residual out of the sum"
    if family == "near-65504" and defect == "x_exponent_paired":
        return "every block of every frame has its maximum in the same binade"
    if family == "near-65504" and defect == "w_exponent_unpaired":
        return "every block of every weight row has its maximum in the same binade"
    return None


class Case:
    """one network the GPU file runs: dims [K, N] (scores of a one-layer network), [K, H, N] (first layer through
    forward_hidden_dev, output layer from the kernel's own hidden values) or KSPLIT_DIMS (its last two layers)"""

    def __init__(self, scheme, dims, T, family="gaussian", act=ACT_RELU, tuning="", seed=1):
        self.scheme, self.dims, self.T, self.family, self.act, self.tuning, self.seed = scheme, tuple(dims), T, family, act, tuning, seed

    @property
    def id(self):
        s = "%s-T%d-%s" % (self.scheme, self.T, "x".join(str(d) for d in self.dims))
        if self.family != "gaussian":
            s += "-" + self.family
        if len(self.dims) > 2:
            s += "-act%d" % self.act
        if self.tuning:
            s += "-" + self.tuning.replace("=", "")
        return s

    def network(self):
        """x, Ws, biases, activations, log prior"""
        d = self.dims
        x, W, b = operands(self.family, self.T, d[0], d[1], self.seed)
        Ws, bs = [W], [b]
        for l in range(1, len(d) - 1):
            _, W, b = operands("gaussian", 1, d[l], d[l + 1], self.seed + l)
            Ws.append(W)
            bs.append(b)
        acts = [self.act] * (len(d) - 2) + [ACT_NONE]
        if len(d) > 2 and self.act == ACT_SIGMOID:
            # sigmoid outputs of a centred layer nearly all have their block maximum in [0.5, 1): one binade, and it would not matter
            # who shares an exponent with whom.  A bias of -3 spreads the hidden values over 0.007 .. 0.3
            bs[0] = (bs[0] - 3.0).astype(np.float32)
        # (families of tiny magnitudes carry neither a bias nor a prior: an addend of order 1 would put every score's ulp above them)
        return x, Ws, bs, acts, None if self.family in NO_PRIOR else log_prior(d[-1], self.seed)

    def layers(self):
        """indices of the layers that are compared at the bar, each on its own.  Split bf16 keeps a hidden layer's output as the two
        planes hi + lo (16 significant bits), so forward_hidden_dev cannot show its first layer's sum at f32 accuracy: that layer
        is compared through one-layer networks only (and coarsely in the two-layer ones, see the GPU file)"""
        n = len(self.dims) - 1
        return [n - 1] if self.scheme == "bf16x3" and n > 1 else list(range(n))[-2:]

    def restate_layer(self, l, x_in, defect=None, x_split=None, exact_only=False, rows=None):
        """layer l on the input x_in (layer 0: the features; else the hidden values in front of it); rows: only the layer's first
        `rows` outputs (a multiple of 64, so that every row keeps its partner)"""
        _, Ws, bs, acts, logp = self.network()
        last = l == len(Ws) - 1
        lp = logp if last else None
        return restate(self.scheme, x_in, Ws[l][:rows], bs[l][:rows], act=acts[l], last=last, log_prior=None if lp is None else lp[:rows],
                       defect=defect, x_split=x_split, exact_only=exact_only)

    def bar(self, l, x_in, res):
        """the bar of layer l's comparison.  bar(res) everywhere but on the f16-subnormal family in f16mx: there the kernel stood at 2.15
        (65 x 97 x 65) and 1.07 (65 x 440 x 130) of it, and the excess is accumulation, not the cross terms -- the device conversions
        equal the restatement on every tie, subnormal and saturated value probed through the scorer; the excess follows the
        products of two f16-subnormal operands (a twelfth of them lost, toward zero), which a matrix instruction adds beside products
        2^17 times their size; fifteen products of 0.75 ulp of a sixteenth one come out as 10 ulp, not 11.25.  So, as for any excess
        that scales with 2^-24 sum |terms|, the derived worst case of accumulation_bar takes the place of the measured f32 distance
        (kernel: 0.73 and 0.21 of it; every planted defect still leaves it, by a factor of 3.7 at the least)"""
        if self.scheme == "f16mx" and self.family == "f16-subnormal" and l == 0:
            return accumulation_bar(res, x_in, self.network()[1][0])
        return bar(res)

    def exemption(self, l, defect):
        d = self.dims
        return exemption(self.scheme, defect, self.T, d[l], d[l + 1], self.family if l == 0 else "gaussian", fed_by_epilogue=l > 0)


def gpu_cases():
    cases = []
    for scheme in ("f16mx", "bf16x3"):
        off = "mx_fallback=off" if scheme == "f16mx" else ""
        for T, K, N in SHAPES:
            # (K = 1: a single product shows a rounding defect only if its own residual rounds the other way, and the one pair of
            # frames 0 and 32 shows a shared exponent only if their two values lie in different binades -- the first seeds whose
            # operands show every defect of both schemes)
            cases.append(Case(scheme, [K, N], T, tuning=off, seed={(1, 1, 1): 5, (33, 1, 65): 2}.get((T, K, N), 1)))
        for fam in FAMILIES[1:]:
            for T, K, N in FAMILY_SHAPES:
                cases.append(Case(scheme, [K, N], T, family=fam, tuning=off, seed=2))
        cases.append(Case(scheme, [440, 130], 65, tuning=off, seed=2))     # gaussian at the families' second shape (the first is in SHAPES)
        for act in ACTIVATIONS:
            cases.append(Case(scheme, TWO_LAYER, 65, act=act, tuning=off, seed=3))
        for T, K, H, N in ((33, 33, 97, 33), (257, 7, 33, 1), (64, 440, 257, 130)):
            cases.append(Case(scheme, [K, H, N], T, tuning=off, seed=4))
        for tile in (F16MX_TILES if scheme == "f16mx" else BF16X3_TILES):
            cases.append(Case(scheme, TWO_LAYER, TWO_LAYER_T, tuning=(off + "," if off else "") + "tile=" + tile, seed=5))
    for T in KSPLIT_T:
        cases.append(Case("f16mx", KSPLIT_DIMS, T, tuning="mx_fallback=off,ksplit=4", seed=6))
    return cases
