"""CPU tests of tests/split_gemm_reference.py (the plain restatement of the f16mx and split-bf16 arithmetic) and of the bar that
tests/test_ffnn_split_exact_gpu.py holds the kernels to:
  * the e2m3 conversion: every code, every midpoint, saturation, the subnormal step, signed zero;
  * the restatement equals the project's other route to the same numbers, tools/emulate_split_f16_f8.py (exponents by log2,
    rounding by rint), operand by operand and in the f32 result;
  * THE BAR IS SHARP: on every case of the GPU file, every planted defect that can act there moves at least one output beyond the bar;
  * the scheme itself -- S against the true product -- lies far outside the bar: the bar sees what 1e-4 |ref| + 1e-4 cannot."""
import os
import sys

import numpy as np
import pytest

from tests import split_gemm_reference as R
from tests import synth

QUIET = dict(over="ignore", invalid="ignore", divide="ignore")   # (a planted defect may push a value out of range; the comparison then sees it)


# ------------------------------------------------------------------------------------------------ e2m3
def test_e2m3_every_code_decodes_and_encodes_to_itself():
    codes = np.arange(64)
    vals = R.e2m3_decode(codes)
    assert np.array_equal(R.e2m3_encode(vals), codes)
    assert np.array_equal(R.e2m3_encode(vals, truncate=True), codes)
    assert vals[31] == 7.5 and vals[63] == -7.5 and vals[1] == 0.125 and vals[8] == 1.0 and vals[7] == 0.875
    assert np.all(np.diff(R.E2M3_MAGNITUDES) > 0)


def test_e2m3_midpoints_round_to_the_even_code():
    m = R.E2M3_MAGNITUDES
    for c in range(31):
        mid = 0.5 * (m[c] + m[c + 1])            # exact: neighbouring codes differ by 1/8, 1/4 or 1/2
        even = c if c % 2 == 0 else c + 1
        assert R.e2m3_encode(mid) == even and R.e2m3_encode(-mid) == (even | 32), c
        below, above = np.nextafter(mid, 0.0), np.nextafter(mid, 8.0)
        assert R.e2m3_encode(below) == c and R.e2m3_encode(above) == c + 1, c
        assert R.e2m3_encode(mid, truncate=True) == c and R.e2m3_encode(above, truncate=True) == c


def test_e2m3_saturation_edge_subnormal_step_and_signed_zero():
    assert [float(R.e2m3(v)) for v in (7.0, 7.25, 7.5, 7.75, np.nextafter(8.0, 0.0), 8.0, 1e30)] == [7.0, 7.0, 7.5, 7.5, 7.5, 7.5, 7.5]
    assert float(R.e2m3(np.nextafter(7.25, 8.0))) == 7.5 and float(R.e2m3(-7.75)) == -7.5
    # gradual underflow: below 1 the step stays 1/8 (the subnormals), 1/16 is a tie between the codes 0 and 1
    assert [int(R.e2m3_encode(v)) for v in (0.0, 0.0625, np.nextafter(0.0625, 1.0), 0.125, 0.1875, 0.9375, 1.0)] == [0, 0, 1, 1, 2, 8, 8]
    assert int(R.e2m3_encode(-0.0)) == 32 and int(R.e2m3_encode(-1e-9)) == 32 and int(R.e2m3_encode(0.0)) == 0
    assert np.signbit(R.e2m3_decode(32)) or R.e2m3_decode(32) == 0.0


def test_block_exponent_is_the_biased_exponent_clamped_at_14():
    v = np.array([0.0, 1e-40, 2.0 ** -113, np.nextafter(np.float32(2.0 ** -113), np.float32(0)), 1.0, 1.9999, 2.0, 65504.0], np.float32)
    assert R.block_exponent(v).tolist() == [14, 14, 14, 14, 127, 127, 128, 142]
    assert R.block_exponent(v, clamp=False).tolist()[:4] == [0, 0, 14, 13]


# ------------------------------------------------------------------------------------------------ the project's emulation
def _emulation():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
    try:
        import emulate_split_f16_f8 as emu
    finally:
        sys.path.pop(0)
    return emu


def test_restatement_equals_the_emulation_of_the_scheme_as_built():
    """tools/emulate_split_f16_f8.py, scheme "AMX_PREC_F16MX as built", on synth.ffnn([440, 256, 300, 1000], seed 7) with 64 frames: h, q
    and r of every layer's operands and the layer's f32 result.  Where the two differ the header decides:
      * the emulation takes a FRAME's q under the exponent of the block's largest |h(x)|, the header (and pack_input_mx, which hands the
        maximum of the f32 values to block_exponent) under that of the largest |x|.  They differ only where the maximum rounds up to the
        next power of two in f16 (|x| in [2^e (2 - 2^-11), 2^e 2)): the restatement follows the header, such blocks are counted, and
        the comparison of q(x) leaves them out -- on this network there are none among the features and a handful behind the ReLUs;
      * the emulation has no clamp at 14 and the restatement has: no block of this network is that small.
    The emulation is right about everything it was written to decide (the accuracy of the scheme); tools/ is not changed."""
    emu = _emulation()
    Ws, bs, acts, logp = synth.ffnn([440, 256, 300, 1000], seed=7)
    y = np.random.Generator(np.random.PCG64(6)).standard_normal((64, 440)).astype(np.float32)
    n_diff = 0
    for l, W in enumerate(Ws):
        eh, eq, er = emu.split(W, "e2m3", "e2m3", "block", True, True)
        K = W.shape[1]
        h, q, r = (a[:, :K] for a in R.split_f16mx(W, "w"))
        assert np.array_equal(h, eh) and np.array_equal(r, er.astype(np.float64)) and np.array_equal(q, eq.astype(np.float64)), l
        xh, xq, xr = emu.split(y, "e2m3", "e2m3", "block", True, False)
        h, q, r = (a[:, :K] for a in R.split_f16mx(y, "x"))
        assert np.array_equal(h, xh) and np.array_equal(r, xr.astype(np.float64)), l
        pad = (-K) % 32
        blocks = lambda a: np.pad(np.abs(a), ((0, 0), (0, pad))).reshape(len(a), -1, 32).max(axis=2)
        differ = np.repeat(R.block_exponent(blocks(y)) != R.block_exponent(blocks(xh)), 32, axis=1)[:, :K]
        n_diff += int(differ.any(axis=1).sum())
        assert np.array_equal(q[~differ], xq.astype(np.float64)[~differ]), l
        assert differ.mean() < 1e-2
        # the layer's f32 result: the emulation's three sgemms against the restatement's f32 evaluation, both within f32 accumulation of S64
        res = R.restate("f16mx", y, W, bs[l], act=acts[l], last=l == len(Ws) - 1, log_prior=logp)
        z = xh @ eh.T + (np.where(differ, q, xq).astype(np.float32) @ er.T + xr @ eq.T)
        tol = 4.0 * np.abs(res.S32 - res.S64).max() + 2.0 * R.ulp32(res.S64)
        assert np.all(np.abs(z.astype(np.float64) - res.S64) <= tol), (l, np.abs(z - res.S64).max(), tol.max())
        y = res.out32 if l < len(Ws) - 1 else y
    print("blocks whose exponent the two routes take differently:", n_diff)


def test_bf16x3_restatement_equals_the_emulation():
    emu = _emulation()
    g = np.random.Generator(np.random.PCG64(3))
    v = (g.standard_normal((40, 97)) * np.exp2(g.integers(-20, 20, (40, 97)))).astype(np.float32)
    hi, lo = (a[:, :97] for a in R.split_bf16x3(v))
    eh = emu.bf16_round(v)
    assert np.array_equal(hi, eh) and np.array_equal(lo, emu.bf16_round(v - eh))
    assert np.all(np.abs(v - hi - lo) <= 2.0 ** -16 * np.abs(v))


# ------------------------------------------------------------------------------------------------ the bar is sharp
CASES = R.gpu_cases()


def _chain(case):
    """the case's compared layers, each with its input: the features, or -- standing in for the kernel's own hidden values of the GPU
    run -- the restatement's f32 output of the layer in front"""
    x = case.network()[0]
    out = []
    for l in range(len(case.dims) - 1):
        if l in case.layers():
            out.append((l, x))
        if l < len(case.dims) - 2:
            x = case.restate_layer(l, x).out32
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_planted_defect_leaves_the_bar(case):
    acted = 0
    for l, x_in in _chain(case):
        true = case.restate_layer(l, x_in)
        assert np.isfinite(true.out64).all() and np.isfinite(true.out32).all()
        bar = case.bar(l, x_in, true)
        assert R.distance_over_bar(true.out32, true, bar) <= 0.5          # the restatement's own f32 evaluation sits well inside
        # (a defect has to show in ONE element: on the 2048 x 2048 layer of the split-K network its first 128 outputs are searched)
        rows = 128 if case.dims[l] * case.dims[l + 1] > 1 << 20 else None
        for defect in R.DEFECTS[case.scheme]:
            if case.exemption(l, defect):
                continue
            with np.errstate(**QUIET):
                bad = case.restate_layer(l, x_in, defect=defect, exact_only=True, rows=rows)
            worst = np.nanmax(np.abs(bad.out64 - true.out64[:, :rows]) / (bar if np.ndim(bar) == 0 else bar[:, :rows]))
            assert worst > 1.0, "layer %d, %s: worst distance / bar = %.3g" % (l, defect, worst)
            acted += 1
    assert acted > 0


def test_exemptions_are_the_named_ones():
    """a defect is left out only where it cannot act; every reason, once"""
    reasons = {}
    for c in CASES:
        for l in c.layers():
            for d in R.DEFECTS[c.scheme]:
                why = c.exemption(l, d)
                if why:
                    reasons.setdefault(why, set()).add(d)
    assert len(reasons) <= 12, reasons
    for d in R.F16MX_DEFECTS + R.BF16X3_DEFECTS:     # ... and no defect is exempt everywhere
        scheme = "f16mx" if d in R.F16MX_DEFECTS else "bf16x3"
        assert any(not c.exemption(l, d) for c in CASES if c.scheme == scheme for l in c.layers()), d
    # an exempt defect really does nothing there (checked on the one-layer cases: cheap)
    for c in CASES:
        if len(c.dims) != 2:
            continue
        x = c.network()[0]
        true = None
        for d in R.DEFECTS[c.scheme]:
            if c.exemption(0, d):
                true = true or c.restate_layer(0, x, exact_only=True)
                with np.errstate(**QUIET):
                    assert np.array_equal(c.restate_layer(0, x, defect=d, exact_only=True).S64, true.S64), (c.id, d)


def test_the_scheme_itself_is_far_outside_the_bar():
    """the true f64 product x W^T against S on the gaussian case: the scheme's own approximation, which the bar 1e-4 |ref| + 1e-4 is
    there to admit, is several new bars away (5.7 for split bf16, 10 for f16mx; asserted: more than 4)"""
    for scheme in ("f16mx", "bf16x3"):
        c = R.Case(scheme, [440, 130], 65, seed=2)
        x, Ws, bs, _, logp = c.network()
        res = c.restate_layer(0, x)
        true = -(x.astype(np.float64) @ Ws[0].astype(np.float64).T + res.bias)
        d = np.abs(true - res.out64)
        assert (d / R.bar(res)).max() > 4.0, (scheme, (d / R.bar(res)).max())
