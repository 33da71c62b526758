"""AMX_PREC_F16MX and AMX_PREC_BF16X3 on the GPU against the exact value of the arithmetic they promise (tests/split_gemm_reference.py),
at a bar set by f32 accumulation -- not by the scheme's approximation, which is what 1e-4 |ref| + 1e-4 against the true product measures.
tests/test_split_gemm_reference.py shows on the CPU that every planted defect of the restatement (a truncated residual, a block
exponent taken per row, cross terms missing in the last K-tile, ...) leaves this bar on every case below.

ONE GEMM PER COMPARISON.  A hidden value that differs from the restatement's by an f32 ulp would be re-quantised differently and bring
scheme-sized differences into the next layer, so no comparison runs through two layers:
  * one-layer networks [K, N]: the scores (features through pack_input_mx / pack_input_bf16x3, weights through the host packer);
  * [K, H, N], first layer: forward_hidden_dev against the restatement of layer 1 with the activation applied.  In f16mx that
    call runs the layer as launch_layer<true> -- the SCORE epilogue of the output-layer instantiation of the chosen tile (MfgS for
    tile = 3 / 11 / 14) followed by neg_act_kernel -- so this comparison exercises pack_input_mx, the host packer and that kernel;
    the hidden-layer instantiations (MfgSP, Mfg64, MfgSL, ...) and their quantising epilogue run inside score() and are checked
    through the next comparison only: a wrong hidden GEMM or a wrong block there shows in the output layer at scheme size;
  * [K, H, N], output layer: the scores against the restatement of the output layer FROM THE KERNEL'S OWN HIDDEN VALUES as
    forward_hidden_dev returned them.  f16mx: forward_hidden_dev sends the last hidden layer through the score epilogue, which stores
    -(acc + bias) in f32, and neg_act_kernel takes activate<ACT>(-x) of that; the hidden epilogue of gemm_mx_kernel takes
    activate<ACT>(acc + bias) in front of lane_pack.  -(-v) is exact, both call the one activate<ACT> template on the same f32 sum
    of the same accumulator (every tile configuration issues the same matrix instructions in the same order), the library is built
    with -ffp-contract=off: the f32 values that lane_pack quantises ARE the returned ones, for every activation -- so all five run.
    Split bf16: the export is hi + lo, exact in f32, but the planes themselves are known only up to one choice: where hi + lo lies
    exactly half way between two bf16 numbers, the kernel's hi (rounded from the f32 value, which is gone) may be either neighbour.
    Per frame the restatement is taken with every combination of those choices (there are rarely more than two such values in a
    frame) and the kernel has to agree with ONE of them in all of the frame's scores;
  * split bf16 keeps 16 significant bits of a hidden value, so its FIRST layer behind the hidden epilogue can be compared only at
    bar + 2^-16 |value| -- the one comparison here that the planted defects do not all leave; the first-layer operands are held to
    the bar through the one-layer networks.  NOT COVERED by any comparison: the hidden epilogue's own rounding of lo.  A truncated
    lo there moves the exported value by at most 2^-17 of itself, inside the coarse bound, and the output layer is restated from
    RNE(hid) and hid - RNE(hid), which agree with such planes;
  * ksplit=4 on [64, 2048, 2048, 40]: layer 2 from the hidden values of the truncated network [64, 2048, 2048], layer 3 from the
    network's own; the split sum's other association is inside the bar by construction (factor 4 on the f32 distance).

THE BAR, per output matrix (split_gemm_reference.bar): |got - S64| <= 4 max|S32 - S64| + 2 ulp_f32(max(|z|, |bias|, |S64|)), both
evaluations of the restatement done on the CPU inside the test, nothing taken from the kernel.  Every test prints worst distance / bar.
One term beyond that formula: a hidden layer with a sigmoid, tanh or ELU adds 4 ulp_f32(output) -- the device's expf / tanhf are not
correctly rounded (1-2 ulp) and up to three more f32 roundings follow them; the sharpness test runs with the term in place.
One family stands at the derived worst case of accumulation instead (f16mx on f16-subnormal magnitudes: Case.bar says why, with the
figures measured under both bars)."""
import itertools

import numpy as np
import pytest

from tests import split_gemm_reference as R

pytestmark = pytest.mark.gpu

CASES = R.gpu_cases()


def _scorer(ctx, case, Ws, bs, acts, logp):
    import rasr_amd
    nn = rasr_amd.NnBatchFeatureScorer(ctx, Ws, bs, acts, log_prior=logp, priori_scale=1.0, precision=case.scheme, tuning=case.tuning or None)
    assert nn.effective_precision()[0] == case.scheme
    return nn


def _hidden(ctx, nn, x):
    import torch
    ctx.use_torch_stream()
    xd = torch.from_numpy(x).cuda()
    hid = torch.full((x.shape[0], nn.hidden_dim), float("nan"), dtype=torch.float32, device="cuda")
    nn.forward_hidden_dev(xd, x.shape[1], x.shape[0], hid)
    torch.cuda.synchronize()
    return hid.cpu().numpy()


def _report(capsys, case, what, ratio):
    with capsys.disabled():
        print("\n%-64s %-22s worst distance / bar = %.3f" % (case.id, what, ratio))


def _bf16x3_output_layer_ratio(case, l, hid, got):
    """worst distance / bar of the output layer, the hidden planes taken as described in the module docstring"""
    u = np.ascontiguousarray(hid, np.float32).view(np.uint32)
    tie = ((u & 0xFFFF) == 0x8000)                                   # exactly half way between two bf16 numbers
    hi0 = R.bf16_round(hid)
    lower = (u & 0xFFFF0000).view(np.float32)
    upper = ((u & 0xFFFF0000) + 0x10000).astype(np.uint32).view(np.float32)
    hi1 = np.where(tie, np.where(hi0 == lower, upper, lower), hi0)   # the other neighbour
    res = case.restate_layer(l, hid, x_split=(hi0, (hid - hi0).astype(np.float32)))
    assert np.array_equal(hi0 + (hid - hi0).astype(np.float32), hid)
    bar = R.bar(res)
    wl = R.split_bf16x3(case.network()[1][l])[1][:, :hid.shape[1]].astype(np.float64)
    worst = 0.0
    for t in range(hid.shape[0]):
        ks = np.flatnonzero(tie[t])
        assert len(ks) <= 10, "frame %d: %d hidden values with an open split" % (t, len(ks))
        delta = (hi1[t, ks].astype(np.float64) - hi0[t, ks])[:, None] * wl[:, ks].T      # what taking the other hi adds to S, per value
        best = np.inf
        for choice in itertools.product((0.0, 1.0), repeat=len(ks)):
            want = res.out64[t] - (np.asarray(choice) @ delta if len(ks) else 0.0)      # scores are -(S + bias)
            best = min(best, float((np.abs(got[t] - want) / bar[t]).max()))
        worst = max(worst, best)
    return worst


@pytest.mark.parametrize("case", [c for c in CASES if len(c.dims) == 2], ids=[c.id for c in CASES if len(c.dims) == 2])
def test_one_layer_scores_equal_the_restatement(ctx, case, capsys):
    x, Ws, bs, acts, logp = case.network()
    got = _scorer(ctx, case, Ws, bs, acts, logp).score(x)
    res = case.restate_layer(0, x)
    ratio = R.distance_over_bar(got, res, case.bar(0, x, res))
    _report(capsys, case, "scores", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("case", [c for c in CASES if len(c.dims) == 3], ids=[c.id for c in CASES if len(c.dims) == 3])
def test_two_layer_network_layer_by_layer(ctx, case, capsys):
    x, Ws, bs, acts, logp = case.network()
    nn = _scorer(ctx, case, Ws, bs, acts, logp)
    hid = _hidden(ctx, nn, x)
    got = nn.score(x)
    assert np.isfinite(hid).all() and np.isfinite(got).all()
    first = case.restate_layer(0, x)
    if case.scheme == "f16mx":
        r0 = R.distance_over_bar(hid, first)
        r1 = R.distance_over_bar(got, case.restate_layer(1, hid))
    else:
        r0 = float((np.abs(hid - first.out64) / (R.bar(first) + 2.0 ** -16 * np.abs(first.out64))).max())   # 16 significant bits: see above
        r1 = _bf16x3_output_layer_ratio(case, 1, hid, got)
    _report(capsys, case, "first layer (hidden)", r0)
    _report(capsys, case, "output layer", r1)
    assert r0 <= 1.0 and r1 <= 1.0, (r0, r1)


@pytest.mark.parametrize("case", [c for c in CASES if len(c.dims) == 4], ids=[c.id for c in CASES if len(c.dims) == 4])
def test_split_k_last_two_layers(ctx, case, capsys):
    x, Ws, bs, acts, logp = case.network()
    nn = _scorer(ctx, case, Ws, bs, acts, logp)
    front = _scorer(ctx, case, Ws[:2], bs[:2], [acts[0], R.ACT_NONE], None)      # its last hidden layer is the network's first
    h1 = _hidden(ctx, front, x)
    h2 = _hidden(ctx, nn, x)
    got = nn.score(x)
    r2 = R.distance_over_bar(h2, case.restate_layer(1, h1))
    r3 = R.distance_over_bar(got, case.restate_layer(2, h2))
    _report(capsys, case, "layer 2 (2048 x 2048)", r2)
    _report(capsys, case, "layer 3 (output)", r3)
    assert r2 <= 1.0 and r3 <= 1.0, (r2, r3)
