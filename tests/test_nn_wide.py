"""CPU: the cases of tests/nn_wide_cases.py meet their conditions, and their bars can see what the shapes are for.

tests/test_nn_wide_gpu.py holds the device to bars that are computed, not written (4 x the distance between the restatement with f32
sums and with f64 sums).  A bar is worth what it can tell apart: here a defect of the kind each shape was chosen for is planted in the
RESTATED result -- a strided loop that stops after its first or second trip, frame chunks past the second left out, columns past the
first block left out, two tiles swapped across the diagonal, tile or segment sums past the first 256 left out -- and every one of them
must leave its bar, or move an exact count, on the case meant to catch it.  Nothing here touches the device.
"""
import hashlib

import numpy as np
import pytest

from tests import nn_wide_cases as wc
from tests import nnstep_reference as ns
from tests import nntrain_reference as nr

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------ the cases themselves
def test_the_old_cases_and_networks_did_not_move():
    """the wide networks live outside nr.NETWORKS: the case keys of the two fixtures are what they were"""
    assert sorted(nr.NETWORKS) == ["a", "b"] and nr.NETWORKS["a"] == [24, 40, 33, 50] and nr.NETWORKS["b"] == [7, 130, 129]
    for fn, n, sha in ((nr.gpu_cases, 84, "3143fc799473e56db5bdef9a6a1741a7e21d30a390b549ed198b2eaa7b03c313"),
                       (ns.update_cases, 16, "5d0919b330890cbcbe4c0f45e8eec82901e7e812fc8a8125d8ac58fa1d74a72a"),
                       (ns.stat_cases, 8, "62be16f8340ea32447ebf42a88f854ba86f651ca2ec6fe29cef962a44fbef90c")):
        keys = sorted(fn())
        assert len(keys) == n and hashlib.sha256("\n".join(keys).encode()).hexdigest() == sha, fn.__name__
    # a name and its dimensions give the same network and the same frames
    by_name, by_dims = nr.variant("b", (nr.TANH,), 31, 5, frame_weights=True, pre=True), nr.variant([7, 130, 129], (nr.TANH,), 31, 5, frame_weights=True, pre=True)
    assert all(np.array_equal(p, q) for p, q in zip(by_name[0].Ws + by_name[0].bs + list(by_name[1:]), by_dims[0].Ws + by_dims[0].bs + list(by_dims[1:])))


@pytest.mark.parametrize("key", sorted(wc.CASES))
def test_discrete_results_do_not_depend_on_the_order_of_a_sum(key):
    c = wc.conditions(key)
    print(key, c)
    assert c["min_top2_gap_ulp"] >= 64, c
    assert c["rectified_margin"] >= 1 and c["same_gates"], c
    assert c["same_counts"], c
    a = wc.evaluation(key)
    if not wc.CASES[key].get("options"):     # about half the frames are right: the count can fail in both directions
        assert 0.4 * a["n_observations"] < a["n_classification_errors"] < 0.6 * a["n_observations"]


@pytest.mark.parametrize("key", sorted(wc.STEP_CASES))
def test_the_step_cases_meet_the_same_conditions(key):
    """the group of two mini-batches is compared with the restatement's own gradient: both of its batches (the second is the first
    reversed) keep the margins"""
    ref, x, e, w = wc.step_case(key)
    r32, _, _, _ = wc.step_case(key, "f32")
    margin, same_gates = wc.rectified_margin(ref.net, x, e)
    a, b = ref.step_accumulate(x, e, w), r32.step_accumulate(x, e, w)
    print(key, margin, same_gates, nr.min_top2_gap_ulp(a["softmax"]))
    assert margin >= 1 and same_gates and nr.min_top2_gap_ulp(a["softmax"]) >= 64
    assert a["n_classification_errors"] == b["n_classification_errors"] and a["n_observations"] == wc.STEP_T


def test_the_shapes_reach_what_they_are_for():
    W, D = wc.NETS["W"][0], wc.NETS["D"][0]
    pad = lambda n: (n + 127) // 128      # noqa: E731
    assert [(pad(i), pad(o)) for i, o in zip(W[:-1], W[1:])] == [(3, 1), (1, 3), (3, 6)] and W[0] > 256
    assert (W[-1] + 255) // 256 == 3 and W[-1] % 256 and (D[-1] + 255) // 256 == 5
    assert (pad(W[2]) * 4) * (pad(W[3]) * 4) == 288 and (pad(D[0]) * 4) * (pad(D[1]) * 4) == 1296       # update tiles of 32 x 32
    assert pad(D[0]) * pad(D[1]) * 128 * 128 // 4096 == 324                                              # norm segments
    assert sorted({c["T"] for c in wc.CASES.values()}) == [513, 768, 1000, wc.MAX_FRAMES]
    for i, j in wc.TIE_PAIRS:
        assert i < j < W[-1]
    (a, b), (c, d), (e, f) = wc.TIE_PAIRS
    assert a % 256 == b % 256 and a // 256 != b // 256                             # one thread, two trips
    assert c // 256 == d // 256 == 2 and (c % 256) // 64 != (d % 256) // 64       # two waves of the third trip
    assert e // 256 == 0 and f // 256 == 2 and e % 256 == f % 256                 # trips 0 and 2


# ------------------------------------------------------------------------------------ planted defects: the statistics pass
@pytest.mark.parametrize("key,stop", [("W-T513", 256), ("W-T513", 512), ("D-T513", 256), ("D-T513", 512), ("D-T513", 1024)])
def test_an_output_loop_that_stops_early_is_seen(key, stop):
    """arg-max and error signal over the outputs below `stop` only"""
    net, x, e, w = wc.case(key)
    want, bar, top = wc.evaluation(key), wc.bars(key), len(net.Ws) - 1
    p = want["softmax"]
    errors = int((nr.arg_max(p[:, :stop]) != e).sum())
    assert errors != want["n_classification_errors"]
    E = want["error_signals"][top].copy()
    E[:, stop:] = 0
    layer_input = wc.layer_inputs(net, x, e)[top]
    assert wc.leaves(layer_input.astype(F64).T @ E.astype(F64), want["gradient_weights"][top], bar["gradient_weights/%d" % top])
    assert wc.leaves(E.astype(F64).sum(0), want["gradient_bias"][top], bar["gradient_bias/%d" % top])


@pytest.mark.parametrize("key", ["W-T513", "D-T513"])
def test_frame_chunks_past_the_second_are_seen(key):
    """one frame in the third chunk: without it the gradient, the bias gradient and the feature sums leave their bars"""
    net, x, e, w = wc.case(key)
    want, bar = wc.evaluation(key), wc.bars(key)
    short = nr.accumulate(net, x[:512], e[:512], None, mask=wc.ALL, products="f64")
    got, ref = wc.blocks(short, len(net.Ws)), wc.blocks(want, len(net.Ws))
    for block in ref:
        assert wc.leaves(got[block], ref[block], bar[block]), block
    assert abs(short["objective"] - want["objective"]) > bar["objective"] * abs(want["objective"])


@pytest.mark.parametrize("key", ["W-T513", "D-T513"])
def test_feature_columns_past_the_first_block_are_seen(key):
    want, bar = wc.evaluation(key), wc.bars(key)
    for block in ("feature_sum", "feature_square_sum"):
        got = want[block].copy()
        got[256:] = 0
        assert wc.leaves(got, want[block], bar[block]), block
    top = len(want["gradient_bias"]) - 1
    got = want["gradient_bias"][top].copy()
    got[256:512] = 0      # the bias gradient's second column block
    assert wc.leaves(got, want["gradient_bias"][top], bar["gradient_bias/%d" % top])


def test_two_tiles_swapped_across_the_diagonal_are_seen():
    """W's top layer: a 3 x 6 grid of 128-tiles; tile (0, 1) and tile (1, 0) change places, as a k-tile / n-tile mix-up would have it"""
    want, bar = wc.evaluation("W-T513"), wc.bars("W-T513")
    G = want["gradient_weights"][2].copy()
    G[0:128, 128:256], G[128:256, 0:128] = want["gradient_weights"][2][128:256, 0:128], want["gradient_weights"][2][0:128, 128:256]
    assert wc.leaves(G, want["gradient_weights"][2], bar["gradient_weights/2"])
    # and a stride of the padded rows' (384) in place of the padded columns' (768): every row but the first reads elsewhere
    flat = np.zeros((384, 768), F64)
    flat[:260, :700] = want["gradient_weights"][2]
    other = flat.reshape(-1)[:768 * 384].reshape(768, 384)[:260, :384]
    assert wc.leaves(np.pad(other, ((0, 0), (0, 316))), want["gradient_weights"][2], bar["gradient_weights/2"])


# ------------------------------------------------------------------------------------ planted defects: the step
def restated_group(key):
    """one restated mini-batch of a step case -> (trainer after step_accumulate, finalized G, g, means)"""
    ref, x, e, w = wc.step_case(key)
    ref.step_accumulate(x, e, w)
    G, g, _ = ns.finalize(ref.cfg, ref.G, ref.g, [0.0], ref.n_obs)
    return ref, G, g, ref.means()


def tile_mask(shape, first):
    """the elements of G [in x out] that lie in the first `first` update tiles of 32 x 32 of its padded image, tile rows of `out` tiles"""
    i, o = np.indices(shape)
    return (i // 32) * ((shape[1] + 127) // 128 * 4) + o // 32 < first


def test_tile_sums_past_the_first_256_are_seen():
    """on D (1296 tiles).  W's top layer has 288 tiles too, but its 260 inputs end in tile row 8: the tiles past the first 256 (tile rows
    10 and 11) hold padding alone, so only D can tell"""
    assert not (~tile_mask((260, 700), 256)).any()
    key, l = "D-l1-clip", 0
    ref, G, g, _ = restated_group(key)
    want, bar = float(wc.step_size_parts(ref.cfg, l, G[l], g[l], "f64")), wc.step_bars("D")["step size/0"]
    mask = tile_mask(G[l].shape, 256)
    assert 0 < mask.sum() < mask.size
    got = wc.step_size_parts(ref.cfg, l, np.where(mask, G[l], F32(0)), g[l], "f64")
    print(key, "step size %.9g without the later tiles %.9g bar %.3g" % (want, got, bar))
    assert abs(float(got) - want) > bar * abs(want)


def test_norm_segments_past_the_first_256_are_seen():
    ref, _, _, _ = restated_group("D-l1-clip")
    W, b = ref.net.Ws[0], ref.net.bs[0]
    want, bar = float(ns.regularizer_objective(ref.cfg, [W], [b], ref.n_obs, "f64")), wc.step_bars("D")["regulariser objective"]
    img = wc.padded_transposed_image(W)
    assert img.size // 4096 == 324
    flat = img.reshape(-1).copy()
    flat[256 * 4096:] = 0
    short = flat.reshape(img.shape)[:W.shape[1], :W.shape[0]].T
    got = ns.regularizer_objective(ref.cfg, [short], [b], ref.n_obs, "f64")
    formed = float(F32(ref.criterion + got)) - float(ref.criterion)
    print("regulariser objective %.9g without the later segments %.9g bar %.3g" % (want, formed, bar))
    assert abs(formed - want) > bar * abs(want)


def test_column_partials_past_the_first_eight_tile_rows_are_seen():
    """the bias term with activation statistics, g - G^T m, on W's top layer (260 inputs: nine tile rows of 32, the ninth holds four)"""
    ref, G, g, means = restated_group("W-l2-sgd")
    l, m = 2, means[2]
    assert m is not None and len(m) == 260
    Gu = ns.fma(m[:, None], (-g[l])[None, :], G[l])          # the outer product comes first, as in ns.estimate
    want, bar = ns.delta_bias(Gu, g[l], m, "f64"), wc.step_bars("W")["bias term/2"]
    short = ns.delta_bias(Gu[:256], g[l], m[:256], "f64")
    assert wc.leaves(short, want, bar)
