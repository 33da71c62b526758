"""GPU parity where the launches of cart.hip, cmllr.hip, mllr.hip and ebw.hip split: the cases of tests/accumulator_wide_cases.py (which
tests/test_accumulators_wide.py holds to their purpose) against the restatements of tests/cart_reference.py, cmllr_reference.py,
mllr_reference.py and ebw_reference.py.  Every comparison is bit equality: the f64 of the accumulators as uint64, the f32 of the applied
features and the adapted means as uint32.  The EBW cases also assert, through amx_ebw_last_shape, that the device went where the case
aims."""
import numpy as np
import pytest

from tests import accumulator_wide_cases as wc
from tests import cmllr_reference as cr
from tests import ebw_reference as er
from tests import mllr_reference as mr

pytestmark = pytest.mark.gpu

FILL = -7.0


@pytest.fixture()
def cctx(ctx):
    """the session context on torch's stream, handed out in contract=off and restored to it"""
    ctx.use_torch_stream()
    ctx.set_contract("off")
    yield ctx
    ctx.set_contract("off")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, want):
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]


# ------------------------------------------------------------------------------------------------------------------ CART

@pytest.mark.parametrize("weights,contract", [(True, "fma"), (True, "off"), (False, "off")])
@pytest.mark.parametrize("n_labels", wc.CART_LABELS)
def test_cart_accumulation_with_more_labels_than_lanes(cctx, n_labels, weights, contract):
    import torch

    import rasr_amd
    c = wc.cart_case(n_labels, weights=weights)
    want = wc.cart_restate(c, contract)
    assert want[0, 0] != 0 and want[n_labels - 1, 0] != 0 and want[1, 0] == 0 and want[c["run_label"], 0] != 0
    cctx.set_contract(contract)
    xd, ld = torch.from_numpy(c["feats"]).cuda(), torch.from_numpy(c["labels"]).cuda()
    wd = torch.from_numpy(c["weights"]).cuda() if weights else None
    one = rasr_amd.CartExampleAccumulator(cctx, n_labels, c["dim"])
    one.accumulate(xd, ld, wd)
    same(one.rows(), want)
    three = rasr_amd.CartExampleAccumulator(cctx, n_labels, c["dim"])
    for a, b in zip(c["cuts"], c["cuts"][1:]):
        three.accumulate(xd[a:b], ld[a:b], wd[a:b] if wd is not None else None)
    same(three.rows(), want)
    ids, n_obs, values = one.examples()
    assert list(ids) == [i for i in range(n_labels) if want[i, 0] != 0]
    same(n_obs, want[ids, 0])
    same(values, want[ids, 1:])


# ------------------------------------------------------------------------------------------------------------------ CMLLR

def cmllr_shape():
    import rasr_amd
    return rasr_amd.AffineFeatureTransformEstimator.kernel_shape()


def cmllr_device(cctx, p, pieces, contract, tile=None):
    import torch

    import rasr_amd
    cctx.set_contract(contract)
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    est = rasr_amd.AffineFeatureTransformEstimator(gmm, p["F"], p["n_keys"])
    if tile is not None:
        est.set_tile(tile)
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    xd, ed = torch.from_numpy(p["feats"]).cuda(), torch.from_numpy(p["emission"]).cuda()
    bd = torch.from_numpy(np.ascontiguousarray(p["best"]).view(np.int32)).cuda()
    wd = torch.from_numpy(p["weight"]).cuda() if p["weight"] is not None else None
    for off, keys in pieces:
        est.accumulate_dev(xd, p["F"], off, keys, ed, bd, acc, p["best_ld"], wd)
    torch.cuda.synchronize()
    assert est.pooled == p["pooled"] and est.key_size() == cr.layout(p["F"], p["M"], p["pooled"])["size"]
    return acc.cpu().numpy()


def whole(p):
    return [(p["frame_offsets"], p["seg_key"])]


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("weighted,contract", [(True, "fma"), (False, "off")])
def test_cmllr_triangle_of_129_workgroups_and_a_tile_of_one_component(cctx, weighted, contract, pooled):
    stage, cells, comps = cmllr_shape()
    p = wc.cmllr_wide_triangle(stage, pooled, weighted, comps)
    want = wc.cmllr_restate(p, contract)
    same(cmllr_device(cctx, p, whole(p), contract), want)
    same(cmllr_device(cctx, p, wc.cut_inside(p, 0), contract), want)


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("tile,M", [(48, 48), (48, 49), (48, 50), (16, 32), (16, 33)])
def test_cmllr_model_dimensions_around_a_tile(cctx, tile, M, contract):
    stage, cells, comps = cmllr_shape()
    assert tile in (comps, wc.CMLLR_WIDE_TILE)
    for weighted in (True, False):
        p = wc.cmllr_tile_edge(stage, M, weighted)
        same(cmllr_device(cctx, p, whole(p), contract, tile=tile), wc.cmllr_restate(p, contract))


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_cmllr_three_hundred_keys_in_interleaved_order(cctx, contract):
    for weighted in (True, False):
        p = wc.cmllr_many_keys(weighted)
        want = wc.cmllr_restate(p, contract)
        same(cmllr_device(cctx, p, whole(p), contract), want)
        same(cmllr_device(cctx, p, wc.cut_inside(p, 150), contract), want)


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_cmllr_best_densities_in_a_padded_matrix(cctx, contract):
    p = wc.cmllr_padded_matrix()
    want = wc.cmllr_restate(p, contract)
    same(cmllr_device(cctx, p, whole(p), contract), want)
    same(cmllr_device(cctx, p, wc.cut_inside(p, 0), contract), want)


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_cmllr_apply_over_five_hundred_short_segments(cctx, contract):
    import torch

    import rasr_amd
    c = wc.cmllr_apply_case()
    M, F, off = c["M"], c["F"], c["frame_offsets"]
    cctx.set_contract(contract)
    T = len(c["feats"])
    out = torch.full((T, c["out_ld"]), FILL, dtype=torch.float32, device="cuda")
    tr = rasr_amd.AffineFeatureTransform(cctx, M, F, c["n_keys"])
    n_id = tr.apply_dev(torch.from_numpy(c["transforms"]).cuda(), c["has"], off, c["seg_key"], torch.from_numpy(c["feats"]).cuda(), F, out, c["out_ld"])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want, want_id = cr.apply(c["transforms"], c["has"], c["feats"], off, c["seg_key"], M, F, contract)
    a, b = int(off[0]), int(off[-1])
    assert n_id == want_id
    assert np.array_equal(got[a:b, :M].view(np.uint32), want[a:b].view(np.uint32)), np.argwhere(got[a:b, :M] != want[a:b])[:5]
    assert (got[:a] == FILL).all() and (got[b:] == FILL).all() and (got[:, M:] == FILL).all()


# ------------------------------------------------------------------------------------------------------------------ MLLR

MODES = {"full": mr.FULL, "shift": mr.SHIFT}


def mllr_shape():
    import rasr_amd
    return rasr_amd.ModelTransformEstimator.kernel_shape()


def mllr_device(cctx, p, mode, pieces, contract):
    """(scorer, estimator, the flat buffer) after the calls `pieces`"""
    import torch

    import rasr_amd
    cctx.set_contract(contract)
    gmm = rasr_amd.GmmFeatureScorer(cctx, p["model"])
    est = rasr_amd.ModelTransformEstimator(gmm, mode, p["n_leafs"], p["leaf_of_mixture"], n_keys=p["n_keys"])
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    xd, ed = torch.from_numpy(p["feats"]).cuda(), torch.from_numpy(p["emission"]).cuda()
    bd = torch.from_numpy(np.ascontiguousarray(p["best"]).view(np.int32)).cuda()
    wd = torch.from_numpy(p["weight"]).cuda() if p["weight"] is not None else None
    for off, keys in pieces:
        est.accumulate_dev(xd, p["D"], off, keys, ed, bd, acc, p["best_ld"], wd)
    torch.cuda.synchronize()
    assert est.leaf_size() == mr.leaf_size(MODES[mode], p["D"])
    return gmm, est, acc.cpu().numpy()


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("mode", ["full", "shift"])
def test_mllr_a_leaf_cursor_carried_across_chunks_and_segments(cctx, mode, weighted, contract):
    stage, chunk = mllr_shape()
    p = wc.mllr_long_segment(chunk, weighted)
    want = wc.mllr_restate(p, MODES[mode], contract)
    same(mllr_device(cctx, p, mode, whole(p), contract)[2], want)
    same(mllr_device(cctx, p, mode, wc.mllr_two_calls(p), contract)[2], want)


@pytest.mark.parametrize("mode,weighted,contract", [("full", True, "fma"), ("full", False, "off"), ("shift", True, "off"), ("shift", False, "fma")])
def test_mllr_three_hundred_leaves(cctx, mode, weighted, contract):
    p = wc.mllr_many_leafs(weighted)
    same(mllr_device(cctx, p, mode, whole(p), contract)[2], wc.mllr_restate(p, MODES[mode], contract))


@pytest.mark.parametrize("mode,D,weighted,contract", [("full", 255, True, "fma"), ("shift", 200, True, "off"), ("shift", 200, False, "fma"),
                                                      ("shift", 255, True, "fma"), ("shift", 255, False, "off")])
def test_mllr_widest_models(cctx, mode, D, weighted, contract):
    p = wc.mllr_wide(D, weighted)
    same(mllr_device(cctx, p, mode, whole(p), contract)[2], wc.mllr_restate(p, MODES[mode], contract))


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("mode", ["full", "shift"])
def test_mllr_adapted_means_of_three_hundred_means_in_seventy_dimensions(cctx, mode, contract):
    import torch

    import rasr_amd
    p = wc.mllr_adapt_case()
    D, n_mean = p["D"], len(p["model"]["means"])
    gmm, est, acc = mllr_device(cctx, p, mode, whole(p), contract)
    same(acc, wc.mllr_restate(p, MODES[mode], contract))
    adaptor = rasr_amd.MixtureSetAdaptor(est)

    def adapted(ids, mats, of_mix):
        out = torch.full((n_mean + 1, D), FILL, dtype=torch.float32, device="cuda")
        adaptor.adapt_means_dev(ids, mats, of_mix, out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = mr.adapt_means(p["model"], MODES[mode], ids, mats, of_mix, contract)
        assert np.array_equal(got[:n_mean].view(np.uint32), want.view(np.uint32)), np.argwhere(got[:n_mean] != want)[:5]
        assert (got[n_mean] == FILL).all()
        return want

    seen = []
    for key in (0, 1):   # key 1 has 7 frames: the root-only fallback and the silence fallback, which copy the means
        e = est.estimate(acc, p["tree"], key, min_observation=30.0, min_silence_observation=5.0)
        seen.append((e["root_fallback"], e["silence_fallback"]))
        want = adapted(e["matrix_ids"], e["matrices"], e["matrix_of_mixture"])
        assert np.array_equal(want, p["model"]["means"]) == (key == 1)
    assert seen == [(False, False), (True, True)]
    s = p["synthetic"]
    adapted(s["matrix_ids"], s[mode], s["matrix_of_mixture"])


# ------------------------------------------------------------------------------------------------------------------ EBW

def ebw_device(cctx, c, contract):
    """(accumulator, buffer, best densities [rows, n_mix]) after one call"""
    import torch

    import rasr_amd
    cctx.set_contract(contract)
    gmm = rasr_amd.GmmFeatureScorer(cctx, c["model"])
    ebw = rasr_amd.EbwAccumulator(gmm)
    feats = c["feats"]
    xd = torch.from_numpy(feats).cuda()
    acc = torch.zeros(ebw.accumulator_size(), dtype=torch.float64, device="cuda")
    ebw.accumulate_dev(xd, feats.shape[1], c["frame_offsets"], *c["lattice"], acc)
    torch.cuda.synchronize()
    dense = torch.from_numpy(np.ascontiguousarray(feats[:, :c["D"]])).cuda()
    T = dense.shape[0]
    scores = torch.zeros((T, c["n_mix"]), dtype=torch.float32, device="cuda")
    best = torch.zeros((T, c["n_mix"]), dtype=torch.int32, device="cuda")
    gmm.score_dev(dense, T, scores, best)
    torch.cuda.synchronize()
    return ebw, acc.cpu().numpy(), best.cpu().numpy().view(np.uint32)


def ebw_run(cctx, c, contract, aims):
    """the buffer, the keys and the shape of the call against the restatement and the case's plan; `aims`: what the call must have run"""
    import rasr_amd
    ebw, got, best = ebw_device(cctx, c, contract)
    want, keys = wc.ebw_restate(c, best, contract)
    o = er.layout(c["model"])
    assert ebw.accumulator_size() == o["size"]
    same(got, want)
    assert want[:o["den_density_weights"]].any() and want[o["den_density_weights"]:o["objective"]].any()
    lk = ebw.last_keys()
    ordered = [keys[i] for i in er.key_order(keys, "device")]
    assert len(lk["frame"]) == len(ordered)
    for name in ("frame", "mixture", "side"):
        assert np.array_equal(lk[name], [k[name] for k in ordered]), name
    same(lk["weight"], [k["weight"] for k in ordered])
    shape = ebw.last_shape()
    assert shape == wc.ebw_expected_shape(c, rasr_amd.EbwAccumulator.kernel_shape()[0], len(keys)), shape
    for k, v in aims.items():
        assert shape[k] == v, (k, shape)
    return shape


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_ebw_nine_sort_blocks_three_passes_and_a_recursive_table_scan(cctx, contract):
    ebw_run(cctx, wc.ebw_big_sort(), contract, dict(item_sort_passes=3, item_blocks=9, item_table_recursed=True))


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("n_items", [2047, 2048, 4096])
def test_ebw_item_counts_at_the_edges_of_a_block(cctx, n_items, contract):
    import rasr_amd
    block = rasr_amd.EbwAccumulator.kernel_shape()[0]
    ebw_run(cctx, wc.ebw_item_count(n_items), contract, dict(item_blocks=-(-n_items // block), item_table_recursed=False))


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_ebw_four_item_passes_over_six_hundred_thousand_frames(cctx, contract):
    ebw_run(cctx, wc.ebw_long_corpus(), contract, dict(item_sort_passes=4))


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("pooled", [False, True])
def test_ebw_two_list_passes_and_six_bits_of_mixture(cctx, pooled, contract):
    ebw_run(cctx, wc.ebw_many_lists(pooled), contract, dict(list_sort_passes=2))


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("D", [256, 300])
def test_ebw_chains_of_two_workgroups(cctx, D, contract):
    ebw_run(cctx, wc.ebw_wide_rows(D), contract, {})


def test_ebw_last_shape_of_a_call_that_ends_early(cctx):
    import torch

    import rasr_amd
    c = wc.ebw_item_count(2047)
    gmm = rasr_amd.GmmFeatureScorer(cctx, c["model"])
    ebw = rasr_amd.EbwAccumulator(gmm)
    xd = torch.from_numpy(c["feats"]).cuda()
    acc = torch.zeros(ebw.accumulator_size(), dtype=torch.float64, device="cuda")
    ebw.accumulate_dev(xd, c["feats"].shape[1], c["frame_offsets"], *c["lattice"], acc)
    assert ebw.last_shape()["item_sort_passes"] > 0
    none = (np.array([0, 0], np.int64), np.zeros(0, np.float32), np.array([0], np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    ebw.accumulate_dev(xd, c["feats"].shape[1], c["frame_offsets"], *none, acc)
    assert not any(ebw.last_shape().values()) and len(ebw.last_keys()["frame"]) == 0
    # a refused call leaves no shape of the call before it either
    ebw.accumulate_dev(xd, c["feats"].shape[1], c["frame_offsets"], *c["lattice"], acc)
    assert ebw.last_shape()["item_sort_passes"] > 0
    with pytest.raises(rasr_amd.AmxError, match="feats_ld"):
        ebw.accumulate_dev(xd, c["D"] - 1, c["frame_offsets"], *c["lattice"], acc)
    assert not any(ebw.last_shape().values())
