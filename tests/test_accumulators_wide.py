"""CPU: the cases of tests/accumulator_wide_cases.py hold what they are for -- measured against the launch shapes the library itself
reports (kernel_shape() of the estimators and of EbwAccumulator) -- and the restatements tell each of them from a planted defect on the
case's own data.  tests/test_accumulators_wide_gpu.py runs the same cases on the device."""
import numpy as np
import pytest

from tests import accumulator_wide_cases as wc
from tests import cmllr_reference as cr
from tests import ebw_reference as er
from tests import mllr_reference as mr


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def cmllr_shape():
    import rasr_amd
    return rasr_amd.AffineFeatureTransformEstimator.kernel_shape()


def mllr_shape():
    import rasr_amd
    return rasr_amd.ModelTransformEstimator.kernel_shape()


def ebw_shape():
    import rasr_amd
    return rasr_amd.EbwAccumulator.kernel_shape()


# ------------------------------------------------------------------------------------------------------------------ CART

@pytest.mark.parametrize("n_labels", wc.CART_LABELS)
def test_cart_labels_outnumber_the_lanes_of_the_scan(n_labels):
    # (the library reports no shape for the scan: DecisionTreeTrainer.kernel_shape() is the split search's.  wc.CART_LANES is a constant)
    c = wc.cart_case(n_labels)
    lab, w = c["labels"], c["weights"]
    per = -(-n_labels // wc.CART_LANES)
    assert (per > 1) == (n_labels > wc.CART_LANES)
    counted = lab[(lab >= 0) & (w != 0.0)]
    seen = np.zeros(n_labels, bool)
    seen[counted] = True
    assert seen[0] and seen[n_labels - 1] and not seen[1] and not seen[n_labels - 2] and 0.2 * n_labels < (~seen).sum() < 0.6 * n_labels
    a, b = wc.CART_RUN
    assert b - a > wc.CART_LANES and (lab[a:b] == c["run_label"]).all() and (w[a:b] != 0).all()
    if per > 1:                                                                   # lanes behind the last label have an empty, clamped share
        busy = -(-n_labels // per)
        assert busy < wc.CART_LANES and (n_labels - 1) // per == busy - 1 and c["run_label"] // per >= busy - 2
    assert (lab == -1).any() and (w == 0).any() and c["cuts"][1] % wc.CART_LANES and c["cuts"][2] % wc.CART_LANES
    for contract in ("off", "fma"):
        want = wc.cart_restate(c, contract)
        assert np.array_equal(want[:, 0] != 0, seen)
        assert not np.array_equal(bits(wc.cart_restate(c, contract, reverse=True)), bits(want))
    assert not np.array_equal(bits(wc.cart_restate(c, "off")), bits(wc.cart_restate(c, "fma")))


# ------------------------------------------------------------------------------------------------------------------ CMLLR

def test_cmllr_wide_triangle():
    stage, cells, comps = cmllr_shape()
    p = wc.cmllr_wide_triangle(stage, False, True, comps)
    lay = cr.layout(p["F"], p["M"], False)
    assert -(-p["M"] // comps) == 2 and p["M"] % comps == 1                       # two z tiles, the second with one component
    assert -(-lay["tri"] // cells) == 129 and lay["tri"] % cells == cells // 2    # the last workgroup of the triangle is half full
    assert lay["R"] * stage * 4 == 32768                                          # the largest stage of xi
    assert list(np.diff(p["frame_offsets"])) == [stage + 1, 7] and list(p["seg_key"]) == [0, 1]
    assert cr.layout(p["F"], p["M"], True)["off_g"] > 37000                       # the small kernel's cells when pooled
    want = wc.cmllr_restate(p, "off")
    size = lay["size"]
    assert want[:size].any() and want[size:].any()
    g_last = want[lay["off_g"] + (p["M"] - 1) * lay["tri"]:size]                  # the lone component of the second tile, the last cell
    assert g_last.all() and want[size - 1] != 0
    assert not np.array_equal(bits(wc.cmllr_restate(p, "off", defects=("lower",))), bits(want))
    q = wc.cmllr_wide_triangle(stage, True, False, comps)
    assert q["weight"] is None and q["best_ld"] == 0 and q["pooled"]
    want = wc.cmllr_restate(q, "off")
    assert len(want) == 2 * cr.layout(q["F"], q["M"], True)["off_g"]
    assert not np.array_equal(bits(wc.cmllr_restate(q, "off", defects=("lower",))), bits(want))


def test_cmllr_tile_edges():
    stage, cells, comps = cmllr_shape()
    wide = wc.CMLLR_WIDE_TILE
    for tile, Ms in ((wide, (wide, wide + 1, wide + 2)), (comps, (2 * comps, 2 * comps + 1))):
        assert [-(-M // tile) for M in Ms] == ([1, 2, 2] if tile == wide else [2, 3])
        for M in Ms:
            p = wc.cmllr_tile_edge(stage, M, True)
            n = int(p["frame_offsets"][-1])
            assert n // stage == 2 and 0 < n % stage < stage and len(p["seg_key"]) == 1
            assert cr.layout(64, M, False)["tri"] > 8 * cells
            want = wc.cmllr_restate(p, "fma")
            assert not np.array_equal(bits(wc.cmllr_restate(p, "fma", defects=("lower",))), bits(want))
            assert not np.array_equal(bits(wc.cmllr_restate(p, "off")), bits(want))


def test_cmllr_many_keys():
    p = wc.cmllr_many_keys()
    keys, lens = p["seg_key"], np.diff(p["frame_offsets"])
    assert p["n_keys"] == 300 and len(keys) == 300 and lens.min() == 0 and lens.max() == 3 and (lens == 0).sum() > 30
    used = set(int(k) for k, n in zip(keys, lens) if n)
    assert {0, 299} <= used and len(used) < 60
    assert (np.diff(keys) < 0).sum() > 100                                        # the key order is interleaved
    assert [int(n) for k, n in zip(keys, lens) if k == 7] == [3, 1]
    want = wc.cmllr_restate(p, "fma")
    size = cr.layout(5, 5, False)["size"]
    filled = {k for k in range(300) if want[k * size:(k + 1) * size].any()}
    assert filled <= used and {0, 299, 7} <= filled
    assert not np.array_equal(bits(wc.cmllr_restate(p, "fma", defects=("segment_sorted",))), bits(want))
    cut = wc.cut_inside(p, 150)
    assert cut[0][0][-1] == cut[1][0][0] and lens[150] == 3


def test_cmllr_padded_matrix():
    p = wc.cmllr_padded_matrix()
    n_mix = len(p["model"]["mix_offsets"]) - 1
    assert p["best_ld"] == n_mix + 3 and p["best"].shape[1] == p["best_ld"] and (p["best"][:, n_mix:] == 0).all()
    want = wc.cmllr_restate(p, "off")
    assert not np.array_equal(bits(wc.cmllr_restate(p, "off", defects=("lower",))), bits(want))
    narrow = dict(p, best=np.ascontiguousarray(p["best"][:, :n_mix]), best_ld=n_mix)
    assert np.array_equal(bits(wc.cmllr_restate(narrow, "off")), bits(want))      # the padding is never read
    # planted: the matrix read with the leading dimension n_mix.  Rows 1 and later then start in the row before: other densities
    T = len(p["best"])
    ks = np.diff(p["model"]["mix_offsets"].astype(np.int64))
    misread = np.minimum(p["best"].reshape(-1)[:T * n_mix].reshape(T, n_mix), ks[None, :] - 1).astype(np.uint32)   # (kept inside the mixtures)
    assert not np.array_equal(bits(wc.cmllr_restate(dict(p, best=misread, best_ld=n_mix), "off")), bits(want))


def test_cmllr_apply_case():
    c = wc.cmllr_apply_case()
    off, lens = c["frame_offsets"], c["lens"]
    assert c["M"] > wc.ROW_STRIDE and c["F"] >= c["M"] and c["out_ld"] > c["M"]
    assert off[0] == 5 and len(lens) == 500 and lens.max() == 3
    assert (lens[:6] == 0).all() and (lens[240:252] == 0).all() and (lens[-5:] == 0).all() and lens[6:240].any()
    assert len(c["feats"]) > off[-1] and list(c["has"]) == [1, 0, 1] and set(c["seg_key"][lens > 0]) == {0, 1, 2}
    want, n_id = cr.apply(c["transforms"], c["has"], c["feats"], off, c["seg_key"], c["M"], c["F"], "off")
    assert n_id == int((c["seg_key"] == 1).sum())
    fused, _ = cr.apply(c["transforms"], c["has"], c["feats"], off, c["seg_key"], c["M"], c["F"], "fma")
    assert not np.array_equal(want.view(np.uint32), fused.view(np.uint32))
    # planted: the segment found one too far to the left
    shifted, _ = cr.apply(c["transforms"], c["has"], c["feats"], off, np.roll(c["seg_key"], 1), c["M"], c["F"], "off")
    assert not np.array_equal(want.view(np.uint32), shifted.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ MLLR

@pytest.mark.parametrize("weighted", [True, False])
def test_mllr_long_segment(weighted):
    stage, chunk = mllr_shape()
    p = wc.mllr_long_segment(chunk, weighted)
    off = p["frame_offsets"]
    assert list(np.diff(off)) == [700, 40, 300] and list(p["seg_key"]) == [0, 1, 0] and off[1] > 2 * chunk
    leaf1 = wc.mllr_leaf_frames(p, 0, 1)
    assert {chunk - 1, chunk, 2 * chunk - 1, 2 * chunk} <= set(leaf1)             # the cursor is carried across both chunk boundaries
    assert sum(t >= off[2] for t in leaf1) > 20 and not any(off[1] <= t < off[2] for t in leaf1)   # ... and into the key's next segment
    assert len(wc.mllr_leaf_frames(p, 1, 1)) > 0 and len(leaf1) > 2 * stage
    assert off[0] < p["cut"] < off[1] and p["cut"] % chunk
    for mode in (mr.FULL, mr.SHIFT):
        ls = mr.leaf_size(mode, p["D"])
        want = wc.mllr_restate(p, mode, "off").reshape(2, 4, ls)
        assert want[0, 1].any() and want[1].any() and not want[:, 2].any()
        if mode == mr.FULL:
            assert want[0, 1, 0] == len(leaf1)
        assert not np.array_equal(bits(wc.mllr_restate(p, mode, "off", defect="out_of_order")), bits(want))


def test_mllr_many_leafs():
    stage, chunk = mllr_shape()
    p = wc.mllr_many_leafs()
    assert p["n_leafs"] == 300 > chunk and p["n_mix"] == 400
    for mode in (mr.FULL, mr.SHIFT):
        ls = mr.leaf_size(mode, p["D"])
        want = wc.mllr_restate(p, mode, "off").reshape(2, 300, ls)
        fed = want.reshape(2, 300, -1).any(axis=2).any(axis=0)
        assert fed[299] and fed[chunk:].sum() > 10 and not fed[100:140].any() and fed[:100].sum() > 50
        assert not np.array_equal(bits(wc.mllr_restate(p, mode, "off", defect="out_of_order")), bits(want))


def test_mllr_wide_cases():
    import rasr_amd
    stage, cells = mllr_shape()
    host = lambda mode, D: rasr_amd.ModelTransformEstimator(None, mode, 2, [0, 1, 1, 0], dim=D)   # noqa: E731
    assert host("full", 255).leaf_size() == mr.leaf_size(mr.FULL, 255) and mr.leaf_size(mr.FULL, 255) % cells == 2   # two live lanes
    with pytest.raises(rasr_amd.AmxError):
        host("full", 256)                                                         # 255 is the widest model
    assert -(-mr.leaf_size(mr.SHIFT, 200) // cells) == 2
    assert stage * 255 * 4 * 3 == 48960                                           # the shift estimator's x, mean and variance of a stage
    for mode, D, weighted in ((mr.FULL, 255, True), (mr.SHIFT, 200, True), (mr.SHIFT, 255, False)):
        p = wc.mllr_wide(D, weighted)
        lens = [len(wc.mllr_leaf_frames(p, 0, l)) for l in (0, 1)]
        assert 50 < sum(lens) <= 61 and min(lens) > stage
        want = wc.mllr_restate(p, mode, "off")
        assert want[-1] != 0                                                      # the last live lane's cell
        assert not np.array_equal(bits(wc.mllr_restate(p, mode, "off", defect="out_of_order")), bits(want))
        if mode == mr.FULL:
            assert not np.array_equal(bits(wc.mllr_restate(p, mode, "fma")), bits(want))


def test_mllr_adapt_case():
    p = wc.mllr_adapt_case()
    n_mean = len(p["model"]["means"])
    assert p["D"] > wc.ROW_STRIDE and n_mean >= 300 and (np.diff(p["model"]["mix_offsets"].astype(np.int64)) == 3).all()
    assert list(np.diff(p["frame_offsets"])) == [380, 7]
    s = p["synthetic"]
    for mode, name in ((mr.FULL, "full"), (mr.SHIFT, "shift")):
        want = mr.adapt_means(p["model"], mode, s["matrix_ids"], s[name], s["matrix_of_mixture"], "off")
        assert not np.array_equal(want, p["model"]["means"])
        other = mr.adapt_means(p["model"], mode, s["matrix_ids"], s[name], np.roll(s["matrix_of_mixture"], 1), "off")   # planted: the neighbour's matrix
        assert not np.array_equal(want.view(np.uint32), other.view(np.uint32))
        # (the two contracts differ in the last bits of an f64 chain that is narrowed to f32 once: no planted defect, both are run)
    unit = np.stack([mr.unit_matrix(mr.FULL, p["D"])] * len(s["matrix_ids"]))
    assert np.array_equal(mr.adapt_means(p["model"], mr.FULL, s["matrix_ids"], unit, s["matrix_of_mixture"], "off"), p["model"]["means"])


# ------------------------------------------------------------------------------------------------------------------ EBW

def ebw_checks(c, want_shape):
    """the case's plan against what it is for, and the reversed key order against the restatement; returns the plan"""
    block, stage, threads = ebw_shape()
    keys = er.collect(c["frame_offsets"], *c["lattice"])
    plan = wc.ebw_expected_shape(c, block, len(keys))
    for k, v in want_shape.items():
        assert plan[k] == v, (k, plan[k], v)
    T = c["feats"].shape[0]
    best = np.zeros((T, c["n_mix"]), np.uint32)                                   # every key on its mixture's first density
    want, _ = wc.ebw_restate(c, best, "off")
    rev, _ = wc.ebw_restate(c, best, "off", order=er.key_order(keys, "device")[::-1])
    assert not np.array_equal(bits(rev), bits(want))
    assert np.any(np.abs(c["lattice"][1]) == er.EPSILON)
    sides = {k["side"] for k in keys}
    assert sides == {er.NUM, er.DEN}
    return plan, keys


def test_ebw_big_sort():
    block, stage, threads = ebw_shape()
    c = wc.ebw_big_sort()
    n_items = int(c["lattice"][2][-1])
    assert n_items == 18000 and c["D"] == 39 and len(c["frame_offsets"]) == 2
    plan, keys = ebw_checks(c, dict(item_sort_passes=3, item_blocks=9, item_table_recursed=True))
    assert 256 * plan["item_blocks"] > block and len(keys) > 256 * 8
    w = c["lattice"][1]
    assert len(np.unique(np.frexp(np.abs(w[np.abs(w) > 1e-6]))[1])) >= 20
    per_list = {}
    for k in keys:
        per_list[k["mixture"], k["side"]] = per_list.get((k["mixture"], k["side"]), 0) + 1
    assert max(per_list.values()) > 2 * stage                                     # chains of several stages


@pytest.mark.parametrize("n_items", [2047, 2048, 4096])
def test_ebw_item_counts_at_the_block(n_items):
    block, stage, threads = ebw_shape()
    c = wc.ebw_item_count(n_items)
    assert int(c["lattice"][2][-1]) == n_items and (n_items + 1) % block in (0, 1)
    plan, _ = ebw_checks(c, dict(item_blocks=-(-n_items // block), item_table_recursed=False))
    assert -(-(n_items + 1) // block) == plan["item_blocks"] + (n_items % block == 0)   # the extra element of the heads sits alone in a block


def test_ebw_long_corpus():
    c = wc.ebw_long_corpus()
    n = int(c["frame_offsets"][-1] - c["frame_offsets"][0])
    assert n == 600000 and c["D"] == 2 and 2000 < int(c["lattice"][2][-1]) < 5000
    assert wc.ebw_code_bits(c) == (20, 3, 25)
    ebw_checks(c, dict(item_sort_passes=4))
    seg_of_arc = np.searchsorted(c["lattice"][0], np.arange(len(c["lattice"][1])), side="right") - 1
    fr = c["frame_offsets"][seg_of_arc[np.searchsorted(c["lattice"][2], np.arange(len(c["lattice"][3])), side="right") - 1]] + c["lattice"][3]
    assert fr.max() >= 1 << 19 and fr.min() < 1 << 16                             # the top frame bit is used, and low frames too


@pytest.mark.parametrize("pooled", [False, True])
def test_ebw_many_lists(pooled):
    c = wc.ebw_many_lists(pooled)
    n_lists, list_bits = wc.ebw_list_bits(c["model"])
    assert c["n_mix"] == 40 and 90 <= int(c["model"]["mix_offsets"][-1]) <= 110 and n_lists > 128 and wc.ebw_code_bits(c)[1] == 6
    assert c["model"]["variances"].shape[0] == (1 if pooled else int(c["model"]["mix_offsets"][-1]))
    ebw_checks(c, dict(list_sort_passes=2))


@pytest.mark.parametrize("D", [256, 300])
def test_ebw_wide_rows(D):
    block, stage, threads = ebw_shape()
    c = wc.ebw_wide_rows(D)
    assert -(-(1 + D) // threads) == 2 and (D != 256 or (1 + D) % threads == 1)
    ebw_checks(c, {})
    best = np.zeros((c["feats"].shape[0], c["n_mix"]), np.uint32)
    want, _ = wc.ebw_restate(c, best, "off")
    o = er.layout(c["model"])
    sums = want[o["num_mean_sums"]:o["num_cov_weights"]].reshape(-1, D)
    assert sums[:, D - 1].any()                                                   # the second workgroup's last live lane has work
    assert not np.array_equal(bits(wc.ebw_restate(c, best, "fma")[0]), bits(want))
