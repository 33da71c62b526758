"""Inputs that take the CART, CMLLR, MLLR and EBW accumulators where their launches split: more labels than lanes of the scan, a triangle
and a model wider than one workgroup's share, segments and lists longer than a chunk, sorts of three and four passes, a digit table the
scan has to recurse on.  Pure numpy, deterministic; tests/test_accumulators_wide.py holds every case to what it is for (against the
launch shapes the library reports) and tests/test_accumulators_wide_gpu.py runs them against the restatements, bit for bit.

Every builder returns a dict; the helpers *_restate call the restatement modules with the case's own data."""
import numpy as np

from tests import cart_reference as cart_ref
from tests import cmllr_reference as cmllr_ref
from tests import ebw_reference as ebw_ref
from tests import mllr_reference as mllr_ref
from tests import synth

# Constants of the kernels that no getter of the library reports, copied here from the issue's description of the kernels: the lanes of
# cart_scan_kernel and of a step of cart_place_kernel, and the rows (grid y) over which cmllr_apply_kernel and mllr_adapt_kernel stride.
# If a kernel changes them, the cases built on them no longer aim where they say and nothing here notices
CART_LANES = 256
ROW_STRIDE = 64
CMLLR_WIDE_TILE = 48          # the argument of set_tile


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def offsets(lens, first=0):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + first


# ------------------------------------------------------------------------------------------------------------------ CART

CART_LABELS = (256, 257, 1000)
CART_RUN = (1000, 1300)       # frames of one label in a row


def cart_case(n_labels, T=3000, dim=8, weights=True, seed=0):
    """features, labels, weights: labels 0 and n_labels - 1 present, about a third of the labels absent (1 and n_labels - 2 among them),
    the label `run_label` (in the share of one of the scan's last two busy lanes) owns the frames CART_RUN, some frames carry -1, some weights 0"""
    rng = _rng(1000 + n_labels + seed)
    x = (rng.standard_normal((T, dim)) * 3 + 1).astype(np.float32)
    present = rng.random(n_labels) < 0.65
    present[[0, n_labels - 1, n_labels - 3]] = True
    present[[1, n_labels - 2]] = False
    pool = np.flatnonzero(present)
    lab = pool[rng.integers(0, len(pool), T)].astype(np.int32)
    skipped = rng.random(T) < 0.03
    lab[skipped] = -1
    run_label = n_labels - 3
    lab[CART_RUN[0]:CART_RUN[1]] = run_label
    lab[5], lab[T - 3] = 0, n_labels - 1
    w = None
    if weights:
        w = rng.uniform(0.01, 2.0, T)
        w[rng.random(T) < 0.05] = 0.0
        w[CART_RUN[0]:CART_RUN[1]] = rng.uniform(0.01, 2.0, CART_RUN[1] - CART_RUN[0])
        w[5], w[T - 3] = 0.75, 1.25
    return dict(n_labels=n_labels, dim=dim, T=T, feats=x, labels=lab, weights=w, run_label=run_label, cuts=[0, T // 3, T // 3 + 777, T])


def cart_restate(c, contract, reverse=False):
    """reverse: the planted defect -- the frames added last to first"""
    x, lab, w = c["feats"], c["labels"], c["weights"]
    if reverse:
        x, lab, w = x[::-1], lab[::-1], (None if w is None else w[::-1])
    return cart_ref.accumulate(cart_ref.accumulator(c["n_labels"], c["dim"]), x, lab, w, contract=contract)


# ------------------------------------------------------------------------------------------------------------------ CMLLR

def cmllr_case(F, M, lens, keys, n_keys, seed, pooled=False, weighted=True, matrix=True, best_pad=0, n_mix=4, first=0):
    """a model, frames, a segment table and an alignment as tests/test_cmllr_gpu.py's problem(), with the number of keys, the leading
    dimension of the best-density matrix (n_mix + best_pad) and the first frame of the table free"""
    rng = _rng(seed)
    model = synth.gmm_cart(n_mix, 1, 3, M, seed=seed, pooled=pooled)
    off = offsets(lens, first)
    T = int(off[-1])
    feats = (rng.standard_normal((T, F)) * 1.5 + 0.5).astype(np.float32)
    emission = rng.integers(0, n_mix, T).astype(np.int32)
    if T > 2:
        emission[rng.random(T) < 0.1] = -1
        emission[first + 1] = -1
    ks = np.diff(model["mix_offsets"].astype(np.int64))
    if matrix:
        best = np.zeros((T, n_mix + best_pad), np.uint32)                     # the padding columns name density 0, which every mixture has
        best[:, :n_mix] = np.stack([rng.integers(0, ks[m], T) for m in range(n_mix)], axis=1)
    else:
        best = np.array([rng.integers(0, ks[e]) if e >= 0 else 0xFFFFFFFF for e in emission], np.uint32)
    weight = None
    if weighted:
        weight = rng.uniform(0.05, 2.0, T)
        weight[rng.random(T) < 0.1] = 0.0
        weight[first] = 0.0
    return dict(model=model, F=F, M=M, n_keys=n_keys, feats=feats, frame_offsets=off, seg_key=np.array(keys, np.int32), emission=emission, best=best,
                weight=weight, best_ld=(n_mix + best_pad) if matrix else 0, pooled=pooled)


def cmllr_restate(p, contract, off=None, defects=()):
    return cmllr_ref.accumulate(p["model"], p["F"], p["n_keys"], p["feats"], p["frame_offsets"] if off is None else off, p["seg_key"], p["emission"],
                                p["best"], p["best_ld"], p["weight"], None, contract, defects)


def cut_inside(p, s):
    """the segment table as two calls, cut at a frame inside segment s"""
    off = p["frame_offsets"]
    cut = int(off[s] + (off[s + 1] - off[s] + 1) // 2)
    assert off[s] < cut < off[s + 1]
    return [(np.clip(off, None, cut), p["seg_key"]), (np.clip(off, cut, None), p["seg_key"])]


def cmllr_wide_triangle(stage, pooled, weighted, tile):
    """a. F = 255, M = tile + 1: the triangle of 32,896 cells ends half a workgroup in, the model's second tile holds one component;
    segments of stage + 1 and 7 frames under two keys"""
    return cmllr_case(255, tile + 1, [stage + 1, 7], [0, 1], 2, 255 + weighted, pooled=pooled, weighted=weighted, matrix=weighted)


def cmllr_tile_edge(stage, M, weighted):
    """b. F = 64, one segment of two full stages and a remainder; M is swept around a tile of model components"""
    return cmllr_case(64, M, [2 * stage + 6], [0], 1, 640 + M + weighted, weighted=weighted, matrix=weighted)


def cmllr_many_keys(weighted=True):
    """c. 300 keys, about 300 segments of 0 - 3 frames in interleaved key order: keys 0 and 299 used, most keys unused, some segments empty;
    key 7 owns a segment of 3 frames and later one of 1 (what segment_sorted puts in the other order)"""
    rng = _rng(300)
    n_keys, n_seg = 300, 300
    used = np.concatenate([[0, 299, 7], rng.choice(np.arange(1, 299), 37, replace=False)])
    keys = used[rng.integers(0, len(used), n_seg)].astype(np.int32)
    lens = rng.integers(0, 4, n_seg)
    keys[[3, 150, 290]] = [299, 0, 299]
    lens[[3, 150, 290]] = [2, 3, 1]
    keys[keys == 7] = 0                                                           # key 7 has these two segments only
    keys[[10, 200]], lens[[10, 200]] = 7, [3, 1]
    return cmllr_case(5, 5, lens, keys, n_keys, 301, weighted=weighted, matrix=True)


def cmllr_padded_matrix():
    """d. the best densities in a matrix whose leading dimension is n_mix + 3"""
    return cmllr_case(13, 9, [40, 3, 11], [0, 1, 0], 2, 13, weighted=True, matrix=True, best_pad=3)


def cmllr_apply_case(seed=80):
    """M = 70 rows, F = 80, about 500 segments of 0 - 3 frames with runs of empty segments first, in the middle and last, the first
    frame at row 5, three keys of which key 1 has no transform"""
    rng = _rng(seed)
    M, F, n_seg = 70, 80, 500
    lens = rng.integers(0, 4, n_seg)
    lens[:6] = 0
    lens[240:252] = 0
    lens[-5:] = 0
    keys = rng.integers(0, 3, n_seg).astype(np.int32)
    off = offsets(lens, 5)
    T = int(off[-1]) + 4                                                          # four rows behind the last segment
    x = (rng.standard_normal((T, F)) * 2).astype(np.float32)
    A = rng.standard_normal((3, M, F + 1)).astype(np.float32)
    return dict(M=M, F=F, n_keys=3, lens=lens, frame_offsets=off, seg_key=keys, has=np.array([1, 0, 1], np.int32), feats=x, transforms=A, out_ld=M + 3)


# ------------------------------------------------------------------------------------------------------------------ MLLR

MLLR_LEAFS4 = dict(n_mix=6, n_leafs=4, leaf_of_mixture=np.array([0, 1, 1, 3, 0, 1], np.int32))   # tests/test_mllr_gpu.py's classes


def mllr_case(D, lens, keys, n_keys, seed, n_mix, n_leafs, leaf_of_mixture, weighted=True, matrix=True, k_hi=3, emission=None):
    rng = _rng(seed)
    model = synth.gmm_cart(n_mix, 1, k_hi, D, seed=seed, pooled=False)
    off = offsets(lens)
    T = int(off[-1])
    feats = (rng.standard_normal((T, D)) * 1.5 + 0.5).astype(np.float32)
    if emission is None:
        emission = rng.integers(0, n_mix, T).astype(np.int32)
        emission[rng.random(T) < 0.1] = -1
        emission[1] = -1
    emission = np.asarray(emission, np.int32)
    ks = np.diff(model["mix_offsets"].astype(np.int64))
    if matrix:
        best = np.stack([rng.integers(0, ks[m], T) for m in range(n_mix)], axis=1).astype(np.uint32)
    else:
        best = np.array([rng.integers(0, ks[e]) if e >= 0 else 0xFFFFFFFF for e in emission], np.uint32)
    weight = None
    if weighted:
        weight = rng.uniform(0.05, 2.0, T)
        weight[rng.random(T) < 0.1] = 0.0
        weight[0] = 0.0
    return dict(model=model, D=D, n_keys=n_keys, n_mix=n_mix, n_leafs=n_leafs, leaf_of_mixture=np.asarray(leaf_of_mixture, np.int32), feats=feats,
                frame_offsets=off, seg_key=np.array(keys, np.int32), emission=emission, best=best, weight=weight, best_ld=n_mix if matrix else 0)


def mllr_restate(p, mode, contract, defect=None):
    return mllr_ref.accumulate(p["model"], mode, p["n_keys"], p["n_leafs"], p["leaf_of_mixture"], p["feats"], p["frame_offsets"], p["seg_key"],
                               p["emission"], p["best"], p["weight"], contract, defect=defect)


def mllr_leaf_frames(p, key, leaf):
    """the frames the lists kernel files under (key, leaf), ascending"""
    out = []
    for s, k in enumerate(p["seg_key"]):
        if k == key:
            for t in range(int(p["frame_offsets"][s]), int(p["frame_offsets"][s + 1])):
                if p["emission"][t] >= 0 and p["leaf_of_mixture"][p["emission"][t]] == leaf:
                    out.append(t)
    return out


def mllr_long_segment(chunk, weighted):
    """a. key 0 owns a segment of 700 frames and, behind a segment of key 1, one of 300.  Leaf 1 (mixtures 1, 2, 5) gets the frames
    chunk - 1 and chunk of the long segment, the frames on both sides of 2 chunk, and frames of the second segment"""
    p = mllr_case(5, [700, 40, 300], [0, 1, 0], 2, 700 + weighted, weighted=weighted, matrix=weighted, **MLLR_LEAFS4)
    e = p["emission"]
    e[[chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, 745, 900]] = [1, 2, 5, 1, 2, 5]
    if not p["best_ld"]:
        p["best"][[chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, 745, 900]] = 0
    p["cut"] = chunk + 44                                                        # the second call's chunks start elsewhere
    return p


def mllr_two_calls(p):
    off, cut = p["frame_offsets"], p["cut"]
    return [(np.clip(off, None, cut), p["seg_key"]), (np.clip(off, cut, None), p["seg_key"])]


def mllr_many_leafs(weighted=True):
    """b. 300 leaves over 400 mixtures: leaves of 256 and more receive frames, 299 among them, the leaves 100 - 139 none"""
    rng = _rng(299)
    n_mix, n_leafs, T = 400, 300, 600
    leaf_of_mixture = (np.arange(n_mix) % n_leafs).astype(np.int32)
    allowed = np.array([m for m in range(n_mix) if not 100 <= leaf_of_mixture[m] < 140])
    emission = allowed[rng.integers(0, len(allowed), T)].astype(np.int32)
    emission[rng.random(T) < 0.05] = -1
    emission[[17, 400]] = [299, 299]
    return mllr_case(3, [350, 250], [0, 1], 2, 299, n_mix, n_leafs, leaf_of_mixture, weighted=weighted, matrix=False, k_hi=2, emission=emission)


def mllr_wide(D, weighted):
    """c. about 60 frames of a D-dimensional model, two leaves"""
    return mllr_case(D, [41, 20], [0, 0], 1, 2000 + D + weighted, 4, 2, [0, 1, 1, 0], weighted=weighted, matrix=False, k_hi=2)


def mllr_adapt_case(seed=70):
    """D = 70, 100 mixtures of 3 densities: 300 means.  Key 0 owns 380 frames, key 1 seven (below every threshold: the fallback).  Mixture 3
    is the silence mixture of leaf 3, the others go to leaves 0 - 2 in turn; tree as in tests/test_mllr_gpu.py.  `matrices`: per mode,
    synthetic matrices of the tree's three inner and leaf nodes for the tests that do not estimate"""
    n_mix, D = 100, 70
    rng = _rng(seed)
    leaf_of_mixture = np.array([3 if m == 3 else m % 3 for m in range(n_mix)], np.int32)
    p = mllr_case(D, [380, 7], [0, 1], 2, seed, n_mix, 4, leaf_of_mixture, weighted=False, matrix=True, k_hi=3)
    p["emission"][20:32] = 3                                                      # key 0 sees enough silence
    p["model"] = synth.gmm_cart(n_mix, 3, 3, D, seed=seed, pooled=False)
    p["best"] = rng.integers(0, 3, p["best"].shape).astype(np.uint32)
    p["tree"] = dict(root=0, left=[1, 3, -1, -1, -1], right=[2, 4, -1, -1, -1], previous=[-1, 0, 0, 1, 1], leaf_number=[-1, -1, 2, 0, 1],
                     leaf_list=[3, 4, 2], silence_mixtures=[3])
    ids = np.array([2, 3, 4, 5], np.int32)
    of_mix = ids[np.array([3 if m == 3 else m % 3 for m in range(n_mix)])]
    full = np.stack([mllr_ref.unit_matrix(mllr_ref.FULL, D) + rng.standard_normal((D, D + 1)) * 0.05 for _ in ids])
    shift = rng.standard_normal((len(ids), D)) * 0.3
    p["synthetic"] = dict(matrix_ids=ids, matrix_of_mixture=of_mix.astype(np.int32), full=full, shift=shift)
    return p


# ------------------------------------------------------------------------------------------------------------------ EBW

EBW_KS = (1, 5, 3, 2, 4, 5)   # tests/test_ebw_gpu.py's model: densities per mixture


def ebw_lattice(rng, lens, n_arcs, n_mix, arc_items, last_arc_items=None):
    """per segment n_arcs arcs of arc_items consecutive frames each (the last arc of the last segment: last_arc_items), the first half on
    one emission, the second on another; weights spread over 20 binary exponents, either sign, every 50th at the threshold or one f32 above"""
    arc_off, w, item_off, fr, em = [0], [], [0], [], []
    for s, (n, a) in enumerate(zip(lens, n_arcs)):
        for i in range(a):
            length = arc_items
            if last_arc_items is not None and s == len(lens) - 1 and i == a - 1:
                length = last_arc_items
            start = int(rng.integers(0, n - length + 1))
            e = rng.integers(0, n_mix, 2)
            frames = np.arange(start, start + length)
            mag = float(rng.uniform(1.0, 2.0)) * 2.0 ** -int(rng.integers(0, 20))
            if i % 50 == 3:
                mag = float(ebw_ref.EPSILON)
            if i % 50 == 4:
                mag = float(np.nextafter(ebw_ref.EPSILON, np.float32(1)))
            w.append(mag if rng.random() < 0.5 else -mag)
            fr.extend(frames)
            em.extend(np.where(frames < start + length // 2, e[0], e[1]))
            item_off.append(len(fr))
        arc_off.append(len(w))
    return (np.array(arc_off, np.int64), np.array(w, np.float32), np.array(item_off, np.int64), np.array(fr, np.int32), np.array(em, np.int32))


def ebw_case(D, lens, n_arcs, arc_items, seed, ks=EBW_KS, pooled=False, last_arc_items=None, first=3):
    rng = _rng(seed)
    ks = tuple(int(k) for k in ks)
    model = synth.gmm_cart(len(ks), 1, 5, D, seed=seed, pooled=pooled, ks=ks)
    off = offsets(lens, first)
    feats = (rng.standard_normal((int(off[-1]) + 2, D + 1)) * 1.5 + 0.5).astype(np.float32)        # a leading dimension above D
    lat = ebw_lattice(rng, lens, n_arcs, len(ks), arc_items, last_arc_items)
    return dict(model=model, D=D, n_mix=len(ks), feats=feats, frame_offsets=off, lattice=lat)


def ebw_big_sort():
    """a. one segment of 2100 frames, 1500 arcs of 12 items: nine sort blocks, a digit table the scan recurses on, three item passes"""
    return ebw_case(39, [2100], [1500], 12, 2100)


def ebw_item_count(n_items):
    """b. exactly n_items items in arcs of 8 (the last arc takes the rest)"""
    n_arcs = (n_items + 7) // 8
    return ebw_case(5, [300], [n_arcs], 8, n_items, last_arc_items=n_items - 8 * (n_arcs - 1))


def ebw_long_corpus():
    """c. 600,000 frames at D = 2 in three segments, 400 arcs of 8 items all over them: four item passes"""
    return ebw_case(2, [250000, 50000, 300000], [150, 50, 200], 8, 600000, first=0)


def ebw_many_lists(pooled):
    """d. 40 mixtures with about 100 densities: more lists than one pass of the list sort tells apart, six bits of mixture"""
    ks = _rng(40).integers(1, 5, 40)
    return ebw_case(7, [60, 200], [80, 320], 10, 4000 + pooled, ks=ks, pooled=pooled)


def ebw_wide_rows(D):
    """e. a chain of 1 + D cells in two workgroups"""
    return ebw_case(D, [40], [60], 6, D)


def ebw_code_bits(c):
    """(frame bits, mixture bits, bits the item sort runs over) as amx_ebw_accumulate_dev derives them"""
    n = int(c["frame_offsets"][-1] - c["frame_offsets"][0])
    frame_bits, mix_bits = max(int(max(n, 1) - 1).bit_length(), 1), max(int(c["n_mix"] - 1).bit_length(), 1)
    return frame_bits, mix_bits, frame_bits + mix_bits + 2        # side bit and the bit that marks an item without a side


def ebw_list_bits(model):
    """(lists, bits the list sort runs over)"""
    o = ebw_ref.layout(model)
    n_lists = int(model["mix_offsets"][-1]) + 2 * model["means"].shape[0] + 2 * model["variances"].shape[0]
    assert o["size"] > n_lists
    return n_lists, max(int(n_lists - 1).bit_length(), 1) + 1


def ebw_expected_shape(c, block_items, n_keys):
    """what amx_ebw_last_shape reports for the case, from the documented plan of the call"""
    n_items = int(c["lattice"][2][-1])
    item_blocks, list_blocks = -(-n_items // block_items), -(-3 * n_keys // block_items)
    return dict(item_sort_passes=-(-ebw_code_bits(c)[2] // 8), list_sort_passes=-(-ebw_list_bits(c["model"])[1] // 8), item_blocks=item_blocks,
                list_blocks=list_blocks, item_table_recursed=256 * item_blocks > block_items, list_table_recursed=256 * list_blocks > block_items)


def ebw_restate(c, best, contract, order="device", defect=None):
    off = c["frame_offsets"]
    keys = ebw_ref.collect(off, *c["lattice"], defect=defect)
    t0 = int(off[0])
    return ebw_ref.accumulate(c["model"], c["feats"][t0:, :c["D"]], best[t0:], keys, order, contract, None, defect), keys
