"""GPU parity: amx_accuracy_run_dev through rasr_amd.LatticeAccuracy on synthetic item arrays, every key against
tests/accuracy_reference.py in every bit, in all three modes and both contracts of the frame-phone denominator.  No tolerance appears but
in the end-to-end case, which uses the bars tests/golden/ref_latpost.npz carries.

Shapes.  A wave takes 64 frames per trip: keys of 1, 63, 64, 65 and 130 frames, with runs that cross frames 64 and 128 of their key, one
run per key and one run per frame.  Segment 0 holds the overlap cases by hand (see batch()), segment 1 has no reference key, segment 2 is
random and has more intervals than the lowered LDS capacity."""
import functools

import numpy as np
import pytest

from rasr_amd import _lib
from tests import accuracy_reference as acr

pytestmark = pytest.mark.gpu
F32 = np.float32
LABEL_TOKEN = np.arange(18) // 3   # three allophone states per phoneme; phoneme 0 is the short pause
VARIANTS = {"approximate-phone": ("approximate-phone", "off"), "frame-phone": ("frame-phone", "off"), "frame-phone-fma": ("frame-phone", "fma"),
            "frame-state": ("frame-state", "off")}


def items(*stretches):
    """(label, frames) stretches; a tuple of labels is cycled, which keeps the phoneme and changes the state"""
    return [(lab if isinstance(lab, int) else lab[i % len(lab)]) for lab, n in stretches for i in range(n)]


@functools.lru_cache(maxsize=None)
def batch():
    """-> keys [(segment, tbeg, items or None)], reference flags.  Phonemes: A = 1 (labels 3-5), B = 2, C = 3, D = 4, E = 5."""
    A, B, C, D, E, SP = (3, 4, 5), (6, 7, 8), 9, (12, 13), 15, (0, 1)
    keys = [(0, 0, items((A, 10), (B, 20), (SP, 5), (C, 29))),   # reference [0, 64): A [0, 10), B [10, 30), pause [30, 35), C [35, 64)
            (0, 64, items((D, 60), (B, 10))),                    # reference [64, 134)
            (0, 0, items((A, 10), (B, 20), (SP, 5), (C, 29))),   # the first once more: duplicated intervals
            (0, 5, items((B, 15), (E, 3))),                      # reference: B [5, 20) overlaps the first key's A and B, E [20, 23)
            (0, 9, items((A, 1))),                               # 1 frame, contained in A [0, 10)
            (0, 0, items((B, 63))),                              # 63 frames, one run
            (0, 0, items((A, 1), (B, 1)) * 32),                  # 64 frames, one run per frame
            (0, 10, items((B, 20), (SP, 10), (C, 35))),          # 65 frames: B equals [10, 30) and touches A [0, 10) (re == hs)
            (0, 20, items((D, 60), (C, 10), (D, 60))),           # 130 frames: runs cross frames 64 and 128 of the key; ends beyond frame 134
            (0, 130, items((B, 3), (A, 12))),                    # B overlaps [124, 134) by a part, A lies beyond the reference
            (0, 40, None),                                       # no final state reached
            (1, 0, items((A, 5), (B, 7))), (1, 3, None),         # a segment without reference
            (0, 64, items((D, 52), (B, 4)))]                     # a run of 52 frames: where 1 + 0.3f * (n - 1) rounds differently when fused
    ref = [1, 1, 1, 1] + [0] * 10
    rng = np.random.Generator(np.random.PCG64(11))
    for k in range(48):   # segment 2: random keys of every length class, a third of them reference
        T = int(rng.choice([1, 7, 63, 64, 65, 130]))
        stretches = []
        while sum(n for _, n in stretches) < T:
            stretches.append((int(rng.integers(0, 18)), int(rng.integers(1, 40))))
        keys.append((2, int(rng.integers(0, 200)), items(*stretches)[:T]))
        ref.append(int(k % 3 == 0))
    return keys, ref


def tokens(mode, keys):
    return [(s, b, None if it is None else [int(t) if mode == "frame-state" else int(LABEL_TOKEN[t]) for t in it]) for s, b, it in keys]


@functools.lru_cache(maxsize=None)
def want(variant):
    """the restatement, computed once per variant and never changed"""
    mode, contract = VARIANTS[variant]
    keys, ref = batch()
    return acr.accuracies(mode, tokens(mode, keys), ref, (0, 1, 2) if mode == "frame-state" else (0,), 0.3, contract == "fma")


def run(ctx, variant, which=None, lds=0, poison=None):
    import torch

    import rasr_amd
    mode, contract = VARIANTS[variant]
    keys, ref = batch()
    keys, ref = ([keys[i] for i in which], [ref[i] for i in which]) if which is not None else (keys, ref)
    lens = [len(it) if it is not None else 7 for _, _, it in keys]
    flat = np.concatenate([np.asarray(it if it is not None else [-1] * 7, np.int32) for _, _, it in keys])
    if poison is not None:
        flat[poison[0]] = poison[1]
    ctx.use_torch_stream()
    ctx.set_contract(contract)
    state = mode == "frame-state"
    a = rasr_amd.LatticeAccuracy(ctx, mode, 18 if state else 6, None if state else LABEL_TOKEN, (0, 1, 2) if state else (0,), 0.3)
    a.set_lds_intervals(lds)
    out = torch.full((len(keys),), -7.0, dtype=torch.float32, device="cuda")
    try:
        _, info = a.run([k[0] for k in keys], [k[1] for k in keys], [k[1] + n for k, n in zip(keys, lens)], np.concatenate([[0], np.cumsum(lens)]), ref,
                        torch.from_numpy(flat).cuda(), 3, out)
        arc_key = np.array([len(keys) - 1, -1, 0, 8 % len(keys), -1], np.int32)
        arcs = a.arc_accuracies(arc_key).cpu().numpy()
        return dict(acc=out.cpu().numpy(), info=info, tables=[a.last_reference(s) for s in range(3)], arcs=arcs, arc_key=arc_key)
    except rasr_amd.AmxError as e:
        return dict(acc=out.cpu().numpy(), error=e)
    finally:
        ctx.set_contract("off")
        a.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_key_equals_the_restatement_on_the_lds_and_the_global_path(ctx, variant):
    acc, segs = want(variant)
    keys, ref = batch()
    got = run(ctx, variant)
    bad = [(k, got["acc"][k], acc[k]) for k in range(len(keys)) if bits(got["acc"][k]) != bits(acc[k])]
    assert not bad, bad
    assert np.count_nonzero(acc[:11]) >= 6 and not acc[10:13].any() and len(set(acc.tolist())) > 6, "the cases are not all trivial"
    tables = [acr.table(segs[s]) for s in range(3)]
    assert all(np.array_equal(g, w) for g, w in zip(got["tables"], tables)) and len(tables[1]) == 0 and min(len(tables[0]), len(tables[2])) > 5
    assert got["info"]["reference_intervals"] == sum(len(t) for t in tables) and got["info"]["keys_without_alignment"] == 2
    assert np.array_equal(bits(got["arcs"]), bits([acc[k] if k >= 0 else 0.0 for k in got["arc_key"]]))
    low = run(ctx, variant, lds=5)   # segment 0's and 2's tables are above it, sort and lookups go through global memory
    assert np.array_equal(bits(low["acc"]), bits(got["acc"])) and all(np.array_equal(g, w) for g, w in zip(low["tables"], tables))


@pytest.mark.parametrize("variant", ["approximate-phone", "frame-phone-fma", "frame-state"])
def test_a_key_alone_with_its_reference_equals_the_key_in_the_batch(ctx, variant):
    which = (0, 1, 2, 3, 8)
    alone = run(ctx, variant, which)
    assert np.array_equal(bits(alone["acc"]), bits(want(variant)[0][list(which)])) and alone["acc"][4] != 0


def test_the_contracts_differ_and_a_bad_item_leaves_the_output_untouched(ctx):
    assert not np.array_equal(bits(want("frame-phone")[0]), bits(want("frame-phone-fma")[0])), "normalization 0.3 makes the denominators differ"
    for variant, poison, word in (("approximate-phone", (70, 18), "item 18"), ("frame-state", (3, -2), "item -2"), ("frame-phone", (64, -1), "mixes -1")):
        got = run(ctx, variant, poison=poison)
        assert got["error"].status == _lib.AMX_ERR_INVALID and word in str(got["error"]) and (got["acc"] == -7).all(), str(got["error"])
    assert "key 1, slot 6" in str(run(ctx, "approximate-phone", poison=(70, 18))["error"])


def test_end_to_end_arcalign_accuracy_expectation(ctx):
    """LatticeArcAligner.run -> LatticeAccuracy.run -> arc_accuracies -> LatticePosterior("expectation") on one two-state lattice per segment
    whose parallel arcs are the segment's keys and one arc without pronunciation, against tests/latpost_reference.py fed with the
    restatement's risks"""
    import torch

    import rasr_amd
    from tests import latpost_reference as lr
    from tests.test_arcalign_gpu import N, batch as arc_batch
    from tests.test_latpost_gpu import bar, close
    graphs, keys, off, scores = arc_batch()
    keys = np.array(keys, np.int32)
    ctx.use_torch_stream()
    ctx.set_contract("off")
    al = rasr_amd.LatticeArcAligner(ctx)
    out = al.run(graphs, *keys.T, off, torch.from_numpy(scores).cuda(), N)
    label_token, ref = (np.arange(1200) // 4) % 6, (np.arange(len(keys)) % 5 == 0)
    ac = rasr_amd.LatticeAccuracy(ctx, "approximate-phone", 6, label_token, (0,))
    key_acc, _ = ac.run(keys[:, 1], keys[:, 2], keys[:, 3], out["slot_offsets"], ref, out["label_dev"], 2)
    labels, so = out["label_dev"].cpu().numpy(), out["slot_offsets"]
    toks = [(int(s), int(b), None if labels[so[k]] < 0 else label_token[labels[so[k]:so[k + 1]]].tolist()) for k, (_, s, b, _) in enumerate(keys)]
    want_acc, _ = acr.accuracies("approximate-phone", toks, ref, (0,))
    assert np.array_equal(bits(key_acc.cpu().numpy()), bits(want_acc)) and np.count_nonzero(want_acc) > 10
    arc_key = [[-1] + [k for k in range(len(keys)) if keys[k, 1] == s] for s in range(2)]
    risk = ac.arc_accuracies(arc_key[0] + arc_key[1]).cpu().numpy()
    lats = [lr.lattice(2, [(0, 1, float(a % 3) + 0.5, float(risk[len(arc_key[0]) * s + a])) for a in range(len(arc_key[s]))], 0, {1: 0.0}) for s in range(2)]
    arc, _, info = rasr_amd.LatticePosterior(ctx, "expectation").run(lats)
    arc, a0 = arc.cpu().numpy(), 0
    for s, lat in enumerate(lats):
        lat["arc_risk"] = np.array([want_acc[k] if k >= 0 else 0.0 for k in arc_key[s]], F32)
        w = lr.posterior(lat, lr.EXPECTATION)
        close(arc[a0:a0 + len(arc_key[s])], w["arc"], bar("expectation"), "arcs of segment %d" % s)
        close([info[s]["expectation"]], [w["info"]["expectation"]], bar("expectation_value"), "expectation of segment %d" % s)
        a0 += len(arc_key[s])
    al.close(), ac.close()
