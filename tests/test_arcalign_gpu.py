"""GPU parity: amx_arcalign_run_dev (arcalign_search_kernel<1> and <4>) through rasr_amd.LatticeArcAligner.  Every key against
tests/align_reference.align_segment on the window's rows -- the restatement tests/test_align.py pins on the reference's text -- in every
bit: labels, emission indices, arc scores, alignment score, reached flag, iterations, last threshold, survivor sum; the emission score
against a plain f32 chain.  No tolerance appears here.

Shapes.  State s lives in lane s % 64, slot s / 64: 1, 2, 63 and 64 states run in the one-slot kernel, 65 and 256 in the four-slot one.
The traceback stages 16 frames of back-pointers and the score chain 64 frames: windows of 1, 63, 64, 65 and 130 frames end before, at
and after those stages.  Every matrix has NaN rows around the windows and a padded leading dimension."""
import functools

import numpy as np
import pytest

from rasr_amd import _lib
from tests import align_reference as ar
from tests.test_align import bits, same
from tests.test_arcalign import fan_in, refusals

pytestmark = pytest.mark.gpu
N, F32 = ar.N_COLUMNS, np.float32


def tie_graph(n, seed):
    """ar._random_tie_graph with n states: up to 4 arcs out of each in a shuffled target order, weights in {0, 1, 2}, a fifth of the states final"""
    rng = np.random.Generator(np.random.PCG64(seed))
    arcs = [(s, int(t), e, e * 16 + s % 16, float(rng.integers(0, 3))) for s in range(n) for t in rng.permutation(n)[:int(rng.integers(1, 5))]
            for e in [int(rng.integers(0, N))]]
    return ar.graph(n, 0, {int(s): float(rng.integers(0, 2)) for s in rng.permutation(n)[:max(n // 5, 1)]}, arcs)


def matrix(name, T, integer=False):
    if integer:
        return np.random.Generator(np.random.PCG64(ar._seed(name))).integers(0, 4, (T, N)).astype(F32)
    return ar._gauss(name, T)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (graph, frames, integer scores, cfg)"""
    lin = lambda n: ar.linear_hmm(n, N, 40 + n)
    few = dict(min_acoustic_pruning=4.0)   # several passes until nothing is pruned or the score stands
    return {"lin1_T1": (lin(1), 1, False, {}), "lin2_T63": (lin(2), 63, False, {}), "lin63_T64": (lin(63), 64, False, few),
            "lin64_T65": (lin(64), 65, False, {}), "lin65_T130": (lin(65), 130, False, few), "lin256_T130": (dict(lin(256), initial=60), 130, False, {}),
            "not_reached": (lin(63), 5, False, {}), "fan255": (fan_in(255), 7, True, {}), "tie12": (ar._random_tie_graph(701), 12, True, {}),
            "tie64": (tie_graph(64, 5), 17, True, {}), "tie200": (tie_graph(200, 6), 65, True, dict(min_acoustic_pruning=1.0)), "scale": (lin(40), 50, False, dict(score_scale=0.37))}


@functools.lru_cache(maxsize=None)
def restated(name):
    g, T, integer, cfg = cases()[name]
    return ar.align_segment(g, matrix(name, T, integer), **cfg)


def run(ctx, graphs, keys, off, scores, handle=None, cap=0, **cfg):
    """one amx_arcalign_run_dev call on `scores` between two NaN rows, ld = N + 3; keys: rows of (graph, segment, tbeg, tend).
    Returns the call's dict with the device arrays as numpy arrays"""
    import torch

    import rasr_amd
    host = np.full((len(scores) + 2, N + 3), np.nan, F32)
    host[1:-1, :N] = scores
    a = handle or rasr_amd.LatticeArcAligner(ctx, **cfg)
    a.set_workspace_cap(cap)
    ctx.use_torch_stream()
    out = a.run(graphs, *np.array(keys, np.int32).reshape(-1, 4).T, np.asarray(off) + 1, torch.from_numpy(host).cuda(), N + 3, n_columns=N)
    torch.cuda.synchronize()
    out["launches"] = a.last_launches()
    if handle is None:
        a.close()
    return {k: v.cpu().numpy() if hasattr(v, "cpu") else v for k, v in out.items()}


def check_key(out, k, graph, window, cfg, what):
    want = restated(what) if what in cases() else ar.align_segment(graph, window, **cfg)
    if want["nan"]:   # the library's rule where the reference is undefined: not reached, nothing of the pass that met the NaN is reported
        want = dict(want, score=ar.F32_MAX, reached=False, state_sum=0)
    a, b = out["slot_offsets"][k:k + 2]
    r = out["results"][k]
    assert b - a == len(window), what
    assert np.array_equal(out["label_dev"][a:b], want["label"]) and np.array_equal(out["emission_dev"][a:b], want["emission"]), what
    assert same(out["arc_score_dev"][a:b], np.asarray(want["arc_score"], F32)), what
    assert same(r["score"], F32(want["score"])) and r["reached"] == bool(want["reached"]) and same(out["key_score_dev"][k], r["score"]), what
    assert r["n_iterations"] == want["n_iterations"] and same(r["last_threshold"], F32(want["last_threshold"])), what
    assert r["state_sum"] == want["state_sum"] and (same(np.float64(r["average_states"]), np.float64(want["average_states"])) or want["nan"]), what
    scale, es = F32(cfg.get("score_scale", 1.0)), F32(0)
    for t, e in enumerate(want["emission"] if want["reached"] else []):
        es = F32(es + (window[t, e] if scale == 1 else F32(scale * window[t, e])))
    assert same(out["key_emission_score_dev"][k], es), what
    return want


@pytest.mark.parametrize("name", sorted(cases()))
def test_one_key_equals_the_restatement(ctx, name):
    g, T, integer, cfg = cases()[name]
    scores = np.concatenate([matrix("before", 3), matrix(name, T, integer), matrix("after", 2)])
    out = run(ctx, [g], [(0, 0, 3, 3 + T)], [0, len(scores)], scores, **cfg)
    want = check_key(out, 0, g, scores[3:3 + T], cfg, name)
    assert want["reached"] == (name != "not_reached")
    assert out["counters"][0] == 0 and out["counters"][1] + out["counters"][2] == want["n_iterations"]
    assert out["counters"][1] == ar.count_executed_passes(g, scores[3:3 + T], **cfg), "passes that repeat an outcome are counted, not run"
    if name in ("lin63_T64", "lin65_T130", "tie200"):
        assert out["counters"][1] > 1, "several passes ran"
    if name in ("lin2_T63", "tie64"):
        assert out["counters"][2] > 0, "a pass that pruned nothing ended the work"


def batch():
    """two segments (60 and 45 frames), 5 graphs, 41 keys: overlapping windows, identical windows, one window per graph kind"""
    rng = np.random.Generator(np.random.PCG64(77))
    graphs = [ar.linear_hmm(5, N, 1), ar.linear_hmm(12, N, 2), ar.linear_hmm(70, N, 3), ar._random_tie_graph(700), tie_graph(90, 9)]
    need, lens = [3, 6, 35, 4, 6], [60, 45]
    keys = []
    for i in range(40):
        g, s = i % 5, int(rng.integers(0, 2))
        T = min(int(rng.integers(need[g], need[g] + 20)), lens[s])
        b = int(rng.integers(0, lens[s] - T + 1))
        keys.append((g, s, b, b + T))
    keys.append(keys[7])
    scores = np.concatenate([matrix("batch0", 60), matrix("batch1", 45, integer=True)])
    return graphs, keys, np.array([0, 60, 105]), scores


def test_batch_nan_key_workspace_split_and_no_keys(ctx):
    graphs, keys, off, scores = batch()
    out = run(ctx, graphs, keys, off, scores)
    for k, (g, s, b, e) in enumerate(keys):
        check_key(out, k, graphs[g], scores[off[s] + b:off[s] + e], {}, k)
    assert out["launches"] == 2 and out["counters"][0] == 0, "one launch per kernel variant"
    cut = run(ctx, graphs, keys, off, scores, cap=2000)
    assert cut["launches"] > 4
    for f in ("label_dev", "emission_dev", "arc_score_dev", "key_score_dev", "key_emission_score_dev"):
        assert same(cut[f], out[f]), f
    # a NaN in a column that key 3's graph reads, in the second row of its window: the keys that meet it are counted, no other key changes
    g, s, b, e = keys[3]
    used = sorted({em for arcs in graphs[g]["arcs"] for _, em, _, _ in arcs})
    poisoned = scores.copy()
    poisoned[off[s] + b + 1, used[0]] = np.nan
    other = run(ctx, graphs, keys, off, poisoned)
    met = [k for k, (kg, ks, kb, ke) in enumerate(keys) if ar.align_segment(graphs[kg], poisoned[off[ks] + kb:off[ks] + ke])["nan"]]
    assert 3 in met and other["counters"][0] == len(met)
    for k, (kg, ks, kb, ke) in enumerate(keys):
        check_key(other, k, graphs[kg], poisoned[off[ks] + kb:off[ks] + ke], {}, k)
        assert other["results"][k]["reached"] == (out["results"][k]["reached"] and k not in met)
    none = run(ctx, graphs, [], off, scores)
    assert none["slot_offsets"].tolist() == [0] and none["counters"] == (0, 0, 0) and none["launches"] == 0


def test_a_key_over_a_whole_segment_gives_the_bits_of_the_segment_aligner(ctx):
    import torch

    import rasr_amd
    graphs, _, off, scores = batch()
    pair = [graphs[2], graphs[4]]
    out = run(ctx, pair, [(0, 0, 0, 60), (1, 1, 0, 45)], off, scores)
    al = rasr_amd.ViterbiAligner(ctx)
    label, emission, arc, results, _ = al.align(off, pair, torch.from_numpy(scores).cuda(), N)
    torch.cuda.synchronize()
    assert same(out["label_dev"], label.cpu().numpy()) and same(out["emission_dev"], emission.cpu().numpy()) and same(out["arc_score_dev"], arc.cpu().numpy())
    for r, w in zip(out["results"], results):
        assert {k: bits(np.asarray(v)).tolist() for k, v in r.items()} == {k: bits(np.asarray(v)).tolist() for k, v in w.items()}
    al.close()


def test_every_refusal_leaves_the_outputs_as_they_were(ctx):
    import torch

    import rasr_amd
    a = rasr_amd.LatticeArcAligner(ctx)
    scores, wide = torch.from_numpy(matrix("refusals", 15)).cuda(), torch.zeros((15, 400), dtype=torch.float32, device="cuda")
    for graphs, patch, keys, status, words in refusals():
        if status == _lib.AMX_ERR_STATE:
            continue
        g = rasr_amd.LatticeArcAligner.graphs(graphs)
        for k, (i, v) in patch.items():
            g[k][i] = v
        ints = [torch.full((16,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        floats = [torch.full((16,), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
        with pytest.raises(rasr_amd.AmxError) as e:
            ld = 400 if "emission indices" in words[-1] else N
            a.run(g, *np.array(keys, np.int32).T, [0, 9, 15], wide if ld == 400 else scores, ld, None, ints[0], ints[1], *floats)
        assert e.value.status == status and words[-1] in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert all((t == -7).all() for t in ints + floats), words
    a.close()


def test_expanded_tables_feed_the_sequence_trainer_as_the_restatements_do(ctx):
    """keys on two segments of tests/nnseq_reference's batch -> amx_arcalign_expand -> amx_nnseq_arc_scores_dev, against the same call on
    tables built from the restatement's alignments; arcs with key -1, a key used by two arcs and a key that reaches no final state"""
    import rasr_amd
    from tests import nnseq_reference as sr
    from tests.test_nnseq_gpu import dev, trainers
    net, off, feats, _, _, _, _, _, _ = sr.gpu_batch()
    valid = np.asarray(sr.valid_classes(net))
    assert len(valid) >= N and sr.n_classes(net) <= 64
    rng = np.random.Generator(np.random.PCG64(5))
    scores = np.zeros((int(off[-1]), 64), F32)
    scores[:, valid[:N]] = rng.normal(60.0, 15.0, (int(off[-1]), N)).astype(F32)
    graphs = [ar.linear_hmm(n, N, n) for n in (4, 9, 30)]
    for g in graphs:
        g["arcs"] = [[(t, int(valid[e]), l, w) for t, e, l, w in arcs] for arcs in g["arcs"]]
    keys = np.array([(0, 1, 10, 30), (1, 1, 20, 45), (2, 1, 0, 8), (2, 3, 100, 140), (0, 4, 290, 300)], np.int32)
    arc_offsets, arc_key = np.array([0, 0, 5, 5, 7, 9]), [0, -1, 1, 2, 0, 3, -1, 4, 4]
    a = rasr_amd.LatticeArcAligner(ctx)
    ctx.use_torch_stream()
    out = a.run(graphs, *keys.T, off, dev(scores), 64)
    assert [r["reached"] for r in out["results"]] == [True, True, False, True, True]
    got = rasr_amd.LatticeArcAligner.expand(keys[:, 1], keys[:, 2], keys[:, 3], out["slot_offsets"], out["emission_dev"].cpu().numpy(), arc_offsets, arc_key)
    frames, ems, io = [], [], [0]
    for k in arc_key:
        g, s, b, e = keys[k]
        r = ar.align_segment(graphs[g], scores[off[s] + b:off[s] + e]) if k >= 0 else dict(reached=False)
        if r["reached"]:
            frames += list(range(b, e))
            ems += list(r["emission"])
        io.append(len(frames))
    want = dict(arc_offsets=arc_offsets, item_offsets=np.array(io), item_frame=np.array(frames, np.int32), item_emission=np.array(ems, np.int32))
    tr, seq = trainers(ctx, net)
    seq.forward_dev(dev(feats), feats.shape[1], off)
    assert same(seq.arc_scores(got).cpu().numpy(), seq.arc_scores(want).cpu().numpy()) and int(got["item_offsets"][-1]) == len(frames) > 0
    # the gather of the key scores into arc order
    import torch
    arc = torch.full((len(arc_key),), -7.0, dtype=torch.float32, device="cuda")
    for which, keyed in (("alignment", out["key_score_dev"]), ("emission", out["key_emission_score_dev"])):
        a.arc_scores_dev(arc_key, which, arc)
        assert same(arc.cpu().numpy(), np.array([keyed[k].item() if k >= 0 else 0.0 for k in arc_key], F32)), which
    seq.close(), tr.close(), a.close()
