"""GPU parity: amx_align_viterbi_dev (align_gather_kernel, align_search_kernel, align_traceback_kernel) through the Python class against
the restatement of tests/align_reference.py and against the reference's own results (tests/golden/ref_align.npz), in every bit: labels,
emission indices, arc scores, alignment score, reached flag, iterations, last threshold, survivor sum and average.  No tolerance appears
here except the accumulate test's existing bar in the end-to-end test.

Shapes.  The search kernel gives a segment one workgroup of 256 lanes and a lane the states lane, lane + 256, ...: the linear graphs of 3,
70 and 130 states sit inside one wave, across waves and (2048 states, the limit) in every slot of a lane, where the arcs no longer fit
into LDS and are read from memory.  The next frame's row is fetched one frame ahead: segments of 1, 2 and 3 frames end before, at and
after the first fetched row is used.  Every graph here is narrow (24 columns, at most 300 active hypotheses, 3 arcs into a state):
active sets above 512, 64 arcs out of a state, hundreds to 4096 emissions, the arc count at which LDS is left and calls of hundreds of
segments are in tests/test_align_wide_gpu.py."""
import numpy as np
import pytest

from rasr_amd import _lib
from tests import align_reference as ar
from tests.test_align import all_cases, bits, check_against_fixture, golden, restated, same  # noqa: F401  (golden is a fixture)

pytestmark = pytest.mark.gpu
N = ar.N_COLUMNS


def _torch():
    import torch
    return torch


def device_align(ctx, graphs, off, scores, handle=None, ld=None, rows_before=0, n_columns=N, **cfg):
    """one amx_align_viterbi_dev call; the matrix (n_columns wide) is padded to `ld` columns and shifted down by `rows_before` rows when asked.  Returns
    (label, emission, arc_score) of the call's rows as numpy arrays, the per-segment results and the counters; rows and padding that the
    call must not touch are checked to hold what they held."""
    import rasr_amd
    torch = _torch()
    off = np.asarray(off, np.int64) + rows_before
    ld = ld or n_columns
    rows = int(off[-1])
    host = np.full((max(rows, 1), ld), np.nan, np.float32)
    host[rows_before:rows, :n_columns] = scores
    dev = torch.from_numpy(host).cuda()
    label = torch.full((max(rows, 1),), -7, dtype=torch.int32, device="cuda")
    emission = torch.full((max(rows, 1),), -7, dtype=torch.int32, device="cuda")
    arc = torch.full((max(rows, 1),), -7.0, dtype=torch.float32, device="cuda")
    a = handle or rasr_amd.ViterbiAligner(ctx, **cfg)
    ctx.use_torch_stream()
    _, _, _, results, counters = a.align(off, graphs, dev, ld, n_columns=n_columns, label_dev=label, emission_dev=emission, arc_score_dev=arc)
    torch.cuda.synchronize()
    if handle is None:
        a.close()
    l, e, s = label.cpu().numpy(), emission.cpu().numpy(), arc.cpu().numpy()
    assert (l[:rows_before] == -7).all() and (e[:rows_before] == -7).all() and (s[:rows_before] == -7).all()
    return l[rows_before:rows], e[rows_before:rows], s[rows_before:rows], results, counters


def check_segment(got, want, what):
    """a device result (label, emission, arc, result dict) against a restatement result, in every bit"""
    l, e, s, r = got
    assert np.array_equal(l, want["label"]) and np.array_equal(e, want["emission"]), what
    assert same(s, np.asarray(want["arc_score"], np.float32)), what
    assert same(r["score"], np.float32(want["score"])) and r["reached"] == bool(want["reached"]), what
    assert r["n_iterations"] == want["n_iterations"] and same(r["last_threshold"], np.float32(want["last_threshold"])), what
    assert r["state_sum"] == want["state_sum"], what
    assert same(np.float64(r["average_states"]), np.float64(want["average_states"])) or (np.isnan(r["average_states"]) and np.isnan(want["average_states"])), what


@pytest.mark.parametrize("name", sorted(ar.cases()))
def test_every_case_equals_restatement_and_reference(ctx, golden, name):
    c = all_cases()[name]
    T = len(c["scores"])
    l, e, s, res, counters = device_align(ctx, [c["graph"]], [0, T], c["scores"], **c["cfg"])
    check_segment((l, e, s, res[0]), restated(name), name)
    check_against_fixture(golden, name, dict(res[0], label=l, emission=e, arc_score=s))
    assert counters[0] == 0 and counters[1] + counters[2] == res[0]["n_iterations"]
    assert counters[1] == ar.count_executed_passes(c["graph"], c["scores"], **c["cfg"]), "passes that repeat an outcome are counted, not run"


def batch_results(ctx, handle=None, **kw):
    graphs, off, scores = ar.batch_case(all_cases())
    l, e, s, res, counters = device_align(ctx, graphs, off, scores, handle=handle, **kw)
    return graphs, off, scores, [(l[off[i]:off[i + 1]], e[off[i]:off[i + 1]], s[off[i]:off[i + 1]], res[i]) for i in range(len(graphs))], counters


def test_batch_of_eight_segments(ctx, golden):
    graphs, off, scores, got, counters = batch_results(ctx)
    assert len(graphs) == 8 and 0 in np.diff(off)
    for name, g in zip(ar.BATCH, got):
        check_segment(g, restated(name), name)
        check_against_fixture(golden, name, dict(g[3], label=g[0], emission=g[1], arc_score=g[2]))
    assert counters[0] == 0 and counters[1] + counters[2] == sum(g[3]["n_iterations"] for g in got)


def test_batch_independence_and_call_history(ctx):
    """each segment of the batch aligned alone gives the bits it has inside the batch: on a fresh handle, and on one handle that has
    aligned the whole batch and an unrelated larger graph before (its buffers are sized and filled by those calls)"""
    import rasr_amd
    graphs, off, scores, got, _ = batch_results(ctx)
    used = rasr_amd.ViterbiAligner(ctx)
    batch_results(ctx, handle=used)
    big = ar.linear_hmm(300, N, 77)
    device_align(ctx, [big, big], [0, 150, 190], ar._gauss("history", 190), handle=used)
    for i, name in enumerate(ar.BATCH):
        rows = scores[off[i]:off[i + 1]]
        for handle in (None, used):
            l, e, s, res, _ = device_align(ctx, [graphs[i]], [0, len(rows)], rows, handle=handle)
            for a, b in zip((l, e, s), got[i][:3]):
                assert same(a, b), (name, handle is used)
            assert {k: bits(np.asarray(v)).tolist() for k, v in res[0].items()} == {k: bits(np.asarray(v)).tolist() for k, v in got[i][3].items()}, name
    again = batch_results(ctx, handle=used)[3]
    for g, h in zip(got, again):
        assert all(same(a, b) for a, b in zip(g[:3], h[:3])) and g[3]["n_iterations"] == h[3]["n_iterations"] and same(g[3]["score"], h[3]["score"])
    used.close()


def test_strided_matrix_and_first_row_above_zero(ctx):
    graphs, off, scores, got, _ = batch_results(ctx)
    for kw in (dict(ld=N + 9), dict(rows_before=5), dict(ld=2 * N + 1, rows_before=3)):
        other = batch_results(ctx, **kw)[3]
        for name, g, h in zip(ar.BATCH, got, other):
            assert all(same(a, b) for a, b in zip(g[:3], h[:3])), (name, kw)
            assert g[3]["n_iterations"] == h[3]["n_iterations"] and same(g[3]["score"], h[3]["score"]) and g[3]["state_sum"] == h[3]["state_sum"], (name, kw)


def test_the_state_limit_with_arcs_read_from_memory(ctx):
    """2048 states fill every slot of every lane; their 6141 arcs do not fit into LDS beside the states"""
    g = ar.linear_hmm(_lib.AMX_ALIGN_MAX_STATES, N, 99)
    for T in (5, 40):
        s = ar._gauss("limit%d" % T, T)
        l, e, a, res, _ = device_align(ctx, [g], [0, T], s, max_acoustic_pruning=400.0)
        check_segment((l, e, a, res[0]), ar.align_segment(g, s, max_acoustic_pruning=400.0), T)
    # reached: the same graph entered ten states before its end
    g2 = dict(g, initial=_lib.AMX_ALIGN_MAX_STATES - 10)
    s = ar._gauss("limit_reached", 12)
    l, e, a, res, _ = device_align(ctx, [g2], [0, 12], s)
    want = ar.align_segment(g2, s)
    assert want["reached"]
    check_segment((l, e, a, res[0]), want, "entered late")


def test_nan_rule(ctx):
    """a NaN in a column the graph uses marks that segment only and is counted; a NaN in a column no arc reads changes nothing"""
    graphs, off, scores, got, _ = batch_results(ctx)
    i = ar.BATCH.index("variants")
    used = sorted({e for arcs in graphs[i]["arcs"] for _, e, _, _ in arcs})
    unused = [c for c in range(N) if c not in used]
    assert unused
    poisoned = scores.copy()
    poisoned[off[i]:off[i + 1], unused[0]] = np.nan
    other, counters = batch_results_of(ctx, graphs, off, poisoned)
    assert counters[0] == 0
    for g, h in zip(got, other):
        assert all(same(a, b) for a, b in zip(g[:3], h[:3])) and same(g[3]["score"], h[3]["score"])
    poisoned = scores.copy()
    poisoned[off[i] + 4, used[2]] = np.nan
    other, counters = batch_results_of(ctx, graphs, off, poisoned)
    assert counters[0] == 1
    for k, (g, h) in enumerate(zip(got, other)):
        if k != i:
            assert all(same(a, b) for a, b in zip(g[:3], h[:3])) and same(g[3]["score"], h[3]["score"]), ar.BATCH[k]
    l, e, s, r = other[i]
    want = ar.align_segment(graphs[i], poisoned[off[i]:off[i + 1]])
    assert want["nan"] and not r["reached"] and float(r["score"]) == ar.F32_MAX and (l == -1).all() and (e == -1).all() and not s.any()
    assert r["n_iterations"] == want["n_iterations"] and same(r["last_threshold"], np.float32(want["last_threshold"])) and r["state_sum"] == 0


def batch_results_of(ctx, graphs, off, scores):
    l, e, s, res, counters = device_align(ctx, graphs, off, scores)
    return [(l[off[i]:off[i + 1]], e[off[i]:off[i + 1]], s[off[i]:off[i + 1]], res[i]) for i in range(len(graphs))], counters


def test_score_align_accumulate_end_to_end(ctx):
    """amx_gmm_score_dev -> ViterbiAligner.align -> amx_gmm_accumulate_dev with emission_dev, the matrix never on the host, against the
    oracle's scores -> align_reference -> the oracle's accumulation at test_viterbi_accumulators' bar (weights exactly, f64 sums to
    rtol 1e-12 / atol 1e-9)"""
    import rasr_amd
    from oracle import OracleGmm
    from tests import synth
    torch = _torch()
    M, dim = 24, 16
    model = synth.gmm_cart(M, 1, 4, dim, seed=70)
    lens = (40, 25, 33)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(off[-1])
    x = np.random.Generator(np.random.PCG64(71)).standard_normal((T, dim)).astype(np.float32)
    graphs = [ar.linear_hmm(n, M, 72 + n) for n in (12, 9, 20)]
    sc = rasr_amd.GmmFeatureScorer(ctx, model)
    al = rasr_amd.ViterbiAligner(ctx)
    ctx.use_torch_stream()
    xd = torch.from_numpy(x).cuda()
    scores = torch.empty((T, M), dtype=torch.float32, device="cuda")
    best = torch.empty((T, M), dtype=torch.int32, device="cuda")
    sc.score_dev(xd, T, scores, best)
    label, emission, arc, results, counters = al.align(off, graphs, scores, M)
    acc = torch.zeros(sc.accumulator_size(), dtype=torch.float64, device="cuda")
    sc.accumulate_dev(xd, T, emission, best, M, acc)
    torch.cuda.synchronize()
    o = OracleGmm(model)
    osc, obest = o.score(x)
    wl, we, wa, wr = ar.align_batch(graphs, off, osc)
    assert all(r["reached"] for r in wr) and counters[0] == 0
    assert np.array_equal(label.cpu().numpy(), wl) and np.array_equal(emission.cpu().numpy(), we) and same(arc.cpu().numpy(), wa)
    for r, w in zip(results, wr):
        assert same(r["score"], np.float32(w["score"])) and r["n_iterations"] == w["n_iterations"]
    want = o.accumulate(x, we.astype(np.uint32), obest[np.arange(T), we])
    got = acc.cpu().numpy()
    nk = int(model["mix_offsets"][-1])
    assert np.array_equal(got[:nk], want[:nk]) and got[:nk].sum() == T
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9)
    al.close()


def test_every_refusal_returns_its_code_and_launches_nothing(ctx):
    """with a context: the call's checks come before every launch, so the output buffers keep what they held"""
    import rasr_amd
    torch = _torch()
    small, big = ar.linear_hmm(3, N, 1), ar.linear_hmm(5, N, 2)
    n_small = sum(len(a) for a in small["arcs"])
    scores = torch.from_numpy(ar._gauss("refusals", 9)).cuda()
    a = rasr_amd.ViterbiAligner(ctx)
    fan = ar.graph(2, 0, {1: 0.0}, [(0, 1, i % N, i, 1.0) for i in range(_lib.AMX_ALIGN_MAX_OUT_ARCS + 1)])
    too_many = ar.linear_hmm(_lib.AMX_ALIGN_MAX_STATES + 1, N, 3)
    cases = [([small, big], dict(arc_target=(n_small + 2, 5)), _lib.AMX_ERR_INVALID, ("segment 1", "arc_target[%d] = 5" % (n_small + 2))),
             ([small, big], dict(arc_emission=(1, N)), _lib.AMX_ERR_INVALID, ("segment 0", "arc_emission[1] = %d" % N)),
             ([small, big], dict(initial_state=(0, 3)), _lib.AMX_ERR_INVALID, ("segment 0", "initial_state 3")),
             ([small, big], dict(arc_weight=(0, float("nan"))), _lib.AMX_ERR_INVALID, ("segment 0", "arc_weight[0]")),
             ([small, big], dict(final_weight=(2, float("nan"))), _lib.AMX_ERR_INVALID, ("segment 0", "final_weight of state 2")),
             ([small, fan], dict(), _lib.AMX_ERR_UNSUPPORTED, ("segment 1", "state 0 has 65 arcs")),
             ([small, too_many], dict(), _lib.AMX_ERR_UNSUPPORTED, ("segment 1", "2049 states"))]
    for graphs, patch, status, words in cases:
        g = rasr_amd.ViterbiAligner.graphs(graphs)
        for k, (i, v) in patch.items():
            g[k][i] = v
        label = torch.full((9,), -7, dtype=torch.int32, device="cuda")
        emission, arc = label.clone(), torch.full((9,), -7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(rasr_amd.AmxError) as e:
            a.align([0, 4, 9], g, scores, N, label_dev=label, emission_dev=emission, arc_score_dev=arc)
        assert e.value.status == status, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert (label == -7).all() and (emission == -7).all() and (arc == -7).all()
    for kw, status, word in ((dict(mode=_lib.AMX_ALIGN_BAUM_WELCH), _lib.AMX_ERR_UNSUPPORTED, "mode"),
                             (dict(n_best_pruning=10), _lib.AMX_ERR_UNSUPPORTED, "n_best_pruning"),
                             (dict(min_acoustic_pruning=100.0, max_acoustic_pruning=50.0), _lib.AMX_ERR_INVALID, "min_acoustic_pruning"),
                             (dict(increment_factor=1.0), _lib.AMX_ERR_INVALID, "increment_factor")):
        with pytest.raises(rasr_amd.AmxError) as e:
            rasr_amd.ViterbiAligner(ctx, **kw)
        assert e.value.status == status and word in str(e.value)
    # the handle still works
    l, e, s, res, _ = device_align(ctx, [small], [0, 9], scores.cpu().numpy(), handle=a)
    check_segment((l, e, s, res[0]), ar.align_segment(small, scores.cpu().numpy()), "after the refusals")
    a.close()
