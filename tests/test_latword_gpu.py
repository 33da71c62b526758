"""GPU: rasr_amd.LatticeWordMeasures (latword.hip) against the restatement of tests/latword_reference.py.

The accuracy modes equal the restatement in every bit.  Time-frame modes: the discrete results are equal (which cells exist, the counts,
the refusal); a cell fed by n arcs lies within (n + 4) * 2^-23 of the all-f64 evaluation of the same cell, on the device and in the
restatement (n - 1 f32 additions, the narrowing of p and of the score and a derivative of at most 1.001 give just under
(n + 3) * 2^-24; the bar is twice that); an arc's bar is the sum of its cells' bars over |den| plus (d + 2) * 2^-23 of its value for a
chain over d frames (maximum mode: its largest cell bar).

The fan: k arcs of label 7 from state 0 (frame 0) to state 1 (frame T), the same label on 0 -> 2 -> 1 through the middle, a long arc of
the sparse label 2^30 - 5, label -1, a zero-duration arc 1 -> 3, and state 4, which nothing reaches."""
import numpy as np
import pytest

from tests import latword_reference as wr

pytestmark = pytest.mark.gpu

FAR = 2 ** 30 - 5


def fan(T, k, seed, weights="random"):
    mid = max(T // 2, 1) if T > 1 else 0
    arcs = [(0, 1, 7)] * k + [(0, 2, 7), (2, 1, 7), (0, 1, FAR), (0, 2, -1), (2, 1, FAR), (1, 3, 7), (4, 1, 7), (0, 3, -1)]
    lat = wr.lattice([0, T, mid, T, 0], arcs)
    n, rng = len(arcs), np.random.default_rng(seed)
    r = {"random": rng.uniform(0.05, 1.0, n), "equal": np.ones(n), "decreasing": 2.0 ** np.arange(n) / 2.0 ** n + 1e-3}[weights]
    lat["arc_weight"] = (-np.log(r / (1.01 * r.sum()))).astype(np.float32)   # any subset of the posteriors sums to less than 1
    return lat


def shape():
    import rasr_amd
    return rasr_amd.LatticeWordMeasures.kernel_shape()


def run(ctx, mode, lats, correct=None, normalization=0.0, short_pauses=(), rows=()):
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    m = rasr_amd.LatticeWordMeasures(ctx, mode, normalization, short_pauses)
    w = torch.from_numpy(np.concatenate([l["arc_weight"] for l in lats])).cuda() if mode.startswith("timeframe") else None
    out, info = m.run(lats, w, correct)
    got = out.cpu().numpy(), info, [m.last_row(g, label) for g, label in rows]
    m.close()
    return got


def check_timeframe(ctx, lat, maximum, normalization=0.0, fma=False):
    """one lattice through the device and the restatement -> the largest |device - restatement| over cells and arcs"""
    labels = sorted(set(int(l) for l in lat["arc_label"]))
    got, info, rows = run(ctx, "timeframe-error-max" if maximum else "timeframe-error-sum", [lat], normalization=normalization, rows=[(0, l) for l in labels])
    want, bad, table = wr.timeframe_errors(lat, lat["arc_weight"], maximum, normalization, fma)
    assert bad is None
    fed = wr.arcs(lat)
    assert info[0]["states_unreached"] == 1 and info[0]["feeds"] == sum(e - s for _, _, s, e in fed) and info[0]["labels"] == len({l for _, l, s, e in fed if s < e})
    worst = 0.0
    for label, (lo, score) in zip(labels, rows):
        mine = {t: v for (t, l), v in table.items() if l == label}
        assert (lo, lo + len(score)) == ((min(mine), max(mine) + 1) if mine else (0, 0)), label   # which cells exist
        assert all(score[t - lo] == 0 for t in range(lo, lo + len(score)) if t not in mine), label
        for t, (ref, exact, n) in mine.items():
            bar = (n + 4) * 2.0 ** -23
            assert abs(float(score[t - lo]) - exact) <= bar and abs(float(ref) - exact) <= bar, (label, t, n, score[t - lo], ref, exact)
            worst = max(worst, abs(float(score[t - lo]) - float(ref)))
    reached = {a for a, _, _, _ in fed}
    for a, label, s, e in fed:
        den = float(wr.den(normalization, s, e, fma))
        if s == e:
            assert got[a].tobytes() == want[a].tobytes(), (a, got[a], want[a])   # 0 / den and f32 min, as the text gives them
            continue
        bars = [(table[(t, label)][2] + 4) * 2.0 ** -23 for t in range(s, e)]
        exact = max(table[(t, label)][1] for t in range(s, e)) if maximum else sum(table[(t, label)][1] for t in range(s, e)) / den
        bar = max(bars) if maximum else sum(bars) / abs(den) + (e - s + 2) * 2.0 ** -23 * abs(exact)
        assert abs(float(got[a]) - exact) <= bar and abs(float(want[a]) - exact) <= bar, (a, label, s, e, got[a], want[a], exact, bar)
        worst = max(worst, abs(float(got[a]) - float(want[a])))
    assert all(got[a] == 0 for a in range(len(got)) if a not in reached)
    print("largest |device - restatement|: %.3g" % worst)
    return got


def k_cases():
    L = shape()["list_arcs"]   # label 7 has k + 2 feeding arcs, k + 1 of them over any one frame: one below the threshold, at it, above
    return sorted({1, 2, 64, 65, 300, L - 3, L - 2, L + 1})


@pytest.mark.parametrize("maximum", [False, True], ids=["sum", "max"])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 129])
def test_timeframe_errors_over_segment_lengths(ctx, T, maximum):
    check_timeframe(ctx, fan(T, 3, T), maximum, normalization=0.25)


@pytest.mark.parametrize("k", range(8))
def test_timeframe_errors_over_covering_arcs_and_the_list_threshold(ctx, k):
    check_timeframe(ctx, fan(130, k_cases()[k], k), False)


@pytest.mark.parametrize("weights", ["equal", "decreasing"])
def test_timeframe_errors_ties_and_a_feed_of_new_minima(ctx, weights):
    check_timeframe(ctx, fan(65, 5, 3, weights), False)


@pytest.mark.parametrize("fma", [False, True], ids=["off", "fma"])
def test_both_contracts_of_the_denominator(ctx, fma):
    ctx.set_contract("fma" if fma else "off")
    try:
        lat, cor = fan(65, 2, 5), fan(40, 1, 6)
        check_timeframe(ctx, lat, False, normalization=0.1, fma=fma)
        got = run(ctx, "frame-word-accuracy", [lat], [cor], normalization=0.1)[0]
        assert got.tobytes() == wr.frame_word_accuracy(lat, cor, 0.1, fma).tobytes()
    finally:
        ctx.set_contract("off")
    assert wr.den(0.1, 0, 32, True) != wr.den(0.1, 0, 32, False)   # the two contracts differ on the arc 0 -> 2


def test_the_order_of_the_feeds_is_the_reference_s(ctx):
    """65 arcs of one label over one frame, chosen so that the f32 sum of the reversed feed differs in bits: a kernel that ignores the
    order cannot give both"""
    for seed in range(50):
        rng = np.random.default_rng(seed)
        w = (-np.log(rng.uniform(0.05, 1.0, 65) / 70)).astype(np.float32)
        if wr.cell_score(wr.collect(list(w))) != wr.cell_score(wr.collect(list(w[::-1]))):
            break
    else:
        pytest.fail("no order-sensitive feed among 50 seeds")
    for feed in (w, w[::-1]):
        lat = wr.lattice([0, 1], [(0, 1, 3)] * 65)
        lat["arc_weight"] = np.ascontiguousarray(feed)
        score = run(ctx, "timeframe-error-max", [lat], rows=[(0, 3)])[2][0][1]
        assert abs(float(score[0]) - float(wr.cell_score(wr.collect(list(feed), True), True))) <= 69 * 2.0 ** -23
        same, other = (abs(float(score[0]) - float(wr.cell_score(wr.collect(list(f))))) for f in (feed, feed[::-1]))
        assert same < other, (same, other)   # nearer to its own order's f32 chain than to the reversed one's


@pytest.mark.parametrize("mode", ["timeframe-error-sum", "frame-word-accuracy", "approximate-word"])
def test_a_segment_alone_and_in_two_batches(ctx, mode):
    a, b, c = fan(65, 3, 1), fan(129, 70, 2), fan(1, 1, 3)
    cor = {id(a): fan(40, 1, 4), id(b): fan(129, 2, 5), id(c): fan(64, 1, 6)}
    call = lambda lats: run(ctx, mode, lats, None if mode.startswith("timeframe") else [cor[id(l)] for l in lats], 0.1, (-1,))[0]   # noqa: E731
    alone, n = call([a]), len(a["arc_target"])
    assert np.isfinite(alone).all()
    assert call([b, a, c])[len(b["arc_target"]):][:n].tobytes() == alone.tobytes() and call([c, b, a])[-n:].tobytes() == alone.tobytes()


@pytest.mark.parametrize("T, Tc", [(65, 40), (64, 129), (129, 64), (1, 1)])
def test_accuracy_modes_equal_the_restatement_in_every_bit(ctx, T, Tc):
    lat, cor = fan(T, 3, T), fan(Tc, 2, Tc + 1)
    got, info, _ = run(ctx, "frame-word-accuracy", [lat], [cor], normalization=0.5)
    assert got.tobytes() == wr.frame_word_accuracy(lat, cor, 0.5).tobytes()
    got, info, _ = run(ctx, "approximate-word", [lat], [cor], short_pauses=(-1,))
    assert got.tobytes() == wr.approximate_word(lat, cor, {-1}).tobytes()
    assert info[0]["intervals"] == len({(l, s, e) for _, l, s, e in wr.arcs(cor) if s < e})


def test_refusal_leaves_the_outputs_untouched(ctx):
    import rasr_amd
    import torch
    lat = wr.lattice([0, 70], [(0, 1, 5), (0, 1, 5), (0, 1, 9)])   # two posteriors of 1 on one label: p = -log 2
    assert wr.timeframe_errors(lat, lat["arc_weight"])[1] == (0, 5)
    ctx.use_torch_stream()
    m = rasr_amd.LatticeWordMeasures(ctx, "timeframe-error-sum")
    out = torch.full((3,), 7.0, device="cuda")
    with pytest.raises(rasr_amd.AmxError, match="segment 0, frame 0, label 5"):
        m.run_dev(m.tables([lat]), None, torch.zeros(3, device="cuda"), out)
    assert (out.cpu().numpy() == 7.0).all()


def test_end_to_end_with_the_arc_posteriors(ctx):
    """LatticePosterior("log") -> time-frame errors, and approximate-word -> LatticePosterior("expectation")"""
    import rasr_amd
    ctx.use_torch_stream()
    lat, cor = fan(65, 3, 9), fan(65, 1, 10)
    lat["arc_weight"] = np.random.default_rng(1).uniform(0.5, 3.0, len(lat["arc_target"])).astype(np.float32)
    post = rasr_amd.LatticePosterior(ctx, "log").run([lat])[0]
    m = rasr_amd.LatticeWordMeasures(ctx, "timeframe-error-sum")
    got = m.run([lat], post)[0].cpu().numpy()
    want, bad, _ = wr.timeframe_errors(lat, post.cpu().numpy())
    assert bad is None and np.abs(got - want).max() <= 2 * (65 * 9 + 67 * 65) * 2.0 ** -23   # twice the arc bar for d <= 65, n <= 5, a value <= 65
    risk = rasr_amd.LatticeWordMeasures(ctx, "approximate-word", short_pauses=(-1,)).run([lat], correct=[cor])[0].cpu().numpy()
    assert risk.tobytes() == wr.approximate_word(lat, cor, {-1}).tobytes()
    lat.update(arc_risk=risk, final_risk=np.zeros(5, np.float32))
    _, _, info = rasr_amd.LatticePosterior(ctx, "expectation").run([lat])
    assert -1.0 <= info[0]["expectation"] <= 1.0 and info[0]["expectation"] != 0.0
