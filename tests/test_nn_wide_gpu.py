"""GPU: NN training statistics (nntrain.hip, the f32 GEMM and softmax of ffnn_f32.hpp) and the mini-batch step (nnstep.hip) on the wide
networks and long calls of tests/nn_wide_cases.py, through rasr_amd.FeedForwardTrainer / MiniBatchTrainer against the plain restatements
of tests/nntrain_reference.py and tests/nnstep_reference.py.

Shapes.  W = 300-40-260-700, D = 1030-1100 (one layer) and, for the cap alone, 24-40-33-50; T = 513, 768, 1000 and 4096.  What they reach
that tests/test_nntrain_gpu.py and tests/test_nnstep_gpu.py do not: second and later trips of every 256-strided loop (the softmax, the
arg-max with its cross-wave tie rule, the column sums, the tile and segment sums of the step), 128-tile grids of 3 x 1, 1 x 3 and 3 x 6,
three to sixteen frame chunks, the cap of 4096 frames from both sides, a network without a backward GEMM.  tests/nn_wide_cases.py says
how the labels are made and which conditions the inputs meet; tests/test_nn_wide.py asserts those conditions and that a defect planted
at each of these places leaves the bars used here.

Bars.  Counts, observations, classification errors and the total weight are exact; so is every element-wise result of the step given
the inputs read back from the device.  What lies behind a sum is held to 4 x the distance between the restatement with f32 sums and with
f64 sums, relative to the block's largest magnitude, per network and block the worst over the network's cases as the two golden makers
take it, both evaluated on the CPU inside the test (tests/nn_wide_cases.py); none is written here and nothing is taken from the device.
Every comparison prints the device's distance as a fraction of its bar.
"""
import numpy as np
import pytest

from tests import nn_wide_cases as wc
from tests import nnstep_reference as ns
from tests import nntrain_reference as nr
from tests.test_nnstep_gpu import bits, images_agree, read, same, upload
from tests.test_nnstep_gpu import trainer as step_trainer
from tests.test_nntrain_gpu import run
from tests.test_nntrain_gpu import trainer as stat_trainer

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ALL = wc.ALL


def held(what, block, got, want, bar):
    """a block against its bar, relative to the reference's largest magnitude; prints distance / bar"""
    want = np.asarray(want, F64)
    dev, allowed = float(np.abs(np.asarray(got, F64) - want).max()), bar * float(np.abs(want).max())
    print("%-20s %-22s distance / bar = %.3g / %.3g = %.3f" % (what, block, dev, allowed, dev / allowed))
    assert dev <= allowed, (what, block, dev, allowed)


def check(tr, got, want, bar, what):
    s = tr.statistics(got)
    assert s["n_observations"] == want["n_observations"], what
    assert np.array_equal(s["class_counts"], want["class_counts"]), what
    assert s["n_classification_errors"] == want["n_classification_errors"], what
    assert s["total_weight"] == want["total_weight"], what
    held(what, "objective", s["objective"], want["objective"], bar["objective"])
    n_layers = len(want["gradient_weights"])
    got_blocks, want_blocks = wc.blocks(s, n_layers), wc.blocks(want, n_layers)
    for block in want_blocks:
        assert got_blocks[block].shape == want_blocks[block].shape, (what, block)
        held(what, block, got_blocks[block], want_blocks[block], bar[block])


# ------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("key", sorted(wc.CASES))
def test_every_wide_case_against_the_restatement(ctx, key):
    net, x, e, w = wc.case(key)
    tr = stat_trainer(ctx, net)
    lay, y = nr.layout(net.dims, net.dims[0], net.dims[-1], ALL), tr.layout
    assert tr.accumulator_size() == lay["size"] == y.size
    assert [y.gradient_weights[l] for l in range(tr.n_layers)] == lay["gradient_weights"] and [y.gradient_bias[l] for l in range(tr.n_layers)] == lay["gradient_bias"]
    assert (y.feature_sum, y.feature_square_sum, y.class_counts, y.tail) == (lay["feature_sum"], lay["feature_square_sum"], lay["class_counts"], lay["tail"])
    check(tr, run(tr, x, e, w), wc.evaluation(key), wc.bars(key), key)
    tr.close()


def test_a_wide_buffer_is_written_as_the_reference_writes_it(ctx, tmp_path):
    net, x, e, w = wc.case("W-T513")
    tr = stat_trainer(ctx, net)
    a = run(tr, x, e, w)
    path = str(tmp_path / "wide.stat")
    tr.write(a, path)
    d = net.dims
    with open(path, "rb") as f:
        assert f.read() == nr.statistics_bytes(a, d, d[0], d[-1], ALL)
    assert np.array_equal(tr.read(path), nr.narrowed(a, d, d[0], d[-1], ALL))
    tr.close()


def test_ties_across_trips_and_waves_and_a_vanished_probability(ctx):
    """700 outputs, pairs of identical rows and biases in the top layer, each pair in turn holding every frame's maximum: the two softmax
    values are the same bits, argMax answers the smaller index whichever trip, lane or wave saw the other one.  (300, 556): one thread
    on two trips; (600, 650): two waves of the third trip; (5, 517): trips 0 and 2."""
    T = wc.TIE_T
    for k, (i, j) in enumerate(wc.TIE_PAIRS):
        net, x = wc.tie_network(k)
        tr = stat_trainer(ctx, net)
        for label, errors in ((j, T), (i, 0)):
            e = np.full(T, label, np.uint32)
            want = nr.accumulate(net, x, e, None, mask=ALL)
            p = want["softmax"]
            assert np.array_equal(bits(p[:, i]), bits(p[:, j])) and np.array_equal(p[:, i], p.max(axis=1))       # the premise, on the restatement
            s = tr.statistics(run(tr, x, e, None))
            assert s["n_classification_errors"] == errors == want["n_classification_errors"], (i, j, label)
            assert s["n_observations"] == T and s["total_weight"] == float(T)
        tr.close()
    net, x = wc.tie_network(0, vanish=650)     # exp(-200 - the maximum) is 0 in f32: p[650] = 0
    tr = stat_trainer(ctx, net, mask=nr.BASE)
    s = tr.statistics(run(tr, x, np.full(T, 650, np.uint32), None))
    assert s["objective"] == np.inf and s["n_classification_errors"] == T
    tr.close()


def test_the_cap_from_both_sides(ctx):
    """4096 frames are a call (W-T4096 above holds it to the bars); 4097 are refused with the buffer untouched and the handle usable;
    two calls of 2048 frames into one buffer equal the sum of two buffers"""
    import torch

    import rasr_amd
    net, x, e, w = wc.case("W-T4096")
    assert len(e) == wc.MAX_FRAMES == rasr_amd._lib.AMX_NNTRAIN_MAX_FRAMES
    tr = stat_trainer(ctx, net)
    acc = torch.arange(tr.accumulator_size(), dtype=torch.float64, device="cuda") * 0.5 + 1.0
    before = acc.cpu().numpy()
    with pytest.raises(rasr_amd.AmxError) as err:
        run(tr, np.concatenate([x, x[:1]]), np.concatenate([e, e[:1]]), None, acc)
    assert err.value.status == rasr_amd._lib.AMX_ERR_INVALID and "4097" in str(err.value)
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), before)
    first, second = run(tr, x[:2048], e[:2048], None), run(tr, x[2048:], e[2048:], None)
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    run(tr, x[:2048], e[:2048], None, acc)
    both = run(tr, x[2048:], e[2048:], None, acc)
    assert np.array_equal(both, first + second)
    assert tr.statistics(both)["n_observations"] == wc.MAX_FRAMES
    tr.close()


def test_three_chunks_give_the_same_bits_whatever_ran_before(ctx):
    net, x, e, w = wc.case("W-T768")
    _, lx, le, _ = wc.case("W-T4096")       # the same dimensions: a call of the cap through the same handle
    tr = stat_trainer(ctx, net)
    first = run(tr, x, e, w)
    run(tr, x[:31], e[:31], None)                                       # after a call below one tile
    assert np.array_equal(run(tr, x, e, w), first)
    run(tr, lx, le, None)                                               # after a call of the cap: the workspaces grew
    assert np.array_equal(run(tr, x, e, w), first)
    fresh = stat_trainer(ctx, net)
    assert np.array_equal(run(fresh, x, e, w), first)
    fresh.close()
    tr.close()


# ------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("T", [513, 768])
def test_step_accumulate_equals_the_existing_pass_on_three_chunks(ctx, T):
    import torch
    dims, acts = wc.NETS["W"]
    net, x, e, w = nr.variant(dims, acts, T, 40 + T, frame_weights=True, class_weights=True, disregard=True, clip=0.02)
    tr = step_trainer(ctx, net, ns.Cfg(len(net.Ws)))
    args = upload(x, e, w)
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    tr.accumulate_dev(args[0], args[1], args[2], args[3], acc, args[4])
    torch.cuda.synchronize()
    want = tr.statistics(acc)
    tr.step_accumulate_dev(*args)
    info = tr.step_info()
    for l, (G, g) in enumerate(tr.step_statistics()):
        assert np.array_equal(G.astype(F64), want["gradient_weights"][l]), (T, l)      # the call's f32 total, widened: every bit
        assert np.array_equal(g.astype(F64), want["gradient_bias"][l]), (T, l)
    assert info["n_observations"] == want["n_observations"] and info["n_classification_errors"] == want["n_classification_errors"]
    assert info["total_weight"] == F32(want["total_weight"]) and info["criterion_objective"] == F32(want["objective"])
    tr.close()


def means_of(tr, cfg, L):
    """the activation mean of what feeds each layer, as the device holds it (None where that keeps no statistics)"""
    if all(m == ns.NO_STATISTICS for m in cfg.stat_mode):
        return [None] * L
    stats = tr.activation_statistics()
    return [stats[p - 1][0] if p - 1 in stats else None for p in range(L)]


def check_estimate(key, cfg, L, inputs, outputs, means, what, bars):
    """one estimator step on the read-back inputs (Ws, bs, finalized Gf, gf) against the device's outputs (Ws1, bs1, Gs1, gs1): the
    outer-product term, both weight images' content and the biases in every bit; the bias term behind the gemv to its bar"""
    Ws, bs, Gf, gf = inputs
    Ws1, bs1, Gs1, gs1 = outputs
    plain = [G.copy() for G in Gf]
    Wr, br, _ = ns.estimate(cfg, Ws, bs, Gf, gf, means=means)       # Gf, gf become the update terms
    for l in range(L):
        assert same(Gs1[l], Gf[l]) and same(Ws1[l], Wr[l]), (key, what, l)
        assert not same(Ws1[l], Ws[l]), (key, what, l)
        if means[l] is None:
            assert same(gs1[l], gf[l]) and same(bs1[l], br[l]), (key, what, l)
            continue
        assert not same(Gs1[l], plain[l]), (key, what, l)            # the mean did enter
        held("%s %s" % (key, what), "bias term/%d" % l, gs1[l], gf[l], bars["bias term/%d" % l])
        b = ns.axpy(-F32(F32(cfg.eta * cfg.eta_bias) * cfg.eta_l[l]), gs1[l], bs[l])
        if cfg.estimator == ns.SGD_L1_CLIPPING:
            b = ns.l1_clip(b, F32(F32(cfg.c[l] * cfg.eta) * cfg.eta_l[l]))
        assert same(bs1[l], b), (key, what, l)


@pytest.mark.parametrize("key", sorted(wc.STEP_CASES))
def test_the_wide_update_is_exact(ctx, key):
    import rasr_amd
    import torch
    ref, x, e, w = wc.step_case(key)
    cfg, L, bars = ref.cfg, ref.L, wc.step_bars(wc.STEP_CASES[key]["net"])
    tr = step_trainer(ctx, ref.net, cfg)
    args = upload(x, e, w)
    tr.step_accumulate_dev(*args)
    Ws, bs, Gs, gs = read(tr)
    before = tr.step_info()
    n = before["n_observations"]
    assert n == len(e) and all(same(W, W0) and same(b, b0) for W, W0, b, b0 in zip(Ws, ref.net.Ws, bs, ref.net.bs))
    means = means_of(tr, cfg, L)
    assert [m is not None for m in means] == [mode != ns.NO_STATISTICS for mode in cfg.stat_mode]
    # the regulariser's objective on the read-back parameters
    reg = ns.regularizer_objective(cfg, Ws, bs, n, "f64")
    held(key, "regulariser objective", float(before["objective"]) - float(before["criterion_objective"]), float(reg), bars["regulariser objective"])
    tr.step_estimate_dev()
    out1 = read(tr)
    after = tr.step_info()
    Gf, gf, (of, cf) = ns.finalize(cfg, Gs, gs, [before["objective"], before["criterion_objective"]], n)
    check_estimate(key, cfg, L, (Ws, bs, Gf, gf), out1, means, "step 1", bars)
    assert images_agree(tr)
    assert after["updated"] and bits(F32(after["objective"])) == bits(of) and bits(F32(after["criterion_objective"])) == bits(cf)
    for l in range(L):      # the step sizes: the two asums of the update terms as the device holds them
        held(key, "step size/%d" % l, after["step_size"][l], wc.step_size_parts(cfg, l, out1[2][l], out1[3][l], "f64"), bars["step size/%d" % l])
    # a second estimate on the finalized group scales nothing again and steps once more
    tr.step_estimate_dev()
    out2 = read(tr)
    check_estimate(key, cfg, L, (out1[0], out1[1], [G.copy() for G in out1[2]], [g.copy() for g in out1[3]]), out2, means, "step 2", bars)
    assert images_agree(tr)
    # nothing was written into the padding of either weight image: a FRESH handle on the read-back parameters gives the stepped handle's
    # next gradient in every bit (a padded sigmoid unit outputs 0.5, a padded weight would meet it in the stepped handle's GEMMs alone)
    fresh = rasr_amd.FeedForwardTrainer(ctx, out2[0], out2[1], ref.net.acts)
    acc = torch.zeros(fresh.accumulator_size(), dtype=torch.float64, device="cuda")
    fresh.accumulate_dev(args[0], args[1], args[2], args[3], acc, args[4])
    torch.cuda.synchronize()
    want = fresh.statistics(acc)
    tr.set_estimator()      # no regulariser; the parameters stay
    tr.step_accumulate_dev(*args)
    for l, (G, g) in enumerate(tr.step_statistics()):
        assert np.array_equal(G.astype(F64), want["gradient_weights"][l]), (key, l)
        assert np.array_equal(g.astype(F64), want["gradient_bias"][l]), (key, l)
    fresh.close()
    tr.close()


def test_a_group_of_two_wide_minibatches(ctx):
    key = "W-l2-sgd"
    ref, x, e, w = wc.step_case(key)
    r32, _, _, _ = wc.step_case(key, "f32")
    cfg, L = ref.cfg, ref.L
    cfg.A = r32.cfg.A = 2
    batches = [(x, e, w), (x[::-1].copy(), e[::-1].copy(), w[::-1].copy())]
    tr = step_trainer(ctx, ref.net, cfg)
    zero = lambda ms: [np.zeros_like(m) for m in ms]      # noqa: E731
    add = lambda ps, qs: [(p + q).astype(F32) for p, q in zip(ps, qs)]      # noqa: E731
    for i, (bx, be, bw) in enumerate(batches):
        args = upload(bx, be, bw)
        before = read(tr)
        single = step_trainer(ctx, nr.Net(before[0], before[1], ref.net.acts), ns.Cfg(L))      # one call's gradient bits: a group of one, no regulariser
        single.step_accumulate_dev(*args)
        _, _, Gc, gc = read(single)
        single.close()
        if i == 0:
            info = tr.step_dev(*args)
            assert info["minibatch"] == 1 and not info["updated"] and info["n_observations"] == len(be)
        else:
            tr.step_accumulate_dev(*args)
            info = tr.step_info()
            assert info["minibatch"] == 2 and info["n_observations"] == len(batches[0][1]) + len(be)
        after = read(tr)
        assert all(same(p, q) for p, q in zip(after[0] + after[1], before[0] + before[1]))      # no parameter bit changes before the estimate
        # the regulariser's factor is the group's running count: G = fmaf(c * n_running, W, G_before + call)
        Gr, gr = ns.add_gradient(cfg, before[0], before[1], add(zero(Gc) if i == 0 else before[2], Gc), add(zero(gc) if i == 0 else before[3], gc), info["n_observations"])
        assert all(same(p, q) for p, q in zip(after[2] + after[3], Gr + gr)), i
        for r in (ref, r32):
            r.step_accumulate(bx, be, bw)
    # the group's gradient against the restatement's own: another sum, its bar
    for l in range(L):
        for block, got, a, b in (("group gradient/%d" % l, after[2][l], ref.G[l], r32.G[l]), ("group bias gradient/%d" % l, after[3][l], ref.g[l], r32.g[l])):
            bar = wc.FACTOR * wc.rel(b, a)
            assert bar > 0
            held(key, block, got, a, bar)
    means = means_of(tr, cfg, L)
    tr.step_estimate_dev()
    done = tr.step_info()
    assert done["updated"] and done["minibatch"] == 2
    Gf, gf, _ = ns.finalize(cfg, after[2], after[3], [0.0], done["n_observations"])
    check_estimate(key, cfg, L, (after[0], after[1], Gf, gf), read(tr), means, "group of two", wc.step_bars("W"))
    assert images_agree(tr)
    tr.close()


@pytest.mark.parametrize("contract", ["fma", "off"])
def test_activation_statistics_over_three_chunks(ctx, contract):
    """513 frames: the chain over the first 256 frames starts from the sum, the second and the third chunk's from zero, chunk totals
    added ascending -- exact in the library's order on the layer inputs read back; against the reference's one chain within 4 x the
    distance the restatement measures between the two orders on its own layer inputs"""
    key = "W-l2-sgd"      # an exponential trace on the first hidden layer (40 units), smoothing none on the second (260: two blocks of units)
    c = ns.CONTRACT_FMA if contract == "fma" else ns.CONTRACT_OFF
    before = ctx.contract()      # the session's context is shared: it goes back to what it was
    ctx.set_contract(contract)
    try:
        ref, x, e, w = wc.step_case(key)
        T = len(e)
        tr = step_trainer(ctx, ref.net, ref.cfg)
        one = [None if st is None else ns.ActStat(st.mode, st.f, st.n) for st in ref.stats]
        bar = {}
        Xs, idx = ref.layer_inputs(x, e)
        for p, st in enumerate(ref.stats):
            if st is None:
                continue
            lib, chain = ns.ActStat(st.mode, st.f, st.n), ns.ActStat(st.mode, st.f, st.n)
            lib.update(Xs[p], idx, c)
            chain.update(Xs[p], idx, c, single_chain=True)
            bar[p] = wc.FACTOR * max(wc.rel(lib.sum, chain.sum), wc.rel(lib.sumsq, chain.sumsq))
            assert bar[p] > 0
        assert sorted(bar) == [1, 2]
        for batch in range(2):      # the second batch continues the sums (and, for the trace, is no first batch)
            bx = x if batch == 0 else x[::-1].copy()
            tr.step_accumulate_dev(*upload(bx, e, w))
            keep, _, _ = nr.labels(e, ref.net.class_to_output, ref.net.class_weights, None)
            where = np.nonzero(keep)[0]
            got = tr.activation_statistics()
            assert sorted(got) == [p - 1 for p in sorted(bar)]
            for p in sorted(bar):
                X = tr.layer_input(p, T)[keep]
                ref.stats[p].update(X, where, c)
                one[p].update(X, where, c, single_chain=True)
                mean, var = got[p - 1]
                assert same(mean, ref.stats[p].mean()) and same(var, ref.stats[p].variance()), (contract, batch, p)
                held("%s %s batch %d" % (key, contract, batch), "one chain mean/%d" % (p - 1), mean, one[p].mean(), bar[p])
        tr.close()
    finally:
        ctx.set_contract(before)
