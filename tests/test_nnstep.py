"""CPU: NN mini-batch training without a device.

  * tests/nnstep_reference.py (the restatement the GPU tests compare the device with) equals, bit for bit, what the reference's own text
    computed for part (a) of tests/golden/ref_nnstep.npz behind BLAS-backed stand-ins: the two clips, the three regularisers, finalize,
    both estimators with and without activation means, the statistics updates in a contracted and an uncontracted build;
  * its fused multiply-add is exact and differs from
    the two-rounding form and, on planted values, from the route through f64; its clip treats the planted edge values (zeros of both
    signs, values within one step of the threshold, subnormals) as the reference's text does; its trajectories have not drifted from
    tests/golden/ref_nnstep.npz (tests/golden/make_nnstep_golden.py);
  * the host side of librasr_amd.so on a handle without a context: every refusal of amx_nntrain_set_estimator with its message, stepping
    refused, amx_nntrain_get_parameters, MiniBatchTrainer.save;
  * tests/host_nnstep_test.cc, the same host side as a stand-alone program under the host sanitizers.
"""
import os
import subprocess

import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import nnstep_reference as ns
from tests import nntrain_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_nnstep.npz")))
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_fused_multiply_add_is_exact():
    rng = np.random.Generator(np.random.PCG64(5))
    a, x, y = (rng.standard_normal(100000).astype(F32) for _ in range(3))
    got = ns.fma(a, x, y)
    exact = (a.astype(np.longdouble) * x.astype(np.longdouble) + y.astype(np.longdouble)).astype(F32)     # 64-bit mantissa: 48 + 24 bits fit but for far-apart exponents
    two = ((a * x).astype(F32) + y).astype(F32)
    assert (bits(got) != bits(two)).sum() > 1000                      # the inputs tell one rounding from two
    assert (bits(got) != bits(exact)).sum() <= 2                      # and the long double route (itself two roundings) all but never differs
    # a planted double-rounding case of the f64 route: a * x = 1 + 2^-11 + 2^-24 is the middle of two floats, y lifts it above; f64 rounds y away
    a1, x1, y1 = F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12), F32(2.0 ** -60)
    via_f64 = F32(np.float64(a1) * np.float64(x1) + np.float64(y1))
    assert ns.fma(a1, x1, y1) == F32(1 + 2.0 ** -11 + 2.0 ** -23) and via_f64 == F32(1 + 2.0 ** -11)
    assert ns.axpy(2.0, np.array([1.5], F32), np.array([0.25], F32))[0] == 3.25 and ns.fma(a, x, y).dtype == F32
    assert ns.fma(np.zeros((0, 3), F32), 1.0, 1.0).shape == (0, 3)


def test_the_clip_on_planted_edge_values():
    v = F32(0.125)
    tiny, step = F32(1e-42), np.spacing(v)
    w = np.array([0.0, -0.0, v, -v, v + step, -(v + step), v - step, -(v - step), tiny, -tiny, 1.0, -1.0, np.inf, -np.inf], F32)
    got = ns.l1_clip(w, v)
    want = np.array([0.0, -0.0, 0.0, 0.0, step, -step, 0.0, 0.0, 0.0, 0.0, 0.875, -0.875, np.inf, -np.inf], F32)
    assert np.array_equal(bits(got), bits(want)), (got, want)         # zeros keep their sign; what crosses zero becomes +0
    assert np.array_equal(bits(ns.l1_clip(w, 0.0))[2:], bits(w)[2:])  # a zero threshold changes nothing
    assert np.array_equal(ns.sign(np.array([0.0, -0.0, 2.0, -3.0, tiny, -tiny], F32)), np.array([0, 0, 1, -1, 1, -1], F32))


def test_the_regulariser_and_finalize_follow_the_stated_roundings():
    rng = np.random.Generator(np.random.PCG64(6))
    Ws, bs = [rng.standard_normal((5, 3)).astype(F32)], [rng.standard_normal(5).astype(F32)]
    G, g = [rng.standard_normal((3, 5)).astype(F32)], [rng.standard_normal(5).astype(F32)]
    cfg = ns.Cfg(1, regularizer=ns.L2, regularization_constant=[0.3])
    G2, g2 = ns.add_gradient(cfg, Ws, bs, G, g, 129)
    cf = F32(F32(0.3) * F32(129))
    assert np.array_equal(bits(G2[0]), bits(ns.fma(cf, Ws[0].T, G[0]))) and np.array_equal(bits(g2[0]), bits(ns.fma(cf, bs[0], g[0])))
    cen = ns.Cfg(1, regularizer=ns.CENTERED_L2, regularization_constant=[0.3], center=([Ws[0] * F32(0.5)], [bs[0] * F32(0.5)]))
    G3, _ = ns.add_gradient(cen, Ws, bs, G, g, 129)
    assert np.array_equal(bits(G3[0]), bits(ns.fma(-cf, (Ws[0] * F32(0.5)).T, ns.fma(cf, Ws[0].T, G[0]))))
    off = ns.Cfg(1, regularizer=ns.L2, regularization_constant=[0.3], trainable=[0])
    assert np.array_equal(bits(ns.add_gradient(off, Ws, bs, G, g, 129)[0][0]), bits(G[0]))            # a layer that is not trainable takes none
    assert ns.regularizer_objective(off, Ws, bs, 129, "f64") == 0
    Gf, gf, (o,) = ns.finalize(cfg, G, g, [F32(7.5)], 129)
    s = F32(1.0 / np.float64(F32(129)))
    assert np.array_equal(bits(Gf[0]), bits(G[0] * s)) and o == F32(np.float64(F32(7.5)) * (1.0 / 129.0))
    assert np.array_equal(bits(ns.finalize(cfg, G, g, [F32(7.5)], 1)[0][0]), bits(G[0]))                 # a weight of 1 scales nothing
    # the quirk: without a predecessor the first layer's weights stay, its bias moves
    q = ns.Cfg(1, learning_rate=0.5, update_input_layer_weights=False)
    W1, b1, steps = ns.estimate(q, Ws, bs, G, g)
    assert np.array_equal(bits(W1[0]), bits(Ws[0])) and not np.array_equal(bits(b1[0]), bits(bs[0]))
    assert steps[0] == F32(ns.asum(g[0], "f64") * F32(0.5))
    W2, _, _ = ns.estimate(q, Ws, bs, G, g, has_preprocessing=True)
    assert np.array_equal(bits(W2[0]), bits(ns.fma(F32(-0.5), G[0].T, Ws[0])))


def test_the_stored_trajectories_reproduce():
    for key in ns.TRAJECTORIES:
        tr, batches = ns.trajectory(key)
        objective = []
        for i, (x, e, w) in enumerate(batches):
            info = tr.step(x, e, w)
            assert info["updated"] == ((i + 1) % tr.cfg.A == 0)
            if not info["updated"]:
                continue
            objective.append(info["objective"])
            step = (i + 1) // tr.cfg.A
            if step in ns.TRAJECTORY_STEPS:
                for l in range(tr.L):       # f64 sums in the order of the BLAS at hand: within the bar the fixture stores for this very array
                    for p, got in (("W", tr.net.Ws[l]), ("b", tr.net.bs[l])):
                        want, bar = FX["traj/%s/%d/%s%d" % (key, step, p, l)], FX["bar_traj/%s/%d/%s%d" % (key, step, p, l)][0]
                        assert np.abs(got.astype(np.float64) - want).max() <= bar * np.abs(want).max(), (key, step, p, l)
        want = FX["traj_objective/" + key].astype(np.float64)
        assert np.abs(np.array(objective, np.float64) - want).max() <= FX["bar_traj_objective/" + key][0] * np.abs(want).max()
        assert objective[-1] < objective[0]


# ------------------------------------------------------------------------------------ the reference's own text (fixture part (a))
A_DIMS = [5, 4, 3]


def a_split(flat, gradient):
    """flat -> per layer W [out, in] (gradient: G [in, out]) and the bias, as the generator laid them out"""
    Ws, bs, off = [], [], 0
    for i, o in zip(A_DIMS[:-1], A_DIMS[1:]):
        W = flat[off:off + i * o].reshape(o, i)
        off += i * o
        Ws.append(W.T.copy() if gradient else W.copy())
        bs.append(flat[off:off + o].copy())
        off += o
    return Ws, bs


def a_flat(Ws, bs, gradient):
    return np.concatenate([np.concatenate([(W.T if gradient else W).reshape(-1), b]) for W, b in zip(Ws, bs)]).astype(F32)


def test_the_clip_equals_the_reference_bit_for_bit():
    w = FX["a/clip_in"]
    for k, v in enumerate(FX["a/clip_value"]):
        assert np.array_equal(bits(ns.l1_clip(w, v)), bits(FX["a/clip_vector%d" % k])), v
        assert np.array_equal(bits(ns.l1_clip(w, v)), bits(FX["a/clip_matrix%d" % k])), v


def test_regularisers_and_finalize_equal_the_reference_bit_for_bit():
    for tag in ("random", "dyadic"):
        Ws, bs = a_split(FX["a/%s/par" % tag], False)
        Gs, gs = a_split(FX["a/%s/grad" % tag], True)
        center = a_split(FX["a/%s/center" % tag], False)
        for kind in (ns.L1, ns.L2, ns.CENTERED_L2):
            for tr_tag, tr in (("", [1, 1]), ("_frozen1", [1, 0])):
                cfg = ns.Cfg(2, regularizer=kind, regularization_constant=FX["a/%s/c" % tag], trainable=tr, center=center)
                G2, g2 = ns.add_gradient(cfg, Ws, bs, Gs, gs, 24)
                assert np.array_equal(bits(a_flat(G2, g2, True)), bits(FX["a/%s/reg%d%s_grad" % (tag, kind, tr_tag)])), (tag, kind, tr_tag)
                if tag == "dyadic":     # every sum of this case is exact in f32, whatever its order
                    for sums in ("f64", "f32"):
                        assert ns.regularizer_objective(cfg, Ws, bs, 16, sums) == FX["a/dyadic/reg%d%s_objective" % (kind, tr_tag)][0], (kind, tr_tag)
        for n_obs, normalize in ((129, 1), (1, 1), (129, 0), (16, 1)):
            cfg = ns.Cfg(2, normalize_by_observations=bool(normalize))
            Gf, gf, (o,) = ns.finalize(cfg, Gs, gs, [F32(7.5)], n_obs)
            assert np.array_equal(bits(a_flat(Gf, gf, True)), bits(FX["a/%s/finalize_%d_%d_grad" % (tag, n_obs, normalize)])), (tag, n_obs, normalize)
            assert bits(o) == bits(FX["a/%s/finalize_%d_%d_objective" % (tag, n_obs, normalize)])[0]


def test_both_estimators_equal_the_reference_bit_for_bit():
    for tag in ("random", "dyadic"):
        Ws, bs = a_split(FX["a/%s/par" % tag], False)
        mean0 = ns.fma(F32(1.0 / 4), FX["a/%s/act_sum0" % tag], np.zeros(5, F32))       # smoothing none, 4 observations
        mean1 = ns.fma(F32(1.0), FX["a/%s/act_sum1" % tag], np.zeros(4, F32))           # a trace: nObservations counts as 1
        for clipping in (0, 1):
            for case, n_pred, stats, tr in (("plain", [1, 1], [0, 0], [1, 1]), ("nopred", [0, 1], [0, 1], [1, 1]), ("means", [1, 1], [1, 1], [1, 1]),
                                            ("frozen", [1, 1], [1, 1], [0, 1])):
                Gs, gs = a_split(FX["a/%s/grad" % tag], True)
                cfg = ns.Cfg(2, learning_rate=0.25, bias_learning_rate=0.5, layer_learning_rate=[0.5, 2.0], regularization_constant=FX["a/%s/c" % tag], trainable=tr,
                             estimator=clipping, update_input_layer_weights=bool(n_pred[0]))
                means = [m if on else None for m, on in zip((mean0, mean1), stats)]
                W1, b1, steps = ns.estimate(cfg, Ws, bs, Gs, gs, "f32", means=means)
                key = "a/%s/estimate%d_%s" % (tag, clipping, case)
                wantW, wantb = a_split(FX[key + "_par"], False)
                wantG, wantg = a_split(FX[key + "_grad"], True)
                for l in range(2):
                    assert np.array_equal(bits(W1[l]), bits(wantW[l])) and np.array_equal(bits(Gs[l]), bits(wantG[l])), (key, l)      # element-wise: exact
                    if tag == "dyadic" or means[l] is None or not tr[l]:    # behind the gemv only where a mean enters: exact when its sums are
                        assert np.array_equal(bits(b1[l]), bits(wantb[l])) and np.array_equal(bits(gs[l]), bits(wantg[l])), (key, l)
                if tag == "dyadic":
                    assert np.array_equal(bits(steps), bits(FX[key + "_steps"])), key
        assert not np.array_equal(FX["a/%s/estimate0_means_par" % tag], FX["a/%s/estimate0_plain_par" % tag])


def test_activation_statistics_equal_both_builds_of_the_reference_bit_for_bit():
    frames, Y = FX["a/stat_frames"], FX["a/stat_Y"]
    for contract, c in (("fma", ns.CONTRACT_FMA), ("off", ns.CONTRACT_OFF)):
        for mode, name in ((ns.STAT_NONE, "none"), (ns.EXPONENTIAL_TRACE, "trace")):
            for nb in (1, 3):
                st, off = ns.ActStat(mode, 0.75, 6), 0
                for T in frames[:nb]:
                    st.update(Y[off:off + T], np.arange(T), c)
                    off += T
                key = "a/stat_%s_%s_%d/" % (contract, name, nb)
                for what, got in (("sum", st.sum), ("sumsq", st.sumsq), ("mean", st.mean()), ("variance", st.variance())):
                    assert np.array_equal(bits(got), bits(FX[key + what])), key + what
                assert (1 if mode == ns.EXPONENTIAL_TRACE else st.nobs) == (1 if mode == ns.EXPONENTIAL_TRACE else FX[key + "n_obs"][0])
    # a chain over more than one chunk: the device's rule differs from the reference's one chain, which the fixture bars
    st, one = ns.ActStat(ns.STAT_NONE, 0.5, 6), ns.ActStat(ns.STAT_NONE, 0.5, 6)
    big = np.tile(Y[:150], (2, 1))
    st.update(big, np.arange(300))
    one.update(big, np.arange(300), single_chain=True)
    assert not np.array_equal(bits(st.sum), bits(one.sum)) or not np.array_equal(bits(st.sumsq), bits(one.sumsq))


def host_trainer():
    net, _, _, _ = nr.variant("b", (nr.TANH,), 4, 1)
    return net, rasr_amd.MiniBatchTrainer(None, net.Ws, net.bs, net.acts)


def test_host_only_handle_refusals_and_read_back(tmp_path):
    net, tr = host_trainer()
    tr.set_estimator(learning_rate=0.5, regularizer="l2", regularization_constant=[0.1, 0.0])
    for kw, word in ((dict(regularization_constant=[0.1, -0.5]), "regularization_constant[1]"), (dict(accumulate_multiple_batches=0), "accumulate_multiple_batches"),
                     (dict(learning_rate=float("nan")), "learning_rate"), (dict(layer_learning_rate=[1.0, float("inf")]), "layer_learning_rate[1]"),
                     (dict(regularizer=7), "regularizer"), (dict(estimator=5), "estimator"), (dict(regularizer="centered-l2"), "center")):
        with pytest.raises(rasr_amd.AmxError) as err:
            tr.set_estimator(**kw)
        assert err.value.status == _lib.AMX_ERR_INVALID and word in str(err.value), (kw, str(err.value))
    wrong = ([net.Ws[0], net.Ws[1][:-1]], [net.bs[0], net.bs[1][:-1]])
    with pytest.raises(rasr_amd.AmxError) as err:
        tr.set_estimator(regularizer="centered-l2", center=wrong)
    assert err.value.status == _lib.AMX_ERR_INVALID and "layer 1" in str(err.value) and "130 -> 128" in str(err.value)
    tr.set_estimator(regularizer="centered-l2", center=(net.Ws, net.bs), regularization_constant=[0.1, 0.1])
    # a handle without a context cannot step
    x = np.zeros((4, 7), np.float32)
    for call in (lambda: tr.step_dev(x, 7, 4, np.zeros(4, np.uint32)), lambda: tr.step_accumulate_dev(x, 7, 4, np.zeros(4, np.uint32)), tr.step_estimate_dev,
                 tr.step_info, tr.step_statistics, lambda: tr.estimate(np.zeros(tr.accumulator_size()))):
        with pytest.raises(rasr_amd.AmxError) as err:
            call()
        assert err.value.status == _lib.AMX_ERR_STATE and "without a context" in str(err.value)
    # no network, or other statistics than base + gradient: no estimator
    bare = rasr_amd.FeedForwardTrainer(None, statistics=("class-counts",), n_outputs=3)
    cfg = _lib.NnStepCfg()
    _lib.lib().amx_nnstep_default_cfg(cfg)
    assert (cfg.learning_rate, cfg.bias_learning_rate, cfg.regularizer, cfg.estimator, cfg.accumulate_multiple_batches, cfg.normalize_by_observations,
            cfg.log_step_size, cfg.update_input_layer_weights) == (1.0, 1.0, 0, 0, 1, 1, 0, 1)
    assert _lib.lib().amx_nntrain_set_estimator(bare.h, cfg) == _lib.AMX_ERR_INVALID and b"no network" in _lib.lib().amx_last_error()
    more = rasr_amd.MiniBatchTrainer(None, net.Ws, net.bs, net.acts, statistics=("base", "gradient", "class-counts"))
    with pytest.raises(rasr_amd.AmxError, match="nothing else"):
        more.set_estimator()
    # read-back: what was put in, in both images; save writes [out x (1 + in)] with the bias in column 0
    for image in (0, 1):
        for (W, b), W0, b0 in zip(tr.parameters(image), net.Ws, net.bs):
            assert np.array_equal(bits(W), bits(W0)) and np.array_equal(bits(b), bits(b0))
    with pytest.raises(rasr_amd.AmxError, match="image"):
        tr.parameters(2)
    paths = tr.save(str(tmp_path / "net"))
    assert [os.path.basename(p) for p in paths] == ["net-layer-1.bin", "net-layer-2.bin"]
    for p, W0, b0 in zip(paths, net.Ws, net.bs):
        m = rasr_amd.read_nn_matrix(p)
        assert m.shape == (W0.shape[0], 1 + W0.shape[1])
        W, b = rasr_amd.layer_from_parameters(m)
        assert np.array_equal(bits(W), bits(W0)) and np.array_equal(bits(b), bits(b0))
    assert "MiniBatchTrainer" in rasr_amd.__all__ and issubclass(rasr_amd.MiniBatchTrainer, rasr_amd.FeedForwardTrainer)


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_nnstep_test.cc compiles the host side of nntrain.hip and nnstep.hip into a program of its own: the configuration's
    refusals, the defaults, read-back on a host-only handle, the narrowing of a flat buffer, the info struct; built with
    -fsanitize=address,undefined on the host side only, run as a process of its own (nothing sanitized is loaded into Python).  Sanitizers
    are for machines without a GPU: where one is present the same program is built and run plainly."""
    import torch
    exe = str(tmp_path / "host_nnstep_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_nnstep_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_nnstep_test: ok" in r.stdout, r.stdout + r.stderr
