"""CPU: the NN training statistics without a device.

  * tests/nntrain_reference.py (the restatement the GPU tests compare the device with) equals, bit for bit, what the reference's own
    element-wise functions computed for tests/golden/ref_nntrain.npz (tests/golden/make_nntrain_golden.py), and its whole pass has not
    drifted from the buffers stored there;
  * the restatement's gradient equals central finite differences of its own f64 objective: a misreading shared by the device code and
    the restatement would not survive this;
  * the host side of librasr_amd.so against the fixture: amx_nnstat_write reproduces the bytes the reference's Statistics<f32>::write
    emitted under each flag mask, amx_prior_from_class_counts and amx_nnstat_mean_and_deviation equal the reference's setFromClassCounts and
    finalize in every bit; read, combine and the layout against the restatement (which equals the same fixture), and every refusal;
  * tests/host_nntrain_test.cc, the same host side as a stand-alone program under the host sanitizers.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import nntrain_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_nntrain.npz")))
ALL = nr.CLASS_COUNTS | nr.MEAN_AND_VARIANCE | nr.BASE | nr.GRADIENT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_element_wise_functions_equal_the_reference_bit_for_bit():
    e, y = FX["ew_e"], FX["ew_y"]
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(nr.sigmoid_derivative(e, y)), bits(FX["ew_sigmoid"]))
        assert np.array_equal(bits(nr.tanh_derivative(e, y)), bits(FX["ew_tanh"]))
        assert np.array_equal(bits(nr.rectified_derivative(e, y)), bits(FX["ew_rectified"]))
        for i, c in enumerate(FX["clip_c"]):
            assert np.array_equal(bits(nr.clip(e, c)), bits(FX["ew_clip%d" % i])), c
    assert FX["ew_differs_from_f32"].min() > 100     # the inputs tell a double product from an f32 one


def test_criterion_equals_the_reference_bit_for_bit():
    p, label, w = FX["cr_p"], FX["cr_label"].astype(np.int64), FX["cr_w"]
    am = nr.arg_max(p)
    assert np.array_equal(am, FX["cr_argmax"])
    assert am[0] == 0 and am[1] == 7 and am[2] == 0 and am[3] == 0 and am[4] == 0 and am[5] != 0    # the planted rows
    assert int((am != label).sum()) == int(FX["cr_errors"][0])
    assert np.array_equal(bits(nr.kronecker(p, label)), bits(FX["cr_kronecker"]))
    rows = FX["cr_finite_rows"]
    ones = np.ones(len(rows), np.float32)
    assert bits(nr.seq_sum_f32(nr.objective_terms(p[rows], label[rows], ones), 0)) == bits(FX["cr_ce"])[0]
    assert bits(nr.seq_sum_f32(nr.objective_terms(p[rows], label[rows], w[rows]), 0)) == bits(FX["cr_wce"])[0]
    rows = np.arange(6, len(p))
    assert nr.seq_sum_f32(nr.objective_terms(p[rows], label[rows], w[rows]), 0) == np.inf == FX["cr_wce_with_zero"][0]


def test_the_whole_pass_has_not_drifted_from_the_fixture():
    keys = [k[len("whole_f64/"):] for k in FX if k.startswith("whole_f64/")]
    assert len(keys) == 4
    for key in keys:
        net, x, e, w = nr.variant(**nr.gpu_cases()[key])
        for products in ("f64", "f32"):
            s = nr.accumulate(net, x, e, w, mask=ALL, products=products)
            a = nr.flat(s, net.dims, net.dims[0], net.dims[-1], ALL)
            want = FX["whole_%s/%s" % (products, key)]
            if products == "f64":
                assert np.allclose(a, want, rtol=1e-12, atol=0), key       # f64 sums in the order of the BLAS at hand
            else:   # an sgemm's order is its own: within the bars that the fixture derives from this very evaluation
                assert np.abs(a - want).max() <= max(v[0] for k, v in FX.items() if k.startswith("bar_")) * np.abs(want).max(), key
            assert np.array_equal(a[-4:-1:2], want[-4:-1:2])                # observations, total weight
    assert FX["min_top2_gap_ulp"][0] >= 64


@pytest.mark.parametrize("name,acts", [("a", (nr.SIGMOID, nr.TANH)), ("a", (nr.TANH, nr.RELU)), ("b", (nr.SIGMOID,)), ("b", (nr.NONE,))])
def test_gradient_equals_finite_differences_of_the_f64_objective(name, acts):
    net, x, e, w = nr.variant(name, acts, 19, 4242, frame_weights=True, class_weights=True)
    _, o, wt = nr.labels(e, None, net.class_weights, w)
    s = nr.accumulate(net, x, e, w, mask=nr.BASE | nr.GRADIENT)
    rng = np.random.Generator(np.random.PCG64(1))
    h = 1e-5
    for l in range(len(net.Ws)):
        G, g = s["gradient_weights"][l], s["gradient_bias"][l]
        scale = np.abs(G).max()
        for _ in range(12):
            n, k = rng.integers(0, net.Ws[l].shape[0]), rng.integers(0, net.Ws[l].shape[1])
            vals = []
            for sign in (1, -1):
                Ws = [W.astype(np.float64) for W in net.Ws]
                Ws[l][n, k] += sign * h
                vals.append(nr.objective_f64(Ws, net.bs, net.acts, x, o, wt))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - G[k, n]) <= 1e-6 * scale, (l, n, k, fd, G[k, n])
        for n in rng.integers(0, len(g), 6):
            vals = []
            for sign in (1, -1):
                bs = [b.astype(np.float64) for b in net.bs]
                bs[l][n] += sign * h
                vals.append(nr.objective_f64(net.Ws, bs, net.acts, x, o, wt))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[n]) <= 1e-6 * np.abs(g).max(), (l, n, fd, g[n])
    assert abs(s["objective"] - nr.objective_f64(net.Ws, net.bs, net.acts, x, o, wt)) <= 1e-6 * s["objective"]


def host_trainer(net, mask):
    return rasr_amd.FeedForwardTrainer(None, net.Ws, net.bs, net.acts, statistics=mask, class_weights=net.class_weights,
                                       class_to_output=net.class_to_output)


@pytest.fixture(scope="module")
def buffers():
    """one network's statistics of two batches, from the restatement, for every mask"""
    net, x, e, w = nr.variant("a", (nr.SIGMOID, nr.RELU), 60, 99, frame_weights=True, class_weights=True, disregard=True)
    out = {}
    for mask in range(1, 16):
        out[mask] = tuple(nr.flat(nr.accumulate(net, x[r], e[r], w[r], mask=mask), net.dims, net.dims[0], net.dims[-1], mask)
                          for r in (slice(0, 35), slice(35, 60)))
    return net, out


@pytest.mark.parametrize("mask", range(1, 16))
def test_files_layout_and_combination_for_every_mask(buffers, mask, tmp_path):
    net, bufs = buffers
    a, b = bufs[mask]
    dims = net.dims
    tr = host_trainer(net, mask)
    y, want = tr.layout, nr.layout(dims, dims[0], dims[-1], mask)
    assert tr.accumulator_size() == want["size"] == len(a) and y.tail == want["tail"] and y.class_counts == want["class_counts"]
    assert (y.feature_sum, y.feature_square_sum) == (want["feature_sum"], want["feature_square_sum"])
    assert [y.gradient_weights[l] for l in range(3)] == (want["gradient_weights"] or [-1] * 3)
    assert [y.gradient_bias[l] for l in range(3)] == (want["gradient_bias"] or [-1] * 3)
    pa, pb = str(tmp_path / "a.stat"), str(tmp_path / "b.stat")
    tr.write(a, pa)
    tr.write(b, pb)
    raw = open(pa, "rb").read()
    assert raw == nr.statistics_bytes(a, dims, dims[0], dims[-1], mask)
    assert raw[:16] == nr.magic(mask) and struct.unpack("<I", raw[16:20]) == (2,)
    ra, rb = tr.read(pa), tr.read(pb)
    assert np.array_equal(ra, nr.narrowed(a, dims, dims[0], dims[-1], mask))
    # Statistics<f32>::combine: sums in f32, integers as integers
    both = rasr_amd.combine_nn_statistics(tr, [pa, pb])
    exp = (ra.astype(np.float32) + rb.astype(np.float32)).astype(np.float64)
    exp[y.tail], exp[y.tail + 1] = ra[y.tail] + rb[y.tail], ra[y.tail + 1] + rb[y.tail + 1]
    if mask & nr.CLASS_COUNTS:
        exp[y.class_counts:y.class_counts + dims[-1]] = (ra + rb)[y.class_counts:y.class_counts + dims[-1]]
    assert np.array_equal(both, exp)
    assert np.array_equal(rasr_amd.combine_nn_statistics(tr, [pa]), ra)
    s = tr.statistics(both)
    assert s["n_observations"] == int(ra[y.tail] + rb[y.tail])
    if mask & nr.CLASS_COUNTS:
        for back_off in (0, 1, 5):
            got = rasr_amd.prior_from_class_counts(tr, both, back_off)
            assert np.array_equal(bits(got), bits(nr.prior_from_class_counts(s["class_counts"], net.class_weights, back_off))), back_off
        assert (rasr_amd.prior_from_class_counts(tr, both, 0) == -nr.FLT_MAX).sum() == (s["class_counts"] == 0).sum()
    else:
        with pytest.raises(rasr_amd.AmxError):
            rasr_amd.prior_from_class_counts(tr, both, 1)
    if mask & nr.MEAN_AND_VARIANCE:
        mean, dev = rasr_amd.mean_and_deviation(tr, both)
        wm, wd = nr.mean_and_deviation(s["feature_sum"], s["feature_square_sum"], s["total_weight"])
        assert np.array_equal(bits(mean), bits(wm)) and np.array_equal(bits(dev), bits(wd))
    else:
        with pytest.raises(rasr_amd.AmxError):
            rasr_amd.mean_and_deviation(tr, both)


def fixture_trainer(mask, class_weights=None):
    """a host-only handle with the shapes of the fixture's small object (the weights do not matter to files)"""
    dims = [int(d) for d in FX["write_dims"]]
    Ws = [np.zeros((n, i), np.float32) for i, n in zip(dims[:-1], dims[1:])]
    bs = [np.zeros(n, np.float32) for n in dims[1:]]
    return dims, rasr_amd.FeedForwardTrainer(None, Ws, bs, [nr.SIGMOID] * (len(Ws) - 1) + [nr.NONE], statistics=mask, class_weights=class_weights)


@pytest.mark.parametrize("mask", range(1, 16))
def test_write_reproduces_the_bytes_of_the_reference_for_each_mask(mask, tmp_path):
    """tests/golden/ref_nntrain.npz holds what the reference's Statistics<f32>::write emitted (its own text on its own BinaryOutputStream,
    Math::Vector and Math::Matrix) for a small object under each flag mask"""
    dims, tr = fixture_trainer(mask)
    a, want = FX["write_flat/%d" % mask], FX["write_bytes/%d" % mask].tobytes()
    path = str(tmp_path / "s.stat")
    tr.write(a, path)
    assert open(path, "rb").read() == want
    assert nr.statistics_bytes(a, dims, dims[0], dims[-1], mask) == want        # the restatement the other tests use
    assert np.array_equal(tr.read(path), a)                                     # the object's values are f32 and u32: nothing is lost


def test_prior_equals_the_reference_bit_for_bit():
    counts, cw = FX["prior_counts"], FX["prior_class_weights"]
    tr = rasr_amd.FeedForwardTrainer(None, statistics=("class-counts",), n_outputs=len(counts), class_weights=cw)
    a = np.zeros(tr.accumulator_size())
    a[tr.layout.class_counts:tr.layout.class_counts + len(counts)] = counts
    for b in FX["prior_back_off"]:
        want = FX["prior_log/%d" % b]
        assert np.array_equal(bits(rasr_amd.prior_from_class_counts(tr, a, int(b))), bits(want)), b
        assert np.array_equal(bits(nr.prior_from_class_counts(counts, cw, b)), bits(want)), b
    assert FX["prior_log/0"][2] == -nr.FLT_MAX and FX["prior_log/1"][5] == -nr.FLT_MAX      # a class never seen without back-off; a zero class weight
    for wrong in (-1.0, 2.0 ** 32, np.nan, np.inf, 0.5):       # a count that is no u32 is refused, not cast
        a[tr.layout.class_counts] = wrong
        with pytest.raises(rasr_amd.AmxError) as err:
            rasr_amd.prior_from_class_counts(tr, a, 1)
        assert err.value.status == _lib.AMX_ERR_INVALID


def test_mean_and_deviation_equal_the_reference_bit_for_bit():
    s, q, tw = FX["md_sum"], FX["md_square_sum"], FX["md_total_weight"][0]
    tr = rasr_amd.FeedForwardTrainer(None, statistics=("mean-and-variance",), feature_dim=len(s))
    a = np.zeros(tr.accumulator_size())
    y = tr.layout
    a[y.feature_sum:y.feature_sum + len(s)], a[y.feature_square_sum:y.feature_square_sum + len(s)], a[y.tail + 2], a[y.tail] = s, q, tw, 5000
    mean, dev = rasr_amd.mean_and_deviation(tr, a)
    assert np.array_equal(bits(mean), bits(FX["md_mean"])) and np.array_equal(bits(dev), bits(FX["md_deviation"]))
    wm, wd = nr.mean_and_deviation(s, q, tw)
    assert np.array_equal(bits(wm), bits(FX["md_mean"])) and np.array_equal(bits(wd), bits(FX["md_deviation"]))


def test_counts_that_are_no_u32_are_refused_by_write(tmp_path):
    dims, tr = fixture_trainer(ALL)
    good = FX["write_flat/%d" % ALL]
    y = tr.layout
    for where in (y.tail, y.tail + 1, y.class_counts):
        for wrong in (-1.0, 2.0 ** 32, np.nan, -np.inf, 1.5):
            a = good.copy()
            a[where] = wrong
            with pytest.raises(rasr_amd.AmxError) as err:
                tr.write(a, str(tmp_path / "bad.stat"))
            assert err.value.status == _lib.AMX_ERR_INVALID, (where, wrong)


def test_files_that_are_refused(buffers, tmp_path):
    net, bufs = buffers
    dims = net.dims
    tr = host_trainer(net, ALL)
    a = bufs[ALL][0]
    good = nr.statistics_bytes(a, dims, dims[0], dims[-1], ALL)
    path = str(tmp_path / "x.stat")

    def status(raw):
        open(path, "wb").write(raw)
        with pytest.raises(rasr_amd.AmxError) as err:
            tr.read(path)
        return err.value.status, str(err.value)
    open(path, "wb").write(good)
    tr.read(path)
    # the magic of another mask
    st, msg = status(nr.statistics_bytes(bufs[nr.BASE | nr.GRADIENT][0], dims, dims[0], dims[-1], nr.BASE | nr.GRADIENT))
    assert st == _lib.AMX_ERR_INVALID and "magic" in msg
    # version 3, precision letter D, no statistics file at all
    st, msg = status(nr.statistics_bytes(a, dims, dims[0], dims[-1], ALL, version=3))
    assert st == _lib.AMX_ERR_INVALID and "version" in msg
    st, msg = status(nr.statistics_bytes(a, dims, dims[0], dims[-1], ALL, precision="D"))
    assert st == _lib.AMX_ERR_UNSUPPORTED and "double-precision" in msg
    assert status(b"NNSTAX" + good[6:])[0] == _lib.AMX_ERR_INVALID
    # another network's shapes: one unit more in the middle layer, another feature dimension, another number of layers
    for other in ([24, 41, 33, 50], [25, 40, 33, 50], [24, 40, 50]):
        y = nr.layout(other, other[0], other[-1], ALL)
        st, msg = status(nr.statistics_bytes(np.zeros(y["size"]), other, other[0], other[-1], ALL))
        assert st == _lib.AMX_ERR_INVALID, other
    # truncated anywhere
    for keep in list(range(0, 64)) + list(range(64, len(good), 997)) + [len(good) - 1]:
        assert status(good[:keep])[0] == _lib.AMX_ERR_INVALID, keep
    with pytest.raises(rasr_amd.AmxError):
        tr.read(str(tmp_path / "missing.stat"))
    with pytest.raises(rasr_amd.AmxError):
        rasr_amd.combine_nn_statistics(tr, [])


def test_create_refusals_through_python():
    net, _, _, _ = nr.variant("b", (nr.TANH,), 4, 1)
    for precision in ("bf16", "bf16x3", "f16mx"):
        with pytest.raises(rasr_amd.AmxError) as err:
            rasr_amd.FeedForwardTrainer(None, net.Ws, net.bs, net.acts, precision=precision)
        assert err.value.status == _lib.AMX_ERR_UNSUPPORTED
    with pytest.raises(rasr_amd.AmxError) as err:
        rasr_amd.FeedForwardTrainer(None, net.Ws, net.bs, [_lib.AMX_ACT_ELU, 0])
    assert err.value.status == _lib.AMX_ERR_UNSUPPORTED and "layer 0" in str(err.value)
    with pytest.raises(rasr_amd.AmxError) as err:
        rasr_amd.FeedForwardTrainer(None, net.Ws, net.bs, net.acts, maxout={0: 65})
    assert err.value.status == _lib.AMX_ERR_UNSUPPORTED and "layer 0" in str(err.value) and "maxout" in str(err.value)
    with pytest.raises(rasr_amd.AmxError):
        rasr_amd.FeedForwardTrainer(None, statistics=("gradient",), feature_dim=3, n_outputs=2)
    for name in ("FeedForwardTrainer", "combine_nn_statistics", "prior_from_class_counts", "mean_and_deviation"):
        assert name in rasr_amd.__all__


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_nntrain_test.cc compiles the handle's host side into a program of its own: every create-time refusal, the layout under
    every mask, files written, read, combined and cut short; built with -fsanitize=address,undefined on the host side only, run as a
    process of its own (nothing sanitized is loaded into Python).  Sanitizers are for machines without a GPU: where one is present the
    same program is built and run plainly."""
    import torch
    exe = str(tmp_path / "host_nntrain_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_nntrain_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "host_nntrain_test: ok" in r.stdout, r.stdout + r.stderr
