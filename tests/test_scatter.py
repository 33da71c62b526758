"""LDA scatter-matrix estimation on the host: the plain restatement (tests/scatter_reference.py) against the reference's own text
(tests/golden/ref_scatter.npz, written by tests/golden/make_scatter_golden.py), and the library's host entry points
(amx_scatter_finalize, the accumulator file, amx_matrix_*_f64) against the restatement -- all bit for bit."""
import os

import numpy as np
import pytest

from tests import scatter_reference as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_scatter.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_cases(g):
    """name -> (feats, classes, weights or None)"""
    names = sorted({k[:-len("/feats")] for k in g if k.endswith("/feats")})
    assert len(names) == 8
    return {n: (g[n + "/feats"], g[n + "/classes"], g.get(n + "/weights")) for n in names}


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def estimator(dim, n_classes):
    import rasr_amd
    return rasr_amd.ScatterMatricesEstimator(None, dim, n_classes)


def test_both_builds_of_the_reference_compute_the_same_bits(golden):
    """nothing in the estimator can be contracted: the fixture keeps no contract=fma copy, only the marks that they were equal"""
    assert not [k for k in golden if "/fma/" in k and not k.endswith("_same_as_off")]
    marks = [k for k in golden if k.endswith("_same_as_off")]
    assert len(marks) == 8 * 5 and all(int(golden[k]) == 1 for k in marks)
    assert int(golden["empty_finalize_fails/off"]) == 1 and int(golden["empty_finalize_fails/fma"]) == 1


def test_restatement_equals_the_reference(golden):
    n_classes = int(golden["n_classes"])
    for name, (x, cls, w) in fixture_cases(golden).items():
        dim = x.shape[1]
        assert (cls >= n_classes).any() and (cls == sr.NO_LABEL).any(), name
        acc = sr.accumulate(x, cls, n_classes, w)
        assert bits(acc, golden[name + "/off/acc"]), name
        assert bits(golden[name + "/off/acc_read"], acc), name
        assert sr.file_bytes(acc, dim, n_classes) == golden[name + "/off/file"].tobytes(), name
        for normalize, key in ((False, "matrices"), (True, "matrices_normalized")):
            got = sr.finalize(acc, dim, n_classes, normalize)
            for m, want, what in zip(got, golden["%s/off/%s" % (name, key)], ("between", "within", "total")):
                assert bits(m, want), (name, key, what)
    # class 3 has no observation at dim 5: finalize skips it
    assert not (golden["d5/gauss/weighted/classes"] == 3).any()
    assert golden["d5/gauss/weighted/off/acc"][-1] == 0.0


def test_restatement_rounds_nowhere_on_exact_inputs():
    for dim, T, n_classes in ((7, 500, 5), (65, 300, 1000)):
        x, kx = sr.exact_features(T, dim, 11)
        w, jw = sr.exact_weights(T, 12)
        cls = sr.alignment(T, n_classes, "runs", 13)
        assert np.array_equal(sr.accumulate(x, cls, n_classes), sr.accumulate_int(kx, cls, n_classes))
        want = sr.accumulate(x, cls, n_classes, w)
        assert np.array_equal(want, sr.accumulate_int(kx, cls, n_classes, jw))
        order = np.random.Generator(np.random.PCG64(14)).permutation(T)
        assert np.array_equal(sr.accumulate(x[order], cls[order], n_classes, w[order]), want)
        assert np.array_equal(sr.accumulate(x, cls, n_classes, w, acc=want.copy()), 2 * want)
        kept = len(sr.kept_frames(cls, n_classes)[0])
        assert kept == T - len(np.arange(5, T, 10)) and sr.accumulate(x, cls, n_classes)[-n_classes:].sum() == kept


def test_f32_products_differ_from_f64_products():
    """the point of the f32 rounding: on Gaussian input a product formed in f64 is another number"""
    x = np.random.Generator(np.random.PCG64(5)).standard_normal(13).astype(np.float32)
    p, y = sr.single_frame_products(x, 0.3)
    i, j = sr.tril(13)
    wide = x[i].astype(np.float64) * x[j].astype(np.float64) * np.float64(np.float32(0.3))
    assert (p != wide).mean() > 0.5


def test_library_finalize_and_files_equal_the_restatement(golden, tmp_path):
    import rasr_amd
    n_classes = int(golden["n_classes"])
    cases = {n: (golden[n + "/off/acc"], x.shape[1], n_classes) for n, (x, cls, w) in fixture_cases(golden).items()}
    x, _ = sr.exact_features(300, 65, 21)
    cls = sr.alignment(300, 9, "random", 23)
    cases["exact"] = (sr.accumulate(x, cls, 9, sr.exact_weights(300, 22)[0]), 65, 9)
    for name, (acc, dim, nc) in cases.items():
        est = estimator(dim, nc)
        assert est.accumulator_size() == sr.layout(dim, nc)[2] == len(acc)
        for normalize in (False, True):
            for m, want in zip(est.finalize(acc, normalize), sr.finalize(acc, dim, nc, normalize)):
                assert bits(m, want), (name, normalize)
        path = str(tmp_path / "acc.bin")
        est.write(acc, path)
        with open(path, "rb") as f:
            assert f.read() == sr.file_bytes(acc, dim, nc), name
        d, n, back = rasr_amd.ScatterMatricesEstimator.read(path)
        assert (d, n) == (dim, nc) and bits(back, acc), name
    # the reference's own file, read by the library
    name = "d13/gauss/weighted"
    path = str(tmp_path / "ref.bin")
    with open(path, "wb") as f:
        f.write(golden[name + "/off/file"].tobytes())
    d, n, back = rasr_amd.ScatterMatricesEstimator.read(path)
    assert (d, n) == (13, n_classes) and bits(back, golden[name + "/off/acc"])


def test_finalize_output_matrices_are_nullable():
    from rasr_amd import _lib
    L = _lib.lib()
    x, _ = sr.exact_features(50, 4, 31)
    acc = sr.accumulate(x, sr.alignment(50, 3, "runs", 32), 3)
    want = sr.finalize(acc, 4, 3)
    for k in range(3):
        m = np.zeros((4, 4))
        ptrs = [None, None, None]
        ptrs[k] = m.ctypes.data
        assert L.amx_scatter_finalize(4, 3, acc.ctypes.data, 0, *ptrs) == 0
        assert bits(m, want[k])


def test_finalize_with_an_empty_class_and_without_observations():
    from rasr_amd import AmxError
    dim, nc = 6, 5
    x, _ = sr.exact_features(80, dim, 41)
    cls = sr.alignment(80, nc, "random", 42)
    cls[cls == 2] = 4                      # class 2 stays empty
    acc = sr.accumulate(x, cls, nc)
    assert acc[sr.layout(dim, nc)[1] + 2] == 0
    est = estimator(dim, nc)
    for m, want in zip(est.finalize(acc), sr.finalize(acc, dim, nc)):
        assert np.isfinite(m).all() and bits(m, want)
    b, w, t = est.finalize(acc, normalize=True)
    assert np.allclose(b + w, t, rtol=1e-12, atol=1e-12) and np.array_equal(w, w.T)
    zero = np.zeros(sr.layout(dim, nc)[2])
    with pytest.raises(AmxError, match="No observation has been seen"):
        est.finalize(zero)
    with pytest.raises(ValueError, match="No observation has been seen"):
        sr.finalize(zero, dim, nc)


def test_matrix_f64_round_trip_and_header(tmp_path):
    import rasr_amd
    m = np.random.Generator(np.random.PCG64(51)).standard_normal((5, 7))
    m[1, 2], m[3, 3] = np.inf, -0.0
    p64, p32 = str(tmp_path / "m64.bin"), str(tmp_path / "m32.bin")
    rasr_amd.write_matrix_f64("bin:" + p64, m)
    rasr_amd.write_nn_matrix("bin:" + p32, m.astype(np.float32))
    with open(p64, "rb") as f:
        b64 = f.read()
    with open(p32, "rb") as f:
        b32 = f.read()
    assert b64 == sr.matrix_bytes(m) and b32 == sr.matrix_bytes(m.astype(np.float32))
    assert b64[:16] == b32[:16] and len(b64) == 12 + 5 * (4 + 7 * 8)      # u32 rows, cols, rows, the first row's u32 cols
    assert bits(rasr_amd.read_matrix_f64(p64), m) and bits(rasr_amd.read_matrix_f64("bin:" + p64), m)
    with open(p64, "wb") as f:
        f.write(b64[:-3])
    with pytest.raises(rasr_amd.AmxError, match="amx_matrix_read_f64"):
        rasr_amd.read_matrix_f64(p64)
    with pytest.raises(rasr_amd.AmxError, match="amx_matrix_read_f64"):
        rasr_amd.read_matrix_f64(p32)                                      # an f32 matrix is not an f64 matrix


def test_argument_errors(tmp_path):
    import ctypes as C

    import rasr_amd
    from rasr_amd import _lib
    L = _lib.lib()
    assert L.amx_scatter_accumulator_size(0, 3) == 0 and L.amx_scatter_accumulator_size(1025, 3) == 0 and L.amx_scatter_accumulator_size(4, 0) == 0
    assert L.amx_scatter_accumulator_size(1, 1) == 3 and L.amx_scatter_accumulator_size(1024, 10000) == 1024 * 1025 // 2 + 10000 * 1025
    with pytest.raises(ValueError):
        rasr_amd.ScatterMatricesEstimator(None, 1025, 3)
    acc = np.zeros(16)

    def err(status):
        assert status == _lib.AMX_ERR_INVALID
        return L.amx_last_error().decode()

    path = str(tmp_path / "x.bin").encode()
    for dim, nc in ((0, 3), (1025, 3), (3, 0)):
        assert "amx_scatter_finalize: bad shape" in err(L.amx_scatter_finalize(dim, nc, acc.ctypes.data, 0, None, None, None))
        assert "amx_scatter_accumulator_write: bad shape" in err(L.amx_scatter_accumulator_write(dim, nc, acc.ctypes.data, path))
    assert "NULL" in err(L.amx_scatter_finalize(3, 2, None, 0, None, None, None))
    assert "NULL" in err(L.amx_scatter_accumulator_write(3, 2, None, path))
    d, n, p = C.c_int(), C.c_int(), C.c_void_p()
    assert "cannot open" in err(L.amx_scatter_accumulator_read(str(tmp_path / "missing").encode(), C.byref(d), C.byref(n), C.byref(p)))
    # a truncated file, and one whose header is no accumulator's
    x, _ = sr.exact_features(20, 3, 61)
    good = sr.file_bytes(sr.accumulate(x, np.zeros(20, np.uint32), 2), 3, 2)
    for bad in (good[:-1], good[:30], b"\0\0\0\0" + good[4:], good[:4]):
        with open(path, "wb") as f:
            f.write(bad)
        assert "not a scatter accumulator file" in err(L.amx_scatter_accumulator_read(path, C.byref(d), C.byref(n), C.byref(p)))
        assert not p.value
    # the device entry point refuses a NULL context before it touches the device (its shape rules, which need a context: tests/test_scatter_gpu.py)
    bad_ctx = L.amx_scatter_accumulate_dev(None, None, 3, 1, 3, None, 2, None, None)
    assert "NULL context" in err(bad_ctx)
