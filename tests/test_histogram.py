"""Histogram normalisation on the host: the plain restatement (tests/histogram_reference.py) against the reference's own text
(tests/golden/ref_histogram.npz, written by tests/golden/make_histogram_golden.py), and the library's host entry points (files, tables,
CDFs, percentiles, the inverse CDFs of a host-only amx_histnorm, accumulation on the host) against the fixture -- all bit for bit."""
import os

import numpy as np
import pytest

from tests import histogram_reference as hr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_histogram.npz")
HISTOGRAMS = ("ties2", "ties5", "gauss_a", "gauss_b", "gauss_c", "speaker")
NORMALIZERS = ("single_explicit", "single_proposed", "ties", "two", "three")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def golden_table(g, prefix):
    return hr.Table(g[prefix + "/bucket_size"], int(g[prefix + "/offset"]), g[prefix + "/values"], bool(g[prefix + "/grow"]))


def same_table(got, want):
    """each an hr.Table or the library's (bucket_size, offset, values)"""
    got, want = (t if isinstance(t, hr.Table) else hr.Table(*t) for t in (got, want))
    return bits(np.float32(got.bucket_size), np.float32(want.bucket_size)) and got.offset == want.offset and bits(got.f, want.f)


def dims(g, name):
    return g["h/%s/feats" % name].shape[1]


def library_histogram(g, name, ctx=None):
    """the fixture's frames through the library's host accumulation, in two calls"""
    import rasr_amd
    x = g["h/%s/feats" % name]
    e = rasr_amd.HistogramEstimator(ctx, x.shape[1], float(g["h/%s/bucket_size" % name]))
    e.accumulate(x[:len(x) // 2])
    e.accumulate(x[len(x) // 2:])
    return e


def test_both_builds_of_the_reference_compute_the_same_bits(golden):
    """no multiply of this text feeds an add: neither build holds a fused multiply-add and the fixture keeps no contract=fma copy"""
    assert not [k for k in golden if k.startswith("fma/")]
    assert int(golden["fma_arrays_compared"]) == len([k for k in golden if k.startswith("off/")]) > 400
    assert int(golden["fma_instructions/off"]) == 0 and int(golden["fma_instructions/fma"]) == 0
    assert int(golden["off/scales_refused/too_large"]) == 1 and int(golden["off/scales_refused/negative"]) == 1


def test_fixture_holds_the_cases_it_is_meant_to(golden):
    for name in ("ties2", "ties5"):
        x = golden["h/%s/feats" % name]
        q = x.astype(np.float64) / 0.25
        ties = np.abs(q - np.floor(q)) == 0.5
        assert (ties & (x > 0)).any() and (ties & (x < 0)).any(), name
        assert (np.signbit(x) & (x == 0)).any(), name
    assert golden["h/gauss_a/feats"].shape == (200, 3) and float(golden["h/gauss_a/bucket_size"]) == float(np.float32(0.01))
    assert len({float(golden["h/%s/bucket_size" % n]) for n in ("gauss_a", "gauss_b", "gauss_c")}) == 3
    for name in NORMALIZERS:
        for key in golden["n/%s/tests" % name]:
            assert golden["off/n/%s/test/%s/inside" % (name, key)].all(), (name, key)


def test_restatement_of_the_estimation_equals_the_reference(golden):
    for name in HISTOGRAMS:
        x, bs = golden["h/%s/feats" % name], golden["h/%s/bucket_size" % name]
        tables = hr.estimate(x, bs)
        split = hr.estimate(x[7:], bs, start=hr.estimate(x[:7], bs))
        for d, t in enumerate(tables):
            want = golden_table(golden, "off/h/%s/table/%d" % (name, d))
            assert want.grow and same_table(t, want) and same_table(split[d], want), (name, d)
            assert same_table(golden_table(golden, "off/h/%s/read/%d" % (name, d)), want), (name, d)
            assert same_table(hr.cdf(t), golden_table(golden, "off/h/%s/cdf/%d" % (name, d))), (name, d)
            got = np.array([hr.percentile(t, p) for p in golden["percents"]], np.float32)
            assert bits(got, golden["off/h/%s/percentiles/%d" % (name, d)]), (name, d)
        file = golden["off/h/%s/file" % name].tobytes()
        assert hr.file_bytes(tables) == file, name
        assert all(same_table(a, b) for a, b in zip(hr.parse_file(file), tables)), name


def restated_normalizer(g, name):
    train = [hr.estimate(g["h/%s/feats" % t], g["h/%s/bucket_size" % t]) for t in g["n/%s/train" % name]]
    return train, hr.training_inverses(train, g["n/%s/scales" % name], g["n/%s/probability_bucket_size" % name])


def test_restatement_of_the_normalisation_equals_the_reference(golden):
    for name in NORMALIZERS:
        train, inv = restated_normalizer(golden, name)
        if len(train) > 1:
            assert bits(np.array(hr.normalize_scales(golden["n/%s/scales" % name]), np.float32), golden["off/n/%s/all_scales" % name]), name
        for d, t in enumerate(inv):
            assert same_table(t, golden_table(golden, "off/n/%s/inverse/%d" % (name, d))), (name, d)
        for key in golden["n/%s/tests" % name]:
            x = golden["h/%s/feats" % key]
            cdfs = [hr.cdf(t) for t in hr.estimate(x, golden["h/%s/bucket_size" % key])]
            for d, t in enumerate(cdfs):
                assert same_table(t, golden_table(golden, "off/n/%s/test/%s/cdf/%d" % (name, key, d))), (name, key, d)
            out, n_test, n_inv = hr.apply(x, cdfs, inv)
            assert bits(out, golden["off/n/%s/test/%s/out" % (name, key)]) and (n_test, n_inv) == (0, 0), (name, key)
    assert not hr.scales_well_defined(hr.normalize_scales([1.25])) and not hr.scales_well_defined(hr.normalize_scales([-0.25]))


def test_restatement_clamps_outside_the_tables():
    t = hr.Table(0.5, 2, [0.25, 0.5, 0.75, 1.0])          # buckets of x = -1, -0.5, 0, 0.5
    x = np.array([-1.0, 0.5, -1.3, 0.8, -1e30, 1e30, np.inf, -np.inf, np.nan], np.float32)
    v, c = hr.lookup(t, x)
    assert bits(v, np.array([0.25, 1.0, 0.25, 1.0, 0.25, 1.0, 1.0, 0.25, 0.25], np.float32))
    assert c.tolist() == [False, False, True, True, True, True, True, True, True]
    inv = [hr.Table(0.25, -2, [10.0, 20.0, 30.0])]         # buckets of p = 0.5, 0.75, 1.0
    out, n_test, n_inv = hr.apply(x[:, None], [t], inv)
    assert bits(out[:-1, 0], np.array([10.0, 30.0, 10.0, 30.0, 10.0, 30.0, 30.0, 10.0], np.float32)) and np.isnan(out[-1, 0])
    assert (n_test, n_inv) == (7, 5)                       # p = 0.25 lies below the inverse table's first bucket


def test_library_tables_files_cdfs_and_percentiles_equal_the_fixture(golden, tmp_path):
    import rasr_amd
    for name in HISTOGRAMS:
        e = library_histogram(golden, name)
        info = e.describe()
        assert (info["dim"], info["frozen"], info["frames"]) == (dims(golden, name), 0, len(golden["h/%s/feats" % name]))
        path = str(tmp_path / (name + ".hist"))
        e.write(path)
        with open(path, "rb") as f:
            assert f.read() == golden["off/h/%s/file" % name].tobytes(), name
        ref_path = str(tmp_path / (name + ".ref"))
        with open(ref_path, "wb") as f:
            f.write(golden["off/h/%s/file" % name].tobytes())
        r = rasr_amd.HistogramEstimator.read(ref_path)
        assert r.describe()["frozen"] == 0 and r.describe()["dim"] == e.dim
        for h in (e, r):
            for d in range(e.dim):
                assert same_table(h.table(d), golden_table(golden, "off/h/%s/table/%d" % (name, d))), (name, d)
                assert same_table(h.cdf(d), golden_table(golden, "off/h/%s/cdf/%d" % (name, d))), (name, d)
                got = np.array([h.percentile(d, float(p)) for p in golden["percents"]], np.float32)
                assert bits(got, golden["off/h/%s/percentiles/%d" % (name, d)]), (name, d)


def test_library_inverse_and_test_cdfs_equal_the_fixture(golden):
    import rasr_amd
    for name in NORMALIZERS:
        train = [library_histogram(golden, t) for t in golden["n/%s/train" % name]]
        n = rasr_amd.HistogramNormalization(None, train, float(golden["n/%s/probability_bucket_size" % name]))
        if len(train) > 1:
            with pytest.raises(rasr_amd.AmxError, match="set_scales"):
                n.inverse_cdf(0)
            n.set_scales(golden["n/%s/scales" % name])
        for t in train:
            t.close()                                      # the normaliser keeps copies
        for d in range(n.dim):
            assert same_table(n.inverse_cdf(d), golden_table(golden, "off/n/%s/inverse/%d" % (name, d))), (name, d)
        for i, key in enumerate(golden["n/%s/tests" % name]):
            assert n.add_key(library_histogram(golden, key)) == i
            for d in range(n.dim):
                assert same_table(n.test_cdf(i, d), golden_table(golden, "off/n/%s/test/%s/cdf/%d" % (name, key, d))), (name, key, d)


def test_a_file_of_other_values_loads_frozen_and_refuses_accumulate(golden, tmp_path):
    import rasr_amd
    tables = hr.estimate(golden["h/ties2/feats"], golden["h/ties2/bucket_size"])
    for what, change in (("fraction", lambda t: t.f.__setitem__(1, 2.5)), ("too large", lambda t: t.f.__setitem__(1, 2.0 ** 24 + 2)),
                         ("fixed size", lambda t: setattr(t, "grow", False)), ("negative", lambda t: t.f.__setitem__(0, -1.0))):
        changed = [t.copy() for t in tables]
        change(changed[1])
        path = str(tmp_path / "frozen.hist")
        with open(path, "wb") as f:
            f.write(hr.file_bytes(changed))
        h = rasr_amd.HistogramEstimator.read(path)
        assert h.describe()["frozen"] == 1, what
        assert all(same_table(h.table(d), changed[d]) for d in range(2)), what
        with pytest.raises(rasr_amd.AmxError, match="not counts") as e:
            h.accumulate(np.zeros((1, 2), np.float32))
        assert e.value.status == rasr_amd._lib.AMX_ERR_STATE
        # the device entry point refuses before it looks at the device or the buffer
        assert h.L.amx_histogram_accumulate_dev(h.h, None, 2, 1) == rasr_amd._lib.AMX_ERR_STATE
        out = str(tmp_path / "again.hist")
        h.write(out)
        with open(out, "rb") as f:
            assert f.read() == hr.file_bytes(changed), what


def test_a_count_stops_at_two_to_the_24_through_a_file(tmp_path):
    """the reference adds 1.0f: 16 777 215 + 3 frames is 16 777 216, and it stays there"""
    import rasr_amd
    start = [hr.Table(0.25, 1, [5.0, 16777215.0, 7.0])]
    path = str(tmp_path / "full.hist")
    with open(path, "wb") as f:
        f.write(hr.file_bytes(start))
    h = rasr_amd.HistogramEstimator.read(path)
    assert h.describe()["frozen"] == 0 and h.describe()["frames"] == 16777227
    h.accumulate(np.zeros((3, 1), np.float32))
    assert same_table(h.table(0), hr.Table(0.25, 1, [5.0, 16777216.0, 7.0]))
    assert same_table(h.table(0), hr.estimate(np.zeros((3, 1), np.float32), 0.25, start=start)[0])
    a = np.float32(16777215.0)
    for _ in range(3):
        a = np.float32(a + np.float32(1.0))
    assert a == 16777216.0
    h.accumulate(np.array([[0.0], [0.25], [-0.5]], np.float32))
    assert same_table(h.table(0), hr.Table(0.25, 2, [1.0, 5.0, 16777216.0, 8.0]))
    h.write(path)
    again = rasr_amd.HistogramEstimator.read(path)
    assert again.describe()["frozen"] == 0 and same_table(again.table(0), h.table(0))


def test_host_accumulation_refuses_what_the_cast_is_undefined_for():
    import rasr_amd
    e = rasr_amd.HistogramEstimator(None, 2, 0.5)
    e.accumulate(np.array([[1.0, 2.0]], np.float32))
    before = [e.table(d) for d in range(2)]
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 29, -2.0 ** 29):
        x = np.array([[0.0, 0.0], [3.0, bad]], np.float32)
        assert not hr.acceptable(x, 0.5)
        with pytest.raises(rasr_amd.AmxError):
            e.accumulate(x)
        assert all(same_table(e.table(d), before[d]) for d in range(2)) and e.describe()["frames"] == 1
    x = np.array([[0.0, np.float32(2.0 ** 29 - 64)]], np.float32)
    assert hr.acceptable(x, 0.5)


def test_argument_errors(golden):
    import rasr_amd
    INVALID = rasr_amd._lib.AMX_ERR_INVALID
    for bs in (0.0, -0.25, float("nan"), float("inf")):
        with pytest.raises(rasr_amd.AmxError, match="Bucket size") as e:
            rasr_amd.HistogramEstimator(None, 3, bs)
        assert e.value.status == INVALID
    for dim in (0, -1, 4097):
        with pytest.raises(rasr_amd.AmxError):
            rasr_amd.HistogramEstimator(None, dim, 0.25)
    a, b = library_histogram(golden, "gauss_a"), library_histogram(golden, "gauss_b")
    two, empty = library_histogram(golden, "ties2"), rasr_amd.HistogramEstimator(None, 3, 0.01)
    # an empty histogram has no CDF: as a table, as a training histogram, as a key
    with pytest.raises(rasr_amd.AmxError, match="empty") as e:
        empty.cdf(0)
    assert e.value.status == INVALID
    with pytest.raises(rasr_amd.AmxError, match="empty"):
        rasr_amd.HistogramNormalization(None, [empty])
    n = rasr_amd.HistogramNormalization(None, [a, b])
    with pytest.raises(rasr_amd.AmxError, match="empty"):
        n.add_key(empty)
    # dimension mismatch: among the training histograms, and of a key
    with pytest.raises(rasr_amd.AmxError, match="Mismatch") as e:
        rasr_amd.HistogramNormalization(None, [a, two])
    assert e.value.status == INVALID
    with pytest.raises(rasr_amd.AmxError, match="Mismatch") as e:
        n.add_key(two)
    assert e.value.status == INVALID
    # scales outside [0, 1] (the first one is 1 - the sum of the others)
    for scales in ([1.25], [-0.25], [float("nan")]):
        with pytest.raises(rasr_amd.AmxError, match="scales are smaller than zero or larger than 1") as e:
            n.set_scales(scales)
        assert e.value.status == INVALID
    n.set_scales([1.0])
    n.set_scales([0.0])
    with pytest.raises(rasr_amd.AmxError):
        rasr_amd.HistogramNormalization(None, [a]).set_scales([0.5])
    with pytest.raises(rasr_amd.AmxError):
        rasr_amd.HistogramNormalization(None, [a], -0.5)
    # a host-only handle cannot run on the device
    assert a.L.amx_histogram_accumulate_dev(a.h, None, 3, 1) == rasr_amd._lib.AMX_ERR_STATE
    off, keys = np.array([0, 1], np.int64), np.zeros(1, np.int32)
    assert n.L.amx_histnorm_apply_dev(n.h, 1, off.ctypes.data, keys.ctypes.data, None, 3, None, 3, None) == rasr_amd._lib.AMX_ERR_STATE
