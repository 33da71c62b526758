"""CPU: constrained MLLR without a device.  tests/cmllr_reference.py (plain numpy) against tests/golden/ref_cmllr.npz, what the reference's
own text computes in both of its builds (tests/golden/make_cmllr_golden.py): every accumulator bit and every file byte; then the
library's host side (cmllr_host.cpp: files, combine, estimate, score) against the same fixture.

estimate and score are held to the fixture's MEASURED bar: 4 x the largest distance, over the cases and both builds, between the
restatement with its own LU and the reference's text with OpenBLAS's LU (bar/transform_abs, bar/transform_rel, bar/score_abs,
bar/score_rel in the fixture)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import cmllr_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = cr.fixture()
CASES = cr.case_names(Z)
SMALL = [n for n in CASES if not n.startswith("f45")]
BUILDS = ("off", "fma")
BAR = {k: float(Z["bar/" + k]) for k in ("transform_abs", "transform_rel", "score_abs", "score_rel")}
MIN_OBS = float(Z["min_obs_weight"])
_ACC = {}


def acc_of(name, build):
    """the case's final accumulator of all keys: the restatement's, which test_restatement_equals_the_fixture holds to the reference's bits"""
    if (name, build) not in _ACC:
        _ACC[name, build] = cr.accumulate_case(cr.load_case(Z, name), build)
    return _ACC[name, build]


def estimator(c):
    return rasr_amd.AffineFeatureTransformEstimator(None, c["F"], c["n_keys"], model_dim=c["M"], pooled_variance=c["pooled_variance"])


def test_the_bar_is_the_measured_one_and_small():
    for k, v in BAR.items():
        assert v == 4 * float(Z["measured/" + k]) and 0 < v < 1e-11, (k, v)
    assert float(Z["worst_condition_number"]) < 1e6
    assert int(Z["fma_instructions/off"]) == 0 and int(Z["fma_instructions/fma"]) > 0


def test_vector_fma_equals_the_rational_one():
    rng = np.random.Generator(np.random.PCG64(5))
    a, b = rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 4, 4000), rng.standard_normal(4000)
    c = np.where(rng.random(4000) < 0.3, -a * b * (1 + rng.standard_normal(4000) * 1e-9), rng.standard_normal(4000) * 100)   # cancellation too
    got = cr.fma(a, b, c)
    want = np.array([cr.fma_exact(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.any(got != a * b + c)
    # the f32 one of the apply restatement
    a, b, c = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    c[:700] = -(a[:700] * b[:700])
    want = np.array([np.float32(cr.fma_exact(float(x), float(y), float(z))) for x, y, z in zip(a, b, c)])   # a * b + c fits an f64 here or ...
    got = cr.fma32(a, b, c)
    clear = want.astype(np.float64) == np.array([cr.fma_exact(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)])   # ... is judged where it does
    assert clear.sum() > 500 and np.array_equal(got[clear].view(np.uint32), want[clear].view(np.uint32))
    assert np.any(got != a * b + c)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_fixture(name, build):
    """every accumulator bit after the cut and at the end, in one call and in two; every file byte; combine"""
    c = cr.load_case(Z, name)
    acc = acc_of(name, build)
    assert cr.matches(cr.recorded(Z, name, build, "acc"), acc)
    assert cr.matches(cr.recorded(Z, name, build, "acc"), cr.accumulate_case(c, build, calls=2))
    assert cr.matches(cr.recorded(Z, name, build, "acc_cut"), cr.accumulate_case(c, build, upto=c["cut"]))
    size = cr.layout(c["F"], c["M"], c["pooled"])["size"]
    assert not acc[size:2 * size].any()   # key 1 receives no frame
    for key in (0, 2):
        data = np.frombuffer(cr.file_bytes(acc, c["F"], c["M"], c["pooled_variance"], key), np.uint8)
        assert cr.matches(cr.recorded(Z, name, build, "file/key%d" % key), data)
    combined = cr.combine(acc[:size], acc[2 * size:], 0.5)
    assert cr.matches(cr.recorded(Z, name, build, "combined"), combined)
    if build == "fma" and "exact" in name:
        assert "%s/fma/acc_same_as_off" % name in Z.files   # exactly representable frames: nothing rounds, both builds agree


@pytest.mark.parametrize("name", CASES)
def test_library_files_and_combine(name, tmp_path):
    c = cr.load_case(Z, name)
    est = estimator(c)
    size = est.key_size()
    assert size == cr.layout(c["F"], c["M"], c["pooled"])["size"]
    for build in BUILDS:
        acc = acc_of(name, build)
        for key in (0, 2):
            p = str(tmp_path / ("%s_%d.acc" % (build, key)))
            est.write(acc, p, key)
            assert cr.matches(cr.recorded(Z, name, build, "file/key%d" % key), np.fromfile(p, np.uint8))
            assert np.array_equal(est.read(p).view(np.uint64), acc[key * size:(key + 1) * size].view(np.uint64))
        combined = est.combine(acc, est, acc, 0.5, key=0, other_key=2)
        assert cr.matches(cr.recorded(Z, name, build, "combined"), combined)
        mem, want = est.members(acc, 0), cr.members(acc, c["F"], c["M"], c["pooled"], 0)
        assert mem["beta"] == want["beta"] and np.array_equal(mem["k"], want["k"]) and np.array_equal(mem["cov"], want["cov"])
        assert (mem["G"] is None) == c["pooled"] and (c["pooled"] or np.array_equal(mem["G"], want["G"]))


def _close(got, want, what):
    d = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    scale = float(np.abs(want).max())
    assert d <= BAR[what + "_abs"] and d <= BAR[what + "_rel"] * scale, (what, d, d / scale, BAR)


def _f32_equal_away_from_midpoints(got32, got64_ref, ref32):
    """the narrowed transform equals the reference's wherever the f64 value lies further from an f32 midpoint than the bar"""
    lo = got64_ref.astype(np.float32)
    other = np.where(lo.astype(np.float64) > got64_ref, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf)))
    mid = (lo.astype(np.float64) + other.astype(np.float64)) / 2
    clear = np.abs(got64_ref - mid) > BAR["transform_abs"]
    assert clear.mean() > 0.99
    assert np.array_equal(got32[clear], ref32[clear])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", CASES)
def test_estimate_and_score_within_the_measured_bar(name, build):
    c = cr.load_case(Z, name)
    est, acc = estimator(c), acc_of(name, build)
    for crit, cname, label in ((cr.NAIVE, "naive", "naive"), (cr.MMI_PRIME, "mmi", "mmi-prime")):
        ref64, ref32, ref_score = (cr.recorded(Z, name, build, "%s/%s" % (cname, k))[1] for k in ("transform64", "transform", "score"))
        n_it = len(ref64)
        t32, info = est.estimate(acc, 0, n_it, MIN_OBS, label, c["initial"], details=True)
        assert info["estimated"]
        its = info["iterations"] if crit == cr.MMI_PRIME else info["transform64"][None]
        scores = []
        for n in range(n_it):
            _close(its[n], ref64[n], "transform")
            narrowed = its[n].astype(np.float32)
            _f32_equal_away_from_midpoints(narrowed, ref64[n], ref32[n])
            s = est.score(acc, ref32[n], 0, label)
            _close([s], [ref_score[n]], "score")
            scores.append(s)
        assert np.array_equal(t32, its[-1].astype(np.float32))
        if crit == cr.MMI_PRIME:   # the iteration does not lose likelihood
            assert all(b >= a - BAR["score_abs"] - BAR["score_rel"] * abs(a) for a, b in zip(scores, scores[1:])), scores
        if name in SMALL or crit == cr.NAIVE:   # the restatement itself (it measured the bar: a quarter of it at the most)
            e = cr.estimate(acc[:est.key_size()], c["F"], c["M"], n_it, MIN_OBS, crit, c["initial"], c["pooled_variance"])
            mine = e["iterations"] if crit == cr.MMI_PRIME else e["transform64"][None]
            for n in range(n_it):
                _close(mine[n], ref64[n], "transform")
            if crit == cr.MMI_PRIME:
                assert np.array_equal(np.array([ch[0] for ch in e["choices"]]), Z["%s/%s/mmi/first_root_chosen" % (name, build)])
    # key 2 lies below min-observation-weight: mmi-prime returns the initial transform, a zero column in front of an F-column one
    t, info = est.estimate(acc, 2, 2, MIN_OBS, "mmi-prime", c["initial"], details=True)
    assert not info["estimated"] and np.array_equal(t, cr.recorded(Z, name, build, "below_min_obs/transform")[1])
    if c["initial"] is not None and c["initial"].shape[1] == c["F"]:
        assert not t[:, 0].any() and np.array_equal(t[:, 1:], c["initial"])
    elif c["initial"] is not None:   # F + 1 columns: taken as it is
        assert c["initial"].shape[1] == c["F"] + 1 and np.array_equal(t, c["initial"])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", CASES)
def test_transform_files_are_the_references_bytes(name, build, tmp_path):
    """the XML file the estimator writes per key: restatement and library against the reference writer's bytes, and back"""
    for cname in ("naive", "mmi"):
        t = cr.recorded(Z, name, build, cname + "/transform")[1][-1]
        want = cr.recorded(Z, name, build, cname + "/transform_file")
        assert cr.matches(want, np.frombuffer(cr.transform_file_bytes(t), np.uint8))
        p = str(tmp_path / (cname + ".matrix"))
        rasr_amd.write_transform(p, t)
        assert cr.matches(want, np.fromfile(p, np.uint8))
        back = rasr_amd.read_transform(p)   # six digits do not carry an f32: what comes back is the file's value
        assert back.shape == t.shape and np.array_equal(back, np.array([[np.float32("%e" % float(v)) for v in row] for row in t]))


def test_transform_file_reading_and_refusals(tmp_path):
    p = str(tmp_path / "t.matrix")
    t = np.array([[0.0, -1.5, 1e-40], [3.25e7, 1.0, -2.0 ** -20]], np.float32)
    rasr_amd.write_transform(p, t)
    raw = open(p, "rb").read()
    assert raw == cr.transform_file_bytes(t) and raw.startswith(b'<?xml version="1.0" encoding="ISO-8859-1"?>\n<matrix-f32 nRows="2" nColumns="3">\n0.000000e+00 ')
    # what an XML parser takes: comments in front, the attributes in the other order, single quotes, other white space
    open(p, "w").write("<?xml version='1.0'?>\n<!-- <matrix-f32 nRows=\"9\" nColumns=\"9\"> -->\n<matrix-f32  nColumns = '3'\n nRows='2' >1 2\t3\n\n4 5 6</matrix-f32>")
    assert np.array_equal(rasr_amd.read_transform(p), np.arange(1, 7, dtype=np.float32).reshape(2, 3))
    for cutoff in (10, 50, 80, len(raw) - 20, len(raw) - 3):
        open(p, "wb").write(raw[:cutoff])
        with pytest.raises(rasr_amd.AmxError):
            rasr_amd.read_transform(p)
    for bad in (raw.replace(b"matrix-f32", b"matrix-f64"), raw.replace(b'nRows="2"', b'nRows="3"'), raw.replace(b'nRows="2"', b'nRows="1"'),
                raw.replace(b'nColumns="3"', b'nColumns="0"'), raw.replace(b"-1.5", b"-x.5")):
        open(p, "wb").write(bad)
        with pytest.raises(rasr_amd.AmxError):
            rasr_amd.read_transform(p)
    with pytest.raises(rasr_amd.AmxError):
        rasr_amd.read_transform(str(tmp_path / "missing.matrix"))
    with pytest.raises(rasr_amd.AmxError, match="not finite"):
        rasr_amd.write_transform(p, np.array([[1.0, np.nan]], np.float32))
    with pytest.raises(ValueError):
        rasr_amd.AffineFeatureTransformEstimator(None, 5, 1)
    est = rasr_amd.AffineFeatureTransformEstimator(None, 5, 3, model_dim=5)
    with pytest.raises(ValueError):
        est.members(np.zeros(est.accumulator_size()), None)


def test_every_planted_defect_leaves_its_check():
    """each defect of cmllr_reference.DEFECTS changes accumulator bits, or moves the transform out of the bar, on at least one case --
    except `half`, which provably cannot (see below) and is pinned as such"""
    left = {d: 0 for d in cr.DEFECTS}
    for name in SMALL:
        c = cr.load_case(Z, name)
        want = cr.recorded(Z, name, "off", "acc")
        for d in ("reciprocal", "weight_first", "lower", "pooled_g", "segment_sorted"):
            got = cr.accumulate_case(c, "off", defects=(d,))
            left[d] += not cr.matches(want, got)
        left["restart"] += not cr.matches(want, cr.accumulate_case(c, "off", calls=2, defects=("restart",)))
        acc, ref64 = acc_of(name, "off"), cr.recorded(Z, name, "off", "mmi/transform64")[1]
        size = cr.layout(c["F"], c["M"], c["pooled"])["size"]
        right = cr.estimate(acc[:size], c["F"], c["M"], len(ref64), MIN_OBS, cr.MMI_PRIME, c["initial"], c["pooled_variance"])
        for d in ("half", "wrong_root"):
            e = cr.estimate(acc[:size], c["F"], c["M"], len(ref64), MIN_OBS, cr.MMI_PRIME, c["initial"], c["pooled_variance"], defects=(d,))
            diff = float(np.abs(e["iterations"] - ref64).max())
            left[d] += diff > BAR["transform_abs"] and diff > BAR["transform_rel"] * float(np.abs(ref64).max())
            if d == "half":
                # `1 / 2` as 0.5 changes both likelihoods and never the choice between them: with epsilon1 > 0 (G positive definite) the
                # logarithm's part and the quadratic part of l1 - l2 both carry the sign of epsilon2, so the root the reference's integer
                # division picks is the root the intended formula picks.  This defect cannot leave a mark on a transform; what it
                # changes is pinned here, and the recorded choices are the fixture's.
                assert [ch[0] for ch in e["choices"]] == [ch[0] for ch in right["choices"]] and diff <= BAR["transform_abs"]
                assert any(a[1] != b[1] or a[2] != b[2] for a, b in zip(e["choices"], right["choices"]))
    assert left.pop("half") == 0
    assert all(v > 0 for v in left.values()), left


def test_host_refusals(tmp_path):
    L = _lib.lib()
    name = "f5m5/full/weighted/gauss"
    c, acc = cr.load_case(Z, name), acc_of(name, "off")
    est = estimator(c)
    for call in (lambda: est.estimate(acc, 0, 1, 0.0, "hlda"), lambda: est.score(acc, np.zeros((5, 6), np.float32), 0, "hlda")):
        with pytest.raises(rasr_amd.AmxError, match="hlda") as e:
            call()
        assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    with pytest.raises(rasr_amd.AmxError, match="smaller than model_dim"):
        rasr_amd.AffineFeatureTransformEstimator(None, 4, 1, model_dim=5)
    gmm = rasr_amd.GmmFeatureScorer(None, dict(c["model"]))   # F < M is refused before the scorer's device is asked for
    h = C.c_void_p()
    assert L.amx_cmllr_create(gmm.h, 4, 1, C.byref(h)) == _lib.AMX_ERR_INVALID and b"smaller than the model's dimension" in L.amx_last_error()
    assert L.amx_cmllr_create(gmm.h, 5, 1, C.byref(h)) == _lib.AMX_ERR_STATE
    # combine: pooled with non-pooled, unequal variance vectors, unequal dimensions
    pn = "f5m5/pooled/weighted/gauss"
    pc, pacc = cr.load_case(Z, pn), acc_of(pn, "off")
    pest = estimator(pc)
    with pytest.raises(rasr_amd.AmxError, match="non-pooled"):
        est.combine(acc, pest, pacc)
    other = rasr_amd.AffineFeatureTransformEstimator(None, 5, 3, pooled_variance=pc["pooled_variance"] * np.float32(1.5))
    with pytest.raises(rasr_amd.AmxError, match="variances differ"):
        pest.combine(pacc, other, pacc)
    wide = rasr_amd.AffineFeatureTransformEstimator(None, 6, 3, model_dim=5)
    with pytest.raises(rasr_amd.AmxError, match="feature dimensions"):
        est.combine(acc, wide, np.zeros(wide.accumulator_size()))
    # files: truncated, wrong type tag, a pooled file for a non-pooled model
    p = str(tmp_path / "a.acc")
    est.write(acc, p)
    raw = open(p, "rb").read()
    for cutoff in (3, 20, 45, len(raw) // 2, len(raw) - 1):
        open(p, "wb").write(raw[:cutoff])
        with pytest.raises(rasr_amd.AmxError):
            est.read(p)
    open(p, "wb").write(raw[:4] + raw[4:40].replace(b"affine", b"offine") + raw[40:])
    with pytest.raises(rasr_amd.AmxError, match="type tag"):
        est.read(p)
    pest.write(pacc, p)
    with pytest.raises(rasr_amd.AmxError):
        est.read(p)
    with pytest.raises(rasr_amd.AmxError, match="initial transform"):
        est.estimate(acc, 0, 1, 0.0, "naive", initial=np.zeros((5, 3), np.float32))
    with pytest.raises(rasr_amd.AmxError, match="singular"):
        est.estimate(np.zeros(est.key_size()), 0, 1, 0.0, "naive")


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_cmllr_test.cc compiles cmllr_host.cpp into a program of its own: files, combine, the estimate on exported small cases and
    every refusal; built with -fsanitize=address,undefined on the host side only, run as a process of its own (nothing sanitized is
    loaded into Python).  Sanitizers are for machines without a GPU: where one is present the same program is built and run plainly."""
    import torch
    name = "f13m9/full/weighted/gauss"
    c, acc = cr.load_case(Z, name), acc_of(name, "off")
    size = cr.layout(c["F"], c["M"], False)["size"]
    pn = "f5m5/pooled/unweighted/gauss"
    pc, pacc = cr.load_case(Z, pn), acc_of(pn, "off")
    psize = cr.layout(5, 5, True)["size"]
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:   # per case: F, M, pooled, iterations, [variance], key 0, key 2, initial (M x F, or none), mmi transform64 of the last iteration
        for cc, a, sz, nm in ((c, acc, size, name), (pc, pacc, psize, pn)):
            ref = cr.recorded(Z, nm, "off", "mmi/transform64")[1]
            ini = cc["initial"]
            np.array([cc["F"], cc["M"], int(cc["pooled"]), len(ref), 0 if ini is None else ini.shape[1]], np.int32).tofile(f)
            if cc["pooled"]:
                cc["pooled_variance"].astype(np.float32).tofile(f)
            a[:sz].tofile(f)
            a[2 * sz:3 * sz].tofile(f)
            if ini is not None:
                ini.astype(np.float32).tofile(f)
            ref[-1].tofile(f)
            np.frombuffer(cr.file_bytes(a, cc["F"], cc["M"], cc["pooled_variance"], 0), np.uint8).tofile(str(tmp_path / ("key0_%d.acc" % cc["F"])))
    exe = str(tmp_path / "host_cmllr_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_cmllr_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe, str(data), str(tmp_path), repr(BAR["transform_abs"]), repr(BAR["transform_rel"]), repr(MIN_OBS)], capture_output=True, text=True)
    assert r.returncode == 0 and "host_cmllr_test: ok" in r.stdout, r.stdout + r.stderr
