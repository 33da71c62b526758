"""CPU: Bayes classification.  The restatement of tests/bayes_reference.py against the reference's own results
(tests/golden/ref_bayes.npz, written by tests/golden/make_bayes_golden.py from the reference's text in both of its builds), bit for bit
in every recorded case; the host logic of the amx_bayes handle; and the handle's argument checks once more from a stand-alone program
built with the host sanitizers.  No kernel runs here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rasr_amd import _lib
from tests import bayes_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_bayes.npz")
N_CLASSES = (3, 13)
LENGTHS = (0, 1, 2, 40, 300)
INT_MAX = br.INT_MAX


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def segments(golden, nc):
    """(T, rows slice within the concatenated recordings, scores, weights) per recorded segment length"""
    at = 0
    for i, T in enumerate(LENGTHS):
        yield i, T, slice(at, at + T), golden["in/%d/%d/scores" % (nc, T)], golden["in/%d/%d/weights" % (nc, T)]
        at += T


def test_fixture_holds_what_the_generator_says(golden):
    """both builds agree in every bit (no fma/ copy), all-ones weights equal no weights, and the cases are the ones the tests walk"""
    assert not [k for k in golden if k.startswith("fma/")]
    assert list(golden["fma_differs"]) == [""] and int(golden["fma_arrays_compared"]) > 200
    assert int(golden["fma_instructions/off"]) == 0
    assert bool(golden["off/ones_equal_none"])
    assert len([k for k in golden if k.startswith("cfg/classify/")]) == 9 and len([k for k in golden if k.startswith("cfg/scores/")]) == 4
    for nc in N_CLASSES:
        assert same(golden["off/prior/%d" % nc], br.prior(nc))
        assert golden["in/%d/300/scores" % nc].shape == (300, nc)


@pytest.mark.parametrize("nc", N_CLASSES)
@pytest.mark.parametrize("wk", ("none", "random"))
def test_restatement_equals_the_reference_classification_node(golden, nc, wk):
    modes = sorted(k[len("cfg/classify/"):] for k in golden if k.startswith("cfg/classify/"))
    labels_seen = emitted_frames = eos_seen = 0
    for mode in modes:
        nof, delay, wl, wr = (int(v) for v in golden["cfg/classify/" + mode])
        g = {f: golden["off/c/%d/%s/%s/%s" % (nc, wk, mode, f)] for f in ("frame_label", "frame_scores", "eos_label", "eos_scores", "sum_of_weights", "frames_fed")}
        for i, T, rows, s, w in segments(golden, nc):
            r = br.classify_segment(s, w if wk == "random" else None, number_of_features=nof, delay=delay, window_length=wl, window_right=wr)
            what = (mode, T)
            assert np.array_equal(r["frame_label"], g["frame_label"][rows]), what
            assert same(r["frame_scores"], g["frame_scores"][rows]), what
            assert r["eos_label"] == g["eos_label"][i] and same(r["eos_scores"], g["eos_scores"][i]), what
            assert same(np.float32(r["sum_of_weights"]), g["sum_of_weights"][i]) and r["frames_fed"] == g["frames_fed"][i], what
            assert np.array_equal(r["emitted"], r["frame_label"] >= 0) and r["eos"] == (r["eos_label"] >= 0), what   # the fixture has no label without a winner
            labels_seen += len(set(r["frame_label"][r["emitted"]]))
            emitted_frames += int(r["emitted"].sum())
            eos_seen += int(r["eos"])
    assert labels_seen > 20 and emitted_frames > 1000 and eos_seen > 15


@pytest.mark.parametrize("nc", N_CLASSES)
@pytest.mark.parametrize("wk", ("none", "random"))
def test_restatement_equals_the_reference_score_node(golden, nc, wk):
    for mode in sorted(k[len("cfg/scores/"):] for k in golden if k.startswith("cfg/scores/")):
        delay, single = (int(v) for v in golden["cfg/scores/" + mode])
        g = {f: golden["off/s/%d/%s/%s/%s" % (nc, wk, mode, f)] for f in ("out", "emitted", "eos", "eos_out")}
        for i, T, rows, s, w in segments(golden, nc):
            r = br.scores_segment(s, w if wk == "random" else None, delay=delay, single_frame=bool(single))
            assert np.array_equal(r["emitted"], g["emitted"][rows]) and same(r["out"], g["out"][rows]), (mode, T)
            assert r["eos"] == g["eos"][i] and same(r["eos_out"], g["eos_out"][i]), (mode, T)


def test_first_minimum_wins_and_nothing_not_smaller_than_max_does():
    nan, inf, big = np.float32(np.nan), np.float32(np.inf), br.F32_MAX
    assert br.arg_min(np.array([3, 1, 1, 2], np.float32)) == 1
    assert br.arg_min(np.array([nan, nan], np.float32)) == -1 and br.arg_min(np.array([inf, inf, inf], np.float32)) == -1
    assert br.arg_min(np.array([big, big], np.float32)) == -1
    assert br.arg_min(np.array([nan, 5, nan], np.float32)) == 1 and br.arg_min(np.array([inf, -inf], np.float32)) == 1


# ------------------------------------------------------------------ the handle's host logic

def create(**kw):
    L = _lib.lib()
    cfg = _lib.BayesCfg()
    L.amx_bayes_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    st = L.amx_bayes_create(None, C.byref(cfg), C.byref(h))
    return L, h, st, L.amx_last_error().decode()


def test_default_configuration_is_the_nodes():
    L = _lib.lib()
    cfg = _lib.BayesCfg()
    L.amx_bayes_default_cfg(C.byref(cfg))
    assert (cfg.n_classes, cfg.number_of_features, cfg.delay, cfg.window_length, cfg.window_right, cfg.single_frame) == (0, INT_MAX, INT_MAX, -1, 0, 0)


@pytest.mark.parametrize("n", (1, 2, 3, 13, 64, 200, 1 << 20))
def test_prior_is_the_f32_logarithm(n):
    L, h, st, msg = create(n_classes=n)
    assert st == 0, msg
    v = C.c_float()
    assert L.amx_bayes_prior(h, C.byref(v)) == 0 and same(np.float32(v.value), np.log(np.float32(n)))
    L.amx_bayes_destroy(h)


@pytest.mark.parametrize("kw, words", [
    (dict(), ("n_classes is 0",)), (dict(n_classes=-1), ("n_classes is -1",)),
    (dict(n_classes=3, window_length=4, window_right=4), ("window_right 4", "window_length 4")),
    (dict(n_classes=3, window_length=25, window_right=30), ("window_right 30", "window_length 25")),
    (dict(n_classes=3, window_length=4, window_right=-1), ("window_right -1",)),
    (dict(n_classes=3, window_length=4, number_of_features=16), ("number_of_features 16", "window_length 4")),
    (dict(n_classes=3, delay=5, number_of_features=16), ("number_of_features 16", "delay 5")),
])
def test_every_refusal_names_its_parameter(kw, words):
    L, h, st, msg = create(**kw)
    assert st == _lib.AMX_ERR_INVALID and not h.value
    for w in words:
        assert w in msg, msg


def test_accepted_configurations_and_the_python_class():
    import rasr_amd
    for kw in (dict(n_classes=1), dict(n_classes=13, window_length=25, window_right=24, delay=7), dict(n_classes=3, number_of_features=16),
               dict(n_classes=3, delay=0, single_frame=1), dict(n_classes=3, window_right=9),          # window_right unused without a window
               dict(n_classes=3, number_of_features=0, delay=-1, window_length=0)):                    # "unset" in its other spellings
        L, h, st, msg = create(**kw)
        assert st == 0, (kw, msg)
        L.amx_bayes_destroy(h)
    b = rasr_amd.BayesClassifier(None, 13, window_length=4)
    assert same(b.prior(), br.prior(13)) and b.per_frame
    off = np.array([0, 4], np.int64)
    with pytest.raises(rasr_amd.AmxError) as e:
        b.classify(off, np.zeros((4, 13), np.float32), 13, np.zeros(1, np.int32), frame_label_dev=np.zeros(4, np.int32))
    assert e.value.status == _lib.AMX_ERR_STATE
    b.close()
    with pytest.raises(TypeError):
        rasr_amd.BayesClassifier(None, 3, window=4)
    with pytest.raises(rasr_amd.AmxError, match="window_right"):
        rasr_amd.BayesClassifier(None, 3, window_length=2, window_right=2)
    f = [0.88, 1.0, 1.12]
    assert rasr_amd.BayesClassifier.warping_factors([2, 0, 1, 1], f).tolist() == [1.12, 0.88, 1.0, 1.0]
    for bad in ([0, -1], [3]):
        with pytest.raises(ValueError):
            rasr_amd.BayesClassifier.warping_factors(bad, f)


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_bayes_test.cc compiles the handle's host side into a program of its own and walks through every refusal; built with
    -fsanitize=address,undefined on the host side only, run as a process of its own (nothing sanitized is loaded into Python).
    Sanitizers are for machines without a GPU: where one is present the same program is built and run plainly."""
    import torch
    exe = str(tmp_path / "host_bayes_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_bayes_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_bayes_test: ok" in r.stdout, r.stdout + r.stderr
