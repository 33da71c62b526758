"""CPU: linear-segmentation alignment.  The restatement of tests/linseg_reference.py against the reference's own results
(tests/golden/ref_linseg.npz, written by tests/golden/make_linseg_golden.py from the reference's text in both of its builds), bit for bit in
every recorded case; the host logic of the amx_linseg handle (defaults, refusals, segment tables); and that logic once more from a
stand-alone program built with the host sanitizers.  No kernel runs here."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import linseg_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_linseg.npz")
TABLE_MAX_FRAMES = 24


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


_RESTATED = {}


def restated(name, contract):
    """the restatement's result of a case, computed once per session and never changed"""
    if (name, contract) not in _RESTATED:
        c = lr.cases()[name]
        _RESTATED[name, contract] = lr.segment(c["energy"], c["labels"], c["emissions"], contract=contract, table=len(c["energy"]) <= TABLE_MAX_FRAMES,
                                               **c["cfg"])
    return _RESTATED[name, contract]


def recorded(golden, contract, key):
    """an array of the fixture: the native build's where it differs, else the plain build's"""
    return golden["fma/" + key] if contract == "fma" and "fma/" + key in golden else golden["off/" + key]


def test_fixture_holds_what_the_generator_says(golden):
    cases = lr.cases()
    assert len(cases) >= 40
    for name, c in cases.items():
        assert same(golden["in/%s/energy" % name], c["energy"]) and same(golden["in/%s/labels" % name], c["labels"]), name
        assert same(golden["in/%s/emissions" % name], c["emissions"].astype(np.int32)), name
        cfg = dict(lr.DEFAULTS)
        cfg.update(c["cfg"])
        assert golden["cfg/" + name].tolist() == [float(cfg[k]) for k in ("number_of_iterations", "penalty", "minimum_speech_proportion", "should_use_sietill",
                                                                          "minimum_segment_length", "maximum_segment_length")], name
    # the sizes, parameters and outcomes the cases are there for
    sizes = {len(c["energy"]) for c in cases.values()}
    assert {1, 2, 3, 4, 5, 63, 64, 65, 129, 4097} <= sizes
    reason = lambda n: int(golden["off/%s/reason" % n])
    assert reason("d_mismatch_n1") == lr.MISMATCH and reason("d_states_jump") == lr.JUMP
    assert reason("d_minimum_below") == lr.TOO_SHORT and reason("d_minimum_at") == lr.OK
    assert reason("d_maximum_above") == lr.TOO_LONG and reason("d_maximum_at") == lr.OK
    assert float(golden["off/d_gate_none/score"]) == lr.DBL_MAX and float(golden["off/d_quiet_speech/score"]) == lr.DBL_MAX
    assert float(golden["off/d_iterations_0/score"]) == lr.DBL_MAX and float(golden["off/d_iterations_1/score"]) < 0
    assert (int(golden["off/d_proportion_1/begin"]), int(golden["off/d_proportion_1/end"])) == (0, 63)
    assert (int(golden["off/s_iterations_0/begin"]), int(golden["off/s_iterations_0/end"])) == (0, 128)      # Sietill's iEnd starts at N
    assert (int(golden["off/d_iterations_0/begin"]), int(golden["off/d_iterations_0/end"])) == (0, 127)
    assert (int(golden["off/d_n2/begin"]), int(golden["off/d_n2/end"])) == (0, 0) and (int(golden["off/d_n3/begin"]), int(golden["off/d_n3/end"])) == (0, 1)
    # the two builds: fused multiply-adds exist in the native one only, they change likelihoods, and the site is the one the restatement fuses
    assert int(golden["fma_instructions/off"]) == 0 and int(golden["fma_instructions/fma"]) > 0
    differs = [k for k in golden["fma_differs"].tolist() if k]
    assert differs and all("fma/" + k in golden for k in differs) and any(k.endswith("/table") for k in differs)
    assert not [k for k in differs if k.endswith(("/M", "/Q"))]                                              # x * x is exact: the chains agree
    assert golden["fma_sites"].tolist() == ["sum=%s" % lr.FMA_SITES["sum"]]
    # the cap on the weaker check: only the deliberately degenerate cases may be undecided
    undecided = [n for n in golden["undecided"].tolist() if n]
    assert undecided and all(lr.is_tie(n) for n in undecided)
    for name in cases:
        assert golden["decided/" + name].tolist() == [bool(restated(name, "off")["decided"]), bool(restated(name, "fma")["decided"])], name
        assert name in undecided or all(golden["decided/" + name])


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", sorted(lr.cases()))
def test_restatement_equals_the_reference(golden, name, contract):
    """chains, likelihood tables, delimitations, scores, item lists and reasons, in every bit"""
    r, g = restated(name, contract), lambda f: recorded(golden, contract, "%s/%s" % (name, f))
    assert r["reason"] == int(g("reason")), (lr.REASONS[r["reason"]], lr.REASONS[int(g("reason"))])
    assert (r["begin"], r["end"]) == (int(g("begin")), int(g("end")))
    assert same(np.float64(r["score"]), g("score"))
    assert np.array_equal(r["label"], g("label")) and np.array_equal(r["emission"], g("emission"))
    assert int(g("n_items")) == (len(r["label"]) if r["reason"] == lr.OK else 0)
    if r["M"] is not None:
        assert same(r["M"], g("M")) and same(r["Q"], g("Q"))
    if r["table"] is not None:
        assert same(r["table"], g("table"))
    assert bool(r["decided"]) == bool(golden["decided/" + name][0 if contract == "off" else 1])
    assert r["decided"] or lr.is_tie(name)


def test_the_fused_multiply_add_is_exact():
    """the fallback of math.fma: the rational a * b + c rounded once, against cases whose two roundings differ"""
    a, b, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -(1.0 + 2.0 ** -29)
    assert a * b + c == 0.0 and lr.fma(a, b, c) == 2.0 ** -60
    assert lr.fma(3.0, 0.1, 0.7) == float(3 * lr.Fraction(0.1) + lr.Fraction(0.7))
    assert lr.fma(2.0, 0.0, -1.5) == -1.5 and math.isinf(lr.fma(1e308, 10.0, 0.0)) and math.isnan(lr.fma(math.nan, 1.0, 1.0))
    rng = np.random.Generator(np.random.PCG64(5))
    n = 0
    for x, y, z in rng.standard_normal((2000, 3)):
        f = lr.fma(float(x), float(y), float(z))
        exact = lr.Fraction(float(x)) * lr.Fraction(float(y)) + lr.Fraction(float(z))
        assert abs(lr.Fraction(f) - exact) <= abs(lr.Fraction(float(x) * float(y) + float(z)) - exact)
        n += f != float(x) * float(y) + float(z)
    assert n > 50   # the two forms do differ


def test_added_rule_and_decided_flag_of_the_restatement():
    lab, emi = lr.states(3)
    e = lr.track(40, 3)
    for bad in (np.nan, np.inf, -np.inf):
        x = e.copy()
        x[17] = bad
        assert lr.segment(x, lab, emi)["reason"] == lr.NONFINITE
    assert lr.segment(np.full(4, 3e38, np.float32), lab, emi, penalty=1e-290)["reason"] == lr.NONFINITE     # Q_ leaves the finite range
    assert lr.segment(e, lab[:0], emi[:0])["reason"] == lr.NO_STATES and lr.segment(e[:0], lab, emi)["reason"] == lr.NO_STATES
    # a logarithm one ulp off gives the same delimitation and labels wherever the case is decided
    up = lambda v: np.nextafter(lr.log_ieee(v), np.inf).item()
    down = lambda v: np.nextafter(lr.log_ieee(v), -np.inf).item()
    for name in ("d_n65", "s_n65", "d_penalty_0", "s_proportion_03", "d_states_speech"):
        c, r = lr.cases()[name], restated(name, "off")
        assert r["decided"]
        for log in (up, down):
            o = lr.segment(c["energy"], c["labels"], c["emissions"], log=log, **c["cfg"])
            assert (o["begin"], o["end"], o["reason"]) == (r["begin"], r["end"], r["reason"]) and np.array_equal(o["label"], r["label"])
            S = lr.score_of(c["energy"], r["begin"], r["end"], **c["cfg"])[1]
            assert abs(o["score"] - r["score"]) <= lr.SCORE_MARGIN * S
    assert not restated("tie_constant_d", "off")["decided"] and not restated("tie_constant_s", "fma")["decided"]


# ------------------------------------------------------------------ the handle's host logic

def create(**kw):
    from rasr_amd import _lib
    L = _lib.lib()
    cfg = _lib.LinsegCfg()
    L.amx_linseg_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    st = L.amx_linseg_create(None, C.byref(cfg), C.byref(h))
    return L, h, st, L.amx_last_error().decode()


def test_default_configuration_is_the_segmenters():
    from rasr_amd import _lib
    L = _lib.lib()
    cfg = _lib.LinsegCfg()
    L.amx_linseg_default_cfg(C.byref(cfg))
    got = dict(number_of_iterations=cfg.number_of_iterations, penalty=cfg.penalty, minimum_speech_proportion=cfg.minimum_speech_proportion,
               should_use_sietill=cfg.should_use_sietill, minimum_segment_length=cfg.minimum_segment_length,
               maximum_segment_length=cfg.maximum_segment_length)
    want = dict(lr.DEFAULTS, minimum_speech_proportion=float(np.float32(0.7)))   # the reference's parameter defaults (:81-94, :249-262)
    assert got == want
    assert lr.DEFAULTS == dict(number_of_iterations=3, penalty=100.0, minimum_speech_proportion=0.7, should_use_sietill=0, minimum_segment_length=1,
                               maximum_segment_length=2**31 - 1)
    assert (_lib.AMX_LINSEG_OK, _lib.AMX_LINSEG_TOO_SHORT, _lib.AMX_LINSEG_TOO_LONG, _lib.AMX_LINSEG_NO_STATES, _lib.AMX_LINSEG_JUMP, _lib.AMX_LINSEG_MISMATCH,
            _lib.AMX_LINSEG_NONFINITE, _lib.AMX_LINSEG_N_REASONS) == (lr.OK, lr.TOO_SHORT, lr.TOO_LONG, lr.NO_STATES, lr.JUMP, lr.MISMATCH, lr.NONFINITE, lr.N_REASONS)


@pytest.mark.parametrize("kw, words", [
    (dict(number_of_iterations=-1), ("number_of_iterations -1",)),
    (dict(penalty=float("nan")), ("penalty", "not a number")),
    (dict(penalty=-0.5), ("penalty -0.5",)),
    (dict(minimum_speech_proportion=float("nan")), ("minimum_speech_proportion", "not a number")),
    (dict(minimum_speech_proportion=1.25), ("minimum_speech_proportion 1.25", "[0, 1]")),
    (dict(minimum_speech_proportion=-0.5), ("minimum_speech_proportion -0.5",)),
    (dict(minimum_segment_length=-1), ("minimum_segment_length -1",)),
    (dict(maximum_segment_length=-7), ("maximum_segment_length -7",)),
])
def test_every_refused_configuration_names_its_field(kw, words):
    from rasr_amd import _lib
    L, h, st, msg = create(**kw)
    assert st == _lib.AMX_ERR_INVALID and not h.value, msg
    for w in words:
        assert w in msg, msg


def test_accepted_configurations():
    for kw in (dict(), dict(penalty=0.0, number_of_iterations=0), dict(minimum_speech_proportion=1.0, should_use_sietill=1),
               dict(minimum_speech_proportion=0.0, minimum_segment_length=0, maximum_segment_length=0)):
        L, h, st, msg = create(**kw)
        assert st == 0, (kw, msg)
        L.amx_linseg_destroy(h)


def host_call(frame_offsets, segments, silence=(lr.SILENCE_LABEL, lr.SILENCE_EMISSION), energy_ld=1, **patch):
    """amx_linseg_align_dev on a handle without a context: the checks run, then the call stops with AMX_ERR_STATE before any device work"""
    import rasr_amd
    a = rasr_amd.LinearSegmenter(None)
    m = rasr_amd.LinearSegmenter.models(segments, *silence)
    for k, (i, v) in patch.items():
        m[k] = m[k].copy()
        m[k][i] = v
    try:
        a.align(frame_offsets, m, None, energy_ld)
    except rasr_amd.AmxError as e:
        return e.status, str(e)
    finally:
        a.close()
    return 0, ""


def test_host_only_handle_validates_and_refuses():
    from rasr_amd import _lib
    segs = [lr.states(3), lr.states(0), lr.states(4, first=7)]
    assert host_call([0, 5, 9, 20], segs)[0] == _lib.AMX_ERR_STATE                                # a valid batch reaches the context check
    for kw, words in (
            (dict(frame_offsets=[0, 5, 4, 20]), ("frame offsets decrease at segment 1",)),
            (dict(frame_offsets=[-2, 5, 9, 20]), ("negative frame offset",)),
            (dict(frame_offsets=[0, 5, 9, 2**31]), ("2^31",)),
            (dict(energy_ld=0), ("energy_ld 0",)),
            (dict(state_label=(1, -1)), ("segment 0", "state_label[1] = -1")),
            (dict(state_emission=(4, -3)), ("segment 2", "state_emission[4] = -3")),
            (dict(state_offsets=(0, 1)), ("state_offsets[0] is 1",)),
            (dict(state_offsets=(2, 1)), ("state_offsets decrease at segment 1",)),
            (dict(silence=(-1, 0)), ("silence_label -1",)),
            (dict(silence=(5, -1)), ("silence_emission -1",))):
        kw = dict(kw)
        st, msg = host_call(kw.pop("frame_offsets", [0, 5, 9, 20]), segs, **kw)
        assert st == _lib.AMX_ERR_INVALID, (kw, msg)
        for w in words:
            assert w in msg, msg


def test_the_python_class_and_the_new_names():
    import rasr_amd
    from rasr_amd import _lib
    for n in ("amx_linseg_default_cfg", "amx_linseg_create", "amx_linseg_destroy", "amx_linseg_align_dev"):
        assert n in _lib.SIGNATURES
    assert "LinearSegmenter" in rasr_amd.__all__
    with pytest.raises(TypeError):
        rasr_amd.LinearSegmenter(None, beam=3)
    with pytest.raises(rasr_amd.AmxError, match="penalty"):
        rasr_amd.LinearSegmenter(None, penalty=-1)
    m = rasr_amd.LinearSegmenter.models([([4, 5, 6], [1, 1, 2]), ([], []), ([9], [0])], 77, 3)
    assert m["state_offsets"].tolist() == [0, 3, 3, 4] and m["state_label"].tolist() == [4, 5, 6, 9] and m["state_emission"].tolist() == [1, 1, 2, 0]
    assert (m["silence_label"], m["silence_emission"]) == (77, 3)
    with pytest.raises(ValueError):
        rasr_amd.LinearSegmenter.models([([1, 2], [1])], 0, 0)
    with pytest.raises(ValueError):
        rasr_amd.LinearSegmenter(None).align([0, 1, 2], m, None)


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_linseg_test.cc compiles the handle's host side into a program of its own: every refusal, the segment table of a batch and
    the host instantiation of the kernel's likelihood and index functions; built with -fsanitize=address,undefined on the host side only,
    run as a process of its own (nothing sanitized is loaded into Python).  Sanitizers are for machines without a GPU: where one is
    present the same program is built and run plainly."""
    import torch
    exe = str(tmp_path / "host_linseg_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_linseg_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_linseg_test: ok" in r.stdout, r.stdout + r.stderr
