"""CPU: the lattice word measures' host side through the ABI on a handle without a context (the checks run, then AMX_ERR_STATE), the
symbols, and the restatement's collector against a direct evaluation of hand-written feeds."""
import ctypes as C

import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import latword_reference as wr

GOOD = wr.lattice([0, 5, 2], [(0, 1, 7), (0, 2, 7), (2, 1, -1)])


def status(mode, lat, correct=None):
    m = rasr_amd.LatticeWordMeasures(None, mode)
    try:
        m.run_dev(m.tables([lat]), m.tables([correct]) if correct is not None else None, None, None)
    except rasr_amd.AmxError as e:
        return e.status, str(e)
    return 0, ""


def test_symbols_and_shape():
    assert "LatticeWordMeasures" in rasr_amd.__all__
    assert all(hasattr(_lib.lib(), n) for n in _lib.SIGNATURES if n.startswith("amx_latword_"))
    shape = rasr_amd.LatticeWordMeasures.kernel_shape()
    assert shape["block_frames"] == 64 and shape["list_arcs"] > 64 and shape["wave_arc_frames"] >= 64


@pytest.mark.parametrize("case, text", [("mode", "mode 9"), ("normalization", "not finite"), ("time", "state_time decreases"), ("target", "outside its"),
                                        ("correct", "correct lattices"), ("good", "without a context")])
def test_host_refusals(case, text):
    if case in ("mode", "normalization"):
        cfg, h = _lib.LatwordCfg(9 if case == "mode" else 0, 0.0 if case == "mode" else float("inf")), C.c_void_p()
        assert _lib.lib().amx_latword_create(None, C.byref(cfg), C.byref(h)) == _lib.AMX_ERR_INVALID
        assert text in _lib.lib().amx_last_error().decode()
        return
    lat = dict(GOOD)
    if case == "time":
        lat["state_time"] = np.array([0, 5, 6], np.int32)
    if case == "target":
        lat["arc_target"] = np.array([1, 3, 1], np.int32)
    st, msg = status("approximate-word" if case == "correct" else "timeframe-error-sum", lat)
    assert st == (_lib.AMX_ERR_STATE if case == "good" else _lib.AMX_ERR_INVALID) and text in msg, (st, msg)


@pytest.mark.parametrize("feeds", [[0.5, 0.5, 0.5], [2.0, 1.5, 0.25], [1.25], [0.75, 3.0, 0.75, 0.1]], ids=["tie", "minimum-last", "single", "mixed"])
def test_collector_matches_a_direct_evaluation(feeds):
    """-log sum exp(-a): the stored values are a permutation of the feeds without one copy of the minimum"""
    direct = -np.log(np.sum(np.exp(-np.array(feeds, np.float64))))
    assert wr.collect(feeds, exact=True) == pytest.approx(direct, abs=1e-15)
    assert abs(float(wr.collect(feeds)) - direct) <= (len(feeds) + 4) * 2.0 ** -23
    if len(feeds) == 1:
        assert wr.collect(feeds) == np.float32(feeds[0])
