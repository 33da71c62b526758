"""CPU tests of the NN layer types behind amx_ffnn_create_ex: the numpy restatement (tests/nn_layers_reference.py) against the
reference's own unit test, and the Math::Vector<u32> reader of maxoutvar's `maxout-sizes` file.  No kernel runs here."""
import json
import os
import struct

import numpy as np
import pytest

from tests import nn_layers_reference as ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_restatement_reproduces_the_reference_unit_test():
    """Test/Nn_PreprocessingLayer.cc: the logarithm case and the mean-and-variance case with stddev -0.5"""
    kat = json.load(open(os.path.join(GOLD, "nn_preprocessing_kat.json")))
    x = np.array(kat["input"], np.float32)
    for case in kat["cases"]:
        got = ref.preprocess(x, [tuple(l) for l in case["layers"]])
        assert got.dtype == np.float32
        assert np.allclose(got.astype(np.float64), np.array(case["expected"]), rtol=0, atol=kat["tol"]), (case["name"], got)


def test_restatement_arithmetic():
    """(x - m) * ((f32)1 / s): a zero stddev gives inf / NaN like the reference; log of 0 is -inf; maxout keeps a leading NaN"""
    x = np.array([[3.0, 0.0, -1.0]], np.float32)
    y = ref.mean_and_variance(x, [1.0, 0.0, 0.0], [3.0, 0.0, 2.0])
    assert y[0, 0] == np.float32(2.0) * (np.float32(1) / np.float32(3)) and np.isnan(y[0, 1]) and y[0, 2] == np.float32(-0.5)
    assert ref.logarithm(np.float32([0.0]))[0] == -np.inf
    nan = np.float32("nan")
    m = ref.maxoutvar(np.array([[nan, 5.0, 1.0, nan, 2.0, 7.0]], np.float32), [2, 2, 1, 1])
    assert np.isnan(m[0, 0]) and m[0, 1] == 1.0 and m[0, 2] == 2.0 and m[0, 3] == 7.0
    assert ref.elu(np.float32([-1.0]))[0] == np.float32(np.exp(-1.0)) - np.float32(1) and ref.elu(np.float32([2.5]))[0] == 2.5


def _xml(path, tag, values):
    with open(path, "w") as f:
        f.write('<?xml version="1.0" encoding="ISO-8859-1"?>\n<%s size="%d">\n  %s\n</%s>\n' % (tag, len(values), " ".join(map(str, values)), tag))


def test_vector_u32_round_trips_xml_and_bin(tmp_path):
    import rasr_amd
    sizes = [3, 1, 4, 1, 5, 9, 2, 6]
    _xml(str(tmp_path / "s.xml"), "vector-u32", sizes)
    got = rasr_amd.read_maxout_sizes(str(tmp_path / "s.xml"))
    assert got.dtype == np.uint32 and got.tolist() == sizes
    with open(tmp_path / "s.bin", "wb") as f:
        f.write(struct.pack("<I", len(sizes)) + np.array(sizes, "<u4").tobytes())
    assert rasr_amd.read_maxout_sizes("bin:" + str(tmp_path / "s.bin")).tolist() == sizes


def test_vector_u32_refuses_other_element_types(tmp_path):
    import rasr_amd
    _xml(str(tmp_path / "f.xml"), "vector-f32", [1.0, 2.0])
    with pytest.raises(rasr_amd.AmxError, match="vector-u32"):
        rasr_amd.read_maxout_sizes(str(tmp_path / "f.xml"))
    _xml(str(tmp_path / "n.xml"), "vector-u32", [2, -1])
    with pytest.raises(rasr_amd.AmxError):
        rasr_amd.read_maxout_sizes(str(tmp_path / "n.xml"))
    with open(tmp_path / "short.bin", "wb") as f:
        f.write(struct.pack("<I", 4) + np.array([1, 2], "<u4").tobytes())
    with pytest.raises(rasr_amd.AmxError):
        rasr_amd.read_maxout_sizes("bin:" + str(tmp_path / "short.bin"))
