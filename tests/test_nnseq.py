"""CPU: the restatement of the sequence-discriminative NN training (tests/nnseq_reference.py) against tests/golden/ref_nnseq.npz, which
tests/golden/make_nnseq_golden.py recorded from the reference's own text (collection, rejection, arc score, and the smoothing and
weighting over BLAS);
every planted defect of the restatement is seen by at least one case; the MMI error signal is the derivative of the objective; and the
host-side refusals of amx_nnseq_* through the ABI on a handle without a device."""
import functools
import os

import numpy as np
import pytest

from tests import nnseq_reference as sr

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_nnseq.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def lattice_case(flow, defect=None):
    net, off, feats, emission, *_ = sr.gpu_batch()
    return sr.process(net, feats, off, emission, sr.gpu_flows()[flow], np.zeros(5, F32), rejection=0.3, defect=defect, gradient=True)


def smooth_case(defect=None):
    net, off, feats, emission, *_ = sr.gpu_batch()
    return sr.process(net, feats, off, emission, sr.gpu_flows()["mmi"], np.zeros(5, F32), lam=float(F32(0.3)), rejection=0.3, defect=defect)


def smooth_prior_case(defect=None):
    net, off, feats, emission, *_ = sr.gpu_batch()
    return sr.process(net, feats, off, emission, sr.gpu_flows()["mmi"], np.zeros(5, F32), lam=float(F32(0.3)), rejection=0.3, defect=defect,
                      log_prior=fixture()["smooth_log_prior"], prior_scale=0.7)


def score_case(defect=None):
    net, off, feats, emission, den, *_ = sr.gpu_batch()
    return [sr.arc_scores(net, sr.forward(net, feats[off[s]:off[s + 1]])[1], den, s, defect) for s in range(5)]


def order_result(defect=None):
    net = sr.network()
    e0 = int(sr.valid_classes(net)[7])
    tables, w, thr = sr.order_case(e0)
    E, _ = sr.lattice_error(net, 1, 0, [dict(tables=tables, arc_weight=w, factor=1.0)], None, None, thr, defect=defect)
    return E, sr.class_to_output(net, e0)


def narrowing_result(defect=None):
    net = sr.network()
    e0 = int(sr.valid_classes(net)[7])
    passes, thr = sr.narrowing_case(e0)
    E, _ = sr.lattice_error(net, 1, 0, passes, None, None, thr, defect=defect)
    return E, sr.class_to_output(net, e0)


def chunked_case(defect=None):
    net, off, feats, emission, *_ = sr.gpu_batch()
    st = sr.process(net, feats, off, emission, sr.gpu_flows()["mmi"], np.linspace(-3, 5, 5).astype(F32), rejection=0.3, products="f32", defect=defect)["stats"]
    return np.concatenate([g.reshape(-1) for g in st["gradient_weights"]])


@pytest.mark.parametrize("flow", ["mmi", "me", "me-rejection"])
def test_collection_and_rejection_equal_the_reference_text_in_every_bit(flow):
    fx = fixture()
    for s, seg in enumerate(lattice_case(flow)["segments"]):
        assert np.array_equal(bits(seg["E_lattice"]), fx["E_lattice/%s/%d" % (flow, s)]), (flow, s)
        assert np.array_equal(bits(seg["w"]), fx["w/%s/%d" % (flow, s)]), (flow, s)
        assert seg["rejected"] == fx["rejected/%s/%d" % (flow, s)][0], (flow, s)


def test_scores_smoothing_and_the_two_rounding_cases_equal_the_fixture_in_every_bit():
    fx = fixture()
    for s, sc in enumerate(score_case()):
        assert np.array_equal(bits(sc), fx["scores/%d" % s]), s
    for s, seg in enumerate(smooth_case()["segments"]):
        assert np.array_equal(bits(seg["E"]), fx["E_smooth/%d" % s]), s
    for s, seg in enumerate(smooth_prior_case()["segments"]):
        assert np.array_equal(bits(seg["E"]), fx["E_smooth_prior/%d" % s]), s
    assert np.array_equal(bits(order_result()[0]), fx["order/E"])
    assert np.array_equal(bits(narrowing_result()[0]), fx["narrowing/E"])
    assert np.array_equal(chunked_case(), fx["chunked/mmi"])


def test_the_order_sensitive_key_follows_from_the_arithmetic():
    """f32 weights 1, 2^-24, 2^-53, 2^-53 on one key: in arc order the f64 sum is 1 + 2^-24 (each 2^-53 is half an ulp of the running
    sum and the tie goes to the even neighbour), which narrows to 1.0 (again a tie to even); in the other order the two small terms
    join to 2^-52 first: 1 + 2^-24 + 2^-52, which lies above the tie and narrows to 1 + 2^-23"""
    w = [np.float64(F32(x)) for x in (1.0, 2.0 ** -24, 2.0 ** -53, 2.0 ** -53)]
    forward = ((w[0] + w[1]) + w[2]) + w[3]
    backward = ((w[3] + w[2]) + w[1]) + w[0]
    assert forward == 1 + 2.0 ** -24 and F32(forward) == F32(1.0)
    assert backward == 1 + 2.0 ** -24 + 2.0 ** -52 and F32(backward) == F32(1 + 2.0 ** -23)
    E, o = order_result()
    assert E[0, o] == F32(1.0)
    E, o = order_result("collection-order")
    assert E[0, o] == F32(1 + 2.0 ** -23)
    E, o = narrowing_result()
    assert E[0, o] == F32(1 + 2.0 ** -23)
    E, o = narrowing_result("factor-after-narrowing")
    assert E[0, o] == F32(1.0)


def differs(a, b):
    return not np.array_equal(np.asarray(a).view(np.uint8) if isinstance(a, np.ndarray) else a, np.asarray(b).view(np.uint8) if isinstance(b, np.ndarray) else b)


@pytest.mark.parametrize("defect", sr.DEFECTS)
def test_every_planted_defect_changes_a_case(defect):
    fx = fixture()
    if defect == "collection-order":
        assert differs(bits(order_result(defect)[0]), fx["order/E"])
    elif defect == "factor-after-narrowing":
        assert differs(bits(narrowing_result(defect)[0]), fx["narrowing/E"])
    elif defect == "non-strict-threshold":   # an arc whose weight equals the threshold
        assert any(differs(bits(seg["E_lattice"]), fx["E_lattice/mmi/%d" % s]) for s, seg in enumerate(lattice_case("mmi", defect)["segments"]))
    elif defect == "rejection-wrong-row":
        assert any(differs(bits(seg["w"]), fx["w/mmi/%d" % s]) for s, seg in enumerate(lattice_case("mmi", defect)["segments"]))
    elif defect in ("smoothing-order", "weights-before-smoothing"):
        assert any(differs(bits(seg["E"]), fx["E_smooth/%d" % s]) for s, seg in enumerate(smooth_case(defect)["segments"]))
        assert any(differs(bits(seg["E"]), fx["E_smooth_prior/%d" % s]) for s, seg in enumerate(smooth_prior_case(defect)["segments"]))
    elif defect == "chunks-across-segments":
        assert differs(chunked_case(defect), fx["chunked/mmi"])
    elif defect == "zero-item-arc-nonzero":
        assert any(differs(bits(sc), fx["scores/%d" % s]) for s, sc in enumerate(score_case(defect)))
    else:
        raise AssertionError("no case for %s" % defect)


def test_mmi_error_signal_is_the_derivative_of_the_objective():
    """all in f64, threshold 0, no smoothing: E = d objective / d output, objective = log of the denominator's total flow minus the
    numerator's, through arc scores and an enumeration of the paths; central differences at the fixture's step (1e-5: the truncation
    error h^2 f''' / 6 and the rounding error eps / h are both near 1e-11)"""
    fx = fixture()
    step = float(fx["derivative_step"][0])
    assert step == 1e-5
    dev = sr.mmi_derivative_deviation(*sr.derivative_case(), step)
    print("deviation %.3g, bar %.3g" % (dev, fx["derivative_bar"][0]))
    assert dev <= fx["derivative_bar"][0] < 1e-8


def test_the_restatement_refuses_what_the_device_refuses():
    net, off, feats, emission, den, num, w_den, w_num, _ = sr.gpu_batch()
    bad = dict(den, item_frame=np.array(den["item_frame"]))
    first = int(den["item_offsets"][int(den["arc_offsets"][2])])
    bad["item_frame"][first] = 256
    with pytest.raises(sr.Refused, match="frame"):
        sr.process(net, feats, off, emission, [dict(tables=bad, arc_weight=w_den, factor=1.0)], np.zeros(5, F32))
    with pytest.raises(sr.Refused, match="cell"):
        sr.process(net, feats, off, emission, [dict(tables=den, arc_weight=w_den, factor=-1.0, role=sr.REJECT)], np.zeros(5, F32), rejection=0.3)
    em = np.array(emission)
    em[7] = sr.NO_ALIGNMENT
    got = sr.process(net, feats, off, em, sr.gpu_flows()["mmi"], np.zeros(5, F32), skip=[1, 0, 0, 0, 0])
    assert [s["reason"] for s in got["segments"]] == ["skipped", "no-alignment", "ok", "ok", "ok"]
    assert got["stats"]["n_observations"] == 256 + 257 + 300


# ------------------------------------------------------------------------------------ the ABI on a handle without a device
def host_trainer(statistics=("base", "gradient")):
    import rasr_amd
    net = sr.network()
    return net, rasr_amd.FeedForwardTrainer(None, net.Ws, net.bs, net.acts, statistics=statistics, class_weights=net.class_weights, class_to_output=net.class_to_output)


def test_host_refusals_through_the_abi():
    import rasr_amd
    from rasr_amd import _lib
    net, tr = host_trainer()
    for kw, status, word in ((dict(full_batch=False), _lib.AMX_ERR_UNSUPPORTED, "full_batch"), (dict(accumulate_prior=True), _lib.AMX_ERR_UNSUPPORTED, "accumulate_prior"),
                             (dict(label_type="allophone-state-ids"), _lib.AMX_ERR_UNSUPPORTED, "label_type"), (dict(ce_smoothing_weight=1.5), _lib.AMX_ERR_INVALID, "ce_smoothing_weight"),
                             (dict(frame_rejection_threshold=-0.1), _lib.AMX_ERR_INVALID, "frame_rejection_threshold"),
                             (dict(ce_smoothing_weight=0.5, prior_scale=1.0), _lib.AMX_ERR_INVALID, "log_prior")):
        with pytest.raises(rasr_amd.AmxError, match=word) as e:
            rasr_amd.SegmentwiseNnTrainer(tr, **kw)
        assert e.value.status == status, kw
    _, counts = host_trainer(("class-counts", "base"))
    with pytest.raises(rasr_amd.AmxError, match="base statistics and the gradient only"):
        rasr_amd.SegmentwiseNnTrainer(counts)
    _, nobase = host_trainer(("gradient",))
    with pytest.raises(rasr_amd.AmxError, match="base statistics"):
        rasr_amd.SegmentwiseNnTrainer(nobase)
    with pytest.raises(rasr_amd.AmxError, match="maxout"):   # what amx_nntrain_create refuses stays refused
        rasr_amd.FeedForwardTrainer(None, net.Ws, net.bs, net.acts, maxout={0: 3})
    seq = rasr_amd.SegmentwiseNnTrainer(tr)
    x = np.zeros((8, 20), F32)
    with pytest.raises(rasr_amd.AmxError, match="cap of 4096 frames") as e:   # 17 segments of one frame: 17 x 256 rows
        seq.forward_dev(x, 20, np.arange(18))
    assert e.value.status == _lib.AMX_ERR_INVALID
    with pytest.raises(rasr_amd.AmxError, match="do not ascend"):
        seq.forward_dev(x, 20, [0, 5, 3])
    with pytest.raises(rasr_amd.AmxError, match="without a context") as e:
        seq.forward_dev(x, 20, [0, 4, 8])
    assert e.value.status == _lib.AMX_ERR_STATE
    shape = seq.kernel_shape()
    assert shape["threads"] == 256 and shape["sort_block_items"] % shape["threads"] == 0 and shape["score_block_arcs"] * 64 == shape["threads"]
    cfg = _lib.NnSeqCfg()
    _lib.lib().amx_nnseq_default_cfg(cfg)
    assert cfg.weight_threshold == float(np.finfo(F32).eps) and cfg.ce_smoothing_weight == 0 and cfg.frame_rejection_threshold == 0 and cfg.full_batch == 1
    seq.close(), tr.close()


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_nnseq_test.cc compiles nnseq_host.cpp into a program of its own: the row plan of a batch against the restatement's, the
    checks of the arc tables on heap blocks of exactly their size, every host refusal, the key layout, the sizes of the sort's workspaces
    and the decoding of the device's refusal word; built with -fsanitize=address,undefined on the host side only and run as a process of
    its own (nothing sanitized is loaded into Python).  Where a GPU is present the same program is built and run plainly."""
    import subprocess

    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_nnseq_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(root, "tests", "host_nnseq_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    _, off, _, _, den, *_ = sr.gpu_batch()
    off = np.concatenate([off, [off[-1]]])   # and a segment without frames at the end
    den = dict(den, arc_offsets=np.concatenate([den["arc_offsets"], [den["arc_offsets"][-1]]]))
    rows, row0, row_src = sr.row_plan(off)
    assert rows == 256 + 256 + 256 + 512 + 512 and list(row0) == [0, 256, 512, 768, 1280, 1792, 1792]
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        np.array([len(off) - 1], np.int32).tofile(f)
        np.asarray(off, np.int64).tofile(f)
        for k, t in (("arc_offsets", np.int64), ("item_offsets", np.int64), ("item_frame", np.int32), ("item_emission", np.int32)):
            np.asarray(den[k], t).tofile(f)
        np.array([rows], np.int32).tofile(f)
        row0.tofile(f)
        row_src.tofile(f)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "host_nnseq_test: ok (6 segments, 1792 rows, 65 arcs" in r.stdout, r.stdout + r.stderr
