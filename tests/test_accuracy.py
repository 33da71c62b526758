"""CPU: lattice arc accuracies.  The host refusals of amx_accuracy_create and amx_accuracy_run_dev through the ABI on a handle without a
context (every host check comes before the context is asked for), the symbols of the built library and the kernel's shape.  No kernel
runs here."""
import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib

INV = _lib.AMX_ERR_INVALID
# keys (segment, tbeg, tend), slot_offsets (None: the prefix sum), status, words of the message; two segments
RUN_REFUSALS = [([(0, 2, 2)], None, INV, ("key 0", "begin time 2")),
                ([(0, 0, 4), (1, 5, 3)], None, INV, ("key 1", "begin time 5")),
                ([(0, 0, 4), (2, 0, 3)], None, INV, ("key 1", "segment 2")),
                ([(-1, 0, 4)], None, INV, ("key 0", "segment -1")),
                ([(0, -1, 4)], None, INV, ("key 0", "negative")),
                ([(0, 0, 4), (1, 0, 3)], [0, 4, 8], INV, ("key 1", "4 slots", "3 frames")),
                ([(0, 0, 4)], [1, 5], INV, ("slot_offsets start at 1",)),
                ([(0, 0, 4)], None, _lib.AMX_ERR_STATE, ("without a context",))]
CREATE_REFUSALS = [(dict(mode=3), "mode 3"), (dict(normalization=float("inf")), "not finite"), (dict(normalization=float("nan")), "not finite"),
                   (dict(label_token=[0, 5, 1]), "label_token[1] = 5"), (dict(label_token=[0, -1]), "label_token[1] = -1"), (dict(n_tokens=0), "n_tokens 0")]


@pytest.mark.parametrize("case", range(len(RUN_REFUSALS)))
def test_host_refusals_on_a_handle_without_context(case):
    keys, slots, status, words = RUN_REFUSALS[case]
    seg, tbeg, tend = np.array(keys, np.int32).T
    slots = np.concatenate([[0], np.cumsum(tend - tbeg)]) if slots is None else slots
    a = rasr_amd.LatticeAccuracy(None, "approximate-phone", 5, label_token=[0, 1, 2])
    with pytest.raises(rasr_amd.AmxError) as e:
        a.run(seg, tbeg, tend, slots, np.ones(len(keys)), None, 2)
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    assert a.run([], [], [], [0], [], None, 2)[1] == dict(runs=0, reference_intervals=0, keys_without_alignment=0)
    a.close()


@pytest.mark.parametrize("kw,word", CREATE_REFUSALS)
def test_configurations_create_refuses(kw, word):
    args = dict(dict(mode="frame-phone", n_tokens=5), **kw)
    with pytest.raises(rasr_amd.AmxError) as e:
        rasr_amd.LatticeAccuracy(None, **args)
    assert e.value.status == INV and word in str(e.value), str(e.value)


def test_symbols_and_kernel_shape():
    L = _lib.lib()
    for name in ("create", "destroy", "run_dev", "arc_dev", "kernel_shape", "set_lds_intervals", "last_reference"):
        assert hasattr(L, "amx_accuracy_" + name)
    shape = rasr_amd.LatticeAccuracy.kernel_shape()
    assert shape["frames_per_trip"] == 64 and shape["keys_per_workgroup"] % 4 == 0, "one frame per lane, four waves share a workgroup's keys"
    assert 4 * 16 * shape["lds_intervals"] <= 160 * 1024, "four workgroups' tables (16 bytes per interval) fit a CU's LDS"
    a = rasr_amd.LatticeAccuracy(None, "frame-state", 5)
    with pytest.raises(rasr_amd.AmxError):
        a.set_lds_intervals(shape["lds_intervals"] + 1)
    a.close()
