"""CPU: lattice word-arc alignment.  The host refusals of amx_arcalign_run_dev through the ABI on a handle without a context (every check
comes before the context is asked for), amx_arcalign_expand against a few lines of numpy, and the symbols of the built library.  No kernel
runs here."""
import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import align_reference as ar

N = ar.N_COLUMNS


def fan_in(n_in):
    """n_in arcs into the last state, 62 at the most from each of the states before it, which loop and which one arc each chains"""
    n_src = -(-n_in // 62)
    arcs = [(s, n_src, (s * 62 + i) % N, s * 62 + i, float(i % 3)) for s in range(n_src) for i in range(min(62, n_in - 62 * s))]
    arcs += [(s, s, s % N, 6000 + s, 1.0) for s in range(n_src)] + [(s, s + 1, s % N, 5000 + s, 1.0) for s in range(n_src - 1)]
    return ar.graph(n_src + 1, 0, {n_src: 0.0}, arcs)


def refusals():
    """(graphs, patch of the graph tables, keys (graph, segment, tbeg, tend), status, words of the message); segments of 9 and 6 frames"""
    small, big = ar.linear_hmm(3, N, 1), ar.linear_hmm(5, N, 2)
    inv, uns = _lib.AMX_ERR_INVALID, _lib.AMX_ERR_UNSUPPORTED
    many = ar.graph(6, 0, {5: 0.0}, [(s, 5, 64 * s + i, i, 1.0) for s in range(5) for i in range(64)])
    return [([small, big], {}, [(0, 0, 2, 2)], inv, ("key 0", "begin time 2")),
            ([small, big], {}, [(0, 0, 0, 4), (1, 1, 3, 7)], inv, ("key 1", "[3, 7)", "segment 1 of 6 frames")),
            ([small, big], {}, [(0, 0, -1, 4)], inv, ("key 0", "[-1, 4)")),
            ([small, big], {}, [(2, 0, 0, 4)], inv, ("key 0", "graph 2")),
            ([small, big], {}, [(0, 0, 0, 4), (1, 2, 0, 4)], inv, ("key 1", "segment 2")),
            ([small, big], dict(arc_target=(1, 7)), [(0, 0, 0, 4)], inv, ("segment 0", "arc_target[1] = 7")),
            ([small, big], dict(arc_emission=(0, N)), [(0, 0, 0, 4)], inv, ("arc_emission[0] = %d" % N,)),
            ([small, ar.linear_hmm(257, N, 3)], {}, [(0, 0, 0, 4)], uns, ("graph 1", "257 states")),
            ([small, many], {}, [(0, 0, 0, 4)], uns, ("graph 1", "320 emission indices")),
            ([small, fan_in(256)], {}, [(0, 0, 0, 4)], uns, ("graph 1", "256 arcs into state 5")),
            ([small, ar.graph(2, 0, {1: 0.0}, [(0, 1, i % N, i, 1.0) for i in range(65)])], {}, [(0, 0, 0, 4)], uns, ("state 0 has 65 arcs",)),
            ([small, big], {}, [(1, 0, 0, 4)], _lib.AMX_ERR_STATE, ("without a context",))]


@pytest.mark.parametrize("case", range(len(refusals())))
def test_host_refusals_on_a_handle_without_context(case):
    graphs, patch, keys, status, words = refusals()[case]
    g = rasr_amd.LatticeArcAligner.graphs(graphs)
    n_columns = 400 if "emission indices" in words[-1] else N
    for k, (i, v) in patch.items():
        g[k][i] = v
    a = rasr_amd.LatticeArcAligner(None)
    with pytest.raises(rasr_amd.AmxError) as e:
        a.run(g, *np.array(keys, np.int32).T, [0, 9, 15], None, n_columns)
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    a.close()


def test_a_window_of_too_many_frames_and_the_configurations_align_create_refuses():
    a = rasr_amd.LatticeArcAligner(None)
    with pytest.raises(rasr_amd.AmxError) as e:
        a.run([ar.linear_hmm(3, N, 1)], [0], [0], [0], [_lib.AMX_ARCALIGN_MAX_FRAMES + 1], [0, 70000], None, N)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED and "65536 frames" in str(e.value)
    assert a.run([], [], [], [], [], [0], None, N)["counters"] == (0, 0, 0)
    for kw, status, word in ((dict(mode=_lib.AMX_ALIGN_BAUM_WELCH), _lib.AMX_ERR_UNSUPPORTED, "baum-welch"),
                             (dict(n_best_pruning=10), _lib.AMX_ERR_UNSUPPORTED, "n_best_pruning"),
                             (dict(min_acoustic_pruning=100.0, max_acoustic_pruning=50.0), _lib.AMX_ERR_INVALID, "min_acoustic_pruning")):
        with pytest.raises(rasr_amd.AmxError) as e:
            rasr_amd.LatticeArcAligner(None, **kw)
        assert e.value.status == status and word in str(e.value)


def test_expand_against_numpy():
    """3 keys (key 1 reached no final state), 2 segments, arcs with key -1, a key used twice"""
    seg, tbeg, tend = [0, 0, 1], [2, 0, 1], [5, 4, 3]
    slot_offsets = np.array([0, 3, 7, 9])
    slot_emission = np.array([10, 11, 12, -1, -1, -1, -1, 20, 21], np.int32)
    arc_offsets, arc_key = [0, 4, 6], [0, -1, 1, 0, 2, -1]
    want_frame, want_emission, want_off = [], [], [0]
    for k in arc_key:
        if k >= 0 and slot_emission[slot_offsets[k]] >= 0:
            want_frame += list(range(tbeg[k], tend[k]))
            want_emission += list(slot_emission[slot_offsets[k]:slot_offsets[k + 1]])
        want_off.append(len(want_frame))
    t = rasr_amd.LatticeArcAligner.expand(seg, tbeg, tend, slot_offsets, slot_emission, arc_offsets, arc_key)
    assert t["item_offsets"].tolist() == want_off == [0, 3, 3, 3, 6, 8, 8]
    assert t["item_frame"].tolist() == want_frame and t["item_emission"].tolist() == want_emission
    assert rasr_amd.LatticeArcAligner.expand(seg, tbeg, tend, slot_offsets, slot_emission, arc_offsets, arc_key, count_only=True) == 8
    for bad, word in (([0, -1, 1, 0, 2, 3], "key 3"), ([0, -1, 1, 2, 2, -1], "key 2 of segment 1")):
        with pytest.raises(rasr_amd.AmxError) as e:
            rasr_amd.LatticeArcAligner.expand(seg, tbeg, tend, slot_offsets, slot_emission, arc_offsets, bad)
        assert e.value.status == _lib.AMX_ERR_INVALID and word in str(e.value)


def test_symbols_and_kernel_shape():
    L = _lib.lib()
    for name in ("create", "destroy", "run_dev", "arc_scores_dev", "expand", "kernel_shape", "set_workspace_cap", "last_launches"):
        assert hasattr(L, "amx_arcalign_" + name)
    narrow, wide = rasr_amd.LatticeArcAligner.kernel_shape(False), rasr_amd.LatticeArcAligner.kernel_shape(True)
    assert (narrow["states_per_lane"], wide["states_per_lane"]) == (1, 4) and narrow["keys_per_workgroup"] == wide["keys_per_workgroup"] == 4
    assert 8 * wide["lds_bytes_per_wave"] <= 160 * 1024, "at least eight waves fit a CU's LDS"
