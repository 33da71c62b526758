"""GPU: rasr_amd.LatticeBest (latbest.hip) against the restatement of tests/latbest_reference.py.  Every output is compared for equality:
keep, best_arc, path, kept_index and the integer fields of info exactly; the potentials, best scores and min_weight as f32 with `==`.
The cases are latbest_reference.CASES (fans of 1 ... 300 arcs, the constructed ties, the keep boundary, the dead arc, no final state,
unreached states, a random lattice of 600 states, a lattice one state below and one above the LDS limit), each under four settings."""
import numpy as np
import pytest

from tests import latbest_reference as lr

pytestmark = pytest.mark.gpu

MODES = {"off": (False, True, False), "relative": (True, True, False), "absolute": (True, False, False), "absolute_trim": (True, False, True)}
INTS = ("reason", "path_length", "kept_arcs", "total_arcs", "states_reached", "states_coreached")
FLOATS = ("best_score", "min_weight", "min_weight_threshold")
LDS = [n for n in lr.CASES if n.startswith("lds")]   # one state below and one above the LDS limit
SMALL = [n for n in lr.CASES if n != "random600" and n not in LDS]


def want(name, mode):
    prune, relative, trim = MODES[mode]
    return lr.best(name, lr.CASES[name][1] if prune else None, relative, trim)


def run(ctx, names, mode, potentials="auto", threshold=None):
    """one call over the named cases -> per case what lr.best returns (arc numbers within the lattice)"""
    import rasr_amd
    ctx.use_torch_stream()
    prune, relative, trim = MODES[mode]
    lb = rasr_amd.LatticeBest(ctx, (lr.CASES[names[0]][1] if threshold is None else threshold) if prune else None, relative, trim, potentials)
    r = lb.run([lr.CASES[n][0] for n in names])
    pots = lb.last_potentials(int(r["tables"]["state_offsets"][-1]))
    lb.close()
    host = {k: r[k].cpu().numpy() for k in ("best_arc", "path", "keep", "kept_index")}
    out, a0, s0 = [], 0, 0
    for name, info in zip(names, r["info"]):
        lat = lr.CASES[name][0]
        n, na = lr.n_states(lat), len(lat["arc_target"])
        local = lambda v: np.where(v >= 0, v - a0, -1).astype(np.int32)   # noqa: E731
        out.append(dict(forward=pots["forward"][s0:s0 + n], backward=pots["backward"][s0:s0 + n], best_arc=local(host["best_arc"][s0:s0 + n]),
                        path=local(host["path"][s0:s0 + n]), keep=host["keep"][a0:a0 + na], kept_index=host["kept_index"][a0:a0 + na], info=info))
        a0, s0 = a0 + na, s0 + n
    return out


def same(got, ref, what):
    for k in ("best_arc", "path", "keep", "kept_index"):
        assert np.array_equal(got[k], ref[k]), (what, k, np.flatnonzero(got[k] != ref[k])[:8])
    for k in ("forward", "backward"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], ref[k]), (what, k, np.flatnonzero(got[k] != ref[k])[:8])
    for k in INTS:
        assert got["info"][k] == ref["info"][k], (what, k, got["info"][k], ref["info"][k])
    for k in FLOATS:
        assert np.float32(got["info"][k]) == ref["info"][k], (what, k, got["info"][k], ref["info"][k])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(lr.CASES))
def test_every_output_equals_the_restatement(ctx, name, mode):
    same(run(ctx, [name], mode)[0], want(name, mode), (name, mode))


@pytest.mark.parametrize("name", ["random600", "fan300", "par129"] + LDS)
def test_global_potentials_give_the_same_bits(ctx, name):
    same(run(ctx, [name], "absolute_trim", "global")[0], want(name, "absolute_trim"), name)


@pytest.mark.parametrize("mode", ["relative", "absolute_trim"])
def test_one_call_equals_single_segments_equals_another_batching(ctx, mode):
    names = SMALL + ["random600"]
    refs = [lr.best(n, 0.5 if MODES[mode][0] else None, MODES[mode][1], MODES[mode][2]) for n in names]
    whole = run(ctx, names, mode, threshold=0.5)
    half = len(names) // 3
    parts = run(ctx, names[:half], mode, threshold=0.5) + run(ctx, names[half:], mode, threshold=0.5)
    for i, n in enumerate(names):
        same(whole[i], refs[i], (n, "whole"))
        same(parts[i], refs[i], (n, "parts"))
        if i % 7 == 0:
            same(run(ctx, [n], mode, threshold=0.5)[0], refs[i], (n, "alone"))


def test_a_refused_input_leaves_the_outputs_untouched(ctx):
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    good = lr.CASES["tie2_1_0"][0]
    cycle = lr.lattice([(0, 1, 1.0), (1, 2, 1.0), (2, 1, 1.0), (2, 3, 1.0)], 4, {3: 0.0})
    nan = dict(good, arc_weight=np.array([1.0, np.nan, 0.0, 0.0], np.float32))
    lb = rasr_amd.LatticeBest(ctx, 0.5)
    dev = torch.device("cuda", ctx.device)
    for bad in (cycle, nan):
        t = lb.tables([good, bad])
        bufs = [torch.full((8,), 77, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.uint8, torch.int32)]
        with pytest.raises(rasr_amd.AmxError, match="segment 1"):
            lb.run_dev(t, *bufs)
        torch.cuda.synchronize()
        assert all(bool((b == 77).all()) for b in bufs)
    lb.close()


def test_prune_compact_and_posteriors_end_to_end(ctx):
    """prune on the device, amx_latbest_compact, amx_latpost_run_dev on the result == amx_latpost_run_dev on the lattice the restatement pruned"""
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    name = "random600"
    lat, thr = lr.CASES[name]
    lb = rasr_amd.LatticeBest(ctx, thr, True, True)
    r = lb.run([lat])
    lb.close()
    ref = lr.best(name, thr, True, True)
    assert 0 < ref["info"]["kept_arcs"] < ref["info"]["total_arcs"]
    tables, old_to_new = rasr_amd.LatticeBest.compact(r["tables"], r["keep"].cpu().numpy())
    assert np.array_equal(old_to_new, r["kept_index"].cpu().numpy())
    sel = ref["keep"] != 0
    src = np.repeat(np.arange(lr.n_states(lat)), np.diff(lat["arc_offsets"]))
    pruned = dict(lat, arc_offsets=np.concatenate([[0], np.cumsum(np.bincount(src[sel], minlength=lr.n_states(lat)))]), arc_target=lat["arc_target"][sel],
                  arc_weight=lat["arc_weight"][sel])
    lp = rasr_amd.LatticePosterior(ctx, "log")
    bufs = [torch.empty(n, dtype=torch.float32, device=r["keep"].device) for n in (len(tables["arc_target"]), lr.n_states(lat))]
    got = lp.run_dev(tables, *bufs)
    arc, final, info = lp.run([pruned])
    lp.close()
    n_kept = ref["info"]["kept_arcs"]
    assert np.array_equal(bufs[0][:n_kept].cpu().numpy().view(np.uint32), arc.cpu().numpy().view(np.uint32))
    assert np.array_equal(bufs[1].cpu().numpy().view(np.uint32), final.cpu().numpy().view(np.uint32))
    assert got[0]["total_inv"] == info[0]["total_inv"] and got[0]["reason"] == info[0]["reason"] == 0

