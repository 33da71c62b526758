"""GPU: the device plan of the lattice arc posteriors (latplan.hip) against the host plan (latpost_host.cpp), integer for integer, and the
arc posteriors with plan="device" against plan="host", bit for bit: both run the same two kernels over the same chains.

The cases are the host plan's (latpost_reference.small_cases() and shape_cases()) and a few that stand where the plan kernel itself
switches (LatticePosterior.plan_shape()): a run of more than 64 black stack entries, a stack far deeper than the state count, more levels
than a workgroup has threads, and one lattice below and one above each of the two LDS limits."""
import functools

import numpy as np
import pytest

from tests import latpost_reference as lr

pytestmark = pytest.mark.gpu

ARRAYS = ("discover_index", "level_backward", "level_forward", "level_super", "in_offsets", "in_arc", "final_order")
COUNTS = ("reason", "states_reached", "arcs_reached", "states_coreached", "undefined_states", "undefined_arcs", "levels_forward", "levels_backward")


def parallel(n_arcs, tail=0):
    """`n_arcs` parallel arcs from the initial state to state 1, then a chain of `tail` arcs to the final state"""
    arcs = [(0, 1, 1.0 + 0.001 * (k % 97), 0.01 * (k % 7)) for k in range(n_arcs)] + [(1 + k, 2 + k, 0.5, 0.25) for k in range(tail)]
    return lr.lattice(2 + tail, arcs, 0, {1 + tail: 0.5}, {1 + tail: 0.25})


@functools.lru_cache(maxsize=None)
def cases():
    import rasr_amd
    shape = rasr_amd.LatticePosterior.plan_shape()
    c = dict(lr.small_cases())
    c.update(lr.shape_cases())
    c["parallel_200"] = parallel(200)
    c["complete_40"] = lr.lattice(40, [(i, j, 0.25 + 0.01 * (i + j), 0.1) for i in range(40) for j in range(i + 1, 40)], 0, {39: 0.0})
    c["chain_700"] = lr.lattice(700, [(i, i + 1, 0.5, 0.1) for i in range(699)], 0, {699: 0.25})
    c["states_below"], c["states_above"] = lr.fan(shape["lds_states"] - 2, 21), lr.fan(shape["lds_states"] - 1, 22)
    c["stack_below"], c["stack_above"] = parallel(shape["lds_stack"] - 2, 1), parallel(shape["lds_stack"] - 1, 1)
    return c


def batches():
    """every case alone, then all of them in one call, both ways"""
    names = tuple(cases())
    b = {n: (n,) for n in names}
    b["all"], b["all_reversed"] = names, names[::-1]
    return b


@functools.lru_cache(maxsize=None)
def host_plan(names):
    """the host plan of a batch, computed once and never changed"""
    import rasr_amd
    lp = rasr_amd.LatticePosterior(None, "expectation")
    plan = lp.plan([cases()[n] for n in names])
    lp.close()
    return plan


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_the_added_shapes_stand_where_the_plan_kernel_switches():
    import rasr_amd
    shape, c = rasr_amd.LatticePosterior.plan_shape(), cases()
    arcs = lambda name: len(c[name]["arc_target"])   # noqa: E731
    assert arcs("parallel_200") - 1 > 64                                    # black entries left on the stack when the first copy is done
    assert arcs("complete_40") + 1 > 10 * lr.n_states(c["complete_40"])     # the stack's bound against the state count
    assert host_plan(("chain_700",))["info"][0]["levels_backward"] > shape["threads"]
    assert lr.n_states(c["states_below"]) == shape["lds_states"] == lr.n_states(c["states_above"]) - 1
    assert arcs("stack_below") + 1 == shape["lds_stack"] == arcs("stack_above")
    assert max(arcs("states_below"), arcs("states_above")) + 1 <= shape["lds_stack"] and lr.n_states(c["stack_above"]) <= shape["lds_states"]


@pytest.mark.parametrize("batch", list(lr.small_cases()) + list(lr.shape_cases()) +
                         ["parallel_200", "complete_40", "chain_700", "states_below", "states_above", "stack_below", "stack_above", "all", "all_reversed"])
def test_the_device_plan_equals_the_host_plan(ctx, batch):
    import rasr_amd
    names = batches()[batch]
    want = host_plan(names)
    lp = rasr_amd.LatticePosterior(ctx, "expectation")
    got = lp.plan_dev([cases()[n] for n in names])
    lp.close()
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), (batch, k, np.flatnonzero(got[k] != want[k])[:8])
    for g, name in enumerate(names):
        for k in COUNTS:
            assert got["info"][g][k] == want["info"][g][k], (batch, name, k)


@pytest.mark.parametrize("mode,contract", [("log", "off"), ("prob", "off"), ("expectation", "off"), ("expectation", "fma")])
def test_the_posteriors_are_the_host_plans_in_every_bit(ctx, mode, contract):
    import rasr_amd
    ctx.use_torch_stream()
    ctx.set_contract(contract)
    lats = [cases()[n] for n in cases()]
    n_states = sum(lr.n_states(lat) for lat in lats)
    out = {}
    try:
        for plan in ("host", "device"):
            lp = rasr_amd.LatticePosterior(ctx, mode, plan=plan)
            arc, final, info = lp.run(lats)
            out[plan] = dict(arc=arc.cpu().numpy(), final=final.cpu().numpy(), **lp.last_potentials(n_states),
                             **{k: np.array([i[k] for i in info], np.float64) for k in lp.INFO})
            lp.close()
    finally:
        ctx.set_contract("off")
    assert set(out["device"]) == set(out["host"])
    for k in out["host"]:
        assert np.array_equal(bits(out["device"][k]), bits(out["host"][k])), (mode, contract, k)


@pytest.mark.parametrize("what", ["cycle", "target", "nan_weight"])
def test_a_refusal_is_the_host_plans_and_leaves_the_outputs(ctx, what):
    import torch

    import rasr_amd
    ctx.use_torch_stream()
    good = lr.small_cases()["diamond"]
    bad = {"cycle": lr.lattice(4, [(0, 1, 1.0, 0.0), (1, 2, 1.0, 0.0), (2, 1, 1.0, 0.0), (2, 3, 1.0, 0.0)], 0, {3: 0.0}),
           "target": dict(good, arc_target=np.array([1, 4, 3, 3], np.int32)),
           "nan_weight": dict(good, arc_weight=np.array([1.0, 1.25, np.nan, 1.5], np.float32))}[what]
    raised = {}
    for plan in ("host", "device"):
        lp = rasr_amd.LatticePosterior(ctx, "log", plan=plan)
        t = lp.tables([good, bad, good])
        arc_out = torch.full((len(t["arc_target"]),), 7.0, dtype=torch.float32, device="cuda")
        final_out = torch.full((int(t["state_offsets"][-1]),), 9.0, dtype=torch.float32, device="cuda")
        with pytest.raises(rasr_amd.AmxError) as e:
            lp.run_dev(t, arc_out, final_out)
        raised[plan] = (e.value.status, str(e.value))
        assert bool((arc_out == 7.0).all()) and bool((final_out == 9.0).all()), plan
        lp.close()
    assert raised["device"] == raised["host"] and raised["host"][0] == rasr_amd._lib.AMX_ERR_INVALID and "segment 1" in raised["host"][1]
