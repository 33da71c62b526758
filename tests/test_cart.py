"""CPU: decision-tree state tying.  The restatement of tests/cart_reference.py against the reference's own results (tests/golden/ref_cart.npz,
written by tests/golden/make_cart_golden.py from the reference's text in both of its builds); the planted defects; the host refusals of
amx_cart_train; and the host's tree once more from a stand-alone program built with the host sanitizers.  No kernel runs here.

The fixture's generator asserted, where the reference is mounted, that the restatement equals the reference in every bit.  Here the
logarithm is this machine's libm, which may differ from the generator's in the last bit: every discrete result must be equal on the cases
the generator marked decided, and every f64 within the bar made from glibc's documented 1-ulp bound on log over the node's chain
(cart_reference.score_bar).  The tie_* cases hold equal gains on purpose; one last bit may turn them, so they are held to the fixture only
where this machine's scores are the fixture's bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cart_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cr.cases()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "ref_cart.npz")) as z:
        return {k: z[k] for k in z.files}


def recorded(golden, contract, name):
    """a case's result in the fixture, in the restatement's form: the native build's where it differs, else the plain build's"""
    k = "fma/%s/" % name if contract == "fma" and "fma/%s/node_i" % name in golden else "off/%s/" % name
    g = lambda f: golden[k + f]
    nodes = [dict(step=int(r[0]), row=int(r[1]), left=int(r[2]), right=int(r[3]), depth=int(r[4]), n_obs=int(r[5]), class_id=int(r[6]), score=float(s))
             for r, s in zip(g("node_i"), g("node_score"))]
    log = [dict(node=int(r[0]), step=int(r[1]), row=int(r[2]), depth=int(r[3]), gain=float(f[0]), total_gain=float(f[1])) for r, f in zip(g("log_i"), g("log_f"))]
    qs = [dict(step=int(r[0]), row=int(r[1]), count=int(r[2]), min_depth=int(r[3]), sum_depth=int(r[4]), max_depth=int(r[5]), min_gain=float(f[0]),
               sum_gain=float(f[1]), max_gain=float(f[2])) for r, f in zip(g("qs_i"), g("qs_f"))]
    si, sf = g("scalars_i"), g("scalars_f")
    return dict(nodes=nodes, classes=g("classes"), log=log, question_stats=qs, n_obs=int(si[0]), errors=int(si[1]), n_leaves=int(si[2]),
                initial_score=float(sf[0]), total_gain=float(sf[1]))


_RESTATED = {}


def restated(name, contract):
    if (name, contract) not in _RESTATED:
        _RESTATED[name, contract] = cr.train(contract=contract, **CASES[name])
    return _RESTATED[name, contract]


def test_fixture_holds_the_cases_and_what_the_generator_found(golden):
    assert list(golden["cases"]) == list(CASES) and len(CASES) >= 15
    for name, c in CASES.items():
        k = "in/%s/" % name
        assert golden[k + "n_obs"].tobytes() == c["n_obs"].tobytes() and golden[k + "values"].tobytes() == c["values"].tobytes(), name
        E = len(c["n_obs"])
        bits = np.unpackbits(golden[k + "answers"].view(np.uint8), axis=1, bitorder="little")[:, :E].astype(bool)
        assert np.array_equal(bits, c["answers"]), name
        assert list(golden[k + "plan"]) == [c["max_leaves"], c["variance_clipping"]]
        assert [int(v) for v in golden[k + "step_q"]] == [q for s in c["steps"] for q in s["questions"]]
        assert [list(r) for r in golden[k + "step_i"]] == [[cr.ACTIONS[s["action"]], s.get("min_obs", 0), len(s["questions"])] for s in c["steps"]]
    # the sites the -march=native build fuses are the restatement's, and that build does compute other bits
    assert list(golden["fma_sites"]) == ["variance=1,constant=1", "sum=1,sum_sq=1"]
    assert int(golden["fma_instructions/off"]) == 0 and int(golden["fma_instructions/fma"]) > 0
    assert {"three_actions", "weights", "acc_weights"} <= set(golden["fma_differs"])
    for name in CASES:
        assert bool(golden["decided/" + name].all()) == (not cr.is_tie(name)), name
        assert cr.is_tie(name) or golden["decided_gap/" + name].min() > 1e3, name     # no comparison of a decided case comes near its bar


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_the_reference(golden, name, contract):
    r, g = restated(name, contract), recorded(golden, contract, name)
    same_bits = cr.floats(r).tobytes() == cr.floats(g).tobytes()
    if cr.is_tie(name) and not same_bits:   # this machine's logarithm differs from the generator's in a last bit, which may turn a tie
        assert r["n_leaves"] == len(r["log"]) + 1 and r["n_obs"] == g["n_obs"] and abs(r["initial_score"] - g["initial_score"]) <= golden[
            "score_bar/%s/%s" % (contract, name)][0]
        return
    assert cr.discrete(r) == cr.discrete(g) and r["n_leaves"] == g["n_leaves"]
    # scores within the node's bar, gains within the bars of the three scores they are made of
    bar = golden["score_bar/%s/%s" % (contract, name)]
    assert len(bar) == len(g["nodes"])
    run = 0.0
    for a, b, w in zip(r["nodes"], g["nodes"], bar):
        assert a["score"] == b["score"] or abs(a["score"] - b["score"]) <= w, (name, a, b, w)
    for a, b in zip(r["log"], g["log"]):
        n = g["nodes"][b["node"]]
        w = bar[b["node"]] + bar[n["left"]] + bar[n["right"]]
        run += w + cr.EPS * abs(b["total_gain"])
        assert abs(a["gain"] - b["gain"]) <= w and abs(a["total_gain"] - b["total_gain"]) <= run, (name, a, b, w)
    for a, b in zip(r["question_stats"], g["question_stats"]):
        for f in ("min_gain", "sum_gain", "max_gain"):
            assert abs(a[f] - b[f]) <= run, (name, a, b)
    assert abs(r["initial_score"] - g["initial_score"]) <= bar[0] and abs(r["total_gain"] - g["total_gain"]) <= run + cr.EPS


def test_accumulation_restated_against_the_reference(golden):
    assert len(golden["acc_cases"]) >= 3
    for name in golden["acc_cases"]:
        k = "in/%s/" % name
        x, lab, n_labels = golden[k + "feats"], golden[k + "labels"], int(golden[k + "n_labels"])
        w = golden[k + "weights"] if k + "weights" in golden else None
        for contract in ("off", "fma"):
            want = golden["fma/%s/acc" % name] if contract == "fma" and "fma/%s/acc" % name in golden else golden["off/%s/acc" % name]
            got = cr.accumulate(cr.accumulator(n_labels, x.shape[1]), x, lab, w, contract=contract)
            assert got.tobytes() == want.tobytes(), (name, contract)
        # cut into calls anywhere: the chains continue
        acc = cr.accumulator(n_labels, x.shape[1])
        for a, b in ((0, 11), (11, 12), (12, len(lab))):
            cr.accumulate(acc, x[a:b], lab[a:b], None if w is None else w[a:b])
        assert acc.tobytes() == golden["off/%s/acc" % name].tobytes()


@pytest.mark.parametrize("defect", sorted(cr.PLANTED))
def test_every_planted_defect_leaves_its_case(golden, defect):
    name = cr.PLANTED[defect]
    g, r = recorded(golden, "off", name), cr.train(defect=defect, **CASES[name])
    assert cr.discrete(r) != cr.discrete(g) or cr.floats(r).tobytes() != cr.floats(g).tobytes(), (defect, name)
    assert set(cr.PLANTED) == set(cr.DEFECTS)


def test_the_cases_are_what_their_names_say():
    free = lambda c: dict(c, steps=[dict(action=s["action"], questions=s["questions"]) for s in c["steps"]])
    # min_obs: the unconstrained winner of the root has a side below the bound, and another question takes the root
    c = CASES["min_obs_excludes_best"]
    a, b = restated("min_obs_excludes_best", "off"), cr.train(**free(c))
    best = b["nodes"][0]
    assert min(b["nodes"][best["left"]]["n_obs"], b["nodes"][best["right"]]["n_obs"]) < c["steps"][0]["min_obs"]
    assert a["nodes"][0]["row"] not in (-1, best["row"])
    # min_gain: the root splits, its children would -- their best gains lie below the bound
    c = CASES["min_gain_excludes_best"]
    a, b = restated("min_gain_excludes_best", "off"), cr.train(**free(c))
    assert len(a["log"]) == 1 and len(b["log"]) > 1 and a["log"][0]["gain"] == b["log"][0]["gain"] >= c["steps"][0]["min_gain"]
    below = [l["gain"] for l in b["log"] if l["node"] in (1, 2)]
    assert below and 0 < max(below) < c["steps"][0]["min_gain"]
    # max_leaves is reached in the middle of a step: splits are left in the queue and rolled back
    for name in ("max_leaves_mid_step", "rollback", "tie_twins"):
        a, b = restated(name, "off"), cr.train(**dict(CASES[name], max_leaves=0xffffffff))
        assert a["n_leaves"] == CASES[name]["max_leaves"] < b["n_leaves"], name
    # a step that ends at the leaf limit rolls its queued splits back, and by the same count (nLeaf + nodes + splits >= maxLeaves becomes
    # nLeaf + nodes >= maxLeaves) no later step runs (Cart/DecisionTreeTrainer.cc:635, :681, :694-698): the statistics hold the first step's
    # questions alone
    assert len(CASES["rollback"]["steps"]) == 2 and {q["step"] for q in restated("rollback", "off")["question_stats"]} == {0}
    # all three actions commit splits
    a = restated("three_actions", "off")
    assert {l["step"] for l in a["log"]} == {0, 1, 2}
    # the all-left question never splits, the clipping is active, the weights are fractional, twins wait with equal gains
    c = CASES["all_left"]
    assert c["answers"][3].all() and all(n["row"] != 3 for n in restated("all_left", "off")["nodes"])
    assert cr.floats(restated("clipping", "off")).tobytes() != cr.floats(cr.train(**dict(CASES["clipping"], variance_clipping=0.0))).tobytes()
    assert restated("clipping", "off")["errors"] > 0
    assert not np.all(CASES["weights"]["n_obs"] == np.floor(CASES["weights"]["n_obs"]))
    gains = [l["gain"] for l in restated("tie_twins", "off")["log"]]
    assert len(set(gains)) < len(gains)


def host_train(n_obs, values, answers, steps, **kw):
    import rasr_amd
    try:
        rasr_amd.DecisionTreeTrainer(None, **kw).train(n_obs, values, answers, steps)
    except rasr_amd.AmxError as e:
        return e.status, str(e)
    return 0, ""


def test_host_refusals_name_their_field():
    from rasr_amd import _lib
    c = CASES["e33_q1_d1"]
    n, v, a = c["n_obs"], c["values"], c["answers"]
    ok = [dict(action="split", questions=[0])]
    st, msg = host_train(n, v, a, ok)
    assert st == _lib.AMX_ERR_STATE and "no context" in msg                           # a valid problem reaches the context check
    for steps, status, words in (
            ([dict(action="split", questions=[0], randomize=2)], _lib.AMX_ERR_UNSUPPORTED, ("step 0: randomize 2", "time of day")),
            ([dict(action="split", questions=[0], randomize=0)], _lib.AMX_ERR_INVALID, ("randomize 0",)),
            ([dict(action=7, questions=[0])], _lib.AMX_ERR_INVALID, ("step 0: unknown action 7",)),
            (ok + [dict(action="cluster", questions=[0, 1])], _lib.AMX_ERR_INVALID, ("step 1: questions[1] = 1 of 1 rows",)),
            ([dict(action="split", questions=[-1])], _lib.AMX_ERR_INVALID, ("questions[0] = -1",)),
            ([dict(action="split", questions=[0], min_gain=float("nan"))], _lib.AMX_ERR_INVALID, ("min_gain is not a number",))):
        st, msg = host_train(n, v, a, steps)
        assert st == status, (steps, msg)
        for w in words:
            assert w in msg, msg
    big = n.copy()
    big[:] = 2.0 ** 31
    st, msg = host_train(big, v, a, ok)
    assert st == _lib.AMX_ERR_UNSUPPORTED and "32 bits" in msg
    bad = n.copy()
    bad[7] = np.nan
    st, msg = host_train(bad, v, a, ok)
    assert st == _lib.AMX_ERR_INVALID and "n_obs[7]" in msg
    st, msg = host_train(n, v, a, ok, variance_clipping=float("nan"))
    assert st == _lib.AMX_ERR_INVALID and "variance_clipping" in msg
    wide = np.zeros((2, 2 * 1025))
    st, msg = host_train(np.ones(2), wide, np.zeros((1, 2), bool), ok)
    assert st == _lib.AMX_ERR_UNSUPPORTED and "dim 1025" in msg


def test_the_python_classes_and_the_new_names():
    import rasr_amd
    from rasr_amd import _lib
    for n in ("amx_cart_accumulator_size", "amx_cart_accumulate_dev", "amx_cart_train", "amx_cart_tree_destroy", "amx_cart_tree_info", "amx_cart_tree_get",
              "amx_cart_kernel_shape"):
        assert n in _lib.SIGNATURES
    L = _lib.lib()
    assert L.amx_cart_accumulator_size(10000, 40) == 810000 and L.amx_cart_accumulator_size(5, 0) == 0
    assert L.amx_cart_accumulate_dev(None, None, 4, 4, 1, None, None, 3, None) == _lib.AMX_ERR_INVALID and b"NULL context" in L.amx_last_error()
    for dim in (1, 32, 40):
        assert rasr_amd.DecisionTreeTrainer.kernel_shape(dim) == cr.kernel_shape(dim)
    a = np.random.Generator(np.random.PCG64(1)).random((5, 70)) < 0.5
    p = rasr_amd.DecisionTreeTrainer.pack_answers(a)
    assert p.shape == (5, 3) and p.dtype == np.uint32
    assert all(bool((p[q, e >> 5] >> (e & 31)) & 1) == bool(a[q, e]) for q in range(5) for e in range(70))
    t = rasr_amd.DecisionTreeTrainer(None)
    with pytest.raises(ValueError):
        t.train(np.ones(3), np.ones((3, 3)), np.zeros((1, 3), bool), [])
    with pytest.raises(ValueError):
        t.train(np.ones(3), np.ones((3, 4)), np.zeros((1, 2), np.uint32), [])
    with pytest.raises(TypeError):
        t.train(np.ones(3), np.ones((3, 4)), np.zeros((1, 3), bool), [dict(action="split", questions=[0], min_observations=3)])
    with pytest.raises(ValueError):
        t.train(np.ones(3), np.ones((3, 4)), np.zeros((1, 3), bool), [dict(action="prune", questions=[0])])
    for s in (_lib.CartNode, _lib.CartCommit, _lib.CartQstat, _lib.CartInfo):     # the structured arrays the getters fill have the structs' layout
        assert np.dtype(s).itemsize == C.sizeof(s)


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_cart_test.cc compiles cart.hip's host side into a program of its own: every refusal, and whole trainings of the host's tree
    with the two device seams replaced by plain loops; built with -fsanitize=address,undefined on the host side only, run as a process of
    its own (nothing sanitized is loaded into Python).  Sanitizers are for machines without a GPU: where one is present the same program
    is built and run plainly."""
    import torch
    exe = str(tmp_path / "host_cart_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_cart_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_cart_test: ok" in r.stdout, r.stdout + r.stderr
