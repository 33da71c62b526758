"""GPU parity: amx_cart_accumulate_dev and amx_cart_train (cart.hip) against the restatement of tests/cart_reference.py, which
tests/test_cart.py holds to the reference's own results in both of its builds.

Accumulation: every f64 of the accumulator equals the restatement's bits, in one call and cut into three.
Training: with exact_all the library equals the restatement in every discrete result and every f64 bit (the sums come from the device in
the reference's order, the logarithm is this machine's libm on both sides); in default mode -- the device's gain as a screen, only the
contenders through the host -- tree, log, classes, statistics and error count are identical to exact_all: the check on the margin."""
import numpy as np
import pytest

from tests import cart_reference as cr

pytestmark = pytest.mark.gpu


@pytest.fixture()
def cctx(ctx):
    """the session context on torch's stream, handed out in contract=off and restored to it"""
    ctx.use_torch_stream()
    ctx.set_contract("off")
    yield ctx
    ctx.set_contract("off")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ accumulation

def frames(seed, T, dim, n_labels, weights):
    """features, labels and weights of T frames: label 3 holds 30 % of them, labels 1 and n_labels - 1 are absent, some frames carry -1,
    some weights are 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal((T, dim)) * 3 + 1).astype(np.float32)
    pool = np.array([l for l in range(n_labels) if l not in (1, 3, n_labels - 1)])
    lab = pool[rng.integers(0, len(pool), T)].astype(np.int32)
    lab[rng.random(T) < 0.3] = 3
    lab[rng.random(T) < 0.05] = -1
    w = None
    if weights:
        w = rng.uniform(0.01, 2.0, T)
        w[rng.random(T) < 0.05] = 0.0
    return x, lab, w


ACC_CASES = [(1, 1, False, "off"), (1, 255, True, "fma"), (13, 255, True, "off"), (13, 4097, False, "fma"), (40, 1, True, "fma"),
             (40, 4097, True, "off"), (40, 4097, True, "fma"), (65, 255, False, "off"), (65, 4097, True, "fma")]


@pytest.mark.parametrize("dim,T,weights,contract", ACC_CASES)
def test_accumulation_equals_the_restatement_in_one_call_and_in_three(cctx, dim, T, weights, contract):
    import torch

    import rasr_amd
    n_labels = 9
    x, lab, w = frames(100 + dim + T, T, dim, n_labels, weights)
    want = cr.accumulate(cr.accumulator(n_labels, dim), x, lab, w, contract=contract)
    if T == 4097:
        assert 0.25 * T < (lab == 3).sum() < 0.35 * T and want[1, 0] == 0 and want[n_labels - 1, 0] == 0
    cctx.set_contract(contract)
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    wd = torch.from_numpy(w).cuda() if w is not None else None
    one = rasr_amd.CartExampleAccumulator(cctx, n_labels, dim)
    one.accumulate(xd, ld, wd)
    got = one.rows()
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
    cuts = [0, T // 3, T // 3 + (T + 1) // 2 // 2, T]
    three = rasr_amd.CartExampleAccumulator(cctx, n_labels, dim)
    for a, b in zip(cuts, cuts[1:]):
        if b > a:
            three.accumulate(xd[a:b], ld[a:b], wd[a:b] if wd is not None else None)
    assert np.array_equal(bits(three.rows()), bits(want))
    ids, n_obs, values = one.examples()
    assert list(ids) == [i for i in range(n_labels) if want[i, 0] != 0] and np.array_equal(bits(values), bits(want[ids, 1:]))


def test_accumulation_reads_a_column_block_of_a_wider_matrix(cctx):
    import torch

    import rasr_amd
    x, lab, w = frames(7, 300, 20, 6, True)
    want = cr.accumulate(cr.accumulator(6, 13), x[:, 4:17], lab, w)
    acc = rasr_amd.CartExampleAccumulator(cctx, 6, 13)
    xd = torch.from_numpy(x).cuda()
    acc.accumulate(xd[:, 4:17], torch.from_numpy(lab).cuda(), torch.from_numpy(w).cuda())
    assert np.array_equal(bits(acc.rows()), bits(want))


@pytest.mark.parametrize("bad", [6, 7, -2, 2 ** 31 - 1])
def test_a_label_outside_the_table_is_refused_and_the_buffer_untouched(cctx, bad):
    import torch

    import rasr_amd
    x, lab, w = frames(8, 700, 5, 6, False)
    acc = rasr_amd.CartExampleAccumulator(cctx, 6, 5)
    acc.accumulate(torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda())
    before = acc.rows().copy()
    lab[611] = bad
    lab[650] = bad
    with pytest.raises(rasr_amd.AmxError, match="frame 611: label %d" % bad) as e:
        acc.accumulate(torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda())
    assert e.value.status == -1
    assert np.array_equal(bits(acc.rows()), bits(before))


# ------------------------------------------------------------------------------------------------------------------ training

def shape(dim):
    import rasr_amd
    return rasr_amd.DecisionTreeTrainer.kernel_shape(dim)


_RESTATED, _CASES = {}, {}


def all_cases():
    """the cases at the library's own launch shape, made once per session"""
    if not _CASES:
        _CASES.update(cr.cases(shape))
    return _CASES


def restated(name, contract):
    """the restatement's result of a case, computed once per session and never changed"""
    if (name, contract) not in _RESTATED:
        _RESTATED[name, contract] = cr.train(contract=contract, **all_cases()[name])
    return _RESTATED[name, contract]


def library(ctx, case, exact_all):
    import rasr_amd
    t = rasr_amd.DecisionTreeTrainer(ctx, max_leaves=case["max_leaves"], variance_clipping=case["variance_clipping"], exact_all=exact_all)
    return t.train(case["n_obs"], case["values"], case["answers"], case["steps"])


def as_result(out):
    """the library's structured arrays in the restatement's form"""
    nodes = [dict(step=int(n["step"]), row=int(n["row"]), left=int(n["left"]), right=int(n["right"]), depth=int(n["depth"]), n_obs=int(n["n_obs"]),
                  score=float(n["score"]), class_id=int(n["class_id"])) for n in out["nodes"]]
    log = [dict(node=int(l["node"]), step=int(l["step"]), row=int(l["row"]), depth=int(l["depth"]), gain=float(l["gain"]), total_gain=float(l["total_gain"]))
           for l in out["log"]]
    qs = [dict(step=int(q["step"]), row=int(q["row"]), count=int(q["count"]), min_gain=float(q["min_gain"]), sum_gain=float(q["sum_gain"]),
               max_gain=float(q["max_gain"]), min_depth=int(q["min_depth"]), sum_depth=int(q["sum_depth"]), max_depth=int(q["max_depth"])) for q in out["question_stats"]]
    return dict(nodes=nodes, classes=out["classes"], log=log, question_stats=qs, n_obs=int(out["n_obs"]), initial_score=float(out["initial_score"]),
                total_gain=float(out["total_gain"]), errors=int(out["negative_gain_errors"]))


def assert_same(got, want, what):
    g, w = cr.discrete(got), cr.discrete(want)
    for k in w:
        assert g[k] == w[k], (what, k)
    assert np.array_equal(bits(cr.floats(got)), bits(cr.floats(want))), (what, np.argwhere(bits(cr.floats(got)) != bits(cr.floats(want)))[:5])


CASE_NAMES = sorted(cr.cases())


def test_the_cases_sit_around_the_kernels_own_stage_and_tile():
    c = all_cases()
    for name, dim in (("stage_plus_1", 40), ("tile_plus_1_d32", 32)):
        stage, tile = shape(dim)
        assert stage >= 1 and tile >= 1
        assert len(c[name]["n_obs"]) == stage + 1 and len(c[name]["answers"]) == tile + 1 and c[name]["values"].shape[1] == 2 * dim
    stage, tile = shape(1)
    assert len(c["d1_tile_plus_1"]["n_obs"]) > stage and len(c["d1_tile_plus_1"]["answers"]) == tile + 1
    stage, tile = shape(40)
    assert len(c["big"]["n_obs"]) > 10 * stage and len(c["big"]["answers"]) > 20 * tile


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_training_equals_the_restatement_and_the_screen_changes_nothing(cctx, name, contract):
    case = all_cases()[name]
    want = restated(name, contract)
    cctx.set_contract(contract)
    exact = library(cctx, case, True)
    assert_same(as_result(exact), want, name + " exact_all")
    assert exact["n_leaves"] == want["n_leaves"] and exact["items_screened"] == 0 and exact["items_reevaluated"] > 0
    dflt = library(cctx, case, False)
    assert_same(as_result(dflt), as_result(exact), name + " default against exact_all")
    print("%s %s: %d launches, %d items screened, %d re-evaluated (exact_all: %d)" % (name, contract, dflt["launches"], dflt["items_screened"],
                                                                                      dflt["items_reevaluated"], exact["items_reevaluated"]))
    assert dflt["items_reevaluated"] <= dflt["items_screened"]


def test_the_screen_spares_most_questions_the_host(cctx):
    dflt = library(cctx, all_cases()["big"], False)
    assert dflt["items_reevaluated"] * 4 < dflt["items_screened"]


def test_training_refusals(cctx):
    import rasr_amd
    c = cr.cases()["e33_q1_d1"]
    t = rasr_amd.DecisionTreeTrainer(cctx)
    with pytest.raises(rasr_amd.AmxError, match="randomize 3") as e:
        t.train(c["n_obs"], c["values"], c["answers"], [dict(action="split", questions=[0], randomize=3)])
    assert e.value.status == -2
    with pytest.raises(rasr_amd.AmxError, match=r"questions\[0\] = 1 of 1 rows"):
        t.train(c["n_obs"], c["values"], c["answers"], [dict(action="split", questions=[1])])


# ------------------------------------------------------------------------------------------------------------------ end to end

def test_flat_start_labels_to_examples_to_a_tree(cctx):
    """amx_linseg_align_dev's labels -> accumulate -> train on 8 short segments, against the restatement fed the same labels"""
    import torch

    import rasr_amd
    rng = np.random.Generator(np.random.PCG64(31))
    dim, n_labels, silence = 6, 14, 0
    segs, feats = [], []
    for s in range(8):
        n = int(rng.integers(30, 70))
        n_states = int(rng.integers(3, 7))
        a = int(rng.integers(3, 8))
        e = (rng.standard_normal(n) * 0.3).astype(np.float32)
        e[a:n - a] += 6.0
        states = rng.integers(1, n_labels - 1, n_states).astype(np.int32)   # label 13 is never used
        x = (rng.standard_normal((n, dim)) + states[np.minimum(np.arange(n) * n_states // n, n_states - 1), None] * 0.7).astype(np.float32)
        x[:, 0] = e
        segs.append((e, states, states + 100))
        feats.append(x)
    x = np.concatenate(feats)
    off = np.cumsum([0] + [len(f) for f in feats])
    xd = torch.from_numpy(x).cuda()
    seg = rasr_amd.LinearSegmenter(cctx)
    models = rasr_amd.LinearSegmenter.models([(s[1], s[2]) for s in segs], silence, 100)
    lab, _, results, counters = seg.align(off, models, xd[:, 0], dim)
    assert counters[0] == 8, results
    acc = rasr_amd.CartExampleAccumulator(cctx, n_labels, dim)
    acc.accumulate(xd, lab)
    labels = lab.cpu().numpy()
    want_acc = cr.accumulate(cr.accumulator(n_labels, dim), x, labels)
    assert np.array_equal(bits(acc.rows()), bits(want_acc)) and want_acc[silence, 0] > 0 and want_acc[13, 0] == 0
    ids, n_obs, values = acc.examples()
    by_label = rng.random((9, n_labels)) < 0.5
    answers = by_label[:, ids]
    steps = [dict(action="split", questions=list(range(9)), min_obs=10)]
    got = rasr_amd.DecisionTreeTrainer(cctx, variance_clipping=1e-4).train(n_obs, values, answers, steps)
    want = cr.train(n_obs, values, answers, steps, variance_clipping=1e-4)
    assert len(want["log"]) >= 2
    assert_same(as_result(got), want, "end to end")
