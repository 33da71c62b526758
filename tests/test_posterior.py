"""CPU: state posteriors and model combination.  The restatement of tests/posterior_reference.py against the reference's own results
(tests/golden/ref_posterior.npz, written by tests/golden/make_posterior_golden.py from the reference's text in both of its builds), and
the host logic of the amx_posterior and amx_combine handles.  No kernel runs here.

Bars: s (the stored scores), the minimum, the survivor sets, the sparse index lists and the combined scores equal in bits in both
contract modes; f64 posteriors and logZ within 1e-11 relative; f32 posteriors equal in bits wherever the recorded distance to an f32
midpoint exceeds 1e-11, within one ulp elsewhere.  The 1e-11 is derived: reordering an f64 sum of n <= 16384 non-negative terms moves it
by at most (n - 1) * 2^-53 = 1.8e-12 relative, log1p has condition <= 1, so the argument p - logZ of the last exp moves by < 2e-12
absolute and the posterior by as much relative, plus a few f64 ulp of exp and log1p themselves."""
import ctypes as C
import os

import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import posterior_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_posterior.npz")
DBL_MAX = pr.DBL_MAX
REL = 1e-11


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def close(a, b, rel=REL):
    """|a - b| <= rel * |b|, and exactly 0 where b is 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rel * np.abs(b)))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_names(golden):
    return sorted(k[4:] for k in golden if k.startswith("cfg/"))


def recorded(golden, contract, key):
    return golden["fma/" + key] if contract == "fma" and "fma/" + key in golden else golden["off/" + key]


def case_inputs(golden, name):
    x = {k: golden["in/d/%s/%s" % (name, k)] for k in ("scores", "best", "topo_off", "topo", "filter_mixture", "filter_prior", "disregard", "margin_mixture")}
    n, scale, thr, margin = golden["cfg/" + name]
    n = int(n)
    prior = np.zeros(n)
    in_filter = np.zeros(n, bool)
    prior[x["filter_mixture"]] = x["filter_prior"]
    in_filter[x["filter_mixture"]] = True
    for d in x["disregard"]:   # erased as mixture indices (hh:148-154); a number that names no mixture does nothing
        if 0 <= d < n:
            in_filter[d] = False
    return x, n, float(scale), float(thr), float(margin), prior, in_filter


def test_fixture_holds_what_the_generator_says(golden):
    names = case_names(golden)
    assert len(names) == 24 + 8 + 2 and {int(golden["cfg/" + k][0]) for k in names} == {3, 13, 200}
    assert {float(golden["cfg/" + k][1]) for k in names} == {1.0, 0.37}
    assert {float(golden["cfg/" + k][2]) for k in names} == {DBL_MAX, 30.0, 1e-3}
    assert {float(golden["cfg/" + k][3]) for k in names} == {0.0, 2.5}
    assert any(len(golden["in/d/%s/disregard" % k]) for k in names)
    assert int(golden["fma_instructions/off"]) == 0 and int(golden["fma_instructions/fma"]) > 0
    differs = [str(k) for k in golden["fma_differs"]]
    # the -march=native build contracts prior + scale * score: it differs exactly where scale != 1 and priors are not 0; never in b/
    assert differs and not [k for k in differs if k.startswith("b/")]
    for k in differs:
        if k.startswith("d/"):
            name = k.split("/")[1]
            assert float(golden["cfg/" + name][1]) == 0.37 and np.any(golden["in/d/%s/filter_prior" % name] != 0), k
    assert bool(golden["off/mixture_mode_degenerate"])
    assert float(golden["order_worst_logz_distance"]) <= REL and float(golden["midpoint_share"]) <= 0.01


@pytest.mark.parametrize("contract", ("off", "fma"))
def test_restatement_equals_the_reference_posteriors(golden, contract):
    frames = exempt = total = 0
    for name in case_names(golden):
        x, n, scale, thr, margin, prior, in_filter = case_inputs(golden, name)
        g = {f: recorded(golden, contract, "d/%s/%s" % (name, f)) for f in ("stored", "post", "min", "min_key", "logz", "n_active", "sparse_index",
                                                                          "sparse_value")}
        mid = recorded(golden, contract, "d/%s/midpoint" % name) if contract == "off" or "fma/d/%s/midpoint" % name in golden else golden["off/d/%s/midpoint" % name]
        keys = pr.density_keys(x["topo_off"], x["topo"], x["best"])
        r = pr.posteriors(x["scores"], scale, prior, in_filter, thr, margin, x["margin_mixture"], contract_fma=contract == "fma")
        surv = ~np.isnan(g["post"])
        assert np.array_equal(r["survivors"], surv), name
        assert same(r["stored"][surv], g["stored"][surv]), name
        assert same(r["min"], g["min"]), name
        assert np.array_equal(keys[np.arange(len(keys)), r["min_index"]], g["min_key"]), name
        assert np.array_equal(r["n_survivors"], g["n_active"]), name
        assert close(r["log_z"], g["logz"]), name
        assert close(r["post"][surv], g["post"][surv]), name
        assert not np.any(r["post"][~surv]), name
        far = mid[surv] > REL
        d = pr.ulp_distance32(r["post32"][surv], g["post"][surv].astype(np.float32))
        assert not np.any(d[far]) and np.all(d <= 1), name
        exempt += int(np.sum(~far))
        total += int(np.sum(surv))
        rows = pr.sparse_rows(r, keys)
        for t, (idx, val) in enumerate(rows):
            order = np.argsort(idx, kind="stable")   # the node sorts by key (StatePosteriorFeatureScorerNode.cc:49-57)
            k = len(idx)
            assert same(idx[order], g["sparse_index"][t, :k]) and np.all(g["sparse_index"][t, k:] == -1), (name, t)
            assert np.all(pr.ulp_distance32(val[order], g["sparse_value"][t, :k]) <= (~(mid[t][surv[t]][order] > REL)).astype(np.int64)), (name, t)
        frames += len(rows)
    assert frames == 34 * 43 and exempt <= 0.01 * total


@pytest.mark.parametrize("contract", ("off", "fma"))
def test_restatement_equals_the_reference_likelihoods(golden, contract):
    """likelihoodAndMixtures() without a threshold, from the reference's mixture path itself"""
    seen = 0
    for name in case_names(golden):
        if "off/l/%s/likelihood" % name not in golden:
            continue
        x, n, scale, thr, margin, prior, in_filter = case_inputs(golden, name)
        g = recorded(golden, contract, "l/%s/likelihood" % name)
        r = pr.posteriors(x["scores"], scale, prior, in_filter, DBL_MAX, likelihood=True, contract_fma=contract == "fma")
        assert np.array_equal(r["survivors"], ~np.isnan(g)), name
        assert close(r["post"][r["survivors"]], g[r["survivors"]], 1e-15 * 4), name   # a few ulp of exp
        seen += 1
    assert seen >= 4


@pytest.mark.parametrize("contract", ("off", "fma"))
def test_restatement_equals_the_reference_candidate_lists(golden, contract):
    for n in (3, 13, 200):
        s, off, mix, pri = (golden["in/c/%d/%s" % (n, f)] for f in ("scores", "offsets", "mixture", "prior"))
        assert set(np.diff(off).tolist()) == {0, 1, 2, n, n + 7}
        for scale in (1.0, 0.37):
            g = recorded(golden, contract, "c/%d/%g/post" % (n, scale))
            r = pr.list_posteriors(s, scale, off, mix, pri, contract_fma=contract == "fma")
            assert close(r, g), (n, scale)
            assert same(r == 0, g == 0), (n, scale)   # exp underflows to 0 in the same places


def test_restatement_equals_the_reference_combination(golden):
    names = sorted({k.split("/")[2] for k in golden if k.startswith("in/b/")})
    assert len(names) == 5
    widths = set()
    for name in names:
        table, scales = golden["in/b/%s/table" % name], golden["in/b/%s/scales" % name]
        mats = [golden["in/b/%s/scores%d" % (name, i)] for i in range(table.shape[1])]
        assert same(pr.combine(table, scales, mats), golden["off/b/%s/out" % name]), name
        assert "fma/b/%s/out" % name not in golden
        widths.add(table.shape[1])
    assert widths == {1, 2, 3}


def test_fma_restatement_is_a_fused_multiply_add():
    a, b, c = np.float64(0.37), np.float64(np.float32(51.234567)), np.float64(3.3)
    exact = pr.fma(a, b, c)
    assert exact == pr.fma(b, a, c) and abs(exact - (a * b + c)) <= np.spacing(exact)
    assert pr.fma(1.0, b, c) == b + c and pr.fma(a, b, 0.0) == a * b
    assert pr.fma(2.0 ** -30 + 1, 2.0 ** -30 + 1, -1.0) == 2.0 ** -29 + 2.0 ** -60   # the plain form loses the last term


# ---- the handles, without a device


def test_symbols_present():
    L = _lib.lib()
    for name in ("amx_posterior_default_cfg", "amx_posterior_create", "amx_posterior_destroy", "amx_posterior_set_filter", "amx_posterior_set_default_filter",
                 "amx_posterior_set_single_filter", "amx_posterior_set_disregard", "amx_posterior_filter", "amx_posterior_set_topology",
                 "amx_posterior_set_topology_gmm", "amx_posterior_topology_info", "amx_posterior_dev", "amx_posterior_lists_dev", "amx_posterior_gmm_dev",
                 "amx_combine_create", "amx_combine_destroy", "amx_combine_identity_columns", "amx_combine_dev", "amx_gmm_topology"):
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert "StatePosteriorScorer" in rasr_amd.__all__ and "CombinedScorer" in rasr_amd.__all__


def test_defaults_are_the_references():
    cfg = _lib.PosteriorCfg()
    _lib.lib().amx_posterior_default_cfg(C.byref(cfg))
    assert (cfg.n_mixtures, cfg.scale, cfg.pruning_threshold, cfg.margin, cfg.viterbi) == (0, 1.0, DBL_MAX, 0.0, 1)
    h = rasr_amd.StatePosteriorScorer(None, 5)
    m, p = h.filter()
    assert m.tolist() == [0, 1, 2, 3, 4] and not p.any()   # DefaultFilter


def refused(status, word, fn, *a, **kw):
    with pytest.raises(rasr_amd.AmxError) as e:
        fn(*a, **kw)
    assert e.value.status == status and word in str(e.value), str(e.value)


def test_refused_configurations_name_their_parameter():
    refused(_lib.AMX_ERR_UNSUPPORTED, "viterbi", rasr_amd.StatePosteriorScorer, None, 4, viterbi=0)
    refused(_lib.AMX_ERR_INVALID, "n_mixtures", rasr_amd.StatePosteriorScorer, None, 0)
    refused(_lib.AMX_ERR_INVALID, "scale", rasr_amd.StatePosteriorScorer, None, 4, scale=float("nan"))
    with pytest.raises(TypeError):
        rasr_amd.StatePosteriorScorer(None, 4, context_priors=1)
    h = rasr_amd.StatePosteriorScorer(None, 4)
    refused(_lib.AMX_ERR_INVALID, "mixture[1] = 4", h.set_filter, [0, 4])
    refused(_lib.AMX_ERR_INVALID, "mixture[0] = -1", h.set_filter, [-1])
    refused(_lib.AMX_ERR_INVALID, "empty", h.set_filter, [])
    refused(_lib.AMX_ERR_INVALID, "empty", h.set_disregard, [0, 1, 2, 3])
    assert h.filter()[0].tolist() == [0, 1, 2, 3]   # a refused call changes nothing
    # a handle without a context computes nothing
    refused(_lib.AMX_ERR_STATE, "context", h.posteriors, None, 4, 0)


def test_filter_and_disregard_semantics():
    h = rasr_amd.StatePosteriorScorer(None, 6)
    h.set_filter([4, 1, 3, 1], [0.5, 9.0, 1.5, 2.5])
    m, p = h.filter()
    assert m.tolist() == [1, 3, 4] and p.tolist() == [2.5, 1.5, 0.5]   # increasing order; the last prior of a repeated mixture
    h.set_disregard([3, 5, 77])   # 3 is erased as a MIXTURE index; 5 is not in the filter, 77 names no mixture
    assert h.filter()[0].tolist() == [1, 4]
    h.set_single_filter(4)        # the disregard list applies to every filter set
    assert h.filter()[0].tolist() == [4] and h.filter()[1].tolist() == [0.0]
    refused(_lib.AMX_ERR_INVALID, "empty", h.set_single_filter, 3)
    assert h.filter()[0].tolist() == [4]
    h.set_disregard([])
    h.set_default_filter()
    assert h.filter()[0].tolist() == [0, 1, 2, 3, 4, 5]


def test_topology_flags():
    h = rasr_amd.StatePosteriorScorer(None, 3)
    refused(_lib.AMX_ERR_STATE, "topology", h.topology_info)
    h.set_topology([0, 2, 3, 5], [0, 1, 2, 3, 4])
    assert h.topology_info() == (True, -1)
    h.set_topology([0, 2, 3, 5], [1, 0, 2, 4, 3])   # permuted inside the mixtures only
    assert h.topology_info() == (True, -1)
    h.set_topology([0, 2, 3, 5], [3, 4, 2, 0, 1])
    assert h.topology_info() == (False, -1)
    h.set_topology([0, 2, 3, 5], [0, 1, 2, 1, 4])   # density 1 belongs to mixtures 0 and 2
    assert h.topology_info() == (False, 1)
    h.set_topology([0, 2, 3, 5], [0, 0, 2, 3, 4])   # twice within ONE mixture is no sharing
    assert h.topology_info() == (True, -1)
    refused(_lib.AMX_ERR_INVALID, "no density", h.set_topology, [0, 2, 2, 4], [0, 1, 2, 3])
    with pytest.raises(ValueError):
        h.set_topology([0, 1, 2], [0, 1])


def test_combination_table_validation():
    c = rasr_amd.CombinedScorer(None, [4, 9], [[0, 8], [1, 0], [2, 3], [3, 3]], [1.0, 0.5])
    assert c.identity_columns() == [True, False] and (c.n_models, c.n_emissions) == (2, 4)
    refused(_lib.AMX_ERR_INVALID, "table[1][1] = 9", rasr_amd.CombinedScorer, None, [4, 9], [[0, 8], [1, 9]], [1.0, 0.5])
    refused(_lib.AMX_ERR_INVALID, "table[0][0] = -1", rasr_amd.CombinedScorer, None, [4], [[-1]], [1.0])
    refused(_lib.AMX_ERR_INVALID, "n_models", rasr_amd.CombinedScorer, None, [2] * 9, [[0] * 9], [1.0] * 9)
    refused(_lib.AMX_ERR_INVALID, "n_emissions", rasr_amd.CombinedScorer, None, [2], np.zeros((0, 1), np.int32), [1.0])
    refused(_lib.AMX_ERR_INVALID, "n_mixtures[0]", rasr_amd.CombinedScorer, None, [0], [[0]], [1.0])
    with pytest.raises(ValueError):
        rasr_amd.CombinedScorer(None, [4, 9], [[0], [1]], [1.0, 0.5])
    assert rasr_amd.CombinedScorer(None, [3] * 8, [[0] * 8, [1] * 8, [2] * 8], [1.0] * 8).identity_columns() == [True] * 8
    refused(_lib.AMX_ERR_STATE, "context", c.combine, 0, [None, None], [4, 9], None, 4)
