"""CPU: MLLR without a device.  tests/mllr_reference.py (plain numpy) against tests/golden/ref_mllr.npz, what the reference's own text
computes in both of its builds (tests/golden/make_mllr_golden.py): every accumulator bit, count, index, shift estimate, adapted mean
given W and every file byte; then the library's host side (mllr_host.cpp: files, estimate) against the same fixture.

Only W of the full estimator carries a tolerance, the fixture's MEASURED bar: 4 x the largest distance, over the cases and both builds,
between the restatement with the library's Jacobi eigen-solver and the reference's text with OpenBLAS's dgelsd (bar/w_abs, bar/w_rel
in the fixture)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import mllr_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = mr.fixture()
CASES = mr.case_names(Z)
FULL_CASES = [n for n in CASES if n.startswith("full")]
BUILDS = ("off", "fma")
BAR = {k: float(Z["bar/" + k]) for k in ("w_abs", "w_rel")}
THR = {k[len("thresholds/"):]: tuple(Z[k]) for k in Z.files if k.startswith("thresholds/")}
ESTIMATES = ((0, "low"), (0, "default"), (0, "silence_high"), (2, "low"))
MODES = {mr.FULL: "full", mr.SHIFT: "shift"}
_ACC = {}


def acc_of(name, build):
    """the case's final accumulator of all keys: the restatement's, which test_restatement_equals_the_fixture holds to the reference's bits"""
    if (name, build) not in _ACC:
        _ACC[name, build] = mr.accumulate_case(mr.load_case(Z, name), build)
    return _ACC[name, build]


def estimator(c):
    return rasr_amd.ModelTransformEstimator(None, MODES[c["mode"]], c["n_leafs"], c["leaf_of_mixture"], n_keys=c["n_keys"], dim=c["D"])


def key_part(c, acc, key):
    size = c["n_leafs"] * mr.leaf_size(c["mode"], c["D"])
    return acc[key * size:(key + 1) * size]


def _close(got, want):
    d = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    assert d <= BAR["w_abs"] and d <= BAR["w_rel"] * float(np.abs(want).max()), (d, d / float(np.abs(want).max()), BAR)


def test_the_bar_is_the_measured_one_and_small():
    """4 x the measured distance, and far below what an adapted mean resolves: an f32 mean carries 2^-24 of its size"""
    for k, v in BAR.items():
        assert v == 4 * float(Z["measured/" + k]) and 0 < v < 2.0 ** -24 / 16, (k, v)
    assert int(Z["fma_instructions/off"]) == 0 and int(Z["fma_instructions/fma"]) > 0


def test_the_fixtures_inputs_keep_the_rank_decision_apart():
    """over every G that the full estimator inverts no singular value lies in [1e-14, 1e-10] x the largest, so dgelsd and the Jacobi
    solver truncate alike; rank-deficient and full-rank G both occur (recorded by the generator; recomputed here from the eigenvalues
    of the symmetrised G, whose moduli are its singular values)"""
    ranks = Z["inverted/rank_and_order"]
    assert (ranks[:, 0] < ranks[:, 1]).any() and (ranks[:, 0] == ranks[:, 1]).any()
    seen = []
    for name in FULL_CASES:
        c = mr.load_case(Z, name)
        for tname in ("low", "silence_high"):
            e = mr.estimate(key_part(c, acc_of(name, "off"), 0), c["tree"], c["leaf_of_mixture"], c["mode"], c["D"], c["n_leafs"], *THR[tname])
            for i, lam in e["eigenvalues"].items():
                s = np.sort(np.abs(lam))[::-1] / np.abs(lam).max()
                assert not np.any((s >= 1e-14) & (s <= 1e-10)), (name, i, s)
                seen.append(((s > 1e-12).sum(), len(s)))
    assert any(r < n for r, n in seen) and any(r == n for r, n in seen)
    # a rank-deficient one is a leaf over the threshold whose frames use fewer than D + 1 distinct means
    c = mr.load_case(Z, "full/d16/unweighted")
    assert len(c["model"]["means"]) < 17


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_fixture(name, build):
    """every accumulator bit after the cut and at the end, in one call and in two; the files; counts, ids, indices, shift estimates and
    the adapted means given the reference's matrices in every bit; W within the bar"""
    c = mr.load_case(Z, name)
    mode, D, L = c["mode"], c["D"], c["n_leafs"]
    acc = acc_of(name, build)
    assert mr.same_bits(mr.recorded(Z, name, build, "acc"), acc)
    assert mr.same_bits(mr.recorded(Z, name, build, "acc"), mr.accumulate_case(c, build, calls=2))
    assert mr.same_bits(mr.recorded(Z, name, build, "acc_cut"), mr.accumulate_case(c, build, upto=c["cut"]))
    assert not key_part(c, acc, 1).any()   # key 1 receives no frame
    for key in (0, 2):
        data = mr.accumulator_file(key_part(c, acc, key), mode, D, L, b"key%d" % key, map_ids=mr.map_ids(c["tree"]))
        assert mr.same_bits(mr.recorded(Z, name, build, "file/key%d" % key), np.frombuffer(data, np.uint8))
    for key, tname in ESTIMATES:
        pre = "est/key%d/%s/" % (key, tname)
        ref = {k: mr.recorded(Z, name, build, pre + k) for k in ("matrix_ids", "matrices", "matrix_of_mixture", "node_count", "adapted_means", "adaptor_file")}
        e = mr.estimate(key_part(c, acc, key), c["tree"], c["leaf_of_mixture"], mode, D, L, *THR[tname], contract=build)
        assert mr.same_bits(ref["matrix_ids"], e["matrix_ids"]) and mr.same_bits(ref["matrix_of_mixture"], e["matrix_of_mixture"])
        assert mr.same_bits(ref["node_count"], e["node_count"])
        assert bool(e["flags"] & mr.ROOT_FALLBACK) == (tname == "default" or key == 2)
        assert bool(e["flags"] & mr.SILENCE_FALLBACK) == (tname != "low" or key == 2)
        if mode == mr.SHIFT or e["flags"] == (mr.ROOT_FALLBACK | mr.SILENCE_FALLBACK):
            assert mr.same_bits(ref["matrices"], e["matrices"])
        else:
            for a, b in zip(e["matrices"], ref["matrices"]):
                _close(a, b)
        assert mr.same_bits(ref["adapted_means"], mr.adapt_means(c["model"], mode, ref["matrix_ids"], ref["matrices"], ref["matrix_of_mixture"], build))
        data = mr.adaptor_file(mode, D, ref["matrix_ids"], ref["matrices"], ref["matrix_of_mixture"], b"key%d" % key)
        assert mr.same_bits(ref["adaptor_file"], np.frombuffer(data, np.uint8))


def test_which_sums_depend_on_the_contract_mode():
    """the unweighted full sums are products of two widened f32 values, exact in f64; the shift estimator has no product in front of an
    addition; only the weighted full sums (and what is computed from them) differ between the reference's two builds"""
    for name in CASES:
        same = "%s/fma/acc_same_as_off" % name in Z.files
        assert same == (not (name.startswith("full") and name.endswith("/weighted"))), name   # Z of the weighted full sums
        assert mr.same_bits(acc_of(name, "off"), acc_of(name, "fma")) == same
        if name.startswith("full") and name.endswith("/weighted"):   # the counts count frames in both
            c = mr.load_case(Z, name)
            ls = mr.leaf_size(c["mode"], c["D"])
            a, b = acc_of(name, "off").reshape(-1, ls), acc_of(name, "fma").reshape(-1, ls)
            g0 = 1 + c["D"] * (c["D"] + 1)
            assert np.array_equal(a[:, [0, g0]], b[:, [0, g0]]) and np.array_equal(a[:, 0], np.round(a[:, 0])) and np.array_equal(a[:, 0], a[:, g0])


@pytest.mark.parametrize("name", CASES)
def test_library_files_estimate_and_index_vector(name, tmp_path):
    c = mr.load_case(Z, name)
    mode, D, L = c["mode"], c["D"], c["n_leafs"]
    est = estimator(c)
    assert est.key_size() == L * mr.leaf_size(mode, D) and est.leaf_size() == mr.leaf_size(mode, D)
    for build in BUILDS:
        acc = acc_of(name, build)
        for key in (0, 2):
            p = str(tmp_path / ("%s_%d.acc" % (build, key)))
            est.write(acc, p, key, cluster_id="key%d" % key, map_ids=mr.map_ids(c["tree"]))
            assert mr.same_bits(mr.recorded(Z, name, build, "file/key%d" % key), np.fromfile(p, np.uint8))
            back, mo, ms = est.read(p, thresholds=True)
            assert mr.same_bits(key_part(c, acc, key), back) and (mo, ms) == (1000.0, 500.0)
        for key, tname in ESTIMATES:
            pre = "est/key%d/%s/" % (key, tname)
            ref = {k: mr.recorded(Z, name, build, pre + k) for k in ("matrix_ids", "matrices", "matrix_of_mixture", "node_count", "adaptor_file")}
            e = est.estimate(acc, c["tree"], key, *THR[tname])
            assert mr.same_bits(ref["matrix_ids"], e["matrix_ids"]) and mr.same_bits(ref["matrix_of_mixture"], e["matrix_of_mixture"])
            assert mr.same_bits(ref["node_count"], e["node_count"])
            assert e["root_fallback"] == (tname == "default" or key == 2) and e["silence_fallback"] == (tname != "low" or key == 2)
            if mode == mr.SHIFT or (e["root_fallback"] and e["silence_fallback"]):
                assert mr.same_bits(ref["matrices"], e["matrices"])
            else:
                for a, b in zip(e["matrices"], ref["matrices"]):
                    _close(a, b)
                # the library is the restatement's arithmetic (nothing fused) operation by operation
                mine = mr.estimate(key_part(c, acc, key), c["tree"], c["leaf_of_mixture"], mode, D, L, *THR[tname], contract="off")
                assert mr.same_bits(mine["matrices"], e["matrices"])
            p = str(tmp_path / "a.adaptor")
            est.write_adaptor(p, ref["matrix_ids"], ref["matrices"], ref["matrix_of_mixture"], cluster_id="key%d" % key)
            assert mr.same_bits(ref["adaptor_file"], np.fromfile(p, np.uint8))
            back = est.read_adaptor(p)
            assert all(mr.same_bits(ref[k], back[k]) for k in ("matrix_ids", "matrices", "matrix_of_mixture"))


def test_every_planted_defect_leaves_its_check():
    """each defect of mllr_reference.DEFECTS changes accumulator bits, counts, ids or indices, or moves W out of the bar, on at least one case
    -- except `right_first`, which provably cannot (see below) and is pinned as such"""
    left = {d: 0 for d in mr.DEFECTS}
    for name in CASES:
        c = mr.load_case(Z, name)
        mode, D, L = c["mode"], c["D"], c["n_leafs"]
        want = mr.recorded(Z, name, "off", "acc")
        for d in ("out_of_order", "weighted_count", "f64_subtract"):
            left[d] += not mr.same_bits(want, mr.accumulate_case(c, "off", defect=d))
        if D > 5:   # the estimate's defects show at D = 3 and 5 (rank-deficient G included: the silence leaf has two means)
            continue
        acc = key_part(c, acc_of(name, "off"), 0)
        for d in ("ge_threshold", "right_first", "silence_propagated", "wrong_rcond"):
            for tname in ("low", "silence_high"):
                thr = THR[tname]
                if d == "ge_threshold":   # a threshold that a node's count equals
                    counts = mr.recorded(Z, name, "off", "est/key0/%s/node_count" % tname)
                    thr = (float(counts[c["tree"]["leaf_list"][0]]), thr[1])
                right = mr.estimate(acc, c["tree"], c["leaf_of_mixture"], mode, D, L, *thr)
                e = mr.estimate(acc, c["tree"], c["leaf_of_mixture"], mode, D, L, *thr, defect=d)
                differs = not (mr.same_bits(right["matrix_ids"], e["matrix_ids"]) and mr.same_bits(right["matrix_of_mixture"], e["matrix_of_mixture"]) and
                               mr.same_bits(right["node_count"], e["node_count"]))
                if not differs and mode == mr.SHIFT:
                    differs = not mr.same_bits(right["matrices"], e["matrices"])
                elif not differs:
                    differs = any(float(np.abs(a - b).max()) > min(BAR["w_abs"], BAR["w_rel"] * float(np.abs(b).max()))
                                  for a, b in zip(e["matrices"], right["matrices"]))
                left[d] += differs
    # node = right, then += left: IEEE addition commutes, a + b and b + a are the same bits, and a node has exactly two children -- this
    # defect provably cannot leave a mark (the recursion order decides nothing else either); it is pinned as such
    assert left.pop("right_first") == 0
    assert all(v > 0 for v in left.values()), left


def test_refusals(tmp_path):
    L = _lib.lib()
    name = "full/d5/weighted"
    c, acc = mr.load_case(Z, name), acc_of(name, "off")
    est = estimator(c)
    tree = c["tree"]
    # the modes that are not built name their parameter
    for mode in ("band", "semi-tied"):
        with pytest.raises(rasr_amd.AmxError, match=mode) as e:
            rasr_amd.ModelTransformEstimator(None, mode, 4, c["leaf_of_mixture"], dim=5)
        assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        rasr_amd.ModelTransformEstimator(None, "diagonal", 4, c["leaf_of_mixture"], dim=5)
    with pytest.raises(ValueError):
        rasr_amd.ModelTransformEstimator(None, "full", 4, c["leaf_of_mixture"])
    # limits: D <= 255, n_leafs <= 4096 (host shape), n_keys <= 65535 and the rest at creation, before the scorer's device is asked for
    for kw in (dict(dim=256), dict(dim=5, n_leafs=4097), dict(dim=0)):
        with pytest.raises(rasr_amd.AmxError):
            rasr_amd.ModelTransformEstimator(None, "full", kw.pop("n_leafs", 4), c["leaf_of_mixture"], **kw)
    gmm = rasr_amd.GmmFeatureScorer(None, dict(c["model"]))
    h = C.c_void_p()
    lom = np.ascontiguousarray(c["leaf_of_mixture"], np.int32)
    for args, status, text in (((_lib.AMX_MLLR_FULL, 65536, 4), _lib.AMX_ERR_UNSUPPORTED, b"n_keys"), ((_lib.AMX_MLLR_FULL, 0, 4), _lib.AMX_ERR_INVALID, b"n_keys"),
                               ((_lib.AMX_MLLR_FULL, 1, 4097), _lib.AMX_ERR_UNSUPPORTED, b"n_leafs"), ((_lib.AMX_MLLR_FULL, 1, 3), _lib.AMX_ERR_INVALID, b"leaf 3"),
                               ((_lib.AMX_MLLR_BAND, 1, 4), _lib.AMX_ERR_UNSUPPORTED, b"band"), ((_lib.AMX_MLLR_SEMI_TIED, 1, 4), _lib.AMX_ERR_UNSUPPORTED, b"semi-tied"),
                               ((7, 1, 4), _lib.AMX_ERR_INVALID, b"unknown mode"), ((_lib.AMX_MLLR_FULL, 1, 4), _lib.AMX_ERR_STATE, b"host-only")):
        assert L.amx_mllr_create(gmm.h, args[0], args[1], args[2], lom.ctypes.data, C.byref(h)) == status, (args, L.amx_last_error())
        assert text in L.amx_last_error(), (args, L.amx_last_error())
    wide = dict(c["model"])
    wide["dim"] = 256
    wide["means"] = np.zeros((len(c["model"]["means"]), 256), np.float32)
    wide["variances"] = np.ones((len(c["model"]["variances"]), 256), np.float32)
    gw = rasr_amd.GmmFeatureScorer(None, wide)
    assert L.amx_mllr_create(gw.h, _lib.AMX_MLLR_FULL, 1, 4, lom.ctypes.data, C.byref(h)) == _lib.AMX_ERR_UNSUPPORTED and b"dimension 256" in L.amx_last_error()
    # trees that are no trees, a leaf out of range, silence outside the model
    def broken(**kw):
        t = {k: np.array(v) for k, v in tree.items()}
        for k, (i, v) in kw.items():
            t[k][i] = v
        return t
    root, first = tree["root"], int(tree["leaf_list"][0])
    for t in (broken(left=(root, root)), broken(right=(root, len(tree["left"]))), broken(left=(root, int(tree["right"][root]))),
              broken(leaf_number=(first, c["n_leafs"])), broken(previous=(first, first)), broken(leaf_list=(0, root)),
              broken(silence_mixtures=(0, len(c["leaf_of_mixture"]))), dict(tree, root=-1), dict(tree, root=len(tree["left"]))):
        with pytest.raises(rasr_amd.AmxError) as e:
            est.estimate(acc, t, 0, *THR["low"])
        assert e.value.status == _lib.AMX_ERR_INVALID
    with pytest.raises(ValueError):
        est.estimate(acc, dict(tree, left=tree["left"][:-1]), 0)
    bad = rasr_amd.ModelTransformEstimator(None, "full", 4, np.array([0, 0, 1, 1, 2, 2, 2, 4]), dim=5)
    with pytest.raises(rasr_amd.AmxError, match="leaf 4"):
        bad.estimate(key_part(c, acc, 0), tree, 0)
    # files: truncated, wrong tag, another dimension, another leaf count
    p = str(tmp_path / "a.acc")
    est.write(acc, p, map_ids=mr.map_ids(tree))
    raw = open(p, "rb").read()
    for cutoff in (0, 3, 20, 50, len(raw) // 2, len(raw) - 1):
        open(p, "wb").write(raw[:cutoff])
        with pytest.raises(rasr_amd.AmxError):
            est.read(p)
    open(p, "wb").write(raw.replace(b"full-adaptor", b"fool-adaptor"))
    with pytest.raises(rasr_amd.AmxError, match="type tag"):
        est.read(p)
    open(p, "wb").write(raw)
    with pytest.raises(rasr_amd.AmxError, match="type tag"):
        rasr_amd.ModelTransformEstimator(None, "shift", 4, c["leaf_of_mixture"], dim=5).read(p)
    with pytest.raises(rasr_amd.AmxError, match="dimension"):
        rasr_amd.ModelTransformEstimator(None, "full", 4, c["leaf_of_mixture"], dim=6).read(p)
    with pytest.raises(rasr_amd.AmxError, match="leaf"):
        rasr_amd.ModelTransformEstimator(None, "full", 5, c["leaf_of_mixture"], dim=5).read(p)
    e = est.estimate(acc, tree, 0, *THR["low"])
    q = str(tmp_path / "a.adaptor")
    est.write_adaptor(q, e["matrix_ids"], e["matrices"], e["matrix_of_mixture"])
    raw = open(q, "rb").read()
    for cutoff in (0, 5, 30, len(raw) // 2, len(raw) - 1):
        open(q, "wb").write(raw[:cutoff])
        with pytest.raises(rasr_amd.AmxError):
            est.read_adaptor(q)
    open(q, "wb").write(raw)
    with pytest.raises(rasr_amd.AmxError, match="more matrices"):
        est.read_adaptor(q, max_matrices=1)
    with pytest.raises(rasr_amd.AmxError, match="ascend"):
        est.write_adaptor(q, e["matrix_ids"][::-1], e["matrices"][::-1], e["matrix_of_mixture"])


def test_shared_means_are_refused_by_the_restatement_too():
    """a mean that two (mixture, density) visits reach would be transformed twice by adaptMixtureSet; amx_mllr_create refuses such a
    model on the device (tests/test_mllr_gpu.py), the restatement names it"""
    c = mr.load_case(Z, "full/d3/unweighted")
    assert (mr.mean_mixture(c["model"]) >= 0).all()
    tied = dict(c["model"])
    tied["dens_mean"] = np.array(tied["dens_mean"])
    tied["dens_mean"][1] = tied["dens_mean"][0]
    assert mr.mean_mixture(tied) is None


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_mllr_test.cc compiles mllr_host.cpp into a program of its own: files, the estimate of exported cases and every refusal;
    built with -fsanitize=address,undefined on the host side only, run as a process of its own (nothing sanitized is loaded into Python).
    Sanitizers are for machines without a GPU: where one is present the same program is built and run plainly."""
    import torch
    exe = str(tmp_path / "host_mllr_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_mllr_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    for name in ("full/d5/weighted", "full/d16/unweighted", "shift/d5/weighted"):
        c, acc = mr.load_case(Z, name), acc_of(name, "off")
        tree, pre = c["tree"], "est/key0/low/"
        ref = {k: mr.recorded(Z, name, "off", pre + k) for k in ("matrix_ids", "matrices", "matrix_of_mixture", "adaptor_file")}
        d = tmp_path / name.replace("/", "_")
        d.mkdir()
        with open(d / "case.bin", "wb") as f:
            np.array([c["mode"], c["D"], c["n_leafs"], len(c["leaf_of_mixture"]), len(tree["left"]), tree["root"], len(tree["leaf_list"]),
                      len(tree["silence_mixtures"]), len(ref["matrix_ids"])], np.int32).tofile(f)
            for k in ("left", "right", "previous", "leaf_number", "leaf_list", "silence_mixtures"):
                np.asarray(tree[k], np.int32).tofile(f)
            np.asarray(c["leaf_of_mixture"], np.int32).tofile(f)
            np.array(THR["low"], np.float64).tofile(f)
            key_part(c, acc, 0).tofile(f)
            np.asarray(ref["matrix_ids"], np.int32).tofile(f)
            np.asarray(ref["matrix_of_mixture"], np.int32).tofile(f)
            np.asarray(ref["matrices"], np.float64).tofile(f)
        mr.recorded(Z, name, "off", "file/key0").tofile(str(d / "key0.acc"))
        ref["adaptor_file"].tofile(str(d / "key0.adaptor"))
        r = subprocess.run([exe, str(d / "case.bin"), str(d), repr(BAR["w_abs"]), repr(BAR["w_rel"])], capture_output=True, text=True)
        assert r.returncode == 0 and "host_mllr_test: ok" in r.stdout, name + "\n" + r.stdout + r.stderr
