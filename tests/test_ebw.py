"""CPU side of EBW training.  The restatement of tests/ebw_reference.py (sides, collection, accumulation, file bytes, combine, estimate)
against tests/golden/ref_ebw.npz -- the reference's own text compiled in both builds -- in every bit, in closed form and on exact sums;
its planted defects; ebw_host.cpp (the estimator file, combine, amx_ebw_estimate) through the ABI against the restatement in every bit;
the refusals; the entry points of ebw.hip that need no device; tests/host_ebw_test.cc under the host sanitizers."""
import os

import numpy as np
import pytest

from tests import ebw_reference as er
from tests import synth

KS = (1, 5, 3, 2, 4, 5)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def small(D=4, pooled=False, seed=3):
    """two segments (5 and 9 frames, three rows in front), 40 arcs with weights over 20 binary exponents, a model and random best densities"""
    rng = np.random.Generator(np.random.PCG64(seed))
    model = synth.gmm_cart(len(KS), 1, 5, D, seed=seed, pooled=pooled, ks=KS)
    off = np.array([3, 8, 17], np.int64)
    w, i_off, fr, em = [], [0], [], []
    for a in range(40):
        n = 5 if a < 15 else 9
        length = int(rng.integers(0, n + 1))
        start = int(rng.integers(0, n - length + 1))
        fr.extend(range(start, start + length))
        em.extend(rng.integers(0, 3, length))                       # three mixtures: keys collide
        i_off.append(len(fr))
        w.append(float(rng.uniform(1, 2)) * 2.0 ** -int(rng.integers(0, 20)) * (1 if rng.random() < 0.5 else -1))
    w[7], w[8] = float(er.EPSILON), -float(er.EPSILON)
    lat = (np.array([0, 15, 40], np.int64), np.array(w, np.float32), np.array(i_off, np.int64), np.array(fr, np.int32), np.array(em, np.int32))
    feats = (rng.standard_normal((17, D)) * 1.5).astype(np.float32)
    best = np.stack([rng.integers(0, k, 17) for k in KS], axis=1).astype(np.uint32)
    return dict(model=model, off=off, lat=lat, feats=feats, best=best)


def test_sides_follow_the_f32_comparison():
    up, eps = np.nextafter(er.EPSILON, np.float32(1)), er.EPSILON
    assert [er.side_of(v) for v in (eps, -eps, 0.0, up, -up, 1.0, -1.0)] == [-1, -1, -1, er.NUM, er.DEN, er.NUM, er.DEN]
    assert er.side_of(eps, defect="threshold-not-strict") == er.NUM and er.side_of(-eps, defect="threshold-not-strict") == er.DEN
    assert er.side_of(np.nan) == -1
    # the comparison is f32: a double just above epsilon narrows to epsilon and counts for neither side
    assert er.side_of(float(eps) * (1 + 2.0 ** -40)) == -1
    assert er.side_of(0.5, threshold=0.5) == -1 and er.side_of(-0.75, threshold=0.5) == er.DEN


def test_collection_sums_the_widened_weights_per_side_frame_and_mixture():
    p = small()
    a_off, w, i_off, fr, em = p["lat"]
    keys = er.collect(p["off"], *p["lat"])
    # the same sums from exact integers: every weight is a multiple of 2^-42 below 2, a key's sum is below 2^53 of them
    want, fed = {}, {}
    for s in range(2):
        for a in range(a_off[s], a_off[s + 1]):
            if abs(w[a]) > er.EPSILON:
                for i in range(i_off[a], i_off[a + 1]):
                    k = (er.NUM if w[a] > 0 else er.DEN, int(p["off"][s] - p["off"][0]) + int(fr[i]), int(em[i]))
                    want[k] = want.get(k, 0) + int(abs(float(w[a])) * 2.0 ** 42)
                    fed[k] = fed.get(k, 0) + 1
    assert {(k["side"], k["frame"], k["mixture"]): k["weight"] for k in keys} == {k: v / 2.0 ** 42 for k, v in want.items()}
    assert max(fed.values()) >= 3                                     # keys fed by three and more arcs
    assert any((1 - s, f, m) in want for (s, f, m) in want)
    first = [(k["side"], k["frame"], k["mixture"]) for k in keys]
    assert len(set(first)) == len(first)


def test_accumulation_in_closed_form():
    """one numerator and one denominator key on one density: every cell from its definition"""
    p = small(D=3)
    o, m = er.layout(p["model"]), p["model"]
    keys = [dict(segment=0, side=er.NUM, frame=1, mixture=2, weight=0.75), dict(segment=0, side=er.DEN, frame=4, mixture=2, weight=0.5)]
    best = np.zeros((17, len(KS)), np.uint32)
    best[:, 2] = 1
    acc = er.accumulate(m, p["feats"], best, keys)
    slot = int(m["mix_offsets"][2]) + 1
    d = int(m["dens_index"][slot])
    mean, cov = int(m["dens_mean"][d]), int(m["dens_cov"][d])
    x1, x4 = p["feats"][1].astype(np.float64), p["feats"][4].astype(np.float64)
    want = np.zeros(o["size"])
    want[slot] = 0.75                                                 # weights_: the numerator key only
    want[o["den_density_weights"] + slot] = 0.5
    want[o["num_mean_weights"] + mean], want[o["den_mean_weights"] + mean] = 0.75, 0.5
    want[o["num_cov_weights"] + cov], want[o["den_cov_weights"] + cov] = 0.75, 0.5
    want[o["num_mean_sums"] + 3 * mean:][:3], want[o["den_mean_sums"] + 3 * mean:][:3] = 0.75 * x1, 0.5 * x4
    want[o["num_cov_sums"] + 3 * cov:][:3], want[o["den_cov_sums"] + 3 * cov:][:3] = (0.75 * x1) * x1, (0.5 * x4) * x4
    assert np.array_equal(bits(acc), bits(want))
    best[:, 2] = 0xFFFFFFFF                                           # no density: the keys are left out
    assert not er.accumulate(m, p["feats"], best, keys).any()
    er.accumulate_objective(m, acc, 0.1)
    assert acc[-1] == float(np.float32(0.1)) and o["objective"] == o["size"] - 1


@pytest.mark.parametrize("pooled", [False, True])
def test_orders_contracts_and_defects_are_told_apart(pooled):
    p = small(D=5, pooled=pooled)
    keys = er.collect(p["off"], *p["lat"])
    x, best = p["feats"][3:], p["best"][3:]
    dev = er.accumulate(p["model"], x, best, keys, "device", "off")
    order = er.key_order(keys, "device")
    assert [(keys[i]["frame"], keys[i]["mixture"], keys[i]["side"]) for i in order] == sorted((k["frame"], k["mixture"], k["side"]) for k in keys)
    assert np.array_equal(bits(er.accumulate(p["model"], x, best, keys, order, "off")), bits(dev))
    assert not np.array_equal(bits(er.accumulate(p["model"], x, best, keys, order[::-1], "off")), bits(dev))
    assert not np.array_equal(bits(er.accumulate(p["model"], x, best, keys, "device", "fma")), bits(dev))
    srt = er.accumulate(p["model"], x, best, keys, "sorted", "off")   # another order, the same sums: close, not equal in general
    assert np.allclose(srt, dev, rtol=1e-12, atol=1e-12)
    # cut between the segments: the chains continue
    first = [k for k in keys if k["segment"] == 0]
    second = [k for k in keys if k["segment"] == 1]
    cut = er.accumulate(p["model"], x, best, second, "device", "off", er.accumulate(p["model"], x, best, first, "device", "off"))
    assert np.array_equal(bits(cut), bits(dev))
    for defect in ("threshold-not-strict", "denominator-subtracted", "sides-swapped"):
        bad = er.accumulate(p["model"], x, best, er.collect(p["off"], *p["lat"], defect=defect), "device", "off", defect=defect)
        assert not np.array_equal(bits(bad), bits(dev)), defect
    # reversed arcs: widened f32 weights within 29 binary exponents add without rounding, so the order of collection shows only on weights
    # further apart (tests/test_ebw_gpu.py plants such a key)
    rev = er.collect(p["off"], *p["lat"], defect="reversed-arcs")
    assert {(k["side"], k["frame"], k["mixture"]): k["weight"] for k in rev} == {(k["side"], k["frame"], k["mixture"]): k["weight"] for k in keys}
    wide = (np.array([0, 3], np.int64), np.array([1024 * (1 + 2.0 ** -23), 2.0 ** -22 * (1 + 2.0 ** -21), 2.0 ** -22 * (1 + 2.0 ** -21)], np.float32),
            np.array([0, 1, 2, 3], np.int64), np.zeros(3, np.int32), np.zeros(3, np.int32))
    assert er.collect([0, 1], *wide)[0]["weight"] != er.collect([0, 1], *wide, defect="reversed-arcs")[0]["weight"]


Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ebw.npz"))
CASES = [str(c) for c in Z["cases"]]


def load_case(name):
    model = {k: Z["%s/model/%s" % (name, k)] for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov", "means", "variances", "log_weight")}
    model["dim"] = int(model["means"].shape[1])
    c = {k: Z["%s/%s" % (name, k)] for k in ("frame_offsets", "feats", "best")}
    c["lat"] = tuple(Z["%s/%s" % (name, k)] for k in ("arc_offsets", "arc_weight", "item_offsets", "item_frame", "item_emission"))
    c["model"] = model
    return c


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_text_in_every_bit(name, contract):
    """tests/golden/ref_ebw.npz: the reference's weight test, Collector, functors, unrolledTransform and VectorAccumulator::accumulate
    compiled in both builds, with the order in which its unordered_map walked.  Given that order the restatement is the reference in
    every bit; in the library's order it stays within bar (a), measured by the generator against the reference's text"""
    c = load_case(name)
    keys = er.collect(c["frame_offsets"], *c["lat"])
    order, ref = Z["%s/%s/order" % (name, contract)], Z["%s/%s/acc" % (name, contract)]
    assert sorted(order) == list(range(len(keys)))
    assert np.array_equal(bits([keys[i]["weight"] for i in order]), bits(Z["%s/%s/weights" % (name, contract)]))
    mine = er.accumulate(c["model"], c["feats"], c["best"], keys, order, contract)
    assert np.array_equal(bits(mine), bits(ref)), np.argwhere(bits(mine) != bits(ref))[:5]
    dev = er.accumulate(c["model"], c["feats"], c["best"], keys, "device", contract)
    dist = float(np.max(np.abs(dev - ref) / np.maximum(1.0, np.abs(ref))))
    print("%s %s: device order against the reference's order %.3g, bar (a) %.3g" % (name, contract, dist, float(Z["bar_a"])))
    assert dist <= float(Z["bar_a"]) and float(Z["bar_a"]) == 4.0 * float(Z["bar_a_measured"])
    if c["model"]["dim"] > 1:   # the other build is other bits: the fixture tells the contracts apart
        assert not np.array_equal(bits(er.accumulate(c["model"], c["feats"], c["best"], keys, order, "fma" if contract == "off" else "off")), bits(ref))
    # every planted defect leaves its check: three of them bar (a), which is the check of an accumulation in another order; the reversed
    # arcs the bits of the collected weights, through the one key whose collection rounds
    for defect in ("threshold-not-strict", "denominator-subtracted", "sides-swapped"):
        bad = er.accumulate(c["model"], c["feats"], c["best"], er.collect(c["frame_offsets"], *c["lat"], defect=defect), "device", contract, defect=defect)
        assert float(np.max(np.abs(bad - ref) / np.maximum(1.0, np.abs(ref)))) > float(Z["bar_a"]), defect
    rev = {(k["side"], k["frame"], k["mixture"]): k["weight"] for k in er.collect(c["frame_offsets"], *c["lat"], defect="reversed-arcs")}
    fwd = {(k["side"], k["frame"], k["mixture"]): k["weight"] for k in keys}
    assert [k for k in fwd if fwd[k] != rev[k]] == [(er.NUM, 2, 3)]
    assert not np.array_equal(bits([rev[(keys[i]["side"], keys[i]["frame"], keys[i]["mixture"])] for i in order]), bits(Z["%s/%s/weights" % (name, contract)]))


@pytest.mark.parametrize("name", CASES)
def test_weights_and_file_are_the_reference_classes(name, tmp_path):
    """ref_ebw.npz also holds what the reference's mixture estimators' own text does with a denominator key, called as the mixture set calls
    them: the EBW class leaves weights_ to the numerator (its accumulateDenominator overrides the base class's without calling it), the
    base class subtracts.  The planted defect "denominator-subtracted" is the base class's text.  And it holds the bytes that the
    reference's write chain, compiled, makes of the accumulators: the restatement's and the library's file are those bytes"""
    import rasr_amd
    c = load_case(name)
    keys = er.collect(c["frame_offsets"], *c["lat"])
    nk = int(c["model"]["mix_offsets"][-1])
    for contract in ("off", "fma"):
        order, ref = Z["%s/%s/order" % (name, contract)], Z["%s/%s/acc" % (name, contract)]
        base = Z["%s/%s/base_class_weights" % (name, contract)]
        assert (ref[:nk] >= 0).all() and (base < 0).any()
        bad = er.accumulate(c["model"], c["feats"], c["best"], keys, order, contract, defect="denominator-subtracted")
        assert np.array_equal(bits(bad[:nk]), bits(base)) and not np.array_equal(bits(bad[:nk]), bits(ref[:nk]))
        assert np.array_equal(bits(bad[nk:]), bits(ref[nk:]))
    acc, raw = Z[name + "/file_acc"], Z[name + "/file"].tobytes()
    assert acc[-1] != 0.0 and acc[er.layout(c["model"])["den_density_weights"]:-1].any()
    assert er.file_bytes(c["model"], acc) == raw
    path = str(tmp_path / "ebw.acc")
    rasr_amd.EbwAccumulator.write(c["model"], acc, path)
    assert open(path, "rb").read() == raw
    open(path, "wb").write(raw)
    assert np.array_equal(bits(rasr_amd.EbwAccumulator.read(c["model"], path)), bits(acc))


def test_host_only_handle_layout_and_refusals():
    import ctypes as C

    import rasr_amd
    from rasr_amd import _lib
    L = _lib.lib()
    for pooled in (False, True):
        p = small(D=7, pooled=pooled)
        gmm = rasr_amd.GmmFeatureScorer(None, p["model"])
        ebw = rasr_amd.EbwAccumulator(gmm)
        o = er.layout(p["model"])
        assert ebw.accumulator_size() == o["size"] == 2 * gmm_size(p["model"]) + 1
        assert all(getattr(ebw.layout, k) == v for k, v in o.items())
        assert ebw.weight_threshold == float(er.EPSILON)
        acc = np.arange(o["size"], dtype=np.float64)
        assert ebw.view(acc, "den_cov_sums").shape == (p["model"]["variances"].shape[0], 7) and ebw.view(acc, "objective")[0] == o["size"] - 1
        assert ebw.view(acc, "num_mean_weights")[0] == o["num_mean_weights"]
        with pytest.raises(KeyError):
            ebw.view(acc, "weights")
        before = acc.copy()
        with pytest.raises(rasr_amd.AmxError, match="host-only") as e:
            ebw.accumulate_dev(p["feats"], 7, p["off"], *p["lat"], acc)
        assert e.value.status == _lib.AMX_ERR_STATE and np.array_equal(acc, before)
        with pytest.raises(rasr_amd.AmxError, match="host-only") as e:
            ebw.accumulate_objective(1.0, acc)
        assert e.value.status == _lib.AMX_ERR_STATE and np.array_equal(acc, before)
        with pytest.raises(rasr_amd.AmxError, match="viterbi") as e:
            rasr_amd.EbwAccumulator(gmm, viterbi=False)
        assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
        with pytest.raises(rasr_amd.AmxError, match="weight_threshold") as e:
            rasr_amd.EbwAccumulator(gmm, weight_threshold=float("nan"))
        assert e.value.status == _lib.AMX_ERR_INVALID
        with pytest.raises(rasr_amd.AmxError, match="feats_ld") as e:
            ebw.accumulate_dev(p["feats"], 6, p["off"], *p["lat"], acc)
        assert e.value.status == _lib.AMX_ERR_INVALID
    h = C.c_void_p()
    assert L.amx_ebw_create(None, None, C.byref(h)) == _lib.AMX_ERR_INVALID and not h.value
    assert L.amx_ebw_accumulator_size(None) == 0
    assert L.amx_ebw_layout(None, None) == _lib.AMX_ERR_INVALID
    cfg = _lib.EbwCfg()
    L.amx_ebw_cfg_default(C.byref(cfg))
    assert cfg.viterbi == 1 and cfg.weight_threshold == float(er.EPSILON)


def random_acc(model, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    acc = rng.standard_normal(er.layout(model)["size"]) * 100
    acc[3] = -0.0
    return acc


@pytest.mark.parametrize("pooled", [False, True])
def test_estimator_file_bytes_round_trip_and_combine(tmp_path, pooled):
    import rasr_amd
    from rasr_amd import _lib
    p = small(D=6, pooled=pooled)
    model, o = p["model"], er.layout(p["model"])
    acc = random_acc(model, 11)
    path = str(tmp_path / "ebw.acc")
    assert rasr_amd.EbwAccumulator.topology_size(model) == o["size"]
    rasr_amd.EbwAccumulator.write(model, acc, path)
    raw = open(path, "rb").read()
    assert raw == er.file_bytes(model, acc)
    # the frame of the file is the plain estimator file's, which amx_gmm_accumulator_write writes from the numerator block
    sc = rasr_amd.GmmFeatureScorer(None, model)
    plain = str(tmp_path / "plain.acc")
    sc.write_accumulator(acc[:o["den_density_weights"]], plain)
    assert open(plain, "rb").read() == er.file_bytes(model, acc, plain=True)
    back = rasr_amd.EbwAccumulator.read(model, path)
    assert np.array_equal(bits(back), bits(acc))
    # combine: the sum in every cell, the objective included
    add = random_acc(model, 12)
    both = rasr_amd.EbwAccumulator.combine(model, acc.copy(), add)
    assert np.array_equal(bits(both), bits(er.combine(acc, add))) and both[-1] == acc[-1] + add[-1]

    def refused(match, data=None, mdl=model):
        if data is not None:
            open(path, "wb").write(data)
        with pytest.raises(rasr_amd.AmxError, match=match) as e:
            rasr_amd.EbwAccumulator.read(mdl, path)
        assert e.value.status == _lib.AMX_ERR_INVALID

    # a refused file leaves the caller's buffer as it was (through the ABI: the wrapper hands out a fresh array)
    import ctypes as C
    keep, mark = [], np.full(o["size"], 7.5)
    st = rasr_amd._gmm_struct(model, 1.0, 1.0, keep)
    for cut in list(range(0, len(raw), 37)) + [len(raw) - 1]:
        open(path, "wb").write(raw[:cut])
        assert _lib.lib().amx_ebw_accumulator_read(C.byref(st), path.encode(), mark.ctypes.data) == _lib.AMX_ERR_INVALID, cut
        assert (mark == 7.5).all()
    refused("bytes behind the objective", raw + b"\0")
    refused("not a DTACC", b"SP_ARC1\0" + raw[8:])
    refused("not a DTACC", b"MIXSET\0\0" + raw[8:])          # the plain estimator's magic
    refused("not a DTACC", b"DTACCR\0\0" + raw[8:])          # the Rprop estimator's
    open(path, "wb").write(b"DTACC\0xy" + raw[8:])                # what lies behind the terminator is not compared (strcmp)
    assert np.array_equal(bits(rasr_amd.EbwAccumulator.read(model, path)), bits(acc))
    refused("version below 2", er.file_bytes(model, acc, version=1))
    refused("unknown version", er.file_bytes(model, acc, version=3))
    refused("not a DTACC", er.file_bytes(model, acc, plain=True))                          # the plain estimator's file is not this class's,
    refused("truncated or its topology differs", b"DTACC\0\0\0" + er.file_bytes(model, acc, plain=True)[8:])   # under either magic
    other = small(D=6, pooled=pooled, seed=4)["model"]
    other["dens_mean"] = other["dens_mean"][::-1].copy()
    refused("topology differs", raw, other)
    refused("dimension differs", raw, small(D=5, pooled=pooled)["model"])
    os.remove(path)
    refused("cannot open")
    bad = add.copy()
    bad[5] = np.inf
    before = acc.copy()
    with pytest.raises(rasr_amd.AmxError, match="entry 5 of an accumulator is not finite") as e:
        rasr_amd.EbwAccumulator.combine(model, acc, bad)
    assert e.value.status == _lib.AMX_ERR_INVALID and np.array_equal(bits(acc), bits(before))
    with pytest.raises(ValueError):
        rasr_amd.EbwAccumulator.write(model, acc[:-1], path)
    broken = dict(model)
    broken["dens_cov"] = model["dens_cov"].copy()
    broken["dens_cov"][0] = 1000
    with pytest.raises(rasr_amd.AmxError, match="density 0"):
        rasr_amd.EbwAccumulator.write(broken, acc, path)


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_ebw_test.cc compiles ebw_host.cpp into a program of its own: the file of a model against the restatement's bytes, the
    read of every truncation, mismatched topologies, combine; built with -fsanitize=address,undefined on the host side only and run as a
    process of its own (nothing sanitized is loaded into Python).  Where a GPU is present the same program is built and run plainly."""
    import os
    import subprocess

    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_ebw_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(root, "tests", "host_ebw_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    for pooled, ks in ((False, KS), (True, KS), (False, (1,))):         # the last: one mixture of one density
        model = synth.gmm_cart(len(ks), 1, 5, 3, seed=9, pooled=pooled, ks=ks)
        acc, add = random_acc(model, 21), random_acc(model, 22)
        d = tmp_path / ("case_%d_%d" % (pooled, len(ks)))
        d.mkdir()
        with open(d / "case.bin", "wb") as f:
            np.array([3, len(ks), len(model["dens_mean"]), model["means"].shape[0], model["variances"].shape[0]], np.int32).tofile(f)
            for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov"):
                model[k].astype(np.uint32).tofile(f)
            acc.tofile(f)
            add.tofile(f)
            er.combine(acc, add).tofile(f)
        open(d / "want.acc", "wb").write(er.file_bytes(model, acc))
        r = subprocess.run([exe, str(d / "case.bin"), str(d)], capture_output=True, text=True)
        assert r.returncode == 0 and "host_ebw_test: ok" in r.stdout, r.stdout + r.stderr


def gmm_size(model):
    from tests import train_reference
    return train_reference.layout(model)[-1]


# ---------------------------------------------------------------------------------------------------------------- estimate

def statistics(D, pooled, seed, ks=KS, tweak=None):
    """a model, accumulators as a lattice pass would leave them (numerator around the model's means, denominator shifted), the previous set
    (the model) and an i-smoothing set.  tweak "fallback": the previous weight of slot 2 is 0 (log weight = the smallest f64) and its mean's
    denominator outweighs the numerator by more than minimum-icd, so dtWeight + D <= 0 and the previous mean is kept; "clamp": weights_ of
    slot 2 is negative, which no corpus pass of this class leaves (its denominator never reaches weights_) but a hand-made file may"""
    rng = np.random.Generator(np.random.PCG64(seed))
    model = synth.gmm_cart(len(ks), 1, 5, D, seed=seed, pooled=pooled, ks=ks)
    o, acc = er.layout(model), np.zeros(er.layout(model)["size"])
    for k in range(int(model["mix_offsets"][-1])):
        d = int(model["dens_index"][k])
        j, cv = int(model["dens_mean"][d]), int(model["dens_cov"][d])
        for side, base in ((0, "num"), (1, "den")):
            n = int(rng.integers(3, 30))
            w = rng.uniform(0.05, 2.0, n) * (0.7 if side else 1.0)
            x = (model["means"][j] + rng.standard_normal((n, D)) * np.sqrt(model["variances"][cv]) + (0.3 if side else 0)).astype(np.float32).astype(np.float64)
            acc[(o["den_density_weights"] if side else 0) + k] += w.sum()
            acc[o[base + "_mean_weights"] + j] += w.sum()
            acc[o[base + "_cov_weights"] + cv] += w.sum()
            acc[o[base + "_mean_sums"] + j * D:][:D] += (w[:, None] * x).sum(0)
            acc[o[base + "_cov_sums"] + cv * D:][:D] += (w[:, None] * x * x).sum(0)
    if tweak == "fallback":
        model["log_weight"] = model["log_weight"].copy()
        model["log_weight"][2] = er.F64_MIN
        acc[o["den_mean_weights"] + int(model["dens_mean"][model["dens_index"][2]])] += 200.0
    if tweak == "clamp":
        acc[2] = -3.0
    ism = dict(model, log_weight=np.log(np.concatenate([rng.dirichlet(np.ones(k)) for k in ks])),
               means=(model["means"] + rng.standard_normal(model["means"].shape).astype(np.float32) * np.float32(0.1)).astype(np.float32),
               variances=(model["variances"] * rng.uniform(0.8, 1.2, model["variances"].shape)).astype(np.float32))
    return model, acc, ism


ESTIMATE_CASES = [(3, False, False, {}), (3, True, False, dict(sigma_minimum=0.2)),
                  (5, False, True, dict(i_smoothing_means=3.0, i_smoothing_weights=2.0)),
                  (5, True, True, dict(i_smoothing_means=30.0, i_smoothing_weights=20.0, min_relative_weight=0.05)),
                  (4, True, False, dict(type="local-rwth", min_observation_weight=12.0)),
                  (2, False, True, dict(i_smoothing_means=1.0, i_smoothing_weights=0.5, min_variance=0.8, normalize_mixture_weights=False,
                                        number_of_iterations=3, min_observation_weight=0.0)),
                  (4, False, False, dict(min_observation_weight=1e9)),            # removal down to one density per mixture
                  (3, True, False, dict(min_observation_weight=0.0), "fallback"), (3, True, False, dict(min_observation_weight=0.0), "clamp")]


def library_estimate(model, acc, ism, cfg, contract):
    import rasr_amd
    kw = dict(cfg)
    for a, b in (("min_observation_weight", "minimum_observation_weight"), ("min_relative_weight", "minimum_relative_weight"), ("min_variance", "minimum_variance")):
        if a in kw:
            kw[b] = kw.pop(a)
    return rasr_amd.EbwEstimator(contract=contract, **kw).estimate(model, acc, model, ism)


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("case", range(len(ESTIMATE_CASES)))
def test_library_estimate_equals_the_restatement_in_every_bit(case, contract):
    D, pooled, use_ism, cfg = ESTIMATE_CASES[case][:4]
    for seed in (20, 21):
        model, acc, ism = statistics(D, pooled, seed, tweak=(ESTIMATE_CASES[case] + (None,))[4])
        want = er.estimate(model, acc, model, ism if use_ism else None, cfg, contract)
        new, info = library_estimate(model, acc, ism if use_ism else None, cfg, contract)
        for k in ("mix_offsets", "dens_index", "dens_mean", "dens_cov"):
            assert np.array_equal(new[k], want["model"][k]), k
        assert np.array_equal(bits(new["log_weight"]), bits(want["model"]["log_weight"]))
        assert new["means"].tobytes() == want["model"]["means"].tobytes() and new["variances"].tobytes() == want["model"]["variances"].tobytes()
        assert np.array_equal(bits(info["iteration_constants"]), bits(want["icd"])) and info["sigma_minimum"] == want["sigma_minimum"]
        assert info["i_smoothing_objective"] == (want["i_objective"] if use_ism else 0.0)
        assert (info["n_removed"], info["n_clamped"], info["n_mean_fallback"], info["n_floored"]) == \
            (len(want["removed"]), len(want["clamped"]), len(want["fallback"]), len(want["floored"]))
        if cfg.get("min_observation_weight") == 1e9:
            assert list(np.diff(new["mix_offsets"])) == [1] * len(KS) and info["n_removed"] == sum(KS) - len(KS)
        # the new set makes a scorer's model: weights normalised, variances positive
        assert (new["variances"] > 0).all() and np.isfinite(new["means"]).all()
        tweak = (ESTIMATE_CASES[case] + (None,))[4]
        assert tweak != "fallback" or info["n_mean_fallback"] >= 1
        assert tweak != "clamp" or info["n_clamped"] >= 1


def test_every_planted_defect_of_the_estimate_leaves_the_bits():
    hit = {d: 0 for d in er.ESTIMATE_DEFECTS}
    for D, pooled, use_ism, cfg in [c[:4] for c in ESTIMATE_CASES[:6]]:
        model, acc, ism = statistics(D, pooled, 20)
        good = er.estimate(model, acc, model, ism if use_ism else None, cfg)
        for d in er.ESTIMATE_DEFECTS:
            bad = er.estimate(model, acc, model, ism if use_ism else None, cfg, defect=d)
            same = all(np.asarray(bad["model"][k]).tobytes() == np.asarray(good["model"][k]).tobytes() for k in ("log_weight", "means", "variances", "dens_index"))
            hit[d] += not (same and np.array_equal(bits(bad["icd"]), bits(good["icd"])))
    assert all(v > 0 for v in hit.values()), hit


def test_estimate_refusals_return_their_code_and_write_nothing():
    import ctypes as C

    import rasr_amd
    from rasr_amd import _lib
    model, acc, ism = statistics(3, False, 20)

    def refused(status, match, mdl=model, a=acc, prev=None, i=None, **kw):
        with pytest.raises(rasr_amd.AmxError, match=match) as e:
            rasr_amd.EbwEstimator(**kw).estimate(mdl, a, mdl if prev is None else prev, i)
        assert e.value.status == status
        with pytest.raises(er.Refused) as r:
            er.estimate(mdl, a, mdl if prev is None else prev, i, {k: v for k, v in kw.items() if k in er.ESTIMATE_DEFAULTS})
        assert r.value.kind == ("unsupported" if status == _lib.AMX_ERR_UNSUPPORTED else "invalid")

    refused(_lib.AMX_ERR_UNSUPPORTED, "cambridge", type="cambridge")
    refused(_lib.AMX_ERR_UNSUPPORTED, "local-rwth: the densities of mixture", type="local-rwth")     # one covariance per density
    shared = dict(model, dens_index=model["dens_index"].copy())
    shared["dens_index"][1] = shared["dens_index"][0]                                                  # mixture 1's first density is mixture 0's
    refused(_lib.AMX_ERR_UNSUPPORTED, "density 0 is shared by mixtures 0 and 1", mdl=shared)
    tied = dict(model, dens_mean=model["dens_mean"].copy())
    tied["dens_mean"][1] = 0
    refused(_lib.AMX_ERR_UNSUPPORTED, "mean 0 is shared by densities 0 and 1", mdl=tied)
    bad = acc.copy()
    bad[7] = np.nan
    refused(_lib.AMX_ERR_INVALID, "entry 7 of the accumulator is not finite", a=bad)
    with pytest.raises(rasr_amd.AmxError, match="Rprop") as e:
        rasr_amd.EbwEstimator(estimator="rprop").estimate(model, acc, model)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    with pytest.raises(rasr_amd.AmxError, match="viterbi") as e:
        rasr_amd.EbwEstimator(viterbi=False).estimate(model, acc, model)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED
    other = dict(model, dens_cov=model["dens_cov"][::-1].copy())
    with pytest.raises(rasr_amd.AmxError, match="previous mixture set differs in topology") as e:
        rasr_amd.EbwEstimator().estimate(model, acc, other)
    assert e.value.status == _lib.AMX_ERR_INVALID
    # a denominator that outweighs the numerator everywhere: the summed weight of a covariance is not positive, the reference's verify
    o, neg = er.layout(model), acc.copy()
    neg[o["den_mean_weights"]:o["den_mean_sums"]] = 1e6
    refused(_lib.AMX_ERR_INVALID, "not positive", a=neg, minimum_icd=0.0, step_size=1e-12, min_observation_weight=0.0)
    # nothing is handed out by a refused call
    keep, h = [], C.c_void_p(123)
    st = rasr_amd._gmm_struct(model, 1.0, 1.0, keep)
    cfg = _lib.EbwEstimateCfg()
    _lib.lib().amx_ebw_estimate_cfg_default(C.byref(cfg))
    cfg.iteration_constants = _lib.AMX_EBW_IC_CAMBRIDGE
    assert _lib.lib().amx_ebw_estimate(C.byref(st), acc.ctypes.data, C.byref(st), None, C.byref(cfg), C.byref(h), None, None) == _lib.AMX_ERR_UNSUPPORTED
    assert h.value is None


@pytest.mark.parametrize("contract", ["off", "fma"])
def test_estimate_against_the_reference_text(contract):
    """ref_ebw.npz: Mm/IterationConstants.cc and the estimators' estimate functions compiled in both builds on ESTIMATE_CASES.  Given the
    walks of the reference's hash tables the restatement is the reference in every bit; the library (ascending index) is too where every
    density has its own covariance, and stays within bar (b), measured by the generator, where a covariance is shared"""
    import json
    reached = json.loads(str(Z["estimate_reached"]))
    assert all(reached[k] > 0 for k in ("clamped", "fallback", "removed", "dk_above_default", "xi_branch", "floored")), reached
    assert float(Z["bar_b"]) == 4.0 * float(Z["bar_b_measured"])
    for n, case in enumerate(ESTIMATE_CASES):
        D, pooled, use_ism, cfg = case[:4]
        for seed in (20, 21):
            name = "estimate/%d/%d/%s/" % (n, seed, contract)
            assert json.loads(str(Z["estimate/%d/%d/cfg" % (n, seed)])) == cfg
            model, acc, ism = statistics(D, pooled, seed, tweak=(case + (None,))[4])
            walk, dens, means = (Z[name + k] for k in ("cov_walk", "dens_walk", "mean_walk"))
            orders = dict(cov_walk=list(walk), cov_densities={int(cv): [int(d) for d in dens if int(model["dens_cov"][d]) == cv] for cv in walk},
                          cov_means={int(cv): [int(j) for j in means if int(model["dens_cov"][list(model["dens_mean"]).index(j)]) == cv] for cv in walk})
            mine = er.estimate(model, acc, model, ism if use_ism else None, cfg, contract, orders=orders)
            for k in ("mix_offsets", "dens_index", "log_weight", "means", "variances"):
                assert np.asarray(mine["model"][k]).tobytes() == Z[name + k].tobytes(), (name, k)
            assert np.array_equal(bits(mine["icd"]), bits(Z[name + "icd"]))
            assert not use_ism or mine["i_objective"] == float(Z[name + "i_objective"])
            new, info = library_estimate(model, acc, ism if use_ism else None, cfg, contract)
            if not pooled:
                assert new["means"].tobytes() == Z[name + "means"].tobytes() and new["variances"].tobytes() == Z[name + "variances"].tobytes()
                assert np.array_equal(bits(new["log_weight"]), bits(Z[name + "log_weight"])) and np.array_equal(bits(info["iteration_constants"]), bits(Z[name + "icd"]))
            else:
                for a, b in ((new["means"], Z[name + "means"]), (new["variances"], Z[name + "variances"]), (info["iteration_constants"], Z[name + "icd"]),
                             (np.exp(new["log_weight"]), np.exp(Z[name + "log_weight"]))):
                    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
                    assert float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) <= float(Z["bar_b"]), name
            assert np.array_equal(new["dens_index"], Z[name + "dens_index"]) and np.array_equal(new["mix_offsets"], Z[name + "mix_offsets"])
