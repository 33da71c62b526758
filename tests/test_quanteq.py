"""CPU: quantile equalisation without a device -- the restatement (tests/quanteq_reference.py) against the fixture that the reference's own
text produced in both of its builds (tests/golden/make_quanteq_golden.py), and the library's host side (grid tables, quantile files,
pooling, refusals) against the restatement and the fixture.  No kernel runs here; tests/test_quanteq_gpu.py holds the device parity."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import quanteq_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_quanteq.npz")
BUILDS = ("off", "fma")
INT_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def config_names(estimate=False):
    fx = fixture()
    return [k[4:] for k in fx if k.startswith("cfg/") and bool(config(k[4:])[1]["estimate"]) == estimate]


@functools.lru_cache(maxsize=None)
def config(name):
    fx = fixture()
    c = dict(zip([str(s) for s in fx["cfg_fields"]], fx["cfg/" + name].tolist()))
    dim = int(c.pop("dim"))
    for k in ("quantiles", "combination", "estimate", "mean", "variance", "nq", "pool"):
        c[k] = int(c[k])
    return dim, c


def recorded(build, key):
    """the array of one build: the fma copy is kept only where its bits differ"""
    fx = fixture()
    return fx[build + "/" + key] if build + "/" + key in fx else fx["off/" + key]


def segments(name):
    fx = fixture()
    off = np.concatenate([[0], np.cumsum(fx["lengths/" + name])])
    return [fx["in/" + name][off[s]:off[s + 1]] for s in range(len(off) - 1)], off


def training(name):
    """the training quantiles as the reference's object read them from its file"""
    dim, c = config(name)
    return recorded("off", name + "/training_quantiles")


def same(a, b):
    """equal in every bit; a NaN matches a NaN in the same place (the two builds give NaNs of different sign)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    eq = a.view(u) == b.view(u)
    if a.dtype.kind == "f":
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())


def differing(a, b):
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return int(((a.view(u) != b.view(u)) & ~(np.isnan(a) & np.isnan(b))).sum())


@functools.lru_cache(maxsize=None)
def restated(name, build, variant=()):
    """the restatement of every segment of a configuration (shared by the tests below, never changed)"""
    dim, c = config(name)
    xs, _ = segments(name)
    return [R.equalize(x, training(name), c, build == "fma", variant) for x in xs]


def test_the_fixture_can_tell_the_readings_apart():
    """asserted before anything is compared: each wrong reading changes at least one recorded parameter (d20 holds ordinary segments, a
    constant one, a quantised one and the one-frame segment), pooling changes the training quantiles, and the builds differ"""
    fx = fixture()
    want = np.stack([recorded("off", "d20/params")])[0]
    for variant in ("last_minimum", "linear_grid", "powf"):
        got = np.stack([r["params"] for r in restated("d20", "off", (variant,))])
        assert differing(got[:, :2], want[:, :2]) > 0, "%s changes no alpha or gamma of the fixture" % variant
    got = np.stack([r["params"] for r in restated("d20_cv", "off", ("last_minimum",))])
    assert differing(got[:, 2:4], recorded("off", "d20_cv/params")[:, 2:4]) > 0, "last_minimum changes no lambda or rho"
    got = np.stack([r["params"] for r in restated("d20", "off", ("newest_first",))])
    assert differing(got[:, 4], want[:, 4]) > 0, "newest-first sums change no mean bit"
    dim, c = config("d20_unpooled")
    text = fx["training_file/d20_unpooled"].tobytes()
    assert differing(R.read_quantile_file(text, dim, c["nq"], 1), R.read_quantile_file(text, dim, c["nq"], 0)) > 0
    assert same(R.read_quantile_file(text, dim, c["nq"], 0), fx["off/d20_unpooled/training_quantiles_check"])
    assert int(fx["fma_instructions/off"]) == 0 and int(fx["fma_instructions/fma"]) > 0
    assert "d20/params" in [str(s) for s in fx["fma_differs"]]
    last = len(fx["lengths/d20"]) - 1     # the one-frame segment that was searched for
    assert fx["lengths/d20"][last] == 1
    assert differing(fx["fma/d20/params"][last, :2], fx["off/d20/params"][last, :2]) > 0, "the builds agree on the one-frame segment"


def test_fused_operations_are_libm_s():
    """the vectorised fmaf / fma of the restatement against libm's through ctypes: random operands, near-cancellation, halfway cases"""
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.normal(0, 1, 4000).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, 4000).astype(np.float32)
    b = rng.normal(0, 1, 4000).astype(np.float32)
    c = np.where(rng.random(4000) < 0.5, -(a * b), rng.normal(0, 1, 4000)).astype(np.float32)   # half of them cancel
    c[:100] = np.float32(2.0 ** 24)
    a[:100], b[:100] = np.float32(1.0), (1.0 + rng.integers(0, 4, 100) * 0.5).astype(np.float32)   # sums on and beside a halfway point
    got = R.fmaf(a, b, c)
    want = np.array([R.libm_fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)
    assert same(got, want)
    assert differing(got, (a * b + c).astype(np.float32)) > 0          # and they are not the two-rounding result
    a64 = a.astype(np.float64) * (1 + rng.random(4000) * 1e-9)
    b64 = b.astype(np.float64) * (1 + rng.random(4000) * 1e-9)
    c64 = np.where(rng.random(4000) < 0.5, -(a64 * b64), rng.normal(0, 1, 4000))
    got = R.fma(a64, b64, c64)
    want = np.array([R.libm_fma(x, y, z) for x, y, z in zip(a64.tolist(), b64.tolist(), c64.tolist())], np.float64)
    assert same(got, want)
    assert differing(got, a64 * b64 + c64) > 0


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", config_names())
def test_restatement_equals_the_fixture(name, build):
    got = restated(name, build)
    _, off = segments(name)
    for s, r in enumerate(got):
        assert same(r["params"], recorded(build, name + "/params")[s]), (name, build, s, "alpha gamma lambda rho mean deviation")
        assert same(r["cq_after"], recorded(build, name + "/cq_after")[s]), (name, build, s, "quantiles after the search")
        assert same(r["out"], recorded(build, name + "/out")[off[s]:off[s + 1]]), (name, build, s, "output")
        # the first and the last quantile are never replaced
        assert same(r["quantiles"][[0, -1]], r["cq_after"][[0, -1]])


def host_handle(dim, tq=None, **kw):
    return rasr_amd.QuantileEqualization(None, dim, tq, **kw)


def test_grid_tables():
    """the tables are what the reference's f32 loop variable visits with an f64 step that went through an f32 setter"""
    h = host_handle(3, np.zeros((5, 3), np.float32))
    ga, gg, gl = R.grids(R.DEFAULTS)
    assert len(ga) == 201 and len(gg) == 201 and len(gl) == 101
    assert ga[-1] == np.float32(0.9999992) and gg[-1] == np.float32(2.999998)
    assert same(h.grid("alpha"), ga) and same(h.grid("gamma"), gg) and same(h.grid("lambda"), gl) and same(h.grid("rho"), gl)
    assert differing(ga, R.grid(0.0, 1.0, 0.005, linear=True)) > 0
    h = host_handle(3, np.zeros((5, 3), np.float32), delta_alpha=0.1, delta_gamma=0.25, delta_lambda_and_rho=0.125)
    c = dict(R.DEFAULTS, delta_alpha=0.1, delta_gamma=0.25, delta_lr=0.125)
    for which, want in zip(("alpha", "gamma", "lambda"), R.grids(c)):
        assert same(h.grid(which), want)
    assert len(h.grid("gamma")) == 9 and len(h.grid("lambda")) == 5     # exact steps reach the upper end


def test_quantile_files(tmp_path):
    """the writer's bytes are fprintf's; the reader and the pooling give the bits the reference's object read"""
    fx = fixture()
    for name in config_names(estimate=True):
        dim, c = config(name)
        p = str(tmp_path / (name + ".txt"))
        rasr_amd.write_quantiles(p, fx["off/" + name + "/sums"], int(fx["off/" + name + "/count"]))
        with open(p, "rb") as f:
            assert f.read() == fx["off/" + name + "/file"].tobytes(), name
    for name in config_names():
        dim, c = config(name)
        if not c["quantiles"]:
            continue
        p = str(tmp_path / (name + ".txt"))
        with open(p, "wb") as f:
            f.write(fx["training_file/" + name].tobytes())
        got = rasr_amd.read_quantiles(p, dim, c["nq"], pool=bool(c["pool"]))
        assert same(got, training(name)), name
        assert same(got, R.read_quantile_file(fx["training_file/" + name].tobytes(), dim, c["nq"], c["pool"])), name
    p = str(tmp_path / "d20_unpooled.txt")
    assert differing(rasr_amd.read_quantiles(p, 20, 4, pool=True), rasr_amd.read_quantiles(p, 20, 4, pool=False)) > 0
    with pytest.raises(rasr_amd.AmxError, match="Can't open training quantile file") as e:
        rasr_amd.read_quantiles(str(tmp_path / "missing.txt"), 20, 4)
    assert e.value.status == _lib.AMX_ERR_INVALID
    with pytest.raises(rasr_amd.AmxError, match="does not hold"):
        rasr_amd.read_quantiles(p, 21, 4)


def test_estimated_sums_and_file_of_the_restatement():
    """the estimator's arithmetic: quantiles added in f64 in segment order, one count per segment, in any split"""
    fx = fixture()
    for name in config_names(estimate=True):
        dim, c = config(name)
        xs, _ = segments(name)
        sums, count = R.estimate(xs, c["nq"])
        assert same(sums, fx["off/" + name + "/sums"]) and count == int(fx["off/" + name + "/count"]) == len(xs)
        assert R.write_quantile_file(sums, count) == fx["off/" + name + "/file"].tobytes()
        for cut in range(len(xs) + 1):      # a sum carried over a split is the same chain
            a, n = R.estimate(xs[:cut], c["nq"])
            for x in xs[cut:]:
                a = (np.zeros_like(sums) if a is None else a) + R.quantiles(x, c["nq"]).astype(np.float64)
            assert same(a, sums)


def test_create_refuses_what_is_not_built():
    tq = np.zeros((5, 3), np.float32)
    for kw, word in ((dict(length=100), "length"), (dict(right=5), "right"), (dict(length=100, right=50), "sliding window"),
                     (dict(piecewise_linear=1), "piecewise_linear"), (dict(delta_alpha=0.0), "delta_alpha"), (dict(delta_gamma=-0.01), "delta_gamma"),
                     (dict(delta_lambda_and_rho=0.0), "delta_lambda_and_rho"), (dict(delta_alpha=1e-5), "delta_alpha"),
                     (dict(delta_gamma=1e-4), "delta_gamma"), (dict(number_of_quantiles=0), "number_of_quantiles"),
                     (dict(number_of_quantiles=_lib.AMX_QUANTEQ_MAX_QUANTILES + 1), "number_of_quantiles")):
        with pytest.raises(rasr_amd.AmxError, match=word) as e:
            host_handle(3, None if "number_of_quantiles" in kw else tq, **kw)
        assert e.value.status == _lib.AMX_ERR_UNSUPPORTED, kw
    host_handle(3, np.zeros((17, 3), np.float32), number_of_quantiles=16)      # the documented bound itself works
    with pytest.raises(rasr_amd.AmxError, match="training_quantiles") as e:
        host_handle(3, None)
    assert e.value.status == _lib.AMX_ERR_INVALID
    host_handle(3, None, quantiles=0)
    with pytest.raises(ValueError, match="shape"):
        host_handle(3, np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError, match="unknown parameter"):
        host_handle(3, tq, numberOfQuantiles=4)
    # a handle without a context cannot run
    h = host_handle(3, tq)
    off = np.array([0, 1], np.int64)
    x = np.zeros((1, 3), np.float32)
    with pytest.raises(rasr_amd.AmxError) as e:
        h.apply_dev(off, x, 3, x, 3)
    assert e.value.status == _lib.AMX_ERR_STATE
    est = rasr_amd.QuantileEstimator(None, 3)
    sums, count = est.result()
    assert count == 0 and not sums.any() and sums.shape == (5, 3)
    with pytest.raises(rasr_amd.AmxError) as e:
        est.accumulate_dev(off, x, 3)
    assert e.value.status == _lib.AMX_ERR_STATE
    L = _lib.lib()
    cfg = _lib.QuanteqCfg()
    L.amx_quanteq_default_cfg(C.byref(cfg))
    assert (cfg.quantiles, cfg.combination, cfg.estimate, cfg.mean, cfg.variance, cfg.number_of_quantiles, cfg.pool_quantiles, cfg.piecewise_linear) == \
        (1, 0, 0, 1, 0, 4, 1, 0)
    assert (cfg.overestimation_factor, cfg.delta_alpha, cfg.delta_gamma, cfg.delta_lambda_and_rho, cfg.beta) == \
        (1.0, np.float32(0.005), np.float32(0.01), np.float32(0.005), np.float32(0.05))
    assert cfg.length == INT_MAX and cfg.right == INT_MAX


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_quanteq_test.cc compiles the handle's host side (grids, files, pooling, refusals) into a program of its own; built with
    -fsanitize=address,undefined on the host side only, run as a process of its own (nothing sanitized is loaded into Python).
    Sanitizers are for machines without a GPU: where one is present the same program is built and run plainly."""
    import subprocess

    import torch
    exe = str(tmp_path / "host_quanteq_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(ROOT, "tests", "host_quanteq_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "host_quanteq_test: ok" in r.stdout, r.stdout + r.stderr
