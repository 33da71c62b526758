#!/usr/bin/env python3
"""tools/cmllr_probe.py -- the CMLLR corpus pass at the size of a speaker-adaptive training shard: F = M = 45, 64 segments of 1000
frames, 8 keys, with a pooled and with per-density covariances; beside it the amx_gmm_score_dev call in front of it and
amx_cart_accumulate_dev on the same frames.

    python3 tools/cmllr_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                                 at the first step that fails; the children's JSON lines go to profiles/cmllr_probe.jsonl
    python3 tools/cmllr_probe.py --step NAME     one step; prints one JSON line

Steps: pooled, full (per-density covariances, the G kernel with its default tile of 16 model components), full_tile48 (the same with 48
components per lane: the shape in which a lane keeps all accumulators of the model), full_one_key (all segments of one key: the
smallest grid).

Times are wall times of whole calls (median of --reps, the stream drained) and the kernels' own from the library's event timers."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("pooled", "full", "full_tile48", "full_one_key")


def step(a):
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    ctx.set_contract(a.contract)
    rng = np.random.Generator(np.random.PCG64(21))
    D, n_seg, per, n_keys, n_mix = a.dim, a.segments, a.frames, (1 if a.step == "full_one_key" else a.keys), a.mixtures
    T = n_seg * per
    model = synth.gmm_cart(n_mix, 1, 4, D, seed=21, pooled=a.step == "pooled")
    gmm = rasr_amd.GmmFeatureScorer(ctx, model)
    est = rasr_amd.AffineFeatureTransformEstimator(gmm, D, n_keys)
    if a.step == "full_tile48":
        est.set_tile(48)
    x = torch.from_numpy((rng.standard_normal((T, D)) * 1.5).astype(np.float32)).cuda()
    off = np.arange(n_seg + 1, dtype=np.int64) * per
    keys = (np.arange(n_seg) % n_keys).astype(np.int32)
    emission = torch.from_numpy(np.repeat(rng.integers(0, n_mix, T // 10 + 1), 10)[:T].astype(np.int32)).cuda()   # runs of ten frames
    scores = torch.zeros((T, n_mix), dtype=torch.float32, device="cuda")
    best = torch.zeros((T, n_mix), dtype=torch.int32, device="cuda")
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    cart = rasr_amd.CartExampleAccumulator(ctx, n_mix, D)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        v = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(v)), 3)

    res = dict(step=a.step, contract=a.contract, dim=D, segments=n_seg, frames=T, keys=n_keys, mixtures=n_mix, reps=a.reps,
               accumulator_doubles=est.accumulator_size(), kernel_shape=list(est.kernel_shape()))
    res["gmm_score_ms"] = timed(lambda: gmm.score_dev(x, T, scores, best))
    res["cart_accumulate_ms"] = timed(lambda: cart.accumulate(x, emission))
    res["cmllr_accumulate_ms"] = timed(lambda: est.accumulate_dev(x, D, off, keys, emission, best, acc, n_mix))
    ctx.profile(True)
    ctx.profile_reset()
    est.accumulate_dev(x, D, off, keys, emission, best, acc, n_mix)
    torch.cuda.synchronize()
    res["cmllr_small_kernel_ms"] = round(ctx.profile_get("cmllr_small")[0], 3)
    if a.step != "pooled":
        g_ms = ctx.profile_get("cmllr_g")[0]
        divisions = T * D * (D + 1) * (D + 2) // 2
        res["cmllr_g_kernel_ms"] = round(g_ms, 3)
        res["g_f64_divisions"] = divisions
        res["g_divisions_per_s"] = round(divisions / (g_ms * 1e-3), 0) if g_ms > 0 else None
    ctx.profile(False)
    host = acc.cpu().numpy()
    res["beta_key0"] = float(host[0])
    t0 = time.perf_counter()
    est.estimate(host, 0, iterations=10, min_observation_weight=100.0)
    res["host_estimate_10_iterations_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--dim", type=int, default=45)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000, help="per segment")
    ap.add_argument("--keys", type=int, default=8)
    ap.add_argument("--mixtures", type=int, default=500)
    ap.add_argument("--contract", default="fma")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmllr_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--dim", str(a.dim), "--segments",
               str(a.segments), "--frames", str(a.frames), "--keys", str(a.keys), "--mixtures", str(a.mixtures), "--contract", a.contract, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("cmllr_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(l) for l in lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
