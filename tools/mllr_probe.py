#!/usr/bin/env python3
"""tools/mllr_probe.py -- the MLLR corpus pass at the size of a speaker-adaptive training shard: D = 45, 64 segments of 1000 frames,
8 keys, 71 regression classes; full and shift, weighted and not; the same call with ONE class, so that the dependence on n_leafs is
on record; and the adapted-means kernel for 160 000 means.

    python3 tools/mllr_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                                at the first step that fails; the children's JSON lines are appended to
                                                profiles/mllr_probe.jsonl
    python3 tools/mllr_probe.py --step NAME     one step; prints one JSON line

Times are wall times of whole calls (median of --reps after a warm-up call, the stream drained) and the kernels' own from the library's
event timers (median of --reps calls)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("full", "full_weighted", "shift", "shift_weighted", "full_one_leaf", "full_weighted_one_leaf", "adapt_full", "adapt_shift")


def step(a):
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    ctx.set_contract(a.contract)
    rng = np.random.Generator(np.random.PCG64(21))
    mode = "shift" if "shift" in a.step else "full"
    D, n_seg, per, n_keys = a.dim, a.segments, a.frames, a.keys
    res = dict(step=a.step, contract=a.contract, dim=D, reps=a.reps, kernel_shape=list(rasr_amd.ModelTransformEstimator.kernel_shape()))

    def median_kernel(fn, names):
        ctx.profile(True)
        got = {n: [] for n in names}
        for _ in range(a.reps):
            ctx.profile_reset()
            fn()
            torch.cuda.synchronize()
            for n in names:
                got[n].append(ctx.profile_get(n)[0])
        ctx.profile(False)
        return {n: round(float(np.median(v)), 4) for n, v in got.items()}

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

    if a.step.startswith("adapt"):
        n_mix = a.means // 4
        model = synth.gmm_cart(n_mix, 4, 4, D, seed=21, pooled=False)
        gmm = rasr_amd.GmmFeatureScorer(ctx, model)
        est = rasr_amd.ModelTransformEstimator(gmm, mode, a.leafs, (np.arange(n_mix) % a.leafs).astype(np.int32), n_keys=1)
        ids = np.arange(a.leafs, dtype=np.int32)
        mats = rng.standard_normal((a.leafs, D) if mode == "shift" else (a.leafs, D, D + 1))
        index = (np.arange(n_mix) % a.leafs).astype(np.int32)
        out = torch.zeros((len(model["means"]), D), dtype=torch.float32, device="cuda")
        adaptor = rasr_amd.MixtureSetAdaptor(est)
        res.update(means=len(model["means"]), matrices=a.leafs)
        res["adapt_call_ms"] = timed(lambda: adaptor.adapt_means_dev(ids, mats, index, out))
        res["kernel_ms"] = median_kernel(lambda: adaptor.adapt_means_dev(ids, mats, index, out), ["mllr_adapt"])
        print(json.dumps(res))
        ctx.close()
        return
    n_leafs = 1 if "one_leaf" in a.step else a.leafs
    n_mix, T = a.mixtures, n_seg * per
    model = synth.gmm_cart(n_mix, 1, 4, D, seed=21, pooled=False)
    gmm = rasr_amd.GmmFeatureScorer(ctx, model)
    est = rasr_amd.ModelTransformEstimator(gmm, mode, n_leafs, (np.arange(n_mix) % n_leafs).astype(np.int32), n_keys=n_keys)
    x = torch.from_numpy((rng.standard_normal((T, D)) * 1.5).astype(np.float32)).cuda()
    off = np.arange(n_seg + 1, dtype=np.int64) * per
    keys = (np.arange(n_seg) % n_keys).astype(np.int32)
    emission = torch.from_numpy(np.repeat(rng.integers(0, n_mix, T // 10 + 1), 10)[:T].astype(np.int32)).cuda()   # runs of ten frames
    weight = torch.from_numpy(rng.uniform(0.05, 2.0, T)).cuda() if "weighted" in a.step else None
    scores = torch.zeros((T, n_mix), dtype=torch.float32, device="cuda")
    best = torch.zeros((T, n_mix), dtype=torch.int32, device="cuda")
    acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
    res.update(mode=mode, segments=n_seg, frames=T, keys=n_keys, leafs=n_leafs, mixtures=n_mix, accumulator_doubles=est.accumulator_size(),
               frames_per_list=round(T / (n_keys * n_leafs), 1))
    res["gmm_score_ms"] = timed(lambda: gmm.score_dev(x, T, scores, best))
    call = lambda: est.accumulate_dev(x, D, off, keys, emission, best, acc, n_mix, weight)   # noqa: E731
    res["mllr_accumulate_ms"] = timed(call)
    res["kernel_ms"] = median_kernel(call, ["mllr_resolve", "mllr_lists", "mllr_acc_" + mode])
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--dim", type=int, default=45)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000, help="per segment")
    ap.add_argument("--keys", type=int, default=8)
    ap.add_argument("--leafs", type=int, default=71)
    ap.add_argument("--mixtures", type=int, default=500)
    ap.add_argument("--means", type=int, default=160000, help="of the adapted-means steps")
    ap.add_argument("--contract", default="fma")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mllr_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--dim", str(a.dim), "--segments",
               str(a.segments), "--frames", str(a.frames), "--keys", str(a.keys), "--leafs", str(a.leafs), "--mixtures", str(a.mixtures), "--means",
               str(a.means), "--contract", a.contract, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("mllr_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    with open(a.out, "a") as f:
        f.write("\n".join(json.dumps(l) for l in lines) + "\n")
    print("appended to %s" % a.out)


if __name__ == "__main__":
    main()
