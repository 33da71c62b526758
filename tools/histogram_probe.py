#!/usr/bin/env python3
"""tools/histogram_probe.py -- histogram normalisation on one config-5 shard step: 63 936 frames x 40 components, data resident, at the
estimator's default bucket size 0.0002 (every window far wider than the LDS threshold: atomics on memory) and at 0.01 (windows of a
few hundred buckets: what fits counts in LDS, see the paths printed).  HIP-event time with a synchronise, `--reps` rounds of `--iters`
calls each after a warm-up; prints the median and the spread (min .. max) of the per-round means of
  copy        a plain device copy of the same bytes (the yardstick: both kernels read, apply also writes, every byte once)
  accumulate  amx_histogram_accumulate_dev into a handle that already holds the window (no growth): range kernel, the synchronisation
              that brings 2 dim + 1 integers to the host, count kernel
  apply       amx_histnorm_apply_dev in place over 64 segments of 8 keys, without the clamped counters (no synchronisation)
then the split between the kernels from the library's own per-kernel events (amx_profile_get), the cost of the synchronisation per
accumulate call (the call's time minus its two kernels), and one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, default=63936)
    ap.add_argument("--dim", type=int, default=40)
    a = ap.parse_args()
    import torch

    import rasr_amd
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    T, dim, n_keys, n_seg = a.frames, a.dim, 8, 64
    rng = np.random.Generator(np.random.PCG64(9))
    x_host = (rng.standard_normal((T, dim)) * rng.uniform(0.5, 1.5, dim)).astype(np.float32)
    x = torch.from_numpy(x_host).cuda()
    y = torch.empty_like(x)
    offsets = np.linspace(0, T, n_seg + 1).astype(np.int64)
    seg_keys = np.arange(n_seg) % n_keys
    forms, res = {"copy": lambda: y.copy_(x)}, {"frames": T, "dim": dim, "reps": a.reps, "iters": a.iters, "keys": n_keys, "segments": n_seg}
    keep = []
    for bs in (0.0002, 0.01):
        tag = "bs%g" % bs
        est = rasr_amd.HistogramEstimator(ctx, dim, bs)
        est.accumulate_dev(x, dim, T)   # the window is there from now on
        before = est.describe()
        est.accumulate_dev(x, dim, T)
        after = est.describe()
        res[tag + "_paths"] = {"lds": after["n_lds"] - before["n_lds"], "global": after["n_global"] - before["n_global"],
                               "buckets": int(sum(est.table(d)[2].size for d in range(dim)))}
        print("%s: %s" % (tag, res[tag + "_paths"]))
        norm = rasr_amd.HistogramNormalization(ctx, [est])
        for k in range(n_keys):
            key = rasr_amd.HistogramEstimator(ctx, dim, bs)
            key.accumulate_dev(x[k::n_keys].contiguous(), dim, len(x[k::n_keys]))
            norm.add_key(key)
        z = x.clone()
        keep += [est, norm, z]
        forms[tag + "_accumulate"] = (lambda est=est: est.accumulate_dev(x, dim, T))
        forms[tag + "_apply"] = (lambda norm=norm, z=z: norm.apply_dev(offsets, seg_keys, z, dim, z, dim, count_clamped=False))
    times = {k: [] for k in forms}
    for f in forms.values():   # warm-up
        f()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, f in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                f()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / a.iters)
    for k, v in times.items():
        v = np.array(v)
        res[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}
        print("%-22s median %.4f ms  spread %.4f .. %.4f ms" % (k, np.median(v), v.min(), v.max()))
    # the split between the kernels: the library's per-kernel events, a round of their own (the events serialise the launches)
    ctx.profile(True)
    for k, f in forms.items():
        if k == "copy":
            continue
        ctx.profile_reset()
        for _ in range(a.iters):
            f()
        torch.cuda.synchronize()
        for name in (("hist_range", "hist_count") if k.endswith("accumulate") else ("histnorm_apply",)):
            res[k][name + "_ms"] = round(ctx.profile_get(name)[0], 4)
        if k.endswith("accumulate"):
            res[k]["synchronisation_ms"] = round(res[k]["median_ms"] - res[k]["hist_range_ms"] - res[k]["hist_count_ms"], 4)
        print("%-22s %s" % (k, {n: v for n, v in res[k].items() if n.endswith("_ms") and n not in ("median_ms", "min_ms", "max_ms")}))
    ctx.profile(False)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
