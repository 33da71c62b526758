#!/usr/bin/env python3
"""tools/scatter_probe.py -- the LDA scatter-matrix pass on one config-5 shard step: 63 936 frames, context windows of 9 x 16 = 144 and
11 x 40 = 440 components, 10 000 classes, an alignment in runs, data resident.  HIP-event time of amx_scatter_accumulate_dev (both
kernels) with a synchronise, `--reps` rounds of `--iters` launches each after a warm-up; prints the median and the spread
(min .. max) of the per-round means per form, the split between the two kernels from the library's own per-kernel events
(amx_profile_get), the share of an unverified floor (the four operations per triangle entry and frame -- two f32 multiplies, the widening, the f64 add --
at the datasheet's 78.6 T f64 vector operations per second: 0.32 ms at dim 440) and the bytes the square-sum kernel adds with
atomics (blocks x chunks x 32 KB, from the launch geometry restated here); one JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS_PER_S, OPS_PER_ENTRY = 78.6e12, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, default=63936)
    ap.add_argument("--classes", type=int, default=10000)
    a = ap.parse_args()
    import torch

    import rasr_amd
    from tests import scatter_reference as sr
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    T = a.frames
    cls = torch.from_numpy(sr.alignment(T, a.classes, "runs", 7, skip_every=0).view(np.int32)).cuda()
    rng = np.random.Generator(np.random.PCG64(8))
    w = torch.from_numpy(rng.uniform(0.5, 1.0, T).astype(np.float32)).cuda()
    forms, info = {}, {}
    for dim in (144, 440):
        est = rasr_amd.ScatterMatricesEstimator(ctx, dim, a.classes)
        x = torch.from_numpy(rng.standard_normal((T, dim)).astype(np.float32)).cuda()
        acc = torch.zeros(est.accumulator_size(), dtype=torch.float64, device="cuda")
        forms["dim%d" % dim] = (lambda est=est, x=x, acc=acc, dim=dim: est.accumulate_dev(x, dim, T, cls, acc))
        forms["dim%d_weighted" % dim] = (lambda est=est, x=x, acc=acc, dim=dim: est.accumulate_dev(x, dim, T, cls, acc, w))
        # the launch geometry, RESTATED from amx_scatter_accumulate_dev (scatter.hip: kScatterBlock = kScatterStage = 64, kScatterGroups = 4,
        # the context's CU count) -- the library does not report it, so these figures follow the source by hand
        nb = (dim + 63) // 64
        blocks = nb * (nb + 1) // 2
        want = max(1, -(-4 * n_cu // blocks))
        chunk = -(-(-(-T // want)) // 64) * 64
        chunks = -(-T // chunk)
        info[dim] = dict(blocks=blocks, chunks=chunks, frames_per_chunk=chunk, atomic_bytes=blocks * chunks * 64 * 64 * 8,
                         floor_ms=dim * (dim + 1) // 2 * T * OPS_PER_ENTRY / OPS_PER_S * 1e3)
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
    res = {"frames": T, "classes": a.classes, "reps": a.reps, "iters": a.iters, "n_cu": n_cu}
    for k, v in times.items():
        v = np.array(v)
        res[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}
        print("%-16s median %.4f ms  spread %.4f .. %.4f ms" % (k, np.median(v), v.min(), v.max()))
    # the split between the kernels: the library's per-kernel events, a round of their own (the events serialise the launches)
    ctx.profile(True)
    for k, f in forms.items():
        ctx.profile_reset()
        for _ in range(a.iters):
            f()
        torch.cuda.synchronize()
        res[k]["square_ms"] = round(ctx.profile_get("scatter_square")[0], 4)
        res[k]["class_ms"] = round(ctx.profile_get("scatter_class")[0], 4)
        print("%-16s scatter_square %.4f ms  scatter_class %.4f ms" % (k, res[k]["square_ms"], res[k]["class_ms"]))
    ctx.profile(False)
    for dim, d in info.items():
        d["floor_ms"] = round(d["floor_ms"], 4)
        d["share_of_floor"] = round(d["floor_ms"] / res["dim%d" % dim]["square_ms"], 3)
        d["share_of_floor_weighted"] = round(d["floor_ms"] / res["dim%d_weighted" % dim]["square_ms"], 3)
        res["geometry_dim%d_restated" % dim] = d
        print("dim %d (geometry restated from scatter.hip): %s" % (dim, d))
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
