#!/usr/bin/env python3
"""tools/segclust_probe.py -- the segment clustering at the size of a speaker-adaptive training corpus: 2048 segments of 300 frames,
D = 16 and D = 45, concatenation and max linkage.

    python3 tools/segclust_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                                    at the first step that fails; the children's JSON lines go to profiles/segclust_probe.jsonl
    python3 tools/segclust_probe.py --step NAME     one step; prints one JSON line

Times are wall times of whole calls (median of --reps after a warm-up call, the stream drained) and, from a further call with the library's
event timers on, the time of each kernel group: acc, finalize, pack, the two matrix products, the rows kernel, the merge loop."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("d16", "d45", "d16_maxlinkage")
KERNELS = ("segclust_acc", "segclust_finalize", "segclust_pack", "segclust_r_gemm", "segclust_rows", "segclust_dist_gemm", "segclust_loop")


def step(a):
    import torch

    import rasr_amd
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    D, N, per = (45 if a.step == "d45" else 16), a.segments, a.frames
    rng = np.random.Generator(np.random.PCG64(31))
    speakers = rng.standard_normal((a.speakers, D)) * 2.0
    x = (rng.standard_normal((N, per, D)) * rng.uniform(0.5, 1.5, D) + speakers[rng.integers(0, a.speakers, N)][:, None, :]).astype(np.float32)
    xd = torch.from_numpy(x.reshape(N * per, D)).cuda()
    off = np.arange(N + 1, dtype=np.int64) * per
    sc = rasr_amd.SegmentClustering(ctx, D, amalgamation=1 if a.step == "d16_maxlinkage" else 0)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        v = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(v)), 3)

    def accumulate():
        sc.reset()
        sc.accumulate_dev(xd, off)

    K = D * (D + 1) // 2
    res = dict(step=a.step, dim=D, segments=N, frames=N * per, reps=a.reps, kernel_shape=sc.kernel_shape(),
               r_gemm_f64_flop=2 * N * N * (K + D + 1), dist_gemm_f32_flop=N * N * N)
    res["accumulate_ms"] = timed(accumulate, a.reps)
    res["cluster_ms"] = timed(sc.cluster, a.reps)
    ctx.profile(True)
    ctx.profile_reset()
    accumulate()
    out = sc.cluster()
    torch.cuda.synchronize()
    for k in KERNELS:
        ms, n = ctx.profile_get(k)
        res[k + "_ms"], res[k + "_calls"] = round(ms, 3), n
    ctx.profile(False)
    res.update(alpha=out["alpha"], alpha_iterations=out["alpha_iterations"], n_clusters=out["n_clusters"], n_regularised=out["n_regularised"],
               speakers=a.speakers, merges_per_s=round((N - 1) / (res["segclust_loop_ms"] * 1e-3), 0) if res["segclust_loop_ms"] > 0 else None)
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--segments", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=300, help="per segment")
    ap.add_argument("--speakers", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segclust_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--segments", str(a.segments), "--frames",
               str(a.frames), "--speakers", str(a.speakers), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("segclust_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(l) for l in lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
