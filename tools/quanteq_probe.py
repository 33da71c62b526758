#!/usr/bin/env python3
"""tools/quanteq_probe.py -- quantile equalisation of 64 segments x 1000 frames x 20 and x 40 channels, data resident, with and without
the neighbour combination, next to a device copy of the matrix (the yardstick) and to the time the reference's own text takes for one
such segment on a CPU (cpu_seconds_per_segment of tests/golden/ref_quanteq.npz, measured by tests/golden/make_quanteq_golden.py).

    python3 tools/quanteq_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that
                                                   stops at the first step that fails; the children's JSON lines go to profiles/quanteq_probe.jsonl
    python3 tools/quanteq_probe.py --step NAME     one step: HIP-event time of amx_quanteq_apply_dev (mean and variance normalisation on, the
                                                   parameters not read back), `--reps` rounds of `--iters` calls after a warm-up; prints the
                                                   median and the spread (min .. max) of the per-round means, the library's per-kernel events
                                                   (a round of its own: the events serialise the launches) and one JSON line

A call synchronises the stream once after the quantile kernel (the refusal of non-finite input), so the time of a call holds one
host round trip.  The clock state is what the machine gives a process that sets nothing; the first round is a warm-up."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# step -> (dim, combination); copy_<dim>: a device copy of the matrix
STEPS = {"copy_20": (20, None), "d20": (20, 0), "d20_combination": (20, 1), "copy_40": (40, None), "d40": (40, 0), "d40_combination": (40, 1)}
KERNELS = ("quanteq_quantile", "quanteq_search", "quanteq_combine_search", "quanteq_apply", "quanteq_sum", "quanteq_normalize")


def cpu_seconds(dim, combination):
    try:
        with np.load(os.path.join(ROOT, "tests", "golden", "ref_quanteq.npz")) as z:
            return float(z["cpu_seconds_per_segment/%d/%d" % (dim, combination)]), str(z["cpu_name"])
    except (OSError, KeyError):
        return None, None


def step(a):
    import torch

    import rasr_amd
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    dim, comb = STEPS[a.step]
    n_seg, per_seg, nq = a.segments, a.frames, 4
    T = n_seg * per_seg
    off = np.arange(n_seg + 1, dtype=np.int64) * per_seg
    rng = np.random.Generator(np.random.PCG64(5))
    level = 4.0 + np.arange(dim) / 4.0
    x = torch.from_numpy((level * np.exp(rng.normal(0.0, 0.5, (T, dim)))).astype(np.float32)).cuda()
    out = torch.empty_like(x)
    tq = np.sort(5.0 * np.exp(rng.normal(0.0, 0.6, (nq + 1, 1))), axis=0).astype(np.float32) * np.ones((1, dim), np.float32)   # pooled
    if comb is None:
        run = lambda: out.copy_(x)
    else:
        q = rasr_amd.QuantileEqualization(ctx, dim, tq, combination=comb, variance=1)
        run = lambda: q.apply_dev(off, x, dim, out, dim)
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            run()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / a.iters)
    v = np.array(times)
    res = {"step": a.step, "segments": n_seg, "frames_per_segment": per_seg, "channels": dim, "reps": a.reps, "iters": a.iters,
           "median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4),
           "matrix_mb": round(T * dim * 4 / 1e6, 2)}
    if comb is not None:
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(a.iters):
            run()
        torch.cuda.synchronize()
        for k in KERNELS:
            ms, launches = ctx.profile_get(k)
            if launches:
                res[k + "_ms"] = round(ms, 4)
        ctx.profile(False)
        cpu, name = cpu_seconds(dim, comb)
        if cpu is not None:
            res["cpu_seconds_per_segment"] = round(cpu, 4)
            res["cpu_name"] = name
            res["cpu_ms_for_all_segments"] = round(cpu * n_seg * 1e3, 1)
            res["cpu_over_device"] = round(cpu * n_seg * 1e3 / res["median_ms"], 1)
    print("%-16s median %.4f ms  spread %.4f .. %.4f ms" % (a.step, res["median_ms"], res["min_ms"], res["max_ms"]))
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--timeout", type=int, default=120, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quanteq_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--iters", str(a.iters),
               "--segments", str(a.segments), "--frames", str(a.frames)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("quanteq_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
