#!/usr/bin/env python3
"""tools/latbest_probe.py -- the lattice best path and forward-backward pruning (amx_latbest_run_dev) at the workload of
tools/latpost_probe.py: 64 random lattices of about 2 000 states and 8 000 arcs each, beside the log-semiring potentials kernel of
amx_latpost_run_dev measured in the same process.

    python3 tools/latbest_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                                   at the first step that fails; the children's JSON lines are appended to
                                                   profiles/latbest_probe.jsonl
    python3 tools/latbest_probe.py --step NAME     one step; prints one JSON line

Per call, after a warm-up call, over --reps calls (smallest, median, largest): the wall time with the stream drained; the host's plan and its
packing and enqueueing of the uploads (amx_latbest_last_timing); every kernel from the library's event timers."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"best": (None, True, False), "prune": (8.0, True, False), "prune_trim": (8.0, True, True)}   # threshold, relative, trim
KERNELS = ("latbest_potentials", "latbest_arc", "latbest_path", "latbest_min", "latbest_keep", "latbest_trim", "latbest_scan")


def step(a):
    import torch

    import rasr_amd
    from tests import latpost_reference as lr
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    lats = [lr.random_dag(a.states, a.arcs, 900 + k, n_final=3) for k in range(a.segments)]
    lb = rasr_amd.LatticeBest(ctx, *STEPS[a.step])
    lp = rasr_amd.LatticePosterior(ctx, "log")
    t = lb.tables(lats)
    n_states, n_arcs = int(t["state_offsets"][-1]), len(t["arc_target"])
    bufs = [torch.empty(n, dtype=dt, device="cuda") for n, dt in ((n_states, torch.int32), (n_states, torch.int32), (n_arcs, torch.uint8), (n_arcs, torch.int32))]
    post = [torch.empty(n_arcs, dtype=torch.float32, device="cuda"), torch.empty(n_states, dtype=torch.float32, device="cuda")]
    info = lb.run_dev(t, *bufs)
    lp.run_dev(t, *post)
    torch.cuda.synchronize()
    wall, plan, upload = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        lb.run_dev(t, *bufs)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        p, u = lb.last_timing()
        plan.append(p), upload.append(u)
    ctx.profile(True)
    got = {n: [] for n in KERNELS + ("latpost_potentials",)}
    for _ in range(a.reps):
        ctx.profile_reset()
        lb.run_dev(t, *bufs)
        lp.run_dev(t, *post)
        torch.cuda.synchronize()
        for n in got:
            if n != "latbest_trim" or STEPS[a.step][2]:
                got[n].append(ctx.profile_get(n)[0])
    ctx.profile(False)
    span = lambda v: [round(float(x), 4) for x in (np.min(v), np.median(v), np.max(v))] if v else None   # noqa: E731
    print(json.dumps(dict(step=a.step, reps=a.reps, segments=a.segments, states=n_states, arcs=n_arcs, kept_arcs=int(sum(i["kept_arcs"] for i in info)),
                          levels_forward_max=max(i["levels_forward"] for i in info), levels_backward_max=max(i["levels_backward"] for i in info),
                          min_median_max_ms=dict(call=span(wall), plan=span(plan), upload=span(upload), **{n: span(v) for n, v in got.items()}))))
    lb.close()
    lp.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--states", type=int, default=2000, help="per lattice")
    ap.add_argument("--arcs", type=int, default=8000, help="per lattice")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=120, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latbest_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--segments", str(a.segments), "--states",
               str(a.states), "--arcs", str(a.arcs), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("latbest_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    with open(a.out, "a") as f:
        f.write("\n".join(json.dumps(l) for l in lines) + "\n")
    print("appended to %s" % a.out)


if __name__ == "__main__":
    main()
