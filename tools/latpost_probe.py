#!/usr/bin/env python3
"""tools/latpost_probe.py -- the lattice arc posteriors (amx_latpost_run_dev) at the size of a lattice-training batch: 64 random lattices of
about 2 000 states and 8 000 arcs each, in the three modes.

    python3 tools/latpost_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                                   at the first step that fails; the children's JSON lines are appended to
                                                   profiles/latpost_probe.jsonl
    python3 tools/latpost_probe.py --step NAME     one step; prints one JSON line

Per call (median of --reps after a warm-up call): the wall time with the stream drained; the host's plan and its packing and upload of the
tables (the library's own stop watch, amx_latpost_last_timing); the two kernels from the library's event timers."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("log", "prob", "expectation")
KERNELS = ("latpost_potentials", "latpost_arcs")


def step(a):
    import torch

    import rasr_amd
    from tests import latpost_reference as lr
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    ctx.set_contract(a.contract)
    lats = [lr.random_dag(a.states, a.arcs, 900 + k, n_final=3) for k in range(a.segments)]
    lp = rasr_amd.LatticePosterior(ctx, a.step)
    t = lp.tables(lats)
    n_states, n_arcs = int(t["state_offsets"][-1]), len(t["arc_target"])
    arc_out = torch.empty(n_arcs, dtype=torch.float32, device="cuda")
    final_out = torch.empty(n_states, dtype=torch.float32, device="cuda")
    info = lp.run_dev(t, arc_out, final_out)
    torch.cuda.synchronize()
    wall, plan, upload = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        lp.run_dev(t, arc_out, final_out)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        p, u = lp.last_timing()
        plan.append(p), upload.append(u)
    ctx.profile(True)
    got = {n: [] for n in KERNELS}
    for _ in range(a.reps):
        ctx.profile_reset()
        lp.run_dev(t, arc_out, final_out)
        torch.cuda.synchronize()
        for n in KERNELS:
            got[n].append(ctx.profile_get(n)[0])
    ctx.profile(False)
    med = lambda v: round(float(np.median(v)), 4)   # noqa: E731
    res = dict(step=a.step, contract=a.contract, reps=a.reps, segments=a.segments, states=n_states, arcs=n_arcs,
               levels_backward_max=max(i["levels_backward"] for i in info), levels_forward_max=max(i["levels_forward"] for i in info),
               call_ms=med(wall), plan_ms=med(plan), upload_ms=med(upload), kernel_ms={n: med(v) for n, v in got.items()},
               flows_agree=int(sum(i["flows_agree"] for i in info)))
    print(json.dumps(res))
    lp.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--states", type=int, default=2000, help="per lattice")
    ap.add_argument("--arcs", type=int, default=8000, help="per lattice")
    ap.add_argument("--contract", default="fma")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=120, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latpost_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--segments", str(a.segments), "--states",
               str(a.states), "--arcs", str(a.arcs), "--contract", a.contract, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("latpost_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    with open(a.out, "a") as f:
        f.write("\n".join(json.dumps(l) for l in lines) + "\n")
    print("appended to %s" % a.out)


if __name__ == "__main__":
    main()
