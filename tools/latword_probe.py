#!/usr/bin/env python3
"""tools/latword_probe.py -- the lattice word measures (amx_latword_run_dev) at the workload of tools/latpost_probe.py: 64 random lattices
of about 2 000 states and 8 000 arcs each, beside the kernels of amx_latpost_run_dev measured in the same process.  A state's time is
four frames per position in the lattice's backbone, so an arc lasts 4 ... 44 frames; a fifth of the arcs carry label 0 (silence, all
over the segment), the others one of eight words of their stretch of 40 positions.  The correct lattice is the backbone.

    python3 tools/latword_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                                   at the first step that fails; the children's JSON lines are appended to
                                                   profiles/latword_probe.jsonl
    python3 tools/latword_probe.py --step NAME     one step; prints one JSON line

Per call, after a warm-up call, over --reps calls (smallest, median, largest): the wall time with the stream drained; the host's plan and its
enqueueing of the uploads (amx_latword_last_timing); every kernel from the library's event timers."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("timeframe-error-sum", "timeframe-error-max", "frame-word-accuracy", "approximate-word")
KERNELS = ("latword_list", "latword_cells", "latword_prefix", "latword_arcs", "latword_arcs_wave", "latword_approximate")


def lattices(a):
    from tests import latpost_reference as lr
    lats, correct = [], []
    for k in range(a.segments):
        lat = lr.random_dag(a.states, a.arcs, 900 + k, n_final=3)
        pos = np.argsort(np.random.RandomState(900 + k).permutation(a.states))   # random_dag's first draw: state id -> backbone position
        rng = np.random.RandomState(5000 + k)
        src = np.repeat(np.arange(a.states), np.diff(lat["arc_offsets"]))
        word = 1 + (pos[src] // 40) * 8 + rng.randint(0, 8, len(src))
        lat["state_time"] = (4 * pos).astype(np.int32)
        lat["arc_label"] = np.where(rng.uniform(size=len(src)) < 0.2, 0, word).astype(np.int32)
        lats.append(lat)
        keep = np.flatnonzero(pos[lat["arc_target"]] == pos[src] + 1)   # the backbone's arcs (a parallel random arc may join them)
        off = np.concatenate([[0], np.cumsum(np.bincount(src[keep], minlength=a.states))])
        correct.append(dict(arc_offsets=off, arc_target=lat["arc_target"][keep], arc_label=lat["arc_label"][keep], state_time=lat["state_time"],
                            initial=lat["initial"]))
    return lats, correct


def step(a):
    import torch

    import rasr_amd
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    lats, correct = lattices(a)
    timeframe = a.step.startswith("timeframe")
    lw = rasr_amd.LatticeWordMeasures(ctx, a.step, 0.1, short_pauses=(0,))
    lp = rasr_amd.LatticePosterior(ctx, "log")
    t, c, tp = lw.tables(lats), None if timeframe else lw.tables(correct), lp.tables(lats)
    n_states, n_arcs = int(t["state_offsets"][-1]), len(t["arc_target"])
    post = [torch.empty(n_arcs, dtype=torch.float32, device="cuda"), torch.empty(n_states, dtype=torch.float32, device="cuda")]
    out = torch.empty(n_arcs, dtype=torch.float32, device="cuda")
    lp.run_dev(tp, *post)
    info = lw.run_dev(t, c, post[0] if timeframe else None, out)
    torch.cuda.synchronize()
    wall, plan, upload = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        lw.run_dev(t, c, post[0] if timeframe else None, out)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        p, u = lw.last_timing()
        plan.append(p), upload.append(u)
    ctx.profile(True)
    got = {n: [] for n in KERNELS + ("latpost_potentials", "latpost_arcs")}
    for _ in range(a.reps):
        ctx.profile_reset()
        lp.run_dev(tp, *post)
        lw.run_dev(t, c, post[0] if timeframe else None, out)
        torch.cuda.synchronize()
        for n in got:
            ms, calls = ctx.profile_get(n)
            if calls:
                got[n].append(ms)
    ctx.profile(False)
    span = lambda v: [round(float(x), 4) for x in (np.min(v), np.median(v), np.max(v))] if v else None   # noqa: E731
    print(json.dumps(dict(step=a.step, reps=a.reps, segments=a.segments, states=n_states, arcs=n_arcs, feeds=int(sum(i["feeds"] for i in info)),
                          rows=int(sum(i["labels"] for i in info)), frames_max=max(i["frames"] for i in info), intervals=int(sum(i["intervals"] for i in info)),
                          min_median_max_ms=dict(call=span(wall), plan=span(plan), upload=span(upload), **{n: span(v) for n, v in got.items()}))))
    lw.close()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latword_probe.jsonl"))
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
            sys.exit("latword_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    with open(a.out, "a") as f:
        f.write("\n".join(json.dumps(l) for l in lines) + "\n")
    print("appended to %s" % a.out)


if __name__ == "__main__":
    main()
