#!/usr/bin/env python3
"""tools/nnstep_probe.py -- MiniBatchTrainer on BASELINE config 4's network (440 -> 6 x 2048 rectified -> 10000, 42.4 M parameters) and
1024 resident frames: the statistics pass into the caller's f64 buffer (accumulate_dev) beside the pass into the handle's f32
statistics (step_accumulate_dev), the step alone (step_estimate_dev: finalize, seven update launches, seven bias launches, seven
step-size launches), and the two together with and without the info copy.

    python3 tools/nnstep_probe.py                 the driver: one child process per configuration, each under its own `timeout`, in a
                                                  chain that stops at the first one that fails; the children's JSON lines go to
                                                  profiles/nnstep_probe.jsonl
    python3 tools/nnstep_probe.py --step NAME     one configuration: prints one JSON line

HIP-event time over `--iters` calls after a warm-up, `--reps` rounds; median and spread (min .. max) of the per-round means.  The
update's rate counts 20 bytes per parameter (G and W^T read; G, W^T and W written).  No time is fixed in advance."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"plain": dict(regularizer="none", estimator="mean-normalized-sgd"),
         "l2_clipping": dict(regularizer="l2", estimator="mean-normalized-sgd-l1-clipping")}
DIMS = [440] + [2048] * 6 + [10000]


def step(name, reps, iters):
    import torch

    import rasr_amd
    rng = np.random.default_rng(1)
    Ws = [(rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32) for i, o in zip(DIMS[:-1], DIMS[1:])]
    bs = [np.zeros(o, np.float32) for o in DIMS[1:]]
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    T = 1024
    x = torch.from_numpy(rng.standard_normal((T, DIMS[0])).astype(np.float32)).cuda()
    e = torch.from_numpy(rng.integers(0, DIMS[-1], T).astype(np.int32)).cuda()
    tr = rasr_amd.MiniBatchTrainer(ctx, Ws, bs, [1] * 6 + [0])
    tr.set_estimator(learning_rate=1e-3, regularization_constant=[1e-4] * 7, log_step_size=True, **STEPS[name])
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    calls = {"accumulate_dev": lambda: tr.accumulate_dev(x, DIMS[0], T, e, acc), "step_accumulate_dev": lambda: tr.step_accumulate_dev(x, DIMS[0], T, e),
             "step_estimate_dev": tr.step_estimate_dev, "step_dev": lambda: tr.step_dev(x, DIMS[0], T, e, info=False),
             "step_dev_with_info": lambda: tr.step_dev(x, DIMS[0], T, e)}
    n_par = sum(w.size for w in Ws)
    out = {"step": name, "network": "440-6x2048-10000", "parameters": n_par, "frames": T, "reps": reps, "iters": iters}
    for what, f in calls.items():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        means = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize()
            means.append(a.elapsed_time(b) / iters)
        out[what + "_ms"] = [round(float(v), 4) for v in (np.median(means), min(means), max(means))]
    out["update_tb_per_s"] = round(20.0 * n_par / out["step_estimate_dev_ms"][0] / 1e9, 3)
    tr.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child")
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.iters)
    dst = os.path.join(ROOT, "profiles", "nnstep_probe.jsonl")
    lines = []
    for name in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps),
                            "--iters", str(a.iters)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("step %s ended with status %d:\n%s" % (name, r.returncode, r.stdout + r.stderr))
        lines.append([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        print(lines[-1])
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
