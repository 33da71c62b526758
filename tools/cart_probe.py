#!/usr/bin/env python3
"""tools/cart_probe.py -- decision-tree state tying at the size of the headline model's own tree: about 100 000 examples (allophone states),
1 000 questions, dimension 40, 10 000 leaves; and the example accumulation in front of it (1 000 000 frames, 30 000 labels, one of them
-- silence -- holding 30 % of the frames).

    python3 tools/cart_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                                at the first step that fails; the children's JSON lines go to profiles/cart_probe.jsonl
    python3 tools/cart_probe.py --step NAME     one step; prints one JSON line

Steps: accumulate (wall time of a call and the chain kernel's own), train_default (the device's gain as a screen, the contenders through
the host's logarithm), train_exact_all (every question through the host: the reference mode and the check on the margin).  The two
training steps print a digest of the tree, the log and the classes; the driver records whether they are identical, and the share of
(node, question) items the default mode re-evaluated."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("accumulate", "train_default", "train_exact_all")


def problem(E, Q, dim, seed=11):
    """examples with a centre of their own and a plausible variance; questions that cut the space of centres by random hyperplanes, so
    that gains mean something and the tree grows unevenly"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = rng.integers(1, 200, E).astype(np.float64)
    centre = rng.standard_normal((E, dim)) * 2.0
    mean = centre + rng.standard_normal((E, dim)) / np.sqrt(n)[:, None]
    var = rng.uniform(0.5, 1.5, (E, dim))
    values = np.hstack([mean * n[:, None], (var + mean * mean) * n[:, None]])
    w = rng.standard_normal((Q, dim))
    w[:, rng.integers(0, dim, Q)] *= 4.0
    answers = (w @ centre.T) > rng.standard_normal((Q, 1)) * 2.0
    return n, values, answers


def step_train(a):
    import rasr_amd
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    n, values, answers = problem(a.examples, a.questions, a.dim)
    bits = rasr_amd.DecisionTreeTrainer.pack_answers(answers)
    steps = [dict(action="split", questions=list(range(a.questions)), min_obs=a.min_obs)]
    t = rasr_amd.DecisionTreeTrainer(ctx, max_leaves=a.leaves, exact_all=a.step == "train_exact_all")
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    out = t.train(n, values, bits, steps)
    wall = time.perf_counter() - t0
    ms, launches = ctx.profile_get("cart_eval")
    ctx.profile(False)
    h = hashlib.sha256()
    for k in ("nodes", "classes", "log"):
        h.update(np.ascontiguousarray(out[k]).tobytes())
    res = dict(step=a.step, examples=a.examples, questions=a.questions, dim=a.dim, max_leaves=a.leaves, min_obs=a.min_obs, leaves=out["n_leaves"],
               commits=out["n_commits"], wall_s=round(wall, 3), cart_eval_ms_total=round(ms * launches, 2), cart_eval_ms_mean=round(ms, 4), launches=int(out["launches"]),
               items_screened=int(out["items_screened"]), items_reevaluated=int(out["items_reevaluated"]), negative_gain_errors=int(out["negative_gain_errors"]),
               total_gain=out["total_gain"], digest=h.hexdigest()[:16])
    if out["items_screened"]:
        res["share_reevaluated"] = round(out["items_reevaluated"] / out["items_screened"], 6)
    print(json.dumps(res))
    ctx.close()


def step_accumulate(a):
    import torch

    import rasr_amd
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    rng = np.random.Generator(np.random.PCG64(12))
    T, dim, n_labels = a.frames, a.dim, a.labels
    x = torch.from_numpy(rng.standard_normal((T, dim)).astype(np.float32)).cuda()
    lab = rng.integers(1, n_labels, T).astype(np.int32)
    lab[rng.random(T) < 0.3] = 0
    lab = torch.from_numpy(lab).cuda()
    acc = rasr_amd.CartExampleAccumulator(ctx, n_labels, dim)
    acc.accumulate(x, lab)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        acc.accumulate(x, lab)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    ctx.profile_reset()
    acc.accumulate(x, lab)
    torch.cuda.synchronize()
    ms, launches = ctx.profile_get("cart_accumulate")
    ctx.profile(False)
    v = np.array(times)
    print(json.dumps(dict(step=a.step, frames=T, dim=dim, labels=n_labels, longest_label_frames=int((lab == 0).sum()), reps=a.reps,
                          median_ms=round(float(np.median(v)), 3), min_ms=round(float(v.min()), 3), max_ms=round(float(v.max()), 3),
                          chain_kernel_ms=round(ms, 3))))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--examples", type=int, default=100000)
    ap.add_argument("--questions", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=40)
    ap.add_argument("--leaves", type=int, default=10000)
    ap.add_argument("--min-obs", dest="min_obs", type=int, default=200)
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--labels", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=",".join(STEPS), help="the driver's steps, comma-separated")
    ap.add_argument("--timeout", type=int, default=420, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cart_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step_accumulate(a) if a.step == "accumulate" else step_train(a)
    lines = []
    for name in a.only.split(","):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--examples", str(a.examples), "--questions",
               str(a.questions), "--dim", str(a.dim), "--leaves", str(a.leaves), "--min-obs", str(a.min_obs), "--frames", str(a.frames), "--labels",
               str(a.labels), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("cart_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    by = {l["step"]: l for l in lines}
    if "train_default" in by and "train_exact_all" in by:
        same = by["train_default"]["digest"] == by["train_exact_all"]["digest"]
        by["train_default"]["identical_to_exact_all"] = by["train_exact_all"]["identical_to_default"] = same
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(l) for l in lines) + "\n")
    print("wrote %s" % a.out)
    if "train_default" in by and "train_exact_all" in by and not same:
        sys.exit("cart_probe: the default mode's tree differs from exact_all's")


if __name__ == "__main__":
    main()
