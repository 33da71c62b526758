#!/usr/bin/env python3
"""tools/bayes_probe.py -- Bayes classification of 1000 segments x 1000 frames x 13 classes, data resident, in every mode, next to the
amx_gmm_score_dev call (13 mixtures of one diagonal density, dimension 16, diagonal-maximum) that produces the score matrix, so that the
decision's share of the fast-VTLN loop is visible.

    python3 tools/bayes_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that
                                                 stops at the first step that fails; the children's JSON lines go to profiles/bayes_probe.jsonl
    python3 tools/bayes_probe.py --step NAME     one step: HIP-event time with a synchronise, `--reps` rounds of `--iters` calls after a
                                                 warm-up; prints the median and the spread (min .. max) of the per-round means, the
                                                 library's per-kernel events and one JSON line

Steps: gmm_score (the scorer alone), copy (a device copy of the score matrix, the yardstick: every mode reads it once), segment, first16,
continuous (delay 0), window4, window25, window25_d7, scores (the score node, delay 0).  Weights are not given, the counters are not read
back (no synchronisation inside a call)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"gmm_score": None, "copy": None, "segment": {}, "first16": {"number_of_features": 16}, "continuous": {"delay": 0},
         "window4": {"window_length": 4}, "window25": {"window_length": 25}, "window25_d7": {"window_length": 25, "delay": 7},
         "scores": {"delay": 0}}
KERNELS = ("bayes_sum", "bayes_window", "bayes_argmin")


def step(a):
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    n_seg, per_seg, n, dim = a.segments, a.frames, 13, 16
    T = n_seg * per_seg
    off = np.arange(n_seg + 1, dtype=np.int64) * per_seg
    rng = np.random.Generator(np.random.PCG64(5))
    feats = torch.from_numpy(rng.standard_normal((T, dim)).astype(np.float32)).cuda()
    gmm = rasr_amd.GmmFeatureScorer(ctx, synth.gmm_cart(n, 1, 1, dim, seed=3, pooled=False), "diagonal-maximum")
    scores = torch.empty((T, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gmm.score_dev(feats, T, scores)
    torch.cuda.synchronize()
    lab = torch.empty(n_seg, dtype=torch.int32, device="cuda")
    fl = torch.empty(T, dtype=torch.int32, device="cuda")
    out, em = torch.empty_like(scores), torch.empty(T, dtype=torch.uint8, device="cuda")
    cfg = STEPS[a.step]
    if a.step == "gmm_score":
        run = lambda: gmm.score_dev(feats, T, scores)
    elif a.step == "copy":
        run = lambda: out.copy_(scores)
    elif a.step == "scores":
        b = rasr_amd.BayesClassifier(ctx, n, **cfg)
        run = lambda: b.scores(off, scores, n, out, n, em)
    else:
        b = rasr_amd.BayesClassifier(ctx, n, **cfg)
        run = lambda: b.classify(off, scores, n, lab, frame_label_dev=fl, count_no_winner=False)
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
    res = {"step": a.step, "segments": n_seg, "frames_per_segment": per_seg, "classes": n, "reps": a.reps, "iters": a.iters,
           "median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4),
           "matrix_mb": round(T * n * 4 / 1e6, 1)}
    if cfg is not None:   # the split between the kernels, a round of its own (the events serialise the launches)
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
    print("%-12s median %.4f ms  spread %.4f .. %.4f ms" % (a.step, res["median_ms"], res["min_ms"], res["max_ms"]))
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--segments", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--timeout", type=int, default=120, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bayes_probe.jsonl"))
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
            sys.exit("bayes_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
