#!/usr/bin/env python3
"""tools/posterior_probe.py -- the state-posterior pass and the combination of two score matrices at 63 936 frames x 10 000 mixtures (the
headline's score matrix, 2.56 GB of f32), data resident, next to a device-to-device copy of that matrix (the yardstick: each pass reads
it once) and to the amx_gmm_score_dev call that produced it (10 000 mixtures of one diagonal density, dimension 16, diagonal-maximum).

    python3 tools/posterior_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain
                                                     that stops at the first step that fails; the children's JSON lines go to
                                                     profiles/posterior_probe.jsonl
    python3 tools/posterior_probe.py --step NAME     one step: HIP-event time with a synchronise, `--reps` rounds of `--iters` calls after
                                                     a warm-up; prints the median and the spread (min .. max) of the per-round means and
                                                     one JSON line

Steps: gmm_score, copy, dense (posteriors into a dense f32 matrix, no pruning), sparse_1pct and sparse_all (the sparse form with a
pruning threshold that keeps about 1 % / all of a row; the threshold of the first comes from the 1 % quantile of s - min over the first
64 rows), combine2 (two matrices, both columns the identity, scales 1 and 0.5).  The counters are not read back (no synchronisation
inside a call)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("gmm_score", "copy", "dense", "sparse_1pct", "sparse_all", "combine2")


def step(a):
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    T, n, dim = a.frames, a.mixtures, 16
    rng = np.random.Generator(np.random.PCG64(5))
    feats = torch.from_numpy(rng.standard_normal((T, dim)).astype(np.float32)).cuda()
    gmm = rasr_amd.GmmFeatureScorer(ctx, synth.gmm_cart(n, 1, 1, dim, seed=3, pooled=False), "diagonal-maximum")
    scores = torch.empty((T, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gmm.score_dev(feats, T, scores)
    torch.cuda.synchronize()
    res = {"step": a.step, "frames": T, "mixtures": n, "reps": a.reps, "iters": a.iters, "matrix_mb": round(T * n * 4 / 1e6, 1)}
    if a.step == "gmm_score":
        run = lambda: gmm.score_dev(feats, T, scores)
    elif a.step == "copy":
        out = torch.empty_like(scores)
        run = lambda: out.copy_(scores)
    elif a.step == "dense":
        h = rasr_amd.StatePosteriorScorer(ctx, n)
        out = torch.empty_like(scores)
        run = lambda: h.posteriors(scores, n, T, posterior_f32_dev=out, count_no_minimum=False)
    elif a.step in ("sparse_1pct", "sparse_all"):
        if a.step == "sparse_all":
            threshold, cap = 1e30, n
        else:
            head = scores[:64].cpu().numpy().astype(np.float64)
            threshold = float(np.quantile(head - head.min(axis=1, keepdims=True), 0.01))
            cap = max(64, n // 25)
        h = rasr_amd.StatePosteriorScorer(ctx, n, pruning_threshold=threshold)
        si = torch.empty((T, cap), dtype=torch.int32, device="cuda")
        sv = torch.empty((T, cap), dtype=torch.float32, device="cuda")
        cnt = torch.empty(T, dtype=torch.int32, device="cuda")
        run = lambda: h.posteriors(scores, n, T, sparse_index_dev=si, sparse_value_dev=sv, sparse_count_dev=cnt, sparse_capacity=cap,
                                   count_no_minimum=False)
        res.update(pruning_threshold=threshold, sparse_capacity=cap)
    else:
        other = scores * 0.5
        out = torch.empty_like(scores)
        ident = np.stack([np.arange(n), np.arange(n)], axis=1)
        c = rasr_amd.CombinedScorer(ctx, [n, n], ident, [1.0, 0.5])
        run = lambda: c.combine(T, [scores, other], [n, n], out, n)
    run()
    torch.cuda.synchronize()
    if a.step.startswith("sparse"):
        k = cnt.cpu().numpy()
        res.update(survivors_mean=round(float(k.mean()), 1), survivors_max=int(k.max()))
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
    res.update(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4))
    print("%-12s median %.4f ms  spread %.4f .. %.4f ms" % (a.step, res["median_ms"], res["min_ms"], res["max_ms"]))
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=63936)
    ap.add_argument("--mixtures", type=int, default=10000)
    ap.add_argument("--timeout", type=int, default=150, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--iters", str(a.iters),
               "--frames", str(a.frames), "--mixtures", str(a.mixtures)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("posterior_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
