#!/usr/bin/env python3
"""tools/nntrain_probe.py -- one FeedForwardTrainer.accumulate_dev call (all four statistics) of BASELINE config 4's network
(440 -> 6 x 2048 rectified -> 10000) on 1024 resident frames, and the three GEMM kinds of the pass alone.

    python3 tools/nntrain_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that
                                                   stops at the first step that fails; the children's JSON lines go to
                                                   profiles/nntrain_probe.jsonl
    python3 tools/nntrain_probe.py --step NAME     one step: prints its figures and one JSON line

Steps.  accumulate: HIP-event time of the whole call with a synchronise, `--reps` rounds of `--iters` calls after a warm-up; median and
spread (min .. max) of the per-round means.  The call waits once for its label check, which is inside the figure.
gemm_kinds: the library's own event pairs (Context.profile) in a round of their own, because the events serialise the launches.  The three
GEMM kinds have pairs that enclose their launches and nothing else: nntrain_gemm_forward (7 x gemm_f32_kernel), nntrain_gemm_backward
(6 x nntrain_gemm_bwd_kernel), nntrain_gemm_tn (7 x nntrain_gemm_tn_kernel, one pair per layer); each kind's rate is its multiply-adds
(2 T sum in x out; the backward kind has no first layer) over its time per call.  The other pairs: nntrain_pack, nntrain_softmax,
nntrain_error, nntrain_gradient_sums (the partial adds into the f64 buffer and the bias column sums), nntrain_feature_sums.  No time is
fixed in advance."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("accumulate", "gemm_kinds")
SECTIONS = ("nntrain_feature_sums", "nntrain_pack", "nntrain_gemm_forward", "nntrain_softmax", "nntrain_error", "nntrain_gemm_backward", "nntrain_gemm_tn",
            "nntrain_gradient_sums")


def step(a):
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    dims = [440] + [2048] * 6 + [10000]
    Ws, bs, acts, _ = synth.ffnn(dims, seed=7)
    tr = rasr_amd.FeedForwardTrainer(ctx, Ws, bs, acts, statistics=("class-counts", "mean-and-variance", "base", "gradient"))
    T = a.frames
    rng = np.random.Generator(np.random.PCG64(5))
    feats = torch.from_numpy(rng.standard_normal((T, dims[0])).astype(np.float32)).cuda()
    emission = torch.from_numpy(rng.integers(0, dims[-1], T).astype(np.int32)).cuda()
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")

    def run():
        tr.accumulate_dev(feats, dims[0], T, emission, acc)
    mac = [i * n for i, n in zip(dims[:-1], dims[1:])]
    flop = {"nntrain_gemm_forward": 2.0 * T * sum(mac), "nntrain_gemm_backward": 2.0 * T * sum(mac[1:]), "nntrain_gemm_tn": 2.0 * T * sum(mac)}
    res = {"step": a.step, "network": "440-6x2048-10000", "frames": T, "reps": a.reps, "iters": a.iters, "accumulator_mb": round(acc.numel() * 8 / 1e6, 1)}
    run()
    torch.cuda.synchronize()
    if a.step == "accumulate":
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
        res.update(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4),
                   gemm_tflops=round(sum(flop.values()) / float(np.median(v)) / 1e9, 2))
        print("accumulate   median %.4f ms  spread %.4f .. %.4f ms  (%.1f TF over the three GEMM kinds)" % (res["median_ms"], res["min_ms"], res["max_ms"], res["gemm_tflops"]))
    else:
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(a.iters):
            run()
        torch.cuda.synchronize()
        for k in SECTIONS:
            ms, launches = ctx.profile_get(k)   # the mean over the event pairs of that name, and how many there were
            if launches:
                ms = ms * launches / a.iters    # per call (nntrain_gemm_tn and nntrain_gradient_sums have one pair per layer)
                res[k + "_ms"] = round(ms, 4)
                if k in flop:
                    res[k + "_tflops"] = round(flop[k] / ms / 1e9, 2)
                print("%-24s %.4f ms per call%s" % (k, ms, "  %.1f TF" % res[k + "_tflops"] if k in flop else ""))
        ctx.profile(False)
    print(json.dumps(res))
    tr.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--timeout", type=int, default=180, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nntrain_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--iters", str(a.iters),
               "--frames", str(a.frames)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("nntrain_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
