"""tools/nn_layers_probe.py [--reps N] -- cost of the amx_ffnn_create_ex layer types on BASELINE config 4 (440 -> 6 x 2048 -> 10000).

Variants, per precision (f16mx, bf16x3) and batch (256, 1024, 63 936 frames):
  plain    the network as is (ReLU hidden layers)
  mvn      + a mean-and-variance-normalization input layer (fused into the input pack kernel)
  elu      ELU instead of ReLU in every hidden layer
  maxout   hidden layer 2 widened to 4096 outputs + maxoutvar k = 2 (2048 groups of two), i.e. the same next layer
Every variant's pass is timed with device events around `--reps` back-to-back score_dev calls after a warm-up; the variants alternate
round by round in one process and the median round is reported.  For the maxout variant the profiled time of the maxout kernel alone
and the bound of its extra traffic (the f32 rows of the 4096-wide layer written by the score epilogue and read back, plus the next
operand) at 5 TB/s are printed too; `widened` is the same network with the 4096-wide layer and no maxout, the next layer reading all
4096 (the GEMM work the maxout variant adds, without the maxout)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rasr_amd  # noqa: E402
from tests import synth  # noqa: E402

HBM = 5.0e12   # bytes / s sustained (profiles: ~5 TB/s of the 8 TB/s datasheet)


def networks():
    dims = [440] + [2048] * 6 + [10000]
    Ws, bs, acts, logp = synth.ffnn(dims, seed=7)
    rng = np.random.Generator(np.random.PCG64(8))
    mean = (3 * rng.standard_normal(440)).astype(np.float32)
    std = (0.5 + rng.random(440)).astype(np.float32)
    W2 = (rng.standard_normal((4096, 2048)) / np.sqrt(2048)).astype(np.float32)
    b2 = (0.1 * rng.standard_normal(4096)).astype(np.float32)
    W3w = (rng.standard_normal((2048, 4096)) / np.sqrt(4096)).astype(np.float32)
    Wm, bm = Ws[:2] + [W2] + Ws[3:], bs[:2] + [b2] + bs[3:]
    Ww, bw = Ws[:2] + [W2, W3w] + Ws[4:], list(bm)
    return {
        "plain": dict(Ws=Ws, bs=bs, acts=acts),
        "mvn": dict(Ws=Ws, bs=bs, acts=acts, preprocessing=[("mean-and-variance-normalization", mean, std)]),
        "elu": dict(Ws=Ws, bs=bs, acts=[4 if a else 0 for a in acts]),
        "maxout": dict(Ws=Wm, bs=bm, acts=acts, maxout={2: 2048}),
        "widened": dict(Ws=Ww, bs=bw, acts=acts),
    }, logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", default="256,1024,63936")
    ap.add_argument("--precisions", default="f16mx,bf16x3")
    a = ap.parse_args()
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    nets, logp = networks()
    Tmax = max(int(t) for t in a.frames.split(","))
    x = torch.randn((Tmax, 440), device="cuda")
    sc = torch.empty((Tmax, 10000), device="cuda")
    for prec in a.precisions.split(","):
        h = {k: rasr_amd.NnBatchFeatureScorer(ctx, v["Ws"], v["bs"], v["acts"], log_prior=logp, precision=prec,
                                              preprocessing=v.get("preprocessing"), maxout=v.get("maxout")) for k, v in nets.items()}
        for T in (int(t) for t in a.frames.split(",")):
            times = {k: [] for k in h}
            for k in h:   # warm-up: workspace, kernel attributes
                for _ in range(3):
                    h[k].score_dev(x, 440, T, sc)
            for _ in range(a.rounds):
                for k, nn in h.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        nn.score_dev(x, 440, T, sc)
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / a.reps)
            med = {k: float(np.median(v)) for k, v in times.items()}
            ctx.profile(True)
            ctx.profile_reset()
            h["maxout"].score_dev(x, 440, T, sc)
            torch.cuda.synchronize()
            mo = ctx.profile_get("ffnn_maxout")
            ctx.profile(False)
            mo_ms = mo[0]   # mean launch time
            extra = T * 4096 * 4 * 2 + T * 2048 * (3 if prec == "f16mx" else 4)   # f32 rows out + in, next operand out
            base = med["plain"]
            print("%-6s T=%6d  plain %8.4f ms | mvn %8.4f (%+5.1f %%) | elu %8.4f (%+5.1f %%) | widened %8.4f | maxout %8.4f "
                  "(%+6.3f ms vs plain, %+6.3f vs widened; maxout kernel %.4f ms, traffic bound %.4f ms for %.2f GB) | spread plain %.1f %%" %
                  (prec, T, base, med["mvn"], 100 * (med["mvn"] / base - 1), med["elu"], 100 * (med["elu"] / base - 1), med["widened"],
                   med["maxout"], med["maxout"] - base, med["maxout"] - med["widened"], mo_ms, extra / HBM * 1e3, extra / 1e9,
                   100 * (max(times["plain"]) - min(times["plain"])) / base), flush=True)
        del h
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
