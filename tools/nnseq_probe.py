#!/usr/bin/env python3
"""tools/nnseq_probe.py -- one SegmentwiseNnTrainer batch (forward, arc scores, accumulate) of BASELINE config 4's network
(440 -> 6 x 2048 rectified -> 10000) on 16 segments of 256 frames, the 4096-row cap of a call, with a denominator lattice of 8 000
arcs per segment (the density of tools/latpost_probe.py), each arc aligned to 10..40 frames, and a numerator of one path.

    python3 tools/nnseq_probe.py                 the driver: one child process under its own `timeout`; its JSON lines go to
                                                 profiles/nnseq_probe.jsonl
    python3 tools/nnseq_probe.py --step batch    the measurement: prints its figures and one JSON line per configuration

Two configurations on ONE trainer in ONE process: mmi, the MMI flow (denominator +1 with the rejection test, numerator -1) with smoothing
0.1; ce, the same call with ce_smoothing_weight = 1, where no lattice pass runs -- the baseline beside which the lattice work is read.
After two warm-up batches of each, `--reps` rounds alternate between the two; a round is `--iters` whole batches (forward + scores +
accumulate) under a host clock that ends in a synchronise, and gives one mean per batch; reported are the median and the spread of the
rounds (10 x 10 batches of each configuration, about 3 s in all).  Then, in rounds of their own because the event pairs serialise the
launches, the library's event timers (Context.profile) per stage.  The posteriors are random numbers in (0, 1): the lattice
forward-backward is tools/latpost_probe.py's subject.  No time is fixed in advance."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("batch",)
CONFIGS = (("mmi", 0.1), ("ce", 1.0))
STAGES = {"forward": ("nnseq_pack", "nnseq_gemm_forward"), "scores": ("nnseq_scores",), "sort": ("nnseq_sort",), "collection": ("nnseq_collect", "nnseq_reject"),
          "smoothing": ("nnseq_smooth",), "backward": ("nnseq_gemm_backward",), "gradients": ("nnseq_gemm_tn", "nnseq_gradient_sums")}
NEW = ("scores", "sort", "collection", "smoothing")   # the stages this trainer adds to the frame-wise one; the rest is its GEMMs and sums


def lattice(rng, n_seg, T, arcs, n_classes, lo=10, hi=40):
    ao = np.arange(n_seg + 1, dtype=np.int64) * arcs
    n = rng.integers(lo, hi + 1, n_seg * arcs)
    begin = rng.integers(0, T - hi, n_seg * arcs)
    io = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    frame = (np.repeat(begin, n) + (np.arange(io[-1]) - np.repeat(io[:-1], n))).astype(np.int32)
    # three states per phone of about 9 frames: an emission is held for a few frames
    emission = np.repeat(rng.integers(0, n_classes, (io[-1] + 2) // 3), 3)[:io[-1]].astype(np.int32)
    return dict(arc_offsets=ao, item_offsets=io, item_frame=frame, item_emission=emission)


def step(a):
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    dims = [440] + [2048] * 6 + [10000]
    Ws, bs, acts, _ = synth.ffnn(dims, seed=7)
    tr = rasr_amd.FeedForwardTrainer(ctx, Ws, bs, acts, statistics=("base", "gradient"))
    seqs = {name: rasr_amd.SegmentwiseNnTrainer(tr, ce_smoothing_weight=lam, frame_rejection_threshold=0.05) for name, lam in CONFIGS}
    n_seg, T = a.segments, a.frames
    rng = np.random.Generator(np.random.PCG64(5))
    off = np.arange(n_seg + 1, dtype=np.int64) * T
    feats = torch.from_numpy(rng.standard_normal((n_seg * T, dims[0])).astype(np.float32)).cuda()
    den = lattice(rng, n_seg, T, a.arcs, dims[-1])
    align = np.repeat(rng.integers(0, dims[-1], (n_seg * T + 2) // 3), 3)[:n_seg * T].astype(np.int32)
    num = dict(arc_offsets=np.arange(n_seg + 1, dtype=np.int64), item_offsets=off.copy(), item_frame=np.tile(np.arange(T, dtype=np.int32), n_seg), item_emission=align)
    emission = torch.from_numpy(align).cuda()
    w_den = torch.from_numpy(rng.random(n_seg * a.arcs).astype(np.float32)).cuda()
    w_num = torch.ones(n_seg, dtype=torch.float32, device="cuda")
    scores = torch.zeros(n_seg * a.arcs, dtype=torch.float32, device="cuda")
    acc = torch.zeros(tr.accumulator_size(), dtype=torch.float64, device="cuda")
    passes = [dict(tables=den, arc_weight_dev=w_den, factor=1.0, role="reject"), dict(tables=num, arc_weight_dev=w_num, factor=-1.0)]
    objective = np.zeros(n_seg, np.float32)
    torch.cuda.synchronize()

    def run(name):
        seq = seqs[name]
        seq.forward_dev(feats, dims[0], off)
        seq.arc_scores_dev(den, scores)
        return seq.accumulate_dev(passes, emission, objective, acc)
    res = {}
    for name, lam in CONFIGS:
        for _ in range(2):   # two warm-up batches of each configuration
            info = run(name)
        torch.cuda.synchronize()
        res[name] = {"step": name, "network": "440-6x2048-10000", "segments": n_seg, "frames": n_seg * T, "arcs": int(den["arc_offsets"][-1]),
                     "items": int(den["item_offsets"][-1]), "ce_smoothing_weight": lam, "reps": a.reps, "iters": a.iters,
                     "rejected": int(info["rejected_observations"])}
        res[name].update(seqs[name].last_shape())
    rounds = {name: [] for name, _ in CONFIGS}
    for _ in range(a.reps):   # the two configurations alternate, so that a drift of the clocks meets both
        for name, _ in CONFIGS:
            t0 = time.perf_counter()
            for _ in range(a.iters):
                run(name)
            torch.cuda.synchronize()
            rounds[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
    for name, _ in CONFIGS:
        v = np.array(rounds[name])
        res[name].update(batch_ms=round(float(np.median(v)), 3), batch_min_ms=round(float(v.min()), 3), batch_max_ms=round(float(v.max()), 3))
        print("%-4s batch  median %.3f ms  spread %.3f .. %.3f ms over %d rounds of %d" % (name, res[name]["batch_ms"], res[name]["batch_min_ms"],
                                                                                       res[name]["batch_max_ms"], a.reps, a.iters))
    ctx.profile(True)
    for name, _ in CONFIGS:
        ctx.profile_reset()
        for _ in range(a.iters):
            run(name)
        torch.cuda.synchronize()
        total = 0.0
        for stage, names in STAGES.items():
            ms = 0.0
            for n in names:
                mean, pairs = ctx.profile_get(n)   # the mean over the event pairs of that name, and how many there were
                ms += mean * pairs / a.iters
            res[name][stage + "_ms"] = round(ms, 4)
            total += ms
            print("%-4s %-12s %.4f ms per batch" % (name, stage, ms))
        res[name]["stages_ms"] = round(total, 4)
        res[name]["new_kernels_share"] = round(sum(res[name][s + "_ms"] for s in NEW) / total, 4) if total else None
        res[name]["lattice_only_ms"] = round(sum(res[name][s + "_ms"] for s in ("scores", "sort", "collection")), 4)
    ctx.profile(False)
    for name, _ in CONFIGS:
        print(json.dumps(res[name]))
    for seq in seqs.values():
        seq.close()
    tr.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10, help="batches per round")
    ap.add_argument("--segments", type=int, default=16)
    ap.add_argument("--frames", type=int, default=256, help="per segment")
    ap.add_argument("--arcs", type=int, default=8000, help="of the denominator lattice, per segment")
    ap.add_argument("--timeout", type=int, default=280, help="seconds for the child of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnseq_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--iters", str(a.iters), "--segments", str(a.segments),
               "--frames", str(a.frames), "--arcs", str(a.arcs)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("nnseq_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.extend(l for l in r.stdout.splitlines() if l.startswith("{"))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
