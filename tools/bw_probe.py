#!/usr/bin/env python3
"""tools/bw_probe.py -- Baum-Welch alignment on tools/align_probe.py's workload (64 segments x 1000 frames over left-to-right graphs of
600 states on a score matrix of 10 000 columns, data resident), next to the Viterbi alignment with the same pruning in the same process
and next to the device-to-host copy of the matrix that an alignment on the host would need first.

    python3 tools/bw_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                              at the first step that fails; the children's JSON lines go to profiles/bw_probe.jsonl
    python3 tools/bw_probe.py --step NAME     one step: HIP-event time with a synchronise, `--reps` rounds of `--iters` calls after a
                                              warm-up; prints the median and the spread (min .. max) of the per-round means, the
                                              library's per-kernel events and one JSON line

Steps: d2h_copy (the score matrix into pinned host memory), default (the aligner's default pruning: 50, doubling until the score repeats),
no_pruning (one pass at a threshold nothing exceeds).  The two alignment steps time ViterbiAligner.align and BaumWelchAligner.align (the
item copy-out included) one after the other and report the ratio."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"d2h_copy": None, "default": {}, "no_pruning": {"min_acoustic_pruning": 3e38, "max_acoustic_pruning": 3e38, "increment_factor": 1.0}}
KERNELS = ("align_gather", "align_search", "align_traceback", "bw_gather", "bw_search", "bw_forward", "bw_backward_count", "bw_scan", "bw_backward_write")


def timed(torch, run, reps, iters):
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            run()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / iters)
    v = np.array(times)
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4))


def step(a):
    import torch

    import rasr_amd
    from tests import align_reference as ar
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    n_seg, per_seg, n, dim, states = a.segments, a.frames, a.columns, 40, a.states
    T = n_seg * per_seg
    off = np.arange(n_seg + 1, dtype=np.int64) * per_seg
    rng = np.random.Generator(np.random.PCG64(5))
    feats = torch.from_numpy(rng.standard_normal((T, dim)).astype(np.float32)).cuda()
    gmm = rasr_amd.GmmFeatureScorer(ctx, synth.gmm_cart(n, 1, 1, dim, seed=3, pooled=False), "diagonal-maximum")
    scores = torch.empty((T, n), dtype=torch.float32, device="cuda")
    gmm.score_dev(feats, T, scores)
    torch.cuda.synchronize()
    res = {"step": a.step, "segments": n_seg, "frames_per_segment": per_seg, "states": states, "columns": n, "reps": a.reps, "iters": a.iters,
           "matrix_mb": round(T * n * 4 / 1e6, 1)}
    cfg = STEPS[a.step]
    if cfg is None:
        host = torch.empty((T, n), dtype=torch.float32, pin_memory=True)
        res.update(timed(torch, lambda: host.copy_(scores, non_blocking=True), a.reps, a.iters))
        print("%-12s median %.4f ms  spread %.4f .. %.4f ms" % (a.step, res["median_ms"], res["min_ms"], res["max_ms"]))
        print(json.dumps(res))
        ctx.close()
        return
    graphs = rasr_amd.ViterbiAligner.graphs([ar.linear_hmm(states, n, 100 + s) for s in range(n_seg)])
    label = torch.empty(T, dtype=torch.int32, device="cuda")
    emission, arc = torch.empty_like(label), torch.empty(T, dtype=torch.float32, device="cuda")
    ioff = torch.empty(T + 1, dtype=torch.int64, device="cuda")
    vit, bw = rasr_amd.ViterbiAligner(ctx, **cfg), rasr_amd.BaumWelchAligner(ctx, **cfg)
    last = {}

    def run_viterbi():
        last["viterbi"] = vit.align(off, graphs, scores, n, label_dev=label, emission_dev=emission, arc_score_dev=arc)[3:]

    def run_bw():
        last["bw"] = bw.align(off, graphs, scores, n, item_offsets_dev=ioff)[2:]
    v, b = timed(torch, run_viterbi, a.reps, a.iters), timed(torch, run_bw, a.reps, a.iters)
    res.update({"viterbi_" + k: x for k, x in v.items()})
    res.update({"bw_" + k: x for k, x in b.items()})
    res["bw_over_viterbi"] = round(b["median_ms"] / v["median_ms"], 2)
    for name in ("viterbi", "bw"):
        r, counters = last[name]
        res.update({name + "_reached": int(sum(x["reached"] for x in r)), name + "_iterations": sorted({x["n_iterations"] for x in r}),
                    name + "_average_states": round(float(np.mean([x["average_states"] for x in r])), 1), name + "_passes_run": counters[1]})
    res["items"] = int(sum(x["n_items"] for x in last["bw"][0]))
    res["items_per_frame"] = round(res["items"] / T, 2)
    ctx.profile(True)   # the split between the kernels, a round of its own (the events serialise the launches)
    ctx.profile_reset()
    for _ in range(a.iters):
        run_viterbi()
        run_bw()
    torch.cuda.synchronize()
    for k in KERNELS:
        ms, launches = ctx.profile_get(k)
        if launches:
            res[k + "_ms"] = round(ms, 4)
    ctx.profile(False)
    print("%-12s viterbi median %.4f ms (%.4f .. %.4f)  baum-welch median %.4f ms (%.4f .. %.4f)  ratio %.2f" % (
        a.step, v["median_ms"], v["min_ms"], v["max_ms"], b["median_ms"], b["min_ms"], b["max_ms"], res["bw_over_viterbi"]))
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--states", type=int, default=600)
    ap.add_argument("--columns", type=int, default=10000)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bw_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--iters", str(a.iters),
               "--segments", str(a.segments), "--frames", str(a.frames), "--states", str(a.states), "--columns", str(a.columns)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("bw_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
