#!/usr/bin/env python3
"""tools/linseg_probe.py -- linear-segmentation alignment of 64 segments x 1000 frames (the energy a column of a resident [frames x 40]
feature matrix, flat models of 60 states), next to amx_align_viterbi_dev on the same batch (left-to-right graphs of the same 60 states on a
resident score matrix of 200 columns): what the first alignment of a training costs beside every later one.

    python3 tools/linseg_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that
                                                  stops at the first step that fails; the children's JSON lines go to profiles/linseg_probe.jsonl
    python3 tools/linseg_probe.py --step NAME     one step: HIP-event time with a synchronise, `--reps` rounds of `--iters` calls after a
                                                  warm-up; prints the median and the spread (min .. max) of the per-round means, the
                                                  library's per-kernel events and one JSON line

Steps: linseg_default (three iterations of the delimiter), linseg_sietill (the Sietill delimiter, whose loops are twice as long),
linseg_one_long (ONE segment of 64 000 frames: the serial f64 chain of the longest segment, which bounds a call), viterbi_same_batch
(the Viterbi aligner's default pruning)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"linseg_default": {}, "linseg_sietill": {"should_use_sietill": 1}, "linseg_one_long": {}, "viterbi_same_batch": None}


def step(a):
    import torch

    import rasr_amd
    from tests import align_reference as ar
    from tests import linseg_reference as lr
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    n_seg, per_seg, dim, states, n = a.segments, a.frames, 40, a.states, a.columns
    if a.step == "linseg_one_long":
        n_seg, per_seg = 1, a.segments * a.frames
    T = n_seg * per_seg
    off = np.arange(n_seg + 1, dtype=np.int64) * per_seg
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.standard_normal((T, dim)).astype(np.float32)
    for s in range(n_seg):
        x[s * per_seg:(s + 1) * per_seg, 0] = lr.track(per_seg, 100 + s, lead=0.1 + 0.002 * s, trail=0.1)
    feats = torch.from_numpy(x).cuda()
    label = torch.empty(T, dtype=torch.int32, device="cuda")
    emission = torch.empty_like(label)
    res = {"step": a.step, "segments": n_seg, "frames_per_segment": per_seg, "states": states, "reps": a.reps, "iters": a.iters}
    last = {}
    if a.step == "viterbi_same_batch":
        scores = torch.from_numpy(rng.uniform(0.0, 20.0, (T, n)).astype(np.float32)).cuda()
        arc = torch.empty(T, dtype=torch.float32, device="cuda")
        graphs = rasr_amd.ViterbiAligner.graphs([ar.linear_hmm(states, n, 100 + s) for s in range(n_seg)])
        al = rasr_amd.ViterbiAligner(ctx)
        kernels = ("align_gather", "align_search", "align_traceback")
        res["columns"] = n

        def run():
            _, _, _, results, counters = al.align(off, graphs, scores, n, label_dev=label, emission_dev=emission, arc_score_dev=arc)
            last.update(results=results, counters=counters)
    else:
        models = rasr_amd.LinearSegmenter.models([lr.states(states) for _ in range(n_seg)], lr.SILENCE_LABEL, lr.SILENCE_EMISSION)
        seg = rasr_amd.LinearSegmenter(ctx, **STEPS[a.step])
        kernels = ("linseg",)

        def run():
            _, _, results, counters = seg.align(off, models, feats[:, 0], dim, label, emission)
            last.update(results=results, counters=counters)
    torch.cuda.synchronize()
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
    res.update(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4))
    if a.step == "viterbi_same_batch":
        res.update(reached=int(sum(r["reached"] for r in last["results"])), passes_run=last["counters"][1])
    else:
        res.update(ok=last["counters"][lr.OK], mean_speech_frames=round(float(np.mean([r["speech_end"] - r["speech_begin"] + 1 for r in last["results"]])), 1))
    ctx.profile(True)   # the kernels alone, a round of its own (the events serialise the launches)
    ctx.profile_reset()
    for _ in range(a.iters):
        run()
    torch.cuda.synchronize()
    for k in kernels:
        ms, launches = ctx.profile_get(k)
        if launches:
            res[k + "_ms"] = round(ms / launches, 4)
    ctx.profile(False)
    print("%-20s median %.4f ms  spread %.4f .. %.4f ms" % (a.step, res["median_ms"], res["min_ms"], res["max_ms"]))
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--states", type=int, default=60)
    ap.add_argument("--columns", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=120, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linseg_probe.jsonl"))
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
            sys.exit("linseg_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
