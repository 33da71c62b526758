#!/usr/bin/env python3
"""tools/voicedness_probe.py -- the voicedness kernel on config 2's audio (1000 utterances, seed 3), alternated in one process with the
fused MFCC kernel (MFCC-40) on the same samples.  HIP-event time of amx_voicedness_run_batch_dev / amx_mfcc_run_plan_dev with a
synchronise, `--reps` rounds of `--iters` launches each; prints the median and the spread (min .. max) of the per-round means per
form, one JSON line at the end.  Kernel times without the launch path: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    lens = synth.utterance_lengths(1000, seed=3)
    off = np.concatenate([[0], np.cumsum(lens)])
    base = synth.waveform(int(lens.max()), seed=4)
    pcm = torch.from_numpy(np.concatenate([np.roll(base, u)[:n] for u, n in enumerate(lens)])).cuda()
    pcm16 = pcm.to(torch.int16)
    mfcc = rasr_amd.MfccExtractor(ctx, nr_cepstrum_coefficients=40, filter_width=138.0)
    plan = mfcc.plan(off)
    vc = rasr_amd.VoicednessExtractor(ctx)
    frames = int(sum(vc.n_frames(int(n)) for n in lens))
    ceps = torch.empty((plan.total_frames, 40), dtype=torch.float32, device="cuda")
    out = torch.empty(frames, dtype=torch.float32, device="cuda")
    forms = {"mfcc": lambda: mfcc.run_plan(plan, pcm, ceps),
             "voicedness": lambda: vc.run_batch_dev(off, pcm, out),
             "voicedness_s16": lambda: vc.run_batch_dev(off, pcm16, out)}
    times = {k: [] for k in forms}
    for f in forms.values():   # warm-up
        f()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, f in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                f()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / a.iters)
    res = {"mfcc_frames": plan.total_frames, "voicedness_frames": frames, "reps": a.reps, "iters": a.iters}
    for k, v in times.items():
        v = np.array(v)
        res[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}
        print("%-14s median %.4f ms  spread %.4f .. %.4f ms" % (k, np.median(v), v.min(), v.max()))
    res["voicedness_vs_mfcc"] = round(res["voicedness"]["median_ms"] / res["mfcc"]["median_ms"], 3)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
