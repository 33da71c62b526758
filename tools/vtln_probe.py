#!/usr/bin/env python3
"""tools/vtln_probe.py -- the fused MFCC kernel on config 2 (1000 utterances, seed 3, MFCC-40) in three forms, alternated in one
process: unwarped (amx_mfcc_create), one warping factor for every segment (a VTLN plan of one bank: the unwarped instantiation on
that bank) and 13 factors dealt round the utterances (the bank-per-tile variant).  HIP-event time of amx_mfcc_run_plan_dev with a synchronise, `--reps` rounds of
`--iters` launches each; prints the median and the spread (min .. max) of the per-round means per form, one JSON line at the end.
Kernel times without the launch path: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    grid = [round(0.88 + 0.02 * k, 2) for k in range(13)]
    lens = synth.utterance_lengths(1000, seed=3)
    off = np.concatenate([[0], np.cumsum(lens)])
    base = synth.waveform(int(lens.max()), seed=4)
    pcm = torch.from_numpy(np.concatenate([np.roll(base, u)[:n] for u, n in enumerate(lens)])).cuda()
    kw = dict(nr_cepstrum_coefficients=40, filter_width=138.0)
    plain = rasr_amd.MfccExtractor(ctx, **kw)
    vtln = rasr_amd.MfccExtractor(ctx, warping_factors=grid, **kw)
    forms = {"unwarped": (plain, plain.plan(off)),
             "one_factor": (vtln, vtln.plan(off, warping_factors=[1.0] * 1000)),
             "13_factors": (vtln, vtln.plan(off, warping_factors=[grid[u % 13] for u in range(1000)]))}
    out = torch.empty((forms["unwarped"][1].total_frames, 40), dtype=torch.float32, device="cuda")
    times = {k: [] for k in forms}
    for k, (fe, plan) in forms.items():   # warm-up
        fe.run_plan(plan, pcm, out)
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, (fe, plan) in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                fe.run_plan(plan, pcm, out)
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / a.iters)
    res = {"frames": forms["unwarped"][1].total_frames, "reps": a.reps, "iters": a.iters}
    for k, v in times.items():
        v = np.array(v)
        res[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}
        print("%-11s median %.4f ms  spread %.4f .. %.4f ms" % (k, np.median(v), v.min(), v.max()))
    u = res["unwarped"]["median_ms"]
    res["one_factor_vs_unwarped"] = round(res["one_factor"]["median_ms"] / u, 4)
    res["13_factors_vs_unwarped"] = round(res["13_factors"]["median_ms"] / u, 4)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
