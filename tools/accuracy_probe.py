#!/usr/bin/env python3
"""tools/accuracy_probe.py -- the lattice arc accuracies (amx_accuracy_run_dev) on the workload of tools/arcalign_probe.py: 64 segments of
1000 frames on 10 000 columns, 60 000 keys on left-to-right graphs of 9-60 states, windows of 10-80 frames.  Each segment's reference is
the keys of one path through it: consecutive windows from frame 0 to the segment's end, the first keys of the table.  The alignments are
made once by amx_arcalign_run_dev in the same process; its search kernel's time is written beside the accuracy's for scale.

    python3 tools/accuracy_probe.py        appends one JSON line per mode to profiles/accuracy_probe.jsonl

Per mode, after a warm-up: the call through rasr_amd.LatticeAccuracy (run and arc_accuracies) by the host's clock with the stream drained,
and, from the library's event timers in calls of their own, the table kernels (accuracy_runs + accuracy_table), the accuracy kernel
(accuracy_key) and the check kernel; medians over --reps with the smallest and the largest.  The parent has no route to compare with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = np.array(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--columns", type=int, default=10000)
    ap.add_argument("--keys", type=int, default=60000)
    ap.add_argument("--arcs", type=int, default=128000)
    ap.add_argument("--graphs", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accuracy_probe.jsonl"))
    a = ap.parse_args()
    import torch

    import rasr_amd
    from tests import align_reference as ar
    rng = np.random.Generator(np.random.PCG64(2026))
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    torch.manual_seed(7)
    scores = torch.empty((a.segments * a.frames, a.columns), dtype=torch.float32, device="cuda").normal_(60.0, 15.0)
    off = np.arange(a.segments + 1, dtype=np.int64) * a.frames
    states = rng.integers(9, 61, a.graphs)
    graphs = [ar.linear_hmm(int(n), a.columns, 100 + i) for i, n in enumerate(states)]
    short = np.flatnonzero(states <= 17)   # graphs whose shortest path fits a window of 10 frames
    # the reference: one path of windows through each segment
    ps, pb, pe = [], [], []
    for s in range(a.segments):
        t = 0
        while t < a.frames:
            e = a.frames if a.frames - t < 20 else t + int(rng.integers(10, 81))
            e = min(e, a.frames)
            ps.append(s), pb.append(t), pe.append(e)
            t = e
    n_ref = len(ps)
    n_hyp = a.keys - n_ref
    kg = np.concatenate([rng.choice(short, n_ref), rng.integers(0, a.graphs, n_hyp)]).astype(np.int32)
    T = np.maximum(rng.integers(10, 81, n_hyp), (states[kg[n_ref:]] + 1) // 2 + 1).astype(np.int32)
    ks = np.concatenate([ps, rng.integers(0, a.segments, n_hyp)]).astype(np.int32)
    tb = np.concatenate([pb, (rng.random(n_hyp) * (a.frames - T + 1)).astype(np.int32)]).astype(np.int32)
    te = np.concatenate([pe, tb[n_ref:] + T]).astype(np.int32)
    is_ref = np.arange(a.keys) < n_ref
    arc_key = np.concatenate([np.arange(a.keys), rng.integers(0, a.keys, a.arcs - a.keys)]).astype(np.int32)
    arc = rasr_amd.LatticeArcAligner(ctx)
    tables = rasr_amd.LatticeArcAligner.graphs(graphs)
    al = arc.run(tables, kg, ks, tb, te, off, scores, a.columns)
    torch.cuda.synchronize()
    search = []
    ctx.profile(True)
    for _ in range(3):
        ctx.profile_reset()
        arc.run(tables, kg, ks, tb, te, off, scores, a.columns, **{k: al[k] for k in ("label_dev", "emission_dev", "arc_score_dev", "key_score_dev",
                                                                                      "key_emission_score_dev")})
        torch.cuda.synchronize()
        search.append(ctx.profile_get("arcalign_search")[0])
    ctx.profile(False)
    label_token = np.zeros(1000 + 64, np.int32)
    label_token[1000:] = (np.arange(64) // 3) % 40 + 1   # three states per phoneme; phoneme 1 is the short pause
    modes = {"approximate-phone": (41, label_token, (1,), "label_dev"), "frame-phone": (41, label_token, (1,), "label_dev"),
             "frame-state": (a.columns, None, (0,), "emission_dev")}
    key_acc = torch.empty(a.keys, dtype=torch.float32, device="cuda")
    arc_acc = torch.empty(a.arcs, dtype=torch.float32, device="cuda")
    kernels = ("accuracy_check", "accuracy_runs", "accuracy_table", "accuracy_key", "accuracy_gather")
    with open(a.out, "a") as f:
        for mode, (n_tokens, lt, sp, items) in modes.items():
            acc = rasr_amd.LatticeAccuracy(ctx, mode, n_tokens, lt, sp, 0.3)

            def call():
                info = acc.run(ks, tb, te, al["slot_offsets"], is_ref, al[items], a.segments, key_acc)[1]
                acc.arc_accuracies(arc_key, arc_acc)
                torch.cuda.synchronize()
                return info
            call(), call()
            wall, ms = [], {k: [] for k in kernels}
            for _ in range(a.reps):
                t0 = time.perf_counter()
                info = call()
                wall.append((time.perf_counter() - t0) * 1e3)
            ctx.profile(True)
            for _ in range(a.reps):
                ctx.profile_reset()
                call()
                for k in kernels:
                    ms[k].append(ctx.profile_get(k)[0])
            ctx.profile(False)
            tables_ms = [x + y for x, y in zip(ms["accuracy_runs"], ms["accuracy_table"])]
            line = dict(mode=mode, segments=a.segments, frames=a.frames, keys=a.keys, arcs=a.arcs, reference_keys=n_ref, items=int((te - tb).sum()), reps=a.reps,
                        shape=acc.kernel_shape(), info=info, nonzero_keys=int((key_acc != 0).sum().item()), call_ms=stats(wall), table_kernels_ms=stats(tables_ms),
                        accuracy_kernel_ms=stats(ms["accuracy_key"]), check_kernel_ms=stats(ms["accuracy_check"]), gather_kernel_ms=stats(ms["accuracy_gather"]),
                        arcalign_search_kernel_ms=stats(search))
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))
            acc.close()


if __name__ == "__main__":
    main()
