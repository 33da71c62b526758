#!/usr/bin/env python3
"""tools/arcalign_probe.py -- the lattice word-arc alignments (amx_arcalign_run_dev) at the size of a lattice-training batch: 64 segments of
1000 frames on 10 000 columns, about 60 000 distinct keys drawn by 128 000 arcs, left-to-right graphs of 9-60 states (a cache of 2000),
windows of 10-80 frames, default pruning (the passes that repeat an outcome are counted, not run).

Beside it the only route there was before: keys laid out as disjoint segments on a copied matrix through amx_align_viterbi_dev.  The copy
of ALL keys' rows would be 100 GB at this width, so that route runs on every --baseline-every-th key (its own keys per second are what
compares); the copy itself is not timed.  The two alternate in one process, --reps times after a warm-up of each; medians are reported.

    python3 tools/arcalign_probe.py        appends one JSON line to profiles/arcalign_probe.jsonl

Per route: the call's wall time with the stream drained, the search kernel from the library's event timers (taken in calls of their own),
keys per second of the call, and the share of passes counted but not run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(v):
    return float(np.median(np.array(v, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--columns", type=int, default=10000)
    ap.add_argument("--keys", type=int, default=60000)
    ap.add_argument("--arcs", type=int, default=128000)
    ap.add_argument("--graphs", type=int, default=2000)
    ap.add_argument("--baseline-every", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arcalign_probe.jsonl"))
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
    kg, ks = rng.integers(0, a.graphs, a.keys).astype(np.int32), rng.integers(0, a.segments, a.keys).astype(np.int32)
    T = np.maximum(rng.integers(10, 81, a.keys), (states[kg] + 1) // 2 + 1).astype(np.int32)   # long enough for the graph's shortest path
    tb = (rng.random(a.keys) * (a.frames - T + 1)).astype(np.int32)
    arc_key = np.concatenate([np.arange(a.keys), rng.integers(0, a.keys, a.arcs - a.keys)]).astype(np.int32)
    arc_score = torch.empty(a.arcs, dtype=torch.float32, device="cuda")
    arc = rasr_amd.LatticeArcAligner(ctx)
    tables = rasr_amd.LatticeArcAligner.graphs(graphs)
    # the baseline's keys: disjoint segments of a copied matrix, one graph each
    sub = np.arange(0, a.keys, a.baseline_every)
    rows = np.concatenate([off[ks[k]] + tb[k] + np.arange(T[k]) for k in sub])
    copied = scores[torch.from_numpy(rows).cuda()]
    sub_off = np.concatenate([[0], np.cumsum(T[sub])]).astype(np.int64)
    sub_tables = rasr_amd.ViterbiAligner.graphs([graphs[kg[k]] for k in sub])
    vit = rasr_amd.ViterbiAligner(ctx)
    out = {}

    def run_arc():
        out.update(arc.run(tables, kg, ks, tb, tb + T, off, scores, a.columns, **{k: out.get(k) for k in ("label_dev", "emission_dev", "arc_score_dev",
                                                                                                           "key_score_dev", "key_emission_score_dev")}))
        arc.arc_scores_dev(arc_key, "alignment", arc_score)
        return out["results"], out["counters"]

    def run_vit():
        r = vit.align(sub_off, sub_tables, copied, a.columns, **{k: out.get("v_" + k) for k in ("label_dev", "emission_dev", "arc_score_dev")})
        out.update(v_label_dev=r[0], v_emission_dev=r[1], v_arc_score_dev=r[2])
        return r[3], r[4]

    routes = dict(arcalign=(run_arc, "arcalign_search", a.keys), viterbi_on_copy=(run_vit, "align_search", len(sub)))
    wall, kernel, last = {n: [] for n in routes}, {n: [] for n in routes}, {}
    for n, (fn, _, _) in routes.items():
        fn()
        torch.cuda.synchronize()
    for _ in range(a.reps):
        for n, (fn, _, _) in routes.items():
            t0 = time.perf_counter()
            last[n] = fn()
            torch.cuda.synchronize()
            wall[n].append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    for _ in range(a.reps):
        for n, (fn, name, _) in routes.items():
            ctx.profile_reset()
            fn()
            torch.cuda.synchronize()
            kernel[n].append(ctx.profile_get(name)[0])
    ctx.profile(False)
    agree = sum(x["reached"] == y["reached"] and x["score"] == y["score"] for x, y in zip(last["viterbi_on_copy"][0], [last["arcalign"][0][k] for k in sub]))
    line = dict(segments=a.segments, frames=a.frames, columns=a.columns, graphs=a.graphs, keys=a.keys, arcs=a.arcs, key_frames=int(T.sum()),
                key_cells=int((T * states[kg]).sum()), reps=a.reps, launches=arc.last_launches(), shape_narrow=arc.kernel_shape(False),
                reached=sum(r["reached"] for r in last["arcalign"][0]), baseline_keys=len(sub), baseline_scores_agree=int(agree))
    for n, (_, _, n_keys) in routes.items():
        c = last[n][1]
        line[n] = dict(call_ms=round(median(wall[n]), 3), call_ms_min_max=[round(min(wall[n]), 3), round(max(wall[n]), 3)], kernel_ms=round(median(kernel[n]), 3),
                       keys_per_s=round(n_keys / (median(wall[n]) * 1e-3)), passes_run=c[1], passes_counted=c[2],
                       share_counted=round(c[2] / max(c[1] + c[2], 1), 4))
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
