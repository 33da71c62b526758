#!/usr/bin/env python3
"""tools/ebw_probe.py -- the EBW corpus pass (amx_ebw_accumulate_dev) at the size of a lattice-training shard: 64 segments of 1000 frames,
2000 arcs of 30 items per segment (3.84 million items per call), dimension 45, 500 mixtures of 1 to 4 densities; every frame offers ten
mixtures to the arcs that cross it, so that a segment folds into about 2 x 10^4 (side, frame, mixture) keys.  Once with one covariance per
density and once with a pooled covariance, whose two chains (numerator, denominator) take every key of their side one after the other.

    python3 tools/ebw_probe.py                 the driver: one child process per step, each under its own `timeout`, in a chain that stops
                                               at the first step that fails; the children's JSON lines are appended to
                                               profiles/ebw_probe.jsonl
    python3 tools/ebw_probe.py --step NAME     one step; prints one JSON line

Times are wall times of whole calls (median of --reps after a warm-up call, the stream drained; they include the upload of the arc and
item tables from pageable host memory) and the kernels' own from the library's event timers (median of --reps calls)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("density_covariances", "pooled_covariance")
KERNELS = ("ebw_resolve", "ebw_sort_items", "ebw_keys", "gmm_best_density", "ebw_sort_lists", "ebw_chains")


def step(a):
    import torch

    import rasr_amd
    from tests import synth
    ctx = rasr_amd.Context(0)
    ctx.use_torch_stream()
    ctx.set_contract(a.contract)
    rng = np.random.Generator(np.random.PCG64(33))
    D, n_seg, per, n_arcs, n_items, n_mix = a.dim, a.segments, a.frames, a.arcs, a.items, a.mixtures
    model = synth.gmm_cart(n_mix, 1, 4, D, seed=33, pooled=a.step == "pooled_covariance")
    gmm = rasr_amd.GmmFeatureScorer(ctx, model)
    ebw = rasr_amd.EbwAccumulator(gmm)
    T, A = n_seg * per, n_seg * n_arcs
    x = torch.from_numpy((rng.standard_normal((T, D)) * 1.5).astype(np.float32)).cuda()
    off = np.arange(n_seg + 1, dtype=np.int64) * per
    arc_off = np.arange(n_seg + 1, dtype=np.int64) * n_arcs
    item_off = np.arange(A + 1, dtype=np.int64) * n_items
    start = rng.integers(0, per - n_items + 1, A)
    frame = (start[:, None] + np.arange(n_items)[None, :]).astype(np.int32)
    offered = rng.integers(0, n_mix, (n_seg, per, a.offered))                      # the mixtures a frame offers
    seg = np.repeat(np.arange(n_seg), n_arcs)
    pick = np.repeat(rng.integers(0, a.offered, (A, n_items // 10 + 1)), 10, axis=1)[:, :n_items]   # runs of ten frames
    emission = offered[seg[:, None], frame, pick].astype(np.int32)
    weight = (rng.uniform(1.0, 2.0, A) * 2.0 ** -rng.integers(0, 20, A) * rng.choice([-1.0, 1.0], A)).astype(np.float32)
    acc = torch.zeros(ebw.accumulator_size(), dtype=torch.float64, device="cuda")
    call = lambda: ebw.accumulate_dev(x, D, off, arc_off, weight, item_off, frame.reshape(-1), emission.reshape(-1), acc)   # noqa: E731

    call()
    torch.cuda.synchronize()
    keys = ebw.last_keys()
    v = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    got = {n: [] for n in KERNELS}
    for _ in range(a.reps):
        ctx.profile_reset()
        call()
        torch.cuda.synchronize()
        for n in KERNELS:
            got[n].append(ctx.profile_get(n)[0])
    ctx.profile(False)
    lists = np.bincount(keys["slot"][keys["slot"] >= 0] * 2 + keys["side"][keys["slot"] >= 0])
    res = dict(step=a.step, contract=a.contract, dim=D, reps=a.reps, segments=n_seg, frames=T, arcs=A, items=A * n_items, mixtures=n_mix,
               densities=int(model["mix_offsets"][-1]), covariances=int(model["variances"].shape[0]), keys=int(len(keys["frame"])),
               keys_per_segment=round(len(keys["frame"]) / n_seg, 1), longest_density_list=int(lists.max()),
               accumulator_doubles=ebw.accumulator_size(), ebw_accumulate_ms=round(float(np.median(v)), 3),
               kernel_ms={n: round(float(np.median(t)), 4) for n, t in got.items()})
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--dim", type=int, default=45)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000, help="per segment")
    ap.add_argument("--arcs", type=int, default=2000, help="per segment")
    ap.add_argument("--items", type=int, default=30, help="per arc")
    ap.add_argument("--mixtures", type=int, default=500)
    ap.add_argument("--offered", type=int, default=10, help="mixtures a frame offers to the arcs that cross it")
    ap.add_argument("--contract", default="fma")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each step of the driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ebw_probe.jsonl"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    lines = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--dim", str(a.dim), "--segments",
               str(a.segments), "--frames", str(a.frames), "--arcs", str(a.arcs), "--items", str(a.items), "--mixtures", str(a.mixtures), "--offered",
               str(a.offered), "--contract", a.contract, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:   # nothing more is started after a step that failed, faulted or ran into its limit
            sys.stderr.write(r.stderr)
            sys.exit("ebw_probe: step %s ended with status %d; stopping" % (name, r.returncode))
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    with open(a.out, "a") as f:
        f.write("\n".join(json.dumps(l) for l in lines) + "\n")
    print("appended to %s" % a.out)


if __name__ == "__main__":
    main()
