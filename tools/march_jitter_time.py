"""Measurement (GPU box): what jittering the grid march's lattice costs and whether it changes training
(render(march=grid, march_grad=True, march_jitter=True) with perturb = 1, csrc/march.hip). The scene,
the batches and the grids are those of tools/march_train_time.py: the two-sphere scene trained --iters
iterations, R = 4096 rays of its training pool, grids of 128^3.

Launch times: the count and the write of one list, jittered (a host Philox pair) against unjittered, K in {192, 512}
through the geometry grid, the grid of update()'s defaults and a grid with every cell set; rows alternating in one
process after a warm-up, --reps repetitions, a device event pair around each entry's launches (the count entry is
three launches, and its pair also spans the 4-byte host read of the list's length, the same on both sides, so the
differences are the kernels' and the absolute count times are not), medians. The unjittered rows are this commit's
plain entries. The parent commit's figure rides in every row as parent_march_lists_ms: the march_lists_ms of
profiles/march_train_time.json, count + write of one training step, taken there with an event pair around every
launch; the step rows below carry this commit's march_lists_ms taken by that same method, jittered and not.

Step time: the eager train_step under dense 64 + 128 and march_grad at K = 192 and 512 through the geometry grid,
with and without march_jitter, rows alternating as in march_train_time.py.

Convergence: from the untrained scene, --train iterations on the same seeded batches, five runs: dense 64 + 128 with
perturb = 1; the dense single pass of 192 with and without perturb; march_grad at K = 192 with and without
march_jitter, the grid rebuilt by update() every --refresh iterations. Held-out PSNR of each, rendered as one dense
unperturbed pass of 192 samples through the fine network (the 64 + 128 run also as 64 + 128), and the grid's occupied
fractions.

usage: python tools/march_jitter_time.py [--reps 30] [--steps 20] [--iters 300] [--train 1000] [--refresh 50]
                                         [--out bench_out/march_jitter_time.json]
"""
import argparse
import json
import os

import numpy as np
import torch

from march_train_time import R, RESOLUTION, ROOT, _lib, batches, grid_of, new_scene, nerf, single_pass

SEED, OFFSET = (1 << 40) + 12345, (1 << 33) + 7


def parent_lists_ms():
    """march_lists_ms of the parent commit's recorded steps, by 'K=<K> <grid>'."""
    out = {}
    with open(os.path.join(ROOT, "profiles", "march_train_time.json")) as f:
        for line in f:
            row = json.loads(line)
            if row.get("row", "").startswith("march_grad K="):
                out[row["row"][len("march_grad "):]] = row["march_lists_ms"]
    return out


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def launch_times(a, gpu, s):
    from indoor_nerf_amd.render import _pack_rays
    (ro, rd), _ = next(batches(s, 7, 1))
    rays = _pack_rays(0, 0, None, ro, rd, s.kw["near"], s.kw["far"], False, True)
    out, parent = [], parent_lists_ms()
    for kind in ("geometry", "default", "full"):
        grid = grid_of(s, kind, gpu)
        for K in (192, 512):
            ms = {(j, w): [] for j in (False, True) for w in ("count", "write")}
            n = {}
            for rep in range(a.reps + 3):
                for jit in (False, True):
                    jitter = (None, SEED + rep, OFFSET, None) if jit else None
                    tc, (r, t, counts, offsets, _, cnt) = event_ms(lambda: grid._march_count(rays, K, jitter=jitter))
                    tw, _ = event_ms(lambda: grid._march_write(r, t, K, counts, offsets, cnt, True, jitter=jitter))
                    n[jit] = cnt
                    if rep >= 3:      # the count's time includes its 4-byte host read, the same on both sides
                        ms[(jit, "count")].append(tc)
                        ms[(jit, "write")].append(tw)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            extra_us = 1e3 * (med[(True, "count")] + med[(True, "write")] - med[(False, "count")] - med[(False, "write")])
            row = dict(row=f"launches K={K} {kind}", lattice_points=R * K, kept_plain=n[False], kept_jittered=n[True],
                       count_ms=round(med[(False, "count")], 4), write_ms=round(med[(False, "write")], 4),
                       jitter_count_ms=round(med[(True, "count")], 4), jitter_write_ms=round(med[(True, "write")], 4),
                       jitter_extra_us=round(extra_us, 2), parent_march_lists_ms=parent.get(f"K={K} {kind}"),
                       extra_ns_per_lattice_sample=round(1e3 * extra_us / (R * K), 4),
                       extra_ns_per_kept_sample=round(1e3 * extra_us / max(n[True], 1), 4))
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


def step_times(a, gpu, s):
    for m in (s.coarse, s.fine, s.emb):
        m.train()
    grid = grid_of(s, "geometry", gpu)
    rows = [("dense 64+128", s.kw, None)]
    for K in (192, 512):
        kw = dict(s.kw, perturb=0., march=grid, march_grad=True, march_samples=K)
        rows.append((f"march_grad K={K} geometry", kw, grid))
        rows.append((f"march_grad + march_jitter K={K} geometry", dict(kw, perturb=1.0, march_jitter=True), grid))
    it = [a.iters]

    def step(kw, batch, target):
        it[0] += 1
        return nerf.train_step(batch, target, kw, s.opt, s.args, it[0])

    data = list(batches(s, 7, a.steps + 2))
    for _, kw, _ in rows:
        for b, t in data[:2]:
            step(kw, b, t)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in rows}
    points = {}
    for b, t in data[2:2 + a.steps]:
        for name, kw, grid in rows:
            ms[name].append(event_ms(lambda: step(kw, b, t))[0])
            if grid is not None:
                points[name] = grid.last_counts()
    base = float(np.median(ms["dense 64+128"]))
    out, parent = [], parent_lists_ms()
    for name, kw, grid in rows:
        _lib.set_timing(True)      # one extra step with an event pair around every launch, as march_train_time.py
        try:
            step(kw, *data[-1])
            torch.cuda.synchronize()
            rec = [(n, e0.elapsed_time(e1)) for n, e0, e1 in _lib.timing_records()]
        finally:
            _lib.set_timing(False)
        med = float(np.median(ms[name]))
        row = dict(row="step: " + name, ms=round(med, 3), ms_min=round(min(ms[name]), 3), ms_max=round(max(ms[name]), 3),
                   ratio_to_dense=round(med / base, 3), points=points.get(name, (R * 256, None))[0],
                   lattice_points=points.get(name, (None, None))[1],
                   march_lists_ms=round(sum(t for n, t in rec if "march_count" in n or "march_write" in n), 4),
                   parent_march_lists_ms=parent.get(name.split("K=")[-1] and "K=" + name.split("K=")[-1]),
                   launches=len(rec), launches_ms=round(sum(t for _, t in rec), 3))
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def convergence(a, gpu):
    from indoor_nerf_amd.render import manual_seed
    out = []
    modes = [("dense 64+128 perturb=1", None, None), ("dense 192 perturb=0", 0., None), ("dense 192 perturb=1", 1., None),
             ("march_grad K=192", 0., False), ("march_grad + march_jitter K=192", 1., True)]
    for mode, perturb, jitter in modes:
        torch.manual_seed(0)
        manual_seed(0)
        s = new_scene(gpu)
        grid = nerf.OccupancyGrid(s.bbox, resolution=RESOLUTION, device=gpu) if jitter is not None else None
        fractions = []
        for i, (b, t) in enumerate(batches(s, 100, a.train)):
            if grid is not None and i % a.refresh == 0:
                grid.update(s.emb, [s.fine])
                fractions.append(round(grid.occupied_fraction(), 4))
            if perturb is None:
                kw = s.kw
            elif grid is None:
                kw = dict(single_pass(s), perturb=perturb)
            else:
                kw = dict(s.kw, perturb=perturb, march=grid, march_grad=True, march_jitter=jitter,
                          march_samples=192)
            nerf.train_step(b, t, kw, s.opt, s.args, i + 1)
        for m in (s.coarse, s.fine, s.emb):
            m.eval()
        psnr = s.psnr_of(*s.ev, N_samples=192, N_importance=0, network_fn=s.fine, network_fine=None)[0]
        row = dict(row="convergence: " + mode, iterations=a.train, held_out_psnr_192=round(psnr, 3),
                   occupied_fraction_at_refresh=fractions)
        if perturb is None:
            row["held_out_psnr_64_128"] = round(s.psnr_of(*s.ev)[0], 3)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--iters", type=int, default=300)
    p.add_argument("--train", type=int, default=1000)
    p.add_argument("--refresh", type=int, default=50)
    p.add_argument("--out", default=os.path.join("bench_out", "march_jitter_time.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("march_jitter_time: needs a GPU (a time measured elsewhere says nothing)")
    gpu = torch.device("cuda:0")
    s = new_scene(gpu)
    s.train(a.iters)
    rows = launch_times(a, gpu, s) + step_times(a, gpu, s) + (convergence(a, gpu) if a.train > 0 else [])
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
