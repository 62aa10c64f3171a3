"""Measurement (GPU box): the time of a training step through the grid march (render(march=grid, march_grad=True),
csrc/march_bwd.hip) on the two-sphere scene of tests/test_gpu_converge.py, trained --iters iterations
first, at a batch of R = 4096 rays of its training pool.

Step time: the eager train_step (forward_backward + optimizer step) under each setting, rows alternating in one
process after a warm-up of every row, each step between two device events:
  dense 64 + 128          the parent path (coarse + fine, perturbed): the comparison for every ratio
  dense 192               one unperturbed pass of 192 samples through the fine network
  march_grad K in {192, 512} through the scene's own geometry grid, the grid of update()'s defaults and a grid with
                          every cell set (the path's cost when nothing is skipped)
Per row: ms per step (median and spread), the points the field evaluated, and from one extra step with a pair of
device events around every launch the time of nerf_packed_composite_bwd and the sums of the field's forward and
backward launches.

Convergence: from the untrained scene, --train iterations of march_grad training at K = 192 (one pass through the fine
network, the lattice unperturbed), the grid rebuilt by update() every --refresh iterations, next to the dense single
pass of 192 unperturbed samples at the same count and on the same batches; the held-out PSNR of both, rendered as one
dense pass of 192 samples through the fine network.

usage: python tools/march_train_time.py [--steps 20] [--iters 300] [--train 300] [--refresh 50]
                                        [--out profiles/march_train_time.json]
"""
import argparse
import ast
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import indoor_nerf_amd as nerf  # noqa: E402
from indoor_nerf_amd import _lib  # noqa: E402
from forward_only import two_sphere_scene  # noqa: E402
from render_time import geometry_mask  # noqa: E402
from tables import blender_bbox, convergence_rays  # noqa: E402

R = 4096
RESOLUTION = 128


def new_scene(gpu):
    """The untrained two-sphere scene with a training setup of its own: the namespace of two_sphere_scene plus kw (the
    training keywords, in-kernel draws), opt, args and the training pool (ro, rd, rgb)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "f19_converge.npz"))
    c = ast.literal_eval(str(g["config"]))
    s = two_sphere_scene(nerf, gpu, g)
    s.kw = dict(s.kw_test, perturb=1.0)
    s.args = nerf.make_args(lrate=c["lrate"], lrate_decay=c["lrate_decay"], sparse_loss_weight=c["sparsity"],
                            tv_loss_weight=0.0, N_samples=64, N_importance=128, white_bkgd=True)
    s.opt = nerf.RAdam([{"params": list(s.coarse.parameters()) + list(s.fine.parameters()), "weight_decay": 1e-6},
                        {"params": list(s.emb.parameters()), "eps": 1e-15}], lr=c["lrate"], betas=(0.9, 0.99))
    s.pool = [torch.from_numpy(a).to(gpu) for a in convergence_rays()[0]]
    return s


def batches(s, seed, n):
    rng = np.random.RandomState(seed)
    ro, rd, rgb = s.pool
    for _ in range(n):
        idx = torch.from_numpy(rng.choice(ro.shape[0], R, replace=False).astype(np.int64)).to(ro.device)
        yield (ro[idx], rd[idx]), rgb[idx]


def grid_of(s, kind, gpu):
    lo, hi = blender_bbox()
    grid = nerf.OccupancyGrid(s.bbox, resolution=RESOLUTION, device=gpu)
    if kind == "default":
        grid.update(s.emb, [s.fine])
    else:
        grid.set_mask(np.ones((RESOLUTION,) * 3, bool) if kind == "full" else geometry_mask(lo, hi, RESOLUTION))
    return grid


def single_pass(s, **over):
    return dict(s.kw, perturb=0., N_samples=192, N_importance=0, network_fn=s.fine, network_fine=None, **over)


def step_times(a, gpu):
    s = new_scene(gpu)
    s.train(a.iters)
    for m in (s.coarse, s.fine, s.emb):
        m.train()
    rows = [("dense 64+128", s.kw, None), ("dense 192", single_pass(s), None)]
    for kind in ("geometry", "default", "full"):
        grid = grid_of(s, kind, gpu)
        for K in (192, 512):
            rows.append((f"march_grad K={K} {kind}", dict(s.kw, perturb=0., march=grid, march_grad=True, march_samples=K),
                         grid))
    it = [a.iters]

    def step(kw, batch, target):
        it[0] += 1
        return nerf.train_step(batch, target, kw, s.opt, s.args, it[0])

    data = list(batches(s, 7, a.steps + 3))
    for _, kw, _ in rows:      # warm-up: allocations, optimizer state
        for b, t in data[:2]:
            step(kw, b, t)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in rows}
    for b, t in data[2:2 + a.steps]:
        for name, kw, _ in rows:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(kw, b, t)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    out = []
    base = float(np.median(ms["dense 64+128"]))
    for name, kw, grid in rows:
        _lib.set_timing(True)
        try:
            step(kw, *data[-1])
            torch.cuda.synchronize()
            rec = [(n, e0.elapsed_time(e1)) for n, e0, e1 in _lib.timing_records()]
        finally:
            _lib.set_timing(False)
        total = lambda *keys: round(sum(t for n, t in rec if any(k in n for k in keys)), 4)  # noqa: E731
        med = float(np.median(ms[name]))
        row = dict(row=name, ms=round(med, 3), ms_min=round(min(ms[name]), 3), ms_max=round(max(ms[name]), 3),
                   ratio_to_dense=round(med / base, 3),
                   points=grid.last_counts()[0] if grid is not None else R * (192 if "192" in name else 192 + 64),
                   lattice_points=grid.last_counts()[1] if grid is not None else None,
                   packed_composite_bwd_ms=total("nerf_packed_composite_bwd"),
                   composite_bwd_ms=total("nerf_composite_bwd"),
                   field_fwd_ms=total("nerf_hash_encode_fwd", "nerf_mlp_fwd"),
                   field_bwd_ms=total("nerf_mlp_bwd", "nerf_hash_encode_bwd", "nerf_active_rows"),
                   march_lists_ms=total("nerf_march_count", "nerf_march_write"),
                   launches=len(rec), launches_ms=round(sum(t for _, t in rec), 3))
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def convergence(a, gpu):
    out = []
    for mode in ("dense 192", "march_grad K=192, update() every %d" % a.refresh):
        torch.manual_seed(0)
        s = new_scene(gpu)
        grid = nerf.OccupancyGrid(s.bbox, resolution=RESOLUTION, device=gpu) if mode.startswith("march") else None
        fractions = []
        for i, (b, t) in enumerate(batches(s, 100, a.train)):
            if grid is not None and i % a.refresh == 0:
                grid.update(s.emb, [s.fine])
                fractions.append(round(grid.occupied_fraction(), 4))
            kw = single_pass(s) if grid is None else dict(s.kw, perturb=0., march=grid, march_grad=True, march_samples=192)
            nerf.train_step(b, t, kw, s.opt, s.args, i + 1)
        for m in (s.coarse, s.fine, s.emb):
            m.eval()
        psnr = s.psnr_of(*s.ev, N_samples=192, N_importance=0, network_fn=s.fine, network_fine=None)[0]
        row = dict(row="convergence: " + mode, iterations=a.train, held_out_psnr=round(psnr, 3),
                   occupied_fraction_at_refresh=fractions)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--iters", type=int, default=300)
    p.add_argument("--train", type=int, default=300)
    p.add_argument("--refresh", type=int, default=50)
    p.add_argument("--out", default=os.path.join("bench_out", "march_train_time.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("march_train_time: needs a GPU (a time measured elsewhere says nothing)")
    gpu = torch.device("cuda:0")
    rows = step_times(a, gpu) + convergence(a, gpu)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
