"""Measurement (GPU box): forward-only render time of one 800 x 800 frame of the trained two-sphere
scene (tests/test_gpu_converge.py's setup, 64 coarse + 128 importance samples, chunk 32768), dense and
through an occupancy grid (occupancy.OccupancyGrid).

Dense and grid frames alternate in one process after a warm-up of both; each frame sits between two
device events and ends in a synchronise. Also reported: the grid's build time, its occupied fraction,
the share of the points each pass evaluates and the PSNR of every render against the procedural target.
Besides the grid of update()'s defaults the same frame is timed through grids of other builder settings,
through a grid with every cell set (the path's overhead when nothing inside the box is skipped: two
compaction launches and one 4-byte read of the count per field call, and no coarse-feature reuse) and
through the grid of the scene's own geometry (what a converged field's grid would approach).

With --early-stop the same frame, process and method time early ray termination instead (early_stop.py,
DESIGN.md §14): early_stop in {1e-2, 1e-3} x early_stop_slab in {16, 32, 64}, each without a grid, with
the grid of update()'s defaults and with the scene's own geometry grid, and per slab size a row with a
threshold so small that nothing terminates (1e-300: the path's pure overhead — the compaction of every
slab, one 4-byte read of the count per slab, no coarse-feature reuse). The dense frame of the unchanged
path is the baseline.

With --ray-bounds the same frame, process and method time per-ray sample bounds instead (render(ray_bounds=grid),
csrc/ray_span.hip): through the grid of update()'s defaults, a grid with every cell set (the
path's pure overhead: the span and gather launches and one 4-byte read per frame; every ray of this frame
meets the box) and the scene's own geometry grid, each alone, on top of occupancy=, of early_stop= (1e-3, slabs
of 32) and of both, next to occupancy= alone through the same grid; and, through the geometry grid, with half
the samples (32 + 64) placed inside the spans. Per variant: the share of rays dropped, the mean span over
far - near, the frame time and the PSNR.

With --march the same frame, process and method time grid ray marching instead (render(march=grid), csrc/march.hip,
DESIGN.md §16): the dense 64 + 128 frame of the unchanged path, occupancy= alone and march= at 192, 512 and 1024
lattice samples per ray, each through the grid of update()'s defaults, a grid with every cell set and the scene's
own geometry grid. Per variant: the frame time, the points the field evaluated and the PSNR.

usage: python tools/render_time.py [--frames 10] [--iters 300] [--size 800] [--out bench_out/render_time.json]
       python tools/render_time.py --early-stop [--out profiles/early_stop_render_time.json]
       python tools/render_time.py --ray-bounds [--out profiles/ray_bounds_render_time.json]
       python tools/render_time.py --march [--out profiles/march_render_time.json]
"""
import argparse
import ast
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import indoor_nerf_amd as nerf  # noqa: E402
from tables import (SCENE_SPHERES, blender_bbox, closed_form_table, convergence_rays, pose_spherical,  # noqa: E402
                    procedural_targets)


def trained_scene(iters=300):
    """The two-sphere scene of tests/test_gpu_converge.py trained `iters` iterations on seeded batches:
    (bbox, embedder, coarse net, fine net, render kwargs for evaluation)."""
    if not torch.cuda.is_available():
        raise SystemExit("render_time: needs a GPU (a time measured elsewhere says nothing)")
    gpu = torch.device("cuda:0")
    g = np.load(os.path.join(ROOT, "tests", "golden", "f19_converge.npz"))
    c = ast.literal_eval(str(g["config"]))
    lo, hi = blender_bbox()
    bbox = (torch.from_numpy(lo), torch.from_numpy(hi))
    emb = nerf.HashEmbedder(bbox, finest_resolution=1024).to(gpu)
    table = closed_form_table(scale=c["table_scale"], salt=c["table_salt"])

    def net(prefix):
        m = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                           input_ch=32, input_ch_views=16).to(gpu)
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.copy_(torch.from_numpy(g[prefix + k.replace(".", "_")]))
        return m

    coarse, fine = net("coarse0_"), net("fine0_")
    with torch.no_grad():
        for i, e in enumerate(emb.embeddings):
            e.weight.copy_(torch.from_numpy(table[i]))
    sh = nerf.SHEncoder()
    nqf = lambda inputs, viewdirs, fn: nerf.run_network(inputs, viewdirs, fn, emb, sh)  # noqa: E731
    kw = dict(network_query_fn=nqf, perturb=1.0, N_importance=128, network_fine=fine, N_samples=64,
              network_fn=coarse, embed_fn=emb, use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0,
              predict_normals=False, ndc=False, lindisp=False, near=2.0, far=6.0, pytest=True)
    kw_test = dict(kw, perturb=0.0, pytest=False)
    args = nerf.make_args(lrate=c["lrate"], lrate_decay=c["lrate_decay"], sparse_loss_weight=c["sparsity"],
                          tv_loss_weight=0.0, N_samples=64, N_importance=128, white_bkgd=True)
    (ro, rd, rgb), _, _ = convergence_rays()
    ro, rd, rgb = (torch.from_numpy(x).to(gpu) for x in (ro, rd, rgb))
    opt = nerf.RAdam([{"params": list(coarse.parameters()) + list(fine.parameters()), "weight_decay": 1e-6},
                      {"params": list(emb.parameters()), "eps": 1e-15}], lr=c["lrate"], betas=(0.9, 0.99))
    rng = np.random.RandomState(100)
    for it in range(1, iters + 1):
        idx = torch.from_numpy(rng.choice(ro.shape[0], c["R"], replace=False).astype(np.int64)).to(gpu)
        nerf.train_step((ro[idx], rd[idx]), rgb[idx], kw, opt, args, it)
    for m in (coarse, fine, emb):
        m.eval()

    return bbox, emb, coarse, fine, kw_test


def geometry_mask(lo, hi, res):
    """Cells of the procedural scene itself: those whose centre lies within a sphere's radius plus one
    cell diagonal of its centre (tables.SCENE_SPHERES) — the grid a converged field would approach."""
    cell = (hi - lo) / res
    axes = [lo[a] + (np.arange(res) + 0.5) * cell[a] for a in range(3)]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    mask = np.zeros((res, res, res), bool)
    for c, r in SCENE_SPHERES:
        mask |= np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) <= r + float(np.linalg.norm(cell))
    return mask


def main_early_stop(a):
    """The early-termination table: see the module docstring."""
    bbox, emb, coarse, fine, kw_test = trained_scene(a.iters)
    gpu = torch.device("cuda:0")
    lo, hi = blender_bbox()
    grids = {"no grid": None,
             "default grid": nerf.OccupancyGrid(bbox, resolution=a.resolution, device=gpu).update(emb, [coarse, fine]),
             "geometry grid": nerf.OccupancyGrid(bbox, resolution=a.resolution, device=gpu)}
    grids["geometry grid"].set_mask(geometry_mask(lo, hi, a.resolution))

    H = W = a.size
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    pose = torch.from_numpy(pose_spherical(np.linspace(-180, 180, 101)[34], -30.0, 4.0311))[:3, :4].to(gpu)

    def frame(over, kw=kw_test):
        with torch.no_grad():
            return nerf.render(H, W, K, chunk=a.chunk, c2w=pose, **dict(kw, **over))

    def timed(over):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frame(over)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ro_np, rd_np = nerf.get_rays_np(H, W, K, pose.cpu().numpy())
    target = torch.from_numpy(procedural_targets(np.ascontiguousarray(ro_np.reshape(-1, 3), np.float32),
                                                 np.ascontiguousarray(rd_np.reshape(-1, 3), np.float32))).to(gpu)
    psnr = lambda img: float(-10.0 * torch.log10(((img.reshape(-1, 3) - target) ** 2).mean()))  # noqa: E731

    variants = [("dense", {}, dict(early_stop=None, early_stop_slab=None, grid=None))]
    for slab in (16, 32, 64):
        variants.append((f"overhead (eps 1e-300), slab {slab}", dict(early_stop=1e-300, early_stop_slab=slab),
                         dict(early_stop=1e-300, early_stop_slab=slab, grid="no grid")))
    for gname, grid in grids.items():
        for eps in (1e-2, 1e-3):
            for slab in (16, 32, 64):
                over = dict(early_stop=eps, early_stop_slab=slab, **({} if grid is None else {"occupancy": grid}))
                variants.append((f"eps {eps:g}, slab {slab}, {gname}", over,
                                 dict(early_stop=eps, early_stop_slab=slab, grid=gname)))

    # PSNR, evaluated share per pass and count reads: one untimed frame per variant through a query function
    # that records the counts of every field call (it passes the point tensor on untouched)
    report = {}
    nqf = kw_test["network_query_fn"]
    for name, over, desc in variants:
        calls = []

        def recording(pts, viewdirs, fn, calls=calls, slab=desc["early_stop_slab"]):
            raw = nqf(pts, viewdirs, fn)
            if slab is not None:
                calls.append((pts.shape[1], -(-pts.shape[1] // slab)) + nerf.last_early_stop_counts())
            return raw
        out = frame(over, dict(kw_test, network_query_fn=recording))
        report[name] = dict(desc, psnr_db=psnr(out[0]))
        if calls:
            share = {}
            for pname, spr in (("coarse", 64), ("fine", 192)):
                n, P = sum(k[2] for k in calls if k[0] == spr), sum(k[3] for k in calls if k[0] == spr)
                share[pname] = {"evaluated": n, "points": P, "share": n / max(1, P)}
            report[name].update(evaluated=share, count_reads_per_frame=sum(k[1] for k in calls),
                                alive_samples_mean={"coarse": float(out[3]["early_stop_samples0"].float().mean()),
                                                    "fine": float(out[3]["early_stop_samples"].float().mean())})

    for _, over, _ in variants:         # warm-up of every variant
        timed(over)
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.frames):           # alternating
        for name, over, _ in variants:
            times[name].append(timed(over))
    for name, v in times.items():
        report[name]["render_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                                     "frames": len(v)}
        report[name]["speedup_vs_dense"] = float(np.median(times["dense"]) / np.median(v))
    out = {"scene": f"two-sphere scene, {a.iters} training iterations", "frame": [H, W], "chunk": a.chunk,
           "N_samples": 64, "N_importance": 128, "grid_resolution": a.resolution,
           "grid_occupied_fraction": {k: g.occupied_fraction() for k, g in grids.items() if g is not None},
           "variants": report, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


def main_ray_bounds(a):
    """The per-ray sample-bounds table: see the module docstring."""
    bbox, emb, coarse, fine, kw_test = trained_scene(a.iters)
    gpu = torch.device("cuda:0")
    lo, hi = blender_bbox()
    new_grid = lambda: nerf.OccupancyGrid(bbox, resolution=a.resolution, device=gpu)  # noqa: E731
    grids = {"default grid": new_grid().update(emb, [coarse, fine]), "full grid": new_grid(),
             "geometry grid": new_grid()}
    grids["full grid"].set_mask(np.ones((a.resolution,) * 3, bool))
    grids["geometry grid"].set_mask(geometry_mask(lo, hi, a.resolution))

    H = W = a.size
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    pose = torch.from_numpy(pose_spherical(np.linspace(-180, 180, 101)[34], -30.0, 4.0311))[:3, :4].to(gpu)

    def frame(over):
        with torch.no_grad():
            return nerf.render(H, W, K, chunk=a.chunk, c2w=pose, **dict(kw_test, **over))

    def timed(over):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frame(over)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ro_np, rd_np = nerf.get_rays_np(H, W, K, pose.cpu().numpy())
    target = torch.from_numpy(procedural_targets(np.ascontiguousarray(ro_np.reshape(-1, 3), np.float32),
                                                 np.ascontiguousarray(rd_np.reshape(-1, 3), np.float32))).to(gpu)
    psnr = lambda img: float(-10.0 * torch.log10(((img.reshape(-1, 3) - target) ** 2).mean()))  # noqa: E731

    ert = dict(early_stop=1e-3, early_stop_slab=32)
    variants = [("dense", {})]
    for gname, grid in grids.items():
        variants += [(f"{gname}: occupancy alone", dict(occupancy=grid)),
                     (f"{gname}: ray_bounds", dict(ray_bounds=grid)),
                     (f"{gname}: ray_bounds + occupancy", dict(ray_bounds=grid, occupancy=grid)),
                     (f"{gname}: ray_bounds + early_stop", dict(ray_bounds=grid, **ert)),
                     (f"{gname}: ray_bounds + occupancy + early_stop", dict(ray_bounds=grid, occupancy=grid, **ert))]
    half = dict(N_samples=32, N_importance=64)
    geo = grids["geometry grid"]
    variants += [("32 + 64 samples, unbounded", half),
                 ("geometry grid: ray_bounds, 32 + 64 samples", dict(ray_bounds=geo, **half)),
                 ("geometry grid: ray_bounds + occupancy, 32 + 64 samples", dict(ray_bounds=geo, occupancy=geo, **half))]

    report = {}
    for name, over in variants:         # one untimed frame per variant: PSNR, rays dropped, span length
        out = frame(over)
        report[name] = {"psnr_db": psnr(out[0])}
        if "ray_bounds" in over:
            hit, span = out[3]["ray_hit"], out[3]["ray_span"]
            length = (span[..., 1] - span[..., 0])[hit]
            report[name].update(rays_dropped_share=1.0 - float(hit.float().mean()),
                                span_over_far_minus_near=float(length.mean() / (kw_test["far"] - kw_test["near"]))
                                if length.numel() else None)
    for _, over in variants:            # warm-up of every variant
        timed(over)
    times = {name: [] for name, _ in variants}
    for _ in range(a.frames):           # alternating
        for name, over in variants:
            times[name].append(timed(over))
    for name, v in times.items():
        report[name]["render_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                                     "frames": len(v)}
        report[name]["speedup_vs_dense"] = float(np.median(times["dense"]) / np.median(v))
    out = {"scene": f"two-sphere scene, {a.iters} training iterations", "frame": [H, W], "chunk": a.chunk,
           "N_samples": 64, "N_importance": 128, "grid_resolution": a.resolution,
           "grid_occupied_fraction": {k: g.occupied_fraction() for k, g in grids.items()},
           "overhead_ms_full_grid_minus_dense": float(np.median(times["full grid: ray_bounds"]) -
                                                      np.median(times["dense"])),
           "variants": report, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


def main_march(a):
    """The grid ray-marching table: see the module docstring."""
    bbox, emb, coarse, fine, kw_test = trained_scene(a.iters)
    gpu = torch.device("cuda:0")
    lo, hi = blender_bbox()
    new_grid = lambda: nerf.OccupancyGrid(bbox, resolution=a.resolution, device=gpu)  # noqa: E731
    grids = {"default grid": new_grid().update(emb, [coarse, fine]), "full grid": new_grid(),
             "geometry grid": new_grid()}
    grids["full grid"].set_mask(np.ones((a.resolution,) * 3, bool))
    grids["geometry grid"].set_mask(geometry_mask(lo, hi, a.resolution))

    H = W = a.size
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    pose = torch.from_numpy(pose_spherical(np.linspace(-180, 180, 101)[34], -30.0, 4.0311))[:3, :4].to(gpu)

    def frame(over):
        with torch.no_grad():
            return nerf.render(H, W, K, chunk=a.chunk, c2w=pose, **dict(kw_test, **over))

    def timed(over):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frame(over)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ro_np, rd_np = nerf.get_rays_np(H, W, K, pose.cpu().numpy())
    target = torch.from_numpy(procedural_targets(np.ascontiguousarray(ro_np.reshape(-1, 3), np.float32),
                                                 np.ascontiguousarray(rd_np.reshape(-1, 3), np.float32))).to(gpu)
    psnr = lambda img: float(-10.0 * torch.log10(((img.reshape(-1, 3) - target) ** 2).mean()))  # noqa: E731

    variants = [("dense", {})]
    for gname, grid in grids.items():
        variants.append((f"{gname}: occupancy alone", dict(occupancy=grid)))
        variants += [(f"{gname}: march, K = {k}", dict(march=grid, march_samples=k)) for k in (192, 512, 1024)]

    report = {}
    for name, over in variants:         # one untimed frame per variant: PSNR and the points the field evaluated
        grid, calls = over.get("occupancy"), []
        if grid is not None:
            compact = grid.compact

            def recording(pts, viewdirs, spr, raw, grid=grid, compact=compact, calls=calls):
                res = compact(pts, viewdirs, spr, raw)
                calls.append(grid.last_counts())
                return res
            grid.compact = recording
        out = frame(over)
        if grid is not None:
            del grid.compact
        report[name] = {"psnr_db": psnr(out[0])}
        if "march" in over:
            n, total = int(out[3]["march_samples"].sum()), H * W * over["march_samples"]
        elif grid is not None:
            n, total = sum(c[0] for c in calls), sum(c[1] for c in calls)
        else:
            n = total = H * W * (kw_test["N_samples"] + kw_test["N_samples"] + kw_test["N_importance"])
        report[name].update(evaluated_points=n, lattice_points=total, share=n / max(1, total))
    for _, over in variants:            # warm-up of every variant
        timed(over)
    times = {name: [] for name, _ in variants}
    for _ in range(a.frames):           # alternating
        for name, over in variants:
            times[name].append(timed(over))
    for name, v in times.items():
        report[name]["render_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                                     "frames": len(v)}
        report[name]["speedup_vs_dense"] = float(np.median(times["dense"]) / np.median(v))
    out = {"scene": f"two-sphere scene, {a.iters} training iterations", "frame": [H, W], "chunk": a.chunk,
           "N_samples": 64, "N_importance": 128, "grid_resolution": a.resolution,
           "grid_occupied_fraction": {k: g.occupied_fraction() for k, g in grids.items()},
           "variants": report, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--early-stop", action="store_true", help="time early ray termination (DESIGN.md §14)")
    ap.add_argument("--ray-bounds", action="store_true", help="time per-ray sample bounds (DESIGN.md §15)")
    ap.add_argument("--march", action="store_true", help="time grid ray marching (DESIGN.md §16)")
    a = ap.parse_args()
    if a.out is None:
        a.out = ("profiles/early_stop_render_time.json" if a.early_stop else
                 "profiles/ray_bounds_render_time.json" if a.ray_bounds else
                 "profiles/march_render_time.json" if a.march else "bench_out/render_time.json")
    if a.march:
        return main_march(a)
    if a.early_stop:
        return main_early_stop(a)
    if a.ray_bounds:
        return main_ray_bounds(a)
    bbox, emb, coarse, fine, kw_test = trained_scene(a.iters)
    gpu = torch.device("cuda:0")
    lo, hi = blender_bbox()
    new_grid = lambda: nerf.OccupancyGrid(bbox, resolution=a.resolution, device=gpu)  # noqa: E731

    # the grid with update()'s defaults, and its build time (the first build includes first-launch costs)
    grids = {"grid": new_grid()}
    build_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grids["grid"].update(emb, [coarse, fine])
        torch.cuda.synchronize()
        build_ms.append(1e3 * (time.perf_counter() - t0))
    # other builder settings (sigma_thresh, dilate), every cell set (the path's overhead when nothing inside
    # the box is skipped), and the scene's own geometry (what a converged field's grid would approach)
    for th, dil in ((0.0, 0), (0.1, 1), (0.3, 1)):
        grids[f"grid_thresh{th:g}_dilate{dil}"] = new_grid().update(emb, [coarse, fine], sigma_thresh=th, dilate=dil)
    grids["full_grid"] = new_grid()
    grids["full_grid"].set_mask(np.ones((a.resolution,) * 3, bool))
    grids["geometry_grid"] = new_grid()
    grids["geometry_grid"].set_mask(geometry_mask(lo, hi, a.resolution))

    H = W = a.size
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    pose = torch.from_numpy(pose_spherical(np.linspace(-180, 180, 101)[34], -30.0, 4.0311))[:3, :4].to(gpu)

    def frame(occupancy):
        with torch.no_grad():
            return nerf.render(H, W, K, chunk=a.chunk, c2w=pose, **dict(kw_test, occupancy=occupancy))[0]

    def timed(occupancy):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frame(occupancy)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # PSNR of every render against the procedural target of the same rays
    ro_np, rd_np = nerf.get_rays_np(H, W, K, pose.cpu().numpy())
    target = torch.from_numpy(procedural_targets(np.ascontiguousarray(ro_np.reshape(-1, 3), np.float32),
                                                 np.ascontiguousarray(rd_np.reshape(-1, 3), np.float32))).to(gpu)
    psnr = lambda img: float(-10.0 * torch.log10(((img.reshape(-1, 3) - target) ** 2).mean()))  # noqa: E731
    report = {"dense": {"psnr_db": psnr(frame(None))}}

    # evaluated share per pass: one untimed frame per grid with the compaction's counts recorded
    for name, grid in grids.items():
        calls = []
        compact = grid.compact

        def recording(pts, viewdirs, spr, raw, grid=grid, compact=compact, calls=calls):
            out = compact(pts, viewdirs, spr, raw)
            calls.append((spr,) + grid.last_counts())
            return out
        grid.compact = recording
        img = frame(grid)
        del grid.compact
        share = {}
        for pname, spr in (("coarse", 64), ("fine", 192)):
            n, P = sum(k[1] for k in calls if k[0] == spr), sum(k[2] for k in calls if k[0] == spr)
            share[pname] = {"evaluated": n, "points": P, "share": n / max(1, P)}
        report[name] = {"psnr_db": psnr(img), "occupied_fraction": grid.occupied_fraction(), "evaluated": share,
                        "count_reads_per_frame": len(calls)}

    variants = [("dense", None)] + list(grids.items())
    for _, occ in variants:             # warm-up of every variant
        timed(occ)
    times = {name: [] for name, _ in variants}
    for _ in range(a.frames):           # alternating
        for name, occ in variants:
            times[name].append(timed(occ))
    for name, v in times.items():
        report[name]["render_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                                     "frames": len(v)}
        report[name]["speedup_vs_dense"] = float(np.median(times["dense"]) / np.median(v))
    out = {"scene": f"two-sphere scene, {a.iters} training iterations", "frame": [H, W], "chunk": a.chunk,
           "N_samples": 64, "N_importance": 128, "grid_resolution": a.resolution,
           "grid_build_ms": build_ms, "variants": report, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
