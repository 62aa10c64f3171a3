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

With --mlp-precision the same frame, process and method time the bf16 MLP forward instead (render(mlp_precision="bf16"),
csrc/field_x6.hip mlp_fwd_bf16_kernel): the dense 64 + 128 frame, occupancy= alone and march= at 192
lattice samples through the scene's own geometry grid, and march= at 192 through the grid of update()'s defaults, each
in fp32 and in bf16. Per variant: the frame time and its ratio to the fp32 twin's, the PSNR against the target, the
PSNR of the bf16 frame against its fp32 twin, and from one extra frame with a pair of device events around every
launch the time of the MLP forward launches and their share of all launches' time.

With --table-precision the same frame, process and method time the fp16 hash tables instead (render(table_precision=
"fp16"), csrc/hashgrid_half.hip): the four rows of --mlp-precision, each with fp32 and fp16 tables under
both mlp_precision settings. Per variant: the frame time and its ratio to the fp32-table twin's, the PSNR against the
target, the PSNR of the fp16-table frame against its fp32-table twin, and from one extra frame with a pair of device
events around every launch the time of the hash-encoding launches and their share of all launches' time.

With --march-stop the same frame, process and method time stopping opaque rays inside the march instead
(render(march=grid, march_stop=eps), csrc/march.hip nerf_slab_march_*): through the scene's own geometry
grid and the grid of update()'s defaults, at 192 and 512 lattice samples per ray, the march without stop (the parent
path: the comparison for every ratio), march_stop in {1e-2, 1e-3} x march_stop_slab in {32, 64, 128}, and per slab size
march_stop=1e-300, at which nothing terminates (the cost of the slabs alone). Per variant: the points the field
evaluated, the share of rays stopped, the frame time and its ratio to the unstopped twin's, the PSNR against the target
and against the unstopped twin; for the unstopped rows and the 1e-300 rows also the time of every launch from one extra
frame with a pair of device events around each. --iters sets the training iterations of the scene (300: the hazy scene of the other
tables); --opaque-curve 300,1000,... trains the scene afresh at each count in turn, records the dense PSNR and runs the
table at the first count after which the dense PSNR rises by less than 0.1 dB (the last count if none).

With --feature-precision the same frame, process and method time packed bf16 features instead
(render(mlp_precision="bf16", feature_precision="bf16"), csrc/hashgrid_pkbf.hip): the dense frame and
march= at 192 lattice samples through the geometry grid and the default grid, each with mlp_precision="bf16" without
and with the keyword, on fp32 and on fp16 tables. Per variant: the frame time and its ratio to the unpacked twin's,
whether the image has the twin's bits, and from one extra frame with a pair of device events around every launch the
sums of the hash-encoding and of the MLP forward launches.

With --march-sizes the same frame, process and method time device-sized launches instead (render(march=grid,
march_sizes="device")): through both grids at 192 and 512 lattice samples, in the configuration the
keyword needs (march_sh="rays", mlp_precision="bf16", feature_precision="bf16"), the plain march and march_stop in
{1e-2, 1e-3} x march_stop_slab in {32, 64, 128}, each host-sized and device-sized. Per variant: the frame time, its ratio
to the host-sized twin's and (march_stop rows) to the plain march of the same sizing, the time per extra slab, whether
the image has the twin's bits; the plain host-sized rows are timed twice, which gives the run's spread. For the K = 192
plain rows and their (1e-3, slab 32) rows also the launches of a frame, counted and timed.

usage: python tools/render_time.py [--frames 10] [--iters 300] [--size 800] [--out bench_out/render_time.json]
       python tools/render_time.py --early-stop [--out profiles/early_stop_render_time.json]
       python tools/render_time.py --ray-bounds [--out profiles/ray_bounds_render_time.json]
       python tools/render_time.py --march [--out profiles/march_render_time.json]
       python tools/render_time.py --mlp-precision [--out profiles/mlp_bf16_render_time.json]
       python tools/render_time.py --table-precision [--out profiles/table_fp16_render_time.json]
       python tools/render_time.py --march-stop [--iters 300 | --opaque-curve 300,1000,2000,4000]
                                                [--out profiles/march_stop_render_time.json]
       python tools/render_time.py --march-sizes --iters 1000 [--out profiles/march_sizes_render_time.json]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \
           python tools/render_time.py --march-sizes --trace-sizes host|device --iters 100 --frames 5
       python tools/render_time.py --trace-summary HOST_CSV DEVICE_CSV --frames 5 [--out profiles/march_sizes_trace.json]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import indoor_nerf_amd as nerf  # noqa: E402
from forward_only import two_sphere_scene  # noqa: E402
from tables import SCENE_SPHERES, blender_bbox, pose_spherical, procedural_targets  # noqa: E402


def trained_scene(iters=300):
    """The two-sphere scene of tests/test_gpu_converge.py (tests/forward_only.py builds it) trained `iters`
    iterations on seeded batches: (bbox, embedder, coarse net, fine net, render kwargs for evaluation)."""
    if not torch.cuda.is_available():
        raise SystemExit("render_time: needs a GPU (a time measured elsewhere says nothing)")
    s = two_sphere_scene(nerf, torch.device("cuda:0"), np.load(os.path.join(ROOT, "tests", "golden", "f19_converge.npz")))
    s.train(iters)
    return s.bbox, s.emb, s.coarse, s.fine, s.kw_test


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


# ---------------------------------------------------------------- what every mode shares
def setup(a):
    """The trained scene and the frame of the module docstring: bbox, emb, coarse, fine, kw_test, H, W,
    new_grid(kind=None) (an empty grid, or "default": update()'s defaults, "full": every cell set, "geometry": the
    scene's own geometry), frame(over, kw=kw_test) (render()'s result), timed(over) (one frame between two device
    events, ended by a synchronise: ms) and psnr(img) (dB against the procedural target of the same rays)."""
    bbox, emb, coarse, fine, kw_test = trained_scene(a.iters)
    gpu = torch.device("cuda:0")
    lo, hi = blender_bbox()

    def new_grid(kind=None):
        grid = nerf.OccupancyGrid(bbox, resolution=a.resolution, device=gpu)
        if kind == "default":
            grid.update(emb, [coarse, fine])
        elif kind is not None:
            grid.set_mask(np.ones((a.resolution,) * 3, bool) if kind == "full" else geometry_mask(lo, hi, a.resolution))
        return grid

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
    return types.SimpleNamespace(bbox=bbox, emb=emb, coarse=coarse, fine=fine, kw_test=kw_test, H=H, W=W,
                                 new_grid=new_grid, frame=frame, timed=timed, psnr=psnr)


def frame_with_counts(s, over, grid):
    """One untimed frame with every compaction through `grid` recorded: (render()'s result, [(samples per ray,
    points evaluated, points)] per field call)."""
    calls, compact = [], grid.compact

    def recording(pts, viewdirs, spr, raw):
        res = compact(pts, viewdirs, spr, raw)
        calls.append((spr,) + grid.last_counts())
        return res
    grid.compact = recording
    out = s.frame(over)
    del grid.compact
    return out, calls


def pass_shares(calls):
    """The evaluated share of the coarse (64 samples per ray) and the fine (192) pass, from frame_with_counts' calls."""
    share = {}
    for pname, spr in (("coarse", 64), ("fine", 192)):
        n, P = sum(k[1] for k in calls if k[0] == spr), sum(k[2] for k in calls if k[0] == spr)
        share[pname] = {"evaluated": n, "points": P, "share": n / max(1, P)}
    return share


def measure(a, s, variants, report):
    """The protocol: one warm-up of every variant [(name, over)], then a.frames rounds that alternate over them.
    report[name] receives render_ms and speedup_vs_dense; -> the times per variant."""
    for _, over in variants:
        s.timed(over)
    times = {name: [] for name, _ in variants}
    for _ in range(a.frames):
        for name, over in variants:
            times[name].append(s.timed(over))
    for name, v in times.items():
        report[name]["render_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                                     "frames": len(v)}
        report[name]["speedup_vs_dense"] = float(np.median(times["dense"]) / np.median(v))
    return times


def write(a, s, report, **fields):
    out = {"scene": f"two-sphere scene, {a.iters} training iterations", "frame": [s.H, s.W], "chunk": a.chunk,
           "N_samples": 64, "N_importance": 128, "grid_resolution": a.resolution, **fields,
           "variants": report, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


# ---------------------------------------------------------------- the four modes
def main_occupancy(a):
    """The occupancy-grid table: see the module docstring."""
    s = setup(a)
    # the grid with update()'s defaults, and its build time (the first build includes first-launch costs)
    grids = {"grid": s.new_grid()}
    build_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grids["grid"].update(s.emb, [s.coarse, s.fine])
        torch.cuda.synchronize()
        build_ms.append(1e3 * (time.perf_counter() - t0))
    # other builder settings (sigma_thresh, dilate), every cell set (the path's overhead when nothing inside
    # the box is skipped), and the scene's own geometry (what a converged field's grid would approach)
    for th, dil in ((0.0, 0), (0.1, 1), (0.3, 1)):
        grids[f"grid_thresh{th:g}_dilate{dil}"] = s.new_grid().update(s.emb, [s.coarse, s.fine], sigma_thresh=th,
                                                                     dilate=dil)
    grids.update(full_grid=s.new_grid("full"), geometry_grid=s.new_grid("geometry"))

    report = {"dense": {"psnr_db": s.psnr(s.frame({})[0])}}
    for name, grid in grids.items():    # evaluated share per pass: one untimed frame per grid
        out, calls = frame_with_counts(s, dict(occupancy=grid), grid)
        report[name] = {"psnr_db": s.psnr(out[0]), "occupied_fraction": grid.occupied_fraction(),
                        "evaluated": pass_shares(calls), "count_reads_per_frame": len(calls)}
    measure(a, s, [("dense", {})] + [(name, dict(occupancy=grid)) for name, grid in grids.items()], report)
    write(a, s, report, grid_build_ms=build_ms)


def main_early_stop(a):
    """The early-termination table: see the module docstring."""
    s = setup(a)
    grids = {"no grid": None, "default grid": s.new_grid("default"), "geometry grid": s.new_grid("geometry")}
    variants = [("dense", {})]
    desc = {"dense": dict(early_stop=None, early_stop_slab=None, grid=None)}
    for slab in (16, 32, 64):
        name = f"overhead (eps 1e-300), slab {slab}"
        variants.append((name, dict(early_stop=1e-300, early_stop_slab=slab)))
        desc[name] = dict(early_stop=1e-300, early_stop_slab=slab, grid="no grid")
    for gname, grid in grids.items():
        for eps in (1e-2, 1e-3):
            for slab in (16, 32, 64):
                name = f"eps {eps:g}, slab {slab}, {gname}"
                variants.append((name, dict(early_stop=eps, early_stop_slab=slab,
                                            **({} if grid is None else {"occupancy": grid}))))
                desc[name] = dict(early_stop=eps, early_stop_slab=slab, grid=gname)

    # PSNR, evaluated share per pass and count reads: one untimed frame per variant through a query function
    # that records the counts of every field call (it passes the point tensor on untouched)
    report = {}
    nqf = s.kw_test["network_query_fn"]
    for name, over in variants:
        calls, slab = [], desc[name]["early_stop_slab"]

        def recording(pts, viewdirs, fn, calls=calls, slab=slab):
            raw = nqf(pts, viewdirs, fn)
            if slab is not None:
                calls.append((pts.shape[1],) + nerf.last_early_stop_counts())
            return raw
        out = s.frame(over, dict(s.kw_test, network_query_fn=recording))
        report[name] = dict(desc[name], psnr_db=s.psnr(out[0]))
        if calls:
            report[name].update(evaluated=pass_shares(calls),
                                count_reads_per_frame=sum(-(-k[0] // slab) for k in calls),
                                alive_samples_mean={"coarse": float(out[3]["early_stop_samples0"].float().mean()),
                                                    "fine": float(out[3]["early_stop_samples"].float().mean())})
    measure(a, s, variants, report)
    write(a, s, report, grid_occupied_fraction={k: g.occupied_fraction() for k, g in grids.items() if g is not None})


def main_ray_bounds(a):
    """The per-ray sample-bounds table: see the module docstring."""
    s = setup(a)
    grids = {f"{kind} grid": s.new_grid(kind) for kind in ("default", "full", "geometry")}
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
        out = s.frame(over)
        report[name] = {"psnr_db": s.psnr(out[0])}
        if "ray_bounds" in over:
            hit, span = out[3]["ray_hit"], out[3]["ray_span"]
            length = (span[..., 1] - span[..., 0])[hit]
            report[name].update(rays_dropped_share=1.0 - float(hit.float().mean()),
                                span_over_far_minus_near=float(length.mean() / (s.kw_test["far"] - s.kw_test["near"]))
                                if length.numel() else None)
    times = measure(a, s, variants, report)
    write(a, s, report, grid_occupied_fraction={k: g.occupied_fraction() for k, g in grids.items()},
          overhead_ms_full_grid_minus_dense=float(np.median(times["full grid: ray_bounds"]) - np.median(times["dense"])))


def main_march(a):
    """The grid ray-marching table: see the module docstring."""
    s = setup(a)
    grids = {f"{kind} grid": s.new_grid(kind) for kind in ("default", "full", "geometry")}
    variants = [("dense", {})]
    for gname, grid in grids.items():
        variants.append((f"{gname}: occupancy alone", dict(occupancy=grid)))
        variants += [(f"{gname}: march, K = {k}", dict(march=grid, march_samples=k)) for k in (192, 512, 1024)]

    report = {}
    for name, over in variants:         # one untimed frame per variant: PSNR and the points the field evaluated
        if "occupancy" in over:
            out, calls = frame_with_counts(s, over, over["occupancy"])
            n, total = sum(c[1] for c in calls), sum(c[2] for c in calls)
        else:
            out = s.frame(over)
            if "march" in over:
                n, total = int(out[3]["march_samples"].sum()), s.H * s.W * over["march_samples"]
            else:
                n = total = s.H * s.W * (2 * s.kw_test["N_samples"] + s.kw_test["N_importance"])
        report[name] = dict(psnr_db=s.psnr(out[0]), evaluated_points=n, lattice_points=total, share=n / max(1, total))
    measure(a, s, variants, report)
    write(a, s, report, grid_occupied_fraction={k: g.occupied_fraction() for k, g in grids.items()})


def launch_times(s, over):
    """One untimed frame with a pair of device events around every launch (_lib.set_timing): {entry: ms}."""
    from indoor_nerf_amd import _lib
    _lib.set_timing(True)
    try:
        s.frame(over)
        torch.cuda.synchronize()
        ms = {}
        for name, e0, e1 in _lib.timing_records():
            ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1)
    finally:
        _lib.set_timing(False)
    return ms


def main_mlp_precision(a):
    """The bf16 MLP forward table: see the module docstring."""
    s = setup(a)
    geo, default = s.new_grid("geometry"), s.new_grid("default")
    pairs = [("dense", {}), ("geometry grid: occupancy alone", dict(occupancy=geo)),
             ("geometry grid: march, K = 192", dict(march=geo, march_samples=192)),
             ("default grid: march, K = 192", dict(march=default, march_samples=192))]
    variants, twin = [], {}
    for name, over in pairs:
        variants += [(name, over), (name + ", bf16", dict(over, mlp_precision="bf16"))]
        twin[name + ", bf16"] = name

    report, images = {}, {}
    for name, over in variants:         # untimed frames: PSNR, and where the launches' time goes
        images[name] = s.frame(over)[0]
        ms = launch_times(s, over)
        mlp = sum(v for k, v in ms.items() if k.startswith("nerf_mlp_fwd"))
        report[name] = dict(mlp_precision=over.get("mlp_precision", "fp32"), psnr_db=s.psnr(images[name]),
                            mlp_fwd_launch_ms=mlp, all_launches_ms=sum(ms.values()),
                            mlp_share_of_launch_time=mlp / max(sum(ms.values()), 1e-9),
                            launch_ms={k: round(v, 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])})
        if name in twin:
            d = (images[name] - images[twin[name]]).double()
            report[name]["psnr_vs_fp32_twin_db"] = float(-10.0 * torch.log10((d ** 2).mean()))
            report[name]["max_abs_rgb_diff_vs_fp32_twin"] = float(d.abs().max())
            worst = d.abs().reshape(-1, 3).amax(-1)
            report[name]["pixels_off_fp32_twin_by_more_than"] = {str(t): int((worst > t).sum()) for t in (1e-3, 1e-2, 1e-1)}
    times = measure(a, s, variants, report)
    for name, base in twin.items():
        report[name]["time_over_fp32_twin"] = float(np.median(times[name]) / np.median(times[base]))
    write(a, s, report, grid_occupied_fraction={"geometry grid": geo.occupied_fraction(),
                                                "default grid": default.occupied_fraction()})


def main_table_precision(a):
    """The fp16 hash-table table: see the module docstring."""
    s = setup(a)
    geo, default = s.new_grid("geometry"), s.new_grid("default")
    rows = [("dense", {}), ("geometry grid: occupancy alone", dict(occupancy=geo)),
            ("geometry grid: march, K = 192", dict(march=geo, march_samples=192)),
            ("default grid: march, K = 192", dict(march=default, march_samples=192))]
    variants, twin = [], {}
    for mlp in ("fp32", "bf16"):
        for name, over in rows:
            base = name if mlp == "fp32" else name + ", bf16 MLP"
            over = dict(over) if mlp == "fp32" else dict(over, mlp_precision="bf16")
            variants += [(base, over), (base + ", fp16 tables", dict(over, table_precision="fp16"))]
            twin[base + ", fp16 tables"] = base

    report, images = {}, {}
    for name, over in variants:         # untimed frames: PSNR, and where the launches' time goes
        images[name] = s.frame(over)[0]
        ms = launch_times(s, over)
        enc = sum(v for k, v in ms.items() if k.startswith("nerf_hash_encode_fwd"))
        report[name] = dict(mlp_precision=over.get("mlp_precision", "fp32"),
                            table_precision=over.get("table_precision", "fp32"), psnr_db=s.psnr(images[name]),
                            hash_fwd_launch_ms=enc, all_launches_ms=sum(ms.values()),
                            hash_share_of_launch_time=enc / max(sum(ms.values()), 1e-9),
                            launch_ms={k: round(v, 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])})
        if name in twin:
            d = (images[name] - images[twin[name]]).double()
            report[name]["psnr_vs_fp32_table_twin_db"] = float(-10.0 * torch.log10((d ** 2).mean()))
            report[name]["max_abs_rgb_diff_vs_fp32_table_twin"] = float(d.abs().max())
            worst = d.abs().reshape(-1, 3).amax(-1)
            report[name]["pixels_off_fp32_table_twin_by_more_than"] = {str(t): int((worst > t).sum())
                                                                       for t in (1e-3, 1e-2, 1e-1)}
    times = measure(a, s, variants, report)
    for name, base in twin.items():
        report[name]["time_over_fp32_table_twin"] = float(np.median(times[name]) / np.median(times[base]))
    write(a, s, report, grid_occupied_fraction={"geometry grid": geo.occupied_fraction(),
                                                "default grid": default.occupied_fraction()})


def main_feature_precision(a):
    """The packed bf16 feature table: every row renders with mlp_precision="bf16", without and with
    feature_precision="bf16", on fp32 and on fp16 tables; the pair must give the same image bit for bit."""
    s = setup(a)
    geo, default = s.new_grid("geometry"), s.new_grid("default")
    rows = [("dense", {}), ("geometry grid: march, K = 192", dict(march=geo, march_samples=192)),
            ("default grid: march, K = 192", dict(march=default, march_samples=192))]
    variants, twin = [("dense", {})], {}      # the fp32 dense frame: measure()'s reference for speedup_vs_dense
    for tab in ("fp32", "fp16"):
        for name, over in rows:
            base = name + ", bf16 MLP" + ("" if tab == "fp32" else ", fp16 tables")
            over = dict(over, mlp_precision="bf16", **({} if tab == "fp32" else dict(table_precision="fp16")))
            variants += [(base, over), (base + ", bf16 features", dict(over, feature_precision="bf16"))]
            twin[base + ", bf16 features"] = base

    report, images = {}, {}
    for name, over in variants:         # untimed frames: PSNR, and where the launches' time goes
        images[name] = s.frame(over)[0]
        ms = launch_times(s, over)
        enc = sum(v for k, v in ms.items() if k.startswith("nerf_hash_encode_fwd"))
        mlp = sum(v for k, v in ms.items() if k.startswith("nerf_mlp_fwd"))
        report[name] = dict(table_precision=over.get("table_precision", "fp32"),
                            feature_precision=over.get("feature_precision", "fp32"), psnr_db=s.psnr(images[name]),
                            hash_fwd_launch_ms=enc, mlp_fwd_launch_ms=mlp, all_launches_ms=sum(ms.values()),
                            launch_ms={k: round(v, 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])})
        if name in twin:
            report[name]["same_bits_as_unpacked_twin"] = bool(torch.equal(images[name].contiguous().view(torch.int32),
                                                                          images[twin[name]].contiguous().view(torch.int32)))
    times = measure(a, s, variants, report)
    for name, base in twin.items():
        report[name]["time_over_unpacked_twin"] = float(np.median(times[name]) / np.median(times[base]))
    write(a, s, report, grid_occupied_fraction={"geometry grid": geo.occupied_fraction(),
                                                "default grid": default.occupied_fraction()})


def main_march_sh(a):
    """The march_sh table: the march at K = 192 and 512 through both grids, with the fp32-accurate MLP,
    the bf16 MLP and the bf16 MLP on packed features, each without and with march_sh="rays"; the pair must give the
    same image bit for bit. Per row also the time of its write launches and of its MLP launches in one untimed frame."""
    s = setup(a)
    grids = {f"{kind} grid": s.new_grid(kind) for kind in ("geometry", "default")}
    precisions = (("", {}), (", bf16 MLP", dict(mlp_precision="bf16")),
                  (", bf16 MLP, bf16 features", dict(mlp_precision="bf16", feature_precision="bf16")))
    variants, twin = [("dense", {})], {}      # the fp32 dense frame: measure()'s reference for speedup_vs_dense
    for gname, grid in grids.items():
        for K in (192, 512):
            for pname, pover in precisions:
                base = f"{gname}: march, K = {K}{pname}"
                over = dict(march=grid, march_samples=K, **pover)
                variants += [(base, over), (base + ", SH by ray", dict(over, march_sh="rays"))]
                twin[base + ", SH by ray"] = base

    report, images = {}, {}
    for name, over in variants:         # untimed frames: PSNR, evaluated points, and where the launches' time goes
        out = s.frame(over)
        images[name] = out[0]
        ms = launch_times(s, over)
        report[name] = dict(march_sh=over.get("march_sh", "rows"), psnr_db=s.psnr(images[name]),
                            march_write_launch_ms=sum(v for k, v in ms.items() if "march_write" in k),
                            mlp_fwd_launch_ms=sum(v for k, v in ms.items() if k.startswith("nerf_mlp_fwd")),
                            sh_records_launch_ms=ms.get("nerf_ray_sh_records", 0.0), all_launches_ms=sum(ms.values()),
                            launch_ms={k: round(v, 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])})
        if "march" in over:
            report[name]["evaluated_points"] = int(out[3]["march_samples"].sum())
        if name in twin:
            report[name]["same_bits_as_rows_twin"] = bool(torch.equal(images[name].contiguous().view(torch.int32),
                                                                      images[twin[name]].contiguous().view(torch.int32)))
    times = measure(a, s, variants, report)
    for name, base in twin.items():
        report[name]["time_over_rows_twin"] = float(np.median(times[name]) / np.median(times[base]))
        for k in (name, base):
            report[k]["ns_per_evaluated_point"] = float(np.median(times[k]) * 1e6 / max(1, report[k]["evaluated_points"]))
    write(a, s, report, grid_occupied_fraction={k: g.occupied_fraction() for k, g in grids.items()})


def main_march_sizes(a):
    """The march_sizes table: the march at K = 192 and 512 through both grids in the configuration the
    keyword needs (SH by ray, bf16 MLP, packed bf16 features), plain and with march_stop 1e-2 and 1e-3 in slabs of 32,
    64 and 128, each host-sized and device-sized; the pair must give the same image bit for bit. The plain host-sized
    rows are also timed a second time as variants of their own ("again"): the run's spread."""
    s = setup(a)
    fast = dict(march_sh="rays", mlp_precision="bf16", feature_precision="bf16")
    if a.trace_sizes:       # for a kernel trace of its own: frames of one variant and nothing else after the set-up
        over = dict(march=s.new_grid("geometry"), march_samples=192, march_stop=1e-3, march_stop_slab=32, **fast,
                    **({"march_sizes": "device"} if a.trace_sizes == "device" else {}))
        for _ in range(3 + a.frames):
            s.timed(over)
        return
    grids = {f"{kind} grid": s.new_grid(kind) for kind in ("geometry", "default")}
    variants, twin, desc = [("dense", {})], {}, {"dense": {}}
    for gname, grid in grids.items():
        for K in (192, 512):
            rows = [(f"{gname}: march, K = {K}", dict(march=grid, march_samples=K, **fast), None, None)]
            for eps in (1e-2, 1e-3):
                for slab in (32, 64, 128):
                    rows.append((f"{rows[0][0]}, stop {eps:g}, slab {slab}",
                                 dict(rows[0][1], march_stop=eps, march_stop_slab=slab), eps, slab))
            for base, over, eps, slab in rows:
                variants += [(base, over), (base + ", device sizes", dict(over, march_sizes="device"))]
                twin[base + ", device sizes"] = base
                for name in (base, base + ", device sizes"):
                    desc[name] = dict(grid=gname, march_samples=K, march_stop=eps, march_stop_slab=slab,
                                      slabs=1 if slab is None else -(-K // slab), plain=rows[0][0])
            variants.append((rows[0][0] + ", again", rows[0][1]))
            twin[rows[0][0] + ", again"] = rows[0][0]
            desc[rows[0][0] + ", again"] = desc[rows[0][0]]

    report, images = {}, {}
    for name, over in variants:         # one untimed frame per variant: PSNR, evaluated points, the bits
        out = s.frame(over)
        images[name] = out[0]
        report[name] = dict({k: v for k, v in desc[name].items() if k != "plain"},
                            march_sizes=over.get("march_sizes", "host"), psnr_db=s.psnr(out[0]))
        if "march" in over:
            report[name]["evaluated_points"] = int(out[3]["march_samples"].sum())
        if name in twin:
            report[name]["same_bits_as_host_twin"] = bool(torch.equal(images[name].contiguous().view(torch.int32),
                                                                      images[twin[name]].contiguous().view(torch.int32)))
    for name, over in variants:         # where the launches' time goes: the K = 192 rows at slab 32 and the plain ones
        if "march" in over and over["march_samples"] == 192 and over.get("march_stop_slab") in (None, 32) \
                and over.get("march_stop") in (None, 1e-3) and not name.endswith("again"):
            ms = launch_times(s, over)
            report[name].update(all_launches_ms=sum(ms.values()), launches=launch_counts(s, over),
                                launch_ms={k: round(v, 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])})
    times = measure(a, s, variants, report)
    for name, base in twin.items():
        report[name]["time_over_host_twin"] = float(np.median(times[name]) / np.median(times[base]))
    for name in report:
        if desc[name].get("march_stop") is not None:
            sized = ", device sizes" if name.endswith(", device sizes") else ""
            plain = desc[name]["plain"] + sized
            report[name]["time_over_plain_march"] = float(np.median(times[name]) / np.median(times[plain]))
            report[name]["ms_per_extra_slab_vs_plain_march"] = float(
                (np.median(times[name]) - np.median(times[plain])) / max(1, desc[name]["slabs"] - 1))
    write(a, s, report, grid_occupied_fraction={k: g.occupied_fraction() for k, g in grids.items()})


def trace_summary(path, frames, counts_per_frame):
    """A kernel trace (rocprofv3 --kernel-trace, csv) of a --trace-sizes run -> per frame of its last `frames` frames:
    kernels, their summed duration, the span from the first to the last of them, and the idle share of the span. A
    frame is counts_per_frame launches of march_count_kernel (chunks x slabs)."""
    import csv
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path))]
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "march_count_kernel" in r[2]]
    first = starts[-frames * counts_per_frame]
    part = rows[first:]
    busy, span = sum(e - b for b, e, _ in part), max(e for _, e, _ in part) - part[0][0]
    by = {}
    for b, e, k in part:
        k = k.split("(")[0].replace("void ", "").replace("nerf::", "")
        by.setdefault(k, [0, 0.0])
        by[k][0] += 1
        by[k][1] += (e - b) / 1e3
    return {"frames": frames, "kernels_per_frame": len(part) / frames, "kernel_us_per_frame": busy / 1e3 / frames,
            "span_us_per_frame": span / 1e3 / frames, "idle_share_of_span": 1.0 - busy / span,
            "mean_gap_us": (span - busy) / 1e3 / max(1, len(part) - 1),
            "by_kernel_per_frame": {k: {"launches": v[0] / frames, "us": round(v[1] / frames, 1)}
                                    for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])}}


def launch_counts(s, over):
    """The number of launches of one frame, by entry."""
    from indoor_nerf_amd import _lib
    names, call = {}, _lib.call

    def counting(name, *args):
        names[name] = names.get(name, 0) + 1
        return call(name, *args)
    _lib.call = counting
    try:
        s.frame(over)
    finally:
        _lib.call = call
    return names


def opaque_setup(a, counts):
    """The scene trained afresh at each of `counts` in turn until the dense PSNR of the frame stops rising:
    (setup() of the chosen count, {count: dense PSNR})."""
    curve, prev = {}, None
    for c in counts:
        a.iters = c
        s = setup(a)
        curve[c] = s.psnr(s.frame({})[0])
        print(f"march-stop: {c} iterations, dense PSNR {curve[c]:.3f} dB", flush=True)
        if prev is not None and curve[c] - curve[prev[0]] < 0.1:
            a.iters = prev[0]
            return prev[1], curve
        prev = (c, s)
    return prev[1], curve


def main_march_stop(a):
    """The march_stop table: see the module docstring."""
    curve = None
    if a.opaque_curve:
        s, curve = opaque_setup(a, [int(c) for c in a.opaque_curve.split(",")])
    else:
        s = setup(a)
    grids = {f"{kind} grid": s.new_grid(kind) for kind in ("geometry", "default")}
    variants, twin, desc = [("dense", {})], {}, {"dense": {}}
    for gname, grid in grids.items():
        for K in (192, 512):
            base = f"{gname}: march, K = {K}"
            over = dict(march=grid, march_samples=K)
            variants.append((base, over))
            desc[base] = dict(grid=gname, march_samples=K, march_stop=None, march_stop_slab=None)
            for eps in (1e-2, 1e-3, 1e-300):
                for slab in (32, 64, 128):
                    name = f"{base}, stop {eps:g}, slab {slab}"
                    variants.append((name, dict(over, march_stop=eps, march_stop_slab=slab)))
                    twin[name] = base
                    desc[name] = dict(grid=gname, march_samples=K, march_stop=eps, march_stop_slab=slab)

    report, images = {}, {}
    for name, over in variants:         # one untimed frame per variant: PSNR, evaluated points, rays stopped
        out = s.frame(over)
        images[name] = out[0]
        report[name] = dict(desc[name], psnr_db=s.psnr(out[0]))
        if "march" in over:
            K = over["march_samples"]
            n = int(out[3]["march_samples"].sum())
            report[name].update(evaluated_points=n, lattice_points=s.H * s.W * K, share=n / (s.H * s.W * K))
        if name in twin:
            K = over["march_samples"]
            d = (images[name] - images[twin[name]]).double()
            mse = float((d ** 2).mean())
            report[name].update(rays_stopped_share=float((out[3]["march_stop_samples"] < K).float().mean()),
                                slabs=-(-K // over["march_stop_slab"]),
                                psnr_vs_unstopped_twin_db=float("inf") if mse == 0 else -10.0 * float(np.log10(mse)),
                                max_abs_rgb_diff_vs_unstopped_twin=float(d.abs().max()),
                                evaluated_over_unstopped_twin=report[name]["evaluated_points"]
                                / max(1, report[twin[name]]["evaluated_points"]))
    for name, over in variants:         # where the launches' time goes: the unstopped rows and their pure-overhead twins
        if "march" in over and over.get("march_stop") in (None, 1e-300):
            ms = launch_times(s, over)
            report[name].update(all_launches_ms=sum(ms.values()),
                                launch_ms={k: round(v, 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])})
    times = measure(a, s, variants, report)
    for name, base in twin.items():
        report[name]["time_over_unstopped_twin"] = float(np.median(times[name]) / np.median(times[base]))
        report[name]["ms_per_extra_slab_vs_unstopped_twin"] = float(
            (np.median(times[name]) - np.median(times[base])) / max(1, report[name]["slabs"] - 1))
    write(a, s, report, grid_occupied_fraction={k: g.occupied_fraction() for k, g in grids.items()},
          **({} if curve is None else {"dense_psnr_db_by_training_iterations": curve}))


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
    ap.add_argument("--mlp-precision", action="store_true", help="time the bf16 MLP forward (DESIGN.md §17)")
    ap.add_argument("--table-precision", action="store_true", help="time the fp16 hash tables (DESIGN.md §18)")
    ap.add_argument("--march-stop", action="store_true", help="time stopping rays inside the march (DESIGN.md §19)")
    ap.add_argument("--feature-precision", action="store_true", help="time packed bf16 features (DESIGN.md §20)")
    ap.add_argument("--march-sh", action="store_true", help="time SH read through a ray index (DESIGN.md §21)")
    ap.add_argument("--march-sizes", action="store_true", help="time device-sized launches (DESIGN.md §23)")
    ap.add_argument("--trace-sizes", choices=("host", "device"), default=None,
                    help="--march-sizes: only 3 + --frames frames of the geometry grid's K = 192, stop 1e-3, slab 32 row "
                         "with that sizing, to run under a kernel trace")
    ap.add_argument("--opaque-curve", default=None,
                    help="--march-stop: training iteration counts to try in turn until the dense PSNR stops rising")
    ap.add_argument("--trace-summary", nargs=2, metavar=("HOST_CSV", "DEVICE_CSV"), default=None,
                    help="summarise the kernel traces of the two --trace-sizes runs (no GPU needed)")
    a = ap.parse_args()
    if a.trace_summary:
        chunks = -(-a.size * a.size // a.chunk)
        out = {m: trace_summary(p, a.frames, chunks * 6) for m, p in zip(("host", "device"), a.trace_summary)}
        out["variant"] = "geometry grid: march, K = 192, stop 1e-3, slab 32 (6 slabs), SH by ray, bf16 MLP, bf16 features"
        if a.out:
            with open(a.out, "w") as fp:
                json.dump(out, fp, indent=1)
        print(json.dumps(out))
        return
    mode, out = ((main_march_sizes, "profiles/march_sizes_render_time.json") if a.march_sizes else
                 (main_march_sh, "profiles/march_sh_render_time.json") if a.march_sh else
                 (main_feature_precision, "profiles/feat_bf16_render_time.json") if a.feature_precision else
                 (main_march_stop, "profiles/march_stop_render_time.json") if a.march_stop else
                 (main_table_precision, "profiles/table_fp16_render_time.json") if a.table_precision else
                 (main_mlp_precision, "profiles/mlp_bf16_render_time.json") if a.mlp_precision else
                 (main_march, "profiles/march_render_time.json") if a.march else
                 (main_early_stop, "profiles/early_stop_render_time.json") if a.early_stop else
                 (main_ray_bounds, "profiles/ray_bounds_render_time.json") if a.ray_bounds else
                 (main_occupancy, "bench_out/render_time.json"))
    if a.out is None:
        a.out = out
    mode(a)


if __name__ == "__main__":
    main()
