"""What the forward-only render tests share (test_gpu_occupancy.py, test_gpu_early_stop.py, test_gpu_ray_bounds.py,
test_gpu_march.py, test_gpu_point_compact.py): the cell rule and the masks in NumPy, the bit
comparisons, the drivers of the two compaction entries, the test scene and the trained two-sphere scene.

The test scene (build_scene): that of test_gpu_render_path.py (blender_bbox, tables uniform +-0.05, finest_res
512, 32 + 32 samples, white background, eval mode), two 12 x 16 frames from (-40 deg, 75 deg) at -30 deg, radius 4,
with near = 0.5, far = 9.0, so that about a tenth of the coarse samples lie outside the box. Each test module
builds its own: two of them rescale sigma.
"""
import ast
import types

import numpy as np
import torch

from tables import blender_bbox, closed_form_table, convergence_rays

H, W = 12, 16
NEAR, FAR = 0.5, 9.0
MAPS = ("rgb_map", "depth_map", "acc_map", "rgb0", "depth0", "acc0", "z_std", "sparsity_loss", "sparsity_loss0", "raw")
FORWARD_ONLY = ("occupancy", "early_stop", "ray_bounds", "march")
FILL = {"rgb_map": 1.0, "rgb0": 1.0, "depth_map": float("nan"), "depth0": float("nan")}    # white background


# ---------------------------------------------------------------- the cell rule and the masks
def np_cells(pts, lo, hi, res):
    """The cell rule of csrc/occupancy.hip in NumPy fp32: (linear cell id, inside the box)."""
    pts, lo, hi = (np.asarray(a, np.float32) for a in (pts, lo, hi))
    cell = ((hi - lo) / np.float32(res)).astype(np.float32)
    xc = np.minimum(np.maximum(pts, lo), hi)
    base = np.floor((xc - lo) / cell).astype(np.int64)
    idx = np.minimum(base, res - 1)
    inside = (pts == np.maximum(np.minimum(pts, hi), lo)).all(-1)
    return (idx[..., 0] * res + idx[..., 1]) * res + idx[..., 2], inside


def np_query(pts, lo, hi, mask):
    with np.errstate(invalid="ignore"):
        cid, inside = np_cells(pts, lo, hi, mask.shape[0])
    cid = np.where(inside, cid, 0)          # a NaN point has no cell; it is outside
    return inside & mask.reshape(-1)[cid]


def random_mask(res):
    return np.random.default_rng(res).random((res, res, res)) < 0.5


def ball_mask(res=16, radius=0.35):
    c = (np.arange(res) + 0.5) / res * 2.0 - 1.0
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    return np.sqrt(x * x + y * y + z * z) <= radius


def make_mask(name, res):
    if name == "random":
        return random_mask(res)
    if name == "ball":
        return ball_mask(res)
    return np.full((res, res, res), name == "full")


# ---------------------------------------------------------------- comparisons
def bits_equal(a, b):
    """Same shape, same dtype, same int32 views (identical NaNs compare equal)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_maps_equal(got, ref, what, raw_plus_zero=False):
    for k in MAPS:
        if k not in ref:
            continue
        a, b = got[k], ref[k]
        if k == "raw" and raw_plus_zero:
            a, b = a + 0.0, b + 0.0     # -0.0 (negative x 0 in the reference) -> +0.0, nothing else changes
        assert bits_equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} values"


def scatter_back(part, hit):
    """The scatter of a hand composition: the entries of `part` (the hit rays of a frame, in order) as [H, W]
    frames in which a missed ray holds the background (FILL, 0 elsewhere)."""
    out = {}
    for k, v in part.items():
        full = torch.full((H * W,) + tuple(v.shape[1:]), FILL.get(k, 0), device=v.device, dtype=v.dtype)
        full[hit] = v
        out[k] = full.reshape((H, W) + tuple(v.shape[1:]))
    return out


# ---------------------------------------------------------------- the compaction entries, driven directly
def _two_stage(run, count, gpu):
    """Count, one host read, scatter: as OccupancyGrid.compact and run_network_sparse drive the entries."""
    i32, f = dict(device=gpu, dtype=torch.int32), dict(device=gpu, dtype=torch.float32)
    run(1, 0, None, None, None)
    k = int(count.item())
    rows, pts_c, sh_c = torch.empty(k, **i32), torch.empty(k, 3, **f), torch.empty(k, 16, **f)
    run(2, k, rows if k else None, pts_c if k else None, sh_c if k else None)
    return rows, pts_c, sh_c


def run_compact(L, gpu, pts, R, n, s0, s1, alive, sh_rays, viewdirs, lo, hi, grid, raw):
    """nerf_ert_compact over slab [s0, s1) of R rays x n samples."""
    i32 = dict(device=gpu, dtype=torch.int32)
    count = torch.full((1,), -1, **i32)
    ws = torch.empty(int(L.load().nerf_ert_compact_workspace_bytes(R * (s1 - s0))) // 4, **i32)
    bmin, bmax = L.host_f32(lo), L.host_f32(hi)

    def run(stages, cap, rows, pts_c, sh_c):
        L.call("nerf_ert_compact", L.ptr(pts), R, n, s0, s1, L.ptr(alive, "alive", torch.uint8, True),
               L.ptr(sh_rays, "sh", allow_none=True), L.ptr(viewdirs, "dirs", allow_none=True), bmin, bmax,
               1 if grid is None else grid.resolution, None if grid is None else grid._bits(), stages, cap,
               L.ptr(rows, "rows", torch.int32, True), L.ptr(count, "count", torch.int32),
               L.ptr(pts_c, "pts_c", allow_none=True), L.ptr(sh_c, "sh_c", allow_none=True), L.ptr(raw),
               L.ptr(ws, "ws", torch.int32), ws.numel() * 4, L.stream())
    return _two_stage(run, count, gpu)


def run_occ_compact(L, gpu, pts, samples_per_ray, sh_rays, viewdirs, lo, hi, grid, raw):
    """nerf_occ_compact over all of pts [P, 3]."""
    i32 = dict(device=gpu, dtype=torch.int32)
    P = pts.shape[0]
    count = torch.full((1,), -1, **i32)
    ws = torch.empty(int(L.load().nerf_occ_compact_workspace_bytes(P)) // 4, **i32)
    bmin, bmax = L.host_f32(lo), L.host_f32(hi)

    def run(stages, cap, rows, pts_c, sh_c):
        L.call("nerf_occ_compact", L.ptr(pts), P, L.ptr(sh_rays, "sh", allow_none=True),
               L.ptr(viewdirs, "dirs", allow_none=True), samples_per_ray, bmin, bmax, grid.resolution, grid._bits(),
               stages, cap, L.ptr(rows, "rows", torch.int32, True), L.ptr(count, "count", torch.int32),
               L.ptr(pts_c, "pts_c", allow_none=True), L.ptr(sh_c, "sh_c", allow_none=True), L.ptr(raw),
               L.ptr(ws, "ws", torch.int32), ws.numel() * 4, L.stream())
    return _two_stage(run, count, gpu)


# ---------------------------------------------------------------- the test scene
def build_scene(nerf, gpu, sigma_scale=None):
    """The scene of the module docstring. sigma_scale multiplies row 0 of sigma_net.1.weight (the sigma row; there
    are no biases, so this scales sigma exactly) of both networks.
    -> lo, hi, bbox, kw, emb, K, poses, packed(i), grid_of(mask), frame(i, ...), ray_kw(**over)."""
    from indoor_nerf_amd.render import _pack_rays as pack
    lo, hi = blender_bbox()
    bbox = (torch.from_numpy(lo), torch.from_numpy(hi))
    args = nerf.make_args(bounding_box=bbox, finest_res=512, N_samples=32, N_importance=32, white_bkgd=True)
    torch.manual_seed(0)
    _, kw, _, _, _ = nerf.create_nerf(args, device=gpu)
    kw.update(near=NEAR, far=FAR)
    emb = kw["embed_fn"]
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for e in emb.embeddings:
            e.weight.copy_((torch.rand(e.weight.shape, generator=g) * 2 - 1) * 0.05)
        if sigma_scale is not None:
            for net in (kw["network_fn"], kw["network_fine"]):
                net.sigma_net[1].weight[0].mul_(sigma_scale)
    for m in (kw["network_fn"], kw["network_fine"], emb):
        m.eval()
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = [nerf.pose_spherical(a, -30.0, 4.0) for a in (-40.0, 75.0)]
    cache = {}

    def packed(i):
        """The packed rows [H * W, 11] of frame i, as render() builds them."""
        ro, rd = nerf.get_rays(H, W, K, poses[i][:3, :4].to(gpu))
        return pack(H, W, K, ro, rd, kw["near"], kw["far"], kw["ndc"], kw["use_viewdirs"])

    def grid_of(mask):
        grid = nerf.OccupancyGrid(bbox, resolution=mask.shape[0], device=gpu)
        grid.set_mask(mask)
        return grid

    def frame(i, chunk=4096, retraw=True, **over):
        """One frame's maps and extras through render(); the dense ones (none of the forward-only keywords, the
        package's own query function) are cached."""
        plain = not any(k in over for k in FORWARD_ONLY + ("network_query_fn",))
        key = (i, chunk, retraw, tuple(sorted(over.items()))) if plain else None
        if key in cache:
            return cache[key]
        with torch.no_grad():
            rgb, depth, acc, ex = nerf.render(H, W, K, chunk=chunk, c2w=poses[i][:3, :4].to(gpu), retraw=retraw,
                                              **dict(kw, **over))
        out = dict(ex, rgb_map=rgb, depth_map=depth, acc_map=acc)
        if key is not None:
            cache[key] = out
        return out

    def ray_kw(**over):
        """kw for render_rays / batchify_rays (render()'s own keywords removed)."""
        out = dict(kw, **over)
        for k in ("near", "far", "ndc", "use_viewdirs"):
            out.pop(k)
        return out

    return dict(lo=lo, hi=hi, bbox=bbox, kw=kw, emb=emb, K=K, poses=poses, packed=packed, grid_of=grid_of, frame=frame,
                ray_kw=ray_kw)


# ---------------------------------------------------------------- the trained two-sphere scene
def two_sphere_scene(nerf, gpu, g):
    """The two-sphere scene of test_gpu_converge.py from its golden file g (f19_converge), untrained:
    bbox, emb, coarse, fine, kw_test (render()'s keywords for evaluation), ev and nv (the held-out and the novel
    rays: origins, directions, procedural targets), psnr_of(o, d, target, **over) -> (PSNR in dB of a render with
    kw_test and `over` against target, render()'s extras), and train(iters): that many iterations on seeded
    batches, then eval mode."""
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
    (ro, rd, rgb), ev, nv = ([torch.from_numpy(a).to(gpu) for a in part] for part in convergence_rays())
    opt = nerf.RAdam([{"params": list(coarse.parameters()) + list(fine.parameters()), "weight_decay": 1e-6},
                      {"params": list(emb.parameters()), "eps": 1e-15}], lr=c["lrate"], betas=(0.9, 0.99))

    def psnr_of(o, d, target, **over):
        with torch.no_grad():
            out, _, _, ex = nerf.render(800, 800, None, rays=(o, d), **dict(kw_test, **over))
            return (-10.0 * torch.log10(((out - target) ** 2).mean())).item(), ex

    def train(iters=300):
        rng = np.random.RandomState(100)
        for it in range(1, iters + 1):
            idx = torch.from_numpy(rng.choice(ro.shape[0], c["R"], replace=False).astype(np.int64)).to(gpu)
            nerf.train_step((ro[idx], rd[idx]), rgb[idx], kw, opt, args, it)
        for m in (coarse, fine, emb):
            m.eval()

    return types.SimpleNamespace(bbox=bbox, emb=emb, coarse=coarse, fine=fine, kw_test=kw_test, ev=ev, nv=nv,
                                 psnr_of=psnr_of, train=train)
