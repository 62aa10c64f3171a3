"""Occupancy-grid empty-space skipping (csrc/occupancy.hip, occupancy.py), needs an MI355X.

Scene of test_gpu_render_path.py (blender_bbox, tables uniform +-0.05, finest_res 512, 32 + 32 samples,
white background, eval mode), two 12 x 16 frames with near = 0.5, far = 9.0, so that about a tenth of the
coarse samples lie outside the box. Tensors are compared through their int32 views (identical NaNs
compare equal): the occupancy path is exact masking, not an approximation — the hash gather and the MLP
outputs of a point do not depend on its tile or row (test_gpu_coarse_reuse.py, test_gpu_sh_rows.py), and
a zero raw row is what masking gives.

Two notes on the raw comparisons:
  * full grid vs the dense path: every composited map is bit-identical, but the dense raw keeps the
    colour channels of a sample outside the box (run_network zeroes only its sigma) while the occupancy
    path, by design, writes a zero row there. raw is therefore compared with the dense raw masked by
    query() — every row inside the box bit for bit, every row outside zero — and the dense sigma of the
    rows outside is asserted to be 0 (which is why the maps agree).
  * the masked reference multiplies the dense raw by query(): a negative value times 0 is -0.0, which
    composites exactly like +0.0 (sigmoid(-0) = 0.5, relu(-0) = 0) but has another bit pattern, so raw
    itself is compared after adding 0.0 to both sides (-0 -> +0, every other value unchanged).
"""
import ast

import numpy as np
import pytest
import torch

from tables import blender_bbox, closed_form_table, convergence_rays

pytestmark = pytest.mark.gpu

H, W = 12, 16
MAPS = ("rgb", "depth", "acc", "rgb0", "depth0", "acc0", "z_std", "sparsity_loss", "sparsity_loss0", "raw")


def np_cells(pts, lo, hi, res):
    """The cell rule of csrc/occupancy.hip in NumPy fp32: (linear cell id, inside the box)."""
    pts, lo, hi = (np.asarray(a, np.float32) for a in (pts, lo, hi))
    cell = ((hi - lo) / np.float32(res)).astype(np.float32)
    xc = np.minimum(np.maximum(pts, lo), hi)
    base = np.floor((xc - lo) / cell).astype(np.int64)
    idx = np.minimum(base, res - 1)
    inside = (pts == np.maximum(np.minimum(pts, hi), lo)).all(-1)
    return (idx[:, 0] * res + idx[:, 1]) * res + idx[:, 2], inside


def np_query(pts, lo, hi, mask):
    cid, inside = np_cells(pts, lo, hi, mask.shape[0])
    return inside & mask.reshape(-1)[cid]


def random_mask(res):
    return np.random.default_rng(res).random((res, res, res)) < 0.5


def ball_mask(res=16, radius=0.35):
    c = (np.arange(res) + 0.5) / res * 2.0 - 1.0
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    return np.sqrt(x * x + y * y + z * z) <= radius


def bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    lo, hi = blender_bbox()
    bbox = (torch.from_numpy(lo), torch.from_numpy(hi))
    args = nerf.make_args(bounding_box=bbox, finest_res=512, N_samples=32, N_importance=32, white_bkgd=True)
    torch.manual_seed(0)
    _, kw, _, _, _ = nerf.create_nerf(args, device=gpu)
    kw.update(near=0.5, far=9.0)
    emb = kw["embed_fn"]
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for e in emb.embeddings:
            e.weight.copy_((torch.rand(e.weight.shape, generator=g) * 2 - 1) * 0.05)
    for m in (kw["network_fn"], kw["network_fine"], emb):
        m.eval()
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = [nerf.pose_spherical(a, -30.0, 4.0) for a in (-40.0, 75.0)]
    cache = {}

    def frame(i, chunk=100, **over):
        """One frame's maps; the dense ones (no occupancy, the package's own query function) are cached."""
        key = (i, chunk, tuple(sorted(over.items()))) if "occupancy" not in over and "network_query_fn" not in over else None
        if key in cache:
            return cache[key]
        with torch.no_grad():
            rgb, depth, acc, ex = nerf.render(H, W, K, chunk=chunk, c2w=poses[i][:3, :4].to(gpu), retraw=True,
                                              **dict(kw, **over))
        out = dict(ex, rgb=rgb, depth=depth, acc=acc)
        if key is not None:
            cache[key] = out
        return out

    return dict(lo=lo, hi=hi, bbox=bbox, kw=kw, emb=emb, frame=frame, K=K, poses=poses)


def masked_query_fn(scene, grid):
    """The reference of exact masking: the package's query function (no attribute of the new path on
    its inputs: the plain dense call) with its raw multiplied by grid.query(pts)."""
    nqf = scene["kw"]["network_query_fn"]

    def wrapped(pts, viewdirs, fn):
        return nqf(pts, viewdirs, fn) * grid.query(pts)[..., None]
    return wrapped


def assert_maps_equal(got, ref, what, raw_plus_zero=False):
    for k in MAPS:
        if k not in ref:
            continue
        a, b = got[k], ref[k]
        if k == "raw" and raw_plus_zero:
            a, b = a + 0.0, b + 0.0     # -0.0 (negative x 0 in the reference) -> +0.0, nothing else changes
        assert bits_equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} values"


# ---------------------------------------------------------------- 1. cell rule
@pytest.mark.parametrize("res", [4, 5, 128])
def test_query_matches_numpy_cell_rule(nerf, gpu, scene, res):
    lo, hi = scene["lo"], scene["hi"]
    rng = np.random.default_rng(11)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pts = (mid + (rng.random((4096 + 37, 3)) * 2 - 1) * 1.5 * half).astype(np.float32)
    cell = ((hi - lo) / np.float32(res)).astype(np.float32)
    edges = (lo[0] + np.arange(res + 1, dtype=np.float32) * cell[0]).astype(np.float32)
    edges = np.concatenate([edges, np.nextafter(edges, np.float32(-1e30)), np.nextafter(edges, np.float32(1e30))])
    on_axis = np.tile(mid.astype(np.float32), (edges.shape[0], 1))
    on_axis[:, 0] = edges
    pts = np.concatenate([pts, lo[None], hi[None], on_axis]).astype(np.float32)
    mask = random_mask(res)
    grid = nerf.OccupancyGrid(scene["bbox"], resolution=res, device=gpu)
    grid.set_mask(mask)
    assert np.array_equal(grid.mask().cpu().numpy(), mask)
    got = grid.query(torch.from_numpy(pts).to(gpu)).cpu().numpy()
    want = np_query(pts, lo, hi, mask)
    assert 0.05 < want.mean() < 0.9         # the points exercise both answers
    assert np.array_equal(got, want), f"res {res}: {int((got != want).sum())} of {len(want)} points differ"
    assert abs(grid.occupied_fraction() - mask.mean()) < 1e-6


# ---------------------------------------------------------------- 2. full grid = the dense path
@pytest.mark.parametrize("i", [0, 1])
def test_full_grid_is_the_dense_path(nerf, gpu, scene, i):
    grid = nerf.OccupancyGrid(scene["bbox"], resolution=16, device=gpu)
    grid.set_mask(np.ones((16, 16, 16), bool))
    dense = scene["frame"](i)
    got = scene["frame"](i, occupancy=grid)
    inside = grid.query(dense["pts"])               # full grid: inside the box
    assert 0.01 < 1.0 - float(inside.float().mean()) < 0.5     # some samples do lie outside the box
    assert bool((dense["raw"][..., 3][~inside] == 0).all())  # the dense path gives them sigma = 0 (the box mask)
    ref = dict(dense, raw=torch.where(inside[..., None], dense["raw"], torch.zeros_like(dense["raw"])))
    assert_maps_equal(got, ref, f"pose {i}, full grid")
    assert bits_equal(got["pts"], dense["pts"])


# ---------------------------------------------------------------- 3. a mask is exact masking
@pytest.mark.parametrize("which", ["ball16", "random5"])
def test_mask_is_exact_masking(nerf, gpu, scene, which):
    mask = ball_mask() if which == "ball16" else random_mask(5)
    if which == "ball16":
        assert int(mask.sum()) == 88
    grid = nerf.OccupancyGrid(scene["bbox"], resolution=mask.shape[0], device=gpu)
    grid.set_mask(mask)
    for i in (0, 1):
        ref = scene["frame"](i, network_query_fn=masked_query_fn(scene, grid))
        got = scene["frame"](i, occupancy=grid)
        assert_maps_equal(got, ref, f"{which}, pose {i}", raw_plus_zero=True)
        # coarse pass alone: the raw rows themselves, in one field call and in chunks of 37 and 7 rays
        dense = scene["frame"](i, chunk=4096, N_importance=0)
        for chunk in (4096, 37):
            got = scene["frame"](i, chunk=chunk, N_importance=0, occupancy=grid)
            assert bits_equal(got["pts"], dense["pts"])
            q = grid.query(dense["pts"])
            kept = float(q.float().mean())
            lost = int((~q.view(H * W, -1).any(-1)).sum())
            print(f"{which} pose {i}: {100 * kept:.1f} % of the coarse samples kept, {lost} of {H * W} rays lose all")
            assert 0.0 < kept < 1.0
            assert bits_equal(got["raw"][q], dense["raw"][q]), "kept rows differ from the dense rows"
            assert bool((got["raw"][~q].view(torch.int32) == 0).all()), "skipped rows are not zero"
            assert_maps_equal(got, scene["frame"](i, chunk=chunk, N_importance=0,
                                                  network_query_fn=masked_query_fn(scene, grid)),
                              f"{which}, pose {i}, coarse only, chunk {chunk}", raw_plus_zero=True)
            if chunk == 4096:   # one field call for the whole frame
                assert grid.last_counts() == (int(q.sum()), q.numel())


# ---------------------------------------------------------------- 4. builder
@pytest.mark.parametrize("res", [5, 8])
def test_builder(nerf, gpu, scene, res):
    lo, hi, emb, kw = scene["lo"], scene["hi"], scene["emb"], scene["kw"]
    spc, n_cells = 4, res ** 3
    grid = nerf.OccupancyGrid(scene["bbox"], resolution=res, device=gpu)
    pts = grid.cell_points(0, n_cells, spc, 7)
    # every position classifies into its own cell, sample 0 is the centre, chunking changes nothing
    cid, inside = np_cells(pts.view(-1, 3).cpu().numpy(), lo, hi, res)
    assert inside.all() and np.array_equal(cid, np.repeat(np.arange(n_cells), spc))
    cell = (hi - lo) / np.float32(res)
    ijk = np.stack(np.unravel_index(np.arange(n_cells), (res, res, res)), -1)
    np.testing.assert_allclose(pts[:, 0].cpu().numpy(), lo + (ijk + 0.5) * cell, rtol=0, atol=1e-5)
    assert pts[:, 1:].reshape(-1, 3).unique(dim=0).shape[0] == n_cells * (spc - 1)      # jittered, all distinct
    parts = torch.cat([grid.cell_points(c, min(50, n_cells - c), spc, 7) for c in range(0, n_cells, 50)])
    assert bits_equal(parts, pts)
    assert not bits_equal(grid.cell_points(0, n_cells, spc, 8), pts)
    # mask() = any_k(sigma > 0) per cell, from the ordinary query function on those positions
    view = torch.zeros(n_cells, 3, device=gpu)
    view[:, 0] = 1.0
    want = {}
    with torch.no_grad():
        for name in ("network_fn", "network_fine"):
            sigma = kw["network_query_fn"](pts, view, kw[name])[..., 3]
            want[name] = (sigma > 0).any(-1).view(res, res, res).cpu().numpy()
            grid.update(emb, kw[name], sigma_thresh=0.0, samples_per_cell=spc, dilate=0, seed=7)
            assert np.array_equal(grid.mask().cpu().numpy(), want[name]), name
    both = want["network_fn"] | want["network_fine"]
    print(f"res {res}: occupied {want['network_fn'].mean():.3f} (coarse), {want['network_fine'].mean():.3f} (fine), "
          f"{both.mean():.3f} (union)")
    assert any(0 < m.sum() < m.size for m in want.values())     # a fixture with both answers
    grid.update(emb, [kw["network_fn"], kw["network_fine"]], sigma_thresh=0.0, samples_per_cell=spc, dilate=0, seed=7)
    assert np.array_equal(grid.mask().cpu().numpy(), both)
    bits = grid.bits.clone()
    # the same seed gives the same grid whatever the chunk size
    grid.update(emb, [kw["network_fn"], kw["network_fine"]], sigma_thresh=0.0, samples_per_cell=spc, dilate=0, seed=7,
                chunk_cells=64)
    assert torch.equal(grid.bits, bits)
    # dilate = 1: the 3 x 3 x 3 maximum over the zero-padded mask
    grid.update(emb, [kw["network_fn"], kw["network_fine"]], sigma_thresh=0.0, samples_per_cell=spc, dilate=1, seed=7)
    pad = np.pad(both, 1)
    dil = np.zeros_like(both)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                dil |= pad[dx:dx + res, dy:dy + res, dz:dz + res]
    assert np.array_equal(grid.mask().cpu().numpy(), dil)


# ---------------------------------------------------------------- 5. guards
def test_guards(nerf, gpu, scene):
    kw = scene["kw"]
    grid = nerf.OccupancyGrid(scene["bbox"], resolution=4, device=gpu)
    grid.set_mask(np.ones((4, 4, 4), bool))
    pose = scene["poses"][0][:3, :4].to(gpu)

    def run(**over):
        return nerf.render(H, W, scene["K"], chunk=4096, c2w=pose, **dict(kw, occupancy=grid, **over))

    with torch.no_grad():
        run()                                                     # the supported combination
    with torch.enable_grad(), pytest.raises(ValueError, match="forward-only"):
        run()
    with torch.no_grad(), pytest.raises(ValueError, match="raw_noise_std"):
        run(raw_noise_std=1.0)
    head = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                          input_ch=32, input_ch_views=16, predict_normals=True).to(gpu).eval()
    with torch.no_grad(), pytest.raises(ValueError, match="normals head"):
        run(network_fine=head, predict_normals=True)
    emb_q = nerf.HashEmbedder(scene["bbox"], log2_hashmap_size=14, finest_resolution=512, use_quantization=True)
    emb_q = emb_q.to(gpu).eval()
    sh = nerf.SHEncoder()
    with torch.no_grad(), pytest.raises(ValueError, match="A-CAQ"):
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, fn, emb_q, sh), embed_fn=emb_q)
    with pytest.raises(ValueError, match="A-CAQ"):
        grid.update(emb_q, kw["network_fn"])
    # a query function that does not reach this package's run_network must not fall back to the dense path
    nqf = kw["network_query_fn"]
    with torch.no_grad(), pytest.raises(ValueError, match="network_query_fn"):
        run(network_query_fn=lambda p, v, fn: nqf(p.clone(), v, fn))


# ---------------------------------------------------------------- 6. trained scene, default parameters
def test_trained_scene_psnr_within_0p1_db(nerf, gpu, golden):
    """The two-sphere scene of test_gpu_converge.py, 300 iterations, a grid with the defaults: PSNR of the
    held-out and the novel rays against the procedural targets within 0.1 dB of the dense render (the
    project's parity bar)."""
    g = golden("f19_converge")
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
    (ro, rd, rgb), ev, nv = convergence_rays()
    ro, rd, rgb = (torch.from_numpy(a).to(gpu) for a in (ro, rd, rgb))
    opt = nerf.RAdam([{"params": list(coarse.parameters()) + list(fine.parameters()), "weight_decay": 1e-6},
                      {"params": list(emb.parameters()), "eps": 1e-15}], lr=c["lrate"], betas=(0.9, 0.99))
    def psnr_of(o, d, target, **over):
        with torch.no_grad():
            out, _, _, _ = nerf.render(800, 800, None, rays=(o, d), **dict(kw_test, **over))
            return (-10.0 * torch.log10(((out - target) ** 2).mean())).item()

    ev, nv = ([torch.from_numpy(a).to(gpu) for a in part] for part in (ev, nv))
    before = psnr_of(*ev)
    rng = np.random.RandomState(100)
    for it in range(1, 301):
        idx = torch.from_numpy(rng.choice(ro.shape[0], c["R"], replace=False).astype(np.int64)).to(gpu)
        nerf.train_step((ro[idx], rd[idx]), rgb[idx], kw, opt, args, it)
    for m in (coarse, fine, emb):
        m.eval()
    grid = nerf.OccupancyGrid(bbox, device=gpu).update(emb, [coarse, fine])
    print(f"occupied fraction {grid.occupied_fraction():.4f} of {grid.resolution}^3 cells")

    for name, (o, d, t) in (("held-out", ev), ("novel", nv)):
        dense = psnr_of(o, d, t)
        sparse = psnr_of(o, d, t, occupancy=grid)
        n, P = grid.last_counts()       # the fine pass of the last chunk
        print(f"{name}: dense {dense:.3f} dB, with the grid {sparse:.3f} dB, fine pass evaluated {n} of {P} points "
              f"({100.0 * n / P:.1f} %)")
        assert name != "held-out" or dense > before + 3.0, "fixture: the scene should have been learnt"
        assert abs(dense - sparse) <= 0.1, f"{name}: dense {dense:.3f} dB vs {sparse:.3f} dB with the grid"
