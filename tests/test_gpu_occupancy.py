"""Occupancy-grid empty-space skipping (csrc/occupancy.hip, occupancy.py), needs an MI355X.

The scene of forward_only.py (build_scene), rendered in chunks of 100 rays unless a test says otherwise.
Tensors are compared through their int32 views (identical NaNs compare equal): the occupancy path is exact
masking, not an approximation — the hash gather and the MLP outputs of a point do not depend on its tile or
row (test_gpu_coarse_reuse.py, test_gpu_sh_rows.py), and a zero raw row is what masking gives.

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
import functools

import numpy as np
import pytest
import torch

from forward_only import (H, W, assert_maps_equal, ball_mask, bits_equal, build_scene, np_cells, np_query, random_mask,
                          two_sphere_scene)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    s = build_scene(nerf, gpu)
    s["frame"] = functools.partial(s["frame"], chunk=100)
    return s


def masked_query_fn(scene, grid):
    """The reference of exact masking: the package's query function (no attribute of the new path on
    its inputs: the plain dense call) with its raw multiplied by grid.query(pts)."""
    nqf = scene["kw"]["network_query_fn"]

    def wrapped(pts, viewdirs, fn):
        return nqf(pts, viewdirs, fn) * grid.query(pts)[..., None]
    return wrapped


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
    ts = two_sphere_scene(nerf, gpu, golden("f19_converge"))
    psnr_of = lambda *rays, **over: ts.psnr_of(*rays, **over)[0]  # noqa: E731
    before = psnr_of(*ts.ev)
    ts.train(300)
    grid = nerf.OccupancyGrid(ts.bbox, device=gpu).update(ts.emb, [ts.coarse, ts.fine])
    print(f"occupied fraction {grid.occupied_fraction():.4f} of {grid.resolution}^3 cells")

    for name, (o, d, t) in (("held-out", ts.ev), ("novel", ts.nv)):
        dense = psnr_of(o, d, t)
        sparse = psnr_of(o, d, t, occupancy=grid)
        n, P = grid.last_counts()       # the fine pass of the last chunk
        print(f"{name}: dense {dense:.3f} dB, with the grid {sparse:.3f} dB, fine pass evaluated {n} of {P} points "
              f"({100.0 * n / P:.1f} %)")
        assert name != "held-out" or dense > before + 3.0, "fixture: the scene should have been learnt"
        assert abs(dense - sparse) <= 0.1, f"{name}: dense {dense:.3f} dB vs {sparse:.3f} dB with the grid"
