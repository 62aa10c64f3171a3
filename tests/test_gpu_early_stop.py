"""Early ray termination for forward-only rendering (csrc/early_stop.hip, early_stop.py),
needs an MI355X.

The scene of forward_only.py (build_scene), with one change: that random field has relu(sigma) * delta summing
to only 0.01 - 0.04 per ray, so nothing would ever terminate, and the fixture multiplies the sigma row of both
networks by SIGMA_SCALE = 500 (the dense optical depth after S / 2 samples then has its 0.75 quantile near 7, so
that eps lies well inside (1e-6, 0.1); at 1000 it is 14.2 and eps 6.8e-7 falls outside).

eps is calibrated from the dense render, never from the path under test: tau_q is the QUANTILE = 0.75
quantile, over the rays of both frames, of the dense coarse optical depth after S / 2 samples (fp64, from
the dense raw), eps = exp(-tau_q), and the rule's threshold is tau_max = float32(-log(eps)) as the package
computes it. The fixture asserts 1e-6 < eps < 0.1 and, per pose, on the stops of the NumPy rule applied to
the dense coarse raw at K = 8: at least 3 distinct stop values, at least 20 % of the rays stop early, at
least 5 rays reach S.

Tensors are compared through their int32 views (identical NaNs compare equal). As in
test_gpu_occupancy.py the dense raw keeps the colour channels of a sample outside the box while the new
path writes a zero row there, so the masked reference multiplies the dense raw by "inside the box" as
well (the query of a one-cell grid with its bit set), and raw is compared after adding 0.0 to both sides
(a negative value times 0 is -0.0).
"""
import math

import numpy as np
import pytest
import torch

from forward_only import (FAR, H, NEAR, W, assert_maps_equal, ball_mask, bits_equal, build_scene, np_cells, random_mask,
                          run_compact, two_sphere_scene)
from tables import blender_bbox

pytestmark = pytest.mark.gpu

S = 32
SIGMA_SCALE = 500.0
QUANTILE = 0.75
F0 = np.float32(0.0)


# ---------------------------------------------------------------- NumPy restatements
def np_advance(sigma, z, rays_d, s0, s1, tau_max, tau, alive, stop):
    """The rule of csrc/early_stop.hip for one slab in NumPy fp32: every operation below is one correctly
    rounded float32 operation per ray, the samples strictly in order. -> (tau, alive, stop)."""
    sigma, z, rays_d, tau = (np.asarray(a, np.float32) for a in (sigma, z, rays_d, tau))
    dx, dy, dz = rays_d[:, 0], rays_d[:, 1], rays_d[:, 2]
    with np.errstate(all="ignore"):
        norm = np.sqrt(dx * dx + dy * dy + dz * dz)
        t = tau.copy()
        for i in range(s0, s1):
            d = (z[:, i + 1] - z[:, i]) * norm
            s = np.where(sigma[:, i] > F0, sigma[:, i], F0)
            t = t + s * d
        assert t.dtype == np.float32 and norm.dtype == np.float32
        live = np.asarray(alive).astype(bool)
        tau = np.where(live, t, tau)
        die = live & (tau > np.float32(tau_max))
    return tau, (live & ~die).astype(np.uint8), np.where(die, s1, stop).astype(np.int32)


def np_stops(sigma, z, rays_d, tau_max, K):
    """The stops of a whole pass (every ray alive in slab 0, tau from 0, no decision after the last slab)."""
    R, n = sigma.shape
    tau, alive, stop = np.zeros(R, np.float32), np.ones(R, np.uint8), np.full(R, n, np.int32)
    for s0 in range(0, n, K):
        s1 = min(s0 + K, n)
        if s1 < n:
            tau, alive, stop = np_advance(sigma, z, rays_d, s0, s1, tau_max, tau, alive, stop)
    return stop


def coarse_z(n_rays):
    """The coarse depths of csrc/sampling.hip without perturbation: near * (1 - t) + far * t in fp32."""
    t = torch.linspace(0., 1., steps=S).numpy()
    z = np.float32(NEAR) * (np.float32(1.0) - t) + np.float32(FAR) * t
    assert z.dtype == np.float32
    return np.tile(z, (n_rays, 1))


# ---------------------------------------------------------------- scene
@pytest.fixture(scope="module")
def scene(nerf, gpu):
    sc = build_scene(nerf, gpu, SIGMA_SCALE)
    bbox, frame, poses = sc["bbox"], sc["frame"], sc["poses"]
    box = nerf.OccupancyGrid(bbox, resolution=1, device=gpu)     # query() = inside the box
    box.set_mask(np.ones((1, 1, 1), bool))
    ball = nerf.OccupancyGrid(bbox, resolution=16, device=gpu)
    ball.set_mask(ball_mask())
    # the ball is so small that no ray through it alone reaches tau_max: a half-full grid has rays stop behind it too
    rand = nerf.OccupancyGrid(bbox, resolution=5, device=gpu)
    rand.set_mask(random_mask(5))

    # calibration, from the dense coarse render alone
    dense, taus = [], []
    for i in (0, 1):
        d = frame(i, N_importance=0)
        sigma = d["raw"][..., 3].reshape(H * W, S).cpu().numpy()
        rays_d = d["rays_d"].reshape(H * W, 3).cpu().numpy()
        z = coarse_z(H * W)
        # the restated depths are the path's: pts = o + d * z up to the rounding of three fp32 operations
        o = poses[i][:3, 3].numpy().astype(np.float64)
        p = d["pts"].reshape(H * W, S, 3).cpu().numpy().astype(np.float64)
        z64 = ((p - o) * rays_d[:, None, :]).sum(-1) / (rays_d.astype(np.float64) ** 2).sum(-1)[:, None]
        assert np.abs(z64 - z).max() < 1e-5
        delta = np.diff(z64, axis=1) * np.linalg.norm(rays_d.astype(np.float64), axis=1)[:, None]
        tau64 = np.concatenate([np.zeros((H * W, 1)), np.cumsum(np.maximum(sigma[:, :-1], 0).astype(np.float64) * delta, 1)], 1)
        dense.append(dict(sigma=sigma, rays_d=rays_d, z=z, tau64=tau64))    # tau64[:, b]: depth over samples [0, b)
        taus.append(tau64[:, S // 2])
    tau_q = float(np.quantile(np.concatenate(taus), QUANTILE))
    eps = math.exp(-tau_q)
    tau_max = np.float32(-math.log(eps))
    print(f"calibration: tau quantile {tau_q:.4f}, eps {eps:.3e}, tau_max {float(tau_max):.6f}, total depth per ray "
          f"{np.median(np.concatenate([d['tau64'][:, -1] for d in dense])):.2f} (median)")
    assert 1e-6 < eps < 0.1, f"fixture: eps {eps:.3e} (change SIGMA_SCALE)"
    for i, d in enumerate(dense):
        stop = np_stops(d["sigma"], d["z"], d["rays_d"], tau_max, 8)
        early, full = float((stop < S).mean()), int((stop == S).sum())
        print(f"pose {i}: NumPy stops at K = 8 {sorted(set(stop.tolist()))}, {100 * early:.0f} % stop early, {full} reach S")
        assert len(set(stop.tolist())) >= 3 and early >= 0.2 and full >= 5, "fixture conditions"
    return dict(sc, eps=eps, tau_max=tau_max, dense=dense, box=box, grids={"none": None, "ball16": ball, "random5": rand})


def masked_query_fn(scene, stops, grid):
    """The reference of exact masking: the package's plain dense query function (no attribute of the new
    path on its inputs) with its raw multiplied by (s < stop[r]), by "inside the box" and, with a grid, by
    grid.query(pts). `stops`: one [R] tensor per field call, in call order."""
    nqf, box = scene["kw"]["network_query_fn"], scene["box"]
    calls = iter(stops)

    def wrapped(pts, viewdirs, fn):
        stop = next(calls).reshape(-1)
        m = (torch.arange(pts.shape[1], device=pts.device)[None, :] < stop[:, None]) & box.query(pts)
        if grid is not None:
            m = m & grid.query(pts)
        return nqf(pts, viewdirs, fn) * m[..., None]
    return wrapped


def check_exact_masking(scene, i, eps, K, grid, what):
    """Test 3's body: two-pass maps against the masked reference, then the coarse-only raw rows and counts."""
    import indoor_nerf_amd as nerf
    frame, occ = scene["frame"], ({} if grid is None else {"occupancy": grid})
    got = frame(i, early_stop=eps, early_stop_slab=K, **occ)
    s0, s1 = got["early_stop_samples0"], got["early_stop_samples"]
    assert s0.dtype == torch.int32 and s1.dtype == torch.int32 and s0.shape == (H, W) and s1.shape == (H, W)
    for st, n in ((s0, S), (s1, 2 * S)):
        assert bool(((st == n) | ((st % K == 0) & (st > 0) & (st < n))).all()), "a stop is a multiple of K, or S"
    ref = frame(i, network_query_fn=masked_query_fn(scene, [s0, s1], grid))
    assert_maps_equal(got, ref, what, raw_plus_zero=True)
    assert bits_equal(got["pts"], ref["pts"])
    # coarse pass alone, one field call: the raw rows themselves and the counts
    dense = frame(i, N_importance=0)
    got = frame(i, N_importance=0, early_stop=eps, early_stop_slab=K, **occ)
    assert "early_stop_samples0" not in got
    stop = got["early_stop_samples"].reshape(-1)
    assert bits_equal(got["pts"], dense["pts"])
    q = (torch.arange(S, device=stop.device)[None, :] < stop[:, None]).view(H, W, S) & scene["box"].query(dense["pts"])
    if grid is not None:
        q = q & grid.query(dense["pts"])
    assert bits_equal(got["raw"][q], dense["raw"][q]), f"{what}: kept rows differ from the dense rows"
    assert bool((got["raw"][~q].view(torch.int32) == 0).all()), f"{what}: skipped rows are not zero"
    assert nerf.last_early_stop_counts() == (int(q.sum()), q.numel())
    assert_maps_equal(got, frame(i, N_importance=0, network_query_fn=masked_query_fn(scene, [stop], grid)),
                      what + ", coarse only", raw_plus_zero=True)
    return stop.cpu().numpy(), float(q.float().mean())


# ---------------------------------------------------------------- 1. the rule, bit for bit
@pytest.mark.parametrize("K", [8, 24])
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("R", [1, 63, 193])
def test_advance_matches_numpy_rule(nerf, gpu, R, n, K):
    import indoor_nerf_amd._lib as L
    rng = np.random.default_rng(1000 * R + 10 * n + K)
    sigma = (rng.standard_normal((R, n)) * 3.0).astype(np.float32)        # both signs
    sigma[rng.random((R, n)) < 0.05] = np.nan
    raw = rng.standard_normal((R, n, 4)).astype(np.float32)
    raw[..., 3] = sigma
    z = np.sort(rng.uniform(NEAR, FAR, (R, n)).astype(np.float32), axis=1)
    rays_d = rng.standard_normal((R, 3)).astype(np.float32)
    tau_max = np.float32(4.0)
    tau = rng.uniform(0.0, 2.0, R).astype(np.float32)
    alive = (rng.random(R) < 0.75).astype(np.uint8)                         # some rays already dead
    stop = np.where(alive, n, 0).astype(np.int32)
    d_raw, d_z, d_d = (torch.from_numpy(a).to(gpu) for a in (raw, z, rays_d))
    d_tau, d_alive, d_stop = (torch.from_numpy(a.copy()).to(gpu) for a in (tau, alive, stop))
    died = 0
    for s0 in range(0, n, K):
        s1 = min(s0 + K, n)
        if s1 == n:
            break
        L.call("nerf_ert_advance", L.ptr(d_raw), L.ptr(d_z), L.ptr(d_d), R, n, s0, s1, float(tau_max), L.ptr(d_tau),
               L.ptr(d_alive, "alive", torch.uint8), L.ptr(d_stop, "stop", torch.int32), L.stream())
        before = int(alive.sum())
        tau, alive, stop = np_advance(sigma, z, rays_d, s0, s1, tau_max, tau, alive, stop)
        died += before - int(alive.sum())
        assert np.array_equal(d_tau.cpu().numpy().view(np.int32), tau.view(np.int32)), f"tau after [{s0}, {s1})"
        assert np.array_equal(d_alive.cpu().numpy(), alive) and np.array_equal(d_stop.cpu().numpy(), stop)
    if R > 1:
        assert died > 0 and int(alive.sum()) > 0        # the inputs exercise both outcomes


# ---------------------------------------------------------------- 2. the compaction
@pytest.mark.parametrize("with_grid", [False, True])
@pytest.mark.parametrize("R", [1, 7, 193])
def test_compact_matches_numpy(nerf, gpu, R, with_grid):
    import indoor_nerf_amd._lib as L
    lo, hi = blender_bbox()
    n = 64
    rng = np.random.default_rng(17 * R + with_grid)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pts = (mid + (rng.random((R, n, 3)) * 2 - 1) * 1.3 * half).astype(np.float32)
    mask = random_mask(5)
    grid = None
    if with_grid:
        grid = nerf.OccupancyGrid((torch.from_numpy(lo), torch.from_numpy(hi)), resolution=5, device=gpu)
        grid.set_mask(mask)
    cid, inside = np_cells(pts.reshape(-1, 3), lo, hi, 5)
    ok = (inside & mask.reshape(-1)[cid]) if with_grid else inside
    assert 0.05 < ok.mean() < 0.95
    dirs = rng.standard_normal((R, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    records = rng.standard_normal((R, 40)).astype(np.float32)
    d_pts, d_dirs, d_rec = (torch.from_numpy(a).to(gpu) for a in (pts, dirs, records))
    sh_of_dirs = nerf.SHEncoder()(d_dirs)
    alive_sets = {"random": (rng.random(R) < 0.6).astype(np.uint8), "dead": np.zeros(R, np.uint8), "none": None}
    if R == 1:
        alive_sets["random"] = np.ones(1, np.uint8)
    for (s0, s1) in ((0, 8), (24, 32), (48, 64)):
        for name, alive in alive_sets.items():
            for use_records in (True, False):
                raw = torch.full((R * n, 4), 7.0, device=gpu)
                d_alive = None if alive is None else torch.from_numpy(alive).to(gpu)
                rows, pts_c, sh_c = run_compact(L, gpu, d_pts, R, n, s0, s1, d_alive, d_rec if use_records else None,
                                                None if use_records else d_dirs, lo, hi, grid, raw)
                live = np.ones(R, bool) if alive is None else alive.astype(bool)
                in_slab = np.zeros((R, n), bool)
                in_slab[:, s0:s1] = True
                kept = in_slab & live[:, None] & ok.reshape(R, n)
                want = np.flatnonzero(kept.reshape(-1)).astype(np.int32)      # ascending in p = r * S + s
                what = f"slab [{s0}, {s1}), alive {name}, records {use_records}"
                assert np.array_equal(rows.cpu().numpy(), want), what
                assert name != "dead" or rows.numel() == 0
                assert np.array_equal(pts_c.cpu().numpy().view(np.int32), pts.reshape(-1, 3)[want].view(np.int32)), what
                ray = torch.from_numpy(want // n).to(gpu).long()
                want_sh = d_rec[ray, :16] if use_records else sh_of_dirs[ray]
                assert bits_equal(sh_c, want_sh), what
                # raw: zero rows for the candidates not kept, every other row untouched
                zeroed = torch.from_numpy((in_slab & ~kept).reshape(-1)).to(gpu)
                assert bool((raw[zeroed].view(torch.int32) == 0).all()) and bool((raw[~zeroed] == 7.0).all()), what


# ---------------------------------------------------------------- 3. exact masking
@pytest.mark.parametrize("which", ["none", "ball16", "random5"])
@pytest.mark.parametrize("K", [8, 24])
@pytest.mark.parametrize("i", [0, 1])
def test_early_stop_is_exact_masking(nerf, gpu, scene, i, K, which):
    grid = scene["grids"][which]
    stop, kept = check_exact_masking(scene, i, scene["eps"], K, grid, f"pose {i}, K {K}, grid {which}")
    print(f"pose {i}, K {K}, grid {which}: coarse stops {sorted(set(stop.tolist()))}, {100 * kept:.1f} % of the "
          f"coarse samples evaluated")
    assert 0.0 < kept < 1.0


# ---------------------------------------------------------------- 4. the stops are right
@pytest.mark.parametrize("which", ["none", "ball16", "random5"])
@pytest.mark.parametrize("K", [8, 24])
def test_stops_against_fp64(nerf, gpu, scene, K, which):
    """Band: an fp32 sum of <= 64 non-negative terms with two roundings each has relative error
    <= 66 * 2^-24 ~ 4e-6, far inside 1e-4."""
    grid = scene["grids"][which]
    tau_max = float(scene["tau_max"])
    for i in (0, 1):
        d = scene["dense"][i]
        got = scene["frame"](i, N_importance=0, early_stop=scene["eps"], early_stop_slab=K,
                             **({} if grid is None else {"occupancy": grid}))
        stop = got["early_stop_samples"].reshape(-1).cpu().numpy()
        sigma, tau64 = d["sigma"], d["tau64"]
        if grid is not None:      # the rule sees the masked sigma
            q = grid.query(scene["frame"](i, N_importance=0)["pts"]).reshape(H * W, S).cpu().numpy()
            sigma = np.where(q, sigma, F0)
            z64 = d["z"].astype(np.float64)
            delta = np.diff(z64, axis=1) * np.linalg.norm(d["rays_d"].astype(np.float64), axis=1)[:, None]
            tau64 = np.concatenate([np.zeros((H * W, 1)),
                                    np.cumsum(np.maximum(sigma[:, :-1], 0).astype(np.float64) * delta, 1)], 1)
        assert np.array_equal(stop, np_stops(sigma, d["z"], d["rays_d"], scene["tau_max"], K)), f"pose {i}"
        for b in range(K, S, K):
            before, at = stop > b, stop == b
            assert (tau64[before, b] <= tau_max * (1 + 1e-4)).all(), f"pose {i}: a ray alive past {b} should have died"
            assert (tau64[at, b] >= tau_max * (1 - 1e-4)).all(), f"pose {i}: a ray died at {b} too early"
        assert which == "ball16" or ((stop < S).any() and (stop == S).any())


# ---------------------------------------------------------------- 5. chunking and slab edge cases
def test_chunking_gives_identical_maps_and_stops(nerf, gpu, scene):
    for i in (0, 1):
        a = scene["frame"](i, chunk=4096, early_stop=scene["eps"], early_stop_slab=8)
        b = scene["frame"](i, chunk=37, early_stop=scene["eps"], early_stop_slab=8)
        assert_maps_equal(a, b, f"pose {i}, chunk 37 vs 4096")
        for k in ("early_stop_samples", "early_stop_samples0"):
            assert torch.equal(a[k], b[k]), k


def test_one_slab_is_the_full_grid_occupancy_path(nerf, gpu, scene):
    full = nerf.OccupancyGrid(scene["bbox"], resolution=16, device=gpu)
    full.set_mask(np.ones((16, 16, 16), bool))
    for i in (0, 1):
        got = scene["frame"](i, early_stop=scene["eps"], early_stop_slab=64)
        assert_maps_equal(got, scene["frame"](i, occupancy=full), f"pose {i}, K = 64 >= S")
        assert bool((got["early_stop_samples0"] == S).all()) and bool((got["early_stop_samples"] == 2 * S).all())


def test_threshold_near_one_kills_at_the_first_density(nerf, gpu, scene):
    eps = 1.0 - 1e-6
    for i in (0, 1):
        stop, kept = check_exact_masking(scene, i, eps, 8, None, f"pose {i}, eps 1 - 1e-6")
        d = scene["dense"][i]
        assert np.array_equal(stop, np_stops(d["sigma"], d["z"], d["rays_d"], np.float32(-math.log(eps)), 8))
        # tau_max ~ 1e-6: the first slab with any sigma worth the name kills the ray (delta >= 0.27, so a slab whose
        # relu(sigma) sum to more than 1e-4 adds more than 2e-5), and every later slab has no kept point
        sums = np.maximum(d["sigma"], 0).reshape(H * W, S // 8, 8).sum(-1)
        first = np.argmax(sums > 1e-4, axis=1)
        clear = (sums > 1e-4).any(1) & (np.where(np.arange(S // 8)[None, :] < first[:, None], sums, 0) == 0).all(1)
        want = np.where(8 * (first + 1) < S, 8 * (first + 1), S)
        assert clear.mean() > 0.5 and (stop[clear] == want[clear]).all()
        print(f"pose {i}: stops {sorted(set(stop.tolist()))}, {100 * (stop < S).mean():.0f} % of the rays stopped, "
              f"{100 * kept:.1f} % of the samples evaluated")


# ---------------------------------------------------------------- 6. the bound
@pytest.mark.parametrize("which_eps", ["calibrated", "0.05"])
def test_error_bound(nerf, gpu, scene, which_eps):
    """A pass differs from its unmasked self by at most eps: |rgb - rgb_dense| <= eps per channel and
    0 <= acc_dense - acc <= eps, with 1e-5 of slack for the reordered 64-term fp32 sums (<= 64 * 2^-24 ~ 4e-6).
    Holds for a coarse-only render and for rgb0 / acc0 of the two-pass render."""
    eps = scene["eps"] if which_eps == "calibrated" else 0.05
    for i in (0, 1):
        for K in (8, 24):
            for two_pass in (False, True):
                over = {} if two_pass else {"N_importance": 0}
                dense = scene["frame"](i, **over)
                got = scene["frame"](i, early_stop=eps, early_stop_slab=K, **over)
                rgb, acc = ("rgb0", "acc0") if two_pass else ("rgb_map", "acc_map")
                e_rgb = float((got[rgb] - dense[rgb]).abs().max())
                d_acc = dense[acc] - got[acc]
                stopped = float((got["early_stop_samples0" if two_pass else "early_stop_samples"] < S).float().mean())
                print(f"pose {i}, K {K}, eps {eps:.3e}, {'two-pass' if two_pass else 'coarse only'}: max|d{rgb}| "
                      f"{e_rgb:.3e}, {acc} deficit [{float(d_acc.min()):.3e}, {float(d_acc.max()):.3e}], "
                      f"{100 * stopped:.0f} % of the rays stopped")
                assert stopped > 0.2
                assert e_rgb <= eps + 1e-5
                assert float(d_acc.min()) >= -1e-5 and float(d_acc.max()) <= eps + 1e-5


# ---------------------------------------------------------------- 7. guards
def test_guards(nerf, gpu, scene):
    kw = scene["kw"]
    pose = scene["poses"][0][:3, :4].to(gpu)

    def run(**over):
        return nerf.render(H, W, scene["K"], chunk=4096, c2w=pose, **{**kw, "early_stop": 1e-3, **over})

    with torch.no_grad():
        run()                                                     # the supported combinations
        run(occupancy=scene["grids"]["ball16"], early_stop_slab=5)
    with torch.enable_grad(), pytest.raises(ValueError, match="forward-only"):
        run()
    with torch.no_grad(), pytest.raises(ValueError, match="raw_noise_std"):
        run(raw_noise_std=1.0)
    for bad in (0.0, 1.0, 1.5, -1e-3):
        with torch.no_grad(), pytest.raises(ValueError, match="early_stop must be"):
            run(early_stop=bad)
    with torch.no_grad(), pytest.raises(ValueError, match="early_stop_slab"):
        run(early_stop_slab=0)
    head = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                          input_ch=32, input_ch_views=16, predict_normals=True).to(gpu).eval()
    with torch.no_grad(), pytest.raises(ValueError, match="normals head"):
        run(network_fine=head, predict_normals=True)
    emb_q = nerf.HashEmbedder(scene["bbox"], log2_hashmap_size=14, finest_resolution=512, use_quantization=True)
    emb_q = emb_q.to(gpu).eval()
    sh = nerf.SHEncoder()
    with torch.no_grad(), pytest.raises(ValueError, match="A-CAQ"):
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, fn, emb_q, sh), embed_fn=emb_q)
    with torch.no_grad(), pytest.raises(ValueError, match="fused field modules"):
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, torch.nn.Linear(48, 4).to(gpu), kw["embed_fn"], sh))
    # a query function that does not reach this package's run_network must not fall back to the dense path
    nqf = kw["network_query_fn"]
    with torch.no_grad(), pytest.raises(ValueError, match="network_query_fn"):
        run(network_query_fn=lambda p, v, fn: nqf(p.clone(), v, fn))
    # without the keyword nothing of the new path shows
    with torch.no_grad():
        ex = nerf.render(H, W, scene["K"], chunk=4096, c2w=pose, **kw)[3]
    assert "early_stop_samples" not in ex and "early_stop_samples0" not in ex


# ---------------------------------------------------------------- 8. trained scene, eps = 1e-3
def test_trained_scene_psnr_within_0p1_db(nerf, gpu, golden):
    """The two-sphere scene of test_gpu_converge.py, 300 iterations, early_stop = 1e-3 with and without a
    grid of the defaults: PSNR of the held-out and the novel rays against the procedural targets within
    0.1 dB of the dense render (the project's parity bar; at an RMSE near 0.1 a
    per-pixel change of 1e-3 moves PSNR by at most about 0.09 dB)."""
    ts = two_sphere_scene(nerf, gpu, golden("f19_converge"))
    psnr_of = ts.psnr_of
    before, _ = psnr_of(*ts.ev)
    ts.train(300)
    grid = nerf.OccupancyGrid(ts.bbox, device=gpu).update(ts.emb, [ts.coarse, ts.fine])

    for name, (o, d, t) in (("held-out", ts.ev), ("novel", ts.nv)):
        dense, _ = psnr_of(o, d, t)
        assert name != "held-out" or dense > before + 3.0, "fixture: the scene should have been learnt"
        for label, over in (("no grid", {}), ("default grid", {"occupancy": grid})):
            got, ex = psnr_of(o, d, t, early_stop=1e-3, **over)
            n, P = nerf.last_early_stop_counts()       # the fine pass of the last chunk
            print(f"{name}, {label}: dense {dense:.3f} dB, early_stop 1e-3 {got:.3f} dB; samples alive: coarse "
                  f"{100 * float(ex['early_stop_samples0'].float().mean()) / 64:.1f} %, fine "
                  f"{100 * float(ex['early_stop_samples'].float().mean()) / 192:.1f} %; fine pass evaluated {n} of {P} "
                  f"points ({100.0 * n / P:.1f} %)")
            assert abs(dense - got) <= 0.1, f"{name}, {label}: dense {dense:.3f} dB vs {got:.3f} dB with early_stop"
