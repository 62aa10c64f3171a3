"""Grid ray marching for forward-only rendering (csrc/march.hip, render_rays(march=)), needs
an MI355X.

The scene of forward_only.py (build_scene) with the sigma row of both networks scaled by
SIGMA_SCALE = 500 as test_gpu_early_stop.py does, so that rays through occupied cells become opaque.

What is exact and what is not: the packed lists (counts, offsets, positions, depths, distances) are the NumPy
fp32 restatement bit for bit, and the packed raw rows are the rows of the masked dense render bit for bit (the
hash gather and the MLP outputs of a point do not depend on its tile or row). The composited maps are NOT bit
for bit: both sides form the same per-sample floats and the same non-unit fp64 factors in the same order, but
the fp64 product and sums associate differently. For <= 4096 terms that is <= 2^-40 relative before the single
rounding to fp32, so (float)T differs by at most one fp32 ulp and w by 2^-22 relative; each w c is within
1.5 2^-22 and all terms are non-negative, hence |d rgb| <= 4.2e-7 (9e-7 with the white background),
|d acc| <= 3e-7: the tests use atol 2e-6 (the project's F7 atol). Depth's numerator and acc each are within
4.2e-7 relative, so depth is within 1e-6 and disp within 1.5e-6 relative: the tests use rtol 4e-6 and demand an
identical NaN pattern. A dropped sample, a wrong dist or a lost carry moves the maps by 1e-3 or more.

Measured on the MI355X (test_packed_composite_is_the_dense_kernel, all ten cases together): 0 of 164 924
entries (rgb, disp, acc, depth, weights) are not bit-identical; the test prints the number.
"""
import functools

import numpy as np
import pytest
import torch

from forward_only import FAR, H, NEAR, W, ball_mask, bits_equal, build_scene, np_query, random_mask, scatter_back

pytestmark = pytest.mark.gpu

SIGMA_SCALE = 500.0
f32 = np.float32
MAP_ATOL = 2e-6          # rgb, acc
DEPTH_RTOL = 4e-6        # depth, disp (where finite; identical NaN pattern)


# ---------------------------------------------------------------- NumPy restatements
def np_lattice(rays, K):
    """The lattice of packed rows in fp32, every operation rounded: z [R, K], pts [R, K, 3], dist [R, K]."""
    rays = np.asarray(rays, f32)
    t = torch.linspace(0., 1., steps=K).numpy().astype(f32)
    near, far = rays[:, 6:7], rays[:, 7:8]
    z = (near * (f32(1.0) - t)).astype(f32) + (far * t).astype(f32)
    pts = rays[:, None, 0:3] + (rays[:, None, 3:6] * z[..., None]).astype(f32)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((len(rays), 1), 1e10, f32)], -1).astype(f32)
    return z.astype(f32), pts.astype(f32), dist


def np_march(rays, K, lo, hi, mask):
    z, pts, dist = np_lattice(rays, K)
    keep = np_query(pts.reshape(-1, 3), lo, hi, mask).reshape(len(rays), K)
    counts = keep.sum(-1).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return keep, counts, offsets, pts[keep], z[keep], dist[keep]


def np_bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def hand_rays(lo, hi):
    """Rays a frame does not have; row 0 starts inside the box and leaves it."""
    mid = 0.5 * (lo + hi)
    rows = [
        (mid, [0, 0, -1], 0.0, FAR),                       # starts inside, leaves through the floor
        (hi + 1, [1, 0, 0], NEAR, FAR),                    # misses the box
        (mid, [0.3, 0.2, 0.1], 0.0, 3.0),                  # stays inside
        (mid, [1, 0, 0], 1.0, 1.0),                        # near == far: K samples of one point
        ([np.nan, 0, 0], [0, 0, -1], NEAR, FAR),           # NaN origin: nothing kept
        ([0, 0, hi[2] + 2], [1, 0, 0], NEAR, FAR),         # above the box, parallel to it
    ]
    return np.array([np.concatenate([np.asarray(o, f32), np.asarray(d, f32), [f32(n), f32(f)]]) for o, d, n, f in rows],
                    f32)


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    sc = build_scene(nerf, gpu, SIGMA_SCALE)
    lo, hi, packed = sc["lo"], sc["hi"], sc["packed"]
    frame_rays = np.concatenate([packed(i).cpu().numpy() for i in (0, 1)])
    hand = hand_rays(lo, hi)
    vd = hand[:, 3:6] / np.linalg.norm(hand[:, 3:6], axis=-1, keepdims=True)
    pool = np.concatenate([np.concatenate([hand, vd.astype(f32)], -1), frame_rays]).astype(f32)
    return dict(sc, frame=functools.partial(sc["frame"], retraw=False), pool=pool)


MASKS = {"empty": lambda: np.zeros((4, 4, 4), bool), "full4": lambda: np.ones((4, 4, 4), bool),
         "ball16": ball_mask, "random5": lambda: random_mask(5), "random128": lambda: random_mask(128)}


# ---------------------------------------------------------------- 1. the lists are the NumPy rule
SHAPES = [(R, K) for R in (1, 63, 193, 4097) for K in (1, 64, 65, 200)] + [(63, 2048), (63, 4096)]


@pytest.mark.parametrize("name", list(MASKS))
def test_lists_match_numpy_bit_for_bit(nerf, gpu, scene, name):
    lo, hi, pool = scene["lo"], scene["hi"], scene["pool"]
    mask = MASKS[name]()
    grid = scene["grid_of"](mask)
    for R, K in SHAPES:
        rows11 = np.tile(pool, (R // len(pool) + 1, 1))[:R]
        keep, counts, offsets, pts_c, z_c, dist_c = np_march(rows11, K, lo, hi, mask)
        share = float(keep.mean())
        if R >= 63 and K >= 64:
            assert (counts == 0).any(), "fixture: some rays keep nothing"
            if name in ("ball16", "random5", "random128"):
                assert 0.0 < share < 1.0, f"fixture: kept share {share}"
            assert counts.min() == 0 and (name in ("empty",) or counts.max() > 0)
        if name == "empty":
            assert share == 0.0
        for C in (8, 11):
            got = grid.march(torch.from_numpy(np.ascontiguousarray(rows11[:, :C])).to(gpu), K)
            g_counts, g_off, g_pts, g_z, g_dist, g_sh = got
            what = f"{name} R {R} K {K} C {C}"
            assert g_counts.dtype == torch.int32 and g_off.dtype == torch.int32 and g_off.shape == (R + 1,)
            assert np.array_equal(g_counts.cpu().numpy(), counts), f"{what}: counts"
            assert np.array_equal(g_off.cpu().numpy(), offsets), f"{what}: offsets"
            assert np_bits_equal(g_pts.cpu().numpy(), pts_c), f"{what}: pts_c"
            assert np_bits_equal(g_z.cpu().numpy(), z_c), f"{what}: z_c"
            assert np_bits_equal(g_dist.cpu().numpy(), dist_c), f"{what}: dist_c"
            assert grid.last_counts() == (int(offsets[-1]), R * K)
            if C == 8:
                assert g_sh is None
            else:
                assert g_sh.shape == (int(offsets[-1]), 16) and g_sh.dtype == torch.float32


# ---------------------------------------------------------------- 2. packed compositing = the dense kernel
def composite_inputs(R, S):
    rng = np.random.RandomState(9)
    raw = (rng.randn(R, S, 4) * 2).astype(f32)
    z = np.sort(2 + 4 * rng.rand(R, S), -1).astype(f32)
    d = rng.randn(R, 3).astype(f32)
    p = rng.rand(R)
    p[:3] = 0
    p[3:6] = 1
    keep = rng.rand(R, S) < p[:, None]
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((R, 1), 1e10, f32)], -1).astype(f32)
    return raw, z, d, keep, dist


def march_composite(gpu, raw, z, d, keep, dist, white):
    """nerf_march_composite on the packed rows of the dense inputs."""
    import indoor_nerf_amd._lib as L
    R = raw.shape[0]
    n = int(keep.sum())
    off = np.concatenate([[0], np.cumsum(keep.sum(-1))]).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)   # noqa: E731
    raw_c, z_c, dist_c, off_t, d_t = dev(raw[keep]), dev(z[keep]), dev(dist[keep]), dev(off), dev(d)
    f = dict(device=gpu, dtype=torch.float32)
    rgb, disp, acc, depth, w = (torch.empty(R, 3, **f), torch.empty(R, **f), torch.empty(R, **f), torch.empty(R, **f),
                                torch.empty(n, **f))
    L.call("nerf_march_composite", L.ptr(raw_c), L.ptr(z_c), L.ptr(dist_c), L.ptr(off_t, "offsets", torch.int32),
           L.ptr(d_t), R, n, int(white), L.ptr(rgb), L.ptr(disp), L.ptr(acc), L.ptr(depth), L.ptr(w), L.stream())
    return dict(rgb=rgb.cpu().numpy(), disp=disp.cpu().numpy(), acc=acc.cpu().numpy(), depth=depth.cpu().numpy(),
                weights=w.cpu().numpy())


def assert_classes(acc, what):
    lo, hi, zero = int((acc < 0.5).sum()), int((acc > 0.9).sum()), int((acc == 0).sum())
    print(f"{what}: {lo} rays with acc < 0.5, {hi} with acc > 0.9, {zero} with acc = 0")
    assert lo >= 10 and hi >= 10 and zero >= 3, f"fixture {what}: {lo} / {hi} / {zero}"


def assert_maps_close(got, ref, what):
    np.testing.assert_allclose(got["rgb"], ref["rgb"], rtol=0, atol=MAP_ATOL, err_msg=f"{what}: rgb")
    np.testing.assert_allclose(got["acc"], ref["acc"], rtol=0, atol=MAP_ATOL, err_msg=f"{what}: acc")
    for k in ("depth", "disp"):
        if k in got and k in ref:
            assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), f"{what}: {k} NaN pattern"
            np.testing.assert_allclose(got[k], ref[k], rtol=DEPTH_RTOL, atol=0, equal_nan=True, err_msg=f"{what}: {k}")


def test_packed_composite_is_the_dense_kernel(nerf, gpu):
    R, different, total = 193, 0, 0
    for S in (1, 64, 65, 200, 512):
        raw, z, d, keep, dist = composite_inputs(R, S)
        kept = keep.sum(-1)
        if S >= 64:
            assert kept.min() == 0 and kept.max() == S
        for white in (False, True):
            with torch.no_grad():
                out = nerf.raw2outputs(torch.from_numpy(raw * keep[..., None]).to(gpu), torch.from_numpy(z).to(gpu),
                                       torch.from_numpy(d).to(gpu), 0, white)
            ref = dict(zip(("rgb", "disp", "acc", "weights", "depth"), (o.cpu().numpy() for o in out[:5])))
            what = f"S {S} white {white}"
            if S >= 64:
                assert_classes(ref["acc"], what)
            got = march_composite(gpu, raw, z, d, keep, dist, white)
            assert_maps_close(got, ref, what)
            np.testing.assert_allclose(got["weights"], ref["weights"][keep], rtol=2.5e-7, atol=1e-30,
                                       err_msg=f"{what}: weights")
            for k in ("rgb", "disp", "acc", "depth"):
                different += int((got[k].view(np.int32) != ref[k].view(np.int32)).sum())
                total += got[k].size
            different += int((got["weights"].view(np.int32) != ref["weights"][keep].view(np.int32)).sum())
            total += got["weights"].size
    print(f"packed compositing vs the dense kernel: {different} of {total} entries are not bit-identical")


def test_packed_composite_2048_against_the_oracle(nerf, gpu, oracle):
    R, S = 63, 2048
    raw, z, d, keep, dist = composite_inputs(R, S)
    for white in (False, True):
        out = oracle.composite(torch.from_numpy(raw * keep[..., None]), torch.from_numpy(z), torch.from_numpy(d), None,
                               white)
        ref = dict(zip(("rgb", "disp", "acc", "weights", "depth"), (o.numpy() for o in out[:5])))
        assert_classes(ref["acc"], f"S {S} white {white}")
        got = march_composite(gpu, raw, z, d, keep, dist, white)
        for k in ("rgb", "disp", "acc", "depth"):
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=2e-6, equal_nan=True, err_msg=f"white {white}: {k}")


# ---------------------------------------------------------------- 3. the march = the masked dense render
def march_rays(nerf, scene, i, grid, K, **over):
    with torch.no_grad():
        return nerf.render_rays(scene["packed"](i), march=grid, march_samples=K, retraw=True, **scene["ray_kw"](**over))


def maps_of(d):
    return {k: d[k + "_map"].reshape(H * W, -1).squeeze(-1).cpu().numpy() for k in ("rgb", "acc", "depth")}


@pytest.mark.parametrize("which", ["ball16", "random5"])
def test_march_is_the_masked_dense_render(nerf, gpu, scene, which):
    """Fixture conditions, asserted on the reference: at every K some ray has acc > 0.3 (what SIGMA_SCALE is
    for); some ray has acc = 0, at every K through the ball and at some K through random5 (measured on the
    MI355X: at K = 200 every ray of both frames meets an occupied cell of random5 with sigma > 0, which no
    scale changes; at K = 64 some do not)."""
    grid = scene["grid_of"](MASKS[which]())
    empty_any = 0
    for K in (64, 200, 512):
        empty_any += march_against_masked_dense(nerf, scene, which, grid, K)
    assert empty_any > 0, "fixture: no ray with acc = 0 at any K"


def march_against_masked_dense(nerf, scene, which, grid, K):
    fine = scene["kw"]["network_fine"]
    opaque = empty = 0
    for i in (0, 1):
        ref = scene["frame"](i, retraw=True, N_samples=K, N_importance=0, occupancy=grid, network_fn=fine)
        pts, raw = ref["pts"].reshape(H * W, K, 3), ref["raw"].reshape(H * W, K, 4)
        q = grid.query(pts)
        opaque += int((ref["acc_map"] > 0.3).sum())
        empty += int((ref["acc_map"] == 0).sum())
        got = march_rays(nerf, scene, i, grid, K)
        assert sorted(got) == ["acc_map", "depth_map", "march_offsets", "march_samples", "pts", "raw", "rays_d", "rgb_map",
                               "z_vals"]
        what = f"{which} pose {i} K {K}"
        assert got["march_samples"].dtype == torch.int32
        assert torch.equal(got["march_samples"].long(), q.sum(-1)), f"{what}: march_samples"
        assert int(got["march_offsets"][-1]) == int(q.sum()) and grid.last_counts() == (int(q.sum()), H * W * K)
        assert bits_equal(got["pts"], pts[q]), f"{what}: packed pts"
        assert bits_equal(got["raw"], raw[q]), f"{what}: packed raw"
        assert bits_equal(got["rays_d"], ref["rays_d"].reshape(H * W, 3))
        assert_maps_close(maps_of(got), maps_of(ref), what)
        # the frame through render(): any chunking, any slicing of the point list, the same bits
        base = scene["frame"](i, chunk=4096, march=grid, march_samples=K)
        assert sorted(base) == ["acc_map", "depth_map", "march_samples", "rays_d", "rgb_map"]
        for k in ("rgb_map", "depth_map", "acc_map"):
            assert bits_equal(base[k].reshape(got[k].shape), got[k]), f"{what}: render() vs render_rays, {k}"
        for over in (dict(chunk=37), dict(chunk=4096, march_points=1000), dict(chunk=37, march_points=1000)):
            other = scene["frame"](i, march=grid, march_samples=K, **over)
            for k in base:
                assert bits_equal(other[k], base[k]), f"{what} {over}: {k}"
    print(f"{which} K {K}: reference has {opaque} rays with acc > 0.3 and {empty} with acc = 0 of {2 * H * W}")
    assert opaque > 0, "fixture: raise SIGMA_SCALE"
    assert empty > 0 or which != "ball16", "fixture: no ray with acc = 0"
    return empty


# ---------------------------------------------------------------- 4. beyond 512 samples
def test_march_2048_samples(nerf, gpu, scene, oracle):
    K, mask = 2048, ball_mask()
    grid = scene["grid_of"](mask)
    for i in (0, 1):
        rays = scene["packed"](i).cpu().numpy()
        keep, counts, offsets, pts_c, z_c, _ = np_march(rays, K, scene["lo"], scene["hi"], mask)
        got = march_rays(nerf, scene, i, grid, K)
        assert np.array_equal(got["march_samples"].cpu().numpy(), counts)
        assert np.array_equal(got["march_offsets"].cpu().numpy(), offsets)
        assert np_bits_equal(got["pts"].cpu().numpy(), pts_c) and np_bits_equal(got["z_vals"].cpu().numpy(), z_c)
        assert 0 < counts.max() and counts.min() == 0
        z, _, _ = np_lattice(rays, K)
        raw = np.zeros((H * W, K, 4), f32)
        raw[keep] = got["raw"].cpu().numpy()
        out = oracle.composite(torch.from_numpy(raw), torch.from_numpy(z), torch.from_numpy(rays[:, 3:6].copy()), None,
                               True)
        m = maps_of(got)
        for k, ref in (("rgb", out[0]), ("acc", out[2]), ("depth", out[4])):
            np.testing.assert_allclose(m[k], ref.numpy(), rtol=1e-5, atol=2e-6, equal_nan=True, err_msg=f"pose {i}: {k}")


# ---------------------------------------------------------------- 5. composition with ray_bounds
def test_march_with_ray_bounds_is_the_hand_composition(nerf, gpu, scene):
    grid = scene["grid_of"](ball_mask())
    for i in (0, 1):
        for chunk in (37, 4096):
            rays = scene["packed"](i)
            hit, span, rows, rays_c = grid.bound_rays(rays)
            assert 0 < rows.shape[0] < H * W                     # the frame has misses
            with torch.no_grad():
                part = nerf.batchify_rays(rays_c, chunk, march=grid, march_samples=64, **scene["ray_kw"]())
            got = scene["frame"](i, chunk=chunk, ray_bounds=grid, march=grid, march_samples=64)
            assert sorted(got) == sorted(list(part) + ["ray_hit", "ray_span"])
            for k, full in scatter_back(part, hit).items():
                assert bits_equal(got[k], full), f"pose {i} chunk {chunk}: {k}"
            assert bool((got["march_samples"][~got["ray_hit"]] == 0).all())
            assert bool((got["march_samples"][got["ray_hit"]] > 0).any())


def test_march_with_ray_bounds_and_no_hit_makes_no_field_call(nerf, gpu, scene):
    grid = scene["grid_of"](np.zeros((16, 16, 16), bool))
    calls = []
    nqf = scene["kw"]["network_query_fn"]

    def recording(pts, viewdirs, fn):
        calls.append(tuple(pts.shape))
        return nqf(pts, viewdirs, fn)

    got = scene["frame"](0, ray_bounds=grid, march=grid, march_samples=64, network_query_fn=recording)
    assert calls == []
    ref = scene["frame"](0, ray_bounds=scene["grid_of"](ball_mask()), march=scene["grid_of"](ball_mask()),
                         march_samples=64)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
    assert not got["ray_hit"].any()
    assert bool((got["rgb_map"] == 1).all() and (got["acc_map"] == 0).all() and (got["march_samples"] == 0).all())
    assert bool(torch.isnan(got["depth_map"]).all())
    assert bits_equal(got["ray_span"], scene["packed"](0)[:, 6:8].reshape(H, W, 2))
    # without ray_bounds an empty grid composites every ray to the background, again without a field call
    got = scene["frame"](0, march=grid, march_samples=64, network_query_fn=recording)
    assert calls == []
    assert bool((got["rgb_map"] == 1).all() and (got["acc_map"] == 0).all() and torch.isnan(got["depth_map"]).all())
    scene["frame"](0, march=scene["grid_of"](ball_mask()), march_samples=64, network_query_fn=recording)
    assert len(calls) == 1 and len(calls[0]) == 2 and calls[0][1] == 3     # the recorder does record: one packed list


# ---------------------------------------------------------------- 6. guards
def test_guards(nerf, gpu, scene):
    kw = scene["kw"]
    grid = scene["grid_of"](np.ones((4, 4, 4), bool))

    def run(**over):
        return scene["frame"](0, **dict(dict(march=grid, march_samples=16), **over))

    run()                                                                   # the supported combination
    with pytest.raises(ValueError, match="march must be an OccupancyGrid"):
        run(march=0.5)
    for bad in (0, 4097, 2.5):
        with pytest.raises(ValueError, match="march.*march_samples"):
            run(march_samples=bad)
    with pytest.raises(ValueError, match="march.*march_points"):
        run(march_points=0)
    with pytest.raises(ValueError, match="march does not combine"):
        run(occupancy=grid)
    with pytest.raises(ValueError, match="march does not combine"):
        run(early_stop=0.05)
    with torch.enable_grad(), pytest.raises(ValueError, match="march is forward-only"):
        nerf.render(H, W, scene["K"], c2w=scene["poses"][0][:3, :4].to(gpu), **dict(kw, march=grid))
    with pytest.raises(ValueError, match="march needs raw_noise_std"):
        run(raw_noise_std=1.0)
    with pytest.raises(ValueError, match="march needs perturb"):
        run(perturb=1.0)
    with pytest.raises(ValueError, match="march needs lindisp"):
        run(lindisp=True)
    with pytest.raises(ValueError, match="march does not support predict_normals"):
        run(predict_normals=True)
    head = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                          input_ch=32, input_ch_views=16, predict_normals=True).to(gpu).eval()
    with pytest.raises(ValueError, match="march does not support predict_normals or a normals head"):
        run(network_fine=head)
    emb_q = nerf.HashEmbedder(scene["bbox"], log2_hashmap_size=14, finest_resolution=512, use_quantization=True)
    emb_q = emb_q.to(gpu).eval()
    sh = nerf.SHEncoder()
    with pytest.raises(ValueError, match="march: A-CAQ"):
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, fn, emb_q, sh), embed_fn=emb_q)
    with pytest.raises(ValueError, match="march: A-CAQ"):                   # caught by the field call without embed_fn
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, fn, emb_q, sh), embed_fn=None)
    with pytest.raises(ValueError, match="march needs ray rows with view directions"):
        run(use_viewdirs=False)
    with pytest.raises(ValueError, match="retraw is not available with march"):
        run(retraw=True)
    # a query function that does not reach this package's run_network must not fall back to anything
    with pytest.raises(ValueError, match="march needs a network_query_fn"):
        run(network_query_fn=lambda p, v, fn: torch.zeros(p.shape[0], 4, device=p.device))


def test_without_the_keyword_nothing_changes(nerf, gpu, scene):
    """march=None is the call without it: same entries, same bits."""
    a, b = scene["frame"](0, retraw=True), scene["frame"](0, retraw=True, march=None, march_samples=64)
    assert sorted(a) == sorted(b) and "march_samples" not in a
    for k in a:
        assert bits_equal(a[k], b[k]), k
