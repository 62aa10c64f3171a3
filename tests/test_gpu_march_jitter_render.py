"""The jittered grid march through render_rays (march_jitter=True with perturb > 0), needs an MI355X.

The scene and the helpers of test_gpu_march_grad.py: build_scene with the sigma row of both networks scaled by 500,
300 rays of its two frames, K = 192 and 300, the ball, random_mask(16), every cell set and no cell set.

The yardstick is the masked dense render that exists today, run after the same render.manual_seed: the dense coarse
pass draws one (seed, offset) pair per chunk and so does the march, so both jitter sample k of ray r by the same
uniform. Under torch.no_grad() the dense side is render_rays(N_samples=K, N_importance=0, perturb=1.0, occupancy=grid)
through network_fine; under gradients it is the same call with a network_query_fn that multiplies run_network's raw by
grid.query(pts), as test_gpu_march_grad.py. The dense call does not return its depths, so they are formed here by
nerf_sample_stratified with the pair render._rng() hands out after that manual_seed, and held to the dense call's pts
bit for bit.

Bars: the march's z_vals and pts are the dense arrays' kept entries bit for bit. The maps agree at the bars
test_gpu_march.py uses for the unjittered comparison (its lines 33-34 and 166-172): rgb and acc within MAP_ATOL = 2e-6
absolute, depth within DEPTH_RTOL = 4e-6 relative with the same NaN pattern: both sides composite the same samples
and differ in the fp64 association only, jittered or not. The gradients are held to test_gpu_march_grad.py's bars
(tables within 1e-5 of the level's largest |gradient|, the MLP within 1e-6 of the norm) with that file's depth mask.
Each test prints its figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

from forward_only import H, W, bits_equal, build_scene
from test_gpu_march import DEPTH_RTOL, MAP_ATOL
from test_gpu_march_grad import MASKS, R, SIGMA_SCALE, compare, grads_of, march

pytestmark = pytest.mark.gpu

SEED = 1234


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    sc = build_scene(nerf, gpu, SIGMA_SCALE)
    rays = torch.cat([sc["packed"](0), sc["packed"](1)])[:R].contiguous()
    target = torch.rand(R, 3, device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    fine = sc["kw"]["network_fine"]
    params = list(sc["emb"].parameters()) + list(fine.parameters())
    return dict(sc, rays=rays, target=target, fine=fine, params=params, n_tab=sc["emb"].n_levels)


def seeded(nerf, seed, fn):
    importlib.import_module("indoor_nerf_amd.render").manual_seed(seed)
    return fn()


def jittered(nerf, scene, grid, K, seed=SEED, **over):
    return seeded(nerf, seed, lambda: march(nerf, scene, grid, K, march_jitter=True, perturb=1.0, **over))


def dense_depths(nerf, scene, K, seed=SEED, pytest_u=False):
    """The dense coarse pass's jittered depths z [R, K] and points [R, K, 3] for the chunk scene["rays"]: the sampler
    with the pair the next render call after manual_seed(seed) draws, or with the pytest uniforms."""
    from indoor_nerf_amd import _lib as L
    render = importlib.import_module("indoor_nerf_amd.render")
    rays, gpu = scene["rays"], scene["rays"].device
    if pytest_u:
        u, s, o = render._pytest_uniforms((R, K), gpu), 0, 0
    else:
        render.manual_seed(seed)
        u, (s, o, rng) = None, render._rng()
        assert rng is None
    z, pts = torch.empty(R, K, device=gpu), torch.empty(R, K, 3, device=gpu)
    L.call("nerf_sample_stratified", L.ptr(rays), 11, R, K, L.ptr(render._linspace(K, gpu)), 0, 1,
           L.ptr(u, "u", allow_none=True), s, o, None, L.ptr(z), L.ptr(pts), None, None, L.stream())
    return z, pts


def dense_masked(nerf, scene, grid, K, seed=SEED, grad=False, **over):
    """The masked dense render with perturb = 1 after manual_seed(seed): occupancy=grid under no_grad, the masking
    query function under gradients."""
    kw = dict(N_samples=K, N_importance=0, perturb=1.0, network_fn=scene["fine"], **over)
    if grad:
        nqf = scene["kw"]["network_query_fn"]
        kw["network_query_fn"] = lambda pts, viewdirs, fn: nqf(pts, viewdirs, fn) * grid.query(pts)[..., None]
    else:
        kw["occupancy"] = grid
    return seeded(nerf, seed, lambda: nerf.render_rays(scene["rays"], **scene["ray_kw"](**kw)))


def maps_of(d):
    return {k: d[k + "_map"].detach().reshape(R, -1).squeeze(-1).cpu().numpy() for k in ("rgb", "acc", "depth")}


def assert_maps_close(got, ref, what):
    got, ref = maps_of(got), maps_of(ref)
    nan = np.isnan(ref["depth"])
    worst = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("rgb", "acc")}
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got["depth"] - ref["depth"])[~nan] / np.abs(ref["depth"])[~nan]
    print(f"{what}: worst |d rgb| {worst['rgb']:.3e}, |d acc| {worst['acc']:.3e} (bar {MAP_ATOL:.0e}); worst depth "
          f"rel {float(rel.max()) if rel.size else 0.0:.3e} (bar {DEPTH_RTOL:.0e}); {int(nan.sum())} NaN depths")
    np.testing.assert_allclose(got["rgb"], ref["rgb"], rtol=0, atol=MAP_ATOL, err_msg=f"{what}: rgb")
    np.testing.assert_allclose(got["acc"], ref["acc"], rtol=0, atol=MAP_ATOL, err_msg=f"{what}: acc")
    assert np.array_equal(np.isnan(got["depth"]), nan), f"{what}: depth NaN pattern"
    np.testing.assert_allclose(got["depth"], ref["depth"], rtol=DEPTH_RTOL, atol=0, equal_nan=True,
                               err_msg=f"{what}: depth")


# ---------------------------------------------------------------- perturb == 0: the plain march
@pytest.mark.parametrize("K", [192, 300])
@pytest.mark.parametrize("name", ["ball", "random"])
def test_without_perturb_it_is_the_plain_march(nerf, gpu, scene, name, K):
    grid = scene["grid_of"](MASKS[name]())
    from indoor_nerf_amd import _lib
    with torch.no_grad():
        plain = march(nerf, scene, grid, K, retraw=True)
        _lib.set_timing(True)
        try:
            got = march(nerf, scene, grid, K, retraw=True, march_jitter=True, perturb=0.)
            names = [n for n, _, _ in _lib.timing_records()]
        finally:
            _lib.set_timing(False)
    assert "nerf_march_count" in names and not [n for n in names if "jitter" in n], names
    with torch.enable_grad():
        plain_g = march(nerf, scene, grid, K, retraw=True, march_grad=True)
        got_g = march(nerf, scene, grid, K, retraw=True, march_grad=True, march_jitter=True, perturb=0.)
    for a, b in ((got, plain), (got_g, plain_g), (got_g, plain)):
        assert set(a) == set(b)
        for k in a:
            assert bits_equal(a[k].detach(), b[k].detach()), k
    assert got_g["rgb_map"].requires_grad and int(plain["march_samples"].sum()) > 0


# ---------------------------------------------------------------- the jitter = the masked dense render's
@pytest.mark.parametrize("K", [192, 300])
@pytest.mark.parametrize("name", list(MASKS))
def test_jittered_march_is_the_masked_dense_render(nerf, gpu, scene, name, K):
    grid = scene["grid_of"](MASKS[name]())
    z, pts = dense_depths(nerf, scene, K)
    with torch.no_grad():
        ref = dense_masked(nerf, scene, grid, K, retraw=True)
        _lib = importlib.import_module("indoor_nerf_amd._lib")
        _lib.set_timing(True)
        try:
            got = jittered(nerf, scene, grid, K, retraw=True)
            names = [n for n, _, _ in _lib.timing_records()]
        finally:
            _lib.set_timing(False)
        plain = march(nerf, scene, grid, K, retraw=True)
    assert names[0] == "nerf_jitter_march_count" and ("nerf_jitter_march_write" in names) == (name != "empty") and \
        not [n for n in names if n in ("nerf_march_count", "nerf_march_write")], names
    assert bits_equal(ref["pts"].reshape(R, K, 3), pts), "the dense call drew other numbers than dense_depths"
    keep = grid.query(pts)
    n = int(keep.sum())
    print(f"{name} K={K}: {n} of {R * K} jittered samples kept; the plain lattice keeps {int(plain['march_samples'].sum())}")
    assert sorted(got) == ["acc_map", "depth_map", "march_offsets", "march_samples", "pts", "raw", "rays_d", "rgb_map",
                           "z_vals"]
    assert torch.equal(got["march_samples"].long(), keep.sum(-1)) and int(got["march_offsets"][-1]) == n
    assert grid.last_counts() == (int(plain["march_samples"].sum()), R * K)      # the plain call came last
    assert bits_equal(got["z_vals"], z[keep]), "z_vals"
    assert bits_equal(got["pts"], pts[keep]), "pts"
    assert bits_equal(got["raw"], ref["raw"].reshape(R, K, 4)[keep]), "raw"
    assert (n == 0) == (name == "empty")
    if name != "empty":
        assert not bits_equal(got["z_vals"][:64], plain["z_vals"][:64]) or n != int(plain["march_samples"].sum())
    assert_maps_close(got, ref, f"{name} K={K}")


@pytest.mark.parametrize("K", [192, 300])
@pytest.mark.parametrize("name", ["ball", "random", "full"])
def test_gradients_match_the_masked_dense_path(nerf, gpu, scene, name, K):
    grid = scene["grid_of"](MASKS[name]())
    with torch.no_grad():
        ref = jittered(nerf, scene, grid, K)
    m = (ref["march_samples"] > 0) & (ref["acc_map"] > 0)      # test_gpu_march_grad.py's depth mask, of this jitter
    print(f"{name} K={K}: {int((ref['march_samples'] > 0).sum())} rays with samples, {int(m.sum())} with acc > 0")
    assert int(m.sum()) > R // 10, "fixture: too few rays carry the depth term"
    got, out = grads_of(nerf, scene, lambda: (jittered(nerf, scene, grid, K, march_grad=True), m))
    want, dense = grads_of(nerf, scene, lambda: (dense_masked(nerf, scene, grid, K, grad=True), m))
    for k in ("rgb_map", "depth_map", "acc_map"):
        assert bits_equal(out[k], ref[k]), f"{k}: the march under gradients against the same seed under no_grad"
    for k in ("rgb_map", "acc_map"):
        d = float((out[k] - dense[k]).abs().max())
        print(f"{name} K={K}: worst |d {k}| {d:.3e} (bar {MAP_ATOL:.0e})")
        assert d <= MAP_ATOL, k
    compare(got, want, scene["n_tab"], f"jitter {name} K={K}")


# ---------------------------------------------------------------- seeds and pytest
def test_seeds(nerf, gpu, scene):
    grid = scene["grid_of"](MASKS["random"]())
    with torch.no_grad():
        a = jittered(nerf, scene, grid, 192, seed=1, retraw=True)
        b = jittered(nerf, scene, grid, 192, seed=1, retraw=True)
        c = jittered(nerf, scene, grid, 192, seed=2, retraw=True)
        d = march(nerf, scene, grid, 192, march_jitter=True, perturb=1.0, retraw=True)      # the next draw of seed 2
    for k in a:
        assert bits_equal(a[k], b[k]), k
    for other in (c, d):
        assert other["z_vals"].shape != a["z_vals"].shape or not bits_equal(other["z_vals"], a["z_vals"])
    assert c["z_vals"].shape != d["z_vals"].shape or not bits_equal(c["z_vals"], d["z_vals"])


@pytest.mark.parametrize("K", [192, 300])
def test_pytest_uniforms_are_the_dense_path_s(nerf, gpu, scene, K):
    grid = scene["grid_of"](MASKS["ball"]())
    z, pts = dense_depths(nerf, scene, K, pytest_u=True)
    with torch.no_grad():
        ref = dense_masked(nerf, scene, grid, K, pytest=True)
        got = march(nerf, scene, grid, K, march_jitter=True, perturb=1.0, pytest=True, retraw=True)
        again = jittered(nerf, scene, grid, K, seed=77, pytest=True, retraw=True)      # no seed takes part
    assert bits_equal(ref["pts"].reshape(R, K, 3), pts)
    keep = grid.query(pts)
    assert int(keep.sum()) > 0
    assert bits_equal(got["z_vals"], z[keep]) and bits_equal(got["pts"], pts[keep])
    for k in got:
        assert bits_equal(got[k], again[k]), k
    assert_maps_close(got, ref, f"pytest K={K}")


# ---------------------------------------------------------------- the training step and the forward-only companions
def test_forward_backward_with_the_keywords(nerf, gpu, scene):
    """model.forward_backward with march=, march_grad=True, march_jitter=True and perturb = 1 in its render keywords:
    after the same manual_seed its loss is bit for bit the loss written out by hand on render's rgb, and the gradients
    are those of img2mse(rgb, target).backward() within the bars (measured: every bit the same).

    The hand-written loss is mean((rgb - target)^2) as train_loss (csrc/loss.hip) documents it: the fp32 squares
    summed in fp64, rounded once to fp32, divided by the fp32 count. torch.mean's fp32 tree, which is what
    nerf.img2mse is and what test_gpu_march_grad.py compares with, rounds elsewhere: on this render (576 values)
    forward_backward gives 0.225319043 and img2mse 0.225319013, two units in the last place apart; that file's
    values happen to round alike. The loss launch is not touched by the keyword. The figure is printed."""
    model = importlib.import_module("indoor_nerf_amd.model")
    render = importlib.import_module("indoor_nerf_amd.render")
    K, emb = 192, scene["emb"]
    grid = scene["grid_of"](MASKS["ball"]())
    kw = dict(scene["kw"], march=grid, march_grad=True, march_jitter=True, march_samples=K, perturb=1.0)
    ro, rd = nerf.get_rays(H, W, scene["K"], scene["poses"][0][:3, :4].to(gpu))
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    target = scene["target"][:ro.shape[0]].contiguous()
    args = nerf.make_args(tv_loss_weight=0.0, sparse_loss_weight=1e-4, chunk=4096)
    opt = nerf.RAdam([{"params": list(scene["fine"].parameters()), "weight_decay": 1e-6},
                      {"params": list(emb.parameters()), "eps": 1e-15}], lr=1e-2, betas=(0.9, 0.99))
    nerf.set_deterministic(True)
    try:
        for p in scene["params"]:
            p.grad = None
        with torch.enable_grad():
            render.manual_seed(5)
            rgb, _, _, ex = nerf.render(0, 0, None, chunk=4096, rays=(ro, rd), **kw)
            assert "rgb0" not in ex and int(ex["march_samples"].sum()) > 0
            mse = nerf.img2mse(rgb, target)
            mse.backward()
            d = (rgb.detach() - target) ** 2
            hand = d.double().sum().float() / torch.tensor(float(d.numel()), device=gpu)
            with torch.no_grad():
                plain, _, _, _ = nerf.render(0, 0, None, chunk=4096, rays=(ro, rd), **dict(kw, perturb=0.))
        torch.cuda.synchronize()
        want = [None if p.grad is None else p.grad.detach().clone() for p in scene["params"]]
        with torch.enable_grad():
            render.manual_seed(5)
            loss, img_loss, psnr = model.forward_backward((ro, rd), target, kw, opt, args, 1)
        torch.cuda.synchronize()
        got = [None if p.grad is None else p.grad.detach().clone() for p in scene["params"]]
    finally:
        nerf.set_deterministic(False)
        for p in scene["params"]:
            p.grad = None
    print(f"loss {float(loss.detach()):.9g} by hand {float(hand):.9g}; torch.mean in fp32 {float(mse.detach()):.9g}")
    assert abs(float(loss.detach()) - float(mse.detach())) <= 4 * 2.0 ** -24 * float(mse.detach())
    assert torch.isfinite(loss) and not bits_equal(rgb.detach(), plain), "the jitter changed nothing"
    compare(got, want, scene["n_tab"], "forward_backward with march_jitter")
    assert bits_equal(loss.detach().reshape(1), hand.reshape(1))


def test_one_frame_with_sh_by_ray_and_the_bf16_mlp(nerf, gpu, scene):
    """Under torch.no_grad() the jittered list goes through the ray index and the bf16 forward: the frame is bit for
    bit that of march_sh="rows", and its depths are those of the fp32 call with the same seed."""
    grid = scene["grid_of"](MASKS["random"]())
    with torch.no_grad():
        rows = jittered(nerf, scene, grid, 192, retraw=True, march_sh="rows", mlp_precision="bf16")
        rays = jittered(nerf, scene, grid, 192, retraw=True, march_sh="rays", mlp_precision="bf16")
        fp32 = jittered(nerf, scene, grid, 192, retraw=True)
        sliced = jittered(nerf, scene, grid, 192, retraw=True, march_sh="rays", mlp_precision="bf16",
                          feature_precision="bf16", table_precision="fp16", march_points=1000)
        whole = jittered(nerf, scene, grid, 192, retraw=True, march_sh="rays", mlp_precision="bf16",
                         feature_precision="bf16", table_precision="fp16")
    assert set(rows) == set(rays) and int(rows["march_samples"].sum()) > 1000
    for k in rows:
        assert bits_equal(rows[k], rays[k]), k
        assert bits_equal(sliced[k], whole[k]), k
    for k in ("z_vals", "pts", "march_offsets", "march_samples"):
        assert bits_equal(rows[k], fp32[k]) and bits_equal(whole[k], fp32[k]), k
    assert not bits_equal(rows["raw"], fp32["raw"])
