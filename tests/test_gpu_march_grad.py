"""Training through the grid march (render_rays(march=, march_grad=True)), needs an MI355X.

The scene of forward_only.py (build_scene) with the sigma row of both networks scaled by SIGMA_SCALE = 500, as
test_gpu_march.py; 300 rays of its two frames; the grids are the ball, random_mask(16), every cell set and no cell set.

Forward: under gradients the three maps and march_samples are bit for bit those of the march under torch.no_grad()
(the same launches; the training MLP forward computes the same raw).

Gradients: against the masked dense path that exists today, render_rays(N_samples=K, N_importance=0, perturb=0) with a
network_query_fn that multiplies run_network's raw by grid.query(pts), both sides in deterministic mode with one loss
on rgb_map, depth_map and acc_map. A masked point's raw gradient is exactly zero, so both sides sum the same terms
in another association, and the bars are the project's for that situation (test_gpu_coarse_reuse.py): table
gradients within 1e-5 of the level's largest |gradient| (which is > 0), MLP gradients within 1e-6 of the
reference's norm. The depth term is masked by march_samples > 0 on both sides (a ray without a kept sample has NaN
depth), and by acc > 0 of the march under no_grad: a ray whose kept samples all have sigma <= 0 has acc = 0 and NaN
depth as well, on both sides, and one NaN would reach every shared weight. Those rays still take part through rgb and
acc. Each test prints its figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

from forward_only import H, W, ball_mask, bits_equal, build_scene, random_mask

pytestmark = pytest.mark.gpu

SIGMA_SCALE = 500.0
R = 300
MASKS = {"ball": ball_mask, "random": lambda: random_mask(16), "full": lambda: np.ones((16, 16, 16), bool),
         "empty": lambda: np.zeros((16, 16, 16), bool)}
TABLE_BAR, MLP_BAR = 1e-5, 1e-6


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    sc = build_scene(nerf, gpu, SIGMA_SCALE)
    rays = torch.cat([sc["packed"](0), sc["packed"](1)])[:R].contiguous()
    target = torch.rand(R, 3, device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    fine = sc["kw"]["network_fine"]
    params = list(sc["emb"].parameters()) + list(fine.parameters())
    return dict(sc, rays=rays, target=target, fine=fine, params=params, n_tab=sc["emb"].n_levels)


def march(nerf, scene, grid, K, **over):
    return nerf.render_rays(scene["rays"], march=grid, march_samples=K, **scene["ray_kw"](**over))


def loss_of(out, m, target):
    return (((out["rgb_map"] - target) ** 2).mean() + 0.1 * ((out["depth_map"][m] - 3.0) ** 2).sum() / R
            + ((out["acc_map"] - 0.5) ** 2).mean())


def grads_of(nerf, scene, render):
    """The parameter gradients of loss_of over render() in deterministic mode -> (list, the outputs detached)."""
    nerf.set_deterministic(True)
    try:
        for p in scene["params"]:
            p.grad = None
        with torch.enable_grad():
            out, m = render()
            loss_of(out, m, scene["target"]).backward()
        torch.cuda.synchronize()
        return [None if p.grad is None else p.grad.detach().clone() for p in scene["params"]], \
            {k: v.detach() for k, v in out.items() if torch.is_tensor(v)}
    finally:
        nerf.set_deterministic(False)
        for p in scene["params"]:
            p.grad = None


def depth_mask(nerf, scene, grid, K):
    with torch.no_grad():
        ref = march(nerf, scene, grid, K)
    return ref, (ref["march_samples"] > 0) & (ref["acc_map"] > 0)


def dense_render(nerf, scene, grid, K, m, rows=None):
    """The masked dense path of today (rows: a permutation of the rays, for the yardstick)."""
    nqf = scene["kw"]["network_query_fn"]

    def masked(pts, viewdirs, fn):
        return nqf(pts, viewdirs, fn) * grid.query(pts)[..., None]

    rays = scene["rays"] if rows is None else scene["rays"][rows].contiguous()
    out = nerf.render_rays(rays, **scene["ray_kw"](N_samples=K, N_importance=0, perturb=0., network_fn=scene["fine"],
                                                   network_query_fn=masked))
    if rows is not None:
        inv = torch.empty_like(rows)
        inv[rows] = torch.arange(rows.shape[0], device=rows.device)
        out = {k: (v[inv] if torch.is_tensor(v) and v.shape[:1] == (rays.shape[0],) else v) for k, v in out.items()}
    return out, m


def compare(got, want, n_tab, tag, need_all=True):
    worst_t = worst_m = 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), f"{tag}: param {i}"
        if a is None:
            continue
        if i < n_tab:
            scale = float(b.abs().max())
            worst_t = max(worst_t, float((a - b).abs().max()) / max(scale, 1e-30))
        else:
            worst_m = max(worst_m, float((a - b).norm()) / max(float(b.norm()), 1e-30))
    print(f"{tag}: tables worst |d| / max|g| {worst_t:.3e} (bar {TABLE_BAR:.0e}), MLP worst |d| / |g| {worst_m:.3e} "
          f"(bar {MLP_BAR:.0e})")
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None:
            continue
        if i < n_tab:
            scale = float(b.abs().max())
            assert scale > 0 or not need_all, f"{tag}: table {i}: no gradient"
            assert float((a - b).abs().max()) <= TABLE_BAR * scale + 1e-30, f"{tag}: table {i}"
        else:
            assert float((a - b).norm()) <= MLP_BAR * float(b.norm()) + 1e-30, f"{tag}: mlp param {i - n_tab}"
    assert any(g is not None for g in got), f"{tag}: no gradient at all"


@pytest.mark.parametrize("K", [192, 300])
@pytest.mark.parametrize("name", list(MASKS))
def test_forward_is_the_no_grad_march(nerf, gpu, scene, name, K):
    grid = scene["grid_of"](MASKS[name]())
    with torch.no_grad():
        plain = march(nerf, scene, grid, K)
        ref = march(nerf, scene, grid, K, march_grad=True, retraw=True)
    with torch.enable_grad():
        got = march(nerf, scene, grid, K, march_grad=True, retraw=True)
    assert set(got) == set(ref) == set(plain) | {"raw", "pts", "z_vals", "march_offsets"}
    for k in ("rgb_map", "depth_map", "acc_map"):
        assert bits_equal(got[k], ref[k]) and bits_equal(plain[k], ref[k]), k
        assert got[k].requires_grad and not ref[k].requires_grad
    assert torch.equal(got["march_samples"], ref["march_samples"]) and bits_equal(got["rays_d"], ref["rays_d"])
    assert bits_equal(got["raw"].detach(), ref["raw"]) and got["raw"].requires_grad
    assert torch.equal(got["march_offsets"], ref["march_offsets"]) and bits_equal(got["z_vals"], ref["z_vals"])
    n = int(ref["march_samples"].sum())
    assert got["raw"].shape == (n, 4) and (n == 0) == (name == "empty")
    print(f"{name} K={K}: {n} of {R * K} samples kept")


@pytest.mark.parametrize("K", [192, 300])
@pytest.mark.parametrize("name", ["ball", "random", "full"])
def test_gradients_match_the_masked_dense_path(nerf, gpu, scene, name, K):
    grid = scene["grid_of"](MASKS[name]())
    ref, m = depth_mask(nerf, scene, grid, K)
    print(f"{name} K={K}: {int((ref['march_samples'] > 0).sum())} rays with samples, {int(m.sum())} with acc > 0")
    assert int(m.sum()) > R // 10, "fixture: too few rays carry the depth term"
    got, out = grads_of(nerf, scene, lambda: (march(nerf, scene, grid, K, march_grad=True), m))
    want, dense = grads_of(nerf, scene, lambda: dense_render(nerf, scene, grid, K, m))
    for k in ("rgb_map", "acc_map"):
        assert float((out[k] - dense[k]).abs().max()) <= 2e-6, k      # test_gpu_march.py's MAP_ATOL: the same render
    compare(got, want, scene["n_tab"], f"{name} K={K}")


def test_no_cell_set(nerf, gpu, scene):
    """No kept sample: backward() runs, launches no field work, and every parameter gradient is None or zero."""
    from indoor_nerf_amd import _lib
    grid = scene["grid_of"](MASKS["empty"]())
    for p in scene["params"]:
        p.grad = None
    _lib.set_timing(True)
    try:
        with torch.enable_grad():
            out = march(nerf, scene, grid, 192, march_grad=True)
            assert out["rgb_map"].requires_grad
            (((out["rgb_map"] - scene["target"]) ** 2).mean() + out["acc_map"].sum()).backward()
        torch.cuda.synchronize()
        names = [n for n, _, _ in _lib.timing_records()]
    finally:
        _lib.set_timing(False)
    print("launches:", names)
    assert not [n for n in names if "hash_encode" in n or "mlp" in n or "owner" in n]
    assert bool((out["rgb_map"] == 1).all() and (out["acc_map"] == 0).all() and torch.isnan(out["depth_map"]).all())
    for p in scene["params"]:
        assert p.grad is None or not bool(p.grad.any())


@pytest.mark.parametrize("name", ["ball", "random"])
def test_slices_of_march_points(nerf, gpu, scene, name):
    """march_points smaller than the list: several applications of the field node and a ragged tail; the forward
    keeps its bits and the gradients stay within the bars of the unsliced call."""
    K = 192
    grid = scene["grid_of"](MASKS[name]())
    ref, m = depth_mask(nerf, scene, grid, K)
    n = int(ref["march_samples"].sum())
    assert n > 2000 and n % 1000 != 0, f"fixture: {n} points"
    want, whole = grads_of(nerf, scene, lambda: (march(nerf, scene, grid, K, march_grad=True), m))
    got, sliced = grads_of(nerf, scene, lambda: (march(nerf, scene, grid, K, march_grad=True, march_points=1000), m))
    for k in ("rgb_map", "depth_map", "acc_map"):
        assert bits_equal(sliced[k], whole[k]), k
    compare(got, want, scene["n_tab"], f"{name}: {n} points in slices of 1000")


def test_deterministic_mode_repeats_bit_for_bit(nerf, gpu, scene):
    grid = scene["grid_of"](MASKS["random"]())
    _, m = depth_mask(nerf, scene, grid, 192)
    for over in ({}, dict(march_points=1000)):
        a, _ = grads_of(nerf, scene, lambda: (march(nerf, scene, grid, 192, march_grad=True, **over), m))
        b, _ = grads_of(nerf, scene, lambda: (march(nerf, scene, grid, 192, march_grad=True, **over), m))
        assert any(g is not None and bool(g.any()) for g in a)
        for x, y in zip(a, b):
            assert (x is None) == (y is None) and (x is None or bits_equal(x, y))


@pytest.mark.parametrize("tv_w", [0.0, 1e-3], ids=["no_tv", "tv"])
def test_forward_backward_with_the_keywords(nerf, gpu, scene, tv_w):
    """model.forward_backward with march= and march_grad=True in its render keywords: the loss is bit for bit
    img2mse(rgb, target) (+ tv_w * sum TV) computed by hand through render; the gradients are those of that hand-written
    backward within the bars; one optimizer_update changes the tables."""
    model = importlib.import_module("indoor_nerf_amd.model")
    losses = importlib.import_module("indoor_nerf_amd.losses")
    K, emb = 192, scene["emb"]
    grid = scene["grid_of"](MASKS["ball"]())
    kw = dict(scene["kw"], march=grid, march_grad=True, march_samples=K)
    ro, rd = nerf.get_rays(H, W, scene["K"], scene["poses"][0][:3, :4].to(gpu))
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    target = scene["target"][:ro.shape[0]].contiguous()
    args = nerf.make_args(tv_loss_weight=tv_w, sparse_loss_weight=1e-4, chunk=4096)
    opt = nerf.RAdam([{"params": list(scene["fine"].parameters()), "weight_decay": 1e-6},
                      {"params": list(emb.parameters()), "eps": 1e-15}], lr=1e-2, betas=(0.9, 0.99),
                     degenerated_to_sgd=True)      # RAdam's first five steps move nothing without it
    nerf.set_deterministic(True)
    try:
        for p in scene["params"]:
            p.grad = None
        with torch.enable_grad():
            rgb, _, _, ex = nerf.render(0, 0, None, chunk=4096, rays=(ro, rd), **kw)
            assert "rgb0" not in ex and "sparsity_loss" not in ex and int(ex["march_samples"].sum()) > 0
            hand = nerf.img2mse(rgb, target)
            if tv_w > 0:
                tv = losses.total_variation_all(emb, generator=torch.Generator().manual_seed(5))
                hand = hand + tv_w * sum(tv[i] for i in range(tv.shape[0]))
            hand.backward()
        torch.cuda.synchronize()
        want = [None if p.grad is None else p.grad.detach().clone() for p in scene["params"]]
        with torch.enable_grad():
            loss, img_loss, psnr = model.forward_backward((ro, rd), target, kw, opt, args, 1,
                                                          tv_generator=torch.Generator().manual_seed(5))
        torch.cuda.synchronize()
        got = [None if p.grad is None else p.grad.detach().clone() for p in scene["params"]]
    finally:
        nerf.set_deterministic(False)
    lf, hf = float(loss.detach()), float(hand.detach())
    print(f"tv_w {tv_w}: loss {lf:.9g} by hand {hf:.9g}, |d| {abs(lf - hf):.3e}")
    assert args.tv_loss_weight == tv_w and torch.isfinite(loss)
    compare(got, want, scene["n_tab"], f"forward_backward tv_w {tv_w}")
    assert bits_equal(loss.detach().reshape(1), hand.detach().reshape(1))
    before = [p.detach().clone() for p in scene["params"]]
    try:
        model.optimizer_update(opt)
        torch.cuda.synchronize()
        n_tab = scene["n_tab"]
        changed = sum(int(not torch.equal(a, b.detach())) for a, b in zip(before[:n_tab], scene["params"][:n_tab]))
        print(f"tables changed by one update: {changed} of {n_tab}")
        assert changed == n_tab
    finally:
        with torch.no_grad():      # the scene is the module's: put the parameters back
            for p, b in zip(scene["params"], before):
                p.copy_(b)
                p.grad = None
