"""render_rays(march=grid, march_sizes="device"), needs an MI355X: the length of every packed list of
the march stays in device memory; the lists are allocated at their capacity, the encoder and the MLP read the count
themselves (the _dev entries), and every slab of a chunk is written, evaluated, composited and advanced back to back,
with no host read. None and "host" are the call without the keyword.

The specification needs no tolerance: every kept point goes through the same arithmetic and a ray's entries are
composited in the same order, so a render with the keyword must equal, in every entry and every bit (the NaN pattern
of depth_map included), the same render without it. The routing test is what keeps that equality from being met by a
keyword that is ignored, and the host-read test is what the keyword is for.

The scene of forward_only.py (build_scene) with the sigma row of both networks scaled by 500, as test_gpu_march.py
uses it. "device" needs march_sh="rays", mlp_precision="bf16" and feature_precision="bf16" in the same call: FAST.
"""
import numpy as np
import pytest
import torch

from forward_only import H, W, ball_mask
from test_gpu_march import march_rays
from test_gpu_render_fp16_tables import MASKS, PACKED, SIGMA_SCALE, assert_same, same_bits
from test_gpu_render_march_sh import calls

pytestmark = pytest.mark.gpu

FAST = dict(march_sh="rays", mlp_precision="bf16", feature_precision="bf16")
DEVICE = dict(march_sizes="device")
TABLES = {"fp32 tables": {}, "fp16 tables": dict(table_precision="fp16")}
ENTRIES = ("rgb_map", "depth_map", "acc_map", "march_samples", "rays_d")
DEV_ENTRIES = ("nerf_hash_encode_fwd_pkbf_dev", "nerf_hash_encode_fwd_half_pkbf_dev", "nerf_mlp_fwd_bf16_pkbf_rays_dev")


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    from forward_only import build_scene
    return build_scene(nerf, gpu, SIGMA_SCALE)


def pair(scene, i, **over):
    """Frame i through render() with the keyword and without it (retraw is refused with march)."""
    return (scene["frame"](i, retraw=False, **FAST, **over, **DEVICE), scene["frame"](i, retraw=False, **FAST, **over))


def rays_pair(nerf, scene, i, grid, K, **over):
    """Frame i's rays through render_rays with retraw, with the keyword and without it."""
    return tuple(march_rays(nerf, scene, i, grid, K, **FAST, **over, **kw) for kw in (DEVICE, {}))


def assert_slabs(got, ref, what):
    assert len(got["march_slabs"]) == len(ref["march_slabs"])
    for n, (a, b) in enumerate(zip(got["march_slabs"], ref["march_slabs"])):
        assert len(a) == len(b) == 4
        for x, y, k in zip(a, b, ("offsets", "raw", "pts", "z_vals")):
            assert same_bits(x, y), f"{what} slab {n}: {k}"
    for k in ENTRIES + ("march_stop_samples",):
        assert same_bits(got[k], ref[k]), f"{what}: {k}"


# ---------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("which,K", [("ball16", 64), ("ball16", 200), ("random5", 64), ("random5", 200)])
def test_march_frames_and_packed_entries(nerf, gpu, scene, which, K, tables):
    none, nan = 0, 0
    for i in (0, 1):
        grid = scene["grid_of"](MASKS[which]())
        got, ref = pair(scene, i, march=grid, march_samples=K, **TABLES[tables])
        assert_same(got, ref, f"{which} K {K} {tables} pose {i}")
        none += int((ref["march_samples"] == 0).sum())
        nan += int(torch.isnan(ref["depth_map"]).sum())
        got, ref = rays_pair(nerf, scene, i, grid, K, **TABLES[tables])
        assert ref["raw"].shape[0] > 0 and sorted(got) == sorted(ref)
        for k in PACKED + ("rays_d",):
            assert same_bits(got[k], ref[k]), f"{which} K {K} {tables} pose {i}: {k}"
        assert grid.last_counts() == (ref["raw"].shape[0], H * W * K)
    if which == "ball16":
        assert none >= 50 and nan >= 50, f"fixture: {none} rays keep nothing, {nan} depths are NaN"


@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("slab", [8, 64])
@pytest.mark.parametrize("eps", [1e-3, 0.9])
def test_march_stop_slabs(nerf, gpu, scene, eps, slab, tables):
    """Slabs of 8 and 64 lattice samples at K = 200 through the ball: the ball lies in the middle of [near, far], so
    the leading and the trailing slabs of 8 have empty lists, which the host-sized loop skips and this one launches.
    At 0.9 rays stop and later slabs walk fewer rays."""
    stop = dict(march_stop=eps, march_stop_slab=slab)
    empty_slabs = 0
    for i in (0, 1):
        grid = scene["grid_of"](ball_mask())
        got, ref = pair(scene, i, march=grid, march_samples=200, **stop, **TABLES[tables])
        assert_same(got, ref, f"march_stop {eps} slab {slab} {tables} pose {i}")
        if eps == 0.9:
            assert bool((ref["march_stop_samples"] < 200).any()), "fixture: no ray stops"
        got, ref = rays_pair(nerf, scene, i, grid, 200, **stop, **TABLES[tables])
        assert len(ref["march_slabs"]) == -(-200 // slab) and sum(s[1].shape[0] for s in ref["march_slabs"]) > 0
        assert_slabs(got, ref, f"march_stop {eps} slab {slab} {tables} pose {i}")
        empty_slabs += sum(s[1].shape[0] == 0 for s in ref["march_slabs"])
        assert grid.last_counts() == (sum(s[1].shape[0] for s in ref["march_slabs"]), H * W * 200)
    if slab == 8:
        assert empty_slabs >= 1, "fixture: no slab with an empty list"


def test_one_slab_and_a_last_partial_slab(nerf, gpu, scene):
    """march_stop_slab >= K is one slab (no state is carried); K = 200 in slabs of 64 ends in a slab of 8."""
    grid = scene["grid_of"](ball_mask())
    for slab in (200, 4096):
        got, ref = rays_pair(nerf, scene, 0, grid, 200, march_stop=1e-2, march_stop_slab=slab)
        assert len(ref["march_slabs"]) == 1
        assert_slabs(got, ref, f"one slab of {slab}")


@pytest.mark.parametrize("stop", [False, True])
def test_ray_bounds(nerf, gpu, scene, stop):
    """After ray_bounds' compaction the chunks are the hit rays; with a grid every ray misses no chunk reaches
    render_rays."""
    ball, empty = scene["grid_of"](ball_mask()), scene["grid_of"](np.zeros((4, 4, 4), bool))
    over = dict(march_stop=0.9, march_stop_slab=8) if stop else {}
    for i in (0, 1):
        got, ref = pair(scene, i, ray_bounds=ball, march=ball, march_samples=64, **over)
        assert_same(got, ref, f"ray_bounds stop {stop} pose {i}")
        assert 0 < int(ref["ray_hit"].sum()) < H * W
        got, ref = pair(scene, i, ray_bounds=empty, march=ball, march_samples=64, **over)
        assert_same(got, ref, f"ray_bounds, every ray missed, stop {stop} pose {i}")
        assert not bool(ref["ray_hit"].any())


@pytest.mark.parametrize("stop", [False, True])
def test_chunks_and_slices(nerf, gpu, scene, stop):
    """Chunks of 37 rays and of 4096. Slices of 1,000 points: the capacity of a chunk of 192 rays at K = 200 is 38,400
    entries, 39 slices, of which those beyond the list's length are empty launches."""
    grid = scene["grid_of"](ball_mask())
    over = dict(march_stop=0.9, march_stop_slab=64) if stop else {}
    for i in (0, 1):
        ref = scene["frame"](i, retraw=False, march=grid, march_samples=200, **FAST, **over)
        for chunk in (37, 4096):
            got = scene["frame"](i, chunk=chunk, retraw=False, march=grid, march_samples=200, **FAST, **over, **DEVICE)
            assert_same(got, ref, f"chunk {chunk} stop {stop} pose {i}")
        got = scene["frame"](i, retraw=False, march=grid, march_samples=200, march_points=1000, **FAST, **over, **DEVICE)
        assert_same(got, ref, f"march_points 1000 stop {stop} pose {i}")
        got, whole = rays_pair(nerf, scene, i, grid, 200, march_points=1000, **over)
        n = sum(s[1].shape[0] for s in whole["march_slabs"]) if stop else whole["raw"].shape[0]
        assert 1000 < n < H * W * 200 - 1000, "fixture: no full slice, or no empty one"
        if stop:
            assert_slabs(got, whole, f"march_points 1000 pose {i}")
        else:
            for k in PACKED:
                assert same_bits(got[k], whole[k]), f"march_points 1000 pose {i}: {k}"


@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("fill", [False, True])
def test_empty_and_full_grid(nerf, gpu, scene, fill, stop):
    """An empty grid: every list is empty, every launch is an empty one, every depth is NaN. A full grid: every
    lattice sample inside the box is kept."""
    over = dict(march_stop=0.9, march_stop_slab=8) if stop else {}
    for i in (0, 1):
        grid = scene["grid_of"](np.full((4, 4, 4), fill))
        got, ref = pair(scene, i, march=grid, march_samples=64, **over)
        assert_same(got, ref, f"grid all {fill} stop {stop} pose {i}")
        got, ref = rays_pair(nerf, scene, i, grid, 64, **over)
        if stop:
            assert_slabs(got, ref, f"grid all {fill} pose {i}")
            n = sum(s[1].shape[0] for s in ref["march_slabs"])
        else:
            for k in PACKED + ("rays_d",):
                assert same_bits(got[k], ref[k]), f"grid all {fill} pose {i}: {k}"
            n = ref["raw"].shape[0]
        # full: about half of the lattice lies inside the box; with march_stop the rays stop inside it
        assert (n > (0 if stop else H * W * 64 // 4)) if fill else (n == 0 and bool(torch.isnan(ref["depth_map"]).all()))
        assert grid.last_counts() == (n, H * W * 64)


def test_count_equals_capacity(nerf, gpu, scene):
    """Rays that lie inside the box over all of [near, far] through a full grid: every lattice sample is kept, so the
    device count equals the capacity (the upper end of the kernels' clamp in a render)."""
    lo, hi = scene["lo"], scene["hi"]
    grid = scene["grid_of"](np.ones((4, 4, 4), bool))
    g = torch.Generator().manual_seed(7)
    R, K = 70, 64
    o = torch.from_numpy(0.5 * (lo + hi)).float() + 0.05 * (torch.rand(R, 3, generator=g) - 0.5)
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    reach = 0.3 * float((hi - lo).min())
    rays = torch.cat([o, d, torch.zeros(R, 1), torch.full((R, 1), reach), d], 1).to(gpu).contiguous()
    kw = scene["ray_kw"](**FAST)
    with torch.no_grad():
        for over in ({}, dict(march_stop=0.9, march_stop_slab=8)):
            got, ref = (nerf.render_rays(rays, march=grid, march_samples=K, retraw=True, **kw, **over, **m)
                        for m in (DEVICE, {}))
            assert bool((ref["march_samples"] + (K - ref["march_stop_samples"] if over else 0) == K).all())
            if over:
                assert_slabs(got, ref, "count = capacity")
                assert ref["march_slabs"][0][1].shape[0] == R * 8
            else:
                assert ref["raw"].shape[0] == R * K
                for k in PACKED + ("rays_d",):
                    assert same_bits(got[k], ref[k]), f"count = capacity: {k}"


def test_no_rays(nerf, gpu, scene):
    grid = scene["grid_of"](ball_mask())
    rays = scene["packed"](0)[:0].contiguous()
    with torch.no_grad():
        for over in ({}, dict(march_stop=0.9, march_stop_slab=8)):
            got, ref = (nerf.render_rays(rays, march=grid, march_samples=64, **scene["ray_kw"](**FAST), **over, **m)
                        for m in (DEVICE, {}))
            assert sorted(got) == sorted(ref)
            for k in ref:
                assert same_bits(got[k], ref[k]), k


# ---------------------------------------------------------------- 2. routing
@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("stop", [False, True])
def test_routing(nerf, gpu, scene, stop, tables, monkeypatch):
    grid = scene["grid_of"](ball_mask())
    over = dict(march=grid, march_samples=64, chunk=96, **(dict(march_stop=1e-3, march_stop_slab=8) if stop else {}),
                **FAST, **TABLES[tables])
    base, names, made = calls(scene, monkeypatch, 0, **over)
    field = [n for n in names if "hash_encode" in n or n.startswith("nerf_mlp_fwd")]
    assert field and not any(n in DEV_ENTRIES for n in names)
    for value in (None, "host"):
        same, names2, made2 = calls(scene, monkeypatch, 0, march_sizes=value, **over)
        assert names2 == names and made2 == made, f"march_sizes={value!r}: other launches or buffers"
        assert_same(same, base, f"march_sizes={value!r}")
    got, names3, _ = calls(scene, monkeypatch, 0, **over, **DEVICE)
    assert_same(got, base, "march_sizes='device'")
    field3 = [n for n in names3 if "hash_encode" in n or n.startswith("nerf_mlp_fwd")]
    hash_dev = DEV_ENTRIES[1] if tables == "fp16 tables" else DEV_ENTRIES[0]
    assert field3 and all(n in (hash_dev, DEV_ENTRIES[2]) for n in field3), field3
    assert field3.count(hash_dev) == field3.count(DEV_ENTRIES[2])
    if stop:        # two chunks of eight slabs: every slab is evaluated, composited, and all but the last advanced
        assert field3.count(hash_dev) == 16 and len(field) < 2 * 16
        assert names3.count("nerf_slab_march_composite") == 16 and names3.count("nerf_slab_march_advance") == 14
    else:
        assert field3.count(hash_dev) == 2 and names3.count("nerf_march_composite") == 2


# ---------------------------------------------------------------- 3. no host read
def host_reads(monkeypatch, run):
    seen = []
    with monkeypatch.context() as m:
        for name in ("item", "cpu", "tolist", "numpy"):
            real = getattr(torch.Tensor, name)

            def counting(self, *a, _real=real, _name=name, **kw):
                seen.append(_name)
                return _real(self, *a, **kw)
            m.setattr(torch.Tensor, name, counting)
        out = run()
    return out, seen


@pytest.mark.parametrize("stop", [False, True])
def test_no_host_read(nerf, gpu, scene, stop, monkeypatch):
    grid = scene["grid_of"](ball_mask())
    rays = scene["packed"](0)
    kw = scene["ray_kw"](**FAST, **(dict(march_stop=0.9, march_stop_slab=8) if stop else {}))
    with torch.no_grad():
        nerf.render_rays(rays, march=grid, march_samples=64, **kw, **DEVICE)      # the fp16 image, the t table: made once
        got, seen = host_reads(monkeypatch, lambda: nerf.render_rays(rays, march=grid, march_samples=64, **kw, **DEVICE))
        assert seen == [], f"host reads with march_sizes='device': {seen}"
        ref, seen = host_reads(monkeypatch, lambda: nerf.render_rays(rays, march=grid, march_samples=64, **kw))
        assert len(seen) >= (8 if stop else 1), f"fixture: the host-sized call read {seen}"
    for k in ref:
        assert same_bits(got[k], ref[k]), k
    n = int(ref["march_samples"].sum())
    assert grid.last_counts() == (n, H * W * 64)
    with torch.no_grad():
        nerf.render_rays(rays, march=grid, march_samples=64, **kw, **DEVICE)
        (evaluated, total), seen = host_reads(monkeypatch, grid.last_counts)
    assert (evaluated, total) == (n, H * W * 64) and len(seen) == 1, f"last_counts read {seen}"
    assert host_reads(monkeypatch, grid.last_counts) == ((n, H * W * 64), [])       # resolved once


# ---------------------------------------------------------------- 4. refusals on the device
def test_refusals(nerf, gpu, scene):
    grid = scene["grid_of"](ball_mask())
    rays, kw, K = scene["packed"](0), scene["ray_kw"](), scene["K"]
    pose = scene["poses"][0][:3, :4].to(gpu)
    needs = {"march_sh": "march_sizes='device' needs march_sh='rays' (the device-sized MLP reads SH through the ray "
                         "index)",
             "mlp_precision": "march_sizes='device' needs mlp_precision='bf16' (the device-sized MLP is the bf16 "
                              "forward)",
             "feature_precision": "march_sizes='device' needs feature_precision='bf16' (the device-sized encoder writes "
                                  "packed bf16 features)"}
    with torch.no_grad():
        for missing, msg in needs.items():
            rest = {k: v for k, v in FAST.items() if k != missing}
            if missing == "mlp_precision":
                rest.pop("feature_precision")
            with pytest.raises(ValueError) as e:
                nerf.render_rays(rays, march=grid, **rest, **DEVICE, **kw)
            assert str(e.value) == "render_rays: " + msg
            with pytest.raises(ValueError) as e:
                nerf.render(H, W, K, c2w=pose, march=grid, **rest, **DEVICE, **scene["kw"])
            assert str(e.value) == "render: " + msg
        with pytest.raises(ValueError) as e:
            nerf.render_rays(rays, march=grid, march_sizes="gpu", **FAST, **kw)
        assert str(e.value) == "render_rays: march_sizes must be None, 'host' or 'device', got 'gpu'"
        with pytest.raises(ValueError) as e:
            nerf.render_rays(rays, **DEVICE, **kw)
        assert str(e.value) == ("render_rays: march_sizes='device' needs march= (the sizes are those of a grid march's "
                                "lists)")
    with torch.enable_grad():       # the companions are forward-only themselves and are checked first
        with pytest.raises(ValueError) as e:
            nerf.render_rays(rays, march=grid, **FAST, **DEVICE, **kw)
        assert str(e.value).startswith("render_rays: march_sh is forward-only")
