"""render_rays(march=grid, march_sh="rays"), needs an MI355X: the march's list carries each point's ray
index instead of its SH4 row, one SH record per ray is formed once per chunk, and every MLP launch is the _rays entry of
the call's precision. None and "rows" are the call without the keyword.

The specification needs no tolerance: a record's pieces are what the MLP makes of the per-point row
(test_gpu_sh_rows.py, test_gpu_march_sh.py), so a render with the keyword must equal, in every entry and every bit,
the same render without it. The routing test is what keeps that equality from being met by a keyword that is ignored;
the preconditions (rays without a kept sample, rays with more than a tile of them, a ray's segment cut by a slice) are
what make it more than one ray per launch.

The scene of forward_only.py (build_scene) with the sigma row of both networks scaled by 500, as test_gpu_march.py
uses it.
"""
import numpy as np
import pytest
import torch

from forward_only import H, W, ball_mask
from test_gpu_march import march_rays
from test_gpu_render_fp16_tables import MASKS, PACKED, SIGMA_SCALE, assert_same, same_bits

pytestmark = pytest.mark.gpu

RAYS = dict(march_sh="rays")
PRECISIONS = {"fp32": {}, "bf16": dict(mlp_precision="bf16"),
              "bf16+features": dict(mlp_precision="bf16", feature_precision="bf16"),
              "fp16 tables": dict(table_precision="fp16"),
              "all": dict(mlp_precision="bf16", feature_precision="bf16", table_precision="fp16")}
MLP_ROWS = {"fp32": "nerf_mlp_fwd_ord", "bf16": "nerf_mlp_fwd_bf16", "bf16+features": "nerf_mlp_fwd_bf16_pkbf",
            "fp16 tables": "nerf_mlp_fwd_ord", "all": "nerf_mlp_fwd_bf16_pkbf"}
MLP_RAYS = {"fp32": "nerf_mlp_fwd_rays", "bf16": "nerf_mlp_fwd_bf16_rays", "bf16+features": "nerf_mlp_fwd_bf16_pkbf_rays",
            "fp16 tables": "nerf_mlp_fwd_rays", "all": "nerf_mlp_fwd_bf16_pkbf_rays"}
NEW = ("nerf_ray_sh_records", "nerf_rays_march_write", "nerf_rays_slab_march_write", "nerf_mlp_fwd_rays",
       "nerf_mlp_fwd_bf16_rays", "nerf_mlp_fwd_bf16_pkbf_rays")
STOP = dict(march_stop=1e-3, march_stop_slab=8)


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    from forward_only import build_scene
    return build_scene(nerf, gpu, SIGMA_SCALE)


def pair(scene, i, **over):
    """Frame i through render() with the keyword and without it (retraw is refused with march)."""
    return scene["frame"](i, retraw=False, **over, **RAYS), scene["frame"](i, retraw=False, **over)


# ---------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("which,K", [("ball16", 64), ("ball16", 200), ("random5", 64), ("random5", 200)])
def test_march_frames_and_packed_entries(nerf, gpu, scene, which, K):
    none, tile = 0, 0
    for i in (0, 1):
        grid = scene["grid_of"](MASKS[which]())
        got, ref = pair(scene, i, march=grid, march_samples=K)
        assert_same(got, ref, f"{which} K {K} pose {i}")
        counts = ref["march_samples"].reshape(-1)
        none, tile = none + int((counts == 0).sum()), tile + int((counts > 32).sum())
        got, ref = (march_rays(nerf, scene, i, grid, K, **kw) for kw in (RAYS, {}))
        assert ref["raw"].shape[0] > 0 and sorted(got) == sorted(ref)
        for k in PACKED + ("rays_d",):
            assert same_bits(got[k], ref[k]), f"{which} K {K} pose {i}: {k}"
    if (which, K) == ("ball16", 200):       # NumPy on the CPU gives 101 and 165
        assert none >= 50 and tile >= 50, f"fixture: {none} of {2 * H * W} rays keep nothing, {tile} more than 32"


@pytest.mark.parametrize("name", [k for k in PRECISIONS if k != "fp32"])
def test_precisions(nerf, gpu, scene, name):
    for i in (0, 1):
        grid = scene["grid_of"](ball_mask())
        got, ref = pair(scene, i, march=grid, march_samples=200, **PRECISIONS[name])
        assert_same(got, ref, f"{name} pose {i}")
        plain = scene["frame"](i, retraw=False, march=grid, march_samples=200)
        assert not same_bits(plain["rgb_map"], ref["rgb_map"]), f"{name}: the frame has the fp32 frame's bits"
        got, ref = (march_rays(nerf, scene, i, grid, 200, **PRECISIONS[name], **kw) for kw in (RAYS, {}))
        for k in PACKED:
            assert same_bits(got[k], ref[k]), f"{name} pose {i}: {k}"


@pytest.mark.parametrize("name", ["fp32", "all"])
def test_ray_bounds(nerf, gpu, scene, name):
    """After ray_bounds' compaction the index counts the rows of the compacted rays, the ones the write walks; with a
    grid every ray misses no chunk reaches render_rays."""
    ball, empty = scene["grid_of"](ball_mask()), scene["grid_of"](np.zeros((4, 4, 4), bool))
    for i in (0, 1):
        got, ref = pair(scene, i, ray_bounds=ball, march=ball, march_samples=64, **PRECISIONS[name])
        assert_same(got, ref, f"ray_bounds {name} pose {i}")
        hit = int(ref["ray_hit"].sum())
        assert 0 < hit < H * W, f"fixture: {hit} rays hit"
        got, ref = pair(scene, i, ray_bounds=empty, march=ball, march_samples=64, **STOP, **PRECISIONS[name])
        assert_same(got, ref, f"ray_bounds, every ray missed, {name} pose {i}")
        assert not bool(ref["ray_hit"].any()) and "march_stop_samples" in ref


@pytest.mark.parametrize("eps", [1e-3, 0.9])
@pytest.mark.parametrize("name", ["fp32", "bf16+features"])
def test_march_stop_slabs(nerf, gpu, scene, name, eps):
    """Slabs of 8: at 1e-3 no ray of this scene stops (eight slabs, every ray alive throughout); at 0.9, the
    threshold of test_gpu_march_stop.py's frames, some do, and later slabs walk fewer rays."""
    stop = dict(march_stop=eps, march_stop_slab=8)
    for i in (0, 1):
        grid = scene["grid_of"](ball_mask())
        got, ref = pair(scene, i, march=grid, march_samples=64, **stop, **PRECISIONS[name])
        assert_same(got, ref, f"march_stop {eps} {name} pose {i}")
        if eps == 0.9:
            assert bool((ref["march_stop_samples"] < 64).any()), "fixture: no ray stops"
        got, ref = (march_rays(nerf, scene, i, grid, 64, **stop, **PRECISIONS[name], **kw) for kw in (RAYS, {}))
        assert len(got["march_slabs"]) == len(ref["march_slabs"]) == 8
        assert sum(s[1].shape[0] for s in ref["march_slabs"]) > 0
        for n, (a, b) in enumerate(zip(got["march_slabs"], ref["march_slabs"])):
            for x, y, k in zip(a, b, ("offsets", "raw", "pts", "z_vals")):
                assert same_bits(x, y), f"{eps} {name} pose {i} slab {n}: {k}"
        for k in ("rgb_map", "depth_map", "acc_map", "march_samples", "march_stop_samples", "rays_d"):
            assert same_bits(got[k], ref[k]), f"{eps} {name} pose {i}: {k}"


def test_chunks_and_slices(nerf, gpu, scene):
    """Chunks of 37 rays (the index restarts in every chunk) and of 4096; slices of 1,000 points, which cut rays'
    segments (NumPy on the CPU: 8 of them through ball16 at K = 200), against one slice."""
    grid = scene["grid_of"](ball_mask())
    for i in (0, 1):
        ref = scene["frame"](i, retraw=False, march=grid, march_samples=200)
        for chunk in (37, 4096):
            got = scene["frame"](i, chunk=chunk, retraw=False, march=grid, march_samples=200, **RAYS)
            assert_same(got, ref, f"chunk {chunk} pose {i}")
        whole = march_rays(nerf, scene, i, grid, 200)
        off = whole["march_offsets"].cpu().numpy().astype(np.int64)
        cuts = [b for b in range(1000, off[-1], 1000) if off[np.searchsorted(off, b, side="right") - 1] < b]
        assert cuts, "fixture: no segment is cut by a slice of 1,000 points"
        got = march_rays(nerf, scene, i, grid, 200, march_points=1000, **RAYS)
        for k in PACKED:
            assert same_bits(got[k], whole[k]), f"march_points 1000 pose {i}: {k}"
        for over in (dict(march_points=1000), RAYS):
            assert_same(scene["frame"](i, retraw=False, march=grid, march_samples=200, **over), ref, f"{over} pose {i}")


# ---------------------------------------------------------------- 2. routing
def calls(scene, monkeypatch, i, **over):
    """(frame i, the names of every launch, the shapes of the float32 tensors torch.empty made meanwhile)."""
    import indoor_nerf_amd._lib as L
    names, call, made, empty = [], L.call, [], torch.empty

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    def empty_recording(*size, **kw):
        made.append((tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size), kw.get("dtype")))
        return empty(*size, **kw)
    with monkeypatch.context() as m:
        m.setattr(L, "call", recording)
        m.setattr(torch, "empty", empty_recording)
        out = scene["frame"](i, retraw=False, **over)
    return out, names, made


@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("name", list(PRECISIONS))
def test_routing(nerf, gpu, scene, name, stop, monkeypatch):
    grid = scene["grid_of"](ball_mask())
    over = dict(march=grid, march_samples=64, chunk=96, **(STOP if stop else {}), **PRECISIONS[name])
    write = "nerf_slab_march_write" if stop else "nerf_march_write"
    base, names, made = calls(scene, monkeypatch, 0, **over)
    mlp = [n for n in names if n.startswith("nerf_mlp_fwd")]
    writes = [n for n in names if "march_write" in n]
    assert mlp and mlp == [MLP_ROWS[name]] * len(mlp) and writes == [write] * len(writes), f"{name}: {mlp} {writes}"
    assert not any(n in NEW for n in names)
    assert any(len(s) == 2 and s[1] == 16 and dt == torch.float32 for s, dt in made), "fixture: no SH rows seen"
    for value in (None, "rows"):
        same, names2, made2 = calls(scene, monkeypatch, 0, march_sh=value, **over)
        assert names2 == names and made2 == made, f"{name} march_sh={value!r}: other launches or buffers"
        assert_same(same, base, f"{name} march_sh={value!r}")
    got, names3, made3 = calls(scene, monkeypatch, 0, **over, **RAYS)
    assert_same(got, base, f"{name} march_sh='rays'")
    mlp3 = [n for n in names3 if n.startswith("nerf_mlp_fwd")]
    writes3 = [n for n in names3 if "march_write" in n]
    assert mlp3 == [MLP_RAYS[name]] * len(mlp), f"{name}: {mlp3}"
    assert writes3 == [write.replace("nerf_", "nerf_rays_")] * len(writes), f"{name}: {writes3}"
    # one records launch per chunk that evaluates a point, also over the slabs of march_stop
    chunks = [base["march_samples"].reshape(-1)[c:c + 96] for c in range(0, H * W, 96)]
    busy = sum(int(c.sum()) > 0 for c in chunks)
    assert len(chunks) == 2 and busy >= 1 and names3.count("nerf_ray_sh_records") == busy, f"{name}: {names3}"
    assert not any(len(s) == 2 and s[1] == 16 and dt == torch.float32 for s, dt in made3), "a per-point SH buffer"
    # everything else is launched as before
    strip = lambda ns: [n for n in ns if n not in NEW and not n.startswith("nerf_mlp_fwd") and "march_write" not in n]  # noqa: E731
    assert strip(names3) == strip(names)


# ---------------------------------------------------------------- 3. refusals
def test_refusals(nerf, gpu, scene):
    grid = scene["grid_of"](ball_mask())
    rays, kw, K = scene["packed"](0), scene["ray_kw"](), scene["K"]
    pose = scene["poses"][0][:3, :4].to(gpu)
    with torch.no_grad():
        for bad in ("ray", "RAYS", 1, True):
            msg = f"march_sh must be None, 'rows' or 'rays', got {bad!r}"
            with pytest.raises(ValueError) as e:
                nerf.render_rays(rays, march=grid, march_sh=bad, **kw)
            assert str(e.value) == "render_rays: " + msg
            with pytest.raises(ValueError) as e:
                nerf.render(H, W, K, c2w=pose, march=grid, march_sh=bad, **scene["kw"])
            assert str(e.value) == "render: " + msg
        needs = "march_sh='rays' needs march= (the ray index belongs to a grid march's list)"
        with pytest.raises(ValueError) as e:
            nerf.render_rays(rays, **RAYS, **kw)
        assert str(e.value) == "render_rays: " + needs
        for extra in ({}, dict(ray_bounds=scene["grid_of"](np.zeros((4, 4, 4), bool)))):     # no chunk reaches render_rays
            with pytest.raises(ValueError) as e:
                nerf.render(H, W, K, c2w=pose, **RAYS, **extra, **scene["kw"])
            assert str(e.value) == "render: " + needs
        foreign = lambda pts, viewdirs, fn: torch.zeros(pts.shape[0], 4, device=gpu)  # noqa: E731
        with pytest.raises(ValueError) as e:
            nerf.render_rays(rays, march=grid, march_samples=64, **RAYS, **dict(kw, network_query_fn=foreign))
        assert str(e.value) == "render_rays: march needs a network_query_fn that calls this package's run_network"
    why = "march_sh is forward-only (call under torch.no_grad(); the backward reads per-point SH rows)"
    with torch.enable_grad():
        with pytest.raises(ValueError) as e:
            nerf.render_rays(rays, march=grid, **RAYS, **kw)
        assert str(e.value) == "render_rays: " + why
        with pytest.raises(ValueError) as e:
            nerf.render(H, W, K, c2w=pose, march=grid, **RAYS, **scene["kw"])
        assert str(e.value) == "render: " + why
