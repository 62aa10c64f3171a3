"""The launches of the forward-only render paths, entry by entry, needs an MI355X.

One request object carries every forward-only keyword from render_rays to the fused run_network. Whatever carries
them, a render() call must make the launches it made before: the sequence of entry names of one frame per
configuration (_lib.set_timing) is compared with tests/golden/field_request_launches.json, recorded with this
module's own configurations and scene at the commit before the request was introduced. The pixel values of every
keyword are pinned bit for bit by the test_gpu_render_* modules; this one pins which entries run, and in which order.

The scene of forward_only.py (build_scene), frame 0: 12 x 16 = 192 rays, 32 + 32 samples, chunk 4096 unless said.
"""
import json
import os

import pytest
import torch

from forward_only import H, W, ball_mask, build_scene

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_request_launches.json")
PRECISIONS = dict(mlp_precision="bf16", table_precision="fp16", feature_precision="bf16")


def configurations(grid):
    """name -> render() keywords on top of the scene's; `grid`: the ball mask at resolution 16."""
    early = dict(early_stop=1e-3, early_stop_slab=8)
    by_ray = dict(march=grid, march_samples=16, march_sh="rays", march_points=64, **PRECISIONS)
    return {
        "01 plain": {},
        "02 occupancy": dict(occupancy=grid),
        "03 early_stop": early,
        "04 occupancy + early_stop + ray_bounds": dict(occupancy=grid, ray_bounds=grid, **early),
        "05 bf16 MLP": dict(mlp_precision="bf16"),
        "06 fp16 tables": dict(table_precision="fp16"),
        "07 all precisions, dense": dict(PRECISIONS),
        "08 occupancy + all precisions": dict(occupancy=grid, **PRECISIONS),
        "09 march": dict(march=grid, march_samples=16),
        "10 march + march_stop": dict(march=grid, march_samples=16, march_stop=1e-2, march_stop_slab=8),
        "11 march by ray + all precisions, slices of 64": by_ray,
        "12 as 11 + march_stop + ray_bounds, chunks of 64": dict(by_ray, march_stop=1e-2, march_stop_slab=8,
                                                                 ray_bounds=grid, chunk=64),
    }


def render_frame(nerf, scene, over):
    """Frame 0 through render() (not build_scene's frame: a cached frame launches nothing) -> [rgb, depth, acc, extras]."""
    over = dict(over)
    chunk = over.pop("chunk", 4096)
    with torch.no_grad():
        return nerf.render(H, W, scene["K"], chunk=chunk, c2w=scene["poses"][0][:3, :4].to(scene["gpu"]),
                           **dict(scene["kw"], **over))


def launches(nerf, scene, over):
    """The entry names of one frame's launches, in order."""
    from indoor_nerf_amd import _lib
    _lib.set_timing(True)
    try:
        render_frame(nerf, scene, over)
        torch.cuda.synchronize()
        return [name for name, _, _ in _lib.timing_records()]
    finally:
        _lib.set_timing(False)


def make_scene(nerf, gpu):
    scene = dict(build_scene(nerf, gpu), gpu=gpu)
    return scene, configurations(scene["grid_of"](ball_mask(16)))


def test_same_launches_in_the_same_order(nerf, gpu):
    scene, configs = make_scene(nerf, gpu)
    with open(GOLDEN) as fp:
        golden = json.load(fp)
    assert sorted(golden) == sorted(configs)
    got = {name: launches(nerf, scene, over) for name, over in configs.items()}
    for name in configs:
        assert got[name] == golden[name], f"{name}: launches differ from the recorded ones"
    # several slices per list, several chunks: the configurations reach what they are there for
    assert got["11 march by ray + all precisions, slices of 64"].count("nerf_mlp_fwd_bf16_pkbf_rays") > 1
    assert got["12 as 11 + march_stop + ray_bounds, chunks of 64"].count("nerf_ray_sh_records") > 1
    # no request state survives a call
    assert launches(nerf, scene, {}) == golden["01 plain"]
