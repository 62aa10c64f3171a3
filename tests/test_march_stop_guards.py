"""CPU-only: the refusals of render_rays / render with march_stop=, word for word, each raised before
anything could be launched (the tensors live on the CPU here)."""
import numpy as np
import pytest
import torch

from indoor_nerf_amd import sparse_field

BOX = (torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]))
NEEDS_MARCH = "{}: march_stop needs march= (rays are stopped inside a grid march; early_stop= is the dense path's)"
BAD_EPS = "{}: march_stop must be a float transmittance threshold in (0, 1), got {!r}"
BAD_SLAB = "{}: march_stop_slab must be a positive integer, got {!r}"
EPS_VALUES = (0.0, 1.0, -0.5, 2.0, float("nan"), 1, 0, True, "1e-3", np.float32(1.5))
SLAB_VALUES = (0, -3, 2.5, 64.0, True, "8", None)


def refusal(fn, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        fn(*args, **kwargs)
    return str(e.value)


def test_checker_word_for_word():
    grid = object()     # the checker only asks whether there is a march
    for prefix in ("render_rays", "render"):
        assert refusal(sparse_field.check_march_stop, 1e-3, 64, None, prefix) == NEEDS_MARCH.format(prefix)
        assert refusal(sparse_field.check_march_stop, 2.0, 0, None, prefix) == NEEDS_MARCH.format(prefix)   # comes first
        for bad in EPS_VALUES:
            assert refusal(sparse_field.check_march_stop, bad, 64, grid, prefix) == BAD_EPS.format(prefix, bad)
        for bad in SLAB_VALUES:
            assert refusal(sparse_field.check_march_stop, 1e-3, bad, grid, prefix) == BAD_SLAB.format(prefix, bad)
    assert sparse_field.check_march_stop(None, 0, None, "render_rays") is None      # without the keyword: nothing
    assert sparse_field.check_march_stop(1e-3, 64, grid, "render_rays") == (1e-3, 64)
    assert sparse_field.check_march_stop(np.float64(1e-300), np.int64(1), grid, "render") == (1e-300, 1)
    assert sparse_field.check_march_stop(1.0 - 1e-6, 4096, grid, "render") == (1.0 - 1e-6, 4096)


def test_render_rays_and_render_refuse_before_any_launch(nerf):
    grid = nerf.OccupancyGrid(BOX, resolution=2, device="cpu")
    rays = torch.zeros(4, 11)
    net = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                         input_ch=32, input_ch_views=16)
    emb = nerf.HashEmbedder(BOX, log2_hashmap_size=8, finest_resolution=32)
    o, d = torch.zeros(4, 3), torch.tensor([[0.0, 0.0, -1.0]]).repeat(4, 1)

    def rays_call(rays=rays, **over):
        return nerf.render_rays(rays, net, None, 8, **dict(dict(march=grid, march_stop=1e-3, embed_fn=emb), **over))

    def frame_call(**over):
        kw = dict(dict(march=grid, march_stop=1e-3, embed_fn=emb, network_fn=net, network_query_fn=None, N_samples=8,
                       use_viewdirs=True), **over)
        return nerf.render(2, 2, np.eye(3), rays=(o, d), ndc=False, **kw)

    for prefix, run in (("render_rays", rays_call), ("render", frame_call)):
        with torch.no_grad():
            assert refusal(run, march=None) == NEEDS_MARCH.format(prefix)
            assert refusal(run, march=None, early_stop=1e-3) == NEEDS_MARCH.format(prefix)
            for bad in EPS_VALUES:
                assert refusal(run, march_stop=bad) == BAD_EPS.format(prefix, bad)
            for bad in SLAB_VALUES:
                assert refusal(run, march_stop_slab=bad) == BAD_SLAB.format(prefix, bad)
            if prefix == "render":      # march's own refusals are render_rays', after render() has packed the rays
                continue
            # everything march already refuses, with its own words
            assert refusal(run, early_stop=1e-3) == (
                "render_rays: march does not combine with occupancy= (the march already masks by its grid) or "
                "early_stop= (rays are not stopped inside a march)")
            assert "march does not combine with occupancy=" in refusal(run, occupancy=grid)
            assert "march must be an OccupancyGrid" in refusal(run, march=0.5)
            assert "march_samples must be an integer in 1..4096" in refusal(run, march_samples=0)
            assert "march_points must be a positive integer" in refusal(run, march_points=0)
            assert "march needs raw_noise_std == 0" in refusal(run, raw_noise_std=1.0)
            assert "march needs perturb == 0" in refusal(run, perturb=1.0)
            assert "march needs lindisp=False" in refusal(run, lindisp=True)
            assert "march does not support predict_normals" in refusal(run, predict_normals=True)
    with torch.enable_grad():
        assert "march is forward-only" in refusal(rays_call)
    with torch.no_grad():
        assert "march needs ray rows with view directions" in refusal(rays_call, rays=torch.zeros(4, 8))
        assert "retraw is not available with march" in refusal(frame_call, retraw=True)
        # without march_stop the slab size is not looked at, as early_stop_slab without early_stop
        assert "march needs ray rows with view directions" in refusal(rays_call, rays=torch.zeros(4, 8), march_stop=None,
                                                                       march_stop_slab=0)
