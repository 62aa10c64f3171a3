"""render_rays(mlp_precision="bf16"), needs an MI355X: every MLP forward launch of a forward-only
render goes to nerf_mlp_fwd_bf16, on the dense path and on every path that skips samples; None and "fp32" are the
call without the keyword, bit for bit.

The scene of forward_only.py (build_scene) with the sigma row of both networks scaled by 500, as test_gpu_march.py
uses it, so that rays through occupied cells become opaque.

What is exact: a point's bf16 result does not depend on the points that share its tile or launch
(test_gpu_mlp_bf16.py), so §13's and §16's arguments hold unchanged under bf16: the kept raw rows of occupancy= are
the dense bf16 rows bit for bit and the skipped ones zero, the march's packed raw rows are the rows of the masked
dense bf16 render bit for bit, and its maps are within §16's tolerances of that render.

What is not: the bf16 frame against the fp32 frame. That difference is the format's, and it is measured against a
frame whose field is a torch emulation of the kernel's roundings with fp64 sums (test_gpu_mlp_bf16.emulate64) on the
package's own hash features and SH: the kernel's frame must be closer to the emulated frame than the emulated frame is
to the fp32 frame.
"""
import numpy as np
import pytest
import torch

from forward_only import H, W, ball_mask, bits_equal, build_scene, random_mask
from test_gpu_march import assert_maps_close, maps_of, march_rays
from test_gpu_mlp_bf16 import emulate64

pytestmark = pytest.mark.gpu

SIGMA_SCALE = 500.0
BF16, X6 = "nerf_mlp_fwd_bf16", "nerf_mlp_fwd"
MASKS = {"ball16": ball_mask, "random5": lambda: random_mask(5)}


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    return build_scene(nerf, gpu, SIGMA_SCALE)


def mlp_calls(scene, i, **over):
    """(frame i, the names of its MLP forward launches). The query function is named, so that build_scene's frame
    cache is not used: a cached frame launches nothing."""
    import indoor_nerf_amd._lib as L
    over.setdefault("network_query_fn", scene["kw"]["network_query_fn"])
    L.set_timing(True)
    try:
        out = scene["frame"](i, **over)
        torch.cuda.synchronize()
        names = [n for n, _, _ in L.timing_records() if n.startswith(X6)]
    finally:
        L.set_timing(False)
    return out, names


def same_bits(a, b):
    return torch.equal(a, b) if a.dtype == torch.bool else bits_equal(a, b)


def variants(scene):
    grid = scene["grid_of"](ball_mask())
    return {"dense": {}, "coarse_only": dict(N_importance=0), "occupancy": dict(occupancy=grid),
            "early_stop": dict(early_stop=1e-3, early_stop_slab=8),
            "occupancy+early_stop": dict(occupancy=grid, early_stop=1e-3),
            "ray_bounds": dict(ray_bounds=grid), "ray_bounds+occupancy": dict(ray_bounds=grid, occupancy=grid),
            "march": dict(march=grid, march_samples=64, retraw=False),
            "march+ray_bounds": dict(march=grid, march_samples=64, ray_bounds=grid, retraw=False)}


# ---------------------------------------------------------------- 1. routing
VARIANTS = ["dense", "coarse_only", "occupancy", "early_stop", "occupancy+early_stop", "ray_bounds",
            "ray_bounds+occupancy", "march", "march+ray_bounds"]


@pytest.mark.parametrize("name", VARIANTS)
def test_routing(nerf, gpu, scene, name):
    over = variants(scene)[name]
    base, names = mlp_calls(scene, 0, **over)
    assert names and BF16 not in names, f"{name}: {names}"
    n_launches = len(names)
    for value in (None, "fp32"):
        same, names = mlp_calls(scene, 0, mlp_precision=value, **over)
        assert BF16 not in names and len(names) == n_launches, f"{name} mlp_precision={value!r}: {names}"
        assert sorted(same) == sorted(base)
        for k in base:
            assert same_bits(same[k], base[k]), f"{name} mlp_precision={value!r}: {k} changed"
    got, names = mlp_calls(scene, 0, mlp_precision="bf16", **over)
    assert names == [BF16] * n_launches, f"{name} bf16: {names}"
    assert sorted(got) == sorted(base)
    for k in base:
        assert got[k].shape == base[k].shape and got[k].dtype == base[k].dtype, k
    assert not bits_equal(got["rgb_map"], base["rgb_map"]), f"{name}: the bf16 frame has the fp32 frame's bits"


def test_routing_of_the_fine_pass_without_coarse_reuse(nerf, gpu, scene):
    """The dense fine pass in both forms: in the importance-first order of the coarse-feature reuse (a point order,
    two segments) and re-encoding every point. The two give the same bits, under bf16 as under fp32."""
    import importlib
    R = importlib.import_module("indoor_nerf_amd.render")     # the package re-exports render() under that name
    with_reuse, names = mlp_calls(scene, 1, mlp_precision="bf16")
    assert names == [BF16, BF16] and R.last_reuse_used()
    R.set_coarse_reuse(False)
    try:
        without, names = mlp_calls(scene, 1, mlp_precision="bf16")
        assert names == [BF16, BF16] and not R.last_reuse_used()
    finally:
        R.set_coarse_reuse(True)
    for k in with_reuse:
        assert same_bits(with_reuse[k], without[k]), k


# ---------------------------------------------------------------- 2. the skipping paths stay exact
@pytest.mark.parametrize("which", ["ball16", "random5"])
def test_occupancy_rows_are_the_dense_bf16_rows(nerf, gpu, scene, which):
    grid = scene["grid_of"](MASKS[which]())
    for i in (0, 1):
        dense = scene["frame"](i, chunk=4096, N_importance=0, mlp_precision="bf16")
        fp32 = scene["frame"](i, chunk=4096, N_importance=0)
        assert not bits_equal(dense["raw"], fp32["raw"])
        q = grid.query(dense["pts"])
        assert 0.0 < float(q.float().mean()) < 1.0
        for chunk in (4096, 37):
            got = scene["frame"](i, chunk=chunk, N_importance=0, occupancy=grid, mlp_precision="bf16")
            assert bits_equal(got["pts"], dense["pts"])
            assert bits_equal(got["raw"][q], dense["raw"][q]), f"{which} pose {i}: kept rows differ from the dense rows"
            assert bool((got["raw"][~q].view(torch.int32) == 0).all()), f"{which} pose {i}: skipped rows are not zero"


@pytest.mark.parametrize("which", ["ball16", "random5"])
def test_march_is_the_masked_dense_bf16_render(nerf, gpu, scene, which):
    grid, fine = scene["grid_of"](MASKS[which]()), scene["kw"]["network_fine"]
    opaque = 0
    for K in (64, 200):
        for i in (0, 1):
            ref = scene["frame"](i, retraw=True, N_samples=K, N_importance=0, occupancy=grid, network_fn=fine,
                                 mlp_precision="bf16")
            raw, q = ref["raw"].reshape(H * W, K, 4), grid.query(ref["pts"].reshape(H * W, K, 3))
            opaque += int((ref["acc_map"] > 0.3).sum())
            got = march_rays(nerf, scene, i, grid, K, mlp_precision="bf16")
            what = f"{which} pose {i} K {K}"
            assert bits_equal(got["raw"], raw[q]), f"{what}: packed raw"
            assert_maps_close(maps_of(got), maps_of(ref), what)
            fp32 = march_rays(nerf, scene, i, grid, K)
            assert bits_equal(got["pts"], fp32["pts"]) and not bits_equal(got["raw"], fp32["raw"])
            # the frame through render(): any slicing of the point list, the same bits
            base = scene["frame"](i, chunk=4096, retraw=False, march=grid, march_samples=K, mlp_precision="bf16")
            other = scene["frame"](i, chunk=37, retraw=False, march=grid, march_samples=K, march_points=1000,
                                   mlp_precision="bf16")
            for k in base:
                assert bits_equal(other[k], base[k]), f"{what}: {k}"
                if k.endswith("_map"):
                    assert bits_equal(base[k].reshape(got[k].shape), got[k]), f"{what}: render() vs render_rays, {k}"
    assert opaque > 0, "fixture: raise SIGMA_SCALE"


# ---------------------------------------------------------------- 3. the frame against an emulated frame
def emulated_query_fn(nerf, scene):
    """A torch query function: the package's hash features and SH, then E (the kernel's roundings, fp64 sums) and
    run_network's sigma := 0 outside the box."""
    emb, sh = scene["emb"], nerf.SHEncoder()

    def nqf(pts, viewdirs, fn):
        R, S = pts.shape[0], pts.shape[1]
        feat, keep = emb(pts.reshape(-1, 3))
        shv = sh(viewdirs[:, None].expand(R, S, 3).reshape(-1, 3))
        Wt = dict(zip(("w0", "w1", "c0", "c1", "c2"), (w.detach() for w in fn.mlp_weights())))
        raw = emulate64(Wt, feat.float(), shv.float()).float()
        raw[~keep, 3] = 0
        return raw.reshape(R, S, 4)
    return nqf


@pytest.mark.parametrize("i", [0, 1])
def test_frame_against_the_emulated_frame(nerf, gpu, scene, i):
    fp32 = scene["frame"](i)
    kern = scene["frame"](i, mlp_precision="bf16")
    emu = scene["frame"](i, network_query_fn=emulated_query_fn(nerf, scene))
    assert int((fp32["acc_map"] > 0.3).sum()) > 10, "fixture: raise SIGMA_SCALE"
    for k in ("rgb_map", "acc_map", "depth_map"):
        a, b, c = kern[k].double(), emu[k].double(), fp32[k].double()
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isnan(b), torch.isnan(c)), \
            f"pose {i}: {k} NaN pattern"
        ok = ~torch.isnan(a)
        d_kernel, d_format = float((a - b)[ok].abs().max()), float((b - c)[ok].abs().max())
        print(f"pose {i} {k}: max |kernel - emulated| = {d_kernel:.3e}, max |emulated - fp32| = {d_format:.3e}, "
              f"max |kernel - fp32| = {float((a - c)[ok].abs().max()):.3e}")
        assert d_kernel < d_format, \
            f"pose {i}: {k}: the kernel is {d_kernel:.3e} from the emulation, the format {d_format:.3e}"


# ---------------------------------------------------------------- 4. refusals, through render_rays / render
def test_refusals(nerf, gpu, scene):
    kw, frame = scene["kw"], scene["frame"]

    def run(**over):
        return frame(0, **dict(dict(mlp_precision="bf16"), **over))

    run()                                                                   # the supported call
    run(raw_noise_std=1.0)                                                  # noise is added after the field
    with pytest.raises(ValueError, match="render: mlp_precision must be None, 'fp32' or 'bf16', got 'fp16'"):
        run(mlp_precision="fp16")
    with torch.no_grad(), pytest.raises(ValueError, match="render_rays: mlp_precision must be None, 'fp32' or 'bf16'"):
        nerf.render_rays(scene["packed"](0), **scene["ray_kw"](mlp_precision=16))
    with torch.enable_grad(), pytest.raises(ValueError, match="render: mlp_precision is forward-only"):
        nerf.render(H, W, scene["K"], c2w=scene["poses"][0][:3, :4].to(gpu), **dict(kw, mlp_precision="bf16"))
    with torch.enable_grad(), pytest.raises(ValueError, match="render_rays: mlp_precision is forward-only"):
        nerf.render_rays(scene["packed"](0), **scene["ray_kw"](mlp_precision="bf16"))
    with pytest.raises(ValueError, match="mlp_precision does not support predict_normals or a normals head"):
        run(predict_normals=True)
    head = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                          input_ch=32, input_ch_views=16, predict_normals=True).to(gpu).eval()
    with pytest.raises(ValueError, match="mlp_precision does not support predict_normals or a normals head"):
        run(network_fine=head)
    emb_q = nerf.HashEmbedder(scene["bbox"], log2_hashmap_size=14, finest_resolution=512, use_quantization=True)
    emb_q = emb_q.to(gpu).eval()
    sh = nerf.SHEncoder()
    with pytest.raises(ValueError, match="render_rays: mlp_precision: A-CAQ"):
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, fn, emb_q, sh), embed_fn=emb_q)
    with pytest.raises(ValueError, match="^mlp_precision: A-CAQ"):         # caught by the field call without embed_fn
        run(network_query_fn=lambda p, v, fn: nerf.run_network(p, v, fn, emb_q, sh), embed_fn=None)
    # a query function that does not reach this package's run_network must not render in fp32 silently
    with pytest.raises(ValueError, match="mlp_precision needs a network_query_fn that calls this package's run_"):
        run(network_query_fn=emulated_query_fn(nerf, scene))
    grid = scene["grid_of"](ball_mask())
    with pytest.raises(ValueError, match="mlp_precision needs a network_query_fn"):
        run(march=grid, march_samples=16, retraw=False,
            network_query_fn=lambda p, v, fn: torch.zeros(p.shape[0], 4, device=p.device))
    # training is untouched: the keyword's default under gradients is the call without it
    with torch.enable_grad():
        out = nerf.render_rays(scene["packed"](0)[:8], **scene["ray_kw"](mlp_precision=None))
    assert out["rgb_map"].shape == (8, 3) and np.isfinite(out["rgb_map"].detach().cpu().numpy()).all()
