"""CPU-only: the grid ray-marching entries (csrc/march.hip) are declared in include/nerf_hip.h, bound in _lib
and exported by the built library; their argument checks run on the host, and render_rays' refusals with
march= are raised before anything is launched (the tensors live on the CPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARCH = ["nerf_march_composite", "nerf_march_count", "nerf_march_workspace_bytes", "nerf_march_write"]


def test_march_entries_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = sorted(set(re.findall(r"^\s*(?:int|size_t)\s+(nerf_march_\w+)\s*\(", txt, flags=re.M)))
    assert declared == MARCH
    assert sorted(n for n in L.exported_symbols() if n.startswith("nerf_march_")) == MARCH
    lib = nerf.load_library()
    for name in MARCH:
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
    assert lib.nerf_abi_version() == 12          # additive entries
    p = inspect.signature(nerf.render_rays).parameters
    assert p["march"].default is None and p["march_samples"].default == 512 and p["march_points"].default == 1 << 21
    assert callable(nerf.OccupancyGrid.march)


def test_march_argument_checks(nerf):
    """Validation happens before any launch (no GPU is touched)."""
    import indoor_nerf_amd._lib as L
    lib = nerf.load_library()
    lo, hi = L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1])
    fake = ctypes.c_void_p(1 << 20)
    # one int32 per block of 4096 rays
    assert lib.nerf_march_workspace_bytes(0) == 4
    assert lib.nerf_march_workspace_bytes(4096) == 4
    assert lib.nerf_march_workspace_bytes(4097) == 8
    assert lib.nerf_march_workspace_bytes(-1) == 0

    def count(R=8, C=8, K=64, lo=lo, hi=hi, res=4, p=fake, ws=fake, ws_bytes=4):
        L.call("nerf_march_count", p, R, C, p, K, lo, hi, res, p, p, p, p, ws, ws_bytes, None)

    def write(R=8, C=8, K=64, lo=lo, hi=hi, res=4, p=fake, n=8, cap=8, sh=None):
        L.call("nerf_march_write", p, R, C, p, K, lo, hi, res, p, p, p, n, cap, p, p, p, sh, None)

    for fn in (count, write):
        with pytest.raises(RuntimeError, match="null box"):
            fn(lo=None)
        with pytest.raises(RuntimeError, match="empty box"):
            fn(lo=hi, hi=lo)
        with pytest.raises(RuntimeError, match="res 1025"):
            fn(res=1025)
        with pytest.raises(RuntimeError, match="res 0"):
            fn(res=0)
        for C in (7, 9, 3, 12):
            with pytest.raises(RuntimeError, match=f"rows of {C} columns"):
                fn(C=C)
        for K in (0, -1, 4097):
            with pytest.raises(RuntimeError, match=f"n_samples {K} \\(1..4096\\)"):
                fn(K=K)
        with pytest.raises(RuntimeError, match="use a smaller chunk"):
            fn(R=1 << 19, K=4096)                       # 2^31 lattice samples
        with pytest.raises(RuntimeError, match="n_rays -1"):
            fn(R=-1)
        with pytest.raises(RuntimeError, match="null arg"):
            fn(p=None)
    with pytest.raises(RuntimeError, match="workspace 4 B < 8 B"):
        count(R=4097)
    with pytest.raises(RuntimeError, match="workspace"):
        count(ws=None)
    with pytest.raises(RuntimeError, match="capacity 7 below the count 8"):
        write(cap=7)
    with pytest.raises(RuntimeError, match="count 513 of 512 lattice samples"):
        write(n=513, cap=513)
    with pytest.raises(RuntimeError, match="count -1"):
        write(n=-1)
    with pytest.raises(RuntimeError, match="11 columns"):
        write(sh=fake)                                  # SH rows of rays without view directions

    def composite(R=8, n=8, p=fake, raw=fake):
        L.call("nerf_march_composite", raw, p, p, p, p, R, n, 0, p, p, p, p, None, None)

    with pytest.raises(RuntimeError, match="n_rays -1"):
        composite(R=-1)
    with pytest.raises(RuntimeError, match="n_points -1"):
        composite(n=-1)
    with pytest.raises(RuntimeError, match="n_points 32769 of 8 rays"):
        composite(n=8 * 4096 + 1)
    with pytest.raises(RuntimeError, match="null arg"):
        composite(p=None)
    with pytest.raises(RuntimeError, match="null arg"):
        composite(raw=None)
    with pytest.raises(RuntimeError, match="16-B aligned"):
        composite(raw=ctypes.c_void_p((1 << 20) + 4))


def test_march_empty_calls_accept_null_buffers(nerf):
    """No rays, or an empty list to write: nothing is launched and NULL buffers are accepted."""
    import indoor_nerf_amd._lib as L
    lo, hi = L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1])
    for C in (8, 11):
        L.call("nerf_march_count", None, 0, C, None, 64, lo, hi, 4, None, None, None, None, None, 0, None)
        L.call("nerf_march_write", None, 0, C, None, 64, lo, hi, 4, None, None, None, 0, 0, None, None, None, None, None)
        L.call("nerf_march_write", None, 8, C, None, 64, lo, hi, 4, None, None, None, 0, 0, None, None, None, None, None)
    L.call("nerf_march_composite", None, None, None, None, None, 0, 0, 0, None, None, None, None, None, None)


def test_march_refusals(nerf):
    """Every refusal of render_rays(march=...) is a ValueError that names march, raised before any launch."""
    import torch
    box = (torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]))
    grid = nerf.OccupancyGrid(box, resolution=2, device="cpu")
    rays = torch.zeros(4, 11)
    net = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                         input_ch=32, input_ch_views=16)
    emb = nerf.HashEmbedder(box, log2_hashmap_size=8, finest_resolution=32)

    def run(rays=rays, fn=net, **over):
        return nerf.render_rays(rays, fn, None, 8, **dict(dict(march=grid, embed_fn=emb), **over))

    for bad in (object(), 0.5, box):
        with torch.no_grad(), pytest.raises(ValueError, match="march must be an OccupancyGrid"):
            run(march=bad)
    for bad in (0, -1, 4097, 2.5, None, True):
        with torch.no_grad(), pytest.raises(ValueError, match="march.*march_samples"):
            run(march_samples=bad)
    for bad in (0, -5, 1.5, 1 << 28):
        with torch.no_grad(), pytest.raises(ValueError, match="march.*march_points"):
            run(march_points=bad)
    with torch.no_grad(), pytest.raises(ValueError, match="march does not combine with occupancy"):
        run(occupancy=grid)
    with torch.no_grad(), pytest.raises(ValueError, match="march does not combine with .*early_stop"):
        run(early_stop=1e-3)
    with torch.enable_grad(), pytest.raises(ValueError, match="march is forward-only"):
        run()
    with torch.no_grad(), pytest.raises(ValueError, match="march needs raw_noise_std == 0"):
        run(raw_noise_std=1.0)
    with torch.no_grad(), pytest.raises(ValueError, match="march needs perturb == 0"):
        run(perturb=1.0)
    with torch.no_grad(), pytest.raises(ValueError, match="march needs lindisp=False"):
        run(lindisp=True)
    with torch.no_grad(), pytest.raises(ValueError, match="march does not support predict_normals"):
        run(predict_normals=True)
    head = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                          input_ch=32, input_ch_views=16, predict_normals=True)
    with torch.no_grad(), pytest.raises(ValueError, match="march does not support predict_normals or a normals head"):
        run(network_fine=head)
    emb_q = nerf.HashEmbedder(box, log2_hashmap_size=8, finest_resolution=32, use_quantization=True)
    with torch.no_grad(), pytest.raises(ValueError, match="march: A-CAQ"):
        run(embed_fn=emb_q)
    with torch.no_grad(), pytest.raises(ValueError, match="march: needs the fused field modules"):
        run(fn=torch.nn.Linear(3, 4))
    with torch.no_grad(), pytest.raises(ValueError, match="march needs ray rows with view directions"):
        run(rays=torch.zeros(4, 8))
    # render() refuses the packed entries of several chunks
    o, d = torch.zeros(4, 3), torch.tensor([[0.0, 0.0, -1.0]]).repeat(4, 1)
    with torch.no_grad(), pytest.raises(ValueError, match="retraw is not available with march"):
        nerf.render(2, 2, np.eye(3), rays=(o, d), ndc=False, march=grid, retraw=True, N_samples=4)
    # OccupancyGrid.march's own checks
    for shape in ((4, 6), (8,), (2, 2, 8)):
        with pytest.raises(ValueError, match="packed rows"):
            grid.march(torch.zeros(shape), 8)
    with pytest.raises(ValueError, match="march_samples"):
        grid.march(torch.zeros(4, 8), 4097)
    with pytest.raises(ValueError, match="use a smaller chunk"):
        grid.march(torch.zeros(1 << 19, 8), 4096)
