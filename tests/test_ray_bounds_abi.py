"""CPU-only: the per-ray sample-bound entries (csrc/ray_span.hip) are declared in include/nerf_hip.h, bound
in _lib and exported by the built library; their argument checks run on the host."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN = ["nerf_ray_span", "nerf_ray_span_gather", "nerf_ray_span_workspace_bytes"]


def test_ray_span_entries_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = sorted(set(re.findall(r"^\s*(?:int|size_t)\s+(nerf_ray_span\w*)\s*\(", txt, flags=re.M)))
    assert declared == SPAN
    assert sorted(n for n in L.exported_symbols() if n.startswith("nerf_ray_span")) == SPAN
    lib = nerf.load_library()
    for name in SPAN:
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
    assert lib.nerf_abi_version() == 12          # additive entries
    assert inspect.signature(nerf.render).parameters["ray_bounds"].default is None
    assert callable(nerf.OccupancyGrid.ray_span)


def test_ray_span_argument_checks(nerf):
    """Validation happens before any launch (no GPU is touched)."""
    import indoor_nerf_amd._lib as L
    lib = nerf.load_library()
    lo, hi = L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1])
    fake = ctypes.c_void_p(1 << 20)
    # one int32 per block of 4096 rays
    assert lib.nerf_ray_span_workspace_bytes(0) == 4
    assert lib.nerf_ray_span_workspace_bytes(4096) == 4
    assert lib.nerf_ray_span_workspace_bytes(4097) == 8
    assert lib.nerf_ray_span_workspace_bytes(-1) == 0

    def span(R=8, C=8, lo=lo, hi=hi, res=4, p=fake, ws=fake, ws_bytes=4):
        L.call("nerf_ray_span", p, R, C, lo, hi, res, p, p, p, p, ws, ws_bytes, None)

    with pytest.raises(RuntimeError, match="null box"):
        span(lo=None)
    with pytest.raises(RuntimeError, match="empty box"):
        span(lo=hi, hi=lo)
    with pytest.raises(RuntimeError, match="res 1025"):
        span(res=1025)
    with pytest.raises(RuntimeError, match="res 0"):
        span(res=0)
    for C in (7, 9, 3, 12):
        with pytest.raises(RuntimeError, match=f"rows of {C} columns"):
            span(C=C)
    with pytest.raises(RuntimeError, match="workspace 4 B < 8 B"):
        span(R=4097)
    with pytest.raises(RuntimeError, match="workspace"):
        span(ws=None)
    with pytest.raises(RuntimeError, match="n_rays -1"):
        span(R=-1)
    with pytest.raises(RuntimeError, match="null arg"):
        span(p=None)
    # a box far from the origin at a high resolution: cells of fewer than 2^13 floats, too few for the pad
    with pytest.raises(RuntimeError, match="cells below 2\\^-10 of the box bounds on axis 0"):
        span(lo=L.host_f32([1000, -1, -1]), hi=L.host_f32([1001, 1, 1]), res=16)

    def gather(R=8, C=8, cap=8, p=fake, ws=fake, ws_bytes=4):
        L.call("nerf_ray_span_gather", p, R, C, p, p, cap, p, p, ws, ws_bytes, None)

    with pytest.raises(RuntimeError, match="capacity 9 of 8 rays"):
        gather(cap=9)
    with pytest.raises(RuntimeError, match="capacity -1 of 8 rays"):
        gather(cap=-1)
    for C in (7, 10):
        with pytest.raises(RuntimeError, match=f"rows of {C} columns"):
            gather(C=C)
    with pytest.raises(RuntimeError, match="workspace 4 B < 8 B"):
        gather(R=5000, cap=1)
    with pytest.raises(RuntimeError, match="workspace"):
        gather(ws=None)
    with pytest.raises(RuntimeError, match="null arg"):
        gather(p=None)


def test_ray_span_empty_calls_accept_null_buffers(nerf):
    """No rays, or no hit rays to gather: nothing is launched and NULL buffers are accepted."""
    import indoor_nerf_amd._lib as L
    lo, hi = L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1])
    for C in (8, 11):
        L.call("nerf_ray_span", None, 0, C, lo, hi, 4, None, None, None, None, None, 0, None)
        L.call("nerf_ray_span_gather", None, 0, C, None, None, 0, None, None, None, 0, None)
        L.call("nerf_ray_span_gather", None, 8, C, None, None, 0, None, None, None, 0, None)


def test_ray_bounds_refusals(nerf):
    """render(ray_bounds=...) is forward-only and takes an OccupancyGrid; both are refused before anything is
    launched (the rays live on the CPU here)."""
    import numpy as np
    import torch
    o = torch.zeros(4, 3)
    d = torch.tensor([[0.0, 0.0, -1.0]]).repeat(4, 1)
    box = (torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]))
    grid = nerf.OccupancyGrid(box, resolution=2, device="cpu")
    for bad in (object(), 0.5, box):
        with torch.no_grad(), pytest.raises(ValueError, match="must be an OccupancyGrid"):
            nerf.render(2, 2, np.eye(3), rays=(o, d), ndc=False, ray_bounds=bad, N_samples=4)
    with torch.enable_grad(), pytest.raises(ValueError, match="forward-only"):
        nerf.render(2, 2, np.eye(3), rays=(o, d), ndc=False, ray_bounds=grid, N_samples=4)
    for shape in ((4, 6), (8,), (2, 2, 8)):
        with pytest.raises(ValueError, match="packed rows"):
            grid.ray_span(torch.zeros(shape))
