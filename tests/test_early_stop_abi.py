"""CPU-only: the early-termination entries (csrc/early_stop.hip) are declared in include/nerf_hip.h, bound
in _lib and exported by the built library; their argument checks run on the host."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERT = ["nerf_ert_advance", "nerf_ert_compact", "nerf_ert_compact_workspace_bytes"]


def test_early_stop_entries_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = sorted(set(re.findall(r"^\s*(?:int|size_t)\s+(nerf_ert_\w+)\s*\(", txt, flags=re.M)))
    assert declared == ERT
    assert sorted(n for n in L.exported_symbols() if n.startswith("nerf_ert_")) == ERT
    lib = nerf.load_library()
    for name in ERT:
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
    assert lib.nerf_abi_version() == 12          # additive entries
    assert nerf.last_early_stop_counts() == (0, 0)
    for fn in (nerf.render_rays,):
        p = inspect.signature(fn).parameters
        assert p["early_stop"].default is None and p["early_stop_slab"].default == 32


def test_early_stop_argument_checks(nerf):
    """Validation happens before any launch (no GPU is touched)."""
    import indoor_nerf_amd._lib as L
    lib = nerf.load_library()
    lo, hi = L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1])
    fake = ctypes.c_void_p(1 << 20)
    # one int32 per block of 4096 candidates
    assert lib.nerf_ert_compact_workspace_bytes(0) == 4
    assert lib.nerf_ert_compact_workspace_bytes(4096) == 4
    assert lib.nerf_ert_compact_workspace_bytes(4097) == 8

    def compact(R=8, S=64, s0=0, s1=8, alive=fake, sh=fake, vd=None, lo=lo, hi=hi, res=4, bits=fake, stages=3, cap=0,
                ws_bytes=4):
        L.call("nerf_ert_compact", fake, R, S, s0, s1, alive, sh, vd, lo, hi, res, bits, stages, cap, fake, fake, fake,
               fake, fake, fake, ws_bytes, None)

    with pytest.raises(RuntimeError, match=r"slab \[60, 65\) of 64"):
        compact(s0=60, s1=65)
    with pytest.raises(RuntimeError, match=r"slab \[-1, 8\) of 64"):
        compact(s0=-1)
    with pytest.raises(RuntimeError, match=r"slab \[9, 8\) of 64"):
        compact(s0=9)
    with pytest.raises(RuntimeError, match="capacity 65 of 64 candidates"):
        compact(cap=65)
    with pytest.raises(RuntimeError, match="workspace"):
        compact(R=1000, s1=8, ws_bytes=4)          # 8000 candidates: two blocks
    with pytest.raises(RuntimeError, match="null box"):
        compact(lo=None)
    with pytest.raises(RuntimeError, match="empty box"):
        compact(lo=hi, hi=lo)
    with pytest.raises(RuntimeError, match="res 1025"):
        compact(res=1025)
    with pytest.raises(RuntimeError, match="exactly one"):
        compact(vd=fake)
    with pytest.raises(RuntimeError, match="stages 4"):
        compact(stages=4)
    with pytest.raises(RuntimeError, match="n_rays"):
        compact(R=1 << 26)                          # R * S past 32-bit point indices

    def advance(R=8, S=64, s0=0, s1=8, tau_max=1.0, p=fake):
        L.call("nerf_ert_advance", p, p, p, R, S, s0, s1, tau_max, p, p, p, None)

    with pytest.raises(RuntimeError, match=r"slab \[56, 64\) must end before the last of 64"):
        advance(s0=56, s1=64)                       # no decision follows the last slab
    with pytest.raises(RuntimeError, match=r"slab \[-8, 0\)"):
        advance(s0=-8, s1=0)
    with pytest.raises(RuntimeError, match="tau_max"):
        advance(tau_max=0.0)
    with pytest.raises(RuntimeError, match="tau_max"):
        advance(tau_max=float("nan"))
    with pytest.raises(RuntimeError, match="null arg"):
        advance(p=None)


def test_early_stop_empty_calls_accept_null_buffers(nerf):
    """No rays, or an empty slab: nothing is launched and NULL buffers are accepted (the count stage's
    4-byte clear is the only device operation, and it is not asked for here)."""
    import indoor_nerf_amd._lib as L
    lo, hi = L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1])
    fake = ctypes.c_void_p(1 << 20)
    for R, s0, s1 in ((0, 0, 8), (8, 8, 8)):
        L.call("nerf_ert_compact", None, R, 64, s0, s1, None, None, None, lo, hi, 4, None, 2, 0, None, fake, None, None,
               None, fake, 4, None)
    L.call("nerf_ert_advance", None, None, None, 0, 64, 0, 8, 1.0, None, None, None, None)


def test_early_stop_parameter_checks(nerf):
    """eps outside (0, 1) and a slab below 1 are refused before anything else is looked at."""
    import torch
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        with torch.no_grad(), pytest.raises(ValueError, match="early_stop must be"):
            nerf.render_rays(torch.zeros(1, 11), None, None, 8, early_stop=bad)
    for bad in (0, -3, 2.5):
        with torch.no_grad(), pytest.raises(ValueError, match="early_stop_slab"):
            nerf.render_rays(torch.zeros(1, 11), None, None, 8, early_stop=1e-3, early_stop_slab=bad)
