"""CPU-only: the occupancy-grid entries (csrc/occupancy.hip) are declared in include/nerf_hip.h, bound
in _lib and exported by the built library; their argument checks run on the host."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCC = ["nerf_occ_cell_points", "nerf_occ_compact", "nerf_occ_compact_workspace_bytes", "nerf_occ_dilate",
       "nerf_occ_mark", "nerf_occ_query"]


def test_occupancy_entries_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = sorted(set(re.findall(r"^\s*(?:int|size_t)\s+(nerf_occ_\w+)\s*\(", txt, flags=re.M)))
    assert declared == OCC
    assert sorted(n for n in L.exported_symbols() if n.startswith("nerf_occ_")) == OCC
    lib = nerf.load_library()
    for name in OCC:
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
    assert hasattr(nerf, "OccupancyGrid")


def test_occupancy_argument_checks(nerf):
    """Validation happens before any launch (no GPU is touched)."""
    import indoor_nerf_amd._lib as L
    lib = nerf.load_library()
    lo, hi = L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1])
    fake = ctypes.c_void_p(1 << 20)
    # one int32 per block of 4096 points
    assert lib.nerf_occ_compact_workspace_bytes(0) == 4
    assert lib.nerf_occ_compact_workspace_bytes(4096) == 4
    assert lib.nerf_occ_compact_workspace_bytes(4097) == 8
    with pytest.raises(RuntimeError, match="res 0"):
        L.call("nerf_occ_query", fake, 1, lo, hi, 0, fake, fake, None)
    with pytest.raises(RuntimeError, match="res 1025"):
        L.call("nerf_occ_cell_points", lo, hi, 1025, 0, 1, 1, 0, 0, fake, None)
    with pytest.raises(RuntimeError, match="empty box"):
        L.call("nerf_occ_query", fake, 1, hi, lo, 4, fake, fake, None)
    with pytest.raises(RuntimeError, match=r"cells \[60, \+10\) of 64"):
        L.call("nerf_occ_cell_points", lo, hi, 4, 60, 10, 1, 0, 0, fake, None)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        L.call("nerf_occ_mark", fake, 8, 32, 64, 4, 0.0, fake, None)
    with pytest.raises(RuntimeError, match="aliased"):
        L.call("nerf_occ_dilate", fake, 4, fake, None)
    with pytest.raises(RuntimeError, match="workspace"):
        L.call("nerf_occ_compact", fake, 5000, fake, None, 8, lo, hi, 4, fake, 3, 5000, fake, fake, fake, fake, fake,
               fake, 4, None)
    with pytest.raises(RuntimeError, match="capacity 9 of 8"):
        L.call("nerf_occ_compact", fake, 8, fake, None, 8, lo, hi, 4, fake, 3, 9, fake, fake, fake, fake, fake, fake, 4,
               None)
    with pytest.raises(RuntimeError, match="exactly one"):
        L.call("nerf_occ_compact", fake, 8, fake, fake, 8, lo, hi, 4, fake, 2, 8, fake, fake, fake, fake, fake, fake, 4,
               None)
    # empty calls launch nothing and accept NULL buffers
    L.call("nerf_occ_query", None, 0, lo, hi, 4, None, None, None)
    L.call("nerf_occ_cell_points", lo, hi, 4, 0, 0, 1, 0, 0, None, None)
    L.call("nerf_occ_mark", None, 4, 0, 0, 1, 0.0, None, None)
