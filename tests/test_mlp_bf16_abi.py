"""CPU-only: the bf16 MLP forward entry (csrc/field_x6.hip mlp_fwd_bf16_kernel) is declared in
include/nerf_hip.h, bound in _lib and exported by the built library; its argument checks run on the host before
any launch, and render_rays has the keyword."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "nerf_mlp_fwd_bf16"


def test_entry_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert re.findall(r"^\s*int\s+(nerf_mlp_fwd_bf16)\s*\(", txt, flags=re.M) == [NAME]
    assert NAME in L.exported_symbols()
    lib = nerf.load_library()
    assert hasattr(lib, NAME), f"libnerfhip.so does not export {NAME}"
    assert lib.nerf_abi_version() == 12          # an additive entry
    # nerf_mlp_fwd_ord's arguments without d_geo, d_act_qrec, d_act_minmax, act_calib_points
    sig, ord_sig = L.SIGNATURES[NAME], L.SIGNATURES["nerf_mlp_fwd_ord"]
    assert sig == ord_sig[:11] + ord_sig[15:]
    assert inspect.signature(nerf.render_rays).parameters["mlp_precision"].default is None


def _call(L, n, feat=None, sh=None, dirs=None, spr=1, sh_stride=16, w=None, raw=None, keep=None, order=None, sl=None):
    L.call(NAME, feat, 2, 2 * n if sl is None else sl, sh, sh_stride, dirs, spr, keep, n,
           None if w is None else ctypes.byref(w), raw, order, None)


def test_empty_batch_accepts_null_data(nerf):
    """Zero points: NERF_OK before any launch with NULL per-point buffers; the weights are still checked."""
    import indoor_nerf_amd._lib as L
    w = L.MlpWeights(*([1 << 20] * 5))
    _call(L, 0, w=w)
    _call(L, 0, w=w, order=ctypes.byref(L.PointOrder(None, 0, 0)))
    with pytest.raises(RuntimeError, match="null feature/weight pointer"):
        _call(L, 0)
    with pytest.raises(RuntimeError, match="null feature/weight pointer"):
        _call(L, 0, w=L.MlpWeights(1 << 20, 1 << 20, None, 1 << 20, 1 << 20))


def test_null_arguments_are_refused(nerf):
    """One point with a NULL buffer: each is refused on the host (no launch is reached). A quantizer record or a
    geo output cannot be asked for: the entry has no such argument."""
    import indoor_nerf_amd._lib as L
    fake = ctypes.c_void_p(1 << 20)
    w = L.MlpWeights(*([1 << 20] * 5))
    with pytest.raises(RuntimeError, match="null feature/weight pointer"):
        _call(L, 1, feat=None, sh=fake, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="null feature/weight pointer"):
        _call(L, 1, feat=fake, sh=fake, w=None, raw=fake)
    with pytest.raises(RuntimeError, match="need d_sh or d_viewdirs"):
        _call(L, 1, feat=fake, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="mlp_fwd_bf16: null output"):
        _call(L, 1, feat=fake, sh=fake, w=w, raw=None)
    with pytest.raises(RuntimeError, match="samples_per_ray must be >= 1"):
        _call(L, 1, feat=fake, dirs=fake, spr=0, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="per-ray SH rows must be 16-B aligned"):
        _call(L, 1, feat=fake, sh=ctypes.c_void_p((1 << 20) + 4), sh_stride=0, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="n_points < 0"):
        _call(L, -1, feat=fake, sh=fake, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="point order: seg_split 2 of 1 points"):
        _call(L, 1, feat=fake, sh=fake, w=w, raw=fake, order=ctypes.byref(L.PointOrder(None, 2, 1)))


def test_refuses_batches_past_32bit_indexing(nerf):
    """As nerf_mlp_fwd: 2^27 points x 16 levels would pass 2^31 element indices; refused before any launch, in
    the same words apart from the entry's name."""
    import indoor_nerf_amd._lib as L
    fake = ctypes.c_void_p(1 << 20)
    w = L.MlpWeights(*([1 << 20] * 5))
    P = 1 << 27
    with pytest.raises(RuntimeError, match="32-bit indexing") as e:
        _call(L, P, feat=fake, dirs=fake, spr=192, sh_stride=0, w=w, raw=fake)
    assert str(e.value).endswith(f"mlp_fwd_bf16: {P} points exceed 32-bit indexing")
    with pytest.raises(RuntimeError) as e0:
        L.call("nerf_mlp_fwd", fake, 2, 2 * P, None, 0, fake, 192, None, P, ctypes.byref(w), fake, None, None)
    assert str(e0.value).endswith(f"mlp_fwd(x6): {P} points exceed 32-bit indexing")
