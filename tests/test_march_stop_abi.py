"""CPU-only: the entries that stop rays inside the grid march (csrc/march.hip) are declared in
include/nerf_hip.h, bound in _lib and exported by the built library; their argument checks run on the host before
any launch (the pointers here are fakes that nothing dereferences), and empty calls accept NULL buffers."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAB = ["nerf_slab_march_advance", "nerf_slab_march_composite", "nerf_slab_march_count", "nerf_slab_march_write"]


def test_entries_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    declared = sorted(set(re.findall(r"^\s*int\s+(nerf_slab_march_\w+)\s*\(", txt, flags=re.M)))
    assert declared == SLAB
    assert sorted(n for n in L.exported_symbols() if n.startswith("nerf_slab_march_")) == SLAB
    lib = nerf.load_library()
    for name in SLAB:
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
        assert getattr(lib, name).restype is ctypes.c_int and len(getattr(lib, name).argtypes) == len(L.SIGNATURES[name])
    assert lib.nerf_abi_version() == 12          # additive entries
    for fn in (nerf.render_rays,):
        p = inspect.signature(fn).parameters
        assert p["march_stop"].default is None and p["march_stop_slab"].default == 128


def _host(L):
    return L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1]), ctypes.c_void_p(1 << 20)


def test_count_and_write_checks(nerf):
    import indoor_nerf_amd._lib as L
    lo, hi, fake = _host(L)

    def count(R=8, C=8, K=64, k0=0, k1=64, alive=fake, lo=lo, hi=hi, res=4, p=fake, ws=fake, ws_bytes=4):
        L.call("nerf_slab_march_count", p, R, C, p, K, k0, k1, alive, lo, hi, res, p, p, p, p, ws, ws_bytes, None)

    def write(R=8, C=8, K=64, k0=0, k1=64, lo=lo, hi=hi, res=4, p=fake, n=8, cap=8, sh=None):
        L.call("nerf_slab_march_write", p, R, C, p, K, k0, k1, lo, hi, res, p, p, p, n, cap, p, p, p, sh, None)

    for fn in (count, write):
        # the range
        for k0, k1 in ((-1, 8), (9, 8), (0, 65), (65, 65), (64, 63)):
            with pytest.raises(RuntimeError, match=rf"lattice range \[{k0}, {k1}\) of 64 samples"):
                fn(k0=k0, k1=k1)
        # every check of the existing entries
        with pytest.raises(RuntimeError, match="null box"):
            fn(lo=None)
        with pytest.raises(RuntimeError, match="empty box"):
            fn(lo=hi, hi=lo)
        for res in (0, 1025):
            with pytest.raises(RuntimeError, match=f"res {res}"):
                fn(res=res)
        for C in (7, 9, 3, 12):
            with pytest.raises(RuntimeError, match=f"rows of {C} columns"):
                fn(C=C)
        for K in (0, -1, 4097):
            with pytest.raises(RuntimeError, match=f"n_samples {K} \\(1..4096\\)"):
                fn(K=K, k0=0, k1=0)
        with pytest.raises(RuntimeError, match="use a smaller chunk"):
            fn(R=1 << 19, K=4096)
        with pytest.raises(RuntimeError, match="n_rays -1"):
            fn(R=-1)
        with pytest.raises(RuntimeError, match="slab_march_(count|write): null arg"):
            fn(p=None)
    with pytest.raises(RuntimeError, match="workspace 4 B < 8 B"):
        count(R=4097)
    with pytest.raises(RuntimeError, match="workspace"):
        count(ws=None)
    with pytest.raises(RuntimeError, match="capacity 7 below the count 8"):
        write(cap=7)
    with pytest.raises(RuntimeError, match="count 17 of 16 lattice samples"):
        write(k0=62, k1=64, n=17, cap=17)             # at most n_rays * (k1 - k0)
    with pytest.raises(RuntimeError, match="count -1"):
        write(n=-1)
    with pytest.raises(RuntimeError, match="11 columns"):
        write(sh=fake)


def test_composite_and_advance_checks(nerf):
    import indoor_nerf_amd._lib as L
    _, _, fake = _host(L)

    def composite(R=8, n=8, p=fake, raw=fake, state=fake, first=1, last=1):
        L.call("nerf_slab_march_composite", raw, p, p, p, p, R, n, 0, state, first, last, p, p, p, p, None, None)

    def advance(R=8, n=8, s1=64, tau_max=1.0, p=fake, raw=fake, dist=fake):
        L.call("nerf_slab_march_advance", raw, dist, p, p, R, n, s1, tau_max, p, p, p, None)

    for fn in (composite, advance):
        with pytest.raises(RuntimeError, match="n_rays -1"):
            fn(R=-1)
        with pytest.raises(RuntimeError, match="n_points -1"):
            fn(n=-1)
        with pytest.raises(RuntimeError, match="n_points 32769 of 8 rays"):
            fn(n=8 * 4096 + 1)
        with pytest.raises(RuntimeError, match="null arg"):
            fn(p=None)
        with pytest.raises(RuntimeError, match="null arg"):
            fn(raw=None)
    with pytest.raises(RuntimeError, match="slab_march_composite: null state"):
        composite(state=None)
    with pytest.raises(RuntimeError, match="null state"):
        composite(state=None, first=0, last=0)
    with pytest.raises(RuntimeError, match="16-B aligned"):
        composite(raw=ctypes.c_void_p((1 << 20) + 4))
    with pytest.raises(RuntimeError, match="null arg"):
        advance(dist=None)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="tau_max .* must be positive"):
            advance(tau_max=bad)
    for bad in (-1, 4097):
        with pytest.raises(RuntimeError, match=f"slab end {bad}"):
            advance(s1=bad)


def test_empty_calls_accept_null_buffers(nerf):
    """No rays, or an empty list to write: nothing is launched and NULL buffers are accepted."""
    import indoor_nerf_amd._lib as L
    lo, hi, _ = _host(L)
    for C in (8, 11):
        for k0, k1 in ((0, 64), (8, 8), (63, 64)):
            L.call("nerf_slab_march_count", None, 0, C, None, 64, k0, k1, None, lo, hi, 4, None, None, None, None, None, 0,
                   None)
            for R in (0, 8):
                L.call("nerf_slab_march_write", None, R, C, None, 64, k0, k1, lo, hi, 4, None, None, None, 0, 0, None, None,
                       None, None, None)
    L.call("nerf_slab_march_composite", None, None, None, None, None, 0, 0, 0, None, 1, 1, None, None, None, None, None,
           None)
    L.call("nerf_slab_march_advance", None, None, None, None, 0, 0, 8, 1.0, None, None, None, None)
