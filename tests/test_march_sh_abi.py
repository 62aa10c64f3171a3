"""CPU-only: the entries that read SH through a ray index in the grid march (csrc/march.hip, csrc/field_x6.hip,
DESIGN.md §21) are declared in include/nerf_hip.h, bound in _lib and exported by the built library; their argument
checks run on the host before any launch (the pointers here are fakes that nothing dereferences), and empty calls
accept NULL buffers."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = "nerf_ray_sh_records"
WRITES = {"nerf_rays_march_write": "nerf_march_write", "nerf_rays_slab_march_write": "nerf_slab_march_write"}
MLPS = ["nerf_mlp_fwd_rays", "nerf_mlp_fwd_bf16_rays", "nerf_mlp_fwd_bf16_pkbf_rays"]
NEW = [RECORDS] + list(WRITES) + MLPS


def header():
    return open(os.path.join(ROOT, "include", "nerf_hip.h")).read()


def params(txt, name):
    """The parameter list of the one declaration `int name(...)` of the header, one string per parameter."""
    found = re.findall(r"^\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", txt, flags=re.M)
    assert len(found) == 1, f"{name}: {len(found)} declarations"
    return [" ".join(p.split()) for p in found[0].split(",")]


def test_entries_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = header()
    lib = nerf.load_library()
    for name in NEW:
        assert params(txt, name)
        assert name in L.exported_symbols() and name in L.SIGNATURES
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(L.SIGNATURES[name]) == len(params(txt, name))
    assert lib.nerf_abi_version() == 12          # additive entries


def test_write_entries_change_one_pointer():
    txt = header()
    for new, old in WRITES.items():
        a, b = params(txt, new), params(txt, old)
        assert len(a) == len(b)
        assert [(x, y) for x, y in zip(a, b) if x != y] == [("int32_t* d_ray_c", "float* d_sh_c")], new


def test_mlp_entries_share_one_argument_list():
    txt = header()
    want = ["int64_t feat_stride_point", "int64_t feat_stride_level", "const float* d_sh_rec", "const int32_t* d_ray_of",
            "int64_t n_rays", "const uint8_t* d_keep", "int64_t n_points", "const nerf_mlp_weights* weights",
            "float* d_raw", "void* stream"]
    for name in MLPS:
        p = params(txt, name)
        assert p[0] == ("const uint32_t* d_featw" if name.endswith("pkbf_rays") else "const float* d_feat"), name
        assert p[1:] == want, name
    assert "THE CALLER GUARANTEES 0 <= d_ray_of[p] < n_rays" in txt


def _fakes(L):
    return L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1]), ctypes.c_void_p(1 << 20)


def test_records_checks(nerf):
    import indoor_nerf_amd._lib as L
    _, _, fake = _fakes(L)
    for C in (8, 10, 12):
        with pytest.raises(RuntimeError, match=rf"ray_sh_records: ray rows of {C} columns \(11: the view direction is "
                                               r"columns 8\.\.10\)"):
            L.call(RECORDS, fake, 4, C, fake, None)
    with pytest.raises(RuntimeError, match="ray_sh_records: n_rays -1"):
        L.call(RECORDS, fake, -1, 11, fake, None)
    with pytest.raises(RuntimeError, match="ray_sh_records: 53687092 rays exceed 32-bit indexing"):
        L.call(RECORDS, fake, 53687092, 11, fake, None)          # 40 n_rays >= 2^31
    for rays, rec in ((None, fake), (fake, None)):
        with pytest.raises(RuntimeError, match="ray_sh_records: null arg"):
            L.call(RECORDS, rays, 4, 11, rec, None)
    for off in (4, 8, 12):
        with pytest.raises(RuntimeError, match="ray_sh_records: SH records must be 16-B aligned"):
            L.call(RECORDS, fake, 4, 11, ctypes.c_void_p((1 << 20) + off), None)
    L.call(RECORDS, None, 0, 11, None, None)                     # no rays: nothing launched


def test_write_checks(nerf):
    """Every check of the existing writes, under the new entries' names, and the index pointer."""
    import indoor_nerf_amd._lib as L
    lo, hi, fake = _fakes(L)

    def write(name, R=8, C=8, K=64, k0=0, k1=64, lo=lo, hi=hi, res=4, p=fake, n=8, cap=8, ray_c=fake):
        slab = (k0, k1) if "slab" in name else ()
        L.call(name, p, R, C, p, K, *slab, lo, hi, res, p, p, p, n, cap, p, p, p, ray_c, None)

    for name in WRITES:
        who = name[len("nerf_"):]
        with pytest.raises(RuntimeError, match="null box"):
            write(name, lo=None)
        with pytest.raises(RuntimeError, match="empty box"):
            write(name, lo=hi, hi=lo)
        for res in (0, 1025):
            with pytest.raises(RuntimeError, match=f"res {res}"):
                write(name, res=res)
        for C in (7, 9, 3, 12):
            with pytest.raises(RuntimeError, match=rf"{who}: ray rows of {C} columns \(8 or 11\)"):
                write(name, C=C)
        for K in (0, -1, 4097):
            with pytest.raises(RuntimeError, match=rf"{who}: n_samples {K} \(1\.\.4096\)"):
                write(name, K=K, k0=0, k1=0)
        with pytest.raises(RuntimeError, match=f"{who}: 524288 rays x 4096 samples exceed 2\\^31 - 1; use a smaller chunk"):
            write(name, R=1 << 19, K=4096)
        with pytest.raises(RuntimeError, match=f"{who}: n_rays -1"):
            write(name, R=-1)
        with pytest.raises(RuntimeError, match=f"{who}: capacity 7 below the count 8"):
            write(name, cap=7)
        with pytest.raises(RuntimeError, match=f"{who}: count -1"):
            write(name, n=-1)
        with pytest.raises(RuntimeError, match=f"{who}: null arg"):
            write(name, p=None)
        with pytest.raises(RuntimeError, match=f"{who}: null arg"):
            write(name, ray_c=None)
        for C in (8, 11):                                        # empty: nothing launched, NULL buffers
            for R in (0, 8):
                slab = (8, 8) if "slab" in name else ()
                L.call(name, None, R, C, None, 64, *slab, lo, hi, 4, None, None, None, 0, 0, None, None, None, None, None)
    for k0, k1 in ((-1, 8), (9, 8), (0, 65)):
        with pytest.raises(RuntimeError, match=rf"rays_slab_march_write: lattice range \[{k0}, {k1}\) of 64 samples"):
            write("nerf_rays_slab_march_write", k0=k0, k1=k1)
    with pytest.raises(RuntimeError, match="rays_slab_march_write: count 17 of 16 lattice samples"):
        write("nerf_rays_slab_march_write", k0=62, k1=64, n=17, cap=17)


def test_mlp_checks(nerf):
    import indoor_nerf_amd._lib as L
    _, _, fake = _fakes(L)
    W = L.MlpWeights(*[1 << 20] * 5)

    def run(name, feat=fake, sp=2, sl=2 * 64, rec=fake, ray_of=fake, n_rays=4, keep=None, n=64, w=W, raw=fake):
        L.call(name, feat, sp, sl, rec, ray_of, n_rays, keep, n, None if w is None else ctypes.byref(w), raw, None)

    for name in MLPS:
        who = name[len("nerf_"):]
        with pytest.raises(RuntimeError, match=f"{who}: n_points -1, n_rays 4"):
            run(name, n=-1)
        with pytest.raises(RuntimeError, match=f"{who}: n_points 64, n_rays -1"):
            run(name, n_rays=-1)
        with pytest.raises(RuntimeError, match=f"{who}: null weight pointer"):
            run(name, w=None)
        with pytest.raises(RuntimeError, match=f"{who}: null weight pointer"):
            run(name, w=L.MlpWeights(1 << 20, 1 << 20, 0, 1 << 20, 1 << 20))
        for missing in ("feat", "rec", "ray_of", "raw"):
            with pytest.raises(RuntimeError, match=f"{who}: null arg"):
                run(name, **{missing: None})
        with pytest.raises(RuntimeError, match=f"{who}: 64 points need n_rays >= 1"):
            run(name, n_rays=0)
        with pytest.raises(RuntimeError, match=f"{who}: 53687092 rays exceed 32-bit indexing"):
            run(name, n_rays=53687092)
        with pytest.raises(RuntimeError, match=f"{who}: SH records must be 16-B aligned"):
            run(name, rec=ctypes.c_void_p((1 << 20) + 8))
        with pytest.raises(RuntimeError, match=f"{who}: 64 points exceed 32-bit indexing"):
            run(name, sl=1 << 27)                                # 16 feat_stride_level >= 2^31
        with pytest.raises(RuntimeError, match=f"{who}: 134217728 points exceed 32-bit indexing"):
            run(name, n=1 << 27)                                 # 16 (n + 32) >= 2^31
        # empty: nothing launched; NULL per-point buffers and records, any n_rays
        for n_rays in (0, 4):
            L.call(name, None, 2, 0, None, None, n_rays, None, 0, ctypes.byref(W), None, None)


def test_keyword_default_and_where_it_is_absent(nerf):
    from indoor_nerf_amd import model, occupancy, sparse_field
    assert inspect.signature(nerf.render_rays).parameters["march_sh"].default is None
    assert list(inspect.signature(sparse_field.check_march_sh).parameters) == ["value", "march", "prefix"]
    assert "march_sh" in sparse_field.NOT_IN_TRAINING
    assert "index" in inspect.signature(occupancy.OccupancyGrid._march_write).parameters
    for fn in (occupancy.OccupancyGrid.update, occupancy.OccupancyGrid.march, occupancy.OccupancyGrid.compact):
        assert not any("march_sh" in p or p == "index" for p in inspect.signature(fn).parameters), fn.__name__
    for name, fn in inspect.getmembers(model, inspect.isfunction):      # the training path
        assert "march_sh" not in inspect.signature(fn).parameters, name
