"""CPU-only: the entries that read their point count on the device (csrc/hashgrid_pkbf.hip, csrc/field_x6.hip, DESIGN.md
§23) are declared in include/nerf_hip.h, bound in _lib and exported by the built library; each takes (d_total, base,
capacity) where its host-sized twin takes n_points; their argument checks run on the host before any launch (the
pointers here are fakes that nothing dereferences), and a capacity of 0 launches nothing and accepts NULL buffers."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENC, ENC_HALF, MLP = ("nerf_hash_encode_fwd_pkbf_dev", "nerf_hash_encode_fwd_half_pkbf_dev",
                      "nerf_mlp_fwd_bf16_pkbf_rays_dev")
TWIN = {name: name[:-len("_dev")] for name in (ENC, ENC_HALF, MLP)}
COUNT = ["const int32_t* d_total", "int64_t base", "int64_t capacity"]


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
    for name in TWIN:
        assert params(txt, name)
        assert name in L.exported_symbols() and name in L.SIGNATURES
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(L.SIGNATURES[name]) == len(params(txt, name))
    assert lib.nerf_abi_version() == 12          # additive entries
    for twin in TWIN.values():                   # the twins are declared as they were, once each
        assert params(txt, twin)


def test_signatures_replace_the_count():
    """A _dev entry is its twin with n_points replaced: by (d_total, base, capacity, max_blocks) in the encoders, by
    (d_total, base, capacity) in the MLP. Nothing else differs, names and order included."""
    txt = header()
    for name, twin in TWIN.items():
        new, old = params(txt, name), params(txt, twin)
        at = old.index("int64_t n_points")
        put = COUNT + (["int max_blocks"] if name != MLP else [])
        assert new == old[:at] + put + old[at + 1:], name
    import indoor_nerf_amd._lib as L
    for name, twin in TWIN.items():
        a, b = L.SIGNATURES[name], L.SIGNATURES[twin]
        at = params(txt, twin).index("int64_t n_points")
        put = [L.c_vp, L.c_i64, L.c_i64] + ([L.c_int] if name != MLP else [])
        assert a == b[:at] + put + b[at + 1:], name


def _fakes(L):
    return L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1]), ctypes.c_void_p(1 << 20)


def test_encoder_checks(nerf):
    import indoor_nerf_amd._lib as L
    lo, hi, fake = _fakes(L)
    res = L.host_f32([16.0 * 1.3 ** i for i in range(16)])
    tables = (L.c_vp * 16)(*[1 << 20] * 16)

    def run(name, xyz=fake, total=fake, base=0, cap=64, max_blocks=0, lo=lo, hi=hi, res=res, levels=16, log2_T=19,
            src="given", words=fake, sp=1, sl=64, keep=fake):
        if src == "given":
            src = tables if name == ENC else fake
        L.call(name, xyz, total, base, cap, max_blocks, lo, hi, res, levels, log2_T, src, words, sp, sl, keep, None)

    for name in (ENC, ENC_HALF):
        who = name[len("nerf_"):]
        with pytest.raises(RuntimeError, match=f"{who}: capacity < 0"):
            run(name, cap=-1)
        with pytest.raises(RuntimeError, match=f"{who}: base < 0"):
            run(name, base=-1)
        with pytest.raises(RuntimeError, match=f"{who}: max_blocks < 0"):
            run(name, max_blocks=-1)
        with pytest.raises(RuntimeError, match=f"{who}: null count"):
            run(name, total=None)
        with pytest.raises(RuntimeError, match=f"{who}: null count"):
            run(name, total=None, cap=0)                         # also when nothing would be launched
        for levels in (0, 17):
            with pytest.raises(RuntimeError, match=f"{who}: n_levels {levels}"):
                run(name, levels=levels)
        for log2_T in (0, 31):
            with pytest.raises(RuntimeError, match=f"{who}: log2_T {log2_T}"):
                run(name, log2_T=log2_T)
        for missing in ("xyz", "words", "src", "res", "lo", "hi"):
            with pytest.raises(RuntimeError, match=f"{who}: null arg"):
                run(name, **{missing: None})
        with pytest.raises(RuntimeError, match=f"{who}: capacity 2147483648 exceeds one launch"):
            run(name, cap=1 << 31)
        with pytest.raises(RuntimeError, match=f"{who}: capacity 1073741824 exceeds one launch"):
            run(name, cap=1 << 30)                               # 2^27 virtual blocks at 16 levels
        # a capacity of 0: nothing launched, NULL per-point buffers, any base and grid cap
        for base, max_blocks in ((0, 0), (37, 3)):
            run(name, xyz=None, words=None, keep=None, cap=0, base=base, max_blocks=max_blocks, sl=0)
    with pytest.raises(RuntimeError, match="hash_encode_fwd_pkbf_dev: table 5 is null"):
        holed = (L.c_vp * 16)(*[1 << 20] * 16)
        holed[5] = None
        run(ENC, src=holed)


def test_mlp_checks(nerf):
    import indoor_nerf_amd._lib as L
    _, _, fake = _fakes(L)
    W = L.MlpWeights(*[1 << 20] * 5)
    who = MLP[len("nerf_"):]

    def run(feat=fake, sp=1, sl=64, rec=fake, ray_of=fake, n_rays=4, keep=None, total=fake, base=0, cap=64, w=W, raw=fake):
        L.call(MLP, feat, sp, sl, rec, ray_of, n_rays, keep, total, base, cap, None if w is None else ctypes.byref(w), raw,
               None)

    with pytest.raises(RuntimeError, match=f"{who}: capacity -1, base 0, n_rays 4"):
        run(cap=-1)
    with pytest.raises(RuntimeError, match=f"{who}: capacity 64, base -1, n_rays 4"):
        run(base=-1)
    with pytest.raises(RuntimeError, match=f"{who}: capacity 64, base 0, n_rays -1"):
        run(n_rays=-1)
    with pytest.raises(RuntimeError, match=f"{who}: null weight pointer"):
        run(w=None)
    with pytest.raises(RuntimeError, match=f"{who}: null weight pointer"):
        run(w=L.MlpWeights(1 << 20, 1 << 20, 0, 1 << 20, 1 << 20))
    for cap in (64, 0):
        with pytest.raises(RuntimeError, match=f"{who}: null count"):
            run(total=None, cap=cap)
    for missing in ("feat", "rec", "ray_of", "raw"):
        with pytest.raises(RuntimeError, match=f"{who}: null arg"):
            run(**{missing: None})
    with pytest.raises(RuntimeError, match=f"{who}: a capacity of 64 points needs n_rays >= 1"):
        run(n_rays=0)
    with pytest.raises(RuntimeError, match=f"{who}: 53687092 rays exceed 32-bit indexing"):
        run(n_rays=53687092)
    with pytest.raises(RuntimeError, match=f"{who}: SH records must be 16-B aligned"):
        run(rec=ctypes.c_void_p((1 << 20) + 8))
    with pytest.raises(RuntimeError, match=f"{who}: capacity 64 exceeds 32-bit indexing"):
        run(sl=1 << 27)                                          # 16 feat_stride_level >= 2^31
    with pytest.raises(RuntimeError, match=f"{who}: capacity 134217728 exceeds 32-bit indexing"):
        run(cap=1 << 27)                                         # 16 (capacity + 32) >= 2^31
    for n_rays, base in ((0, 0), (4, 37)):                       # a capacity of 0: nothing launched, NULL buffers
        L.call(MLP, None, 1, 0, None, None, n_rays, None, fake, base, 0, ctypes.byref(W), None, None)


def test_keyword_default_and_where_it_is_absent(nerf):
    from indoor_nerf_amd import model, occupancy, sparse_field
    assert inspect.signature(nerf.render_rays).parameters["march_sizes"].default is None
    assert list(inspect.signature(sparse_field.check_march_sizes).parameters) == \
        ["value", "march", "by_ray", "bf16", "packed", "prefix"]
    assert inspect.signature(sparse_field.field_options).parameters["march_sizes"].default is None
    assert sparse_field.FieldOptions._fields == ("bf16", "half", "packed", "by_ray", "stop")      # the flag is not in it
    assert inspect.signature(occupancy.OccupancyGrid._march_count).parameters["sized"].default == "host"
    assert inspect.signature(nerf.HashEmbedder.encode_into).parameters["count"].default is None
    assert "march_sizes" in sparse_field.NOT_IN_TRAINING
    for fn in (occupancy.OccupancyGrid.update, occupancy.OccupancyGrid.march, occupancy.OccupancyGrid.compact):
        assert not any(p in ("march_sizes", "sized") for p in inspect.signature(fn).parameters), fn.__name__
    for name, fn in inspect.getmembers(model, inspect.isfunction):      # the training path
        assert "march_sizes" not in inspect.signature(fn).parameters, name
