"""CPU-only: the packed bf16 feature entries (csrc/hashgrid_pkbf.hip, csrc/field_x6.hip) are declared
in include/nerf_hip.h, bound in _lib and exported by the built library; their argument checks run on the host before
any launch, and render_rays and HashEmbedder.encode_into have the keywords."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENC, ENC_HALF, MLP = "nerf_hash_encode_fwd_pkbf", "nerf_hash_encode_fwd_half_pkbf", "nerf_mlp_fwd_bf16_pkbf"
UNPACKED = {ENC: "nerf_hash_encode_fwd", ENC_HALF: "nerf_hash_encode_fwd_half", MLP: "nerf_mlp_fwd_bf16"}


def header():
    return open(os.path.join(ROOT, "include", "nerf_hip.h")).read()


def declaration(txt, name):
    """The argument list of `int name(...)` in the header, whitespace collapsed."""
    m = re.search(r"^\s*int\s+" + name + r"\s*\(([^;]*)\);", txt, flags=re.M)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entries_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = header()
    lib = nerf.load_library()
    for name in (ENC, ENC_HALF, MLP):
        assert re.findall(r"^\s*int\s+(" + name + r")\s*\(", txt, flags=re.M) == [name]
        assert name in L.SIGNATURES and name in L.exported_symbols()
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
    assert lib.nerf_abi_version() == 12          # additive entries
    # the name patterns of the entries these sit beside still match one declaration each
    assert re.findall(r"^\s*int\s+(nerf_hash_encode_fwd_half)\s*\(", txt, flags=re.M) == ["nerf_hash_encode_fwd_half"]
    assert re.findall(r"^\s*int\s+(nerf_mlp_fwd_bf16)\s*\(", txt, flags=re.M) == ["nerf_mlp_fwd_bf16"]
    assert re.findall(r"^\s*int\s+(nerf_hash_encode_fwd)\s*\(", txt, flags=re.M) == ["nerf_hash_encode_fwd"]


@pytest.mark.parametrize("name", [ENC, ENC_HALF, MLP])
def test_signature_is_the_unpacked_entrys_with_one_pointer_changed(nerf, name):
    """The same arguments in the same order; the feature pointer alone changes its type (and its name)."""
    import indoor_nerf_amd._lib as L
    assert L.SIGNATURES[name] == L.SIGNATURES[UNPACKED[name]]        # every pointer is a void* to ctypes
    txt = header()
    new, old = declaration(txt, name), declaration(txt, UNPACKED[name])
    assert len(new) == len(old) == 13
    changed = [(a, b) for a, b in zip(new, old) if a != b]
    if name == MLP:
        assert changed == [("const uint32_t* d_featw", "const float* d_feat")]
    else:
        assert changed == [("uint32_t* d_featw", "float* d_feat")]


def test_python_keywords(nerf):
    assert inspect.signature(nerf.render_rays).parameters["feature_precision"].default is None
    assert inspect.signature(nerf.HashEmbedder.encode_into).parameters["packed"].default is False
    from indoor_nerf_amd import sparse_field
    Req = sparse_field.FieldRequest
    assert inspect.signature(Req).parameters["packed"].default is False
    assert Req(bf16=True).packed is False and Req(bf16=True, packed=True).packed is True
    assert list(inspect.signature(sparse_field.check_feature_precision).parameters) == ["value", "mlp_bf16", "prefix"]
    assert "feature_precision" not in inspect.signature(nerf.OccupancyGrid.update).parameters


def _box(L):
    return L.host_f32([-1.0, -1.0, -1.0]), L.host_f32([1.0, 1.0, 1.0]), L.host_f32([16.0, 32.0])


def _enc(L, name, n, xyz=None, src=None, featw=None, keep=None, n_levels=2, log2_T=12, box=True):
    lo, hi, res = _box(L)
    if box is not True:
        lo, hi, res = box
    L.call(name, xyz, n, lo, hi, res, n_levels, log2_T, src, featw, 2, 1, keep, None)


def _source(L, name, tables=(1 << 20, 1 << 21)):
    """A non-NULL table argument of the entry: the pointer array, or the image."""
    return (L.c_vp * 2)(*tables) if name == ENC else ctypes.c_void_p(1 << 20)


@pytest.mark.parametrize("name", [ENC, ENC_HALF])
def test_encoder_empty_batch_accepts_null_data(nerf, name):
    """Zero points: NERF_OK before any launch with NULL per-point buffers; the tables and the box are still checked."""
    import indoor_nerf_amd._lib as L
    who = name[len("nerf_"):]
    _enc(L, name, 0, src=_source(L, name))
    if name == ENC:
        _enc(L, name, 0, src=(L.c_vp * 2)())                    # as the fp32 entry: the tables are read per launch
    with pytest.raises(RuntimeError, match=f"{who}: null arg"):
        _enc(L, name, 0)
    lo, hi, res = _box(L)
    for box in ((None, hi, res), (lo, None, res), (lo, hi, None)):
        with pytest.raises(RuntimeError, match=f"{who}: null arg"):
            _enc(L, name, 0, src=_source(L, name), box=box)


@pytest.mark.parametrize("name", [ENC, ENC_HALF])
def test_encoder_null_and_range_arguments_are_refused(nerf, name):
    """One point with a NULL buffer, or a count out of range: each is refused on the host (no launch is reached), in
    the unpacked entry's words with this entry's name. d_keep may be NULL."""
    import indoor_nerf_amd._lib as L
    who = name[len("nerf_"):]
    fake, src = ctypes.c_void_p(1 << 20), _source(L, name)
    for args in (dict(xyz=None, src=src, featw=fake), dict(xyz=fake, src=src, featw=None),
                 dict(xyz=fake, src=None, featw=fake)):
        with pytest.raises(RuntimeError, match=f"{who}: null arg"):
            _enc(L, name, 1, **args)
    with pytest.raises(RuntimeError, match=f"{who}: n_points < 0"):
        _enc(L, name, -1, xyz=fake, src=src, featw=fake)
    for n_levels in (0, -1, L.MAX_LEVELS + 1):
        with pytest.raises(RuntimeError, match=f"{who}: n_levels {n_levels}"):
            _enc(L, name, 1, xyz=fake, src=src, featw=fake, n_levels=n_levels)
    for log2_T in (0, 31):
        with pytest.raises(RuntimeError, match=f"{who}: log2_T {log2_T}"):
            _enc(L, name, 1, xyz=fake, src=src, featw=fake, log2_T=log2_T)
    if name == ENC:
        with pytest.raises(RuntimeError, match="hash_encode_fwd_pkbf: table 1 is null"):
            _enc(L, name, 1, xyz=fake, src=_source(L, name, (1 << 20, None)), featw=fake)


def _mlp(L, n, featw=None, sh=None, dirs=None, spr=1, sh_stride=16, w=None, raw=None, keep=None, order=None, sl=None):
    L.call(MLP, featw, 1, n if sl is None else sl, sh, sh_stride, dirs, spr, keep, n,
           None if w is None else ctypes.byref(w), raw, order, None)


def test_mlp_empty_batch_accepts_null_data(nerf):
    import indoor_nerf_amd._lib as L
    w = L.MlpWeights(*([1 << 20] * 5))
    _mlp(L, 0, w=w)
    _mlp(L, 0, w=w, order=ctypes.byref(L.PointOrder(None, 0, 0)))
    with pytest.raises(RuntimeError, match="null feature/weight pointer"):
        _mlp(L, 0)
    with pytest.raises(RuntimeError, match="null feature/weight pointer"):
        _mlp(L, 0, w=L.MlpWeights(1 << 20, 1 << 20, None, 1 << 20, 1 << 20))


def test_mlp_null_and_range_arguments_are_refused(nerf):
    """nerf_mlp_fwd_bf16's refusals, with this entry's name where the message names one."""
    import indoor_nerf_amd._lib as L
    fake = ctypes.c_void_p(1 << 20)
    w = L.MlpWeights(*([1 << 20] * 5))
    with pytest.raises(RuntimeError, match="null feature/weight pointer"):
        _mlp(L, 1, featw=None, sh=fake, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="null feature/weight pointer"):
        _mlp(L, 1, featw=fake, sh=fake, w=None, raw=fake)
    with pytest.raises(RuntimeError, match="need d_sh or d_viewdirs"):
        _mlp(L, 1, featw=fake, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="mlp_fwd_bf16_pkbf: null output"):
        _mlp(L, 1, featw=fake, sh=fake, w=w, raw=None)
    with pytest.raises(RuntimeError, match="samples_per_ray must be >= 1"):
        _mlp(L, 1, featw=fake, dirs=fake, spr=0, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="per-ray SH rows must be 16-B aligned"):
        _mlp(L, 1, featw=fake, sh=ctypes.c_void_p((1 << 20) + 4), sh_stride=0, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="n_points < 0"):
        _mlp(L, -1, featw=fake, sh=fake, w=w, raw=fake)
    with pytest.raises(RuntimeError, match="point order: seg_split 2 of 1 points"):
        _mlp(L, 1, featw=fake, sh=fake, w=w, raw=fake, order=ctypes.byref(L.PointOrder(None, 2, 1)))
    # 2^27 points x 16 levels of words pass 2^31 element indices, as for the fp32 features
    P = 1 << 27
    with pytest.raises(RuntimeError, match="32-bit indexing") as e:
        _mlp(L, P, featw=fake, dirs=fake, spr=192, sh_stride=0, w=w, raw=fake)
    assert str(e.value).endswith(f"mlp_fwd_bf16_pkbf: {P} points exceed 32-bit indexing")
    # the unpacked entry keeps its own name
    with pytest.raises(RuntimeError, match="mlp_fwd_bf16: null output"):
        L.call("nerf_mlp_fwd_bf16", fake, 2, 2, fake, 16, None, 1, None, 1, ctypes.byref(w), None, None, None)
