"""nerf_composite_fwd / nerf_composite_bwd / nerf_composite_fwd_tv (csrc/composite.hip) against the float64
reference of tests/composite_ref.py at every width the dispatch distinguishes (needs an MI355X).

One wave handles one ray and each lane owns K = ceil(S / 64) samples; NERF_COMPOSITE_DISPATCH instantiates
K = 1, 2, 3, 4, 6, 8, and K = 6 serves S = 257 .. 384 (K = 5 pads every lane). The widths are both edges of every
template plus 300 and 320 / 321 (K = 5 -> 6) and S = 1, 2; R = 9 is two blocks and one wave, R = 1 one wave. Every
output buffer starts as NaN, so an element the kernel leaves out shows.

Bars. Forward: the project's rtol 1e-4, atol 1e-5 on all seven outputs, identical NaN pattern (a ray without any
positive sigma has acc = 0 and NaN depth and disp, as the reference). Backward without the entropy gradient: the
project's rtol 1e-3, atol 1e-5, every upstream gradient together and, at S = 300, each alone (the NULL ones switch
need_depth and the sums the backward skips). Backward of the entropy gradient alone: per ray,
|err| <= ENT_BAR * max_j |graw_ref[ray]|; -g_ent log p_j spans 16 units along a ray and the suffix recurrence
gw_j - U_j cancels it, so no float32 per-sample arithmetic meets the elementwise bar at S >= 257. ENT_BAR = 5.36e-4 is
four times the worst ratio of the float32 autograd oracle (composite_ref.composite at float32, not the code under
test) against the float64 reference over these same cases and seeds: 1.341e-4 (S = 300, C = 7; by template K = 1, 2,
3, 4, 6, 8: 9.6e-6, 5.5e-6, 2.0e-5, 2.3e-5, 1.3e-4, 5.0e-5; test_composite_ref_cpu.test_entropy_yardstick). Channel-3
elements whose reference p_j lies at the clamp's jumps (composite_ref.entropy_excluded) are left out; their share must
stay under 0.1 % and is 0 for these inputs on the CPU.
"""
import ctypes

import numpy as np
import pytest
import torch

import composite_ref as cr

pytestmark = pytest.mark.gpu

CASES = cr.composite_cases()
IDS = [f"S{S}-R{R}-C{C}-w{w}-n{n}" for S, R, C, w, n in CASES]
OUT_SHAPES = dict(rgb=lambda R, S: (R, 3), disp=lambda R, S: (R,), acc=lambda R, S: (R,), weights=lambda R, S: (R, S),
                  depth=lambda R, S: (R,), entropy=lambda R, S: (R,), normal=lambda R, S: (R, 3))


def _dev(a, gpu):
    return None if a is None else torch.tensor(np.asarray(a)).to(gpu)      # a copy: the cached inputs are read-only


def _nan(shape, gpu):
    return torch.full(shape, float("nan"), device=gpu, dtype=torch.float32)


def _forward(gpu, d, white, tv=None):
    """nerf_composite_fwd (or _fwd_tv with tv = (job, L, log2_T)) on NaN-filled outputs -> {name: array}."""
    from indoor_nerf_amd import _lib
    R, S, C = d["raw"].shape
    raw, z, rd, noise = (_dev(d.get(k), gpu) for k in ("raw", "z", "rays_d", "noise"))
    out = {n: _nan(OUT_SHAPES[n](R, S), gpu) for n in cr.FWD_NAMES if n != "normal" or C == 7}
    args = [_lib.ptr(raw), C, _lib.ptr(z), _lib.ptr(rd), _lib.ptr(noise, allow_none=True), R, S, int(white)]
    args += [_lib.ptr(out[n]) if n in out else None for n in cr.FWD_NAMES]
    if tv is None:
        _lib.call("nerf_composite_fwd", *args, _lib.stream())
    else:
        _lib.call("nerf_composite_fwd_tv", *args, ctypes.byref(tv[0]), tv[1], tv[2], _lib.stream())
    torch.cuda.synchronize()
    return {n: v.cpu().numpy() for n, v in out.items()}


def _backward(gpu, d, white, which):
    """nerf_composite_bwd with the upstream gradients named in `which` (the rest NULL) on a NaN-filled graw."""
    from indoor_nerf_amd import _lib
    R, S, C = d["raw"].shape
    raw, z, rd, noise = (_dev(d.get(k), gpu) for k in ("raw", "z", "rays_d", "noise"))
    gs = [_dev(d[n], gpu) if n in which and d.get(n) is not None else None for n in cr.GRAD_NAMES]
    graw = _nan((R, S, C), gpu)
    _lib.call("nerf_composite_bwd", _lib.ptr(raw), C, _lib.ptr(z), _lib.ptr(rd), _lib.ptr(noise, allow_none=True), R, S,
              int(white), *[_lib.ptr(g, allow_none=True) for g in gs], _lib.ptr(graw), _lib.stream())
    torch.cuda.synchronize()
    return graw.cpu().numpy()


def _check_forward(got, want, tag):
    for n, ref in zip(cr.FWD_NAMES, want):
        if ref is None:
            assert n not in got
            continue
        err = np.abs(got[n].astype(np.float64) - ref)
        ok = np.isfinite(ref)
        print(f"{tag} {n}: worst err / bar {float((err[ok] / (1e-5 + 1e-4 * np.abs(ref[ok]))).max()) if ok.any() else 0:.3f}")
    for n, ref in zip(cr.FWD_NAMES, want):
        if ref is None:
            continue
        np.testing.assert_array_equal(np.isnan(got[n]), np.isnan(ref), err_msg=f"{tag} {n}: NaN pattern")
        np.testing.assert_allclose(got[n], ref, rtol=1e-4, atol=1e-5, equal_nan=True, err_msg=f"{tag} {n}")
    assert not np.isnan(got["weights"]).any(), f"{tag}: NaN left in weights"


def _check_grad(got, want, tag):
    err = np.abs(got.astype(np.float64) - want)
    print(f"{tag}: worst err / bar {float(np.nanmax(err / (1e-5 + 1e-3 * np.abs(want)))):.3f}, max |graw| "
          f"{float(np.abs(want).max()):.3e}")
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-5, err_msg=tag)


def _check_entropy(got, want, weights64, tag):
    excluded = cr.entropy_excluded(weights64)
    ratio, share = cr.entropy_ratio(got, want, excluded)
    print(f"{tag}: worst err / max|graw_ref[ray]| {ratio:.3e} (bar {cr.ENT_BAR:.2e}), excluded share {share:.2e}")
    assert share <= cr.ENT_EXCLUDED_MAX, f"{tag}: {share:.2e} of the elements excluded"
    assert np.isfinite(got).all(), f"{tag}: non-finite gradient"
    assert (got[..., :3] == 0).all() and (got[..., 4:] == 0).all(), f"{tag}: entropy reaches sigma only"
    assert ratio <= cr.ENT_BAR, f"{tag}: {ratio:.3e} > {cr.ENT_BAR:.2e}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_vs_fp64(nerf, gpu, case):
    d = cr.composite_inputs(*case)
    _, want = cr.composite_reference(*case, ("g_entropy",))
    _check_forward(_forward(gpu, d, case[3]), want, "fwd")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_without_entropy_vs_fp64(nerf, gpu, case):
    d = cr.composite_inputs(*case)
    which = tuple(n for n in cr.REST if d[n] is not None)
    want, _ = cr.composite_reference(*case, which)
    _check_grad(_backward(gpu, d, case[3], which), want, "bwd")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_entropy_alone_vs_fp64(nerf, gpu, case):
    d = cr.composite_inputs(*case)
    want, out = cr.composite_reference(*case, ("g_entropy",))
    _check_entropy(_backward(gpu, d, case[3], ("g_entropy",)), want, out[3], "entropy")


ALONE = [(c, n) for c in CASES if c[0] == cr.ALONE_S and c[1] == 9 for n in cr.REST if n != "g_normal" or c[2] == 7]


@pytest.mark.parametrize("case,name", ALONE, ids=[f"C{c[2]}-{n}" for c, n in ALONE])
def test_backward_each_gradient_alone(nerf, gpu, case, name):
    """S = 300 (K = 5 in the K = 6 template): one upstream gradient, the rest NULL."""
    d = cr.composite_inputs(*case)
    want, _ = cr.composite_reference(*case, (name,))
    _check_grad(_backward(gpu, d, case[3], (name,)), want, name)


@pytest.mark.parametrize("S", cr.EDGE_WIDTHS)
def test_edge_rays(nerf, gpu, S):
    """composite_ref.edge_batch: a ray without positive sigma, an opaque first sample, a ray with 1 - acc < 1e-6
    (the entropy backward's clamp branch, gW = 0) and tied depths, beside plain rays."""
    d = cr.edge_batch(S)
    want_g, want = cr.edge_reference(S, ("g_rgb",))
    got = _forward(gpu, d, 0)
    _check_forward(got, want, "edge fwd")
    assert got["acc"][0] == 0 and (got["weights"][0] == 0).all() and np.isnan(got["depth"][0]) and np.isnan(got["disp"][0])
    assert 1 - want[2][2] < 1e-6 and got["acc"][2] > 1 - 1e-6
    graw = _backward(gpu, d, 0, ("g_rgb",))
    assert (graw[0, :, 3] == 0).all()
    _check_grad(graw, want_g, "edge bwd g_rgb")
    tied = np.flatnonzero(np.diff(d["z"][3]) == 0)
    assert (graw[3, tied, 3] == 0).all() and (got["weights"][3, tied] == 0).all()
    want_e, out = cr.edge_reference(S, ("g_entropy",))
    _check_entropy(_backward(gpu, d, 0, ("g_entropy",)), want_e, out[3], "edge entropy")


# ---------------------------------------------------------------- TV in the same launch
TV_LOG2_T, TV_CUBES = 12, (3, 50)
TV_MIN_VERTEX = ((5, 7, 11), (100, 200, 300))


def _tv_setup(gpu, oracle, device_corner):
    """Two levels of 2^12 rows (the 51^3 cuboid's vertices collide many times over) -> (job, keep-alive, tables,
    float64 losses, loss buffer, verts buffer, the cuboids' rows per level)."""
    from indoor_nerf_amd import _lib
    rng = np.random.RandomState(5)
    tables = [(0.1 * rng.randn(1 << TV_LOG2_T, 2)).astype(np.float32) for _ in TV_CUBES]
    want, rows, collisions = [], [], 0
    for t, mv, c in zip(tables, TV_MIN_VERTEX, TV_CUBES):
        loss, n = cr.tv_sum(oracle, t, mv, c, TV_LOG2_T)
        want.append(loss)
        collisions += n
        ar = torch.arange(c + 1)
        g = torch.stack(torch.meshgrid(mv[0] + ar, mv[1] + ar, mv[2] + ar, indexing="ij"), -1)
        rows.append(oracle.spatial_hash(g, TV_LOG2_T).reshape(-1).numpy())
    assert collisions > 100_000
    dt = [_dev(t, gpu) for t in tables]
    ptrs = _lib.ptr_array(dt)
    mv = (_lib.c_i64 * 6)(*[v for m in TV_MIN_VERTEX for v in m])
    dmv = torch.tensor(TV_MIN_VERTEX, dtype=torch.int64, device=gpu)
    cb = (_lib.c_int * 2)(*TV_CUBES)
    loss = torch.zeros(2, device=gpu)
    verts = _nan((sum((c + 1) ** 3 for c in TV_CUBES), 2), gpu)
    job = _lib.TVFwdJob(_lib.c_vp(ctypes.addressof(ptrs)), None if device_corner else _lib.c_vp(ctypes.addressof(mv)),
                        _lib.c_vp(dmv.data_ptr()) if device_corner else None, _lib.c_vp(ctypes.addressof(cb)),
                        _lib.ptr(loss), _lib.ptr(verts))
    return job, (dt, ptrs, mv, dmv, cb), tables, np.asarray(want), loss, verts, rows


def _check_tv(tables, want, loss, verts, rows, tag):
    got = loss.cpu().numpy()
    print(f"{tag}: TV losses {got} vs float64 {want}, rel err {np.abs(got - want) / want}")
    np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=tag)
    v = verts.cpu().numpy()
    np.testing.assert_array_equal(v, np.concatenate([t[r] for t, r in zip(tables, rows)]), err_msg=f"{tag}: vertex rows")


@pytest.mark.parametrize("S,device_corner", [(128, False), (300, True)])
def test_forward_with_tv_in_the_same_launch(nerf, gpu, oracle, S, device_corner):
    """nerf_composite_fwd_tv: the composite outputs are those of nerf_composite_fwd bit for bit, the per-level TV
    losses (and nerf_tv_fwd's) are the float64 TV sum to rtol 1e-5, test_tv_loss's bar; the cuboid corners come from
    the host copy at S = 128 and from device slots at S = 300."""
    from indoor_nerf_amd import _lib
    case = next(c for c in CASES if c[0] == S and c[1] == 9 and c[2] == 4)
    d = cr.composite_inputs(*case)
    job, keep, tables, want, loss, verts, rows = _tv_setup(gpu, oracle, device_corner)
    plain = _forward(gpu, d, case[3])
    fused = _forward(gpu, d, case[3], tv=(job, 2, TV_LOG2_T))
    for n in plain:
        np.testing.assert_array_equal(fused[n], plain[n], err_msg=n)
    _check_tv(tables, want, loss, verts, rows, "fused")
    loss.zero_()
    verts.fill_(float("nan"))
    dt, ptrs, mv, dmv, cb = keep
    _lib.call("nerf_tv_fwd", ptrs, 2, TV_LOG2_T, None if device_corner else mv,
              _lib.c_vp(dmv.data_ptr()) if device_corner else None, cb, _lib.ptr(loss), _lib.ptr(verts), _lib.stream())
    torch.cuda.synchronize()
    _check_tv(tables, want, loss, verts, rows, "nerf_tv_fwd")


# ---------------------------------------------------------------- rejection
@pytest.mark.parametrize("S", [0, 513])
def test_unsupported_widths_are_rejected(nerf, gpu, oracle, S):
    """S = 0 and S = 513: an error from all three entry points, and nothing written."""
    d = cr.composite_inputs(512, 9, 4, 1, 1)       # the buffers hold 513 samples a ray
    wide = dict(d, raw=np.concatenate([d["raw"], d["raw"][:, :1]], 1), z=np.concatenate([d["z"], d["z"][:, :1]], 1),
                g_weights=np.concatenate([d["g_weights"], d["g_weights"][:, :1]], 1))
    from indoor_nerf_amd import _lib
    R = 9
    raw, z, rd = _dev(wide["raw"], gpu), _dev(wide["z"], gpu), _dev(wide["rays_d"], gpu)
    out = {n: _nan(OUT_SHAPES[n](R, 513), gpu) for n in cr.FWD_NAMES[:-1]}
    fargs = [_lib.ptr(raw), 4, _lib.ptr(z), _lib.ptr(rd), None, R, S, 1] + [_lib.ptr(out[n]) for n in cr.FWD_NAMES[:-1]] + [None]
    job, keep, _, _, loss, verts, _ = _tv_setup(gpu, oracle, False)
    loss.fill_(float("nan"))
    with pytest.raises(RuntimeError, match="S must be 1..512"):
        _lib.call("nerf_composite_fwd", *fargs, _lib.stream())
    with pytest.raises(RuntimeError, match="S must be 1..512"):
        _lib.call("nerf_composite_fwd_tv", *fargs, ctypes.byref(job), 2, TV_LOG2_T, _lib.stream())
    gs = [_dev(wide[n], gpu) for n in cr.GRAD_NAMES[:-1]]
    graw = _nan((R, 513, 4), gpu)
    with pytest.raises(RuntimeError, match="S must be 1..512"):
        _lib.call("nerf_composite_bwd", *fargs[:8], *[_lib.ptr(g) for g in gs], None, _lib.ptr(graw), _lib.stream())
    torch.cuda.synchronize()
    for n, v in list(out.items()) + [("graw", graw), ("tv loss", loss), ("tv verts", verts)]:
        assert bool(torch.isnan(v).all()), f"{n} was written"
