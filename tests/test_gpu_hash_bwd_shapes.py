"""The hash backward's bin and owner passes (csrc/hashgrid.hip: bwd_bin_block / bin_chunk, hash_bwd_owner_kernel)
against the float64 scatter of hash_bwd_ref.py at the shapes where they take their other paths (needs an MI355X).

Each case drives the C entries through _lib.call on a workspace filled with 0xA5 bytes, in three modes unless it
says otherwise: the default binned path (nerf_hash_encode_bwd_ws, deterministic 0), the deterministic one (run
twice, bit-identical) and the float atomics (nerf_hash_encode_bwd). Bars per row and feature, with scale = the
scatter of |terms| and count = the terms of the row:

* default      |got - want| <= 2e-6 * scale + 1e-30: three fp32 products, at most six additions of the in-wave run
               merge and the final rounding of the fp64 slice sum are about 10 * 2^-24 = 6e-7 (the 1 - w the kernel
               forms in fp32 and the reference in float64 adds three more roundings: 13 * 2^-24 = 8e-7).
* deterministic the same plus count * 2^-70 * M, M the level's largest |term|: the owner rounds every entry to a
               fixed-point grid of about 2^-75 of the level's largest entry; the bar allows 32 times that. (An
               entry is a term or a merged run of up to 64, so the largest term is the stricter M. The grid is
               half of 2^(E + 2b - 123) for entries below 2^E and at most 2^b of them, b = 12 + bits of the chunk
               count: 2^-73 of the largest entry at the 4,099 chunks of case e, 2^-91 or finer elsewhere.)
* atomics      (count + 10) * 2^-24 * scale + 1e-30: count fp32 additions in any order.

Rows without a term keep their prior contents bit for bit. Every case prints max(err / bound) per mode; DESIGN.md
§2 records the largest.
"""
import numpy as np
import pytest
import torch

import hash_bwd_ref as hb
from tables import blender_bbox

pytestmark = pytest.mark.gpu

LEVELS = (16.0, 1024.0)
MODES = ("default", "deterministic", "atomics")
OVERWRITE = 2                      # NERF_OWNER_OVERWRITE (include/nerf_hip.h)


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(nerf, gpu, oracle):
    from indoor_nerf_amd import _lib
    c = _Ctx()
    c.L, c.lib, c.gpu, c.oracle = _lib, _lib.load(), gpu, oracle
    c.C = int(c.lib.nerf_hash_bwd_chunk_points())
    assert c.C == 512                                  # the CPU test's fixture conditions are stated for it
    lo, hi = blender_bbox()
    c.lo, c.hi = torch.from_numpy(lo), torch.from_numpy(hi)
    c.bmin, c.bmax = _lib.host_f32(lo), _lib.host_f32(hi)
    return c


# ---------------------------------------------------------------- drivers
def _dev(c, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(c.gpu)


def _workspace(c, n_levels, log2_T, n_points, det):
    nbytes = int(c.lib.nerf_hash_encode_bwd_workspace_bytes(n_levels, log2_T, n_points, det))
    assert nbytes > 0, (n_levels, log2_T, n_points, det)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=c.gpu)
    ws.fill_(0xA5)                                     # stale bytes must not matter
    return ws, nbytes


def _tables(c, n_levels, log2_T, stale=False):
    if not stale:
        return [torch.zeros(1 << log2_T, 2, device=c.gpu) for _ in range(n_levels)]
    return [torch.full((8 << log2_T,), 0xA5, dtype=torch.uint8, device=c.gpu).view(torch.float32).view(-1, 2)
            for _ in range(n_levels)]


def _run(c, mode, xt, P, levels, log2_T, dptr, sp, sl):
    """One whole backward into zeroed tables. dptr: device pointer of (point 0, level 0, feature 0)."""
    _lib, n = c.L, len(levels)
    g = _tables(c, n, log2_T)
    res = _lib.host_f32(levels)
    if mode == "atomics":
        _lib.call("nerf_hash_encode_bwd", _lib.ptr(xt), P, c.bmin, c.bmax, res, n, log2_T, dptr, sp, sl,
                  _lib.ptr_array(g), _lib.stream())
    else:
        det = int(mode == "deterministic")
        ws, nbytes = _workspace(c, n, log2_T, P, det)
        _lib.call("nerf_hash_encode_bwd_ws", _lib.ptr(xt), P, c.bmin, c.bmax, res, n, log2_T, dptr, sp, sl,
                  _lib.ptr_array(g), det, _lib.ptr(ws, dtype=torch.uint8), nbytes, _lib.stream())
    torch.cuda.synchronize()
    return g


def _bin(c, xt, P, levels, log2_T, dt, sp, sl, base, cap, det, ws, nbytes):
    _lib = c.L
    _lib.call("nerf_hash_encode_bwd_bin", _lib.ptr(xt), P, c.bmin, c.bmax, _lib.host_f32(levels), len(levels), log2_T,
              _lib.ptr(dt), sp, sl, base, cap, det, _lib.ptr(ws, dtype=torch.uint8), nbytes, _lib.stream())


def _owner(c, n_levels, lv0, lv1, log2_T, n_chunks, cap, g, flags, ws, nbytes):
    _lib = c.L
    _lib.call("nerf_hash_encode_bwd_owner_range", n_levels, lv0, lv1, log2_T, n_chunks, cap, _lib.ptr_array(g), flags,
              _lib.ptr(ws, dtype=torch.uint8), nbytes, _lib.stream())
    torch.cuda.synchronize()


# ---------------------------------------------------------------- reference and bars
def _refs(c, x, d, levels, log2_T):
    """Per level (want, scale, count, M) for points x [P, 3] and gradients d [L, P, 2] (NumPy)."""
    out = []
    for lvl, r in enumerate(levels):
        want, scale, count, _ = hb.scatter_ref(c.oracle, x, d[lvl], c.lo, c.hi, r, log2_T)
        out.append((want, scale, count, hb.largest_term(c.oracle, x, d[lvl], c.lo, c.hi, r)))
    return out


def _bound(mode, scale, count, M):
    if mode == "atomics":
        return (count.double() + 10)[:, None] * 2.0 ** -24 * scale + 1e-30
    b = 2e-6 * scale + 1e-30
    if mode == "deterministic":
        b = b + (count.double() * 2.0 ** -70 * M)[:, None]
    return b


_WORST = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(case, mode, got, refs, levels=None, bound=_bound):
    """got[lvl] (device) against refs[lvl]; rows without a term are +0 bit for bit. Prints max(err / bound)."""
    worst = 0.0
    for lvl, (want, scale, count, M) in enumerate(refs):
        if levels is not None and lvl not in levels:
            continue
        g = got[lvl].cpu()
        assert bool(torch.isfinite(g).all()), f"{case} {mode} level {lvl}: non-finite gradient"
        assert not bool(_bits(g[count == 0]).any()), f"{case} {mode} level {lvl}: a row without a term was written"
        ratio = (g.double() - want).abs() / bound(mode, scale, count, M)
        worst = max(worst, float(ratio.max()))
        assert float(ratio.max()) <= 1.0, (f"{case} {mode} level {lvl}: max err / bound {float(ratio.max()):.3f} at row "
                                           f"{int(ratio.max(1).values.argmax())}, {int((ratio > 1).any(1).sum())} rows off")
    _WORST[mode] = max(_WORST.get(mode, 0.0), worst)
    print(f"hash-bwd {case:<28s} {mode:<13s} max err/bound {worst:.4f}   (largest so far {_WORST[mode]:.4f})")
    return worst


def _all_modes(c, case, x, d, levels=LEVELS, log2_T=19, modes=MODES):
    """Level-major gradients d [L, P, 2] through every mode; the deterministic one twice, bit-identical."""
    P, n = x.shape[0], len(levels)
    xt, dt = _dev(c, x), _dev(c, d)
    refs = _refs(c, x, d, levels, log2_T)
    out = {}
    for mode in modes:
        g = _run(c, mode, xt, P, levels, log2_T, c.L.ptr(dt), 2, 2 * P)
        if mode == "deterministic":
            g2 = _run(c, mode, xt, P, levels, log2_T, c.L.ptr(dt), 2, 2 * P)
            for a, b in zip(g, g2):
                assert torch.equal(_bits(a), _bits(b)), f"{case}: deterministic runs differ"
        _check(case, mode, g, refs)
        out[mode] = g
    return out, refs


# ---------------------------------------------------------------- the cases
RAGGED = {"1": lambda C: 1, "63": lambda C: 63, "64": lambda C: 64, "65": lambda C: 65, "C-1": lambda C: C - 1,
          "C": lambda C: C, "C+1": lambda C: C + 1, "2C+1": lambda C: 2 * C + 1}


@pytest.mark.parametrize("P", list(RAGGED))
def test_a_ragged_counts(ctx, P):
    """A last wave with 1 or 63 valid lanes, a last chunk with one point; a tenth of the points outside the box;
    three levels (an odd count for the owner's level dispatch order)."""
    P = RAGGED[P](ctx.C)
    x = hb.random_points(P, seed=100 + P)
    d = hb.random_grads(3, P, seed=200 + P)
    _all_modes(ctx, f"a ragged P={P}", x, d, levels=(16.0, 27.0, 1024.0))


def test_b_runs(ctx):
    """Runs of 1..70, 128, 130 and C + 1 copies of a point at two lane offsets, and the two short scan variants
    (hash_bwd_ref.run_points; its layout is asserted in test_hash_bwd_ref_cpu.py)."""
    x, _ = hb.run_points(ctx.C)
    d = hb.random_grads(2, len(x), seed=3)
    _all_modes(ctx, "b runs", x, d)


def test_c_one_cell_one_slice(ctx):
    C = ctx.C
    x = hb.identical_points(4097)                                               # (i)
    _all_modes(ctx, "c(i) 4097 identical", x, hb.random_grads(2, len(x), seed=11))
    x = hb.one_cell_points(C)                                                   # (ii)
    _all_modes(ctx, "c(ii) one finest cell", x, hb.random_grads(2, C, seed=12))
    for mode, (log2_T, slice_log2) in hb.ONE_SLICE.items():                     # (iii)
        x, _ = hb.one_slice_points(ctx.oracle, C, log2_T, slice_log2)
        d = np.concatenate([hb.random_grads(1, C, seed=4), hb.random_grads(1, C, seed=13)])
        _all_modes(ctx, f"c(iii) one slice 2^{log2_T}", x, d, log2_T=log2_T, modes=(mode, "atomics"))
    x = hb.vertex_points(C)                                                     # (iv): level 16 all dropped as zero
    d = hb.random_grads(2, C, seed=14)
    d[0] = 0.0
    out, _ = _all_modes(ctx, "c(iv) finest vertices", x, d)
    for g in out.values():
        assert not bool(_bits(g[0]).any())
    x = hb.random_points(3 * C, seed=15)                                        # (v): a chunk of +-0 gradients
    d = hb.random_grads(2, 3 * C, seed=16)
    d[:, C:2 * C] = 0.0
    d[:, C:2 * C:2] = -0.0
    assert np.signbit(d[:, C:2 * C:2]).all()
    _all_modes(ctx, "c(v) zero chunk", x, d)


@pytest.mark.parametrize("mode,log2_T", [("default", t) for t in (4, 12, 13, 14, 20)] +
                         [("deterministic", t) for t in (11, 12, 13, 19)])
def test_d_table_sizes(ctx, mode, log2_T):
    """Partial, exactly one and many owner slices (2^13 rows in the default mode, 2^12 in the deterministic one) up
    to the 128 owners of the default mode's largest binned table."""
    P = 3 * ctx.C + 1
    if mode == "default" and log2_T == 20:
        assert int(ctx.lib.nerf_hash_encode_bwd_workspace_bytes(2, 20, P, 0)) > 0       # binned, 128 owners
    _all_modes(ctx, f"d log2_T={log2_T}", hb.random_points(P, seed=log2_T), hb.random_grads(2, P, seed=50 + log2_T),
               log2_T=log2_T, modes=(mode,))


def test_d_binned_path_ends(ctx):
    """log2_T 21: no binned path, and _ws with a workspace pointer still gives the atomics' result. log2_T 20 with the
    deterministic flag: refused with the documented error."""
    _lib, P = ctx.L, 3 * ctx.C + 1
    x, d = hb.random_points(P, seed=21), hb.random_grads(2, P, seed=71)
    xt, dt = _dev(ctx, x), _dev(ctx, d)
    res = _lib.host_f32(LEVELS)
    assert int(ctx.lib.nerf_hash_encode_bwd_workspace_bytes(2, 21, P, 0)) == 0
    assert int(ctx.lib.nerf_hash_encode_bwd_workspace_bytes(2, 20, P, 1)) == 0
    spare = torch.full((4096,), 0xA5, dtype=torch.uint8, device=ctx.gpu)
    refs = _refs(ctx, x, d, LEVELS, 21)
    for ws in (spare, None):
        g = _tables(ctx, 2, 21)
        _lib.call("nerf_hash_encode_bwd_ws", _lib.ptr(xt), P, ctx.bmin, ctx.bmax, res, 2, 21, _lib.ptr(dt), 2, 2 * P,
                  _lib.ptr_array(g), 0, _lib.ptr(ws, dtype=torch.uint8, allow_none=True), 4096 if ws is not None else 0,
                  _lib.stream())
        torch.cuda.synchronize()
        _check("d log2_T=21 via _ws", "atomics", g, refs)
    assert bool((spare == 0xA5).all())
    g = _tables(ctx, 2, 20)
    with pytest.raises(RuntimeError, match="deterministic mode needs the binned path"):
        _lib.call("nerf_hash_encode_bwd_ws", _lib.ptr(xt), P, ctx.bmin, ctx.bmax, res, 2, 20, _lib.ptr(dt), 2, 2 * P,
                  _lib.ptr_array(g), 1, _lib.ptr(spare, dtype=torch.uint8), 4096, _lib.stream())
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in g)


def test_e_two_owner_windows(ctx):
    """4099 chunks: the owner pass scans its chunks in windows of kScanPer * THREADS = 4 * 1024 = 4096 (csrc/
    hashgrid.hip, hash_bwd_owner_kernel: `constexpr int kOwnerWindow = kScanPer * THREADS`, no entry exports it), so
    this walks a second window: the last thread's s_pre[nw] store of a full window, the barrier between windows and
    region0 with w0 > 0. Gradients are zero except where hash_bwd_ref.window_grads puts them."""
    C = ctx.C
    P = 4098 * C + 1
    assert (P + C - 1) // C > 4 * 1024
    rng = np.random.RandomState(8)
    lo, hi = blender_bbox()
    x = (lo + (hi - lo) * rng.rand(P, 3).astype(np.float32)).astype(np.float32)
    d, live = hb.window_grads(P, C, 2)
    refs = _refs(ctx, x[live], d[:, live], LEVELS, 19)
    xt, dt = _dev(ctx, x), _dev(ctx, d)
    for mode in ("default", "deterministic"):
        g = _run(ctx, mode, xt, P, LEVELS, 19, ctx.L.ptr(dt), 2, 2 * P)
        _check("e 4099 chunks", mode, g, refs)
        if mode == "deterministic":
            g2 = _run(ctx, mode, xt, P, LEVELS, 19, ctx.L.ptr(dt), 2, 2 * P)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(g, g2))


def test_f_strides(ctx):
    """Level-major (2, 2P), point-major (2L, 2) and a [P, 48] buffer with NaN in the unused columns (48, 2)."""
    _lib, P, n = ctx.L, 2 * ctx.C + 1, 2
    x, d = hb.random_points(P, seed=31), hb.random_grads(n, P, seed=32)
    refs = _refs(ctx, x, d, LEVELS, 19)
    xt = _dev(ctx, x)
    level_major = _dev(ctx, d)
    point_major = _dev(ctx, d.transpose(1, 0, 2))                                # [P, L, 2]
    wide_np = np.full((P, 48), np.nan, np.float32)
    wide_np[:, 6:6 + 2 * n] = d.transpose(1, 0, 2).reshape(P, 2 * n)
    wide = _dev(ctx, wide_np)
    layouts = (("(2, 2P)", _lib.ptr(level_major), 2, 2 * P), ("(2L, 2)", _lib.ptr(point_major), 2 * n, 2),
               ("(48, 2)", _lib.ptr_at(wide, 6), 48, 2))
    for mode in MODES:
        first = None
        for name, dptr, sp, sl in layouts:
            g = _run(ctx, mode, xt, P, LEVELS, 19, dptr, sp, sl)
            _check(f"f strides {name}", mode, g, refs)
            if mode == "deterministic":
                first = first or g
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, g)), name


@pytest.mark.parametrize("mode", ["default", "deterministic"])
def test_g_accumulate_overwrite_ranges(ctx, mode):
    """Two bin calls (chunks [0, 3) of 2C + 1 points, chunk 3 of C - 1) share one owner pass; level ranges, the
    accumulating second pass and NERF_OWNER_OVERWRITE on tables of stale bytes."""
    C, det, levels, T = ctx.C, int(mode == "deterministic"), (16.0, 27.0, 1024.0), 19
    Pa, Pb, cap = 2 * C + 1, C - 1, 4
    xa, xb = hb.random_points(Pa, seed=41), hb.random_points(Pb, seed=42)
    da, db = hb.random_grads(3, Pa, seed=43), hb.random_grads(3, Pb, seed=44)
    refs = _refs(ctx, np.concatenate([xa, xb]), np.concatenate([da, db], 1), levels, T)
    ws, nbytes = _workspace(ctx, 3, T, C * cap, det)
    xat, xbt, dat, dbt = (_dev(ctx, a) for a in (xa, xb, da, db))
    _bin(ctx, xat, Pa, levels, T, dat, 2, 2 * Pa, 0, cap, det, ws, nbytes)
    _bin(ctx, xbt, Pb, levels, T, dbt, 2, 2 * Pb, 3, cap, det, ws, nbytes)
    whole = _tables(ctx, 3, T)
    _owner(ctx, 3, 0, 3, T, 4, cap, whole, det, ws, nbytes)
    _check("g [0, 3)", mode, whole, refs)
    # ranges: [0, 1) leaves levels 1 and 2 untouched (stale bytes stay); with [1, 3) it equals the single call
    stale = _tables(ctx, 3, T, stale=True)
    _owner(ctx, 3, 0, 1, T, 4, cap, stale, det | OVERWRITE, ws, nbytes)
    _check("g [0, 1) overwrite", mode, stale, refs, levels=(0,))
    for lvl in (1, 2):
        assert bool((stale[lvl].view(torch.uint8) == 0xA5).all()), f"level {lvl} outside the range was written"
    parts = _tables(ctx, 3, T)
    _owner(ctx, 3, 0, 1, T, 4, cap, parts, det, ws, nbytes)
    assert not bool(parts[1].any()) and not bool(parts[2].any())
    _owner(ctx, 3, 1, 3, T, 4, cap, parts, det, ws, nbytes)
    _check("g [0, 1) + [1, 3)", mode, parts, refs)
    if det:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(whole, parts))
    # accumulate: a second pass adds onto the first. Each pass is within the bar of the reference and the second
    # rounds fp32(first + sum) once more: twice the bar plus 2^-24 of the result
    _owner(ctx, 3, 0, 3, T, 4, cap, parts, det, ws, nbytes)
    twice = [(2 * w, s, n, M) for w, s, n, M in refs]
    _check("g accumulate twice", mode, parts, twice,
           bound=lambda m, s, n, M: 2 * _bound(m, s, n, M) + 2.0 ** -24 * 2 * s)
    # overwrite on stale tables: rows without a term become +0 (checked bit for bit by _check), the others the sum
    stale = _tables(ctx, 3, T, stale=True)
    _owner(ctx, 3, 0, 3, T, 4, cap, stale, det | OVERWRITE, ws, nbytes)
    _check("g overwrite", mode, stale, refs)
    if det:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(whole, stale))
    stale = _tables(ctx, 3, T, stale=True)
    _owner(ctx, 3, 0, 3, T, 0, cap, stale, det | OVERWRITE, ws, nbytes)         # no chunks: all zeros
    assert not any(bool(_bits(t).any()) for t in stale)


def test_h_edge_coordinates(ctx):
    """Grid vertices (weights exactly 0 and 1), box bounds, outside points, zero, subnormal, tiny and huge
    coordinates: the cut of the forward's edge-point set that test_hash_bwd_ref_cpu.py describes."""
    res_all = ctx.oracle.level_resolutions(16, 1024).numpy()
    x, _ = hb.edge_points_bwd(ctx.oracle, res_all, LEVELS, 8 * ctx.C + 37)
    _all_modes(ctx, "h edge coordinates", x, hb.random_grads(2, len(x), seed=61))


@pytest.mark.parametrize("mode", ["default", "deterministic"])
def test_i_bin_rows(ctx, mode):
    """nerf_hash_encode_bwd_bin_rows directly: a row map into a larger buffer, a second gradient with its own row map
    and level-major strides, and a device count that cuts the points short (P + 5 clamps to P)."""
    _lib, C, det, T, n = ctx.L, ctx.C, int(mode == "deterministic"), 19, 2
    P, R = 2 * C + 1, 3 * C
    rng = np.random.RandomState(81)
    xbuf = hb.random_points(R, seed=82)
    d1 = hb.random_grads(n, R, seed=83).transpose(1, 0, 2).copy()                # [R, L, 2]: strides (2L, 2)
    d2 = hb.random_grads(n, R, seed=84)                                          # [L, R, 2]: strides (2, 2R)
    rows, rows2 = rng.permutation(R)[:P].astype(np.int32), rng.permutation(R)[:P].astype(np.int32)
    xt, d1t, d2t, rt, r2t = (_dev(ctx, a) for a in (xbuf, d1, d2, rows, rows2))
    res = _lib.host_f32(LEVELS)
    cap = (P + C - 1) // C
    ws, nbytes = _workspace(ctx, n, T, C * cap, det)
    zero = np.zeros((n, P, 2), np.float32)
    g1, g2 = d1[rows].transpose(1, 0, 2), d2[:, rows2]                           # [L, P, 2] each
    for count in (0, 1, C, C + 1, P, P + 5):
        ct = torch.tensor([count], dtype=torch.int32, device=ctx.gpu)
        live = min(count, P)
        for name, use1, use2 in (("dfeat", True, False), ("dfeat2", False, True), ("both", True, True)):
            d = ((g1 if use1 else zero) + (g2 if use2 else zero)).astype(np.float32)      # summed in fp32, as the kernel
            refs = _refs(ctx, xbuf[rows[:live]], d[:, :live], LEVELS, T)
            ws.fill_(0xA5)
            _lib.call("nerf_hash_encode_bwd_bin_rows", _lib.ptr(xt), _lib.ptr(rt, dtype=torch.int32),
                      _lib.ptr(ct, dtype=torch.int32), P, ctx.bmin, ctx.bmax, res, n, T,
                      _lib.ptr(d1t) if use1 else None, 2 * n, 2, _lib.ptr(d2t) if use2 else None,
                      _lib.ptr(r2t, dtype=torch.int32) if use2 else None, 2, 2 * R, 0, cap, det,
                      _lib.ptr(ws, dtype=torch.uint8), nbytes, _lib.stream())
            g = _tables(ctx, n, T)
            _owner(ctx, n, 0, n, T, cap, cap, g, det, ws, nbytes)
            _check(f"i rows count={count} {name}", mode, g, refs)


def test_j_dynamic_range(ctx):
    """Sixteen clusters whose gradients span 18 decades inside one level: the deterministic owner's fixed-point
    scale comes from the largest entry, and the smallest cluster must survive it (count * 2^-70 * M)."""
    P = ctx.C + 1
    x, cl = hb.cluster_points(P)
    d = hb.random_grads(2, P, seed=5) * (10.0 ** (-12 + 1.2 * cl))[None, :, None].astype(np.float32)
    _all_modes(ctx, "j 18 decades", x, d)
