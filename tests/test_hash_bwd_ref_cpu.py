"""The hash backward's float64 reference checked against itself, and every point-set builder of hash_bwd_ref.py
checked for the property its GPU case relies on (test_gpu_hash_bwd_shapes.py) — on the reference alone, so a case
is known to exercise what it claims before a GPU sees it. Needs no GPU.
"""
import numpy as np
import pytest
import torch

import hash_bwd_ref as hb
from tables import blender_bbox

C = 512            # NERF_HASH_CHUNK_POINTS (include/nerf_hip.h); the GPU test asserts the library agrees
LEVELS = (16.0, 1024.0)


def _box():
    lo, hi = blender_bbox()
    return torch.from_numpy(lo), torch.from_numpy(hi)


@pytest.mark.parametrize("log2_T", [12, 19])
def test_scatter_ref_equals_fp64_autograd(oracle, log2_T):
    """scatter_ref against float64 autograd on double tables: F.embedding's backward and trilinear()'s blend order,
    independent of scatter_ref's corner loop.

    oracle.hash_encode itself forms 1 - w in fp32 (hash_encoding.py:56-80 on fp32 points) where scatter_ref, like the
    two older tests, forms it in float64 from the fp32 w: its autograd gradient differs from scatter_ref by that
    rounding, one 2^-24 per factor, and is held to 4 * 2^-24 of the sum of |terms|. With the same hash_encode steps
    (voxel_corners, embedding, trilinear) fed the fp32 weights as float64 values, both sum the same products in
    float64 in different orders: 1e-12 of the sum of |terms|."""
    bmin, bmax = _box()
    P = 2000
    x = torch.from_numpy(hb.random_points(P, seed=log2_T))
    d = torch.from_numpy(hb.random_grads(2, P, seed=log2_T + 1))
    dd = d.permute(1, 0, 2).reshape(P, 4).double()
    res = [torch.tensor(r) for r in LEVELS]
    tabs = [torch.zeros(1 << log2_T, 2, dtype=torch.float64, requires_grad=True) for _ in LEVELS]
    feat, _ = oracle.hash_encode(x, tabs, bmin, bmax, res, log2_T=log2_T)
    assert feat.dtype == torch.float64
    (feat * dd).sum().backward()
    tabs64 = [torch.zeros(1 << log2_T, 2, dtype=torch.float64, requires_grad=True) for _ in LEVELS]
    outs = []
    for lvl in range(2):
        vmin, vmax, idx, _ = oracle.voxel_corners(x, bmin, bmax, res[lvl], log2_T)
        w = ((x - vmin) / (vmax - vmin)).double()                 # the fp32 weights, as float64 values
        e = torch.nn.functional.embedding(idx, tabs64[lvl])
        outs.append(oracle.trilinear(w, torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64), e))
    (torch.cat(outs, -1) * dd).sum().backward()
    for lvl in range(2):
        want, scale, count, idx = hb.scatter_ref(oracle, x, d[lvl], bmin, bmax, res[lvl], log2_T)
        assert idx.shape == (P, 8) and int(count.sum()) == 8 * P
        err = (tabs64[lvl].grad - want).abs()
        assert bool((err <= 1e-12 * scale).all()), f"level {lvl}: max {float((err / scale.clamp_min(1e-300)).max()):.3e}"
        err = (tabs[lvl].grad - want).abs()
        assert bool((err <= 4 * 2.0 ** -24 * scale).all()), f"level {lvl}: {float((err / scale.clamp_min(1e-300)).max()):.3e}"
        assert bool((want[count == 0] == 0).all()) and bool((scale[count > 0].sum(-1) >= 0).all())
        # leaving out zero-gradient points is exact
        d0 = d[lvl].clone()
        d0[::3] = 0.0
        a = hb.scatter_ref(oracle, x, d0, bmin, bmax, res[lvl], log2_T)
        b = hb.scatter_ref(oracle, x, d0, bmin, bmax, res[lvl], log2_T, drop_zero=False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert a[3].shape[0] == P - len(range(0, P, 3)) and b[3].shape[0] == P


def test_random_points_leave_the_box():
    lo, hi = blender_bbox()
    x = hb.random_points(2 * C + 1, seed=1)
    out = ((x < lo) | (x > hi)).any(1)
    assert 0.05 < out.mean() < 0.2
    d = np.maximum(lo - x, x - hi).max(1)[out]
    assert d.max() <= 0.1 + 1e-6 and d.min() > 0
    assert len(hb.random_points(1, seed=2)) == 1


def test_run_points_runs_and_lanes(oracle):
    """(b): the runs the reference sees are the runs that were laid out, at both levels; the named lengths start at
    the intended lanes in both parts; some row collects a whole chunk; and part 2 gives the two short scans."""
    bmin, bmax = _box()
    x, table = hb.run_points(C)
    P = len(x)
    for r in LEVELS:
        base = hb.cells(oracle, x, r)
        np.testing.assert_array_equal(hb.runs_of(base), table[:, 1:])
    lane_of = {n: (n * (n - 1) // 2) % 64 for n in (2, 3, 4, 5, 17, 64)}
    assert lane_of == {2: 1, 3: 3, 4: 6, 5: 10, 17: 8, 64: 32}
    for part, shift in ((0, 0), (1, hb.RUN_SHIFT)):
        rows = table[table[:, 0] == part]
        assert list(rows[:, 2]) == list(hb.RUN_LENGTHS) + [C + 1]
        for n, lane in lane_of.items():
            (start,) = rows[rows[:, 2] == n][:, 1]
            assert start % 64 == (lane + shift) % 64, (part, n)
    # the lane pairs 15/16, 31/32, 47/48 and 63/0 are each crossed by a run in both parts
    for part in (0, 1):
        rows = table[table[:, 0] == part]
        for edge in (16, 32, 48, 0):
            assert any(any((p % 64) == edge for p in range(s + 1, s + n)) for _, s, n in rows if n <= 70), (part, edge)
    assert any(s % 64 + n == 64 for _, s, n in table if n > 1)          # a run ending on lane 63
    # some run fills a whole wave (lanes 0..63 of one wave)
    assert any((s + 63) // 64 * 64 + 64 <= s + n for _, s, n in table)
    d = hb.random_grads(2, P, seed=3)
    assert (d > 0).any() and (d < 0).any()
    _, _, count, _ = hb.scatter_ref(oracle, x, d[0], bmin, bmax, LEVELS[0], 19)
    assert int(count.max()) >= C
    variants = hb.wave_scan_variants(hb.cells(oracle, x, LEVELS[1]))
    p2 = int(table[table[:, 0] == 2][0, 1])
    assert p2 % 64 == 0
    assert list(variants[p2 // 64:p2 // 64 + 3]) == [1, 2, 2]
    assert (variants[:p2 // 64] == 4).any()
    rows2 = table[table[:, 0] == 2]
    assert all(s % 16 + n <= 16 for _, s, n in rows2) and set(rows2[:, 2]) == {1, 2, 3, 4}


def test_one_cell_and_one_slice_sets(oracle):
    bmin, bmax = _box()
    # (i) identical points: one run per wave
    x = hb.identical_points(4097)
    assert len(np.unique(x, axis=0)) == 1
    # (ii) all different, one finest cell (hence one cell of the coarse level too)
    x = hb.one_cell_points(C)
    assert len(np.unique(x, axis=0)) == C
    for r in LEVELS:
        assert len(np.unique(hb.cells(oracle, x, r), axis=0)) == 1
    # (iii) one owner slice holds all 8C entries of the chunk at the res-16 level, each mode at its own table size
    for mode, (log2_T, slice_log2) in hb.ONE_SLICE.items():
        x, owner = hb.one_slice_points(oracle, C, log2_T, slice_log2)
        d = hb.random_grads(1, C, seed=4)[0]
        _, _, count, idx = hb.scatter_ref(oracle, x, d, bmin, bmax, 16.0, log2_T)
        assert log2_T - slice_log2 == 1                                        # two owner slices, one of them empty
        assert torch.unique(idx >> slice_log2).tolist() == [owner], mode
        assert (hb.wave_scan_variants(hb.cells(oracle, x, 16.0)) == 0).all()   # no merge: 8 entries per point
        vmin, vmax, _, _ = oracle.voxel_corners(torch.from_numpy(x), bmin, bmax, torch.tensor(16.0), log2_T)
        w = (torch.from_numpy(x) - vmin) / (vmax - vmin)
        assert bool(((w > 0) & (w < 1)).all()) and bool((torch.from_numpy(d) != 0).all())    # none dropped as zero
        assert int(count.sum()) == 8 * C == 4096                               # the segment word's count: 0x1000
    # the same search finds nothing at 2^19 rows, which is why the case runs at small tables
    for slice_log2 in (12, 13):
        with pytest.raises(AssertionError):
            hb.one_slice_points(oracle, C, 19, slice_log2)


def test_vertex_points_have_zero_weights(oracle):
    """(iv): on level-1024 vertices the oracle's weights are exactly 0 (or, where base * cell + lo rounds past the
    point, a cell below with weight 1): at most one corner in 8 is left per point."""
    bmin, bmax = _box()
    x = torch.from_numpy(hb.vertex_points(C))
    vmin, vmax, _, _ = oracle.voxel_corners(x, bmin, bmax, torch.tensor(1024.0), 19)
    w = (x - vmin) / (vmax - vmin)
    exact = (w == 0) | (w == 1)
    assert float(exact.float().mean()) > 0.9, float(exact.float().mean())
    nz = torch.ones(len(x), 8)
    for c in range(8):
        i, j, k = (c >> 2) & 1, (c >> 1) & 1, c & 1
        nz[:, c] = ((w[:, 2] if k else 1 - w[:, 2]) * (w[:, 1] if j else 1 - w[:, 1]) * (w[:, 0] if i else 1 - w[:, 0])) != 0
    assert float(nz.sum(1).mean()) < 2.0, float(nz.sum(1).mean())      # of 8 corners per point


def test_cluster_scales_can_fail_the_deterministic_bar(oracle):
    """(j): the smallest cluster's scale lies above the deterministic term count * 2^-70 * M of its rows, so losing
    that cluster to the fixed-point scale of the largest would fail the case."""
    bmin, bmax = _box()
    x, cl = hb.cluster_points(C + 1)
    d = hb.random_grads(2, C + 1, seed=5) * (10.0 ** (-12 + 1.2 * cl))[None, :, None].astype(np.float32)
    for lvl, r in enumerate(LEVELS):
        assert len(np.unique(hb.cells(oracle, x, r)[:16], axis=0)) == 16
        M = hb.largest_term(oracle, x, d[lvl], bmin, bmax, r)
        _, scale, count, idx = hb.scatter_ref(oracle, x, d[lvl], bmin, bmax, r, 19)
        own = cl == 0
        _, scale0, _, _ = hb.scatter_ref(oracle, x[own], d[lvl][own], bmin, bmax, r, 19)
        rows = torch.unique(idx[torch.from_numpy(own)])
        bar = 2e-6 * scale[rows] + 1e-30 + (count[rows].double() * 2.0 ** -70 * M)[:, None]
        # losing the cluster leaves an error of about its own sum of |terms| on its rows: above the bar on most
        assert float((scale0[rows] > 4 * bar).float().mean()) > 0.5, float((scale0[rows] / bar).median())
        assert float(scale.max()) / float(scale0.max()) > 1e15     # sixteen clusters span 18 decades


def test_edge_points_cut(oracle):
    """(h): the backward's cut of the forward's edge-point set keeps every kind of edge; the points whose fp32
    corner weights overflow in the oracle itself (two +-1e30 coordinates in one point: 1e32 * 1e32) are the only
    ones dropped."""
    lo, hi = blender_bbox()
    res_all = oracle.level_resolutions(16, 1024).numpy()
    n0 = 8 * C + 37
    x, dropped = hb.edge_points_bwd(oracle, res_all, LEVELS, n0)
    assert len(x) + dropped == n0
    full, _ = hb.edge_points_bwd(oracle, res_all, (), n0)
    huge = (np.abs(full) >= 1e29).sum(1)
    assert dropped == int((huge >= 2).sum()), (dropped, int((huge >= 2).sum()))
    print(f"edge cut: {len(x)} points, {dropped} dropped (two or more +-1e30 coordinates)")
    for s in hb.EDGE_SPECIALS:                                     # every special survives, +-1e30 included
        assert (x.view(np.uint32) == np.float32(s).view(np.uint32)).any(), s
    assert (x == lo).any() and (x == hi).any()
    assert ((x < lo) | (x > hi)).any(1).mean() > 0.05
    xt = torch.from_numpy(x)
    for r in LEVELS:
        vmin, vmax, _, _ = oracle.voxel_corners(xt, torch.from_numpy(lo), torch.from_numpy(hi), torch.tensor(r), 19)
        w = (xt - vmin) / (vmax - vmin)
        assert bool(torch.isfinite(w).all())
        assert int(((w == 0) | (w == 1)).sum()) > 20               # grid vertices of this level
    assert (hb.wave_scan_variants(hb.cells(oracle, x, 16.0)) != 0).any()


def test_window_grads_cover_both_owner_windows():
    """(e): more than the 4096 chunks of one owner window, every chunk with entries, whole chunks either side of
    the window boundary."""
    P = 4098 * C + 1
    d, idx = hb.window_grads(P, C, 2)
    live = np.zeros(P, bool)
    live[idx] = True
    assert d.shape == (2, P, 2) and not d[:, ~live].any() and (d[:, live] != 0).all()
    n_chunks = (P + C - 1) // C
    assert n_chunks == 4099 > 4 * 1024
    per_chunk = np.add.reduceat(live, np.arange(0, P, C))
    assert per_chunk.min() >= 1 and (per_chunk[4095:4098] == C).all() and per_chunk[4098] == 1
    assert 20000 < live.sum() < 30000
