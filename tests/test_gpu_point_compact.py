"""The point compaction of the forward-only render paths (csrc/sparse_points.hip over csrc/compact_common.h):
nerf_occ_compact and nerf_ert_compact called directly, against NumPy, needs an MI355X.

The cell rule, the masks and the drivers of the two entries are those of forward_only.py. Points are
uniform in the scene box scaled by 1.3 about its centre (45 % inside), the grid is the half-full random mask
at resolution 5, alive flags are set with probability 0.6: every case keeps between 5 % and 95 % of its
candidates, which each test asserts on the CPU before anything runs on the GPU (sizes below 64 excepted).
Sizes: the wave (64), thread-block (256) and compaction-block (4096) edges, slabs whose candidates leave the
first compaction block, and 258 blocks, from which on a thread of the scatter kernel sums more than one block
count.
"""
import numpy as np
import pytest
import torch

from forward_only import bits_equal, np_cells, random_mask, run_compact, run_occ_compact
from tables import blender_bbox

pytestmark = pytest.mark.gpu

RES = 5


def make_inputs(n_rays, n_points, seed):
    """Host inputs of one case: points [n_points, 3], unit view directions [n_rays, 3], SH records [n_rays, 40],
    and per point "inside the box" and "inside and in an occupied cell" of the NumPy cell rule."""
    lo, hi = blender_bbox()
    rng = np.random.default_rng(seed)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pts = (mid + (rng.random((n_points, 3)) * 2 - 1) * 1.3 * half).astype(np.float32)
    dirs = rng.standard_normal((n_rays, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    records = rng.standard_normal((n_rays, 40)).astype(np.float32)
    cid, inside = np_cells(pts, lo, hi, RES)
    return dict(lo=lo, hi=hi, rng=rng, pts=pts, dirs=dirs, records=records, inside=inside,
                occupied=inside & random_mask(RES).reshape(-1)[cid])


def assert_fraction(kept, cand):
    if int(cand.sum()) >= 64:
        assert 0.05 < kept.sum() / cand.sum() < 0.95, "inputs: the kept fraction must lie strictly inside (5 %, 95 %)"


def random_grid(nerf, gpu, h):
    grid = nerf.OccupancyGrid((torch.from_numpy(h["lo"]), torch.from_numpy(h["hi"])), resolution=RES, device=gpu)
    grid.set_mask(random_mask(RES))
    return grid


def check_outputs(got, raw, h, kept, cand, samples_per_ray, want_sh_rows, what):
    """rows ascending = flatnonzero(kept); pts_c, sh_c bit-equal; raw zero exactly at the candidates not kept."""
    rows, pts_c, sh_c = got
    want = np.flatnonzero(kept).astype(np.int32)
    assert np.array_equal(rows.cpu().numpy(), want), what
    assert np.array_equal(pts_c.cpu().numpy().view(np.int32), h["pts"][want].view(np.int32)), what
    ray = torch.from_numpy(want // samples_per_ray).to(raw.device).long()
    assert bits_equal(sh_c, want_sh_rows[ray]), what
    zeroed = torch.from_numpy(cand & ~kept).to(raw.device)
    assert bool((raw[zeroed].view(torch.int32) == 0).all()) and bool((raw[~zeroed] == 7.0).all()), what


def sh_sources(nerf, gpu, h):
    """(name, SH records or None, view directions or None, the [R, 16] rows the kept points must receive)."""
    d_dirs, d_rec = torch.from_numpy(h["dirs"]).to(gpu), torch.from_numpy(h["records"]).to(gpu)
    return (("records", d_rec, None, d_rec[:, :16]), ("viewdirs", None, d_dirs, nerf.SHEncoder()(d_dirs)))


# ---------------------------------------------------------------- 1. small sizes, a partial last ray
@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 255, 257, 4095, 4096, 4097, 8193])
def test_occ_compact_small_sizes(nerf, gpu, n_points):
    import indoor_nerf_amd._lib as L
    S = 7
    h = make_inputs(-(-n_points // S), n_points, 100 + n_points)
    kept, cand = h["occupied"], np.ones(n_points, bool)
    assert_fraction(kept, cand)
    grid, d_pts = random_grid(nerf, gpu, h), torch.from_numpy(h["pts"]).to(gpu)
    for name, rec, dirs, want_sh in sh_sources(nerf, gpu, h):
        raw = torch.full((n_points, 4), 7.0, device=gpu)
        got = run_occ_compact(L, gpu, d_pts, S, rec, dirs, h["lo"], h["hi"], grid, raw)
        check_outputs(got, raw, h, kept, cand, S, want_sh, f"{n_points} points, SH from {name}")


# ---------------------------------------------------------------- 2. the two entries agree
def test_occ_entry_equals_one_slab_ert_entry(nerf, gpu):
    import indoor_nerf_amd._lib as L
    R, S = 65, 64
    h = make_inputs(R, R * S, 2)
    assert_fraction(h["occupied"], np.ones(R * S, bool))
    grid, d_pts = random_grid(nerf, gpu, h), torch.from_numpy(h["pts"]).to(gpu)
    for name, rec, dirs, _ in sh_sources(nerf, gpu, h):
        raw_o, raw_e = torch.full((R * S, 4), 7.0, device=gpu), torch.full((R * S, 4), 7.0, device=gpu)
        occ = run_occ_compact(L, gpu, d_pts, S, rec, dirs, h["lo"], h["hi"], grid, raw_o)
        ert = run_compact(L, gpu, d_pts, R, S, 0, S, None, rec, dirs, h["lo"], h["hi"], grid, raw_e)
        assert occ[0].numel() == ert[0].numel() == int(h["occupied"].sum()), name      # count
        assert torch.equal(occ[0], ert[0]) and bits_equal(occ[1], ert[1]) and bits_equal(occ[2], ert[2]), name
        assert bits_equal(raw_o, raw_e), name


# ---------------------------------------------------------------- 3. slabs that leave the first block
@pytest.mark.parametrize("with_grid", [False, True])
@pytest.mark.parametrize("R", [257, 513])
def test_ert_compact_slab_past_one_block(nerf, gpu, R, with_grid):
    import indoor_nerf_amd._lib as L
    S, s0, s1 = 64, 24, 40
    h = make_inputs(R, R * S, 3 * R + with_grid)
    alive = (h["rng"].random(R) < 0.6).astype(np.uint8)
    cand = np.zeros((R, S), bool)
    cand[:, s0:s1] = True
    cand = cand.reshape(-1)
    kept = cand & np.repeat(alive.astype(bool), S) & (h["occupied"] if with_grid else h["inside"])
    assert_fraction(kept, cand)
    grid = random_grid(nerf, gpu, h) if with_grid else None
    d_pts, d_alive = torch.from_numpy(h["pts"]).to(gpu), torch.from_numpy(alive).to(gpu)
    for name, rec, dirs, want_sh in sh_sources(nerf, gpu, h):
        raw = torch.full((R * S, 4), 7.0, device=gpu)
        got = run_compact(L, gpu, d_pts, R, S, s0, s1, d_alive, rec, dirs, h["lo"], h["hi"], grid, raw)
        check_outputs(got, raw, h, kept, cand, S, want_sh, f"R {R}, grid {with_grid}, SH from {name}")


# ---------------------------------------------------------------- 4. the block offset's strided loop
def test_258_blocks_sum_two_counts_per_thread(nerf, gpu):
    """1 052 736 candidates = 258 compaction blocks: thread 0 of block 257 adds block_counts[0] and [256]."""
    import indoor_nerf_amd._lib as L
    R, S = 16449, 64
    assert -(-R * S // 4096) == 258
    h = make_inputs(R, R * S, 4)
    assert_fraction(h["occupied"], np.ones(R * S, bool))
    want = np.flatnonzero(h["occupied"]).astype(np.int32)
    grid, d_pts = random_grid(nerf, gpu, h), torch.from_numpy(h["pts"]).to(gpu)
    d_rec = torch.from_numpy(h["records"]).to(gpu)
    raw = torch.empty(R * S, 4, device=gpu)
    rows = run_compact(L, gpu, d_pts, R, S, 0, S, None, d_rec, None, h["lo"], h["hi"], grid, raw)[0]
    assert rows.numel() == want.size and np.array_equal(rows.cpu().numpy(), want), "nerf_ert_compact"
    rows = run_occ_compact(L, gpu, d_pts, S, d_rec, None, h["lo"], h["hi"], grid, raw)[0]
    assert rows.numel() == want.size and np.array_equal(rows.cpu().numpy(), want), "nerf_occ_compact"
