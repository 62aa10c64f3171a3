"""What the hash-backward value tests share (test_hash_bwd_ref_cpu.py, test_gpu_hash_bwd_shapes.py, and the two
older gradient checks in test_gpu_parity.py / test_gpu_determinism.py): the float64 scatter reference of
nerf_hash_encode_bwd_* and seeded builders of the point sets at which the bin and owner passes of
csrc/hashgrid.hip take their other paths. No test and no fixture lives here.

Every builder returns NumPy fp32 (and, where a case needs it, a small table describing what it built); the
property a GPU case relies on is asserted on the reference alone in test_hash_bwd_ref_cpu.py.
"""
import numpy as np
import torch

from tables import blender_bbox

WAVE = 64          # lanes of a wave: the run merge of bwd_bin_block works inside one
ROW = 16           # lanes of a DPP row: wave_segmented_inclusive_sum's short variants stay inside one


# ---------------------------------------------------------------- the reference
def scatter_ref(oracle, xyz, dfeat_level, bmin, bmax, res, log2_T, drop_zero=True):
    """One level's table gradient as a float64 scatter: (want [T, 2], scale [T, 2], count [T], idx [n, 8]).

    Corners and fp32 weights come from oracle.voxel_corners (utils.py:95-117), the products and index_add_ run
    in float64. scale is the scatter of |terms|, count the number of terms per row (8 per scattered point, the
    zero-weight ones included). Points whose gradient is all zero add nothing and are left out before the
    scatter when drop_zero is set (exact); idx holds the hashed corners of the n points that were scattered.
    """
    xyz = torch.as_tensor(xyz, dtype=torch.float32)
    g = torch.as_tensor(dfeat_level, dtype=torch.float32)
    bmin, bmax = torch.as_tensor(bmin), torch.as_tensor(bmax)
    res = torch.as_tensor(res, dtype=torch.float32)
    if drop_zero:
        live = (g != 0).any(-1)
        if not bool(live.all()):
            xyz, g = xyz[live], g[live]
    T = 1 << log2_T
    vmin, vmax, idx, _ = oracle.voxel_corners(xyz, bmin, bmax, res, log2_T)
    w = ((xyz - vmin) / (vmax - vmin)).double()
    wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
    gl = g.double()
    contrib = []
    for c in range(8):
        i, j, k = (c >> 2) & 1, (c >> 1) & 1, c & 1
        contrib.append(gl * ((wz if k else 1 - wz) * (wy if j else 1 - wy) * (wx if i else 1 - wx)))
    contrib = torch.stack(contrib, 1).reshape(-1, 2)
    flat = idx.reshape(-1)
    want = torch.zeros(T, 2, dtype=torch.float64).index_add_(0, flat, contrib)
    scale = torch.zeros(T, 2, dtype=torch.float64).index_add_(0, flat, contrib.abs())
    count = torch.bincount(flat, minlength=T)
    return want, scale, count, idx


def largest_term(oracle, xyz, dfeat_level, bmin, bmax, res):
    """The level's largest |term| in float64: a lower bound of the largest |entry| the bin pass records (an entry
    is a term or the sum of a merged run), so the deterministic bar built on it is the stricter one."""
    xyz = torch.as_tensor(xyz, dtype=torch.float32)
    g = torch.as_tensor(dfeat_level, dtype=torch.float32)
    live = (g != 0).any(-1)
    xyz, g = xyz[live], g[live]
    if xyz.shape[0] == 0:
        return 0.0
    vmin, vmax, _, _ = oracle.voxel_corners(xyz, torch.as_tensor(bmin), torch.as_tensor(bmax),
                                            torch.as_tensor(res, dtype=torch.float32), 19)
    w = ((xyz - vmin) / (vmax - vmin)).double()
    ww = torch.maximum(w.abs(), (1 - w).abs()).prod(-1, keepdim=True)
    return float((g.double().abs() * ww).max())


def cells(oracle, xyz, res):
    """Voxel base of every point at one level ([P, 3] int64), from the oracle (the key of the bin pass's run merge)."""
    lo, hi = blender_bbox()
    xyz = torch.as_tensor(xyz, dtype=torch.float32)
    bmin, bmax = torch.from_numpy(lo), torch.from_numpy(hi)
    r = torch.as_tensor(res, dtype=torch.float32)
    xc = torch.clamp(xyz, min=bmin, max=bmax)
    return torch.floor((xc - bmin) / ((bmax - bmin) / r)).long().numpy()


def runs_of(base):
    """(start, length) of every maximal run of consecutive equal voxel bases, as the merge sees them WITHOUT the
    wave boundary (a run that crosses a wave is one row here)."""
    base = np.asarray(base)
    head = np.ones(len(base), bool)
    head[1:] = (base[1:] != base[:-1]).any(-1)
    start = np.flatnonzero(head)
    return np.stack([start, np.diff(np.append(start, len(base)))], 1)


def wave_scan_variants(base, n_valid=None):
    """Per wave of 64 points, the scan wave_segmented_inclusive_sum picks (csrc/common.h): 0 = no scan (every run of
    length 1), 1 / 2 = the one- / two-step scan, 4 = the full scan with row carries. From the voxel bases alone."""
    base = np.asarray(base)
    P = len(base) if n_valid is None else n_valid
    out = []
    for w0 in range(0, P, WAVE):
        b = base[w0:min(w0 + WAVE, P)]
        n = len(b)
        head = np.ones(WAVE, bool)
        head[1:n] = (b[1:] != b[:-1]).any(-1)
        head[n + 1:] = False                       # invalid lanes (x = y = z = 0, key bit 31) form one run
        lane = np.arange(WAVE)
        start = np.maximum.accumulate(np.where(head, lane, 0))
        span = lane - start
        if head.all():
            out.append(0)
        elif (start < (lane & ~(ROW - 1))).any():
            out.append(4)
        elif (span >= 4).any():
            out.append(4)
        elif (span >= 2).any():
            out.append(2)
        else:
            out.append(1)
    return np.asarray(out)


# ---------------------------------------------------------------- point sets
def random_points(P, seed, outside=0.1, margin=0.1):
    """Uniform points in the box, a fraction `outside` of them pushed out of it by up to `margin` on one axis."""
    lo, hi = blender_bbox()
    rng = np.random.RandomState(seed)
    x = (lo + (hi - lo) * rng.rand(P, 3)).astype(np.float32)
    out = np.flatnonzero(rng.rand(P) < outside)
    ax = rng.randint(0, 3, len(out))
    d = (margin * (0.05 + 0.95 * rng.rand(len(out)))).astype(np.float32)
    up = rng.rand(len(out)) < 0.5
    x[out, ax] = np.where(up, hi[ax] + d, lo[ax] - d).astype(np.float32)
    return x


def random_grads(L, P, seed, decades=0.0):
    """[L, P, 2] gradients with mixed signs (optionally spread over `decades` decades)."""
    rng = np.random.RandomState(seed)
    g = rng.randn(L, P, 2)
    if decades:
        g = g * 10.0 ** rng.uniform(-decades, 0, (L, P, 1))
    return g.astype(np.float32)


def _cell_point(rng, k, res=16):
    """A point well inside coarse cell number k (mod res^3) of the res^3 grid: consecutive k never share a voxel at
    this level or at any finer one."""
    lo, hi = blender_bbox()
    k = k % (res ** 3)
    ijk = np.array([k % res, (k // res) % res, k // (res * res)], np.float64)
    u = 0.1 + 0.8 * rng.rand(3)
    return (lo + (hi - lo) * ((ijk + u) / res)).astype(np.float32)


RUN_LENGTHS = tuple(range(1, 71)) + (128, 130)    # then C + 1
RUN_SHIFT = 13


def run_points(C, seed=7):
    """Runs of consecutive copies of one point: (xyz, table), table rows (part, start, length).

    part 0: lengths 1..70, 128, 130, C + 1, from point 0 (length n starts at point n(n-1)/2).
    part 1: the same lengths from the next point whose lane is RUN_SHIFT (single points pad up to it), so the runs
            start at other lanes and cross lanes 15/16, 31/32, 47/48 and 63/0 elsewhere.
    part 2: from the next wave boundary, one wave of pairs and singles (the one-step scan), one of runs up to four
            (the two-step scan) and one of triples and pairs, every run inside one 16-lane row.
    Every run has its own coarse cell, so neighbouring runs never merge at any level.
    """
    rng = np.random.RandomState(seed)
    pts, table = [], []
    k = [0]

    def add(part, n):
        table.append((part, sum(len(p) for p in pts), n))
        pts.append(np.repeat(_cell_point(rng, 37 * k[0] + 5)[None], n, 0))
        k[0] += 1

    def pad_to(lane, modulo):
        while sum(len(p) for p in pts) % modulo != lane:
            add(-1, 1)

    lengths = RUN_LENGTHS + (C + 1,)
    for n in lengths:
        add(0, n)
    pad_to(RUN_SHIFT, WAVE)
    for n in lengths:
        add(1, n)
    pad_to(0, WAVE)
    for row in ((2, 2, 2, 1, 2, 2, 2, 1, 2),) * 4 + ((4, 3, 2, 1, 4, 2),) * 4 + ((3, 3, 2, 3, 3, 2),) * 4:
        assert sum(row) == ROW
        for n in row:
            add(2, n)
    return np.concatenate(pts).astype(np.float32), np.asarray(table, np.int64)


def identical_points(n, seed=3):
    rng = np.random.RandomState(seed)
    return np.repeat(_cell_point(rng, 1234)[None], n, 0).astype(np.float32)


def one_cell_points(n, res=1024, seed=4):
    """n different points inside one cell of the res^3 grid (so one cell of every coarser level of a 16..res
    pyramid whose cells nest; asserted for the levels used in the CPU test)."""
    lo, hi = blender_bbox()
    rng = np.random.RandomState(seed)
    ijk = np.array([517, 300, 771], np.float64) % res
    u = 0.05 + 0.9 * rng.rand(n, 3)
    x = (lo.astype(np.float64) + (hi.astype(np.float64) - lo) * ((ijk + u) / res)).astype(np.float32)
    assert len(np.unique(x, axis=0)) == n
    return x


ONE_SLICE = {"default": (14, 13), "deterministic": (13, 12)}   # mode -> (log2_T, owner slice log2); see one_slice_points


def one_slice_points(oracle, n, log2_T, slice_log2, res=16, seed=5):
    """n points whose 8 corners all hash into ONE owner slice of 2^slice_log2 rows at the res^3 level, consecutive
    points in different cells (no run merge: the chunk keeps all 8n entries, in one segment). -> (xyz, owner)

    The corners (y, z) and (y + 1, z) of a cell differ by y * 2654435761 ^ (y + 1) * 2654435761; the prime's low
    bits step by several slices per unit of y, and a search with the oracle's hash over the 16^3 cells finds such
    cells only where the table has TWO owner slices: log2_T = 14 for the default mode's 2^13-row slices, log2_T = 13
    for the deterministic mode's 2^12-row slices (ONE_SLICE; none at 2^15 .. 2^20 rows, which the CPU test shows for
    2^19). So each mode runs the case at its own table size and point set.
    """
    lo, hi = blender_bbox()
    corners = oracle.corner_offsets()
    g = torch.stack(torch.meshgrid(*[torch.arange(res)] * 3, indexing="ij"), -1).reshape(-1, 3)
    sl = oracle.spatial_hash(g[:, None, :] + corners[None], log2_T) >> slice_log2          # [res^3, 8]
    same = (sl == sl[:, :1]).all(1)
    owners, counts = torch.unique(sl[same, 0], return_counts=True)
    owner = int(owners[counts.argmax()]) if len(owners) else -1
    good = g[same & (sl[:, 0] == owner)].numpy()
    if len(good) < 2:
        raise AssertionError(f"no two cells of the {res}^3 level keep their corners in one slice at log2_T {log2_T}")
    rng = np.random.RandomState(seed)
    pick = np.arange(n) % len(good)                     # consecutive points: different cells
    u = 0.1 + 0.8 * rng.rand(n, 3)
    x = (lo.astype(np.float64) + (hi.astype(np.float64) - lo) * ((good[pick] + u) / res)).astype(np.float32)
    return x, owner


def vertex_points(n, res=1024, seed=6):
    """n points exactly on vertices of the res^3 grid on all three axes: base * cell + lo in fp32, the kernels' vmin."""
    lo, hi = blender_bbox()
    rng = np.random.RandomState(seed)
    cell = ((hi - lo) / np.float32(res)).astype(np.float32)
    k = np.floor(rng.rand(n, 3) * res).astype(np.float32)
    return (k * cell + lo).astype(np.float32)


def cluster_points(n, n_clusters=16, seed=8):
    """n points in n_clusters clusters, each cluster inside its own coarse cell (cluster of point p: p % n_clusters,
    so every wave holds all of them and no two neighbours merge)."""
    rng = np.random.RandomState(seed)
    x = np.stack([_cell_point(rng, 211 * (p % n_clusters) + 9) for p in range(n)])
    return x.astype(np.float32), np.arange(n) % n_clusters


EDGE_SPECIALS = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, 1e-45, 3e-22, 1e30, -1e30, 1e-6, -1e-6], np.float32)


def edge_points(level_res, n=1 << 20, seed=11):
    """Where the voxel math is most fragile: points exactly on grid vertices of every level, on and outside the box
    bounds, zero, subnormal, tiny and huge coordinates, spread over waves and in runs (the set of
    test_hash_encode_edge_points_vs_c_oracle, value for value)."""
    lo, hi = blender_bbox()
    rng = np.random.RandomState(seed)
    x = (lo - 0.3 + (hi - lo + 0.6) * rng.rand(n, 3)).astype(np.float32)
    res = np.asarray(level_res, np.float32)
    cell = ((hi.astype(np.float32) - lo.astype(np.float32))[None, :] / res[:, None]).astype(np.float32)   # [L, 3]
    # grid vertices: base * cell + lo in fp32 (the kernels' vmin), every level, random axes
    m = n // 4
    lv = rng.randint(0, len(res), m)
    k = np.floor(rng.rand(m, 3) * res[lv][:, None]).astype(np.float32)
    verts = (k * cell[lv] + lo.astype(np.float32)).astype(np.float32)
    axes = rng.rand(m, 3) < 0.6
    x[:m][axes] = verts[axes]
    specials = EDGE_SPECIALS
    sel = rng.rand(n, 3) < 0.002                                   # scattered: one wave in ~10
    x[sel] = rng.choice(specials, int(sel.sum()))
    for a in range(3):                                             # exact box bounds
        b = rng.rand(n) < 0.01
        x[b, a] = np.where(rng.rand(int(b.sum())) < 0.5, lo[a], hi[a]).astype(np.float32)
    x[n - 4096:n - 2048, 1] = 0.0                                   # a run of zero coordinates
    x[n - 2048:, 2] = 1e-38
    perm = rng.permutation(n - 4096)
    x[:n - 4096] = x[perm]
    return x


def edge_points_bwd(oracle, level_res_all, levels, n_points):
    """The backward's cut of edge_points: a stride through the scattered part (so the scattered specials, rare in
    any prefix, are all there) plus 64 points of each trailing run, n_points in all; then without the points whose
    fp32 corner weights are not all finite at `levels` in the oracle. Returns (xyz, n_dropped)."""
    x = edge_points(level_res_all)
    n = len(x)
    body = n - 4096
    is_special = np.isin(x[:body], EDGE_SPECIALS[2:]).any(1) | (np.abs(x[:body]) >= 1e29).any(1)
    sp = np.flatnonzero(is_special)
    sp = sp[:: max(1, len(sp) // 512)][:512]
    rest = n_points - 128 - len(sp)
    plain = np.setdiff1d(np.arange(0, body, body // (rest + 600)), sp)[:rest]
    order = np.sort(np.concatenate([sp, plain]))
    cut = np.concatenate([x[order], x[n - 4096:n - 4096 + 64], x[n - 64:]])
    assert len(cut) == n_points
    lo, hi = blender_bbox()
    ok = np.ones(len(cut), bool)
    xt = torch.from_numpy(cut)
    for r in levels:
        vmin, vmax, _, _ = oracle.voxel_corners(xt, torch.from_numpy(lo), torch.from_numpy(hi),
                                                torch.tensor(r, dtype=torch.float32), 19)
        w = (xt - vmin) / (vmax - vmin)
        ow = 1 - w
        for c in range(8):
            i, j, kk = (c >> 2) & 1, (c >> 1) & 1, c & 1
            p = (w[:, 2] if kk else ow[:, 2]) * (w[:, 1] if j else ow[:, 1]) * (w[:, 0] if i else ow[:, 0])
            ok &= torch.isfinite(p).numpy()
    return cut[ok], int((~ok).sum())


def window_grads(P, C, L, seed=9):
    """Case (e)'s gradients, level-major [L, P, 2]: zero except on points [0, 700), the points of chunks 4095..4097
    with 5 either side, the last 600 points and every 97th point. Returns (dfeat, live point indices)."""
    rng = np.random.RandomState(seed)
    live = np.zeros(P, bool)
    live[:700] = True
    live[4095 * C - 5:min(4098 * C + 5, P)] = True
    live[P - 600:] = True
    live[::97] = True
    idx = np.flatnonzero(live)
    d = np.zeros((L, P, 2), np.float32)
    d[:, idx] = rng.randn(L, len(idx), 2).astype(np.float32)
    return d, idx
