"""Per-ray sample bounds from the occupancy grid (csrc/ray_span.hip, render(ray_bounds=grid)),
needs an MI355X.

The scene of forward_only.py (build_scene; perturb = 0).

The span kernel is held to three things: it is the same bits as np_span below (its rule restated in NumPy
fp32, vectorised over the rays), it is conservative against the cell rule applied to fp32 sample positions
o + d t (np_query), and it is tight against a brute-force fp64 reference (ref_interval). render(ray_bounds=)
is held to being the hand composition of existing pieces, bit for bit.
"""
import numpy as np
import pytest
import torch

from forward_only import (FAR, H, NEAR, W, ball_mask, bits_equal, build_scene, make_mask, np_query, random_mask,
                          scatter_back)

pytestmark = pytest.mark.gpu

f32 = np.float32
PAD_SCALE = f32(0.0625)      # pad = 2^-4 min_a cell_a / |d_a| (csrc/ray_span.hip)


# ---------------------------------------------------------------- the span rule in NumPy fp32
def np_axis(x, lo, hi, cell, res):
    """occ_common.h's occ_axis on one axis: (cell index, inside). fmin / fmax as fminf / fmaxf: a NaN clamps to lo."""
    xc = np.fmin(np.fmax(x, lo), hi)
    base = np.floor((xc - lo) / cell).astype(np.int64)
    return np.minimum(base, res - 1), x == np.maximum(np.minimum(x, hi), lo)


def np_pad(rays, lo, hi, res):
    rays, lo, hi = (np.asarray(a, f32) for a in (rays, lo, hi))
    cell = ((hi - lo) / f32(res)).astype(f32)
    with np.errstate(all="ignore"):
        p = np.where(rays[:, 3:6] != 0, cell / np.abs(rays[:, 3:6]), f32(np.inf)).astype(f32).min(-1)
    return np.where(np.isinf(p), f32(0), PAD_SCALE * p).astype(f32)


def np_span(rays, lo, hi, mask):
    """csrc/ray_span.hip's rule, operation by operation in fp32 (every array below is float32 or integer; NumPy
    does not fuse a multiply-add), all rays in lockstep: (hit bool [R], span float32 [R, 2])."""
    rays, lo, hi = (np.asarray(a, f32) for a in (rays, lo, hi))
    res = mask.shape[0]
    cell = ((hi - lo) / f32(res)).astype(f32)
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    R = rays.shape[0]
    ar = np.arange(R)
    t0, t1 = near.copy(), far.copy()
    pad, eps = np.full(R, np.inf, f32), np.zeros((R, 3), f32)
    idx, step = np.zeros((R, 3), np.int64), np.zeros((R, 3), np.int64)
    ok = np.ones(R, bool)

    def edge(a_cell, a_lo, a_hi, k):
        return np.where(k >= res, a_hi, k.astype(f32) * a_cell + a_lo).astype(f32)

    with np.errstate(all="ignore"):
        for a in range(3):
            oa, da = o[:, a], d[:, a]
            zero, nz = da == 0, (da > 0) | (da < 0)
            ia, ina = np_axis(oa, lo[a], hi[a], cell[a], res)
            idx[:, a] = np.where(zero, ia, 0)
            ok &= np.where(zero, ina, nz & (oa == oa))       # a NaN origin or direction is a miss
            ta, tb = (lo[a] - oa) / da, (hi[a] - oa) / da
            ta, tb = np.where(da < 0, tb, ta), np.where(da < 0, ta, tb)
            t0 = np.where(nz & (ta > t0), ta, t0)
            t1 = np.where(nz & (tb < t1), tb, t1)
            step[:, a] = np.where(da > 0, 1, np.where(da < 0, -1, 0))
            p = cell[a] / np.abs(da)
            pad = np.where(nz & (p < pad), p, pad)
            big = np.maximum(np.abs(lo[a]), np.abs(hi[a]))
            eps[:, a] = np.where(nz, (np.abs(oa) + big) * f32(2.0 ** -20) / np.abs(da), f32(0))
        alive = ok & (t0 < t1)
        pad = np.where(np.isinf(pad), f32(0), PAD_SCALE * pad).astype(f32)
        tmax = np.full((R, 3), np.inf, f32)
        for a in range(3):
            nz = step[:, a] != 0
            p = np.fmin(np.fmax(o[:, a] + d[:, a] * t0, lo[a]), hi[a])
            ia, _ = np_axis(p, lo[a], hi[a], cell[a], res)
            idx[:, a] = np.where(nz, ia, idx[:, a])
            k = np.where(step[:, a] > 0, idx[:, a] + 1, idx[:, a])
            tmax[:, a] = np.where(nz, (edge(cell[a], lo[a], hi[a], k) - o[:, a]) / d[:, a], f32(np.inf))
        t, tn, tf = t0.copy(), np.zeros(R, f32), np.zeros(R, f32)
        hit = np.zeros(R, bool)
        for _ in range(3 * res + 1):
            te, ax = t1.copy(), np.full(R, -1)
            for a in range(3):
                c = tmax[:, a] < te
                te, ax = np.where(c, tmax[:, a], te), np.where(c, a, ax)
            cnt = alive & (te > t) & mask[idx[:, 0], idx[:, 1], idx[:, 2]]
            tn = np.where(cnt & ~hit, t, tn)
            hit |= cnt
            tf = np.where(cnt, te, tf)
            alive &= ax >= 0
            axc = np.maximum(ax, 0)
            # near-ties
            tied = np.zeros(R, np.int64)
            for a in range(3):
                tied |= np.where(alive & (ax != a) & (tmax[:, a] - te <= eps[ar, axc] + eps[:, a]), 1 << a, 0)
            both = np.where(tied > 0, tied | (1 << axc), 0)
            tc = np.where(te > t, te, t)
            for m in range(1, 7):
                use = (tied > 0) & ((m & ~both) == 0) & (m != both)
                ks = [idx[:, a] + np.where(m >> a & 1, step[:, a], 0) for a in range(3)]
                for k in ks:
                    use &= (k >= 0) & (k < res)
                ks = [np.clip(k, 0, res - 1) for k in ks]
                cnt = use & mask[ks[0], ks[1], ks[2]]
                tn = np.where(cnt & ~hit, tc, tn)
                hit |= cnt
                tf = np.where(cnt, tc, tf)
            st = step[ar, axc]
            k = idx[ar, axc] + st
            alive &= (k >= 0) & (k < res)
            kc = np.clip(k, 0, res - 1)
            tm = (edge(cell[axc], lo[axc], hi[axc], np.where(st > 0, kc + 1, kc)) - o[ar, axc]) / d[ar, axc]
            idx[ar[alive], axc[alive]] = kc[alive]
            tmax[ar[alive], axc[alive]] = tm[alive]
            t = np.where(alive & (te > t), te, t)
            if not alive.any():
                break
        a_lo, a_hi = tn - pad, tf + pad
        n2, f2 = np.where(a_lo > near, a_lo, near), np.where(a_hi < far, a_hi, far)
        hit &= f2 > n2
    span = np.stack([np.where(hit, n2, near), np.where(hit, f2, far)], -1).astype(f32)
    return hit, span


# ---------------------------------------------------------------- the fp64 reference
def ref_interval(ray, lo, hi, mask):
    """Brute force in fp64: (inf I, sup I, longest stretch of I) for I = the depths of [near, far] at which
    o + t d is inside the box and in an occupied cell, or None when I has no interior. Every face crossing of
    every axis is sorted and the midpoint of each segment between two crossings is classified."""
    ray, lo, hi = np.asarray(ray, f32).astype(np.float64), np.asarray(lo, f32), np.asarray(hi, f32)
    res = mask.shape[0]
    cell = ((hi - lo) / f32(res)).astype(f32).astype(np.float64)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    o, d, near, far = ray[0:3], ray[3:6], ray[6], ray[7]
    ts = [near, far]
    for a in range(3):
        if d[a] != 0:
            edges = np.concatenate([lo[a] + np.arange(res) * cell[a], [hi[a]]])
            ts.extend((edges - o[a]) / d[a])
    ts = np.unique(np.clip(np.asarray(ts), near, far))
    if len(ts) < 2:
        return None
    mid = 0.5 * (ts[1:] + ts[:-1])
    p = o + mid[:, None] * d
    inside = ((p >= lo) & (p <= hi)).all(-1)
    idx = np.clip(np.floor((np.clip(p, lo, hi) - lo) / cell).astype(np.int64), 0, res - 1)
    occ = inside & mask[idx[:, 0], idx[:, 1], idx[:, 2]]
    if not occ.any():
        return None
    first, last = np.argmax(occ), len(occ) - 1 - np.argmax(occ[::-1])
    # longest run of consecutive occupied segments
    best = run = 0.0
    for i in range(len(occ)):
        run = run + (ts[i + 1] - ts[i]) if occ[i] else 0.0
        best = max(best, run)
    return ts[first], ts[last + 1], best


def near_tied(ray, lo, hi, res):
    """fp64: inside the box and [near, far] the ray crosses faces of two axes at depths closer than the
    rounding of fp32 sample positions (csrc/ray_span.hip's eps_a + eps_b): it runs through cell edges."""
    ray, lo, hi = np.asarray(ray, f32).astype(np.float64), np.asarray(lo, f32), np.asarray(hi, f32)
    cell = ((hi - lo) / f32(res)).astype(f32).astype(np.float64)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    o, d, near, far = ray[0:3], ray[3:6], ray[6], ray[7]
    ts, eps = [], []
    for a in range(3):
        if d[a] != 0:
            t = (np.concatenate([lo[a] + np.arange(1, res) * cell[a]]) - o[a]) / d[a]
            ts.append(t[(t >= near) & (t <= far)])
            eps.append((abs(o[a]) + max(abs(lo[a]), abs(hi[a]))) * 2.0 ** -20 / abs(d[a]))
    for i in range(len(ts)):
        for j in range(i + 1, len(ts)):
            if len(ts[i]) and len(ts[j]):
                gap = np.abs(ts[i][:, None] - ts[j][None, :])
                p = o + 0.5 * (ts[i][:, None, None] + ts[j][None, :, None]) * d
                inside = ((p >= lo) & (p <= hi)).all(-1)
                if bool((inside & (gap <= eps[i] + eps[j])).any()):
                    return True
    return False


def ref_widened(ray, lo, hi, mask, w):
    """fp64: (inf, sup) of the depths of [near - w, far + w] at which the ray is in some occupied cell with
    each of its three slabs widened by w in depth (on an axis with d = 0: by w in position), or None."""
    ray, lo, hi = np.asarray(ray, f32).astype(np.float64), np.asarray(lo, f32), np.asarray(hi, f32)
    res = mask.shape[0]
    cell = ((hi - lo) / f32(res)).astype(f32).astype(np.float64)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    o, d, near, far = ray[0:3], ray[3:6], ray[6], ray[7]
    ijk = np.argwhere(mask)
    if len(ijk) == 0:
        return None
    tin, tout = np.full(len(ijk), near - w), np.full(len(ijk), far + w)
    for a in range(3):
        e0 = lo[a] + ijk[:, a] * cell[a]
        e1 = np.where(ijk[:, a] == res - 1, hi[a], lo[a] + (ijk[:, a] + 1) * cell[a])
        if d[a] == 0:
            out = (o[a] < e0 - w) | (o[a] > e1 + w)
            tin, tout = np.where(out, np.inf, tin), np.where(out, -np.inf, tout)
        else:
            ta, tb = (e0 - o[a]) / d[a], (e1 - o[a]) / d[a]
            tin, tout = np.maximum(tin, np.minimum(ta, tb) - w), np.minimum(tout, np.maximum(ta, tb) + w)
    ok = tin <= tout
    return (float(tin[ok].min()), float(tout[ok].max())) if ok.any() else None


# ---------------------------------------------------------------- rays
def special_rays(lo, hi):
    """Packed rows [n, 8] of the cases a DDA gets wrong first. The box centre is a cell corner at every even
    resolution, and x_mid a cell-boundary plane."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    c = (0.5 * (lo + hi)).astype(f32)
    ext = hi - lo
    x_mid = f32(f32(ext[0] / f32(2)) + lo[0])
    diag = (ext / np.linalg.norm(ext)).astype(f32)
    g = np.array([0.5, 0.6, 0.62], f32)          # a generic direction
    rows = [
        # axis-parallel, two components exactly 0: inside / outside the box on the constant axes
        ([lo[0] - 1, c[1] + 0.1, c[2] - 0.2], [1, 0, 0], NEAR, FAR),
        ([c[0] + 0.1, hi[1] + 1, c[2] + 0.2], [0, -1, 0], NEAR, FAR),
        ([lo[0] - 1, hi[1] + 0.5, c[2]], [1, 0, 0], NEAR, FAR),
        ([c[0], c[1], hi[2] + 1], [0, 0, -1], NEAR, FAR),
        # one component exactly 0: inside / outside
        ([c[0] + 0.3, lo[1] - 1, lo[2] - 0.5], [0, 0.8, 0.6], NEAR, FAR),
        ([c[0] - 0.2, c[1] + 0.4, hi[2] + 0.7], [0.3, 0, -0.9], NEAR, FAR),
        ([hi[0] + 0.1, lo[1] - 1, c[2]], [0, 0.8, 0.6], NEAR, FAR),
        # lying in a cell-boundary plane (x = x_mid), and along a cell edge of it
        ([x_mid, lo[1] - 1, c[2] + 0.05], [0, 1, 0.01], NEAR, FAR),
        ([x_mid, lo[1] - 1, c[2]], [0, 1, 0], NEAR, FAR),
        ([lo[0], lo[1] - 1, c[2] + 0.3], [0, 1, 0.1], NEAR, FAR),            # in the box's own face
        # negative directions
        (hi + 1, [-0.6, -0.5, -0.62], NEAR, FAR),
        ([hi[0] + 1, c[1] - 0.2, lo[2] - 1], [-0.7, 0.05, 0.7], NEAR, FAR),
        # origin inside a cell (occupied under ball, full and, maybe, random), near = 0
        (c + f32(0.01), g, 0.0, FAR),
        (c + f32(0.01), -g, 0.0, FAR),
        # near and far both inside one cell
        (c + f32(0.01), g, 0.001, 0.02),
        (c - f32(0.01), -g, 0.001, 0.02),
        # far short of the box, and near past it
        ([lo[0] - 2, c[1], c[2]], [1, 0.1, 0.05], 0.5, 1.5),
        ([lo[0] - 2, c[1], c[2]], [1, 0.1, 0.05], 12.0, 20.0),
        # far / near inside the box, short of / past the ball
        ([lo[0] - 1, c[1], c[2]], [1, 0.02, 0.03], 0.5, 3.0),
        ([lo[0] - 1, c[1], c[2]], [1, 0.02, 0.03], 5.5, 20.0),
        # missing the box
        ([lo[0] - 1, hi[1] + 1, c[2]], [0.1, 1, 0], NEAR, FAR),
        ([lo[0] - 1, c[1], c[2]], [-1, 0.2, 0.1], NEAR, FAR),
        ([lo[0] - 1, lo[1] - 1, c[2]], [1, -1, 0.3], NEAR, FAR),
        # through the box's corner: entering at it, leaving at it, only touching it, and the main diagonal
        (lo - 2 * g, g, NEAR, FAR),
        (c + 0.3 * g, (hi - (c + 0.3 * g)) / 3, NEAR, FAR),
        ([hi[0] - 1, hi[1] + 1, hi[2]], [1, -1, 0], NEAR, FAR),
        (lo - diag, diag, NEAR, 2 * FAR),
        (hi + diag, -diag, NEAR, 2 * FAR),
    ]
    return np.array([np.concatenate([np.asarray(o, f32), np.asarray(d, f32), [f32(n), f32(f)]]) for o, d, n, f in rows],
                    f32)


def random_rays(n, lo, hi, seed=5):
    """Origins in twice the box, directions towards a point of 1.2 times the box (most cross it)."""
    rng = np.random.default_rng(seed)
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    o = c + (rng.random((n, 3)) * 2 - 1) * 2.0 * half
    d = c + (rng.random((n, 3)) * 2 - 1) * 1.2 * half - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    near = rng.random(n) * 0.5
    far = near + rng.random(n) * 12.0
    return np.concatenate([o, d, near[:, None], far[:, None]], -1).astype(f32)


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    sc = build_scene(nerf, gpu)
    lo, hi, packed = sc["lo"], sc["hi"], sc["packed"]
    frame_rays = np.concatenate([packed(i).cpu().numpy()[:, :8] for i in (0, 1)])
    pool = np.concatenate([special_rays(lo, hi), frame_rays, random_rays(4097, lo, hi)])[:4097]
    return dict(sc, pool=pool, n_special=len(special_rays(lo, hi)))


def gpu_span(scene, gpu, rays, mask, cols=8):
    rows = np.asarray(rays, f32)
    if cols == 11:
        rows = np.concatenate([rows, np.zeros((len(rows), 3), f32)], -1)
    hit, span = scene["grid_of"](mask).ray_span(torch.from_numpy(rows).to(gpu))
    assert hit.dtype == torch.bool and span.dtype == torch.float32 and span.shape == (len(rows), 2)
    return hit.cpu().numpy(), span.cpu().numpy()


# ---------------------------------------------------------------- 1. the kernel is its NumPy restatement
CASES = [(1, 16, "ball"), (63, 1, "full"), (63, 4, "random"), (63, 5, "random"), (63, 16, "ball"), (63, 128, "random"),
         (193, 1, "empty"), (193, 4, "full"), (193, 5, "random"), (193, 16, "random"), (193, 16, "ball"),
         (193, 16, "empty"), (193, 128, "ball"), (193, 128, "full"), (4097, 1, "full"), (4097, 4, "random"),
         (4097, 5, "random"), (4097, 16, "ball"), (4097, 16, "full"), (4097, 128, "random")]


@pytest.mark.parametrize("R,res,name", CASES)
def test_span_kernel_matches_numpy_bit_for_bit(nerf, gpu, scene, R, res, name):
    lo, hi = scene["lo"], scene["hi"]
    mask = make_mask(name, res)
    if name == "ball" and res == 16:
        assert int(mask.sum()) == 88
    rays = scene["pool"][12:13] if R == 1 else scene["pool"][:R]     # R = 1: the origin inside the ball
    assert R == 1 or R > scene["n_special"]                          # every special case is in every other set
    want_hit, want_span = np_span(rays, lo, hi, mask)
    for cols in (8, 11):
        hit, span = gpu_span(scene, gpu, rays, mask, cols)
        assert np.array_equal(hit, want_hit), f"hit differs on rays {np.nonzero(hit != want_hit)[0][:8]}"
        assert np.array_equal(span.view(np.int32), want_span.view(np.int32)), \
            f"span differs on rays {np.nonzero((span != want_span).any(-1))[0][:8]}"
    assert bool((span[:, 0] >= rays[:, 6]).all() and (span[:, 1] <= rays[:, 7]).all())     # inside [near, far]
    assert np.array_equal(span[~hit], rays[~hit][:, 6:8])
    assert bool((span[hit][:, 1] > span[hit][:, 0]).all())
    if R > 1 and name in ("random", "ball"):
        assert hit.any() and (~hit).any()                            # both answers occur
    if name == "empty":
        assert not hit.any()


def test_nan_rays_miss(nerf, gpu, scene):
    """A NaN in the origin, the direction, near or far is a miss with the span [near, far] as given."""
    lo, hi = scene["lo"], scene["hi"]
    base = scene["pool"][12]                                         # hits every non-empty mask
    rays = np.tile(base, (9, 1))
    for c in range(8):
        rays[c + 1, c] = np.nan
    mask = make_mask("full", 4)
    hit, span = gpu_span(scene, gpu, rays, mask)
    want_hit, want_span = np_span(rays, lo, hi, mask)
    assert hit.tolist() == [True] + [False] * 8 and np.array_equal(hit, want_hit)
    assert np.array_equal(span.view(np.int32), want_span.view(np.int32))
    assert np.array_equal(span[1:].view(np.int32), rays[1:, 6:8].view(np.int32))


# ---------------------------------------------------------------- 1b. the compaction
@pytest.mark.parametrize("R", [63, 193, 4097, 3 * 4096 + 5])
@pytest.mark.parametrize("res,name", [(16, "ball"), (5, "random"), (4, "full"), (16, "empty")])
def test_gather_is_the_hit_rows_in_order(nerf, gpu, scene, R, res, name):
    """bound_rays: rows = the hit rays ascending, rays_c = their rows with columns 6:8 replaced by the span, for 8
    and 11 columns; R crosses the wave (64), the k-loop (256) and the block (4096) of the gather kernel."""
    lo, hi = scene["lo"], scene["hi"]
    pool = scene["pool"]
    if R > len(pool):
        pool = np.concatenate([pool, random_rays(R - len(pool), lo, hi, seed=9)])
    grid = scene["grid_of"](make_mask(name, res))
    for cols in (8, 11):
        rows_np = pool[:R]
        if cols == 11:        # distinct view-direction columns: a row gathered from the wrong ray shows
            rows_np = np.concatenate([rows_np, np.arange(3 * R, dtype=f32).reshape(R, 3)], -1)
        rays = torch.from_numpy(rows_np).to(gpu)
        want_hit, want_span = grid.ray_span(rays)
        hit, span, rows, rays_c = grid.bound_rays(rays)
        assert torch.equal(hit, want_hit) and bits_equal(span, want_span)
        assert rows.dtype == torch.int32 and rows.shape == (int(hit.sum()),)
        assert torch.equal(rows, torch.nonzero(hit).flatten().to(torch.int32))
        want = rays[hit].clone()
        want[:, 6:8] = span[hit]
        assert rays_c.shape == (int(hit.sum()), cols) and bits_equal(rays_c, want)
    if name in ("ball", "random"):
        assert 0 < int(hit.sum()) < R
    elif name == "empty":
        assert int(hit.sum()) == 0


def test_special_rays_are_what_they_claim(scene):
    """The fixture's own claims, in fp64 against the full grid: which of the special rays meet the box."""
    lo, hi = scene["lo"], scene["hi"]
    sp = special_rays(lo, hi)
    meets = np.array([ref_interval(r, lo, hi, np.ones((1, 1, 1), bool)) is not None for r in sp])
    #                  parallel      one zero   plane    neg   inside  one cell  far/near      miss     corner
    want = np.array([1, 1, 0, 1,  1, 1, 0,  1, 1, 1,  1, 1,  1, 1,  1, 1,  0, 0, 1, 1,  0, 0, 0,  1, 1, 0, 1, 1], bool)
    meets[25] = False           # the ray that only touches a corner: a graze of rounding's size either way
    assert np.array_equal(meets, want), np.nonzero(meets != want)[0]
    assert int((sp[:, 3:6] == 0).sum(-1).max()) == 2 and bool((sp[:, 3:6] < 0).any())


# ---------------------------------------------------------------- 2. conservative
@pytest.mark.parametrize("res,name", [(16, "ball"), (5, "random"), (16, "random"), (128, "random"), (4, "full")])
def test_span_is_conservative(nerf, gpu, scene, res, name):
    """No depth whose fp32 sample position o + d t the cell rule calls occupied lies outside the span: an
    8192-point lattice on [near, far] plus every face crossing (edge - o) / d and its two float neighbours."""
    lo, hi = scene["lo"], scene["hi"]
    mask = make_mask(name, res)
    rays = scene["pool"][:scene["n_special"] + 2 * H * W + 40]
    hit, span = gpu_span(scene, gpu, rays, mask)
    cell = ((hi - lo) / f32(res)).astype(f32)
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    lattice = (near[:, None] + (far - near)[:, None] * (np.arange(8192, dtype=f32) / f32(8191))).astype(f32)
    ts = [lattice]
    with np.errstate(all="ignore"):
        for a in range(3):
            edges = np.concatenate([lo[a] + np.arange(res, dtype=f32) * cell[a], hi[a:a + 1]]).astype(f32)
            tc = ((edges[None, :] - o[:, a:a + 1]) / d[:, a:a + 1]).astype(f32)
            ts += [tc, np.nextafter(tc, f32(-np.inf)), np.nextafter(tc, f32(np.inf))]
    t = np.concatenate(ts, -1)
    valid = np.isfinite(t) & (t >= near[:, None]) & (t <= far[:, None])
    t = np.where(valid, t, near[:, None]).astype(f32)
    pts = (o[:, None, :] + d[:, None, :] * t[:, :, None]).astype(f32)
    occ = np_query(pts.reshape(-1, 3), lo, hi, mask).reshape(t.shape) & valid
    share = float(occ[:, :8192].mean())
    print(f"res {res} {name}: {100 * share:.2f} % of the lattice points occupied, {int(hit.sum())} of {len(hit)} rays hit")
    assert 0.0 < share < 1.0
    outside = occ & ~(hit[:, None] & (t >= span[:, 0:1]) & (t <= span[:, 1:2]))
    assert not outside.any(), (f"{int(outside.sum())} occupied depths outside the span, rays "
                               f"{np.nonzero(outside.any(-1))[0][:8]}")


# ---------------------------------------------------------------- 3. tight
@pytest.mark.parametrize("res,name", [(16, "ball"), (5, "random"), (16, "random"), (4, "random"), (1, "full")])
def test_span_is_tight(nerf, gpu, scene, res, name):
    """Against the fp64 reference: near' >= max(near, inf I - 2 pad), far' <= min(far, sup I + 2 pad); a ray that
    crosses occupied cells over more than 2 pad is not missed; a hit ray has something within 2 pad.
    The two main diagonals of the box (the last two special rays) run through cell edges: fp32 sample positions
    on them do land in cells the exact ray only touches (test_span_is_conservative holds the kernel to those), so
    no span can be both conservative and within 2 pad of the exact I there. For such rays (near_tied: those
    two, asserted) I is taken over cells widened by pad and the span may exceed it by pad, 2 pad in all."""
    lo, hi = scene["lo"], scene["hi"]
    mask = make_mask(name, res)
    rays = scene["pool"][:scene["n_special"] + 2 * H * W + 40]
    hit, span = gpu_span(scene, gpu, rays, mask)
    pad = np_pad(rays, lo, hi, res).astype(np.float64)
    n_hit, tied = 0, []
    for r, ray in enumerate(rays):
        near, far = float(ray[6]), float(ray[7])
        ref = ref_interval(ray, lo, hi, mask)
        if ref is not None and ref[2] > 2 * pad[r]:
            assert hit[r], f"ray {r}: crosses occupied cells over {ref[2]:.3g} > 2 pad = {2 * pad[r]:.3g}, reported missed"
        if not hit[r]:
            continue
        n_hit += 1
        slack = 2 * pad[r]
        if near_tied(ray, lo, hi, res):
            tied.append(r)
            ref, slack = ref_widened(ray, lo, hi, mask, pad[r]), pad[r]
        if ref is None:
            assert ref_widened(ray, lo, hi, mask, 2 * pad[r]) is not None, f"ray {r}: hit, nothing within 2 pad"
            continue
        assert span[r, 0] >= max(near, ref[0] - slack), f"ray {r}: near' {span[r, 0]} vs inf I {ref[0]}"
        assert span[r, 1] <= min(far, ref[1] + slack), f"ray {r}: far' {span[r, 1]} vs sup I {ref[1]}"
    assert 0 < n_hit < len(rays)
    # the exemption covers the two main diagonals (the last two special rays) and nothing else
    assert set(tied) <= {scene["n_special"] - 2, scene["n_special"] - 1}, tied


# ---------------------------------------------------------------- 4. render(ray_bounds=) = the hand composition
def hand_composition(nerf, scene, i, grid, chunk, **over):
    """The same thing from existing pieces: pack, ray_span, torch indexing, batchify_rays, scatter."""
    kw = dict(scene["kw"], **over)
    rays = scene["packed"](i)
    hit, span = grid.ray_span(rays)
    sel = rays[hit].clone()
    sel[:, 6:8] = span[hit]
    for k in ("near", "far", "ndc", "use_viewdirs"):
        kw.pop(k)
    with torch.no_grad():
        part = nerf.batchify_rays(sel, chunk, retraw=True, **kw)
    out = scatter_back(part, hit)
    out.update(ray_hit=hit.reshape(H, W), ray_span=span.reshape(H, W, 2))
    return out


@pytest.mark.parametrize("which", ["ball16", "random5"])
@pytest.mark.parametrize("i", [0, 1])
def test_render_is_the_hand_composition(nerf, gpu, scene, i, which):
    mask = ball_mask() if which == "ball16" else random_mask(5)
    grid = scene["grid_of"](mask)
    variants = [dict(N_importance=0), dict(), dict(occupancy=grid), dict(N_importance=0, occupancy=grid),
                dict(early_stop=0.05, early_stop_slab=8), dict(occupancy=grid, early_stop=0.05, early_stop_slab=8)]
    for over in variants:
        for chunk in (37, 4096):
            want = hand_composition(nerf, scene, i, grid, chunk, **over)
            got = scene["frame"](i, chunk=chunk, ray_bounds=grid, **over)
            assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
            for k in want:
                assert bits_equal(got[k].to(want[k].dtype) if got[k].dtype == torch.bool else got[k],
                                  want[k]), f"{which} pose {i} {sorted(over)} chunk {chunk}: {k} differs"
            hit = got["ray_hit"]
            assert hit.any() and (which != "ball16" or not hit.all())    # ball16: the frame has both kinds of ray
            assert bool((got["rgb_map"][~hit] == 1).all() and (got["acc_map"][~hit] == 0).all())
            assert bool(torch.isnan(got["depth_map"][~hit]).all())
            if "early_stop" in over:
                assert got["early_stop_samples"].dtype == torch.int32
                assert bool((got["early_stop_samples"][~hit] == 0).all())


def test_without_the_keyword_nothing_changes(nerf, gpu, scene):
    """ray_bounds=None is the call without it: same entries, same bits."""
    a, b = scene["frame"](0), scene["frame"](0, ray_bounds=None)
    assert sorted(a) == sorted(b) and "ray_hit" not in a
    for k in a:
        assert bits_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 5. full grid
def test_full_grid_gives_the_box_clip(nerf, gpu, scene):
    """Every ray that meets the box is hit, its span is the box clip of [near, far] widened by at most pad."""
    lo, hi = scene["lo"], scene["hi"]
    rays = scene["pool"][:scene["n_special"] + 2 * H * W + 200]
    hit, span = gpu_span(scene, gpu, rays, np.ones((16, 16, 16), bool))
    pad = np_pad(rays, lo, hi, 16).astype(np.float64)
    one = np.ones((1, 1, 1), bool)
    for r, ray in enumerate(rays):
        ref = ref_interval(ray, lo, hi, one)         # the box clip of [near, far], fp64
        if ref is None or ref[1] - ref[0] <= 1e-5:
            # missing the box, or only grazing it (the corner-touching ray): a hit must be a graze
            assert not hit[r] or span[r, 1] - span[r, 0] <= 2 * pad[r] + 1e-5, f"ray {r} misses the box"
            continue
        assert hit[r], f"ray {r} meets the box over {ref[1] - ref[0]:.3g}"
        tol = 1e-5 * max(1.0, abs(ref[0]), abs(ref[1]))          # fp32 depths of the faces
        assert max(ray[6], ref[0] - pad[r]) - tol <= span[r, 0] <= ref[0] + tol, f"ray {r}: near' {span[r, 0]} vs {ref[0]}"
        assert ref[1] - tol <= span[r, 1] <= min(ray[7], ref[1] + pad[r]) + tol, f"ray {r}: far' {span[r, 1]} vs {ref[1]}"
    assert hit.any() and (~hit).any()


def test_full_grid_render_drops_the_rays_that_miss_the_box(nerf, gpu, scene):
    """Rendered with a full grid: the rays that miss the box are dropped and are exactly the background."""
    grid = scene["grid_of"](np.ones((16, 16, 16), bool))
    dropped = 0
    for i in (0, 1):
        got = scene["frame"](i, ray_bounds=grid)
        miss = ~got["ray_hit"]
        dropped += int(miss.sum())
        assert bool((got["rgb_map"][miss] == 1).all())
    # the camera of this scene sits inside the box: every frame ray meets it. A camera further out drops rays.
    far_pose = nerf.pose_spherical(-40.0, -30.0, 9.0)[:3, :4].to(gpu)
    K = scene["K"].copy()
    K[0, 0] = K[1, 1] = 0.25 * K[0, 0]
    with torch.no_grad():
        rgb, _, _, ex = nerf.render(H, W, K, chunk=4096, c2w=far_pose, ray_bounds=grid, **dict(scene["kw"], far=20.0))
    miss = ~ex["ray_hit"]
    print(f"full grid: {dropped} of {2 * H * W} scene rays and {int(miss.sum())} of {H * W} wide-angle rays miss the box")
    assert 0 < int(miss.sum()) < H * W
    assert bool((rgb[miss] == 1).all())


# ---------------------------------------------------------------- 6. empty grid
def test_empty_grid_makes_no_field_call(nerf, gpu, scene):
    grid = scene["grid_of"](np.zeros((16, 16, 16), bool))
    calls = []
    nqf = scene["kw"]["network_query_fn"]

    def recording(pts, viewdirs, fn):
        calls.append(tuple(pts.shape))
        return nqf(pts, viewdirs, fn)

    head = nerf.NeRFSmall(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                          input_ch=32, input_ch_views=16, predict_normals=True).to(gpu).eval()
    for over in (dict(), dict(N_importance=0), dict(early_stop=0.05), dict(network_fine=head, predict_normals=True)):
        got = scene["frame"](0, ray_bounds=grid, network_query_fn=recording, **over)
        assert calls == []
        assert not got["ray_hit"].any()
        assert bool((got["rgb_map"] == 1).all() and (got["acc_map"] == 0).all())
        assert bool(torch.isnan(got["depth_map"]).all())
        assert bits_equal(got["ray_span"], scene["packed"](0)[:, 6:8].reshape(H, W, 2))
        # the entries of a frame with hits, in the frame's shape
        ref = scene["frame"](0, ray_bounds=scene["grid_of"](ball_mask()), **over)
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
    scene["frame"](0, network_query_fn=recording)
    assert len(calls) == 2                                          # the recorder does record


# ---------------------------------------------------------------- 7. the point of the feature
def test_bounded_samples_are_closer_to_the_truth(nerf, gpu, scene):
    """ball16, coarse only, occupancy=grid on both sides: against a 256-sample unbounded render, 32 samples
    placed inside the span are closer than 32 samples over [near, far] (mean |rgb - truth| over the hit rays of
    both poses). No margin: inside the ball the bounded samples are several times denser.
    Measured on the MI355X: see DESIGN.md §15."""
    grid = scene["grid_of"](ball_mask())
    num_b = num_u = 0.0
    n = 0
    for i in (0, 1):
        truth = scene["frame"](i, N_importance=0, N_samples=256, occupancy=grid)["rgb_map"]
        unb = scene["frame"](i, N_importance=0, N_samples=32, occupancy=grid)["rgb_map"]
        got = scene["frame"](i, N_importance=0, N_samples=32, occupancy=grid, ray_bounds=grid)
        hit = got["ray_hit"]
        num_b += float((got["rgb_map"][hit] - truth[hit]).abs().sum())
        num_u += float((unb[hit] - truth[hit]).abs().sum())
        n += int(hit.sum()) * 3
        # a missed ray is the background in all three
        assert bool((truth[~hit] == 1).all() and (unb[~hit] == 1).all() and (got["rgb_map"][~hit] == 1).all())
        span = got["ray_span"][hit]
        print(f"pose {i}: {int(hit.sum())} of {H * W} rays hit, mean span {float((span[:, 1] - span[:, 0]).mean()):.3f} "
              f"of {FAR - NEAR}")
    err_b, err_u = num_b / n, num_u / n
    print(f"mean |rgb - truth|: 32 bounded samples {err_b:.3e}, 32 unbounded samples {err_u:.3e}")
    assert n > 0 and err_b < err_u
