"""SH read through a ray index in the grid march, driven through the C entries (csrc/march.hip, csrc/field_x6.hip;
DESIGN.md §21), needs an MI355X.

The specification has no tolerance. nerf_ray_sh_records writes the record nerf_sample_stratified_sh writes per ray;
the two writes with a ray index leave the positions, depths and distances of nerf_march_write / nerf_slab_march_write
and the row number of each entry's ray; and each _rays forward gives, in every bit of raw, its twin's result at
sh_stride 16 on the rows gathered from the records (rec[ray_of, :16]): the record's pieces are what the twin's split
makes of such a row (test_gpu_sh_rows.py), piece 0 is the bf16 forward's rounding of it.

The sensitivity test is what keeps those equalities from being met by a kernel that ignores the index: with one
random unit view direction per ray, rolling the ray map by one ray must change a colour channel in at least half of
the points. The same inputs are first run through the oracle's NeRFSmall on the CPU, where the share is 100 %.
"""
import ctypes

import numpy as np
import pytest
import torch

from forward_only import FAR, NEAR, ball_mask, random_mask
from tables import blender_bbox
from test_gpu_feat_bf16 import bits, real_weights
from test_gpu_march import hand_rays
from test_gpu_mlp_bf16 import weights_struct

pytestmark = pytest.mark.gpu

ENTRIES = [("nerf_mlp_fwd_rays", "nerf_mlp_fwd_ord", False), ("nerf_mlp_fwd_bf16_rays", "nerf_mlp_fwd_bf16", False),
           ("nerf_mlp_fwd_bf16_pkbf_rays", "nerf_mlp_fwd_bf16_pkbf", True)]
MLP_POINTS = (1, 31, 32, 33, 257, 4097)
GRIDS = {"empty": lambda: np.zeros((4, 4, 4), bool), "full": lambda: np.ones((4, 4, 4), bool), "ball16": ball_mask,
         "random5": lambda: random_mask(5)}


def unit_dirs(n, seed):
    d = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed))
    return d / d.norm(dim=-1, keepdim=True)


def records(L, rays):
    rec = torch.full((rays.shape[0], 40), float("nan"), device=rays.device)
    L.call("nerf_ray_sh_records", L.ptr(rays, "rays"), rays.shape[0], rays.shape[1], L.ptr(rec, "rec"), L.stream())
    return rec


def rays_of_dirs(gpu, dirs):
    """Packed rows [R, 11] whose view directions (columns 8..10) are `dirs`."""
    R = dirs.shape[0]
    g = torch.Generator().manual_seed(R)
    return torch.cat([torch.rand(R, 8, generator=g), dirs], 1).to(gpu).contiguous()


# ---------------------------------------------------------------- 1. the records
@pytest.mark.parametrize("R", [1, 63, 64, 65, 193, 4097])
def test_records_are_the_samplers(nerf, gpu, R):
    import indoor_nerf_amd._lib as L
    from indoor_nerf_amd.render import _linspace
    specials = [torch.tensor([float("nan"), 0.3, 0.2]), torch.zeros(3)]
    for first in range(2 if R == 1 else 1):
        dirs = unit_dirs(R, R)
        dirs[0] = specials[first]
        if R > 1:
            dirs[R - 1] = specials[1]
        rays = rays_of_dirs(gpu, dirs)
        f = dict(device=gpu, dtype=torch.float32)
        z, pts, ref = torch.empty(R, 2, **f), torch.empty(R, 2, 3, **f), torch.full((R, 40), float("nan"), **f)
        rd, vd = torch.empty(R, 3, **f), torch.empty(R, 3, **f)
        L.call("nerf_sample_stratified_sh", L.ptr(rays), 11, R, 2, L.ptr(_linspace(2, gpu)), 0, 0, None, 0, 0, None,
               L.ptr(z), L.ptr(pts), L.ptr(rd), L.ptr(vd), L.ptr(ref), L.stream())
        rec = records(L, rays)
        assert torch.equal(bits(rec), bits(ref)), f"R {R}: {int((bits(rec) != bits(ref)).any(1).sum())} records differ"
        assert bool(torch.isnan(ref[0, 3]).item()) == (first == 0)      # coefficient 3 is -c x
        if R > 1:
            assert float(ref[R - 1, 0]) == pytest.approx(0.2820948) and not bool(ref[R - 1, 1:16].any())
            assert bool((ref[1:R - 1, 1:16] != 0).any(1).all()) if R > 2 else True


# ---------------------------------------------------------------- 2. the writes
def ray_pool(lo, hi):
    """test_gpu_march's hand-made rows (inside, missing, NaN, ...) and rays from a sphere of radius 4 at the box."""
    hand = hand_rays(lo, hi)
    rng = np.random.default_rng(5)
    o = rng.normal(size=(180, 3))
    o = 4.0 * o / np.linalg.norm(o, axis=-1, keepdims=True)
    target = lo + (hi - lo) * (rng.random((180, 3)) * 1.6 - 0.3)
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rows = np.concatenate([o, d, np.full((180, 1), NEAR), np.full((180, 1), FAR)], -1)
    rows = np.concatenate([hand, rows]).astype(np.float32)
    vd = rows[:, 3:6] / np.linalg.norm(rows[:, 3:6], axis=-1, keepdims=True)
    return np.concatenate([rows, vd.astype(np.float32)], -1)


@pytest.mark.parametrize("name", list(GRIDS))
def test_writes_leave_the_list_and_the_ray_of_each_entry(nerf, gpu, name):
    lo, hi = blender_bbox()
    grid = nerf.OccupancyGrid((torch.from_numpy(lo), torch.from_numpy(hi)), resolution=GRIDS[name]().shape[0], device=gpu)
    grid.set_mask(GRIDS[name]())
    pool = ray_pool(lo, hi)
    cases = [(R, K, None, None) for R in (1, 63, 193, 4097) for K in (1, 64, 65, 200)] + [(193, 200, 64, 130)]
    kept = 0
    for R, K, k0, k1 in cases:
        rows11 = torch.from_numpy(np.tile(pool, (R // len(pool) + 1, 1))[:R].copy()).to(gpu)
        alive = None
        if k0 is not None:
            alive = (torch.arange(R, device=gpu) % 3 != 2).to(torch.uint8)
        ref = None
        for C in (11, 8):
            rays, t, counts, offsets, _, n = grid._march_count(rows11[:, :C].contiguous(), K, k0, k1, alive)
            want = torch.repeat_interleave(torch.arange(R, device=gpu, dtype=torch.int32), counts.long())
            assert want.shape == (n,)
            what = f"{name} R {R} K {K} range {k0} {k1} C {C}"
            if C == 11:
                ref = grid._march_write(rays, t, K, counts, offsets, n, True, k0, k1)
                assert ref[3].shape == (n, 16)
                if alive is not None and name != "empty":
                    assert n > 0 and not bool(counts[alive == 0].any()) and bool(counts[alive != 0].any()), what
            pts_c, z_c, dist_c, ray_c = grid._march_write(rays, t, K, counts, offsets, n, True, k0, k1, index=True)
            assert ray_c.dtype == torch.int32 and torch.equal(ray_c, want), f"{what}: ray_c"
            for got, r, k in zip((pts_c, z_c, dist_c), ref, ("pts_c", "z_c", "dist_c")):
                assert torch.equal(bits(got), bits(r)), f"{what}: {k}"
            kept += n
    assert (kept == 0) == (name == "empty"), f"fixture: {kept} kept samples through {name}"


def test_write_stores_nothing_past_the_list(nerf, gpu):
    """The entry driven directly, into buffers longer than the list: the rows past it keep their contents."""
    import indoor_nerf_amd._lib as L
    lo, hi = blender_bbox()
    grid = nerf.OccupancyGrid((torch.from_numpy(lo), torch.from_numpy(hi)), resolution=4, device=gpu)
    grid.set_mask(np.ones((4, 4, 4), bool))
    rows = torch.from_numpy(ray_pool(lo, hi)[:63, :8].copy()).to(gpu)
    rays, t, counts, offsets, _, n = grid._march_count(rows, 64)
    assert n > 100
    fill, f = -7, dict(device=gpu, dtype=torch.float32)
    ray_c = torch.full((n + 9,), fill, device=gpu, dtype=torch.int32)
    pts_c, z_c, dist_c = torch.zeros(n + 9, 3, **f), torch.zeros(n + 9, **f), torch.zeros(n + 9, **f)
    L.call("nerf_rays_march_write", L.ptr(rays), 63, 8, L.ptr(t), 64, grid._bmin, grid._bmax, 4, grid._bits(),
           L.ptr(counts, "c", torch.int32), L.ptr(offsets, "o", torch.int32), n, n, L.ptr(pts_c), L.ptr(z_c),
           L.ptr(dist_c), L.ptr(ray_c, "ray_c", torch.int32), L.stream())
    want = torch.repeat_interleave(torch.arange(63, device=gpu, dtype=torch.int32), counts.long())
    assert torch.equal(ray_c[:n], want) and bool((ray_c[n:] == fill).all())


# ---------------------------------------------------------------- 3. the forwards
def features(gpu, P, layout, packed):
    """Random features of P points -> (tensor, point stride, level stride): fp32 pairs or, packed, bf16 words."""
    x = torch.randn(P, 32, generator=torch.Generator().manual_seed(100 + P)) * 0.5
    if packed:
        words = x.to(torch.bfloat16).contiguous().view(torch.int32).reshape(P, 16)
        return (words.contiguous().to(gpu), 16, 1) if layout == "point" else (words.t().contiguous().to(gpu), 1, P)
    if layout == "point":
        return x.contiguous().to(gpu), 32, 2
    return x.view(P, 16, 2).permute(1, 0, 2).contiguous().to(gpu), 2, 2 * P


def ray_maps(P):
    """name -> (int32 map [P], n_rays): the hand-made maps of the module docstring's cases."""
    seg, ids, r = [49, 1, 1, 17, 40, 1, 33], [], 0
    while len(ids) < P:                       # segments of 1, segments across a 32-point tile boundary, and every
        ids += [r] * seg[r % len(seg)]        # third ray index skipped (a ray without a point)
        r += 2 if r % 3 == 2 else 1
    segmented = np.asarray(ids[:P], np.int32)
    n_seg = int(segmented[-1]) + 1            # the last index is n_rays - 1
    rng = np.random.default_rng(P)
    return {"one ray": (np.full(P, 4, np.int32), 5), "n_rays 1": (np.zeros(P, np.int32), 1),
            "segments of 1": (np.arange(P, dtype=np.int32), P), "segmented": (segmented, n_seg),
            "permuted": (rng.permutation(segmented), n_seg), "a ray beyond": (segmented, n_seg + 3)}


def launch(L, entry, W, feat, sp, sl, view, keep, P, tail, row0=0):
    raw = torch.full((P, 4), float("nan"), device=feat.device)
    dt = feat.dtype
    L.call(entry, L.ptr_at(feat, sp * row0, "feat", dtype=dt), sp, sl, *view,
           None if keep is None else L.ptr_at(keep, row0, "keep", dtype=torch.bool), P, ctypes.byref(W), L.ptr(raw), *tail,
           L.stream())
    return raw


def twin_tail(twin):
    return (None, None, None, 0, None) if twin == "nerf_mlp_fwd_ord" else (None,)


@pytest.mark.parametrize("P", MLP_POINTS)
@pytest.mark.parametrize("entry,twin,packed", ENTRIES)
def test_rays_entry_is_its_twin_on_the_gathered_rows(nerf, gpu, entry, twin, packed, P):
    import indoor_nerf_amd._lib as L
    Wt = real_weights(gpu)                   # kept alive: the struct holds bare pointers
    W = weights_struct(L, Wt)
    keep_flags = torch.from_numpy(np.random.default_rng(P).random(P) < 0.5).to(gpu)
    seen = set()
    for name, (m, n_rays) in ray_maps(P).items():
        assert 0 <= int(m.min()) and int(m.max()) < n_rays
        if name in ("one ray", "n_rays 1", "segmented", "permuted"):
            assert int(m.max()) == n_rays - 1
        if name == "segmented" and P > 49:
            assert int(m[31]) == int(m[32]), "fixture: no segment across the first tile boundary"
            assert len(set(m.tolist())) < int(m.max()) + 1, "fixture: no ray index is skipped"
        if name == "permuted" and P > 49:
            assert bool((np.diff(m) < 0).any()), "fixture: the permuted map is monotone"
        ray_of = torch.from_numpy(m).to(gpu)
        rec = records(L, rays_of_dirs(gpu, unit_dirs(n_rays, 7 + n_rays)))
        rows = rec[ray_of.long(), :16].contiguous()
        for layout in ("level", "point"):
            feat, sp, sl = features(gpu, P, layout, packed)
            for keep in (None, keep_flags):
                what = f"{entry} P {P} {name} {layout} keep {keep is not None}"
                ref = launch(L, twin, W, feat, sp, sl, (L.ptr(rows, "rows"), 16, None, 1), keep, P, twin_tail(twin))
                got = launch(L, entry, W, feat, sp, sl,
                             (L.ptr(rec, "rec"), L.ptr(ray_of, "ray_of", torch.int32), n_rays), keep, P, ())
                assert bool(torch.isfinite(ref).all()), what
                assert torch.equal(bits(got), bits(ref)), \
                    f"{what}: {int((bits(got) != bits(ref)).any(1).sum())} rows differ from the twin's"
                if keep is not None:
                    assert not bool(got[~keep, 3].any()) and (P < 31 or bool(got[keep, 3].any()))
        seen.add(name)
    assert len(seen) == 6
    del Wt


@pytest.mark.parametrize("entry,twin,packed", ENTRIES)
def test_slices_give_the_same_rows(nerf, gpu, entry, twin, packed):
    """The points from row 37 on, and from row 13 on, in launches of their own (feature, keep, index and raw pointers
    advanced): the rows of the whole launch."""
    import indoor_nerf_amd._lib as L
    P = 4097
    Wt = real_weights(gpu)                   # kept alive: the struct holds bare pointers
    W = weights_struct(L, Wt)
    m, n_rays = ray_maps(P)["segmented"]
    ray_of = torch.from_numpy(m).to(gpu)
    rec = records(L, rays_of_dirs(gpu, unit_dirs(n_rays, 3)))
    keep = torch.from_numpy(np.random.default_rng(1).random(P) < 0.7).to(gpu)
    for layout in ("level", "point"):
        feat, sp, sl = features(gpu, P, layout, packed)

        def run(row0):
            view = (L.ptr(rec, "rec"), L.ptr_at(ray_of, row0, "ray_of", dtype=torch.int32), n_rays)
            return launch(L, entry, W, feat, sp, sl, view, keep, P - row0, (), row0=row0)
        whole = run(0)
        for row0 in (37, 13):
            assert int(m[row0 - 1]) == int(m[row0]), "fixture: the slice does not cut a ray's segment"
            assert torch.equal(bits(run(row0)), bits(whole[row0:])), f"{entry} {layout}: from row {row0}"
    del Wt


def test_rolling_the_ray_map_changes_the_colours(nerf, gpu, oracle):
    """A kernel that ignored the index, or read another ray's record, cannot pass the bit comparisons above: with
    distinct random unit view directions per ray, the neighbouring ray's record changes at least one rgb channel in
    at least half of the points, for every entry. Checked on the CPU first, with the oracle's NeRFSmall on the same
    features, weights and directions."""
    import indoor_nerf_amd._lib as L
    P = 4097
    Wt = real_weights(gpu)
    W = weights_struct(L, Wt)
    m, n_rays = ray_maps(P)["segmented"]
    rolled = (m + 1) % n_rays
    dirs = unit_dirs(n_rays, 11)
    x = torch.randn(P, 32, generator=torch.Generator().manual_seed(100 + P)) * 0.5      # features(): the same values
    w = {k: Wt[s].cpu() for k, s in zip(oracle.MLP_KEYS, ("w0", "w1", "c0", "c1", "c2"))}
    cpu = [oracle.mlp_forward(torch.cat([x, oracle.sh4(dirs[torch.from_numpy(i).long()])], -1), w) for i in (m, rolled)]
    cpu_share = float((cpu[0][:, :3] != cpu[1][:, :3]).any(1).float().mean())
    print(f"oracle: rolling the ray map changes rgb in {100 * cpu_share:.2f} % of {P} points")
    assert cpu_share >= 0.5, f"fixture: the CPU network changes only {cpu_share:.3f} of the points"
    rec = records(L, rays_of_dirs(gpu, dirs))
    for entry, _, packed in ENTRIES:
        feat, sp, sl = features(gpu, P, "level", packed)
        raws = [launch(L, entry, W, feat, sp, sl,
                       (L.ptr(rec, "rec"), L.ptr(t, "ray_of", torch.int32), n_rays), None, P, ())
                for t in (torch.from_numpy(m).to(gpu), torch.from_numpy(rolled.astype(np.int32)).to(gpu))]
        share = float((raws[0][:, :3] != raws[1][:, :3]).any(1).float().mean())
        print(f"{entry}: rolling the ray map changes rgb in {100 * share:.2f} % of {P} points")
        assert share >= 0.5, f"{entry}: only {share:.3f} of the points change with the ray map"
        assert torch.equal(bits(raws[0][:, 3]), bits(raws[1][:, 3])), f"{entry}: sigma depends on the view direction"
