"""The jittered walk of the grid march at kernel level (nerf_jitter_march_count / nerf_jitter_march_write; DESIGN.md
§25), needs an MI355X.

The yardstick is made of entries the project already trusts, so every comparison is bit for bit: the dense jittered
depths and points of nerf_sample_stratified(lindisp=0, perturb=1) over the same rays, table and uniforms, the answer
of nerf_occ_query on those points, and the kept entries in row-major order: z, pts, z[k + 1] - z[k] of the dense row
(1e10 for the last lattice sample), the counts and their exclusive scan. The SH rows are the ray's record
(nerf_ray_sh_records) and, where the plain march keeps a sample of the same ray, nerf_march_write's row of that ray;
the ray indices are arange.

Shapes at the walk's edges: K in {1, 2, 3, 63, 64, 65, 130, 4096} (below, at and above one 64-wide iteration, two
iterations and a ragged third, the largest lattice) for R in {1, 5, 257} (four rays per block: one block not full,
two blocks, 65 blocks), and 4097 rays at K = 3 (one past a compaction block of 4096 rays). At K = 3, 63 and 65 the
Philox groups of four indices straddle rays. The rays are six hand-made rows (test_gpu_march.py's) and the scene's two
frames, tiled. The uniforms come from an explicit array (u = 0 and the largest float below 1 in every stratum: where
(r + k) % 3 is 0 and 1), from a host (seed, offset) pair with both above 2^32, and from the same pair in device
memory."""
import numpy as np
import pytest
import torch

from forward_only import ball_mask, bits_equal, build_scene, np_query, random_mask
from test_gpu_march import hand_rays

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(R, K) for K in (1, 2, 3, 63, 64, 65, 130, 4096) for R in (1, 5, 257)] + [(4097, 3)]
MASKS = {"ball": ball_mask, "random": lambda: random_mask(16), "full": lambda: np.ones((16, 16, 16), bool),
         "empty": lambda: np.zeros((16, 16, 16), bool)}
SOURCES = ("array", "host", "device")
SEED, OFFSET = (1 << 40) + 12345, (1 << 33) + 7
CPU_POINTS = 257 * 4096     # the precondition is checked from the mask in NumPy up to this many lattice samples
SENTINEL = -7.25
EXTRA = 7                   # rows behind the list's end; the capacity covers 3 of them


@pytest.fixture(scope="module")
def scene(nerf, gpu):
    sc = build_scene(nerf, gpu)
    hand = hand_rays(sc["lo"], sc["hi"])
    vd = hand[:, 3:6] / np.linalg.norm(hand[:, 3:6], axis=-1, keepdims=True)
    frames = np.concatenate([sc["packed"](i).cpu().numpy() for i in (0, 1)])
    pool = np.concatenate([np.concatenate([hand, vd.astype(f32)], -1), frames]).astype(f32)
    return dict(sc, pool=pool, dense={}, grids={})


def rays_of(scene, gpu, R):
    pool = scene["pool"]
    return torch.from_numpy(np.ascontiguousarray(np.tile(pool, (R // len(pool) + 1, 1))[:R])).to(gpu)


def uniforms(gpu, source, R, K):
    """(u or None, seed, offset, the device pair or None) as the entries take them, and the tensors to keep alive."""
    if source == "array":
        u = np.random.default_rng(1000 * K + R).random((R, K)).astype(f32)
        rk = np.arange(R)[:, None] + np.arange(K)[None, :]
        u[rk % 3 == 0] = 0.0
        u[rk % 3 == 1] = np.nextafter(f32(1.0), f32(0.0))
        return (torch.from_numpy(u).to(gpu), 0, 0, None)
    if source == "host":
        return (None, SEED, OFFSET, None)
    return (None, 1, 2, torch.tensor([SEED, OFFSET], dtype=torch.int64, device=gpu))      # the host pair must lose


def dense_reference(scene, gpu, source, R, K):
    """nerf_sample_stratified(perturb=1) over the shape: rays, the uniforms, z [R, K], pts [R, K, 3], dist [R, K].
    Computed once per (source, shape) and shared by the grids."""
    from indoor_nerf_amd import _lib as L
    from indoor_nerf_amd.render import _linspace
    key = (source, R, K)
    if key not in scene["dense"]:
        rays = rays_of(scene, gpu, R)
        jit = uniforms(gpu, source, R, K)
        z = torch.empty(R, K, device=gpu)
        pts = torch.empty(R, K, 3, device=gpu)
        L.call("nerf_sample_stratified", L.ptr(rays), 11, R, K, L.ptr(_linspace(K, gpu)), 0, 1,
               L.ptr(jit[0], "u", allow_none=True), jit[1], jit[2],
               None if jit[3] is None else L.ptr(jit[3], "rng", torch.int64), L.ptr(z), L.ptr(pts), None, None,
               L.stream())
        dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=gpu)], -1)
        scene["dense"][key] = (rays, jit, z, pts, dist)
    return scene["dense"][key]


def grid_of(scene, name):
    if name not in scene["grids"]:
        scene["grids"][name] = (MASKS[name](), scene["grid_of"](MASKS[name]()))
    return scene["grids"][name]


def jitter_lists(grid, rays, K, jit, index, C=11):
    """The two entries driven directly: the count, one host read, and the write into buffers that hold EXTRA rows of
    SENTINEL behind the list, with a capacity that covers three of them.
    -> counts, offsets, rays_d, n, pts_c, z_c, dist_c, last (SH rows, or ray indices with index)."""
    from indoor_nerf_amd import _lib as L
    from indoor_nerf_amd.render import _linspace
    rays = rays[:, :C].contiguous()
    R, dev = rays.shape[0], rays.device
    i32, f = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    t = _linspace(K, dev)
    counts, offsets, rays_d = torch.full((R,), -1, **i32), torch.full((R + 1,), -1, **i32), torch.empty(R, 3, **f)
    ws = torch.empty(int(L.load().nerf_march_workspace_bytes(R)) // 4, **i32)
    u, seed, off, rng = jit
    uni = (L.ptr(u, "u", allow_none=True), seed, off, None if rng is None else L.ptr(rng, "rng", torch.int64))
    front = (L.ptr(rays), R, C, L.ptr(t), K, grid._bmin, grid._bmax, grid.resolution, grid._bits())
    L.call("nerf_jitter_march_count", *front, L.ptr(counts, "counts", torch.int32),
           L.ptr(offsets, "offsets", torch.int32), L.ptr(rays_d), L.ptr(ws, "ws", torch.int32), ws.numel() * 4, *uni,
           L.stream())
    n = int(offsets[R].item())
    pts_c, z_c, dist_c = (torch.full((n + EXTRA,) + s, SENTINEL, **f) for s in ((3,), (), ()))
    last = torch.full((n + EXTRA,), -9, **i32) if index else torch.full((n + EXTRA, 16), SENTINEL, **f)
    sh_ptr, ray_ptr = (None, L.ptr(last, "ray_c", torch.int32)) if index else (L.ptr(last, "sh_c"), None)
    L.call("nerf_jitter_march_write", *front, L.ptr(counts, "counts", torch.int32),
           L.ptr(offsets, "offsets", torch.int32), n, n + 3, L.ptr(pts_c), L.ptr(z_c), L.ptr(dist_c), sh_ptr, ray_ptr,
           *uni, L.stream())
    return counts, offsets, rays_d, n, pts_c, z_c, dist_c, last


def assert_list_is_the_reference(got, ref, keep, what, index, rec):
    counts, offsets, rays_d, n, pts_c, z_c, dist_c, last = got
    rays, _, z, pts, dist = ref
    R = rays.shape[0]
    want_counts = keep.sum(-1).to(torch.int32)
    assert torch.equal(counts, want_counts), f"{what}: counts"
    want_off = torch.cat([torch.zeros(1, device=keep.device, dtype=torch.int64), want_counts.long().cumsum(0)])
    assert torch.equal(offsets.long(), want_off), f"{what}: offsets"
    assert n == int(keep.sum()), f"{what}: n"
    assert bits_equal(rays_d, rays[:, 3:6]), f"{what}: rays_d"
    assert bits_equal(z_c[:n], z[keep]), f"{what}: z_c"
    assert bits_equal(pts_c[:n], pts[keep]), f"{what}: pts_c"
    assert bits_equal(dist_c[:n], dist[keep]), f"{what}: dist_c"
    ray_of = torch.arange(R, device=keep.device)[:, None].expand_as(keep)[keep]
    if index:
        assert torch.equal(last[:n].long(), ray_of), f"{what}: ray_c"
        assert bool((last[n:] == -9).all()), f"{what}: ray_c written behind the list"
    else:
        assert bits_equal(last[:n], rec[ray_of, :16].contiguous()), f"{what}: sh_c"
        assert bool((last[n:] == SENTINEL).all()), f"{what}: sh_c written behind the list"
    for name, buf in (("pts_c", pts_c), ("z_c", z_c), ("dist_c", dist_c)):
        assert bool((buf[n:] == SENTINEL).all()), f"{what}: {name} written behind the list"


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", list(MASKS))
def test_lists_are_the_dense_sampler_s_kept_entries(nerf, gpu, scene, name, source):
    mask, grid = grid_of(scene, name)
    lo, hi = scene["lo"], scene["hi"]
    mixed_shapes, mixed_at = 0, {K: [] for _, K in SHAPES if K >= 63}
    for R, K in SHAPES:
        ref = dense_reference(scene, gpu, source, R, K)
        rays, jit, z, pts, _ = ref
        keep = grid.query(pts)
        what = f"{name} {source} R {R} K {K}"
        if R * K <= CPU_POINTS:
            # the precondition, from the mask: some ray has a kept and a skipped sample in one 64-wide iteration
            keep_np = np_query(pts.cpu().numpy().reshape(-1, 3), lo, hi, mask).reshape(R, K)
            assert np.array_equal(keep_np, keep.cpu().numpy()), f"{what}: nerf_occ_query against the mask"
            pad = np.zeros((R, -K % 64), bool)
            it = np.concatenate([keep_np, pad], -1).reshape(R, -1, 64)
            live = (np.concatenate([np.ones((R, K), bool), pad], -1).reshape(R, -1, 64)).sum(-1)
            mixed = bool(((it.sum(-1) > 0) & (it.sum(-1) < live)).any())
            mixed_shapes += mixed
            if mixed and K >= 63:
                mixed_at[K].append(R)
            # asked of the shapes with the frames' rays: of the hand-made rows only row 0 leaves the ball, at a cell
            # face that at K = 4096 lies next to lattice sample 512, the first of an iteration, so whether one of
            # its iterations is mixed hangs on that sample's jitter
            if name in ("ball", "random") and K >= 63 and R == 257:
                assert mixed, f"fixture {what}: no iteration with a kept and a skipped sample"
            if name == "full" and K >= 63:
                assert mixed, f"fixture {what}: no ray leaves the box"
            if name == "empty":
                assert not keep_np.any()
        if source == "array":      # the strata's two ends are in the array, at every k (from three rays on)
            u = jit[0]
            top = float(np.nextafter(f32(1.0), f32(0.0)))
            assert bool((u == 0).any()) and (R * K < 2 or bool((u == top).any()))
            if R >= 3:
                assert bool((u == 0).any(0).all()) and bool((u == u.max()).any(0).all()) and float(u.max()) < 1.0
        rec = nerf.OccupancyGrid._ray_sh_records(rays)
        for index in (False, True):
            got = jitter_lists(grid, rays, K, jit, index)
            assert_list_is_the_reference(got, ref, keep, f"{what} index {index}", index, rec)
        if (R, K) in ((5, 65), (257, 3)):      # rows without view directions carry a ray index
            got = jitter_lists(grid, rays, K, jit, True, C=8)
            assert_list_is_the_reference(got, ref, keep, f"{what} C 8", True, rec)
    print(f"{name} {source}: {mixed_shapes} shapes with a kept and a skipped sample in one iteration")
    assert (mixed_shapes > 0) == (name != "empty")
    if name in ("ball", "random"):      # at every K of an iteration or more, the reference list of some R is non-trivial
        assert all(mixed_at.values()), f"fixture {name} {source}: mixed iterations at K -> R {mixed_at}"


@pytest.mark.parametrize("name", ["ball", "random"])
def test_the_jitter_moves_the_list_and_repeats(nerf, gpu, scene, name):
    """The jittered list differs from the plain one (the comparison above is not one of two unjittered lists), two
    seeds differ, and the same call twice gives the same bits; the SH rows are nerf_march_write's of the same ray."""
    _, grid = grid_of(scene, name)
    R, K = 257, 130
    rays = rays_of(scene, gpu, R)
    a = jitter_lists(grid, rays, K, (None, SEED, OFFSET, None), False)
    b = jitter_lists(grid, rays, K, (None, SEED, OFFSET, None), False)
    c = jitter_lists(grid, rays, K, (None, SEED + 1, OFFSET, None), False)
    for x, y in zip(a, b):
        assert (x == y) if isinstance(x, int) else bits_equal(x, y)
    assert a[3] > 0 and not (a[3] == c[3] and bits_equal(a[5], c[5]))
    counts, offsets, pts_c, z_c, dist_c, sh_c = grid.march(rays, K)
    assert not (a[3] == int(offsets[-1]) and bits_equal(a[5][:a[3]], z_c))
    both = ((counts > 0) & (a[0] > 0)).nonzero().reshape(-1)
    assert both.numel() > 10
    for r in both.tolist()[:64]:
        row = sh_c[int(offsets[r])]
        seg = a[7][int(a[1][r]):int(a[1][r + 1])]
        assert bits_equal(seg, row.expand_as(seg).contiguous()), f"ray {r}: SH rows"


def test_the_unjittered_entries_keep_their_bits(nerf, gpu, scene):
    """nerf_march_count and nerf_march_write before and after a jittered call over the same buffers' shapes."""
    _, grid = grid_of(scene, "random")
    R, K = 257, 130
    rays = rays_of(scene, gpu, R)
    before = grid.march(rays, K)
    jitter_lists(grid, rays, K, (None, SEED, OFFSET, None), False)
    jitter_lists(grid, rays, K, (None, SEED, OFFSET, None), True)
    after = grid.march(rays, K)
    assert int(before[1][-1]) > 0
    for x, y in zip(before, after):
        assert bits_equal(x, y)
