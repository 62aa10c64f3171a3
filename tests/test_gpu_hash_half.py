"""The fp16 hash-table entries driven directly (csrc/hashgrid_half.hip), needs an MI355X.

The specification: nerf_hash_tables_to_half rounds every table value once to IEEE binary16 (round to nearest even,
subnormals kept, overflow to inf, NaN stays NaN), and nerf_hash_encode_fwd_half on that image gives, bit for bit, the
features and keep flags of nerf_hash_encode_fwd on the fp32 tables t.half().float(). The rounded tables ("the twin")
are computed on the CPU by torch; the fp32 kernel on the twin is the reference, GPU against GPU, so nothing here has a
tolerance except the bound against the unrounded tables, which is derived below.
"""
import numpy as np
import pytest
import torch

from tables import blender_bbox

pytestmark = pytest.mark.gpu

N_LEVELS = 16
CONVERT, HALF, FP32 = "nerf_hash_tables_to_half", "nerf_hash_encode_fwd_half", "nerf_hash_encode_fwd"
POINTS = (1, 127, 128, 129, 255, 256, 257, 4097, 131105)      # the block and points-per-thread edges of both row kinds
_SETS = {}


def level_res():
    from indoor_nerf_amd.hashgrid import level_resolutions
    return level_resolutions(torch.tensor(16), torch.tensor(1024), N_LEVELS)[0]


def table_set(gpu, log2_T, scale):
    """(fp32 tables, their twins t.half().float() computed on the CPU, the CPU tables), cached per module."""
    key = (log2_T, scale)
    if key not in _SETS:
        g = torch.Generator().manual_seed(1000 * log2_T + int(scale * 1e6))
        cpu = [(torch.rand(1 << log2_T, 2, generator=g) * 2 - 1) * scale for _ in range(N_LEVELS)]
        _SETS[key] = ([t.to(gpu) for t in cpu], [t.half().float().to(gpu) for t in cpu], cpu)
    return _SETS[key]


def convert(L, gpu, tabs, log2_T):
    """The image of `tabs` as the uint8 buffer the entry writes."""
    nbytes = int(L.load().nerf_hash_half_bytes(len(tabs), log2_T))
    assert nbytes == len(tabs) * (1 << log2_T) * 4
    buf = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    L.call(CONVERT, L.ptr_array(tabs), len(tabs), log2_T, L.ptr(buf, "image", dtype=torch.uint8), L.stream())
    return buf


def encode(L, gpu, x, log2_T, tabs=None, image=None, layout="point", with_keep=True, row0=0, rows=None):
    """One launch of the fp32 entry (tabs) or the fp16 entry (image) -> (feat, keep); the points land in rows
    row0 .. row0 + P of buffers of `rows` rows, whose other rows hold a fill that must survive."""
    lo, hi = blender_bbox()
    P = x.shape[0]
    rows = P + row0 if rows is None else rows
    if layout == "point":
        feat, sp, sl = torch.full((rows, 2 * N_LEVELS), 7.0, device=gpu), 2 * N_LEVELS, 2
    else:
        feat, sp, sl = torch.full((N_LEVELS, rows, 2), 7.0, device=gpu), 2, 2 * rows
    keep = torch.full((rows,), True, device=gpu) if with_keep else None
    front = (L.ptr(x, "xyz"), P, L.host_f32(lo), L.host_f32(hi), L.host_f32(level_res()), N_LEVELS, log2_T)
    back = (L.ptr_at(feat, sp * row0, "feat"), sp, sl,
            None if keep is None else L.ptr_at(keep, row0, "keep", dtype=torch.bool), L.stream())
    if image is None:
        L.call(FP32, *front, L.ptr_array(tabs), *back)
    else:
        L.call(HALF, *front, L.ptr(image, "image", dtype=torch.uint8), *back)
    return feat, keep


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def random_points(gpu, n, seed):
    lo, hi = blender_bbox()
    rng = np.random.RandomState(seed)
    return torch.from_numpy((lo - 0.1 + (hi - lo + 0.2) * rng.rand(n, 3)).astype(np.float32)).to(gpu)


# ---------------------------------------------------------------- 1. the conversion
def seeded_values():
    """The values the conversion must get right, as fp32."""
    f = np.float32
    ties = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),      # down to even, up to even
            2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -24 + 2.0 ** -25]                 # ties among subnormals
    near_ties = [np.nextafter(f(1 + 2.0 ** -11), f(2)), np.nextafter(f(1 + 2.0 ** -11), f(0)),
                 np.nextafter(f(2.0 ** -25), f(1)), np.nextafter(f(2.0 ** -25), f(0))]
    subnormal = [6.0e-5, -6.0e-5, 6.1e-5, 3.0e-5, -1.0e-5, 1.0e-6, 5.96e-8, 6.0e-8, 1.0e-8, -1.0e-8, 1.0e-30, 1.0e-45,
                 2.0 ** -14, np.nextafter(f(2.0 ** -14), f(0))]
    edges = [0.0, -0.0, 65504.0, -65504.0, 65519.996, 65520.0, -65520.0, np.nextafter(f(65520), f(0)), 65536.0, 1e30,
             -1e30, np.inf, -np.inf, np.nan, -np.nan]
    return np.array(ties + near_ties + subnormal + edges, np.float32)


@pytest.mark.parametrize("log2_T", [12, 1])
def test_conversion_is_torchs_float16_bit_for_bit(nerf, gpu, log2_T):
    """Every value of a 16-level set: the seeded ones at scattered places (so that they meet every lane position of
    the 16-byte reads), the rest random at the encoder's own +-1e-4 initialisation (partly fp16 subnormals) and at
    +-0.05. log2_T = 1: the tables too small for the 16-byte path."""
    import indoor_nerf_amd._lib as L
    T = 1 << log2_T
    rng = np.random.RandomState(log2_T)
    vals = seeded_values()
    cpu = []
    for lvl in range(N_LEVELS):
        t = ((rng.rand(T, 2) * 2 - 1) * (1e-4 if lvl % 2 else 0.05)).astype(np.float32)
        flat = t.reshape(-1)
        if log2_T > 1:
            at = rng.choice(flat.size, 4 * vals.size, replace=False)
            flat[at] = np.tile(vals, 4)
        else:
            flat[:] = vals[(4 * lvl + np.arange(4)) % vals.size]
        cpu.append(torch.from_numpy(t))
    ref = torch.stack([t.to(torch.float16) for t in cpu])                 # [L, T, 2], round to nearest even
    image = convert(L, gpu, [t.to(gpu) for t in cpu], log2_T)
    got = image.cpu().view(torch.float16).reshape(N_LEVELS, T, 2)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "NaN-ness"
    assert int(nan.sum()) >= (2 if log2_T > 1 else 1)
    a, b = got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan]
    assert torch.equal(a, b), f"{int((a != b).sum())} values differ from torch's float16"
    if log2_T > 1:           # the fixture holds what it claims: subnormals, both infinities, both zeros
        r = ref.float()
        sub = (r != 0) & (r.abs() < 2.0 ** -14)
        assert int(sub.sum()) > 1000 and bool(torch.isinf(r).any()) and bool((r == 65504).any())
        src = torch.stack(cpu)
        assert bool(((r == 0) & (src != 0)).any()), "no value underflows to zero"
        assert bool((torch.isinf(r) & torch.isfinite(src)).any()), "no finite value overflows to inf"


def test_conversion_of_unaligned_tables(nerf, gpu):
    """Tables off a 16-byte boundary take the one-entry-per-lane kernel: the same bits."""
    import indoor_nerf_amd._lib as L
    g = torch.Generator().manual_seed(5)
    base = (torch.rand(N_LEVELS, (1 << 12) + 2, 2, generator=g) * 2 - 1) * 1e-4
    dev = base.to(gpu)
    tabs = [dev[lvl, 1:-1] for lvl in range(N_LEVELS)]         # 8 bytes past a 16-byte boundary
    assert all(t.data_ptr() % 16 == 8 and t.is_contiguous() for t in tabs)
    got = convert(L, gpu, tabs, 12).cpu().view(torch.int16).reshape(N_LEVELS, 1 << 12, 2)
    assert torch.equal(got, base[:, 1:-1].to(torch.float16).view(torch.int16))


# ---------------------------------------------------------------- 2. the features
@pytest.mark.parametrize("scale", [0.05, 1e-4])
@pytest.mark.parametrize("log2_T", [12, 15, 19])
def test_features_are_the_fp32_kernels_on_the_rounded_tables(nerf, gpu, log2_T, scale):
    """log2_T 12 / 15 / 19: no, three and six grouped coarse levels. +-1e-4: subnormals on the gather side."""
    import indoor_nerf_amd._lib as L
    tabs, twins, _ = table_set(gpu, log2_T, scale)
    image = convert(L, gpu, tabs, log2_T)
    differs = False
    for P in POINTS:
        x = random_points(gpu, P, P)
        for layout in ("point", "level"):
            for with_keep in (False, True):
                got, keep = encode(L, gpu, x, log2_T, image=image, layout=layout, with_keep=with_keep)
                ref, ref_keep = encode(L, gpu, x, log2_T, tabs=twins, layout=layout, with_keep=with_keep)
                what = f"log2_T {log2_T} scale {scale} P {P} {layout} keep {with_keep}"
                assert same_bits(got, ref), f"{what}: feat differs in {int((got != ref).sum())} values"
                if with_keep:
                    assert torch.equal(keep, ref_keep), f"{what}: keep"
        if P == POINTS[-1]:
            assert 0.0 < float(keep.float().mean()) < 1.0, "fixture: points on both sides of the box"
            plain, _ = encode(L, gpu, x, log2_T, tabs=tabs, layout="level")
            differs = not same_bits(plain, ref)
    assert differs, "the rounded tables give the unrounded tables' features: the comparison shows nothing"


def edge_points(n=65536):
    """The constructions of test_gpu_parity.test_hash_encode_edge_points_vs_c_oracle at n points, plus NaN
    coordinates: grid vertices of every level, exact box bounds, zero, subnormal, tiny and huge coordinates scattered
    over the waves, runs of zeros and of a subnormal."""
    lo, hi = blender_bbox()
    rng = np.random.RandomState(11)
    x = (lo - 0.3 + (hi - lo + 0.6) * rng.rand(n, 3)).astype(np.float32)
    res = np.asarray(level_res(), np.float32)
    cell = ((hi.astype(np.float32) - lo.astype(np.float32))[None, :] / res[:, None]).astype(np.float32)
    m = n // 4
    lv = rng.randint(0, len(res), m)
    k = np.floor(rng.rand(m, 3) * res[lv][:, None]).astype(np.float32)
    verts = (k * cell[lv] + lo.astype(np.float32)).astype(np.float32)
    axes = rng.rand(m, 3) < 0.6
    x[:m][axes] = verts[axes]
    specials = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, 1e-45, 3e-22, 1e30, -1e30, 1e-6, -1e-6, np.nan, np.inf],
                        np.float32)
    sel = rng.rand(n, 3) < 0.002
    x[sel] = rng.choice(specials, int(sel.sum()))
    for a in range(3):
        b = rng.rand(n) < 0.01
        x[b, a] = np.where(rng.rand(int(b.sum())) < 0.5, lo[a], hi[a]).astype(np.float32)
    x[n - 4096:n - 2048, 1] = 0.0
    x[n - 2048:, 2] = 1e-38
    perm = rng.permutation(n - 4096)
    x[:n - 4096] = x[perm]
    assert np.isnan(x).any() and (x == lo[0]).any()
    return x


def test_edge_points(nerf, gpu):
    """Where the voxel math is most fragile, so that the waves take both division paths: bit for bit the fp32
    kernel on the rounded tables, NaN features included."""
    import indoor_nerf_amd._lib as L
    tabs, twins, _ = table_set(gpu, 19, 0.05)
    image = convert(L, gpu, tabs, 19)
    x = torch.from_numpy(edge_points()).to(gpu)
    got, keep = encode(L, gpu, x, 19, image=image)
    ref, ref_keep = encode(L, gpu, x, 19, tabs=twins)
    assert same_bits(got, ref), f"feat differs in {int((got.view(torch.int32) != ref.view(torch.int32)).sum())} values"
    assert torch.equal(keep, ref_keep)
    assert not bool(keep[torch.isnan(x).any(-1)].any()), "a NaN point is outside the box"


@pytest.mark.parametrize("scale", [0.05, 1e-4])
def test_error_against_the_unrounded_tables(nerf, gpu, scale):
    """Against nerf_hash_encode_fwd on the fp32 tables themselves. A feature is a convex combination of eight
    entries (the trilinear weights are in [0, 1] and sum to 1 up to rounding), so it moves by at most the largest
    rounding error of an entry of its level: half an fp16 ulp, at most 2^-11 M_l for a normal and 2^-25 for a
    subnormal result, M_l the level's largest |entry|. Both kernels then do the same seven fp32 blends, each within
    half an fp32 ulp of a value of magnitude at most M_l (1 + 2^-20): 8 ulp(M_l) covers both sides' rounding.
        |feat_half - feat_fp32| <= max(2^-11 M_l, 2^-25) + 8 ulp(M_l)
    Only points inside the box: outside it the weights leave [0, 1]."""
    import indoor_nerf_amd._lib as L
    tabs, twins, cpu = table_set(gpu, 19, scale)
    if scale == 0.05:
        # a random fp32 value fits fp16's 11 significant bits with chance 2^-13: nearly every entry is changed, so the
        # equality with the twin above cannot be met by a kernel that reads the fp32 tables
        changed = np.mean([float((t.half().float() != t).float().mean()) for t in cpu])
        assert changed >= 0.99, f"only {changed:.4f} of the entries are changed by the rounding"
    image = convert(L, gpu, tabs, 19)
    x = random_points(gpu, 131105, 77)
    got, keep = encode(L, gpu, x, 19, image=image, layout="level")
    ref, _ = encode(L, gpu, x, 19, tabs=tabs, layout="level")
    assert int(keep.sum()) > 65536
    err = (got.double() - ref.double()).abs()[:, keep].amax(dim=(1, 2)).cpu().numpy()
    for lvl in range(N_LEVELS):
        M = float(cpu[lvl].abs().max())
        bound = max(2.0 ** -11 * M, 2.0 ** -25) + 8 * float(np.spacing(np.float32(M)))
        print(f"scale {scale} level {lvl}: max |d feat| = {err[lvl]:.3e}, bound {bound:.3e}")
        assert err[lvl] <= bound, f"level {lvl}: {err[lvl]:.3e} > {bound:.3e}"
    assert err.max() > 0


def test_slices_and_row_offsets_give_the_same_bits(nerf, gpu):
    """The same 4,097 points in one launch, in slices of 37, and shifted by 13 rows of the buffers: a point's result
    does not depend on its launch or its row, and the rows outside a launch keep their contents."""
    import indoor_nerf_amd._lib as L
    tabs, _, _ = table_set(gpu, 19, 0.05)
    image = convert(L, gpu, tabs, 19)
    P = 4097
    x = random_points(gpu, P, 4097)
    for layout in ("point", "level"):
        whole, keep = encode(L, gpu, x, 19, image=image, layout=layout)
        shifted, skeep = encode(L, gpu, x, 19, image=image, layout=layout, row0=13, rows=P + 20)
        rows = (lambda t: t) if layout == "point" else (lambda t: t.transpose(0, 1))
        assert same_bits(rows(shifted)[13:13 + P], rows(whole)), f"{layout}: rows shifted by 13"
        assert torch.equal(skeep[13:13 + P], keep)
        for edge in (rows(shifted)[:13], rows(shifted)[13 + P:]):
            assert bool((edge == 7.0).all()), f"{layout}: a row outside the launch was written"
        parts = [encode(L, gpu, x[s:s + 37].contiguous(), 19, image=image, layout=layout) for s in range(0, P, 37)]
        cat = torch.cat([rows(f) for f, _ in parts])
        assert same_bits(cat, rows(whole).contiguous()), f"{layout}: slices of 37"
        assert torch.equal(torch.cat([k for _, k in parts]), keep)


def test_embedder_route(nerf, gpu):
    """HashEmbedder.encode_into(half=True): the cached image, built once, and the entry above; row0 as for fp32."""
    import indoor_nerf_amd._lib as L
    lo, hi = blender_bbox()
    emb = nerf.HashEmbedder((torch.from_numpy(lo), torch.from_numpy(hi)), finest_resolution=1024,
                            log2_hashmap_size=15).to(gpu).eval()
    tabs, _, _ = table_set(gpu, 15, 0.05)
    with torch.no_grad():
        for e, t in zip(emb.embeddings, tabs):
            e.weight.copy_(t)
    x = random_points(gpu, 257, 3)
    ref, ref_keep = encode(L, gpu, x, 15, image=convert(L, gpu, tabs, 15), layout="level", row0=5)
    feat, keep = torch.full((N_LEVELS, 262, 2), 7.0, device=gpu), torch.full((262,), True, device=gpu)
    with torch.no_grad():
        emb.encode_into(x, feat, 2, 2 * 262, keep, row0=5, half=True)
        buf = emb.half_tables()
        assert emb.half_tables() is buf and buf.dtype == torch.uint8 and buf.numel() == N_LEVELS * (1 << 15) * 4
    assert same_bits(feat, ref) and torch.equal(keep, ref_keep)
    assert not any("half" in k for k in emb.state_dict())
