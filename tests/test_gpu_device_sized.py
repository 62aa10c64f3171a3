"""The launches sized on the device, driven through the C entries (csrc/hashgrid_pkbf.hip
hash_encode_fwd_pkbf_dev_kernel, csrc/field_x6.hip mlp_fwd_bf16_kernel<true, ray index, DevCount>), needs
an MI355X.

The specification has no tolerance. Each _dev entry takes (d_total, base, capacity) where its host-sized twin takes
n_points and covers n = clamp(*d_total - base, 0, capacity) points: the first n entries of every output are, in every
bit, the twin's at n_points = n, and every entry at or beyond n still holds the sentinel its buffer was filled with.
The totals below hit both ends of the clamp (total < base, a negative total, total > base + capacity) and its middle.
The points beyond n are NaN: they are not points of the launch and nothing may come of them.
"""
import ctypes

import pytest
import torch

from tables import blender_bbox
from test_gpu_feat_bf16 import FILL, bits, encode_pk, real_weights
from test_gpu_hash_half import N_LEVELS, convert, level_res, random_points, table_set
from test_gpu_march_sh import rays_of_dirs, records, unit_dirs
from test_gpu_mlp_bf16 import weights_struct

pytestmark = pytest.mark.gpu

ENC_POINTS = (0, 1, 127, 128, 129, 257, 4097)
MLP_POINTS = (0, 1, 31, 32, 33, 257, 4097)
BIG = 131105
KEEP_FILL = 7
N_RAYS = 37
DEV = {False: "nerf_hash_encode_fwd_pkbf_dev", True: "nerf_hash_encode_fwd_half_pkbf_dev"}
MLP, MLP_DEV = "nerf_mlp_fwd_bf16_pkbf_rays", "nerf_mlp_fwd_bf16_pkbf_rays_dev"


def cases(n):
    """(capacity, base, total) of every launch at count n: capacities n, n + 1 and 2 n + 300, bases 0 and 37; the
    total that gives n exactly and, where the capacity is n, one beyond base + capacity (the upper clamp); at n = 0
    also a total below the base and a negative one (the lower clamp)."""
    out = []
    for cap in (n, n + 1, 2 * n + 300):
        for base in (0, 37):
            out.append((cap, base, base + n))
            if cap == n:
                out.append((cap, base, base + n + 5))
            if n == 0:
                out += [(cap, base, base - 30), (cap, base, -3)]
    return out


def total_of(gpu, value):
    return torch.tensor([value], device=gpu, dtype=torch.int32)


# ---------------------------------------------------------------- 1. the encoder
@pytest.fixture(scope="module")
def sources(gpu):
    """log2_T -> (tables, fp16 image), and the 4,097 points every count is a prefix of."""
    import indoor_nerf_amd._lib as L
    out = {}
    for log2_T in (12, 19):
        tabs, _, _ = table_set(gpu, log2_T, 0.05)
        out[log2_T] = (tabs, convert(L, gpu, tabs, log2_T))
    return out, random_points(gpu, 4097, 4097)


def encode_dev(L, gpu, x, n, cap, base, total, log2_T, tabs=None, image=None, max_blocks=0):
    """One _dev launch over a buffer of `cap` points whose first n are x[:n] -> (words int32 [16, cap], keep uint8
    [cap]), level stride = capacity."""
    lo, hi = blender_bbox()
    pts = torch.full((cap, 3), float("nan"), device=gpu)
    pts[:n] = x[:n]
    words = torch.full((N_LEVELS, cap), FILL, device=gpu, dtype=torch.int32)
    keep = torch.full((cap,), KEEP_FILL, device=gpu, dtype=torch.uint8)
    d_total = total_of(gpu, total)
    src = L.ptr_array(tabs) if image is None else L.ptr(image, "image", dtype=torch.uint8)
    L.call(DEV[image is not None], L.ptr(pts, "xyz", allow_none=True) if cap else None,
           L.ptr(d_total, "total", torch.int32), base, cap, max_blocks, L.host_f32(lo), L.host_f32(hi),
           L.host_f32(level_res()), N_LEVELS, log2_T, src, L.ptr(words, "words", torch.int32) if cap else None, 1, cap,
           L.ptr(keep, "keep", torch.uint8) if cap else None, L.stream())
    return words, keep


def assert_encoded(words, keep, ref, ref_keep, n, what):
    assert torch.equal(words[:, :n], ref[:, :n]), f"{what}: words"
    assert torch.equal(keep[:n], ref_keep[:n].to(torch.uint8)), f"{what}: keep"
    assert bool((words[:, n:] == FILL).all()), f"{what}: a word at or beyond n was written"
    assert bool((keep[n:] == KEEP_FILL).all()), f"{what}: a keep byte at or beyond n was written"


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("log2_T", [12, 19])
def test_encoder_equals_the_host_sized_entry(nerf, gpu, sources, log2_T, half):
    import indoor_nerf_amd._lib as L
    by_T, x = sources
    tabs, image = by_T[log2_T]
    src = dict(image=image) if half else dict(tabs=tabs)
    ref, ref_keep = encode_pk(L, gpu, x, log2_T, layout="level", **src)       # a point's words do not depend on n
    launches = 0
    for n in ENC_POINTS:
        if n:   # ... which is asserted, not assumed: the host-sized entry at this n
            at_n, keep_n = encode_pk(L, gpu, x[:n].contiguous(), log2_T, layout="level", **src)
            assert torch.equal(at_n, ref[:, :n]) and torch.equal(keep_n, ref_keep[:n])
        for cap, base, total in cases(n):
            words, keep = encode_dev(L, gpu, x, n, cap, base, total, log2_T, **src)
            assert_encoded(words, keep, ref, ref_keep, n, f"log2_T {log2_T} half {half} n {n} cap {cap} base {base} "
                                                          f"total {total}")
            launches += 1
    assert launches >= 6 * len(ENC_POINTS)
    assert bool(ref_keep.any()) and not bool(ref_keep.all()), "fixture: keep is constant"


@pytest.mark.parametrize("half", [False, True])
def test_encoder_grid_stride_and_large_capacity(nerf, gpu, sources, half):
    """n = 4,097 under grids of 1 and 3 blocks (the virtual-block loop and its wrap; the host-sized grid is 289
    blocks) and the default grid, and once in a capacity of 131,105 points, whose default grid is far larger than
    the blocks of 4,097 points."""
    import indoor_nerf_amd._lib as L
    by_T, x = sources
    tabs, image = by_T[19]
    src = dict(image=image) if half else dict(tabs=tabs)
    ref, ref_keep = encode_pk(L, gpu, x, 19, layout="level", **src)
    for max_blocks in (1, 3, 0):
        for cap, base in ((4097, 0), (4400, 37)):
            words, keep = encode_dev(L, gpu, x, 4097, cap, base, base + 4097, 19, max_blocks=max_blocks, **src)
            assert_encoded(words, keep, ref, ref_keep, 4097, f"half {half} max_blocks {max_blocks} cap {cap}")
    words, keep = encode_dev(L, gpu, x, 4097, BIG, 37, 37 + 4097, 19, **src)
    assert_encoded(words, keep, ref, ref_keep, 4097, f"half {half} capacity {BIG}")
    words, keep = encode_dev(L, gpu, x, 0, BIG, 37, 12, 19, **src)
    assert_encoded(words, keep, ref, ref_keep, 0, f"half {half} capacity {BIG}, empty")


# ---------------------------------------------------------------- 2. the MLP
@pytest.fixture(scope="module")
def mlp_inputs(gpu, sources):
    """4,097 points' packed words [16, 4097], keep flags, ray indices into 37 records, and the weights."""
    import indoor_nerf_amd._lib as L
    by_T, x = sources
    words, _ = encode_pk(L, gpu, x, 19, tabs=by_T[19][0], layout="level")
    g = torch.Generator().manual_seed(5)
    keep = (torch.rand(4097, generator=g) < 0.5).to(gpu)
    ray_of = torch.randint(0, N_RAYS, (4097,), generator=g, dtype=torch.int32).to(gpu)
    rec = records(L, rays_of_dirs(gpu, unit_dirs(N_RAYS, 9)))
    return words, keep, ray_of, rec, real_weights(gpu)


def mlp_host(L, gpu, inputs, n, with_keep):
    words, keep, ray_of, rec, W = inputs
    raw = torch.full((n, 4), float("nan"), device=gpu)
    w = words[:, :n].contiguous()
    L.call(MLP, L.ptr(w, "words", torch.int32) if n else None, 1, n, L.ptr(rec, "rec"),
           L.ptr(ray_of, "ray_of", torch.int32), N_RAYS, L.ptr(keep, "keep", torch.bool) if with_keep else None, n,
           ctypes.byref(weights_struct(L, W)), L.ptr(raw, "raw") if n else None, L.stream())
    return raw


def mlp_dev(L, gpu, inputs, n, cap, base, total, with_keep):
    words, keep, ray_of, rec, W = inputs
    w = torch.full((N_LEVELS, cap), FILL, device=gpu, dtype=torch.int32)
    w[:, :n] = words[:, :n]
    k = torch.ones(cap, device=gpu, dtype=torch.bool)
    k[:n] = keep[:n]
    r = torch.zeros(cap, device=gpu, dtype=torch.int32)      # beyond n: a valid index, were it read
    r[:n] = ray_of[:n]
    raw = torch.full((cap, 4), float("nan"), device=gpu)
    d_total = total_of(gpu, total)
    L.call(MLP_DEV, L.ptr(w, "words", torch.int32) if cap else None, 1, cap, L.ptr(rec, "rec"),
           L.ptr(r, "ray_of", torch.int32) if cap else None, N_RAYS,
           L.ptr(k, "keep", torch.bool) if with_keep and cap else None, L.ptr(d_total, "total", torch.int32), base, cap,
           ctypes.byref(weights_struct(L, W)), L.ptr(raw, "raw") if cap else None, L.stream())
    return raw


@pytest.mark.parametrize("with_keep", [False, True])
def test_mlp_equals_the_host_sized_entry(nerf, gpu, mlp_inputs, with_keep):
    import indoor_nerf_amd._lib as L
    nan_bits = bits(torch.full((1, 4), float("nan"), device=gpu))
    for n in MLP_POINTS:
        ref = mlp_host(L, gpu, mlp_inputs, n, with_keep)
        assert bool(torch.isfinite(ref).all())
        extra = [(BIG, 37, 37 + n)] if n == 4097 else []
        for cap, base, total in cases(n) + extra:
            raw = mlp_dev(L, gpu, mlp_inputs, n, cap, base, total, with_keep)
            what = f"keep {with_keep} n {n} cap {cap} base {base} total {total}"
            assert torch.equal(bits(raw[:n]), bits(ref)), \
                f"{what}: {int((bits(raw[:n]) != bits(ref)).any(1).sum())} rows differ from the host-sized raw"
            assert bool((bits(raw[n:]) == nan_bits).all()), f"{what}: a row at or beyond n was written"
    if with_keep:
        plain = mlp_host(L, gpu, mlp_inputs, 4097, False)
        assert not torch.equal(bits(plain), bits(ref)), "fixture: keep changes nothing"
