"""Packed bf16 hash features driven through the C entries (csrc/hashgrid_pkbf.hip, csrc/field_x6.hip
mlp_fwd_bf16_kernel<true>), needs an MI355X.

The specification has no tolerance. nerf_hash_encode_fwd_pkbf / nerf_hash_encode_fwd_half_pkbf write, per (point,
level), the word {bf16_rne(f0), bf16_rne(f1)} of exactly the fp32 features the unpacked entry writes, and
nerf_mlp_fwd_bf16_pkbf on those words gives, in every bit of raw, nerf_mlp_fwd_bf16 on the fp32 features. The encoder
is compared with torch's float32 -> bfloat16 on the CPU (round to nearest even) over values in the normal range (and
zero); NaN features are compared as NaN-ness. The MLP comparison is the same conversion instruction at both sites.
"""
import ctypes

import numpy as np
import pytest
import torch

from tables import blender_bbox
from test_gpu_hash_half import N_LEVELS, POINTS, convert, edge_points, encode, level_res, random_points, table_set
from test_gpu_mlp_bf16 import SHAPES, exact, weights_struct  # noqa: F401  (exact: a module-scoped fixture)

pytestmark = pytest.mark.gpu

PK, HALF_PK, MLP, MLP_PK = ("nerf_hash_encode_fwd_pkbf", "nerf_hash_encode_fwd_half_pkbf", "nerf_mlp_fwd_bf16",
                            "nerf_mlp_fwd_bf16_pkbf")
FILL = 0x07070707
MLP_POINTS = (1, 31, 32, 33, 257, 4097, 131105)


# ---------------------------------------------------------------- drivers and references
def encode_pk(L, gpu, x, log2_T, tabs=None, image=None, layout="point", with_keep=True, row0=0, rows=None):
    """test_gpu_hash_half.encode for the packed entries -> (words int32, keep): "point" [rows, 16] with word strides
    (16, 1), "level" [16, rows] with (1, rows)."""
    lo, hi = blender_bbox()
    P = x.shape[0]
    rows = P + row0 if rows is None else rows
    if layout == "point":
        words, sp, sl = torch.full((rows, N_LEVELS), FILL, device=gpu, dtype=torch.int32), N_LEVELS, 1
    else:
        words, sp, sl = torch.full((N_LEVELS, rows), FILL, device=gpu, dtype=torch.int32), 1, rows
    keep = torch.full((rows,), True, device=gpu) if with_keep else None
    front = (L.ptr(x, "xyz"), P, L.host_f32(lo), L.host_f32(hi), L.host_f32(level_res()), N_LEVELS, log2_T)
    back = (L.ptr_at(words, sp * row0, "words", dtype=torch.int32), sp, sl,
            None if keep is None else L.ptr_at(keep, row0, "keep", dtype=torch.bool), L.stream())
    if image is None:
        L.call(PK, *front, L.ptr_array(tabs), *back)
    else:
        L.call(HALF_PK, *front, L.ptr(image, "image", dtype=torch.uint8), *back)
    return words, keep


def as_entries(feat, layout):
    """The unpacked features of encode() as [..., 2] in the shape of the packed words."""
    return feat.view(feat.shape[0], N_LEVELS, 2) if layout == "point" else feat


def torch_halves(feat):
    """float32 [..., 2] -> what the words must hold, as int16 halves [..., 2] (torch on the CPU, round to nearest
    even), the NaN mask, and the mask of values the comparison covers (zero or normal range, not NaN)."""
    f = feat.detach().cpu()
    ref = f.to(torch.bfloat16).view(torch.int16)
    nan = torch.isnan(f)
    covered = ~nan & ((f == 0) | (f.abs() >= 2.0 ** -126))
    return ref, nan, covered


def assert_words(words, feat, layout, what):
    """words == pk(feat) in every covered half, NaN where feat is NaN; -> the share of features the rounding moved."""
    f = as_entries(feat, layout)
    ref, nan, covered = torch_halves(f)
    got = words.cpu().contiguous().view(torch.int16).reshape(ref.shape)      # little endian: half 0 is f0
    got_nan = torch.isnan(got.view(torch.bfloat16).float())
    assert torch.equal(got_nan, nan), f"{what}: NaN-ness"
    assert float((covered | nan).float().mean()) > 0.999, f"{what}: the fixture's features are subnormal"
    bad = (got != ref) & covered
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} halves differ from torch's bfloat16"
    fc = f.cpu()
    return float(((fc.to(torch.bfloat16).float() != fc) & covered).float().mean())


def widen(words, layout):
    """The words as the fp32 features they stand for, in encode()'s unpacked shape of that layout."""
    w = words.contiguous()
    f = torch.stack([(w << 16).view(torch.float32), (w & -65536).view(torch.float32)], -1)
    return f.reshape(f.shape[0], 2 * N_LEVELS).contiguous() if layout == "point" else f.contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- 1. the encoder on fp32 tables
@pytest.mark.parametrize("scale", [0.05, 1e-4])
@pytest.mark.parametrize("log2_T", [12, 15, 19])
def test_words_are_the_rounded_features(nerf, gpu, log2_T, scale):
    """Every point count of the fp32 test (the block's 128 points and the row's 256, each +- 1, a multi-block odd
    count), both layouts, with and without keep. On the +-0.05 tables nearly every feature is moved by the rounding,
    so a kernel that truncated, or stored something else, cannot pass."""
    import indoor_nerf_amd._lib as L
    tabs, _, _ = table_set(gpu, log2_T, scale)
    moved = []
    for P in POINTS:
        x = random_points(gpu, P, P)
        for layout in ("point", "level"):
            for with_keep in (False, True):
                ref, ref_keep = encode(L, gpu, x, log2_T, tabs=tabs, layout=layout, with_keep=with_keep)
                words, keep = encode_pk(L, gpu, x, log2_T, tabs=tabs, layout=layout, with_keep=with_keep)
                what = f"log2_T {log2_T} scale {scale} P {P} {layout} keep {with_keep}"
                moved.append(assert_words(words, ref, layout, what))
                if with_keep:
                    assert torch.equal(keep, ref_keep), f"{what}: keep"
    print(f"log2_T {log2_T} scale {scale}: the rounding moves {100 * min(moved):.2f} % of the features at least")
    if scale == 0.05:
        assert moved[-1] >= 0.99, f"only {moved[-1]:.4f} of the features change under the rounding"


def test_edge_points(nerf, gpu):
    """test_gpu_hash_half's 65,536 edge points (box faces, grid vertices, NaN and inf coordinates): both division
    paths run, NaN features stay NaN."""
    import indoor_nerf_amd._lib as L
    tabs, _, _ = table_set(gpu, 19, 0.05)
    x = torch.from_numpy(edge_points()).to(gpu)
    for layout in ("point", "level"):
        ref, ref_keep = encode(L, gpu, x, 19, tabs=tabs, layout=layout)
        words, keep = encode_pk(L, gpu, x, 19, tabs=tabs, layout=layout)
        assert_words(words, ref, layout, f"edge points {layout}")
        assert torch.equal(keep, ref_keep)
        assert bool(torch.isnan(ref).any()), "fixture: no NaN feature"
    assert not bool(keep[torch.isnan(x).any(-1)].any())


def test_ties_round_to_even(nerf, gpu):
    """Tables that hold only +-257 2^k and +-259 2^k, points on grid vertices: where all three weights are exactly 0
    the feature is one table entry, an exact bf16 tie. 257 2^k -> 256 2^k (down to even), 259 2^k -> 260 2^k (up to
    even), for both signs and in both halves of the word: truncation, round-half-up and round-half-away each miss
    one of them."""
    import indoor_nerf_amd._lib as L
    log2_T, T = 15, 1 << 15
    rng = np.random.RandomState(3)
    tabs = []
    for lvl in range(N_LEVELS):
        # entry i of level lvl: two bits of i + lvl per half choose the tie and its sign, so that entry 0 (the box
        # corner's vertex) alone meets every tie in both halves over the 16 levels
        code = np.stack([(np.arange(T) + lvl) & 3, ((np.arange(T) + lvl) >> 2) & 3], 1)
        mant = np.where(code & 1, 257.0, 259.0) * np.where(code & 2, 1.0, -1.0)
        tabs.append(torch.from_numpy((mant * 2.0 ** (lvl - 12)).astype(np.float32)).to(gpu))
    lo, hi = blender_bbox()
    res = np.asarray(level_res(), np.float32)
    cell = ((hi.astype(np.float32) - lo.astype(np.float32))[None, :] / res[:, None]).astype(np.float32)
    n = 16384
    lv = rng.randint(0, N_LEVELS, n)
    k = np.floor(rng.rand(n, 3) * res[lv][:, None]).astype(np.float32)
    pts = (k * cell[lv] + lo.astype(np.float32)).astype(np.float32)
    pts[:64] = lo.astype(np.float32)                          # the box corner: a vertex of every level
    x = torch.from_numpy(pts).to(gpu)
    ref, _ = encode(L, gpu, x, log2_T, tabs=tabs, layout="level")
    words, _ = encode_pk(L, gpu, x, log2_T, tabs=tabs, layout="level")
    assert_words(words, ref, "level", "ties")
    f = ref.cpu().numpy().astype(np.float64)                  # [L, n, 2]
    m, e = np.frexp(np.abs(f))
    got = widen(words, "level").cpu().numpy().astype(np.float64)
    for tie, even in ((257, 256), (259, 260)):
        for sign in (1.0, -1.0):
            for half in (0, 1):
                at = (m[..., half] == tie / 512.0) & (np.sign(f[..., half]) == sign)
                assert int(at.sum()) >= 100, f"fixture: {int(at.sum())} ties {sign * tie} in half {half}"
                want = sign * even / 512.0 * 2.0 ** e[..., half][at]
                assert np.array_equal(got[..., half][at], want), f"tie {sign * tie} in half {half}"


# ---------------------------------------------------------------- 2. the encoder on the fp16 image
@pytest.mark.parametrize("log2_T", [12, 19])
def test_words_from_the_fp16_image(nerf, gpu, log2_T):
    import indoor_nerf_amd._lib as L
    tabs, _, _ = table_set(gpu, log2_T, 0.05)
    image = convert(L, gpu, tabs, log2_T)
    for P in (1, 129, 4097):
        x = random_points(gpu, P, P)
        for layout in ("point", "level"):
            for with_keep in (False, True):
                ref, ref_keep = encode(L, gpu, x, log2_T, image=image, layout=layout, with_keep=with_keep)
                words, keep = encode_pk(L, gpu, x, log2_T, image=image, layout=layout, with_keep=with_keep)
                what = f"half log2_T {log2_T} P {P} {layout} keep {with_keep}"
                moved = assert_words(words, ref, layout, what)
                if with_keep:
                    assert torch.equal(keep, ref_keep), f"{what}: keep"
        if P == 4097:       # the last launch above: level-major words of the image
            assert moved >= 0.99
            plain, _ = encode_pk(L, gpu, x, log2_T, tabs=tabs, layout="level")
            assert not torch.equal(plain, words), "the image's words are the fp32 tables' words"


# ---------------------------------------------------------------- 3. the MLP on the words
SPR, SPR2 = 3, 2


def real_weights(gpu):
    g = torch.Generator().manual_seed(11)
    return {k: ((torch.rand(s, generator=g) * 2 - 1) / np.sqrt(s[1])).to(gpu) for k, s in SHAPES.items()}


def views(L, gpu, P):
    """name -> (d_sh, sh_stride, d_viewdirs, samples_per_ray) of the three view modes, over P // 2 + 2 rays (enough
    for SPR points per ray and for the two-segment order below); the tensors are returned to keep them alive."""
    from indoor_nerf_amd.render import _linspace
    g = torch.Generator().manual_seed(P)
    R = P // 2 + 2
    sh = (torch.randn(P, 16, generator=g) * 0.5).to(gpu)
    d = torch.randn(R, 3, generator=g)
    dirs = (d / d.norm(dim=-1, keepdim=True)).to(gpu).contiguous()
    rays = torch.cat([torch.zeros(R, 3, device=gpu), dirs, torch.full((R, 1), 2.0, device=gpu),
                      torch.full((R, 1), 6.0, device=gpu), dirs], 1).contiguous()
    f = dict(device=gpu, dtype=torch.float32)
    z, pts, rd, vd, rec = (torch.empty(R, 2, **f), torch.empty(R, 2, 3, **f), torch.empty(R, 3, **f),
                           torch.empty(R, 3, **f), torch.empty(R, 40, **f))
    L.call("nerf_sample_stratified_sh", L.ptr(rays), 11, R, 2, L.ptr(_linspace(2, gpu)), 0, 0, None, 0, 0, None,
           L.ptr(z), L.ptr(pts), L.ptr(rd), L.ptr(vd), L.ptr(rec), L.stream())
    return {"rows": (L.ptr(sh, "sh"), 16, None, 1), "viewdirs": (None, 0, L.ptr(dirs, "dirs"), SPR),
            "records": (L.ptr(rec, "rec"), 0, None, SPR)}, (sh, dirs, rec)


def mlp(L, entry, W, feat_ptr, sp, sl, P, view, keep=None, order=None):
    raw = torch.full((P, 4), float("nan"), device=W["w0"].device)
    L.call(entry, feat_ptr, sp, sl, *view, L.ptr(keep, "keep", torch.bool, True), P,
           ctypes.byref(weights_struct(L, W)), L.ptr(raw, "raw"), order, L.stream())
    return raw


def fine_pass_order(L, gpu, P):
    """A permuted io_rows with seg_split / spr2 as the coarse-reuse fine pass sets them: the first seg_split points
    SPR to a ray, the others SPR2 to a ray."""
    rows = torch.from_numpy(np.random.default_rng(P).permutation(P).astype(np.int32)).to(gpu)
    return ctypes.byref(L.PointOrder(L.ptr(rows, "rows", torch.int32).value, (P // 5) * SPR, SPR2)), rows


@pytest.mark.parametrize("P", MLP_POINTS)
def test_mlp_on_words_is_the_mlp_on_the_features(nerf, gpu, P):
    """Real features (the +-0.05 tables through both encoders), every layout, keep, order and view mode: raw of the
    packed entry on the words == raw of nerf_mlp_fwd_bf16 on the fp32 features they were rounded from == raw of
    nerf_mlp_fwd_bf16 on the words widened back to fp32."""
    import indoor_nerf_amd._lib as L
    tabs, _, _ = table_set(gpu, 19, 0.05)
    W = real_weights(gpu)
    x = random_points(gpu, P, 7 * P)
    view_of, alive = views(L, gpu, P)
    keep_flags = torch.from_numpy(np.random.default_rng(P).random(P) < 0.5).to(gpu)
    order, rows = fine_pass_order(L, gpu, P)
    for layout in ("point", "level"):
        feat, _ = encode(L, gpu, x, 19, tabs=tabs, layout=layout)
        words, _ = encode_pk(L, gpu, x, 19, tabs=tabs, layout=layout)
        wide = widen(words, layout)
        fs, ws = ((2 * N_LEVELS, 2), (N_LEVELS, 1)) if layout == "point" else ((2, 2 * P), (1, P))
        for keep in (None, keep_flags):
            for o in (None, order):
                for mode, view in view_of.items():
                    what = f"P {P} {layout} keep {keep is not None} order {o is not None} {mode}"
                    ref = mlp(L, MLP, W, L.ptr(feat, "feat"), *fs, P, view, keep, o)
                    got = mlp(L, MLP_PK, W, L.ptr(words, "words", torch.int32), *ws, P, view, keep, o)
                    again = mlp(L, MLP, W, L.ptr(wide, "wide"), *fs, P, view, keep, o)
                    assert bool(torch.isfinite(ref).all()), what
                    assert torch.equal(bits(got), bits(ref)), \
                        f"{what}: {int((bits(got) != bits(ref)).any(1).sum())} rows differ from the fp32 features' raw"
                    assert torch.equal(bits(again), bits(ref)), f"{what}: the widened words"
    del alive, rows


@pytest.mark.parametrize("P", MLP_POINTS)
def test_mlp_on_exact_integers(nerf, gpu, exact, P):  # noqa: F811
    """test_gpu_mlp_bf16's integer data, on which every product, sum and rounding is exact: raw equals the int64
    evaluation bit for bit."""
    import indoor_nerf_amd._lib as L
    e = exact
    x, sh, ref, keep = e["x"][:P], e["sh"][:P].contiguous(), e["ref"][:P], e["keep"][:P].contiguous()
    halves = x.to(torch.bfloat16)
    assert torch.equal(halves.float(), x), "fixture: the integers are not bf16 numbers"
    words_point = halves.contiguous().view(torch.int32).reshape(P, N_LEVELS)         # [P, 16]: {f0 low, f1 high}
    ref_keep = ref.clone()
    ref_keep[~keep, 3] = 0.0
    perm = torch.from_numpy(np.random.default_rng(P).permutation(P).astype(np.int32)).to(gpu)
    order = ctypes.byref(L.PointOrder(L.ptr(perm, "rows", torch.int32).value, 0, 0))
    view = (L.ptr(sh, "sh"), 16, None, 1)
    for layout in ("point", "level"):
        words = words_point.contiguous() if layout == "point" else words_point.t().contiguous()
        ws = (N_LEVELS, 1) if layout == "point" else (1, P)
        for k in (None, keep):
            for o in (None, order):
                want = ref if k is None else ref_keep
                if o is not None:
                    want = torch.empty_like(want).index_copy_(0, perm.long(), want)
                got = mlp(L, MLP_PK, e["W"], L.ptr(words, "words", torch.int32), *ws, P, view, k, o)
                assert torch.equal(bits(got), bits(want)), f"P {P} {layout} keep {k is not None} order {o is not None}"


# ---------------------------------------------------------------- 4. slices and row offsets
def test_slices_and_row_offsets_give_the_same_bits(nerf, gpu):
    """The same 4,097 points in one launch, in slices of 37, and shifted by 13 rows of the buffers: the same words
    and the same raw, and the rows outside a launch keep their contents."""
    import indoor_nerf_amd._lib as L
    tabs, _, _ = table_set(gpu, 19, 0.05)
    image = convert(L, gpu, tabs, 19)
    W = real_weights(gpu)
    P = 4097
    x = random_points(gpu, P, 4097)
    sh = (torch.randn(P, 16, generator=torch.Generator().manual_seed(1)) * 0.5).to(gpu)

    def raw_of(words, layout, n, row0=0, s0=0):
        rows_total = words.shape[0] if layout == "point" else words.shape[1]
        sp, sl = (N_LEVELS, 1) if layout == "point" else (1, rows_total)
        view = (L.ptr_at(sh, 16 * s0, "sh"), 16, None, 1)
        return mlp(L, MLP_PK, W, L.ptr_at(words, sp * row0, "words", dtype=torch.int32), sp, sl, n, view)

    for src in (dict(tabs=tabs), dict(image=image)):
        for layout in ("point", "level"):
            rows = (lambda t: t) if layout == "point" else (lambda t: t.t())
            whole, keep = encode_pk(L, gpu, x, 19, layout=layout, **src)
            raw = raw_of(whole, layout, P)
            assert bool(torch.isfinite(raw).all())
            shifted, skeep = encode_pk(L, gpu, x, 19, layout=layout, row0=13, rows=P + 20, **src)
            assert torch.equal(rows(shifted)[13:13 + P], rows(whole)), f"{layout}: rows shifted by 13"
            assert torch.equal(skeep[13:13 + P], keep)
            for edge in (rows(shifted)[:13], rows(shifted)[13 + P:]):
                assert bool((edge == FILL).all()), f"{layout}: a row outside the launch was written"
            assert torch.equal(bits(raw_of(shifted, layout, P, row0=13)), bits(raw)), f"{layout}: raw, shifted rows"
            parts, raws = [], []
            for s in range(0, P, 37):
                w, k = encode_pk(L, gpu, x[s:s + 37].contiguous(), 19, layout=layout, **src)
                parts.append((rows(w), k))
                raws.append(raw_of(w, layout, k.shape[0], s0=s))
            assert torch.equal(torch.cat([w for w, _ in parts]), rows(whole)), f"{layout}: slices of 37"
            assert torch.equal(torch.cat([k for _, k in parts]), keep)
            assert torch.equal(bits(torch.cat(raws)), bits(raw)), f"{layout}: raw, slices of 37"


def test_embedder_route(nerf, gpu):
    """HashEmbedder.encode_into(packed=True) calls the packed entry of its tables (half=True: of the image), with
    row0 as for fp32, and checks the buffer in words."""
    import indoor_nerf_amd._lib as L
    lo, hi = blender_bbox()
    emb = nerf.HashEmbedder((torch.from_numpy(lo), torch.from_numpy(hi)), finest_resolution=1024,
                            log2_hashmap_size=15).to(gpu).eval()
    tabs, _, _ = table_set(gpu, 15, 0.05)
    with torch.no_grad():
        for e, t in zip(emb.embeddings, tabs):
            e.weight.copy_(t)
    x = random_points(gpu, 257, 3)
    for half in (False, True):
        src = dict(image=convert(L, gpu, tabs, 15)) if half else dict(tabs=tabs)
        ref, ref_keep = encode_pk(L, gpu, x, 15, layout="level", row0=5, **src)
        words = torch.full((N_LEVELS, 262), FILL, device=gpu, dtype=torch.int32)
        keep = torch.full((262,), True, device=gpu)
        with torch.no_grad():
            emb.encode_into(x, words, 1, 262, keep, row0=5, half=half, packed=True)
            with pytest.raises(ValueError, match="encode_into: rows out of the feature / keep buffers"):
                emb.encode_into(x, words, 1, 262, keep, row0=6, half=half, packed=True)
            with pytest.raises(TypeError, match="feat: expected torch.int32"):
                emb.encode_into(x, torch.empty(N_LEVELS, 262, 2, device=gpu), 1, 262, keep, half=half, packed=True)
        assert torch.equal(words, ref) and torch.equal(keep, ref_keep), f"half {half}"
