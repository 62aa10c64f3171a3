"""The MLP kernels' prologue (csrc/field_x6.hip fill_images): the bf16 weight image every block builds from the fp32
weights in one round of 16-byte loads, and the first tile's inputs that are loaded before it.

The image (nerf_mlp_weight_image) is compared bit for bit with a NumPy construction from the layout documented at the
top of field_x6.hip; the construction rounds to nearest even with integer arithmetic and is itself checked against
v == p0 + p1 + p2. The kernels run at the shapes where the prologue or the early loads can go wrong, against the fp64
evaluation and the bar of test_gpu_mlp_x6.py (its _check_vs_fp64, with its _run replaced by direct calls of the
entries under test)."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_mlp_x6 as x6

pytestmark = pytest.mark.gpu

S32, S64 = 36, 68                                       # padded row strides
IM_W0, IM_W1, IM_C0, IM_C1, IM_C2, IM_PIECE = 0, 2304, 3392, 5696, 10048, 11136
NAMES = ("sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight", "color_net.1.weight", "color_net.2.weight")


def bf16_rne_bits(v32):
    """bf16 bits of fp32 values, round to nearest even, integer arithmetic (finite inputs)."""
    b = np.ascontiguousarray(v32, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split3(v32):
    """The three pieces of each fp32 value: piece k is the RNE of the exact remainder (formed in fp64)."""
    rem = np.asarray(v32, np.float32).astype(np.float64)
    out = []
    for _ in range(3):
        r32 = rem.astype(np.float32)
        assert np.array_equal(r32.astype(np.float64), rem), "remainder not representable in fp32"
        p = bf16_rne_bits(r32)
        out.append(p)
        rem = rem - bf16_value(p).astype(np.float64)
    return out


def build_image(w0, w1, c0, c1, c2):
    """-> (image [3, IM_PIECE] uint16, mask [IM_PIECE] of the logical elements)."""
    c0p = np.zeros((64, 32), np.float32)
    c0p[:, 1:16] = c0[:, 16:31]                         # geo columns; column 0 (the sigma slot) stays 0
    c0p[:, 16:32] = c0[:, 0:16]                         # SH columns
    c2p = np.zeros((16, 64), np.float32)
    c2p[:3] = c2                                        # rows 3..15 zero
    img, mask = np.zeros((3, IM_PIECE), np.uint16), np.zeros(IM_PIECE, bool)
    for base, stride, m in ((IM_W0, S32, w0), (IM_W1, S64, w1), (IM_C0, S32, c0p), (IM_C1, S64, c1), (IM_C2, S64, c2p)):
        rows, cols = m.shape
        off = (base + stride * np.arange(rows)[:, None] + np.arange(cols)[None, :]).ravel()
        for k, p in enumerate(split3(m.ravel())):
            img[k, off] = p
        assert not mask[off].any()
        mask[off] = True
    return img, mask


def tie_values():
    """fp32 values on a bf16 rounding tie: for piece 0 (low half 0x8000, even and odd bf16 neighbours, both signs) and
    for piece 1 (a bf16 value a plus a 9-significant-bit b below half an ulp of a: piece 0 is a, b ties)."""
    t0 = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3C7F8000, 0x41008000], np.uint32).view(np.float32)
    t1 = []
    for e in (0, -5, 3):
        for m in (257, 259, 511):
            for sa in (1.0, -1.0):
                for sb in (1.0, -1.0):
                    t1.append(sa * 1.5 * 2.0 ** e + sb * m * 2.0 ** (e - 18))
    t1 = np.array(t1, np.float64)
    assert np.array_equal(t1.astype(np.float32).astype(np.float64), t1)
    return np.concatenate([t0, t1.astype(np.float32)])


def _weights(seed=0):
    """The five matrices: normal values over several magnitudes, exact zeros, both signs, and the ties."""
    rng = np.random.default_rng(seed)
    ties = tie_values()
    out = []
    for shape in ((64, 32), (16, 64), (64, 31), (64, 64), (3, 64)):
        n = shape[0] * shape[1]
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-4, 2, n)).astype(np.float32)
        v[rng.random(n) < 0.05] = 0.0
        pos = rng.choice(n, ties.size, replace=False)
        v[pos] = ties
        out.append(v.reshape(shape))
    return out


def test_numpy_image_builder_is_an_exact_split():
    """The reference itself: p0 + p1 + p2 == v in fp64 for every logical element, the zeros where the layout has
    them, and the rounding of the tie values to even."""
    ws = _weights()
    img, mask = build_image(*ws)
    vals = sum(bf16_value(img[k]).astype(np.float64) for k in range(3))
    w0, w1, c0, c1, c2 = ws
    assert np.array_equal(vals[IM_W0:IM_W0 + 64 * S32].reshape(64, S32)[:, :32], w0.astype(np.float64))
    assert np.array_equal(vals[IM_W1:IM_W1 + 16 * S64].reshape(16, S64)[:, :64], w1.astype(np.float64))
    c0i = vals[IM_C0:IM_C0 + 64 * S32].reshape(64, S32)
    assert np.array_equal(c0i[:, 1:16], c0[:, 16:31].astype(np.float64)) and not c0i[:, 0].any()
    assert np.array_equal(c0i[:, 16:32], c0[:, :16].astype(np.float64))
    assert np.array_equal(vals[IM_C1:IM_C1 + 64 * S64].reshape(64, S64)[:, :64], c1.astype(np.float64))
    c2i = vals[IM_C2:IM_C2 + 16 * S64].reshape(16, S64)[:, :64]
    assert np.array_equal(c2i[:3], c2.astype(np.float64)) and not c2i[3:].any()
    assert int(mask.sum()) == 2048 + 1024 + 2048 + 4096 + 1024
    # ties go to the even bf16: 1.00390625 (0x3F808000) -> 0x3F80, 1.01171875 (0x3F818000) -> 0x3F82
    t = np.array([0x3F808000, 0x3F818000, 0xBF818000], np.uint32).view(np.float32)
    assert bf16_rne_bits(t).tolist() == [0x3F80, 0x3F82, 0xBF82]
    p0, p1, _ = split3(np.array([1.5 + 257 * 2.0 ** -18, 1.5 + 259 * 2.0 ** -18], np.float32))
    assert p0.tolist() == [0x3FC0, 0x3FC0]
    assert bf16_value(p1).tolist() == [256 * 2.0 ** -18, 260 * 2.0 ** -18]


def test_weight_image_bitwise(nerf, gpu):
    from indoor_nerf_amd import _lib
    ws = _weights()
    want, mask = build_image(*ws)
    dw = [torch.from_numpy(w).to(gpu).contiguous() for w in ws]
    w = _lib.MlpWeights(*[_lib.ptr(t).value for t in dw])
    out = torch.zeros(3 * IM_PIECE, device=gpu, dtype=torch.int16)
    _lib.call("nerf_mlp_weight_image", ctypes.byref(w), _lib.ptr(out, dtype=torch.int16), _lib.stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16).reshape(3, IM_PIECE)
    for k in range(3):
        bad = np.nonzero((got[k] != want[k]) & mask)[0]
        assert bad.size == 0, f"piece {k}: {bad.size} elements differ, first at {bad[:8].tolist()}"


def _launch(nets, xs, graws, save_h3, det_ws=None):
    """The training forward (nerf_mlp_fwd_h3, with or without the saved-h3 buffer) of each net, then ONE
    nerf_mlp_bwd_batch launch of all of them; -> per net (raw, dx, weight gradients) as test_gpu_mlp_x6._run."""
    from indoor_nerf_amd import _lib
    lib = _lib.load()
    keep, jobs, res = [], [], []
    for net, x, graw in zip(nets, xs, graws):
        x, graw = x.contiguous(), graw.contiguous()
        P = x.shape[0]
        wts = [p.detach() for p in net.mlp_weights()]
        w = _lib.MlpWeights(*[_lib.ptr(t).value for t in wts])
        raw, dx, dsh = torch.empty(P, 4, device=x.device), torch.zeros_like(x), torch.empty(P, 16, device=x.device)
        h3 = torch.empty(int(lib.nerf_mlp_h3_bytes(P)) // 4, device=x.device) if save_h3 else None
        grads = [torch.zeros_like(t) for t in wts]
        xp, shp = _lib.ptr(x), _lib.c_vp(x.data_ptr() + 32 * 4)
        _lib.call("nerf_mlp_fwd_h3", xp, 48, 2, shp, 48, None, 1, None, P, ctypes.byref(w), _lib.ptr(raw), None, None,
                  None, 0, None, _lib.ptr(h3, allow_none=True), _lib.stream())
        j = _lib.MlpBwdJob()
        j.feat, j.feat_stride_point, j.feat_stride_level, j.sh, j.sh_stride = xp, 48, 2, shp, 48
        j.samples_per_ray, j.n_points, j.weights, j.graw = 1, P, w, _lib.ptr(graw)
        j.grads = _lib.MlpGrads(*[_lib.ptr(t).value for t in grads])
        j.dfeat, j.dsh, j.h3 = _lib.ptr(dx), _lib.ptr(dsh), _lib.ptr(h3, allow_none=True)
        jobs.append(j)
        keep.append((x, graw, wts, h3))
        res.append((raw, dx, dsh, grads))
    arr = (_lib.MlpBwdJob * len(jobs))(*jobs)
    _lib.call("nerf_mlp_bwd_batch", arr, len(jobs), _lib.ptr(det_ws, allow_none=True),
              0 if det_ws is None else det_ws.numel() * 4, _lib.stream())
    torch.cuda.synchronize()
    out = []
    for raw, dx, dsh, grads in res:
        dx[:, 32:] = dsh
        out.append((raw.double(), dx.double(), {k: g.double() for k, g in zip(NAMES, grads)}))
    return out


def _inputs(nerf, gpu, sizes, seed):
    torch.manual_seed(seed)
    nets = [nerf.NeRFSmall(2, 64, 15, 3, 64, 32, 16).to(gpu) for _ in sizes]
    xs = [torch.randn(P, 48, device=gpu) * 0.3 for P in sizes]
    graws = [torch.randn(P, 4, device=gpu) for P in sizes]
    return nets, xs, graws


def _check(monkeypatch, nets, xs, graws, results):
    for net, x, graw, r in zip(nets, xs, graws, results):
        assert [k for k, _ in net.named_parameters()] == list(NAMES)
        monkeypatch.setattr(x6, "_run", lambda *_a, r=r: r)
        fails = x6._check_vs_fp64(net, x, graw)
        assert not fails, (x.shape[0], fails)


@pytest.mark.parametrize("save_h3", [False, True])
@pytest.mark.parametrize("P", [1, 33, 257, 32 * 8 * 2 + 1])
def test_forward_first_tile_shapes(nerf, gpu, monkeypatch, P, save_h3):
    """A block of waves with no tile (1), a one-point tail tile (33, 257), one tile more than a full round of a
    block (513): the forward with and without the saved h3, its backward on that h3 (or recomputing)."""
    nets, xs, graws = _inputs(nerf, gpu, [P], 10 + P)
    _check(monkeypatch, nets, xs, graws, _launch(nets, xs, graws, save_h3))


@pytest.mark.parametrize("sizes", [(1, 33), (65, 257)])
def test_batched_backward_two_jobs(nerf, gpu, monkeypatch, sizes):
    nets, xs, graws = _inputs(nerf, gpu, sizes, 20 + sizes[0])
    _check(monkeypatch, nets, xs, graws, _launch(nets, xs, graws, True))


def test_deterministic_backward_repeats_bitwise(nerf, gpu):
    from indoor_nerf_amd import field
    nets, xs, graws = _inputs(nerf, gpu, (65, 257), 30)
    nerf.set_deterministic(True)
    try:
        ws = field._det_workspace(gpu)
        a = _launch(nets, xs, graws, True, det_ws=ws)
        b = _launch(nets, xs, graws, True, det_ws=ws)
    finally:
        nerf.set_deterministic(False)
    for (_, dxa, ga), (_, dxb, gb) in zip(a, b):
        assert torch.equal(dxa, dxb)
        for k in NAMES:
            assert torch.equal(ga[k], gb[k]), k
            assert ga[k].abs().sum() > 0
