"""nerf_mlp_fwd_bf16 (csrc/field_x6.hip mlp_fwd_bf16_kernel) driven through the C entry.

The network (no biases): h1 = relu(W0 x), o = W1 h1, sigma = o[0], h2 = relu(C0 [sh ; o[1:16]]), h3 = relu(C1 h2),
rgb = C2 h3, raw = [rgb, sigma]. The bf16 forward rounds W0, W1, C0, C1, x, sh and the layer operands h1, o[1:16], h2
to bf16 (round to nearest even), multiplies exactly, sums in fp32, and leaves sigma, h3 and the C2 layer in fp32.

1. Integer data on which every product, sum and rounding is exact: the kernel's raw equals an int64 evaluation bit for
   bit, in every layout, with and without keep and a row order, at every tile shape; so does nerf_mlp_fwd_ord.
2. One rounding site at a time sees the ties 257, 259, -257, -259 (-> 256, 260, -256, -260 under round to nearest
   even; truncation, round-half-up and round-half-away each miss one of them); sigma and h3 are not rounded.
3. Real data against E, a torch emulation that rounds at the same sites and sums in fp64, and against F, the fp32
   evaluation (nerf_mlp_fwd_ord): at most 1 % of the points off E by more than 1e-5, and every point closer to E
   than max |E - F|, the format's own error on that data. Measured on the MI355X: 0.015-0.016 % of 200,000 points
   and max |K - E| = 4.1e-4 against max |E - F| = 2.0e-3; a torch emulation with fp32 sums in the kernel's place
   gives 0.021 % and the same two maxima.
4. A point's raw row has the same bits whatever points share its tile or its launch.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"w0": (64, 32), "w1": (16, 64), "c0": (64, 31), "c1": (64, 64), "c2": (3, 64)}
TIES = {257: 256, 259: 260, -257: -256, -259: -260}


# ---------------------------------------------------------------- references (host)
def bf16_rne(a):
    """fp32 -> bf16 -> fp32, round to nearest even, on the bits (finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


def net_exact(W, x, sh, rnd=bf16_rne):
    """The network in float64 on data whose sums are exact (integers far below 2^24), rounding with rnd at the
    kernel's sites -> raw [P, 4] and the values each site saw before its rounding."""
    W0, W1, C0, C1 = (rnd(W[k]) for k in ("w0", "w1", "c0", "c1"))
    h1 = np.maximum(rnd(x) @ W0.T, 0)
    o = rnd(h1) @ W1.T
    h2 = np.maximum(rnd(sh) @ C0[:, :16].T + rnd(o[:, 1:]) @ C0[:, 16:].T, 0)
    h3 = np.maximum(rnd(h2) @ C1.T, 0)
    rgb = h3 @ np.asarray(W["c2"], np.float64).T
    return np.concatenate([rgb, o[:, :1]], 1), dict(h1=h1, o=o, h2=h2, h3=h3)


def emulate64(W, x, sh):
    """E: torch, the kernel's roundings, fp64 sums. W, x, sh: fp32 tensors on the device -> raw [P, 4] fp64."""
    def b(t):
        return t.to(torch.bfloat16).double()
    W0, W1, C0, C1 = (b(W[k]) for k in ("w0", "w1", "c0", "c1"))
    h1 = torch.relu(b(x) @ W0.T)
    o = b(h1.float()) @ W1.T
    h2 = torch.relu(b(sh) @ C0[:, :16].T + b(o[:, 1:].float()) @ C0[:, 16:].T)
    h3 = torch.relu(b(h2.float()) @ C1.T)
    return torch.cat([h3 @ W["c2"].double().T, o[:, :1]], 1)


# ---------------------------------------------------------------- the driver
def weights_struct(L, W):
    return L.MlpWeights(*[L.ptr(W[k], k).value for k in ("w0", "w1", "c0", "c1", "c2")])


def launch(L, entry, W, x, sh, layout="levels", keep=None, rows=None, viewdirs=None, records=None, spr=1):
    """One launch of `entry` ("bf16" or "ord") over the points x [P, 32] -> raw [P, 4] (NaN where nothing was
    stored). layout: "levels" (features [16][P][2], SH rows at stride 16) or "rows48" ([P, 48] = [x | sh]); rows:
    int32 io_rows; viewdirs [R, 3] or records [R, 40] with spr points per ray replace the SH rows."""
    P = x.shape[0]
    raw = torch.full((P, 4), float("nan"), device=x.device)
    if layout == "levels":
        feat = x.view(P, 16, 2).permute(1, 0, 2).contiguous()
        f_args = (L.ptr(feat, "feat"), 2, 2 * P)
        sh = None if sh is None else sh.contiguous()
        s_args = (L.ptr(sh, "sh", allow_none=True), 16)
    else:
        buf = torch.cat([x, sh], 1).contiguous()
        f_args = (L.ptr(buf, "x48"), 48, 2)
        s_args = (L.ptr_at(buf, 32, "sh48"), 48)
    if viewdirs is not None:
        s_args, v_args = (None, 0), (L.ptr(viewdirs, "viewdirs"), spr)
    elif records is not None:
        s_args, v_args = (L.ptr(records, "records"), 0), (None, spr)
    else:
        v_args = (None, 1)
    order = None if rows is None else ctypes.byref(L.PointOrder(L.ptr(rows, "rows", torch.int32).value, 0, 0))
    front = (*f_args, *s_args, *v_args, L.ptr(keep, "keep", torch.bool, True), P, ctypes.byref(weights_struct(L, W)),
             L.ptr(raw, "raw"))
    if entry == "bf16":
        L.call("nerf_mlp_fwd_bf16", *front, order, L.stream())
    else:
        L.call("nerf_mlp_fwd_ord", *front, None, None, None, 0, order, L.stream())
    return raw


def bits(t):
    return t.contiguous().view(torch.int32)


def dev(W, gpu):
    return {k: torch.from_numpy(np.asarray(v, np.float32)).to(gpu) for k, v in W.items()}


# ---------------------------------------------------------------- 1. exact integers
P_MAX = 131105


def sparse_signs(rng, shape, per_row):
    w = np.zeros(shape, np.int64)
    for r in range(shape[0]):
        w[r, rng.choice(shape[1], per_row, replace=False)] = rng.choice([-1, 1], per_row)
    return w


@pytest.fixture(scope="module")
def exact(gpu):
    """Integer weights and inputs, the int64 evaluation, and what makes the data exact: every rounded value is a
    bf16 number already (so rounding changes nothing) and every sum is an integer below 2^24."""
    rng = np.random.default_rng(7)
    W = {k: sparse_signs(rng, SHAPES[k], 3 if k == "c0" else 4) for k in ("w0", "w1", "c0", "c1")}
    W["c2"] = rng.integers(-2, 3, SHAPES["c2"])
    x, sh = rng.integers(-4, 5, (P_MAX, 32)), rng.integers(-4, 5, (P_MAX, 16))
    ref, act = net_exact(W, x, sh, rnd=lambda a: np.asarray(a, np.float64))      # no rounding at all
    rounded, _ = net_exact(W, x, sh)
    assert np.array_equal(ref, rounded), "the integer data is not bf16-exact"
    for k in ("h1", "h2"):
        assert np.array_equal(bf16_rne(act[k]), act[k]), k
    assert np.array_equal(bf16_rne(act["o"][:, 1:]), act["o"][:, 1:])
    assert max(np.abs(v).max() for v in act.values()) * 64 * 2 < 2 ** 24 and np.abs(ref).max() < 2 ** 24
    # the data exercises the network: about half of the ReLUs are open, nearly every colour is nonzero (on this
    # seed: max h1 16, |o| 39, h2 69, h3 97, |rgb| 456; 99.5 % of the colours and 87 % of the sigmas nonzero)
    for k in ("h1", "h2", "h3"):
        assert 0.3 < (act[k] > 0).mean() < 0.7, (k, (act[k] > 0).mean())
    assert (ref[:, :3] != 0).mean() > 0.99 and (ref[:, 3] != 0).mean() > 0.8
    # the same through torch's bf16 conversion
    xt, st = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(sh.astype(np.float32))
    Wt = {k: torch.from_numpy(v.astype(np.float32)) for k, v in W.items()}
    assert np.array_equal(emulate64(Wt, xt[:4097], st[:4097]).numpy(), ref[:4097])
    keep = rng.random(P_MAX) < 0.5
    to = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(gpu)  # noqa: E731
    return dict(W=dev(W, gpu), x=to(x), sh=to(sh), ref=to(ref), keep=to(keep, np.bool_), rng=rng)


@pytest.mark.parametrize("P", [1, 31, 32, 33, 257, 4097, P_MAX])
def test_exact_integers(nerf, gpu, exact, P):
    """P_MAX: 4098 tiles for the launch's 512 blocks of 8 waves, so two waves run a second tile."""
    import indoor_nerf_amd._lib as L
    e = exact
    x, sh, ref, keep = e["x"][:P], e["sh"][:P], e["ref"][:P], e["keep"][:P]
    perm = torch.from_numpy(np.random.default_rng(P).permutation(P).astype(np.int32)).to(gpu)
    ref_keep = ref.clone()
    ref_keep[~keep, 3] = 0.0
    for layout in ("levels", "rows48"):
        for k in (None, keep):
            for rows in (None, perm):
                want = ref if k is None else ref_keep
                if rows is not None:
                    want = torch.empty_like(want).index_copy_(0, rows.long(), want)
                for entry in ("bf16", "ord"):
                    got = launch(L, entry, e["W"], x, sh, layout, keep=k, rows=rows)
                    what = f"{entry} P={P} {layout} keep={k is not None} rows={rows is not None}"
                    assert torch.equal(bits(got), bits(want)), \
                        f"{what}: {int((bits(got) != bits(want)).any(1).sum())} rows differ"


# ---------------------------------------------------------------- 2. round to nearest even, site by site
def zero_weights():
    return {k: np.zeros(s, np.float64) for k, s in SHAPES.items()}


def carry_o1_to_rgb0(W):
    """rgb0 = bf16(o[1]) for either sign: h2[0] = relu(o1), h2[1] = relu(-o1), h3 = h2, rgb0 = h3[0] - h3[1]."""
    W["c0"][0, 16], W["c0"][1, 16] = 1, -1          # C0 column 16 multiplies o[1]
    W["c1"][0, 0] = W["c1"][1, 1] = 1
    W["c2"][0, 0], W["c2"][0, 1] = 1, -1


def tie_cases():
    """site -> (W, x [P, 32], sh [P, 16], the site's values (array, pre-rounding), {channel: expected column})."""
    t = np.array(list(TIES), np.float64)
    r = np.array(list(TIES.values()), np.float64)
    pos = t > 0
    cases = {}
    # features: x0 = tie; h1[0] = relu(x0), h1[1] = relu(-x0); sigma = o[0] = o[1] = h1[0] - h1[1] = bf16(x0)
    W, x, sh = zero_weights(), np.zeros((4, 32)), np.zeros((4, 16))
    x[:, 0] = t
    W["w0"][0, 0], W["w0"][1, 0] = 1, -1
    W["w1"][0, 0] = W["w1"][1, 0] = 1
    W["w1"][0, 1] = W["w1"][1, 1] = -1
    carry_o1_to_rgb0(W)
    cases["features"] = (W, x, sh, lambda a, v=x[:, 0].copy(): v, {3: r, 0: r})
    # SH rows: sh0 = tie; h2[0] = relu(sh0), h2[1] = relu(-sh0); rgb0 = h3[0] - h3[1] = bf16(sh0)
    W, x, sh = zero_weights(), np.zeros((4, 32)), np.zeros((4, 16))
    sh[:, 0] = t
    W["c0"][0, 0], W["c0"][1, 0] = 1, -1
    W["c1"][0, 0] = W["c1"][1, 1] = 1
    W["c2"][0, 0], W["c2"][0, 1] = 1, -1
    cases["sh"] = (W, x, sh, lambda a, v=sh[:, 0].copy(): v, {0: r, 3: np.zeros(4)})
    # a weight of W0 (the image's first matrix): W0[q, q] = tie q; point p = 4 s + q has x_q = +1 (s = 0) or -1:
    # sigma = sum_q h1[q] = relu(+-bf16(tie q))
    W, x, sh = zero_weights(), np.zeros((8, 32)), np.zeros((8, 16))
    for q in range(4):
        W["w0"][q, q] = t[q]
        x[q, q], x[4 + q, q] = 1, -1
    W["w1"][0, :4] = 1
    cases["weight_w0"] = (W, x, sh, lambda a, v=np.diag(W["w0"])[:4].copy(): v,
                          {3: np.concatenate([np.maximum(r, 0), np.maximum(-r, 0)])})
    # a weight of C1 (the image's last rounded matrix): C1[q, q] = tie q, h2[q] = sh_q = 1 at point q; C2 row 0 adds
    # h3[0..3] = relu(bf16(tie q)), C2 row 1 is fed by the negated weights in rows 4..7
    W, x, sh = zero_weights(), np.zeros((4, 32)), np.zeros((4, 16))
    for q in range(4):
        W["c0"][q, q] = W["c0"][4 + q, q] = 1
        W["c1"][q, q], W["c1"][4 + q, 4 + q] = t[q], -t[q]
        sh[q, q] = 1
    W["c2"][0, :4] = W["c2"][1, 4:8] = 1
    cases["weight_c1"] = (W, x, sh, lambda a, v=np.diag(W["c1"])[:4].copy(): v,
                          {0: np.maximum(r, 0), 1: np.maximum(-r, 0)})
    # h1 (after the ReLU: the positive ties): h1[0] = x0 + x1 = 256 + {1, 3}; sigma = bf16(h1[0])
    W, x, sh = zero_weights(), np.zeros((2, 32)), np.zeros((2, 16))
    x[:, 0], x[:, 1] = 256, t[pos] - 256
    W["w0"][0, 0] = W["w0"][0, 1] = 1
    W["w1"][0, 0] = 1
    cases["h1"] = (W, x, sh, lambda a: a["h1"][:, 0], {3: r[pos]})
    # o rows 1..15: o[0] = o[1] = h1[0] + h1[1] - h1[2] - h1[3] = +-(256 + {1, 3}); sigma = o[0] keeps 257, 259
    # (the fp32 accumulator, unrounded) while rgb0 = bf16(o[1])
    W, x, sh = zero_weights(), np.zeros((4, 32)), np.zeros((4, 16))
    for p in range(4):
        x[p, 0 if pos[p] else 2], x[p, 1 if pos[p] else 3] = 256, abs(t[p]) - 256
    for q in range(4):
        W["w0"][q, q] = 1
        W["w1"][0, q] = W["w1"][1, q] = 1 if q < 2 else -1
    carry_o1_to_rgb0(W)
    cases["o"] = (W, x, sh, lambda a: a["o"][:, 1], {3: t, 0: r})
    # h2 (after the ReLU): h2[0] = sh0 + sh1 = 256 + {1, 3}; h3[0] = bf16(h2[0]) -> rgb0; h3[1] = bf16(h2[0]) + h2[1]
    # = 257 / 261 is NOT rounded on its way to rgb1
    W, x, sh = zero_weights(), np.zeros((2, 32)), np.zeros((2, 16))
    sh[:, 0], sh[:, 1], sh[:, 2] = 256, t[pos] - 256, 1
    W["c0"][0, 0] = W["c0"][0, 1] = W["c0"][1, 2] = 1
    W["c1"][0, 0] = W["c1"][1, 0] = W["c1"][1, 1] = 1
    W["c2"][0, 0] = W["c2"][1, 1] = 1
    cases["h2"] = (W, x, sh, lambda a: a["h2"][:, 0], {0: r[pos], 1: r[pos] + 1})
    return cases


def test_ties_round_like_torch():
    t = torch.tensor(list(TIES), dtype=torch.float32)
    want = torch.tensor(list(TIES.values()), dtype=torch.float32)
    assert torch.equal(t.to(torch.bfloat16).float(), want)
    assert np.array_equal(bf16_rne(t.numpy()), want.numpy().astype(np.float64))
    # what the other rounding rules would give: each misses at least one tie
    trunc = (t.view(torch.int32) & -65536).view(torch.float32)
    assert not torch.equal(trunc, want)


@pytest.mark.parametrize("site", ["features", "sh", "weight_w0", "weight_c1", "h1", "o", "h2"])
def test_round_to_nearest_even(nerf, gpu, site):
    import indoor_nerf_amd._lib as L
    W, x, sh, site_values, literal = tie_cases()[site]
    ref, act = net_exact(W, x, sh)
    seen = np.asarray(site_values(act), np.float64)
    assert set(seen.tolist()) <= set(TIES) and len(seen) >= 2, f"{site}: the site sees {seen}, not the ties"
    for ch, col in literal.items():          # the emulation, against the values written out by hand
        assert np.array_equal(ref[:, ch], col), (site, ch, ref[:, ch], col)
    Wd = dev(W, gpu)
    xd, sd = (torch.from_numpy(a.astype(np.float32)).to(gpu) for a in (x, sh))
    want = torch.from_numpy(ref.astype(np.float32)).to(gpu)
    for layout in ("levels", "rows48"):
        got = launch(L, "bf16", Wd, xd, sd, layout)
        assert torch.equal(bits(got + 0.0), bits(want + 0.0)), f"{site} {layout}: {got.tolist()} != {want.tolist()}"


# ---------------------------------------------------------------- 3. real values
P_REAL, SPR = 200000, 8


@pytest.fixture(scope="module")
def real(gpu):
    g = torch.Generator().manual_seed(11)
    W = {k: ((torch.rand(s, generator=g) * 2 - 1) / np.sqrt(s[1])).to(gpu) for k, s in SHAPES.items()}
    x = (torch.randn(P_REAL, 32, generator=g) * 0.5).to(gpu)
    sh = (torch.randn(P_REAL, 16, generator=g) * 0.5).to(gpu)
    d = torch.randn(P_REAL // SPR, 3, generator=g)
    return dict(W=W, x=x, sh=sh, dirs=(d / d.norm(dim=-1, keepdim=True)).to(gpu).contiguous())


def check_real(got, E, F, what):
    """The two conditions of the module docstring; the figures are printed before they are asserted."""
    dev_e = (got.double() - E).abs().amax(1)
    fmt = float((E - F.double()).abs().max())
    frac, worst = float((dev_e > 1e-5).double().mean()), float(dev_e.max())
    print(f"{what}: {100 * frac:.4f} % of {got.shape[0]} points off E by > 1e-5, max |K - E| = {worst:.3e}, "
          f"max |E - F| = {fmt:.3e}")
    assert torch.isfinite(got).all()
    assert frac <= 0.01, f"{what}: {100 * frac:.3f} % of the points differ from the emulation by more than 1e-5"
    assert worst < fmt, f"{what}: max |K - E| = {worst:.3e} is not below the format's error {fmt:.3e}"


@pytest.mark.parametrize("mode", ["rows", "viewdirs", "records"])
def test_real_values_against_emulation(nerf, gpu, real, mode):
    import indoor_nerf_amd._lib as L
    from indoor_nerf_amd.render import _linspace
    W, x = real["W"], real["x"]
    R = P_REAL // SPR
    if mode == "rows":
        sh, kw = real["sh"], {}
    elif mode == "viewdirs":
        rows = torch.empty(R, 16, device=gpu)
        L.call("nerf_sh4_fwd", L.ptr(real["dirs"]), R, L.ptr(rows), L.stream())
        sh, kw = rows.repeat_interleave(SPR, 0), dict(viewdirs=real["dirs"], spr=SPR)
    else:   # the per-ray records of the stratified sampler: 16 fp32 coefficients + their bf16 pieces
        rays = torch.cat([torch.zeros(R, 3, device=gpu), real["dirs"], torch.full((R, 1), 2.0, device=gpu),
                          torch.full((R, 1), 6.0, device=gpu), real["dirs"]], 1).contiguous()
        f = dict(device=gpu, dtype=torch.float32)
        z, pts, rd, vd, rec = (torch.empty(R, SPR, **f), torch.empty(R, SPR, 3, **f), torch.empty(R, 3, **f),
                               torch.empty(R, 3, **f), torch.empty(R, 40, **f))
        L.call("nerf_sample_stratified_sh", L.ptr(rays), 11, R, SPR, L.ptr(_linspace(SPR, gpu)), 0, 0, None, 0, 0, None,
               L.ptr(z), L.ptr(pts), L.ptr(rd), L.ptr(vd), L.ptr(rec), L.stream())
        sh, kw = rec[:, :16].repeat_interleave(SPR, 0), dict(records=rec, spr=SPR)
    E = emulate64(W, x, sh)
    F = launch(L, "ord", W, x, sh if mode == "rows" else None, **kw)
    got = launch(L, "bf16", W, x, sh if mode == "rows" else None, **kw)
    check_real(got, E, F, mode)
    if mode == "rows":
        check_real(launch(L, "bf16", W, x, sh, "rows48"), E, F, "rows48")


# ---------------------------------------------------------------- 4. independence of a point's company
def test_point_results_do_not_depend_on_their_company(nerf, gpu, real):
    import indoor_nerf_amd._lib as L
    n = 4097
    W, x, sh = real["W"], real["x"][:n].contiguous(), real["sh"][:n].contiguous()
    base = launch(L, "bf16", W, x, sh)
    assert torch.isfinite(base).all()
    sliced = torch.cat([launch(L, "bf16", W, x[i:i + 37].contiguous(), sh[i:i + 37].contiguous())
                        for i in range(0, n, 37)], 0)
    assert torch.equal(bits(sliced), bits(base)), "slices of 37"
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n).astype(np.int32)).to(gpu)
    # point perm[i] sits at position i and writes row perm[i]
    moved = launch(L, "bf16", W, x[perm.long()].contiguous(), sh[perm.long()].contiguous(), rows=perm)
    assert torch.equal(bits(moved), bits(base)), "a permuted order"
    more = launch(L, "bf16", W, real["x"][:n + 1000].contiguous(), real["sh"][:n + 1000].contiguous())
    assert torch.equal(bits(more[:n]), bits(base)), "other points appended"
    shifted = launch(L, "bf16", W, real["x"][13:n + 13].contiguous(), real["sh"][13:n + 13].contiguous())
    assert torch.equal(bits(shifted[:n - 13]), bits(base[13:])), "the same points at other lanes"
