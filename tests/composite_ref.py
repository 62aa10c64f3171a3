"""What the compositing and sampling width tests share (test_composite_ref_cpu.py, test_gpu_composite_widths.py,
test_gpu_sampler_widths.py): a float64 restatement of raw2outputs (run_nerf.py:347-411) whose backward is torch
autograd, of sample_pdf (run_nerf_helpers.py:354-397) with given uniforms, of the merged depths and z_std
(run_nerf.py:508-513, :541) and of the TV sum (loss.py:11-43); and the seeded builders of the cases at which the
kernels of csrc/composite.hip and csrc/sampling.hip dispatch. No test and no fixture lives here.

Every input is a float32 value promoted exactly to float64. The one thing that does NOT follow the dtype is the
Categorical clamp's eps: it is float32's (EPS32) at every precision, because that is the function the kernels (and
the reference, which runs in float32) compute; oracle.composite takes eps from the dtype and so computes another
function in float64. With dtype=torch.float32 `composite` is the fp32 autograd oracle the entropy bar is measured
with (bit for bit oracle.composite, test_composite_ref_cpu.py).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 1.1920928955078125e-07      # torch.finfo(torch.float32).eps: the Categorical clamp (run_nerf.py:404-406)

FWD_NAMES = ("rgb", "disp", "acc", "weights", "depth", "entropy", "normal")
GRAD_NAMES = ("g_rgb", "g_disp", "g_acc", "g_weights", "g_depth", "g_entropy", "g_normal")


def _t(x, dtype):
    if x is None or torch.is_tensor(x):
        return x if x is None else x.to(dtype)
    return torch.tensor(np.asarray(x)).to(dtype)      # a copy: the cached inputs are read-only


# ---------------------------------------------------------------- the references
def composite(raw, z, rays_d, noise=None, white_bkgd=False, dtype=torch.float64):
    """raw2outputs -> (rgb, disp, acc, weights, depth, entropy, normal); normal is None for 4 raw channels, else
    n = sum(w * n_j) / max(|.|, 1e-12). A raw that is already a tensor of `dtype` is used as it is (autograd leaf)."""
    raw, z, rays_d, noise = _t(raw, dtype), _t(z, dtype), _t(rays_d, dtype), _t(noise, dtype)
    dz = z[..., 1:] - z[..., :-1]
    dz = torch.cat([dz, torch.full_like(z[..., :1], 1e10)], -1)          # S = 1: the one delta is 1e10
    dz = dz * torch.norm(rays_d[..., None, :], dim=-1)
    color = torch.sigmoid(raw[..., :3])
    s = raw[..., 3] if noise is None else raw[..., 3] + noise
    alpha = 1.0 - torch.exp(-F.relu(s) * dz)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    w = alpha * trans
    rgb = torch.sum(w[..., None] * color, -2)
    depth = torch.sum(w * z, -1) / torch.sum(w, -1)
    disp = 1.0 / torch.max(1e-10 * torch.ones_like(depth), depth)
    acc = torch.sum(w, -1)
    if white_bkgd:
        rgb = rgb + (1.0 - acc[..., None])
    probs = entropy_probs(w)
    logp = torch.log(probs.clamp(min=EPS32, max=1 - EPS32))
    entropy = -(logp * probs).sum(-1)
    normal = None
    if raw.shape[-1] >= 7:
        nraw = torch.sum(w[..., None] * raw[..., 4:7], -2)
        normal = nraw / torch.norm(nraw, dim=-1, keepdim=True).clamp(min=1e-12)
    return rgb, disp, acc, w, depth, entropy, normal


def entropy_probs(w):
    """torch.distributions.Categorical(probs=[w, max(1 - sum w, 1e-6)]).probs (run_nerf.py:404-406): [R, S + 1]."""
    probs = torch.cat([w, (1.0 - w.sum(-1, keepdim=True)).clamp(min=1e-6)], -1)
    return probs / probs.sum(-1, keepdim=True)


def composite_grad(raw, z, rays_d, noise, white_bkgd, grads, dtype=torch.float64):
    """d sum_k <out_k, grads[k]> / d raw by autograd; grads maps GRAD_NAMES to arrays, a missing or None entry is a
    NULL upstream gradient. -> (graw [R, S, C] of `dtype`, the forward outputs, detached)."""
    leaf = _t(raw, dtype).clone().requires_grad_(True)
    out = composite(leaf, z, rays_d, noise, white_bkgd, dtype)
    loss = None
    for name, o in zip(GRAD_NAMES, out):
        g = grads.get(name)
        if g is None or o is None:
            continue
        term = (o * _t(g, dtype)).sum()
        loss = term if loss is None else loss + term
    loss.backward()
    return leaf.grad, tuple(None if o is None else o.detach() for o in out)


def sample_pdf(bins, weights, u, dtype=torch.float64):
    """sample_pdf with given uniforms u [R, N] (run_nerf_helpers.py:354-397)."""
    bins, weights, u = _t(bins, dtype), _t(weights, dtype), _t(u, dtype).contiguous()
    weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    hi_idx = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(hi_idx - 1, min=0)
    above = torch.clamp(hi_idx, max=cdf.shape[-1] - 1)
    cdf_lo, cdf_hi = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bin_lo, bin_hi = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = cdf_hi - cdf_lo
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_lo) / denom
    return bin_lo + t * (bin_hi - bin_lo)


def bin_mass(weights, dtype=torch.float64):
    """Probability mass of every bin of sample_pdf's pdf ([R, nb - 1]): below 1e-5 the `denom < 1e-5 -> 1` rule
    makes the sample jump with one ulp of the float32 CDF."""
    w = _t(weights, dtype) + 1e-5
    return w / w.sum(-1, keepdim=True)


def sample_fine(z, weights, u, dtype=torch.float64):
    """The hierarchical step of render_rays (run_nerf.py:508-513, :541) on coarse depths z [R, S] and coarse weights
    [R, S]: -> (samples [R, N], z_fine [R, S + N] sorted, z_std [R] population)."""
    z = _t(z, dtype)
    zmid = 0.5 * (z[..., 1:] + z[..., :-1])
    samples = sample_pdf(zmid, _t(weights, dtype)[..., 1:-1], u, dtype)
    z_fine = torch.sort(torch.cat([z, samples], -1), -1).values
    return samples, z_fine, torch.std(samples, dim=-1, unbiased=False)


def tv_sum(oracle, table, min_vertex, cube, log2_T):
    """total_variation_loss (loss.py:11-43) of one level over the cuboid at min_vertex, summed in float64."""
    table = torch.as_tensor(table).double()
    ar = torch.arange(cube + 1)
    mv = [int(v) for v in min_vertex]
    gx, gy, gz = torch.meshgrid(mv[0] + ar, mv[1] + ar, mv[2] + ar, indexing="ij")
    idx = oracle.spatial_hash(torch.stack([gx, gy, gz], -1), log2_T)
    e = table[idx]
    tx = torch.pow(e[1:] - e[:-1], 2).sum()
    ty = torch.pow(e[:, 1:] - e[:, :-1], 2).sum()
    tz = torch.pow(e[:, :, 1:] - e[:, :, :-1], 2).sum()
    return float((tx + ty + tz) / cube), int(idx.numel() - torch.unique(idx).numel())


# ---------------------------------------------------------------- compositing cases
# Each template of NERF_COMPOSITE_DISPATCH (K = 1, 2, 3, 4, 6, 8 samples per lane) at both edges, K = 5 .. 6 inside
# the K = 6 template (S = 257 .. 384 pads every lane), and S = 1 and 2.
WIDTHS = (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 300, 320, 321, 384, 385, 448, 512)
WIDTHS_ONE_RAY = (1, 64, 300, 512)                  # R = 1: one wave of one block
WIDTHS_NORMALS = (63, 128, 192, 256, 300, 384, 512)  # C = 7: one S per template (two for K = 6: K = 5 and K = 6)
ALONE_S = 300                                        # every upstream gradient alone at this width
EDGE_WIDTHS = (130, 300)


def composite_cases():
    """(S, R, C, white, noise) of every random case: R = 9 (two blocks and one wave) at every width, white background
    and noise alternating so that each is on for half the cases and the four combinations all occur."""
    cases = []
    for i, S in enumerate(WIDTHS):
        cases.append((S, 9, 4, i % 2, ((i + 1) // 2) % 2))
    for i, S in enumerate(WIDTHS_ONE_RAY):
        cases.append((S, 1, 4, (i + 1) % 2, i // 2))
    for i, S in enumerate(WIDTHS_NORMALS):
        cases.append((S, 9, 7, (i // 2) % 2, (i + 1) % 2))
    return cases


def case_seed(S, R, C, white, noise):
    return ((S * 16 + R) * 8 + C) * 4 + 2 * white + noise


@functools.lru_cache(maxsize=None)
def composite_inputs(S, R, C, white, noise):
    """raw = 2 * randn, z sorted in [2, 6], rays_d = randn, noise = randn or None, and every upstream gradient."""
    rng = np.random.RandomState(case_seed(S, R, C, white, noise))
    f = np.float32
    d = dict(raw=(2 * rng.randn(R, S, C)).astype(f), z=np.sort(2 + 4 * rng.rand(R, S), -1).astype(f),
             rays_d=rng.randn(R, 3).astype(f), noise=rng.randn(R, S).astype(f) if noise else None,
             g_rgb=rng.randn(R, 3).astype(f), g_disp=rng.randn(R).astype(f), g_acc=rng.randn(R).astype(f),
             g_weights=(0.1 * rng.randn(R, S)).astype(f), g_depth=rng.randn(R).astype(f),
             g_entropy=rng.randn(R).astype(f), g_normal=rng.randn(R, 3).astype(f) if C == 7 else None)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


REST = tuple(n for n in GRAD_NAMES if n != "g_entropy")


@functools.lru_cache(maxsize=None)
def composite_reference(S, R, C, white, noise, which):
    """The float64 forward and the raw gradient for the upstream gradients named in `which` (a tuple of GRAD_NAMES)."""
    d = composite_inputs(S, R, C, white, noise)
    grads = {n: d[n] for n in which}
    graw, out = composite_grad(d["raw"], d["z"], d["rays_d"], d["noise"], bool(white), grads)
    return graw.numpy(), tuple(None if o is None else o.numpy() for o in out)


def entropy_excluded(weights64):
    """[R, S] mask of the samples whose reference p_j lies where the entropy gradient jumps (the clamp's mask), so
    that channel 3 of those elements is left out of the entropy bar: within 1e-3 relative of eps, or within 2 eps
    (absolute) of 1 - eps. The second window is narrower than 1e-3 relative to 1 - eps, which would take every
    p_j > 0.999 (each opaque ray of S = 1 and 2, where p = 1 - 1e-6) out of the check; 2 eps = 2.4e-7 still covers
    the kernel's p = fl(fl(w) / fl(Z)), three float32 roundings (1.8e-7) away from the exact quotient."""
    p = entropy_probs(torch.as_tensor(weights64).double())[..., :-1].numpy()
    return (np.abs(p - EPS32) <= 1e-3 * EPS32) | (np.abs(p - (1 - EPS32)) <= 2 * EPS32)


def entropy_ratio(graw, graw_ref, excluded):
    """max over the compared elements of |err| / max_j |graw_ref[ray]| (0 for a ray whose reference is all zero and
    whose error is zero), and the excluded share of all elements."""
    err = np.abs(np.asarray(graw, np.float64) - graw_ref)
    err[..., 3][excluded] = 0.0
    scale = np.abs(graw_ref).reshape(graw_ref.shape[0], -1).max(-1)
    worst = err.reshape(err.shape[0], -1).max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(worst == 0, 0.0, worst / scale)
    return float(ratio.max()), float(excluded.sum()) / err.size


@functools.lru_cache(maxsize=None)
def edge_batch(S):
    """Four rays as rows of one batch (C = 4, no noise): 0 every sigma <= 0 (two of them exactly 0); 1 an opaque
    first sample (sigma = 50 over a step of 1); 2 dense everywhere, so 1 - acc < 1e-6 (the entropy's clamp branch);
    3 tied z values in runs of three (delta = 0 inside a run). Rows 4..8 are plain random rays."""
    rng = np.random.RandomState(1000 + S)
    f = np.float32
    R = 9
    raw = (2 * rng.randn(R, S, 4)).astype(f)
    z = np.sort(2 + 4 * rng.rand(R, S), -1).astype(f)
    raw[0, :, 3] = -np.abs(raw[0, :, 3])
    raw[0, 5, 3] = 0.0
    raw[0, S - 1, 3] = -0.0
    raw[1, 0, 3] = 50.0
    z[1, 0] = 2.0
    z[1, 1:] = np.sort(3 + 3 * rng.rand(S - 1)).astype(f)
    raw[2, :, 3] = 5.0 + np.abs(raw[2, :, 3])
    z[3] = np.repeat(z[3, ::3], 3)[:S]
    d = dict(raw=raw, z=z, rays_d=rng.randn(R, 3).astype(f), g_rgb=rng.randn(R, 3).astype(f),
             g_entropy=rng.randn(R).astype(f))
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def edge_reference(S, which):
    d = edge_batch(S)
    graw, out = composite_grad(d["raw"], d["z"], d["rays_d"], None, False, {n: d[n] for n in which})
    return graw.numpy(), tuple(None if o is None else o.numpy() for o in out)


# Measured on the CPU (entropy_oracle_worst, pinned by test_composite_ref_cpu.py): the float32 oracle's worst ratio
# is 1.341e-4 (S = 300, R = 9, C = 7); by template K = 1, 2, 3, 4, 6, 8: 9.6e-6, 5.5e-6, 2.0e-5, 2.3e-5, 1.3e-4,
# 5.0e-5. Nothing is excluded for these inputs (share 0). The kernels' bar is four times the oracle's worst.
ENT_ORACLE_WORST = 1.341e-4
ENT_BAR = 4 * ENT_ORACLE_WORST
ENT_EXCLUDED_MAX = 1e-3


def entropy_oracle_worst():
    """The entropy bar's yardstick: over every random case and both edge batches, the worst entropy_ratio of the
    float32 autograd oracle (composite with dtype=float32: float32's eps, which is the clamp fix) against the float64
    reference, g_entropy alone. -> (worst ratio, worst excluded share, {case: ratio})."""
    ratios, shares = {}, []
    for case in composite_cases():
        d = composite_inputs(*case)
        g64, out64 = composite_reference(*case, ("g_entropy",))
        g32, _ = composite_grad(d["raw"], d["z"], d["rays_d"], d["noise"], bool(case[3]),
                                {"g_entropy": d["g_entropy"]}, torch.float32)
        ratios[case], share = entropy_ratio(g32.numpy(), g64, entropy_excluded(out64[3]))
        shares.append(share)
    for S in EDGE_WIDTHS:
        d = edge_batch(S)
        g64, out64 = edge_reference(S, ("g_entropy",))
        g32, _ = composite_grad(d["raw"], d["z"], d["rays_d"], None, False, {"g_entropy": d["g_entropy"]},
                                torch.float32)
        ratios[("edge", S)], share = entropy_ratio(g32.numpy(), g64, entropy_excluded(out64[3]))
        shares.append(share)
    return max(ratios.values()), max(shares), ratios


# ---------------------------------------------------------------- sampler cases
SAMPLER_S = (3, 66, 67, 130, 131, 194, 195, 256)     # build_cdf's per = ceil((S - 2) / 64) = 1 .. 4 at both edges
SAMPLER_N = (1, 63, 65, 128, 129, 256, 700)          # register bitonic H = 1, 2; LDS bitonic; rank sort at S = 256
MAX_MERGED = 1024                                    # kMaxMerged (csrc/sampling.hip)
MIN_BIN_MASS = 6.5e-4                                # under the smallest bin mass of the sampler cases (6.79e-4, CPU test)


def sampler_cases():
    """Every S with three of the N and every N with several S, so that each width of build_cdf (per = 1 .. 4) meets
    the register sort with one and with two elements per lane and the LDS sort (test_composite_ref_cpu.py); N = 700
    only where S + N fits the merged row, with (256, 700) the rank-sort fallback (S + P2 = 1280)."""
    cases = []
    for i, S in enumerate(SAMPLER_S):
        for k in range(3):
            N = SAMPLER_N[(i + 2 * k) % len(SAMPLER_N)]
            if S + N <= MAX_MERGED and (S, N) not in cases:
                cases.append((S, N))
    for extra in ((256, 700), (3, 1), (256, 256), (195, 129), (66, 700)):
        if extra not in cases:
            cases.append(extra)
    return cases


def sort_path(S, N):
    """The path sample_fine_ray takes for sorted coarse depths: 'reg1' / 'reg2' (register bitonic, one or two
    elements per lane), 'lds' (LDS bitonic), 'rank' (rank sort: S + P2 > 1024)."""
    P2 = 1
    while P2 < N:
        P2 <<= 1
    if S + P2 > MAX_MERGED:
        return "rank"
    return "reg1" if P2 <= 64 else "reg2" if P2 <= 128 else "lds"


@functools.lru_cache(maxsize=None)
def sampler_inputs(S, N, R=9):
    """rays [R, 11] (origin, direction, near, far, view direction), coarse z sorted in [2, 6], weights uniform in
    [0.1, 1], uniforms u in [0, 1)."""
    rng = np.random.RandomState(S * 1000 + N)
    f = np.float32
    d = dict(rays=rng.randn(R, 11).astype(f), z=np.sort(2 + 4 * rng.rand(R, S), -1).astype(f),
             w=(0.1 + 0.9 * rng.rand(R, S)).astype(f), u=rng.rand(R, N).astype(f))
    for v in d.values():
        v.setflags(write=False)
    return d


FUSED_CASES = ((128, 64), (100, 129))                # nerf_composite_sample_fine: K = 2; register sort and LDS sort


@functools.lru_cache(maxsize=None)
def fused_inputs(S, N, R=9):
    """A thin medium, so that every bin of the coarse pdf carries mass (asserted on the CPU): sigma in [0.3, 0.6],
    unit directions, depths jittered inside the middle half of S even strata of [2, 6]."""
    rng = np.random.RandomState(S * 1000 + N + 7)
    f = np.float32
    raw = (2 * rng.randn(R, S, 4)).astype(f)
    raw[..., 3] = (0.3 + 0.3 * rng.rand(R, S)).astype(f)
    z = (2 + 4 * (np.arange(S)[None] + 0.25 + 0.5 * rng.rand(R, S)) / S).astype(f)
    dirs = rng.randn(R, 3)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    rays = rng.randn(R, 11).astype(f)
    rays[:, 3:6] = dirs.astype(f)
    d = dict(raw=raw, z=z, rays=rays, rays_d=np.ascontiguousarray(rays[:, 3:6]), u=rng.rand(R, N).astype(f))
    for v in d.values():
        v.setflags(write=False)
    return d
