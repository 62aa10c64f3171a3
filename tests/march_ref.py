"""What the tests of the grid march's backward share (test_march_grad_cpu.py, test_gpu_march_bwd.py):
a float64 restatement of the packed compositing (nerf_march_composite: raw2outputs, run_nerf.py:347-411, over a list
of variable-length segments with an explicit distance per entry) whose backward is torch autograd, and the seeded
inputs of the kernel test. No test and no fixture lives here.

Every input is a float32 value promoted exactly to float64. A ray's segment is entries [offsets[r], offsets[r + 1])
of the list; a ray with an empty segment has rgb 0 (1 with a white background), acc 0 and NaN depth and disp, and
takes no part in the backward."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

GRAD_NAMES = ("g_rgb", "g_disp", "g_acc", "g_depth", "g_weights")     # nerf_packed_composite_bwd's order


def _t(x):
    return x.double() if torch.is_tensor(x) else torch.tensor(np.asarray(x)).double()


def segment(raw, z, dist, d, white_bkgd=False):
    """One ray: raw [S, 4], z [S], dist [S] (S >= 1), d [3] -> (rgb [3], disp, acc, weights [S], depth)."""
    delta = dist * torch.linalg.vector_norm(d)
    alpha = 1.0 - torch.exp(-F.relu(raw[:, 3]) * delta)
    trans = torch.cumprod(torch.cat([alpha.new_ones(1), 1.0 - alpha + 1e-10]), 0)[:-1]
    w = alpha * trans
    rgb = (w[:, None] * torch.sigmoid(raw[:, :3])).sum(0)
    acc = w.sum()
    depth = (w * z).sum() / acc
    disp = 1.0 / torch.maximum(torch.full_like(depth, 1e-10), depth)
    if white_bkgd:
        rgb = rgb + (1.0 - acc)
    return rgb, disp, acc, w, depth


def composite(raw, z, dist, rays_d, offsets=None, white_bkgd=False):
    """The packed list (offsets None: one segment, rays_d [3] or [1, 3]) -> rgb [R, 3], disp [R], acc [R],
    weights [n], depth [R]; entries outside every segment get weight 0."""
    if not (torch.is_tensor(raw) and raw.dtype == torch.float64):     # a float64 tensor is used as it is (a leaf)
        raw = _t(raw)
    z, dist, rays_d = _t(z), _t(dist), _t(rays_d).reshape(-1, 3)
    n = raw.shape[0]
    off = [0, n] if offsets is None else [min(max(int(o), 0), n) for o in np.asarray(offsets).reshape(-1)]
    rgb, disp, acc, depth, ws = [], [], [], [], torch.zeros(n, dtype=torch.float64)
    parts = []
    for r in range(len(off) - 1):
        b, e = min(off[r], off[r + 1]), off[r + 1]
        if e <= b:
            bg = 1.0 if white_bkgd else 0.0
            rgb.append(raw.new_full((3,), bg)); acc.append(raw.new_zeros(())); depth.append(raw.new_full((), float("nan")))
            disp.append(raw.new_full((), float("nan")))
            continue
        c, dp, a, w, de = segment(raw[b:e], z[b:e], dist[b:e], rays_d[r], white_bkgd)
        rgb.append(c); disp.append(dp); acc.append(a); depth.append(de)
        parts.append((b, e, w))
    for b, e, w in parts:      # segments of a march do not overlap
        ws = torch.cat([ws[:b], w, ws[e:]])
    return torch.stack(rgb), torch.stack(disp), torch.stack(acc), ws, torch.stack(depth)


def composite_grad(raw, z, dist, rays_d, offsets, white_bkgd, grads):
    """d sum_k <out_k, grads[k]> / d raw by autograd over the rays with a segment; grads maps GRAD_NAMES to arrays, a
    missing or None entry is a NULL upstream gradient. -> (graw [n, 4] float64, the forward outputs, detached)."""
    leaf = _t(raw).clone().requires_grad_(True)
    rgb, disp, acc, w, depth = composite(leaf, z, dist, rays_d, offsets, white_bkgd)
    live = ~torch.isnan(depth.detach())       # an empty segment: constant outputs, NaN depth
    loss = leaf.sum() * 0.0
    for name, o in zip(GRAD_NAMES, (rgb, disp, acc, depth, w)):
        g = grads.get(name)
        if g is None:
            continue
        g = _t(g)
        loss = loss + ((o * g).sum() if name == "g_weights" else (o[live] * g[live]).sum())
    loss.backward()
    return leaf.grad, tuple(o.detach() for o in (rgb, disp, acc, w, depth))


# ---------------------------------------------------------------- the kernel test's inputs
# R = 13 (not a multiple of the four rays of a block); the empty rays first, in the middle and last; 4097 needs 65
# tiles of 64 entries, 8200 spans three super-blocks of 64 tiles with a ragged tail
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 300, 0, 4096, 4097, 8200, 0)
UNIFORM_SIGMA = (1, 2, 4, 6, 10)      # these segments' sigma is uniform in [0.3, 0.6] (the short ones among them: a
#                                       ray whose sigmas all come out <= 0 has a zero gradient); the rest 2 randn
GRAD_SETS = (GRAD_NAMES,) + tuple((n,) for n in GRAD_NAMES)


def _segment_inputs(i, S):
    rng = np.random.default_rng(1000 + i)
    raw = (2.0 * rng.standard_normal((S, 4))).astype(np.float32)
    if i in UNIFORM_SIGMA:
        raw[:, 3] = rng.uniform(0.3, 0.6, S).astype(np.float32)
    z = np.sort(rng.uniform(2.0, 6.0, S)).astype(np.float32)
    dist = np.empty(S, np.float32)
    dist[:-1] = z[1:] - z[:-1]
    dist[-1] = np.float32(1e10) if i % 2 == 0 else np.float32(0.01)
    return raw, z, dist


def _upstream(rng, R, n):
    return dict(g_rgb=rng.standard_normal((R, 3)).astype(np.float32), g_disp=rng.standard_normal(R).astype(np.float32),
                g_acc=rng.standard_normal(R).astype(np.float32), g_depth=rng.standard_normal(R).astype(np.float32),
                g_weights=rng.standard_normal(n).astype(np.float32))


@functools.lru_cache(maxsize=None)
def main_inputs():
    """The list of LENGTHS: raw [n, 4], z, dist [n], offsets int32 [R + 1], rays_d [R, 3] and the five upstream
    gradients (read-only arrays)."""
    segs = [_segment_inputs(i, S) for i, S in enumerate(LENGTHS) if S > 0]
    d = dict(raw=np.concatenate([s[0] for s in segs]), z=np.concatenate([s[1] for s in segs]),
             dist=np.concatenate([s[2] for s in segs]),
             offsets=np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32))
    rng = np.random.default_rng(7)
    d["rays_d"] = rng.standard_normal((len(LENGTHS), 3)).astype(np.float32)
    d.update(_upstream(rng, len(LENGTHS), d["raw"].shape[0]))
    for v in d.values():
        v.setflags(write=False)
    return d


DEAD_LENGTHS = (70, 100, 130)     # ray 0: every sigma <= 0; ray 1: an ordinary ray; ray 2: an opaque first sample
DEAD_GRADS = ("g_rgb", "g_acc", "g_weights")


@functools.lru_cache(maxsize=None)
def dead_inputs():
    """Three rays: one whose sigmas are all <= 0 (one exact 0 and one -0.0 among them: no sigma gradient at all), an
    ordinary one between, and one whose first sample is opaque (sigma 1e4: alpha = 1, T = 1e-10 behind it)."""
    segs = [_segment_inputs(100 + i, S) for i, S in enumerate(DEAD_LENGTHS)]
    segs[0][0][:, 3] = -np.abs(segs[0][0][:, 3])
    segs[0][0][5, 3] = 0.0
    segs[0][0][66, 3] = -0.0
    segs[2][0][0, 3] = 1e4
    segs[2][1][1] = segs[2][1][0] + np.float32(0.05)      # a first interval that is not tiny
    segs[2][1][:] = np.sort(segs[2][1])
    segs[2][2][:-1] = segs[2][1][1:] - segs[2][1][:-1]
    d = dict(raw=np.concatenate([s[0] for s in segs]), z=np.concatenate([s[1] for s in segs]),
             dist=np.concatenate([s[2] for s in segs]),
             offsets=np.concatenate([[0], np.cumsum(DEAD_LENGTHS)]).astype(np.int32))
    rng = np.random.default_rng(11)
    d["rays_d"] = rng.standard_normal((3, 3)).astype(np.float32)
    d.update(_upstream(rng, 3, d["raw"].shape[0]))
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(which, white, dead=False):
    """composite_grad of main_inputs() (dead: dead_inputs()) with the upstream gradients named in `which` -> (graw
    [n, 4], outputs) as float64 arrays, computed once per set."""
    d = dead_inputs() if dead else main_inputs()
    g, out = composite_grad(d["raw"], d["z"], d["dist"], d["rays_d"], d["offsets"], white, {k: d[k] for k in which})
    g, out = g.numpy(), tuple(o.numpy() for o in out)
    g.setflags(write=False)
    return g, out


def ray_max(g, offsets):
    """max |g| over each ray's segment ([R]; 0 for an empty one)."""
    return np.array([np.abs(g[offsets[r]:offsets[r + 1]]).max() if offsets[r + 1] > offsets[r] else 0.0
                     for r in range(len(offsets) - 1)])
