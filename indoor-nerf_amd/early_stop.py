"""Early ray termination for forward-only rendering.

render_rays(..., early_stop=eps) runs each field call front to back in slabs of early_stop_slab samples
(run_network_early_stop): the samples of the rays still alive — inside the box and, with an occupancy
grid, in an occupied cell — are compacted in ascending order (csrc/early_stop.hip), hash-encoded and run
through the MLP; after every slab but the last each ray alive adds the slab to its optical depth and dies
for all later slabs once tau > -log(eps). A sample of a dead ray gets an all-zero raw row, exactly as a
sample the grid skips, so the composited maps are the dense ones with sigma masked per sample, and each
pass differs from its unmasked self by at most eps per channel.

    render_kwargs_test["early_stop"] = 1e-3             # render / render_path stop rays at T < 1e-3
    render_kwargs_test["occupancy"] = grid               # optional: composes with an OccupancyGrid

Forward-only, with the occupancy path's refusals (occupancy.py).
"""
import math

import numpy as np
import torch

from . import _lib
from .hashgrid import SHEncoder
from .occupancy import _check_modules

_LAST = {"counts": (0, 0)}


def last_counts():
    """(points evaluated, points total) of the most recent field call, summed over its slabs."""
    return _LAST["counts"]


def check_params(early_stop, early_stop_slab):
    """(eps, K) of render_rays' keyword arguments, or ValueError."""
    eps = float(early_stop)
    if not 0.0 < eps < 1.0:
        raise ValueError(f"render_rays: early_stop must be a transmittance threshold in (0, 1), got {early_stop}")
    if int(early_stop_slab) != early_stop_slab or int(early_stop_slab) < 1:
        raise ValueError(f"render_rays: early_stop_slab must be an integer >= 1, got {early_stop_slab}")
    return eps, int(early_stop_slab)


def tau_max_of(eps):
    """float32(-log(eps)): the logarithm in double on the host, rounded once."""
    return float(np.float32(-math.log(eps)))


class EarlyStopRequest:
    """render_rays' early-termination request on its way to the fused run_network (attached to the point
    tensor as `pts._nerf_early_stop`): the pass's z [R, S] and rays_d [R, 3], eps, the slab size and the
    optional occupancy grid. run_network sets `used` (a foreign query function leaves it False and
    render_rays raises) and `stop` (int32 [R]: leading samples for which the ray was alive)."""

    def __init__(self, z, rays_d, eps, slab, grid=None):
        self.z, self.rays_d, self.eps, self.slab, self.grid = z, rays_d, eps, slab, grid
        self.used, self.stop = False, None


def run_network_early_stop(inputs, viewdirs, fn, embed_fn, embeddirs_fn, req):
    """run_network (field.py) with early ray termination: inputs [R, S, 3], viewdirs [R, 3] -> raw [R, S, 4]
    with the field evaluated at the kept samples only and zero rows elsewhere; req.stop receives the stops."""
    from .field import _point_order, _weights_struct
    if not isinstance(embeddirs_fn, SHEncoder) or viewdirs is None or inputs.dim() != 3:
        raise ValueError("early_stop: needs the fused field call (SHEncoder view encoding, viewdirs, inputs [R, S, 3])")
    _check_modules(embed_fn, fn, "early_stop")
    if fn.raw_channels != 4:
        raise ValueError("early_stop: a normals head is not supported (run_network's box mask then lands on n_z, "
                         "not on sigma, so a skipped sample is not a zero-weight sample)")
    if torch.is_grad_enabled():
        raise ValueError("early_stop: forward-only (call under torch.no_grad(); rays are not stopped in training)")
    if embed_fn.training:
        embed_fn.current_step += 1
    R, S = inputs.shape[0], inputs.shape[1]
    P, dev, K = R * S, inputs.device, req.slab
    if 16 * (P + 32) >= 2 ** 31:
        raise ValueError(f"early_stop: {P} points per field call exceed the MLP's 32-bit row indexing; use a smaller chunk")
    if tuple(req.z.shape) != (R, S) or tuple(req.rays_d.shape) != (R, 3):
        raise ValueError("early_stop: z / rays_d of the request do not match the points")
    pts = inputs.detach().reshape(-1, 3).float().contiguous()
    sh_rays = getattr(viewdirs, "_nerf_sh", None)
    viewdirs = viewdirs.detach().float().contiguous()
    z, rays_d = req.z.detach().float().contiguous(), req.rays_d.detach().float().contiguous()
    grid = req.grid
    if grid is not None:
        bmin, bmax, res, bits = grid._bmin, grid._bmax, grid.resolution, grid._bits()
    else:
        bmin, bmax, res, bits = embed_fn._meta["bmin"], embed_fn._meta["bmax"], 1, None   # the encoder's own box
    tau_max = tau_max_of(req.eps)

    f, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    raw = torch.empty(P, 4, **f)
    tau = torch.zeros(R, **f)
    alive = torch.ones(R, device=dev, dtype=torch.uint8)
    stop = torch.full((R,), S, **i32)
    # scratch of the worst-case slab (every candidate kept), once per field call
    cap, L = R * min(K, S), embed_fn.n_levels
    count = torch.empty(1, **i32)
    ws = torch.empty(int(_lib.load().nerf_ert_compact_workspace_bytes(cap)) // 4, **i32)
    rows, pts_c, sh_c = torch.empty(cap, **i32), torch.empty(cap, 3, **f), torch.empty(cap, 16, **f)
    feat, keep = torch.empty(L * cap * 2, **f), torch.empty(cap, device=dev, dtype=torch.bool)
    weights = _weights_struct(fn.mlp_weights())
    evaluated = 0

    def compact(s0, s1, stages, n):
        _lib.call("nerf_ert_compact", _lib.ptr(pts, "pts"), R, S, s0, s1, _lib.ptr(alive, "alive", torch.uint8),
                  _lib.ptr(sh_rays, "sh_rows", allow_none=True),
                  None if sh_rays is not None else _lib.ptr(viewdirs, "viewdirs"), bmin, bmax, res, bits, stages, n,
                  _lib.ptr(rows, "rows", torch.int32), _lib.ptr(count, "count", torch.int32),
                  _lib.ptr(pts_c, "pts_c"), _lib.ptr(sh_c, "sh_c"), _lib.ptr(raw, "raw"),
                  _lib.ptr(ws, "workspace", torch.int32), ws.numel() * 4, _lib.stream())

    for s0 in range(0, S if R > 0 else 0, K):
        s1 = min(s0 + K, S)
        compact(s0, s1, 1, 0)
        n = int(count.item())      # one 4-byte host read per slab sizes the encode and MLP launches
        compact(s0, s1, 2, n)
        if n > 0:
            ft = feat[:L * n * 2]
            embed_fn.encode_into(pts_c[:n], ft, 2, 2 * n, keep[:n])
            _lib.call("nerf_mlp_fwd_ord", _lib.ptr(ft, "feat"), 2, 2 * n, _lib.ptr(sh_c, "sh_c"), 16, None, 1,
                      _lib.ptr(keep, "keep", torch.bool), n, weights, _lib.ptr(raw, "raw"),
                      None, None, None, 0, _point_order((rows, 0, 0)), _lib.stream())
        evaluated += n
        if s1 < S:
            _lib.call("nerf_ert_advance", _lib.ptr(raw, "raw"), _lib.ptr(z, "z"), _lib.ptr(rays_d, "rays_d"), R, S,
                      s0, s1, tau_max, _lib.ptr(tau, "tau"), _lib.ptr(alive, "alive", torch.uint8),
                      _lib.ptr(stop, "stop", torch.int32), _lib.stream())
    _LAST["counts"] = (evaluated, P)
    req.stop = stop
    return raw.reshape(R, S, 4)
