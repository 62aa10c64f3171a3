"""Volumetric renderer on the HIP kernels.

API mirror of PocketNeRF/run_nerf.py:71-151, :347-549 (batchify_rays, render, raw2outputs,
render_rays) and PocketNeRF/run_nerf_helpers.py:10-13, :311-397 (img2mse, mse2psnr, to8b,
get_rays, get_rays_np, ndc_rays, sample_pdf). Sampling, compositing and the hierarchical
resampling run in libnerfhip (csrc/sampling.hip, csrc/composite.hip); the field query goes
through network_query_fn (field.run_network -> the fused hash-grid + MLP kernels).

Randomness: pytest=True reproduces the reference's np.random.seed(0) draws exactly; otherwise
stratified jitter and importance uniforms are drawn in-kernel (Philox4x32-10) from a seed taken
from torch's CPU generator, and raw noise uses torch.randn like the reference.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, sparse_field
from .hashgrid import early_tv

img2mse = lambda x, y: torch.mean((x - y) ** 2)  # noqa: E731
# The reference divides by torch.log(torch.Tensor([10.])) (a [1] float32 tensor): same value and shape
# here without creating a device tensor from host data (that copy would synchronise the stream).
mse2psnr = lambda x: (-10. * torch.log(x) / _LOG10_F32).reshape(1)  # noqa: E731
_LOG10_F32 = float(np.float32(np.log(10.0)))
to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)  # noqa: E731

_LINSPACE = {}
_SEED_GEN = None

# run_nerf.py:40 DEBUG: when True, render_rays tests every returned tensor for NaN/Inf (one fused
# device count, csrc/checks.hip, and one host read per call) and prints the reference's message.
# The package namespace re-exports the render() function under this module's name, so set it with
# set_debug() (or on the module: importlib.import_module("indoor_nerf_amd.render").DEBUG).
DEBUG = False


def set_debug(enabled=True):
    """run_nerf.py:40's module flag (DEBUG = True) for this package."""
    global DEBUG
    DEBUG = bool(enabled)


def check_numerics(ret):
    """run_nerf.py:545-547 over the tensors of `ret`; returns the keys that hold NaN/Inf."""
    items = [(k, v) for k, v in ret.items() if torch.is_tensor(v) and v.dtype == torch.float32 and v.is_cuda]
    bad = []
    for i in range(0, len(items), _lib.MAX_CHECK):
        part = items[i:i + _lib.MAX_CHECK]
        ts = [v.contiguous() for _, v in part]
        counts = torch.empty(len(ts), dtype=torch.int32, device=ts[0].device)
        sizes = (_lib.c_i64 * len(ts))(*[t.numel() for t in ts])
        _lib.call("nerf_count_nonfinite", _lib.ptr_array(ts, "ret"), sizes, len(ts),
                  _lib.ptr(counts, "counts", dtype=torch.int32), _lib.stream())
        bad += [k for (k, _), c in zip(part, counts.tolist()) if c]
    for k in bad:
        print(f"! [Numerical Error] {k} contains nan or inf.")
    return bad


def _linspace(n, device):
    key = (n, str(device))
    if key not in _LINSPACE:
        _LINSPACE[key] = torch.linspace(0., 1., steps=n).to(device)   # CPU linspace values, as the reference
    return _LINSPACE[key]


def _draw_seed():
    global _SEED_GEN
    if _SEED_GEN is None:
        _SEED_GEN = torch.Generator().manual_seed(torch.initial_seed() & ((1 << 63) - 1))
    s = torch.randint(0, 2 ** 62, (2,), generator=_SEED_GEN)
    return int(s[0]), int(s[1])


def _rng():
    """(seed, offset, d_rng) for an in-kernel Philox draw. Eager: a fresh host seed. While a
    training step is being captured (graphs.GraphedTrainStep): two device slots that a filler
    refreshes with a fresh seed before every replay."""
    from . import graphs
    sc = graphs.active()
    if sc is None:
        s, o = _draw_seed()
        return s, o, None
    off, ptr = sc.alloc_i64(2)

    def fill(hi, hf, off=off):
        s, o = _draw_seed()
        hi[off], hi[off + 1] = s, o
    sc.add_filler(fill)
    return 0, 0, _lib.c_vp(ptr)


def manual_seed(seed):
    """Seed the in-kernel Philox draws (stratified jitter, importance uniforms)."""
    global _SEED_GEN
    _SEED_GEN = torch.Generator().manual_seed(int(seed))


_PYTEST_SHARD = (0, 1)


def pytest_shard(rank, world):
    """pytest=True draws for a data-parallel shard: every draw then takes the reference's
    np.random.seed(0) uniforms for the GLOBAL batch (world x this rank's rays, run_nerf.py:482-486,
    run_nerf_helpers.py:368-377) and keeps this rank's contiguous rows, so that G shards see exactly
    the draws one process sees for the whole batch (tests/test_gpu_dist.py). (0, 1) = off."""
    global _PYTEST_SHARD
    if not (0 <= rank < world):
        raise ValueError(f"pytest_shard: rank {rank} of {world}")
    _PYTEST_SHARD = (int(rank), int(world))


def _pytest_uniforms(shape, device):
    np.random.seed(0)
    rank, world = _PYTEST_SHARD
    if world == 1:
        return torch.from_numpy(np.random.rand(*shape).astype(np.float32)).to(device)
    full = np.random.rand(shape[0] * world, *shape[1:]).astype(np.float32)
    return torch.from_numpy(full[rank * shape[0]:(rank + 1) * shape[0]]).to(device)


# ---------------------------------------------------------------- compositing

class CompositeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, z, rays_d, noise, white_bkgd, sampler=None, defer=False):
        if z.requires_grad or rays_d.requires_grad:
            raise NotImplementedError("raw2outputs: gradients w.r.t. z_vals / rays_d are not implemented "
                                      "(the reference detaches both)")
        ctx.set_materialize_grads(False)
        raw = raw.contiguous()
        z = z.contiguous().float()
        rays_d = rays_d.contiguous().float()
        R, S, C = raw.shape
        dev = raw.device
        f = dict(device=dev, dtype=torch.float32)
        rgb, disp, acc = torch.empty(R, 3, **f), torch.empty(R, **f), torch.empty(R, **f)
        weights, depth, ent = torch.empty(R, S, **f), torch.empty(R, **f), torch.empty(R, **f)
        normal = torch.empty(R, 3, **f) if C == 7 else None
        cargs = (_lib.ptr(raw, "raw"), C, _lib.ptr(z, "z_vals"), _lib.ptr(rays_d, "rays_d"),
                 _lib.ptr(noise, "noise", allow_none=True), R, S, int(bool(white_bkgd)), _lib.ptr(rgb, "rgb"),
                 _lib.ptr(disp, "disp"), _lib.ptr(acc, "acc"), _lib.ptr(weights, "weights"), _lib.ptr(depth, "depth"),
                 _lib.ptr(ent, "entropy"), _lib.ptr(normal, "normal", allow_none=True))
        tv = early_tv(dev) if sampler is None else None
        if tv is not None:   # a captured step's TV forward in the same launch (losses.tv_forward_early)
            from .hashgrid import join_tables
            join_tables(dev)                    # a pending all-gather of table levels (dist.py): TV reads them all
            _lib.flush_zero_fills([tv.out])     # its accumulator's fill: normally done by nerf_rays_pack_z
            job = _lib.TVFwdJob(_lib.c_vp(ctypes.addressof(tv.ptrs)), None, tv.dmv, _lib.c_vp(ctypes.addressof(tv.cb)),
                                _lib.ptr(tv.out, "tv_loss"), _lib.ptr(tv.verts, "tv_verts"))
            _lib.call("nerf_composite_fwd_tv", *cargs, ctypes.byref(job), len(tv.tables), tv.log2_T, _lib.stream())
            tv.launched = True
        elif sampler is None:
            _lib.call("nerf_composite_fwd", *cargs, _lib.stream())
        else:   # the coarse pass: the hierarchical sampler on these weights in the same launch
            _lib.call("nerf_composite_sample_fine", *cargs, *sampler, _lib.stream())
        ctx.save_for_backward(raw, z, rays_d, noise)
        ctx.white, ctx.defer = int(bool(white_bkgd)), defer
        outs = (rgb, disp, acc, weights, depth, ent)
        return outs + ((normal,) if normal is not None else ())

    @staticmethod
    def backward(ctx, *grads):
        raw, z, rays_d, noise = ctx.saved_tensors
        R, S, C = raw.shape
        names = ["g_rgb", "g_disp", "g_acc", "g_weights", "g_depth", "g_entropy", "g_normal"]
        gs = [None if g is None else g.contiguous().float() for g in grads] + [None] * (7 - len(grads))
        graw = torch.empty_like(raw)
        job = _lib.CompositeBwdJob(_lib.ptr(raw, "raw"), C, _lib.ptr(z, "z_vals"), _lib.ptr(rays_d, "rays_d"),
                                   _lib.ptr(noise, "noise", allow_none=True), R, S, ctx.white,
                                   *[_lib.ptr(g, n, allow_none=True) for g, n in zip(gs, names)],
                                   _lib.ptr(graw, "grad_raw"))
        task = torch._C._current_graph_task_id()
        if ctx.defer and _DEFER["on"] and task != -1 and task != _DEFER["off_task"]:
            # graw is read only by the field's (deferred) backward: launched with the pass's other
            # compositing backward as the pass's final callback (field._PendingField)
            from .field import _pending_field
            _pending_field(raw.device).add(CompositeJob(job, (raw, z, rays_d, noise, gs, graw)))
        else:
            _lib.call("nerf_composite_bwd_batch", (_lib.CompositeBwdJob * 1)(job), 1, _lib.stream())
        return graw, None, None, None, None, None, None


class CompositeJob:
    """A compositing backward awaiting its launch (nerf_composite_bwd_batch: the fine and the coarse
    pass's in one launch); `refs` keeps its inputs and output alive until then."""

    def __init__(self, job, refs):
        self.job, self.refs = job, refs
        self.stream = torch.cuda.current_stream()


def run_composite_jobs(jobs):
    if jobs:
        _lib.call("nerf_composite_bwd_batch", (_lib.CompositeBwdJob * len(jobs))(*[j.job for j in jobs]), len(jobs),
                  _lib.stream())


class MarchCompositeFn(torch.autograd.Function):
    """The packed compositing of a grid march under gradients (march_grad): raw [n, 4], z [n],
    dist [n], offsets int32 [R + 1], rays_d [R, 3] -> (rgb_map, depth_map, acc_map). The forward is
    nerf_march_composite, the launch of the forward-only march; the backward is nerf_packed_composite_bwd, launched
    at once. Gradients flow to raw only (z, dist and rays_d are not differentiated, as in CompositeFn)."""

    @staticmethod
    def forward(ctx, raw, z, dist, offsets, rays_d, white_bkgd):
        if z.requires_grad or dist.requires_grad or rays_d.requires_grad:
            raise NotImplementedError("march: gradients w.r.t. z_vals / dists / rays_d are not implemented")
        ctx.set_materialize_grads(False)
        raw = raw.contiguous()
        R, n = rays_d.shape[0], raw.shape[0]
        f = dict(device=raw.device, dtype=torch.float32)
        rgb, depth, acc = torch.empty(R, 3, **f), torch.empty(R, **f), torch.empty(R, **f)
        if R > 0:
            _lib.call("nerf_march_composite", _lib.ptr(raw, "raw"), _lib.ptr(z, "z_c"), _lib.ptr(dist, "dist_c"),
                      _lib.ptr(offsets, "offsets", torch.int32), _lib.ptr(rays_d, "rays_d"), R, n,
                      int(bool(white_bkgd)), _lib.ptr(rgb, "rgb"), None, _lib.ptr(acc, "acc"), _lib.ptr(depth, "depth"),
                      None, _lib.stream())
        ctx.save_for_backward(raw, z, dist, offsets, rays_d)
        ctx.white = int(bool(white_bkgd))
        return rgb, depth, acc

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_acc):
        raw, z, dist, offsets, rays_d = ctx.saved_tensors
        if g_rgb is None and g_depth is None and g_acc is None:
            return None, None, None, None, None, None
        gs = [None if g is None else g.contiguous().float() for g in (g_rgb, g_acc, g_depth)]
        graw = torch.empty_like(raw)   # a march's segments tile its list: every row is written
        _lib.call("nerf_packed_composite_bwd", _lib.ptr(raw, "raw"), _lib.ptr(z, "z_c"), _lib.ptr(dist, "dist_c"),
                  _lib.ptr(offsets, "offsets", torch.int32), _lib.ptr(rays_d, "rays_d"), rays_d.shape[0], raw.shape[0],
                  ctx.white, _lib.ptr(gs[0], "g_rgb", allow_none=True), None, _lib.ptr(gs[1], "g_acc", allow_none=True),
                  _lib.ptr(gs[2], "g_depth", allow_none=True), None, _lib.ptr(graw, "grad_raw"), _lib.stream())
        return graw, None, None, None, None, None


_DEFER = {"on": True, "off_task": None}


def set_batched_composite_bwd(enabled=True):
    """Defer the compositing backward of a field's raw output to the pass's final callback, where the
    fine and the coarse pass's run as one launch (on by default). Taken only for raw straight from the
    fused field without a normals head (the field's own backward is deferred too, so nothing else reads
    the raw gradient before the launch); a render_rays raw output that is itself differentiated
    (retraw) flushes the deferred launch first (_RawGuardFn)."""
    _DEFER["on"] = bool(enabled)


def batched_composite_bwd():
    return _DEFER["on"]


class _RawGuardFn(torch.autograd.Function):
    """render_rays' raw output (retraw) when the compositing backward of the same raw may be deferred:
    identity forward; a gradient through it (a loss on raw itself) launches any deferred compositing
    backward at once and turns deferral off for the rest of the pass, so autograd's sum of the two
    raw gradients reads a written buffer."""

    @staticmethod
    def forward(ctx, raw):
        return raw.view_as(raw)

    @staticmethod
    def backward(ctx, g):
        _DEFER["off_task"] = torch._C._current_graph_task_id()
        from .field import _pending_field
        _pending_field(g.device).flush_composites()
        return g


_FUSED_SAMPLER = {"on": True}
_SH_ROWS = {"on": True}


def set_sh_rows(enabled=True):
    """render_rays writes each ray's SH4 view encoding once (nerf_sample_stratified_sh) and the fused
    field's MLP kernels load it instead of evaluating SH per point (on by default; bit-identical)."""
    _SH_ROWS["on"] = bool(enabled)


def sh_rows():
    return _SH_ROWS["on"]


def set_fused_coarse_sampler(enabled=True):
    """render_rays' coarse compositing and hierarchical sampler in one launch (nerf_composite_sample_fine,
    on by default; bit-identical to nerf_composite_fwd + nerf_sample_fine_rows)."""
    _FUSED_SAMPLER["on"] = bool(enabled)


def fused_coarse_sampler():
    return _FUSED_SAMPLER["on"]


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, pytest=False, predict_normals=False,
                _sampler=None, _defer=False):
    """run_nerf.py:347-411 -> (rgb_map, disp_map, acc_map, weights, depth_map, sparsity_loss[, normal_map]).
    Internal (render_rays): _sampler = its nerf_sample_fine_rows arguments after d_weights' group;
    _defer = raw reaches nothing but this call and render_rays' guarded raw output."""
    R, S = raw.shape[0], raw.shape[1]
    noise = None
    if raw_noise_std > 0.:
        if pytest:
            noise = _pytest_uniforms((R, S), raw.device) * raw_noise_std
        else:
            # torch.randn(R, S) * raw_noise_std (run_nerf.py) in one launch: normal_'s transform z * std + 0
            # rounds like the product, from the same generator draws (tests/test_gpu_parity.py)
            noise = torch.empty(R, S, device=raw.device).normal_(0.0, raw_noise_std)
    if raw.shape[-1] not in (4, 7):
        raise ValueError(f"raw2outputs: raw must have 4 or 7 channels, got {raw.shape[-1]}")
    if not predict_normals and raw.shape[-1] == 7:
        raw = raw[..., :4]      # the reference reads channels 0..3 only
    defer = _defer and bool(getattr(raw, "_nerf_field_raw", False)) and raw.dtype == torch.float32
    outs = CompositeFn.apply(raw.float(), z_vals, rays_d, noise, white_bkgd, _sampler, defer)
    if predict_normals:
        if raw.shape[-1] == 4:
            # the reference slices raw[..., 4:7] of a 4-channel raw (the coarse net has no normals
            # head, run_nerf.py:240-247 vs :260-268): an empty [R, 0] normal map (run_nerf.py:361,407)
            return outs + (raw.new_zeros(R, 0),)
        return outs
    return outs[:6]


# ---------------------------------------------------------------- coarse-feature reuse

_REUSE = {"on": True}


def set_coarse_reuse(enabled=True):
    """the fine pass of render_rays encodes only its importance samples and takes
    the hash features of its coarse points from the coarse pass (on by default; off = re-encode all
    of them, as the reference does). Features are bit-identical either way."""
    _REUSE["on"] = bool(enabled)


def coarse_reuse():
    return _REUSE["on"]


def last_reuse_used():
    """Whether the last render_rays call's fine pass took the coarse features (bench.py's pricing)."""
    return _REUSE.get("last", False)


class CoarseReuse:
    """Hand-over of one render_rays call's coarse hash encoding to its fine pass.

    The reference merges the coarse depths into the fine ones (run_nerf.py:512-516: torch.sort of
    cat([z_vals, z_samples]), then rays_o + rays_d * z) and queries both networks through ONE
    embedder (run_nerf.py:225,275), so 64 of a ray's 192 fine points are the coarse points bit for
    bit and, the tables being unchanged inside an iteration, so are their 16-level features.
    render_rays attaches this object to the coarse and then the fine point tensors
    (`pts._nerf_reuse`); field.FieldFn (the fused run_network) encodes the coarse points into the tail
    rows of one feature buffer [L, R*(S+N), 2] laid out in importance-first order (importance sample k
    of ray r at row r*N + k, then coarse sample i at R*N + r*S + i), and the fine pass gathers only its
    importance samples, into the head rows: no copy, no scattered writes. The fine MLP walks that order
    (nerf_point_order: raw / geo / graw / dgeo stay in the merged order at rows inv, = the sampler's
    importance rows then its coarse rows), so its d feat is importance-first too: the fine bin reads
    the importance samples' rows contiguously and the coarse bin adds the coarse points' fine d feat
    (the tail rows) to their coarse d feat (nerf_hash_encode_bwd_bin_rows): each shared point is binned
    once. Any other network_query_fn ignores the attribute."""

    def __init__(self, R, S, N):
        self.R, self.S, self.N = R, S, N
        self.state = "armed"          # -> "recorded" (coarse FieldFn) -> "rows" (sample_fine) -> "used"
        self.feat = self.keep = self.pts = self.embedder = self.versions = None
        self.inv = self.imp_pts = None

    def alloc(self, n_levels, device, packed=False):
        """The shared feature / keep buffers; returns them and the coarse pass's first row. packed: the features as
        bf16 words [L, P] int32 (feature_precision="bf16")."""
        P = self.R * (self.S + self.N)
        self.feat = sparse_field.level_features(n_levels, P, device, packed)
        self.keep = torch.empty(P, device=device, dtype=torch.bool)
        return self.feat, self.keep, self.R * self.N

    def record(self, pts, embedder, tables):
        self.pts, self.embedder = pts, embedder
        self.versions = [t._version for t in tables]
        self.state = "recorded"

    def matches(self, embedder, tables, P):
        return (self.state == "rows" and embedder is self.embedder and P == self.R * (self.S + self.N)
                and [t._version for t in tables] == self.versions)

    @property
    def used(self):
        return self.state == "used"

    def release_forward(self):
        """After the fine forward: only the row maps and the coarse points stay (the backward's)."""
        self.feat = self.keep = self.embedder = None


# ---------------------------------------------------------------- sampling

def sample_pdf(bins, weights, N_samples, det=False, pytest=False):
    """run_nerf_helpers.py:354-397 (no gradient: the reference detaches its samples)."""
    bins = bins.detach().contiguous().float()
    weights = weights.detach().contiguous().float()
    R, nb = bins.shape
    if weights.shape != (R, nb - 1):
        raise ValueError(f"sample_pdf: weights {tuple(weights.shape)} must be [R, n_bins - 1] = [{R}, {nb - 1}]")
    out = torch.empty(R, N_samples, device=bins.device, dtype=torch.float32)
    t_imp = _linspace(N_samples, bins.device) if det else None
    u = _pytest_uniforms((R, N_samples), bins.device) if (pytest and not det) else None
    seed, off, rng = _rng()
    _lib.call("nerf_sample_pdf", _lib.ptr(bins, "bins"), nb, _lib.ptr(weights, "weights"), nb - 1, R, nb, N_samples,
              int(det), _lib.ptr(t_imp, "t", allow_none=True), _lib.ptr(u, "u", allow_none=True), seed, off, rng,
              _lib.ptr(out, "samples"), _lib.stream())
    return out


def _query(network_query_fn, pts, viewdirs, fn, req=None):
    """The field call of one pass -> (raw, stops). req: its sparse_field.FieldRequest, which rides on the points as
    `pts._nerf_req` for the length of the call (the only place that attaches one), or None: the plain
    call, nothing attached. stops: int32 [R] with early ray termination (early_stop.py), None otherwise."""
    if req is None:
        return network_query_fn(pts, viewdirs, fn), None
    pts._nerf_req = req
    try:
        raw = network_query_fn(pts, viewdirs, fn)
    finally:
        del pts._nerf_req
    if not req.used:   # a foreign query function ignores the attribute: never fall back to another path silently
        raise ValueError(f"render_rays: {req.blame} needs a network_query_fn that calls this package's run_network")
    return raw, req.stop


def last_early_stop_counts():
    """(points evaluated, points total) of the most recent field call with early_stop, summed over its
    slabs (the analogue of OccupancyGrid.last_counts())."""
    from .early_stop import last_counts
    return last_counts()


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, embed_fn=None, retraw=False, lindisp=False,
                perturb=0., N_importance=0, network_fine=None, white_bkgd=False, raw_noise_std=0., verbose=False,
                pytest=False, predict_normals=False, occupancy=None, early_stop=None, early_stop_slab=32,
                march=None, march_samples=512, march_points=1 << 21, mlp_precision=None,
                table_precision=None, march_stop=None, march_stop_slab=128, feature_precision=None, march_sh=None,
                march_sizes=None, march_grad=False, march_jitter=False):
    """run_nerf.py:414-549. occupancy (an occupancy.OccupancyGrid; forward-only rendering):
    the field runs only at the samples inside the box and in an occupied cell, every other sample gets an
    all-zero raw row (weight 0). None (the default) is the dense path.
    early_stop (a transmittance threshold 0 < eps < 1; forward-only rendering): each pass
    runs front to back in slabs of early_stop_slab samples and a ray whose optical depth has passed
    -log(eps) gets all-zero raw rows in every later slab; the result then also holds early_stop_samples
    (int32 [R], the leading samples of the final pass for which the ray was alive) and, with
    N_importance > 0, early_stop_samples0 (the coarse pass). Composes with occupancy. None (the default)
    leaves the call as it is without it.
    march (an occupancy.OccupancyGrid; forward-only rendering): one pass over march_samples
    (1..4096) samples per ray at the coarse sampler's unperturbed depths, through network_fine (network_fn
    without one), of which only those inside the box and in an occupied cell are ever formed: a packed list
    per ray, the field on the list (in slices of at most march_points points) and the compositing of the
    list. The result is what masking sigma by grid.query in that dense render gives: rgb_map, depth_map,
    acc_map, march_samples (int32 [R], the kept samples per ray) and rays_d; with retraw also the packed
    raw [n, 4], pts [n, 3], z_vals [n] and march_offsets (int32 [R + 1]). N_samples and N_importance are not
    used. None (the default) leaves the call as it is without it.
    mlp_precision (None, "fp32" or "bf16"; forward-only rendering): "bf16" runs every MLP forward
    of the call with one bf16 piece per operand and fp32 sums (nerf_mlp_fwd_bf16) instead of the fp32-accurate
    kernel: weights, hash features, SH and hidden activations are rounded to bf16, sigma and the colour layer's
    sums stay fp32. Composes with occupancy=, early_stop= and march=. None and "fp32" are the call without it.
    table_precision (None, "fp32" or "fp16"; forward-only rendering): "fp16" makes every hash-encoding
    launch of the call gather from an fp16 image of the tables (HashEmbedder.half_tables, nerf_hash_encode_fwd_half):
    each table value rounded once to binary16, everything else unchanged, so the result is bit for bit the default
    render of a model whose tables are t.half().float(). Composes with occupancy=, early_stop=, march= and
    mlp_precision=. None and "fp32" are the call without it.
    march_stop (a float transmittance threshold 0 < eps < 1; with march=): the march runs front to back
    in slabs of march_stop_slab lattice samples, and a ray whose optical depth over the samples evaluated so far has
    passed -log(eps) after a slab is not walked in any later slab. The result is the march with sigma masked by
    k < march_stop_samples[r] (int32 [R]: the slab boundary at which the ray stopped, march_samples if it never
    did); march_samples then counts the samples actually evaluated. Each map differs from the unstopped march's by
    at most eps. With retraw the packed entries come per slab: march_slabs, a list of (offsets, raw, pts, z_vals).
    Composes with mlp_precision=, table_precision= and render's ray_bounds=. None (the default) is the march
    without it: no other launch, no other buffer.
    feature_precision (None, "fp32" or "bf16"; with mlp_precision="bf16"): "bf16" makes every
    hash-encoding launch of the call write one word {bf16 f0, bf16 f1} per (point, level) instead of two floats
    (nerf_hash_encode_fwd_pkbf, with fp16 tables nerf_hash_encode_fwd_half_pkbf) and every MLP forward launch read
    those words (nerf_mlp_fwd_bf16_pkbf): the rounding the bf16 MLP does first, done by the encoder, so the result is
    bit for bit the mlp_precision="bf16" render at half the feature bytes. Composes with occupancy=, early_stop=,
    march=, march_stop=, table_precision= and render's ray_bounds=. None and "fp32" are the call without it.
    march_sh (None, "rows" or "rays"; with march=): "rays" makes the march's list carry each point's ray
    index (4 B) instead of its SH4 row (64 B); one SH record per ray is formed once per chunk (nerf_ray_sh_records) and
    the MLP reads it through the index (the _rays entry of the call's precision). The result is bit for bit the march
    without it, in every entry. Composes with march_stop=, mlp_precision=, table_precision=, feature_precision= and
    render's ray_bounds=. None and "rows" are the call without it: the same launches, the same buffers.
    march_sizes (None, "host" or "device"; with march=, march_sh="rays", mlp_precision="bf16" and
    feature_precision="bf16"): "device" keeps the length of every packed list in device memory. The
    lists are allocated at their capacity (40 B per lattice sample of the chunk, or of the slab with march_stop), the
    encoder and the MLP read the count themselves (the _dev entries) over ceil(capacity / march_points) slices, and
    every slab of a chunk is written, evaluated, composited and advanced back to back: the host reads nothing and no
    launch depends on a count. The result is bit for bit the call without it, in every entry. With retraw the packed
    entries are views of the first n rows, which costs one read after the chunk's last launch. Composes with
    march_stop=, table_precision=, march_points= and render's ray_bounds=. None and "host" are the call without it:
    the same launches, the same buffers.
    march_grad (a bool; with march=): True lets the plain march run under gradients, for training
    through the grid. The field on the list is then field.PackedFieldFn (per slice of march_points points) and the
    compositing MarchCompositeFn, whose backward is nerf_packed_composite_bwd; the result holds the same entries,
    rgb_map, depth_map and acc_map bit for bit those of the call under torch.no_grad(), and with retraw the packed raw
    is attached to the graph. Under torch.no_grad() the call is the march without it: the same launches, the same
    bits. Does not combine with march_stop= (the slabs' carried state has no backward); march_sh="rays",
    mlp_precision="bf16", table_precision="fp16", feature_precision="bf16" and march_sizes="device" stay forward-only.
    False (the default) leaves every call as it is: march= under gradients is refused.
    march_jitter (a bool; with march=): True lets the march take perturb > 0: lattice sample k of a ray
    then lies at the depth the dense coarse sampler gives it with perturb (uniform in its stratum, bit for bit; with
    pytest the reference's np.random.seed(0) uniforms, else an in-kernel Philox draw that render.manual_seed makes
    repeatable, one seed per chunk), and the packed dists are those of the jittered depths. With perturb == 0 the call
    is the plain march: the same launches, the same bits, so one dict serves training and evaluation. Composes with
    march_grad under gradients, and with march_sh, mlp_precision, table_precision, feature_precision and march_points
    under torch.no_grad(). Does not combine with march_stop=, march_sizes="device" or render's ray_bounds=. False
    (the default) leaves every call as it is: march= with perturb > 0 is refused."""
    # march_sizes is passed only when given: tests/test_field_request.py pins this call's eight positional arguments
    # and empty keywords for a call without it (the same in render())
    opts = sparse_field.field_options("render_rays", march, march_sh, march_stop, march_stop_slab, mlp_precision,
                                      table_precision, feature_precision,
                                      **({} if march_sizes is None else dict(march_sizes=march_sizes)))
    march_grad = sparse_field.check_march_grad(march_grad, march, opts.stop, "render_rays")
    march_jitter = sparse_field.check_march_jitter(march_jitter, march, opts.stop, march_sizes, "render_rays")
    nets = [network_fn] + ([] if network_fine is None else [network_fine])
    if opts.half:
        sparse_field.check_table_nets(nets, embed_fn)
    if opts.bf16:
        sparse_field.check_mlp_nets(nets, embed_fn, predict_normals)
    if march is not None:
        return _render_rays_march(ray_batch, network_fn, network_query_fn, march, march_samples, march_points, opts,
                                  embed_fn=embed_fn, retraw=retraw, lindisp=lindisp, perturb=perturb,
                                  network_fine=network_fine, white_bkgd=white_bkgd, raw_noise_std=raw_noise_std,
                                  predict_normals=predict_normals, occupancy=occupancy, early_stop=early_stop,
                                  device_sizes=sparse_field.device_sized(march_sizes), march_grad=march_grad,
                                  march_jitter=march_jitter, pytest=pytest)
    early = None
    if early_stop is not None:
        from .early_stop import check_params
        early = check_params(early_stop, early_stop_slab)
    if early is not None or occupancy is not None:
        sparse_field.check_forward_only("occupancy" if early is None else "early_stop", "render_rays", raw_noise_std)
    rays = ray_batch.detach().float().contiguous()
    R, C = rays.shape
    dev = rays.device
    f = dict(device=dev, dtype=torch.float32)
    # contiguous copies of the directions (compositing) and view directions (field), written by the
    # sampler launch instead of two slicing copies
    viewdirs = torch.empty(R, 3, **f) if C > 8 else None
    rays_d = torch.empty(R, 3, **f)

    z = torch.empty(R, N_samples, **f)
    pts = torch.empty(R, N_samples, 3, **f)
    u = _pytest_uniforms((R, N_samples), dev) if (perturb > 0. and pytest) else None
    seed, off, rng = (0, 0, None) if (u is not None or not perturb > 0.) else _rng()
    # the view directions' SH4 rows, once per ray (the fused field reads them instead of evaluating
    # SH per point, field.FieldFn): attached to the viewdirs tensor the field receives
    # [R, 40]: 16 fp32 coefficients + their three bf16 pieces (the MLP's pre-split C0 operand)
    sh_rays = torch.empty(R, 40, **f) if (viewdirs is not None and _SH_ROWS["on"]) else None
    _lib.call("nerf_sample_stratified_sh", _lib.ptr(rays, "ray_batch"), C, R, N_samples,
              _lib.ptr(_linspace(N_samples, dev)), int(bool(lindisp)), int(perturb > 0.), _lib.ptr(u, "u", allow_none=True),
              seed, off, rng, _lib.ptr(z, "z"), _lib.ptr(pts, "pts"), _lib.ptr(rays_d, "rays_d"),
              _lib.ptr(viewdirs, "viewdirs", allow_none=True), _lib.ptr(sh_rays, "sh_rows", allow_none=True),
              _lib.stream())
    if sh_rays is not None:
        viewdirs._nerf_sh = sh_rays

    # coarse-feature reuse is off with an occupancy grid or early termination (each pass encodes its own kept points)
    reuse = (CoarseReuse(R, N_samples, N_importance)
             if (N_importance > 0 and _REUSE["on"] and R > 0 and occupancy is None and early is None) else None)
    if reuse is not None:
        pts._nerf_reuse = reuse       # the fused run_network records the coarse encoding in it
    raw, stops = _query(network_query_fn, pts, viewdirs, network_fn,
                        opts.request(occupancy, None if early is None else (z, rays_d) + early))
    if reuse is not None:
        del pts._nerf_reuse
        if reuse.state != "recorded" or R * (N_samples + N_importance) > 2 ** 31 - 1:
            reuse = None
    ret = {}
    if N_importance > 0:
        det = perturb == 0.
        M = N_samples + N_importance
        z_fine = torch.empty(R, M, **f)
        pts_fine = torch.empty(R, M, 3, **f)
        z_std = torch.empty(R, **f)
        t_imp = _linspace(N_importance, dev) if det else None
        u_imp = _pytest_uniforms((R, N_importance), dev) if (pytest and not det) else None
        seed, off, rng = (0, 0, None) if (det or u_imp is not None) else _rng()
        i32 = dict(device=dev, dtype=torch.int32)
        if reuse is not None:
            # inv = [importance rows | coarse rows]: the merged row of each importance-first position
            reuse.inv, reuse.imp_pts = torch.empty(R * M, **i32), torch.empty(R, N_importance, 3, **f)
            reuse.state = "rows"
        inv = None if reuse is None else reuse.inv
        # nerf_sample_fine_rows' arguments after (d_z, d_weights, n_rays, n_samples)
        samp = (N_importance, int(det), _lib.ptr(t_imp, "t", allow_none=True), _lib.ptr(u_imp, "u", allow_none=True),
                seed, off, rng, _lib.ptr(z_fine, "z_fine"), _lib.ptr(pts_fine, "pts_fine"), _lib.ptr(z_std, "z_std"),
                None, None if inv is None else _lib.ptr_at(inv, R * N_importance, "coarse_rows", torch.int32),
                _lib.ptr(inv, "imp_rows", torch.int32, True),
                _lib.ptr(None if reuse is None else reuse.imp_pts, "imp_pts", allow_none=True), None)
        fused = _FUSED_SAMPLER["on"]
        outs = raw2outputs(raw, z, rays_d, raw_noise_std, white_bkgd, pytest=pytest, predict_normals=predict_normals,
                           _sampler=(_lib.ptr(rays, "ray_batch"), C) + samp if fused else None, _defer=True)
        weights = outs[3]
        if not fused:
            _lib.call("nerf_sample_fine_rows", _lib.ptr(rays, "ray_batch"), C, _lib.ptr(z, "z"),
                      _lib.ptr(weights.detach().contiguous(), "weights"), R, N_samples, *samp, _lib.stream())
        rgb_map_0, _, acc_map_0, _, depth_map_0, sparsity_loss_0 = outs[:6]
        normal_map_0 = outs[6] if predict_normals else None
        z, pts = z_fine, pts_fine
        run_fn = network_fn if network_fine is None else network_fine
        if reuse is not None:
            pts._nerf_reuse = reuse
        stops0 = stops
        raw, stops = _query(network_query_fn, pts, viewdirs, run_fn,
                            opts.request(occupancy, None if early is None else (z, rays_d) + early))
        if reuse is not None:
            del pts._nerf_reuse
            reuse.release_forward()
        _REUSE["last"] = reuse is not None and reuse.used
        outs = raw2outputs(raw, z, rays_d, raw_noise_std, white_bkgd, pytest=pytest, predict_normals=predict_normals,
                           _defer=True)
        rgb_map, disp_map, acc_map, weights, depth_map, sparsity_loss = outs[:6]
        normal_map = outs[6] if predict_normals else None
        ret.update(rgb0=rgb_map_0, depth0=depth_map_0, acc0=acc_map_0, sparsity_loss0=sparsity_loss_0, z_std=z_std)
        if early is not None:
            ret["early_stop_samples0"] = stops0
        if predict_normals:
            ret["normal0"] = normal_map_0
    else:
        outs = raw2outputs(raw, z, rays_d, raw_noise_std, white_bkgd, pytest=pytest, predict_normals=predict_normals,
                           _defer=True)
        rgb_map, disp_map, acc_map, weights, depth_map, sparsity_loss = outs[:6]
        normal_map = outs[6] if predict_normals else None

    # the entries of ret, their shapes and dtypes are restated for zero rays in _no_rays_result (render's
    # ray_bounds path, when no ray of a frame is hit): keep the two in step
    ret.update(rgb_map=rgb_map, depth_map=depth_map, acc_map=acc_map, sparsity_loss=sparsity_loss, pts=pts,
               rays_d=rays_d)
    if predict_normals:
        ret["normal_map"] = normal_map
    if early is not None:
        ret["early_stop_samples"] = stops
    if retraw:
        ret["raw"] = _RawGuardFn.apply(raw) if getattr(raw, "_nerf_field_raw", False) else raw
    if DEBUG:
        check_numerics(ret)
    return ret


def _check_march(grid, march_samples, march_points, fn, embed_fn, lindisp, perturb, raw_noise_std, predict_normals,
                 occupancy, early_stop, march_grad=False, march_jitter=False):
    """render_rays' refusals with march= after field_options', all before any launch -> K. march_grad: the call may
    run under gradients. march_jitter: the call may carry perturb > 0."""
    from .occupancy import OccupancyGrid, _check_modules, check_march_samples
    from .sparse_field import check_forward_only, check_march_points
    if not isinstance(grid, OccupancyGrid):
        raise ValueError(f"render_rays: march must be an OccupancyGrid, got {type(grid).__name__}")
    K = check_march_samples(march_samples, "render_rays: march")
    check_march_points(march_points)
    if occupancy is not None or early_stop is not None:
        raise ValueError("render_rays: march does not combine with occupancy= (the march already masks by its grid) "
                         "or early_stop= (rays are not stopped inside a march)")
    check_forward_only("march", "render_rays", raw_noise_std, grad=march_grad)
    if perturb > 0. and not march_jitter:
        raise ValueError("render_rays: march needs perturb == 0 (the lattice is the unperturbed coarse sampling)")
    if lindisp:
        raise ValueError("render_rays: march needs lindisp=False (the lattice is linear in depth)")
    if predict_normals or getattr(fn, "raw_channels", 4) != 4:
        raise ValueError("render_rays: march does not support predict_normals or a normals head")
    if embed_fn is not None:
        _check_modules(embed_fn, fn, "render_rays: march")
    return K


def _render_rays_march(ray_batch, network_fn, network_query_fn, grid, march_samples, march_points, opts, embed_fn=None,
                       retraw=False, lindisp=False, perturb=0., network_fine=None, white_bkgd=False, raw_noise_std=0.,
                       predict_normals=False, occupancy=None, early_stop=None, device_sizes=False, march_grad=False,
                       march_jitter=False, pytest=False):
    """render_rays with march=: count and write the packed list (csrc/march.hip), the field on
    the list (sparse_field.run_network_packed), the packed compositing. opts: the call's FieldOptions. With
    opts.stop (march_stop) the same in slabs (_march_slabs). opts.by_ray (march_sh="rays", DESIGN.md
    §21): the write leaves a ray index in place of the SH rows, and the field reads the SH records of the chunk's
    packed rays through it. device_sizes (march_sizes="device"): the list's length stays on the device;
    the list is allocated at its capacity R K, the composite is given that capacity as its list bound (it clamps a
    segment into the list, and every offset is at most the true length, which is at most the capacity) and the field
    runs whenever the capacity is not 0. march_grad under gradients: the field call's list allows
    gradients (field.PackedFieldFn), the compositing is MarchCompositeFn, and both run for an empty list too, so that
    the maps stay attached to the graph. march_jitter with perturb > 0: the count and the write are the
    nerf_jitter_ entries with the dense coarse pass's uniforms (pytest: _pytest_uniforms((R, K)); else one _rng() draw
    per chunk); everything after the write takes the jittered list unchanged."""
    run_fn = network_fn if network_fine is None else network_fine
    K = _check_march(grid, march_samples, march_points, run_fn, embed_fn, lindisp, perturb, raw_noise_std,
                     predict_normals, occupancy, early_stop, march_grad, march_jitter)
    train = march_grad and torch.is_grad_enabled()   # march_sh="rays" and march_sizes="device" have refused gradients
    if not torch.is_tensor(ray_batch) or ray_batch.dim() != 2 or ray_batch.shape[1] != 11:
        raise ValueError("render_rays: march needs ray rows with view directions ([R, 11]: use_viewdirs=True)")
    by_ray = opts.by_ray
    records = []   # by_ray: the SH records of the chunk's packed rays, formed before its first field call

    def field(rays, pts_c, sh_c, total=None):
        """The field on a packed list of n > 0 points (by_ray: sh_c is the points' ray index into `rays`, the same
        packed rows in every slab of a chunk). total (device_sizes): the list's length, int32 [1] on the device; the
        buffers then hold the list's capacity."""
        if by_ray:
            if not records:
                records.append(grid._ray_sh_records(rays))
            march = sparse_field.MarchList(None, march_points, ray_c=sh_c, sh_rec=records[0], total=total,
                                           capacity=None if total is None else pts_c.shape[0])
        else:
            march = sparse_field.MarchList(sh_c, march_points, grad=train)
        return _query(network_query_fn, pts_c, rays[:, 8:11], run_fn, opts.request(march=march))[0]

    if opts.stop is not None:
        ret = _march_slabs(ray_batch, grid, K, opts, field, white_bkgd, retraw, device_sizes)
        if DEBUG:
            check_numerics(ret)
        return ret
    jitter = None
    if march_jitter and perturb > 0.:   # the dense coarse pass's uniforms: the same draws in the same order
        u = _pytest_uniforms((ray_batch.shape[0], K), ray_batch.device) if pytest else None
        jitter = (u,) + ((0, 0, None) if u is not None else _rng())
    rays, t, counts, offsets, rays_d, n = grid._march_count(ray_batch, K, sized="device" if device_sizes else "host",
                                                            jitter=jitter)
    R, dev = rays.shape[0], rays.device
    pts_c, z_c, dist_c, sh_c = grid._march_write(rays, t, K, counts, offsets, n, True, index=by_ray, jitter=jitter)
    f = dict(device=dev, dtype=torch.float32)
    if device_sizes:
        grid._last = ([n], R * K)        # the count as device elements, one per list: last_counts() reads them when asked
        total, n = n, pts_c.shape[0]     # from here on n is the capacity: the bound every launch is given
        raw = field(rays, pts_c, sh_c, total) if n > 0 else torch.empty(0, 4, **f)
    else:
        grid._last = (n, R * K)
        raw = field(rays, pts_c, sh_c) if n > 0 else torch.empty(0, 4, **f)
    if train:
        if n == 0:
            raw = field(rays, pts_c, sh_c)
        rgb_map, depth_map, acc_map = MarchCompositeFn.apply(raw, z_c, dist_c, offsets, rays_d, white_bkgd)
    else:
        rgb_map, depth_map, acc_map = torch.empty(R, 3, **f), torch.empty(R, **f), torch.empty(R, **f)
    if R > 0 and not train:
        _lib.call("nerf_march_composite", _lib.ptr(raw, "raw"), _lib.ptr(z_c, "z_c"), _lib.ptr(dist_c, "dist_c"),
                  _lib.ptr(offsets, "offsets", torch.int32), _lib.ptr(rays_d, "rays_d"), R, n, int(bool(white_bkgd)),
                  _lib.ptr(rgb_map, "rgb"), None, _lib.ptr(acc_map, "acc"), _lib.ptr(depth_map, "depth"), None,
                  _lib.stream())
    # restated for zero rays in _no_rays_result: keep the two in step
    ret = dict(rgb_map=rgb_map, depth_map=depth_map, acc_map=acc_map, march_samples=counts, rays_d=rays_d)
    if retraw:
        if device_sizes:    # the one read of the chunk, after its last launch: the packed entries as views [:n]
            n = int(total.item())
            raw, pts_c, z_c = raw[:n], pts_c[:n], z_c[:n]
        ret.update(raw=raw, pts=pts_c, z_vals=z_c, march_offsets=offsets)
    if DEBUG:
        check_numerics(ret)
    return ret


def _march_slabs(ray_batch, grid, K, opts, field, white_bkgd, retraw, device_sizes=False):
    """The march of _render_rays_march with march_stop, opts.stop = (eps, slab): the lattice front to
    back in slabs; per slab the packed list of the rays alive (one 4-byte host read sizes it), field(rays, pts_c,
    sh_c) on it, its compositing into the per-ray state and, unless it is the last, the stopping rule. A slab with
    an empty list skips the field and its launches (the last slab's compositing always runs: it writes the maps).
    opts.by_ray: every slab's write leaves the ray index in place of the SH rows.
    device_sizes (march_sizes="device"): no read; every slab's list is allocated at its capacity
    R (k1 - k0), and every slab is evaluated, composited (first = slab 0) and, unless it is the last, advanced, an
    empty one too: an empty segment leaves a ray's state, tau, alive and stop as they are, so the bits are those of
    the loop that skips."""
    from .early_stop import tau_max_of
    (eps, Ks), by_ray = opts.stop, opts.by_ray
    tau_max = tau_max_of(eps)
    rays = tau = alive = stops = state = rays_d = None
    rgb_map = depth_map = acc_map = None
    slabs, counts_all, evaluated, first, totals = [], [], 0, True, []
    for k0 in range(0, K, Ks):
        k1 = min(k0 + Ks, K)
        rays, t, counts, offsets, dirs, n = grid._march_count(ray_batch if rays is None else rays, K, k0, k1, alive,
                                                              dirs=rays_d is None,
                                                              sized="device" if device_sizes else "host")
        R, dev = rays.shape[0], rays.device
        f = dict(device=dev, dtype=torch.float32)
        if rays_d is None:      # slab 0: the state every later slab carries
            rays_d = dirs
            rgb_map, depth_map, acc_map = torch.empty(R, 3, **f), torch.empty(R, **f), torch.empty(R, **f)
            if k1 < K:
                tau, alive = torch.zeros(R, **f), torch.ones(R, device=dev, dtype=torch.uint8)
                state = torch.empty(R, 6, device=dev, dtype=torch.float64)
            stops = torch.full((R,), K, device=dev, dtype=torch.int32)
        pts_c, z_c, dist_c, sh_c = grid._march_write(rays, t, K, counts, offsets, n, True, k0, k1, index=by_ray)
        if device_sizes:
            totals.append(n)
            total, n = n, pts_c.shape[0]     # from here on n is the capacity: the bound every launch is given
            raw = field(rays, pts_c, sh_c, total) if n > 0 else torch.empty(0, 4, **f)
            first = k0 == 0
        else:
            raw = field(rays, pts_c, sh_c) if n > 0 else torch.empty(0, 4, **f)
            evaluated += n
        counts_all.append(counts)
        if retraw:
            slabs.append((offsets, raw, pts_c, z_c))
        last = k1 == K
        if R > 0 and (n > 0 or last):
            if state is None:   # one slab: no state to carry
                state = torch.empty(R, 6, device=dev, dtype=torch.float64)
            _lib.call("nerf_slab_march_composite", _lib.ptr(raw, "raw"), _lib.ptr(z_c, "z_c"), _lib.ptr(dist_c, "dist_c"),
                      _lib.ptr(offsets, "offsets", torch.int32), _lib.ptr(rays_d, "rays_d"), R, n,
                      int(bool(white_bkgd)), _lib.ptr(state, "state", torch.float64), int(first), int(last),
                      _lib.ptr(rgb_map, "rgb"), None, _lib.ptr(acc_map, "acc"), _lib.ptr(depth_map, "depth"), None,
                      _lib.stream())
            first = False
        if R > 0 and n > 0 and not last:
            _lib.call("nerf_slab_march_advance", _lib.ptr(raw, "raw"), _lib.ptr(dist_c, "dist_c"),
                      _lib.ptr(offsets, "offsets", torch.int32), _lib.ptr(rays_d, "rays_d"), R, n, k1, tau_max,
                      _lib.ptr(tau, "tau"), _lib.ptr(alive, "alive", torch.uint8), _lib.ptr(stops, "stop", torch.int32),
                      _lib.stream())
    # host-sized: the evaluated count, an int; device-sized: one device element per slab (views into the slabs' offsets,
    # which they keep alive until the next march through this grid or until last_counts() resolves them)
    grid._last = (totals if device_sizes else evaluated, rays.shape[0] * K)
    if device_sizes and retraw:     # the one read of the chunk, after its last launch: the packed entries as views [:n]
        ns = torch.cat(totals).tolist()
        slabs = [(o, raw[:m], p[:m], z[:m]) for (o, raw, p, z), m in zip(slabs, ns)]
    total = counts_all[0] if len(counts_all) == 1 else torch.stack(counts_all).sum(0, dtype=torch.int32)
    # restated for zero rays in _no_rays_result: keep the two in step
    ret = dict(rgb_map=rgb_map, depth_map=depth_map, acc_map=acc_map, march_samples=total, rays_d=rays_d,
               march_stop_samples=stops)
    if retraw:
        ret["march_slabs"] = slabs
    return ret


def batchify_rays(rays_flat, chunk=1024 * 32, **kwargs):
    """run_nerf.py:71-83."""
    all_ret = {}
    for i in range(0, rays_flat.shape[0], chunk):
        ret = render_rays(rays_flat[i:i + chunk], **kwargs)
        for k in ret:
            all_ret.setdefault(k, []).append(ret[k])
    return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in all_ret.items()}


def camera(K, c2w):
    """nerf_camera of a float64 (or float32) K and a [3,4] pose: the float32 values get_rays'
    tensor ops see (run_nerf_helpers.py:311-320)."""
    cam = _lib.Camera()
    pose = torch.as_tensor(c2w, dtype=torch.float32).detach().cpu().reshape(-1, 4)[:3]
    for k, v in enumerate(pose.reshape(-1).tolist()):
        cam.c2w[k] = v
    Kf = [[float(np.float32(float(K[r][c]))) for c in range(3)] for r in range(2)]
    cam.fx, cam.fy, cam.cx, cam.cy = Kf[0][0], Kf[1][1], Kf[0][2], Kf[1][2]
    return cam


def get_rays(H, W, K, c2w, device=None):
    """run_nerf_helpers.py:311-320 -> rays_o, rays_d [H, W, 3] on the device (csrc/rays.hip,
    one launch; the pose is read on the host)."""
    device = torch.device(device) if device is not None else (c2w.device if torch.is_tensor(c2w) else
                                                               torch.device("cuda"))
    H, W = int(H), int(W)
    rays_o = torch.empty(H, W, 3, device=device, dtype=torch.float32)
    rays_d = torch.empty(H, W, 3, device=device, dtype=torch.float32)
    _lib.call("nerf_sample_rays", camera(K, c2w), H, W, 0, 0, H, W, H * W, 0, 0, 0, None, 0,
              _lib.ptr(rays_o, "rays_o"), _lib.ptr(rays_d, "rays_d"), None, None, _lib.stream())
    return rays_o, rays_d


def get_rays_np(H, W, K, c2w):
    """run_nerf_helpers.py:323-330."""
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    dirs = np.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -np.ones_like(i)], -1)
    rays_d = np.sum(dirs[..., np.newaxis, :] * c2w[:3, :3], -1)
    rays_o = np.broadcast_to(c2w[:3, -1], np.shape(rays_d))
    return rays_o, rays_d


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """run_nerf_helpers.py:333-350."""
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    rays_o = rays_o + t[..., None] * rays_d
    o0 = -1. / (W / (2. * focal)) * rays_o[..., 0] / rays_o[..., 2]
    o1 = -1. / (H / (2. * focal)) * rays_o[..., 1] / rays_o[..., 2]
    o2 = 1. + 2. * near / rays_o[..., 2]
    d0 = -1. / (W / (2. * focal)) * (rays_d[..., 0] / rays_d[..., 2] - rays_o[..., 0] / rays_o[..., 2])
    d1 = -1. / (H / (2. * focal)) * (rays_d[..., 1] / rays_d[..., 2] - rays_o[..., 1] / rays_o[..., 2])
    d2 = -2. * near / rays_o[..., 2]
    return torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)


def _pack_rays(H, W, K, rays_o, rays_d, near, far, ndc, use_viewdirs):
    """render()'s prologue (run_nerf.py:115-140) in one launch (csrc/rays.hip nerf_rays_pack):
    viewdirs = d/|d|, ndc_rays (near plane 1), [o, d, near, far, viewdir] per ray."""
    o = torch.reshape(rays_o, [-1, 3]).float().contiguous()
    d = torch.reshape(rays_d, [-1, 3]).float().contiguous()
    n = d.shape[0]
    out = torch.empty(n, 11 if use_viewdirs else 8, device=d.device, dtype=torch.float32)
    cw = ch = 0.0
    if ndc:
        focal = K[0][0]
        # -1./(W/(2.*focal)) is a python double in the reference; torch rounds it to float32
        cw = float(np.float32(-1. / (W / (2. * float(focal)))))
        ch = float(np.float32(-1. / (H / (2. * float(focal)))))
    zeros, nz, keep = _lib.take_zero_fills(d.device)   # a training step's zero fills ride along (_lib.defer_fill_zero)
    _lib.call("nerf_rays_pack_z", _lib.ptr(o, "rays_o"), _lib.ptr(d, "rays_d"), n, float(near), float(far),
              int(bool(ndc)), cw, ch, int(bool(use_viewdirs)), _lib.ptr(out, "rays"), zeros, nz, _lib.stream())
    del keep
    return out


def _missed_value(key, white_bkgd):
    """What a ray that crosses no occupied cell gets in entry `key` of render_rays' result: compositing's
    value for an all-zero raw wherever that does not depend on sample positions, else 0."""
    if key in ("rgb_map", "rgb0"):
        return 1.0 if white_bkgd else 0.0
    if key in ("depth_map", "depth0"):
        return float("nan")         # sum(w z) / sum(w) with sum(w) == 0 (composite_common.h)
    return 0


def _no_rays_result(device, N_samples, N_importance=0, retraw=False, predict_normals=False, early_stop=None,
                    network_fn=None, network_fine=None, march=None, march_stop=None, **_):
    """render_rays' result for zero rays, without a field call (every ray of the frame missed)."""
    f = dict(device=device, dtype=torch.float32)
    if march is not None:   # _render_rays_march's entries (render() refuses retraw with march)
        ret = dict(rgb_map=torch.empty(0, 3, **f), depth_map=torch.empty(0, **f), acc_map=torch.empty(0, **f),
                   march_samples=torch.empty(0, device=device, dtype=torch.int32), rays_d=torch.empty(0, 3, **f))
        if march_stop is not None:
            ret["march_stop_samples"] = torch.empty(0, device=device, dtype=torch.int32)
        return ret
    M = N_samples + N_importance
    fine = network_fn if network_fine is None else network_fine
    ret = {}
    for sfx, on in (("0", N_importance > 0), ("", True)):
        if not on:
            continue
        names = ("rgb0", "depth0", "acc0", "sparsity_loss0") if sfx else ("rgb_map", "depth_map", "acc_map",
                                                                          "sparsity_loss")
        for k in names:
            ret[k] = torch.empty((0, 3) if k.startswith("rgb") else (0,), **f)
        if early_stop is not None:
            ret["early_stop_samples" + sfx] = torch.empty(0, device=device, dtype=torch.int32)
        if predict_normals:
            net = network_fn if sfx else fine
            ret["normal0" if sfx else "normal_map"] = torch.empty(0, 3 if getattr(net, "raw_channels", 4) == 7 else 0, **f)
    if N_importance > 0:
        ret["z_std"] = torch.empty(0, **f)
    ret.update(pts=torch.empty(0, M, 3, **f), rays_d=torch.empty(0, 3, **f))
    if retraw:
        ret["raw"] = torch.empty(0, M, getattr(fine, "raw_channels", 4), **f)
    return ret


def _check_ray_bounds(grid):
    from .occupancy import OccupancyGrid
    from .sparse_field import check_forward_only
    if not isinstance(grid, OccupancyGrid):
        raise ValueError(f"render: ray_bounds must be an OccupancyGrid, got {type(grid).__name__}")
    check_forward_only("ray_bounds", "render")


def _render_bounded(rays, chunk, grid, kwargs):
    """batchify_rays over the rays that cross an occupied cell of `grid`, each with its own [near, far]
    tightened to the span of those cells (csrc/ray_span.hip), scattered back to all rays."""
    R = rays.shape[0]
    hit, span, rows, rays_c = grid.bound_rays(rays)
    if rows.shape[0] > 0:
        part = batchify_rays(rays_c, chunk, **kwargs)
    else:
        part = _no_rays_result(rays.device, **kwargs)
    if rows.shape[0] == R:          # every ray is hit, in order: nothing to scatter
        all_ret = dict(part)
    else:
        white = bool(kwargs.get("white_bkgd", False))
        idx = rows.long()
        all_ret = {}
        for k, v in part.items():
            # a missed ray never stopped: its march_stop_samples is the lattice's length
            fill = kwargs.get("march_samples", 512) if k == "march_stop_samples" else _missed_value(k, white)
            full = torch.full((R,) + tuple(v.shape[1:]), fill, device=v.device, dtype=v.dtype)
            all_ret[k] = full.index_copy_(0, idx, v)
    all_ret.update(ray_hit=hit, ray_span=span)
    return all_ret


def render(H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., use_viewdirs=False,
           c2w_staticcam=None, ray_bounds=None, **kwargs):
    """run_nerf.py:86-151 -> [rgb_map, depth_map, acc_map, extras]. ray_bounds (an occupancy.OccupancyGrid;
    forward-only rendering): the packed rays are marched through the grid first; a ray that
    crosses no occupied cell gets the background without a field call, every other ray places its samples
    between its first and its last occupied cell instead of over [near, far]. The extras then also hold
    ray_hit (bool) and ray_span ([near', far'] per ray). Composes with occupancy= and early_stop=. None (the
    default) leaves the call as it is without it.
    march, march_samples, march_points go to render_rays; with ray_bounds each ray's lattice
    spans its own [near', far']. mlp_precision and table_precision go to
    render_rays as well, and so do march_stop and march_stop_slab and feature_precision (DESIGN.md
    §20), march_sh and march_sizes (the one count read per frame of ray_bounds stays),
    and march_grad (the march under gradients; ray_bounds stays forward-only) and march_jitter
    (perturb > 0 jitters the march's lattice; refused with ray_bounds).
    retraw is refused with march: the packed entries of several chunks do not
    concatenate."""
    # render_rays' value checks, also when no chunk reaches it (ray_bounds with every ray missed)
    # march_sizes only when given, as in render_rays: the pinned call record of tests/test_field_request.py
    opts = sparse_field.field_options("render", kwargs.get("march"), kwargs.get("march_sh"), kwargs.get("march_stop"),
                                      kwargs.get("march_stop_slab", 128), kwargs.get("mlp_precision"),
                                      kwargs.get("table_precision"), kwargs.get("feature_precision"),
                                      **({} if kwargs.get("march_sizes") is None
                                         else dict(march_sizes=kwargs["march_sizes"])))
    sparse_field.check_march_grad(kwargs.get("march_grad", False), kwargs.get("march"), opts.stop, "render")
    if sparse_field.check_march_jitter(kwargs.get("march_jitter", False), kwargs.get("march"), opts.stop,
                                       kwargs.get("march_sizes"), "render") and ray_bounds is not None:
        raise ValueError("render: march_jitter=True does not combine with ray_bounds= (a bounded ray's lattice has no "
                         "jittered entries)")
    if kwargs.get("march") is not None and kwargs.get("retraw"):
        raise ValueError("render: retraw is not available with march (the packed entries of several chunks do not "
                         "concatenate; call render_rays on one chunk)")
    if ray_bounds is not None:
        _check_ray_bounds(ray_bounds)
    if opts.half:
        nets = [kwargs[k] for k in ("network_fn", "network_fine") if kwargs.get(k) is not None]
        sparse_field.check_table_nets(nets, kwargs.get("embed_fn"), "render")
    if c2w is not None:
        rays_o, rays_d = get_rays(H, W, K, c2w)
    else:
        rays_o, rays_d = rays
    sh = rays_d.shape
    if use_viewdirs and c2w_staticcam is not None:
        # viewdirs from the moving camera, rays from the static one (run_nerf.py:115-126)
        vd = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
        rays_o, rays_d = get_rays(H, W, K, c2w_staticcam)
        rays = _pack_rays(H, W, K, rays_o, rays_d, near, far, ndc, False)
        rays = torch.cat([rays, torch.reshape(vd, [-1, 3]).float()], -1)
    else:
        rays = _pack_rays(H, W, K, rays_o, rays_d, near, far, ndc, use_viewdirs)
    if ray_bounds is None:
        all_ret = batchify_rays(rays, chunk, **kwargs)
    else:
        all_ret = _render_bounded(rays, chunk, ray_bounds, kwargs)
    for k in all_ret:
        all_ret[k] = torch.reshape(all_ret[k], list(sh[:-1]) + list(all_ret[k].shape[1:]))
    k_extract = ["rgb_map", "depth_map", "acc_map"]
    return [all_ret[k] for k in k_extract] + [{k: all_ret[k] for k in all_ret if k not in k_extract}]


def render_path(render_poses, hwf, K, chunk, render_kwargs, gt_imgs=None, savedir=None, render_factor=0):
    """run_nerf.py:154-215: full frames along a camera path through render() (device ray generation,
    chunked fused field, compositing) -> (rgbs [N,H,W,3], depths [N,H,W] normalised to [0,1]) as
    numpy. With gt_imgs (and render_factor 0) the per-view PSNR -10 log10(mean((rgb - gt)^2)) is
    printed and its average pickled to savedir, as the reference does; savedir also receives each
    view as 8-bit PNGs ({i:03d}.png colour, {i:03d}_depth.png depth) instead of the reference's
    matplotlib figure. As the reference, render_factor shrinks H, W and focal but passes K unchanged
    to render()."""
    H, W, focal = hwf
    near, far = render_kwargs["near"], render_kwargs["far"]
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
    rgbs, depths, psnrs = [], [], []
    dev = next(render_kwargs["network_fn"].parameters()).device     # the reference's default CUDA tensors
    for i, c2w in enumerate(render_poses):
        c2w = (c2w if torch.is_tensor(c2w) else torch.as_tensor(np.asarray(c2w, np.float32))).to(dev)
        with torch.no_grad():
            rgb, depth, acc, _ = render(H, W, K, chunk=chunk, c2w=c2w[:3, :4], **render_kwargs)
        rgb_np = rgb.cpu().numpy()
        rgbs.append(rgb_np)
        depths.append(((depth - near) / (far - near)).cpu().numpy())
        if gt_imgs is not None and render_factor == 0:
            gt = gt_imgs[i].cpu().numpy() if torch.is_tensor(gt_imgs[i]) else np.asarray(gt_imgs[i])
            p = -10. * np.log10(np.mean(np.square(rgb_np - gt)))
            print(p)
            psnrs.append(p)
        if savedir is not None:
            from PIL import Image
            os.makedirs(savedir, exist_ok=True)
            Image.fromarray(to8b(rgbs[-1])).save(os.path.join(savedir, f"{i:03d}.png"))
            Image.fromarray(to8b(np.clip(depths[-1], 0, 1))).save(os.path.join(savedir, f"{i:03d}_depth.png"))
    rgbs, depths = np.stack(rgbs, 0), np.stack(depths, 0)
    if gt_imgs is not None and render_factor == 0:
        avg = sum(psnrs) / len(psnrs)
        print("Avg PSNR over Test set: ", avg)
        if savedir is not None:
            import pickle
            with open(os.path.join(savedir, "test_psnrs_avg{:0.2f}.pkl".format(avg)), "wb") as fp:
                pickle.dump(psnrs, fp)
    return rgbs, depths
