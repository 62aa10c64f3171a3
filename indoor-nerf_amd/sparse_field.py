"""The field call of the forward-only render paths that evaluate only some samples: an occupancy grid
(occupancy.py), early ray termination (early_stop.py), or both; and the field
call of a grid march over its packed list of kept samples (MarchList). Also the one request
that carries every forward-only keyword to the field (FieldOptions, FieldRequest).

render_rays attaches a FieldRequest to the point tensor of a pass; the fused run_network (field.py) hands
a sparse call to run_network_sparse. The kept samples are compacted in ascending order
(csrc/sparse_points.hip), hash-encoded and run through the MLP, whose results land in their rows of raw;
every other sample gets an all-zero raw row, which compositing gives weight 0 exactly.
"""
import typing

import numpy as np
import torch

from . import _lib
from .early_stop import _LAST, tau_max_of
from .hashgrid import SHEncoder
from .occupancy import _check_modules

# why each keyword is forward-only (check_forward_only's and _begin_field_call's refusals)
NOT_IN_TRAINING = {"occupancy": "the grid is not used in training", "early_stop": "rays are not stopped in training",
                   "march": "rays are not marched in training", "ray_bounds": "rays are not bounded in training",
                   "mlp_precision": "the backward recomputes the forward in fp32",
                   "table_precision": "the backward scatters into the fp32 tables",
                   "feature_precision": "the backward reads fp32 features",
                   "march_sh": "the backward reads per-point SH rows",
                   "march_sizes": "the backward needs the list lengths on the host"}
DEFAULT_MARCH_POINTS = 1 << 21


class FieldOptions(typing.NamedTuple):
    """What the call-level keywords of one render_rays / render call ask of its field calls (field_options builds it):
    bf16 (mlp_precision="bf16"), half (table_precision="fp16", §18), packed (feature_precision="bf16",
    §20), by_ray (march_sh="rays", §21) and stop = (eps, slab) of march_stop or None (§19)."""
    bf16: bool = False
    half: bool = False
    packed: bool = False
    by_ray: bool = False
    stop: typing.Optional[tuple] = None

    def request(self, grid=None, early=None, march=None):
        """The FieldRequest of one field call under these options, or None when the call asks for nothing (the
        default path: nothing is built, nothing rides on the points)."""
        if grid is None and early is None and march is None and not (self.bf16 or self.half):
            return None
        return FieldRequest(grid, early, march, self.bf16, self.half, self.packed)


class MarchList:
    """The packed list of a grid march's field call (FieldRequest.march): the SH4 rows of the points'
    rays, sh_c [n, 16], and the largest slice of points per encode + MLP launch. With march_sh="rays" 
    sh_c is None and the list carries the points' ray index, ray_c int32 [n], and one SH record per ray, sh_rec
    [R, 40] (0 <= ray_c < R: the march's write guarantees it). With march_sizes="device"  the list's
    buffers hold `capacity` entries and its length is `total`, one int32 element in device memory. grad (march_grad,
    DESIGN.md §24): the field call may run under gradients, through field.PackedFieldFn; only a list of SH rows."""

    total = capacity = None     # a host-sized list: its length is the tensors'
    grad = False                # a forward-only list

    def __init__(self, sh_c, max_points=DEFAULT_MARCH_POINTS, ray_c=None, sh_rec=None, total=None, capacity=None,
                 grad=False):
        if (sh_c is None) == (ray_c is None) or (ray_c is None) != (sh_rec is None):
            raise ValueError("march: a request carries either sh_c or (ray_c, sh_rec)")
        if (total is None) != (capacity is None) or (total is not None and ray_c is None):
            raise ValueError("march: a device-sized list carries (total, capacity) and a ray index")
        self.sh_c, self.max_points = sh_c, check_march_points(max_points)
        self.ray_c, self.sh_rec = ray_c, sh_rec
        if total is not None:     # a host-sized list stays the four attributes it was
            self.total, self.capacity = total, capacity
        if grad:                  # likewise: a forward-only list carries nothing new
            if sh_c is None:
                raise ValueError("march: a list under gradients carries SH rows (the backward reads per-point SH rows)")
            self.grad = True


class FieldRequest:
    """One field call of a forward-only render on its way from render_rays to the fused run_network (field.py),
    attached to the point tensor as `pts._nerf_req` by render._query alone: the occupancy grid or
    None; early = (z [R, S], rays_d [R, 3], eps, slab) of early ray termination or None; march, the MarchList of a
    grid march's packed points [n, 3], or None; bf16, half, packed as in FieldOptions. run_network sets `used` (a
    foreign query function leaves it False and render._query raises) and, with early, `stop` (int32 [R]: leading
    samples for which the ray was alive)."""

    def __init__(self, grid=None, early=None, march=None, bf16=False, half=False, packed=False):
        if packed and not bf16:
            raise ValueError("field request: packed bf16 features need the bf16 MLP")
        if march is not None and (grid is not None or early is not None):
            raise ValueError("field request: a march's list does not combine with a grid or early termination")
        self.grid, self.early, self.march = grid, early, march
        self.bf16, self.half, self.packed = bool(bf16), bool(half), bool(packed)
        self.used, self.stop = False, None

    @property
    def what(self):
        """The keyword of the sparse field call the request asks for; None: the dense call."""
        if self.march is not None:
            return "march"
        if self.early is not None:
            return "early_stop"
        return None if self.grid is None else "occupancy"

    @property
    def blame(self):
        """The keyword that render._query's refusal of a foreign query function names."""
        return "table_precision" if self.half else "mlp_precision" if self.bf16 else self.what


def field_options(prefix, march, march_sh, march_stop, march_stop_slab, mlp_precision, table_precision,
                  feature_precision, march_sizes=None):
    """The value checks of the call-level forward-only keywords of `prefix` (render_rays, render), in one fixed
    order -> FieldOptions. The checks that need the call's modules (check_table_nets, check_mlp_nets) follow in the
    caller. march_sizes is checked last, against the others' answers; its own answer is not part of
    FieldOptions: the caller asks device_sized(march_sizes)."""
    by_ray = check_march_sh(march_sh, march, prefix)
    stop = check_march_stop(march_stop, march_stop_slab, march, prefix)
    bf16 = check_mlp_precision(mlp_precision, prefix)
    packed = check_feature_precision(feature_precision, bf16, prefix)
    half = check_table_precision(table_precision, prefix)
    check_march_sizes(march_sizes, march, by_ray, bf16, packed, prefix)
    return FieldOptions(bf16, half, packed, by_ray, stop)


def device_sized(value):
    """Whether a march_sizes value that check_march_sizes accepted asks for device-sized launches."""
    return isinstance(value, str) and value == "device"


def check_march_sizes(value, march, by_ray, bf16, packed, prefix):
    """march_sizes of `prefix` (render_rays, render) -> whether the march keeps its list lengths in device memory
    (DESIGN.md §23); its refusals, one fixed sentence each: an unknown value, "device" without march=, without each
    of march_sh="rays", mlp_precision="bf16" and feature_precision="bf16" (by_ray, bf16, packed: the answers of their
    checks), gradients enabled."""
    if value is None or (isinstance(value, str) and value == "host"):
        return False
    if not (isinstance(value, str) and value == "device"):
        raise ValueError(f"{prefix}: march_sizes must be None, 'host' or 'device', got {value!r}")
    if march is None:
        raise ValueError(f"{prefix}: march_sizes='device' needs march= (the sizes are those of a grid march's lists)")
    if not by_ray:
        raise ValueError(f"{prefix}: march_sizes='device' needs march_sh='rays' (the device-sized MLP reads SH through "
                         "the ray index)")
    if not bf16:
        raise ValueError(f"{prefix}: march_sizes='device' needs mlp_precision='bf16' (the device-sized MLP is the bf16 "
                         "forward)")
    if not packed:
        raise ValueError(f"{prefix}: march_sizes='device' needs feature_precision='bf16' (the device-sized encoder "
                         "writes packed bf16 features)")
    check_forward_only("march_sizes", prefix)
    return True


def check_mlp_precision(value, prefix):
    """mlp_precision of `prefix` (render_rays, render) -> whether it asks for the bf16 forward; its refusals: an
    unknown value, gradients enabled. Raw noise is fine: it is added after the field."""
    if value is None or (isinstance(value, str) and value == "fp32"):
        return False
    if not (isinstance(value, str) and value == "bf16"):
        raise ValueError(f"{prefix}: mlp_precision must be None, 'fp32' or 'bf16', got {value!r}")
    check_forward_only("mlp_precision", prefix)
    return True


def check_mlp_nets(nets, embed_fn, predict_normals, prefix="render_rays"):
    """render_rays' refusals with mlp_precision="bf16" that need its modules: before any launch, for the
    networks of every pass."""
    if predict_normals or any(getattr(fn, "raw_channels", 4) != 4 for fn in nets):
        raise ValueError(f"{prefix}: mlp_precision does not support predict_normals or a normals head")
    if embed_fn is not None:
        for fn in nets:
            _check_modules(embed_fn, fn, f"{prefix}: mlp_precision")


def check_mlp_field(call_ok, shape_words, fn, embed_fn):
    """The dense run_network's refusals for a request with bf16, all before any launch (call_ok: SHEncoder view
    encoding, viewdirs and the inputs that shape_words describes), in _begin_field_call's order."""
    what = "mlp_precision"
    if not call_ok:
        raise ValueError(f"{what}: needs the fused field call (SHEncoder view encoding, viewdirs, {shape_words})")
    _check_modules(embed_fn, fn, what)
    if fn.raw_channels != 4:
        raise ValueError(f"{what}: a normals head is not supported (the bf16 forward has no geo output)")
    if torch.is_grad_enabled():
        raise ValueError(f"{what}: forward-only (call under torch.no_grad(); {NOT_IN_TRAINING[what]})")


def check_feature_precision(value, mlp_bf16, prefix):
    """feature_precision of `prefix` (render_rays, render) -> whether it asks for packed bf16 features; its refusals:
    an unknown value, a call whose MLP is not the bf16 one (mlp_bf16: check_mlp_precision's answer), gradients
    enabled."""
    if value is None or (isinstance(value, str) and value == "fp32"):
        return False
    if not (isinstance(value, str) and value == "bf16"):
        raise ValueError(f"{prefix}: feature_precision must be None, 'fp32' or 'bf16', got {value!r}")
    if not mlp_bf16:
        raise ValueError(f"{prefix}: feature_precision='bf16' needs mlp_precision='bf16' (the fp32-accurate MLP reads "
                         "fp32 features)")
    check_forward_only("feature_precision", prefix)
    return True


def is_packed(req):
    """Whether the field call of FieldRequest `req` (or None) keeps packed bf16 features."""
    return req is not None and req.packed


def feature_buffer(req, n, device):
    """An uninitialised flat feature buffer of n (point, level) entries for the field call of FieldRequest `req` (or
    None) -> (buffer, w, dtype): w elements per entry, 2 float32 or, packed, 1 int32 word (half the bytes)."""
    if is_packed(req):
        return torch.empty(n, device=device, dtype=torch.int32), 1, torch.int32
    return torch.empty(2 * n, device=device, dtype=torch.float32), 2, torch.float32


def level_features(n_levels, P, device, packed=False):
    """The dense field call's uninitialised feature buffer of P points (FieldFn.forward, render.CoarseReuse):
    [L, P, 2] float32 or, packed, one bf16 word pair per entry, [L, P] int32."""
    if packed:
        return torch.empty(n_levels, P, device=device, dtype=torch.int32)
    return torch.empty(n_levels, P, 2, device=device, dtype=torch.float32)


def mlp_forward(req, feat, sl, sh_c, keep, n, weights, raw, order, rays=None):
    """The MLP launch of the sparse field calls: n points with level-major features (level stride sl; packed: in
    words, point stride 1) and SH rows at stride 16 -> their rows of raw (order: a nerf_point_order or None); req:
    the call's FieldRequest or None. rays = (ray index pointer, SH records pointer, number of records) instead of
    sh_c (march_sh="rays"; identity order): the _rays entry of the same precision."""
    bf16, packed = req is not None and req.bf16, is_packed(req)
    if rays is not None:
        if sh_c is not None or order is not None:
            raise ValueError("march_sh: a ray index replaces the SH rows and has no point order")
        ray_of, sh_rec, n_rays = rays
        name = "nerf_mlp_fwd_bf16_pkbf_rays" if packed else "nerf_mlp_fwd_bf16_rays" if bf16 else "nerf_mlp_fwd_rays"
        _lib.call(name, feat, 1 if packed else 2, sl, sh_rec, ray_of, n_rays, keep, n, weights, raw, _lib.stream())
        return
    front = (feat, 1 if packed else 2, sl, sh_c, 16, None, 1, keep, n, weights, raw)
    if bf16:
        _lib.call("nerf_mlp_fwd_bf16_pkbf" if packed else "nerf_mlp_fwd_bf16", *front, order, _lib.stream())
    else:
        _lib.call("nerf_mlp_fwd_ord", *front, None, None, None, 0, order, _lib.stream())


def check_table_precision(value, prefix):
    """table_precision of `prefix` (render_rays, render) -> whether it asks for the fp16 tables; its refusals: an
    unknown value, gradients enabled. Raw noise is fine: the encoding does not care."""
    if value is None or (isinstance(value, str) and value == "fp32"):
        return False
    if not (isinstance(value, str) and value == "fp16"):
        raise ValueError(f"{prefix}: table_precision must be None, 'fp32' or 'fp16', got {value!r}")
    check_forward_only("table_precision", prefix)
    return True


def _check_table_modules(embed_fn, fn, what):
    """The modules the fp16 gather can serve: the fused field's, with plain fp32 tables. A normals head and a
    quantized MLP are fine: the encoding does not care."""
    from .field import NeRFSmall
    from .hashgrid import HashEmbedder
    if not isinstance(embed_fn, HashEmbedder) or not isinstance(fn, NeRFSmall):
        raise ValueError(f"{what}: needs the fused field modules (HashEmbedder + NeRFSmall), got "
                         f"{type(embed_fn).__name__} + {type(fn).__name__}")
    if embed_fn.use_quantization:
        raise ValueError(f"{what}: A-CAQ quantizers are not supported (they have their own packed tables)")


def check_table_nets(nets, embed_fn, prefix="render_rays"):
    """render_rays' refusals with table_precision="fp16" that need its modules: before any launch, for the
    networks of every pass."""
    if embed_fn is not None:
        for fn in nets:
            _check_table_modules(embed_fn, fn, f"{prefix}: table_precision")


def check_table_field(call_ok, shape_words, fn, embed_fn):
    """The dense run_network's refusals for a request with half, all before any launch (call_ok: SHEncoder view
    encoding, viewdirs and the inputs that shape_words describes)."""
    what = "table_precision"
    if not call_ok:
        raise ValueError(f"{what}: needs the fused field call (SHEncoder view encoding, viewdirs, {shape_words})")
    _check_table_modules(embed_fn, fn, what)
    if torch.is_grad_enabled():
        raise ValueError(f"{what}: forward-only (call under torch.no_grad(); {NOT_IN_TRAINING[what]})")


def check_march_points(m):
    if isinstance(m, bool) or not isinstance(m, int) or m < 1:
        raise ValueError(f"march: march_points must be a positive integer, got {m!r}")
    if 16 * (m + 32) >= 2 ** 31:
        raise ValueError(f"march: march_points {m} exceeds the MLP's 32-bit row indexing (16 (n + 32) < 2^31)")
    return m


def check_march_stop(march_stop, march_stop_slab, march, prefix):
    """march_stop / march_stop_slab of `prefix` (render_rays, render) -> (eps, slab), or None without march_stop;
    their refusals, one fixed sentence each."""
    if march_stop is None:
        return None
    if march is None:
        raise ValueError(f"{prefix}: march_stop needs march= (rays are stopped inside a grid march; early_stop= is the "
                         "dense path's)")
    if isinstance(march_stop, bool) or not isinstance(march_stop, (float, np.floating)) or not 0.0 < march_stop < 1.0:
        raise ValueError(f"{prefix}: march_stop must be a float transmittance threshold in (0, 1), got {march_stop!r}")
    if (isinstance(march_stop_slab, bool) or not isinstance(march_stop_slab, (int, np.integer))
            or march_stop_slab < 1):
        raise ValueError(f"{prefix}: march_stop_slab must be a positive integer, got {march_stop_slab!r}")
    return float(march_stop), int(march_stop_slab)


def check_march_sh(value, march, prefix):
    """march_sh of `prefix` (render_rays, render) -> whether the march's list carries a ray index instead of SH rows
    (DESIGN.md §21); its refusals, one fixed sentence each: an unknown value, "rays" without march=, gradients
    enabled."""
    if value is None or (isinstance(value, str) and value == "rows"):
        return False
    if not (isinstance(value, str) and value == "rays"):
        raise ValueError(f"{prefix}: march_sh must be None, 'rows' or 'rays', got {value!r}")
    if march is None:
        raise ValueError(f"{prefix}: march_sh='rays' needs march= (the ray index belongs to a grid march's list)")
    check_forward_only("march_sh", prefix)
    return True


def check_march_grad(value, march, stop, prefix):
    """march_grad of `prefix` (render_rays, render) -> whether the march may run under gradients; its
    refusals, one fixed sentence each: a value that is not a bool, True without march=, True with march_stop= (stop:
    check_march_stop's answer). It follows field_options, whose forward-only keywords refuse gradients first."""
    if not isinstance(value, bool):
        raise ValueError(f"{prefix}: march_grad must be a bool, got {value!r}")
    if not value:
        return False
    if march is None:
        raise ValueError(f"{prefix}: march_grad=True needs march= (the gradients are those of a grid march)")
    if stop is not None:
        raise ValueError(f"{prefix}: march_grad=True does not combine with march_stop= (the slabs' carried state has no "
                         "backward)")
    return True


def check_march_jitter(value, march, stop, march_sizes, prefix):
    """march_jitter of `prefix` (render_rays, render) -> whether perturb > 0 jitters the march's lattice (DESIGN.md
    §25); its refusals, one fixed sentence each: a value that is not a bool, True without march=, True with march_stop=
    (stop: check_march_stop's answer) or with march_sizes="device": the slab walk and the device-sized path have no
    jittered entries. It follows field_options and check_march_grad."""
    if not isinstance(value, bool):
        raise ValueError(f"{prefix}: march_jitter must be a bool, got {value!r}")
    if not value:
        return False
    if march is None:
        raise ValueError(f"{prefix}: march_jitter=True needs march= (the jitter is that of a grid march's lattice)")
    if stop is not None:
        raise ValueError(f"{prefix}: march_jitter=True does not combine with march_stop= (the slab walk has no jittered "
                         "entries)")
    if device_sized(march_sizes):
        raise ValueError(f"{prefix}: march_jitter=True does not combine with march_sizes='device' (the device-sized "
                         "path has no jittered entries)")
    return True


def check_forward_only(what, prefix, raw_noise_std=0., grad=False):
    """The refusals every forward-only keyword `what` of `prefix` (render_rays, render) shares: no gradients (grad:
    the call carries march_grad=True), no raw noise."""
    if torch.is_grad_enabled() and not grad:
        raise ValueError(f"{prefix}: {what} is forward-only (call under torch.no_grad(); {NOT_IN_TRAINING[what]})")
    if raw_noise_std > 0.:
        raise ValueError(f"{prefix}: {what} needs raw_noise_std == 0 (noise makes relu(sigma + noise) > 0 at skipped "
                         "samples)")


def _begin_field_call(what, inputs_ok, shape_words, viewdirs, fn, embed_fn, embeddirs_fn, grad=False):
    """What run_network_sparse and run_network_packed do first: their refusals, all before any launch (inputs_ok:
    the inputs are what shape_words says; grad: the request's list allows gradients, MarchList.grad), then the step
    count of a training-mode encoder."""
    if not isinstance(embeddirs_fn, SHEncoder) or viewdirs is None or not inputs_ok:
        raise ValueError(f"{what}: needs the fused field call (SHEncoder view encoding, viewdirs, {shape_words})")
    _check_modules(embed_fn, fn, what)
    if fn.raw_channels != 4:
        raise ValueError(f"{what}: a normals head is not supported (run_network's box mask then lands on n_z, "
                         "not on sigma, so a skipped sample is not a zero-weight sample)")
    if torch.is_grad_enabled() and not grad:
        raise ValueError(f"{what}: forward-only (call under torch.no_grad(); {NOT_IN_TRAINING[what]})")
    if embed_fn.training:
        embed_fn.current_step += 1


def run_network_packed(inputs, viewdirs, fn, embed_fn, embeddirs_fn, req):
    """run_network (field.py) for a FieldRequest with a MarchList: inputs [n, 3], the packed kept samples of a
    march -> raw [n, 4]. The hash encoding and the MLP (identity order, SH rows at stride 16, or with a list by ray
    index the slice of the index and the whole of the records) run over the list in slices of at most max_points
    points; a point's result does not depend on its slice."""
    from .field import _weights_struct
    ml = req.march
    by_ray = ml.ray_c is not None
    _begin_field_call("march", inputs.dim() == 2, "packed inputs [n, 3]", viewdirs, fn, embed_fn, embeddirs_fn,
                      grad=ml.grad)
    if ml.grad and torch.is_grad_enabled():
        return _run_network_packed_grad(inputs, fn, embed_fn, req)
    if ml.total is not None:
        return _run_network_packed_dev(inputs, fn, embed_fn, req)
    n, dev, L = inputs.shape[0], inputs.device, embed_fn.n_levels
    if by_ray:
        if tuple(ml.ray_c.shape) != (n,) or ml.sh_rec.dim() != 2 or ml.sh_rec.shape[1] != 40:
            raise ValueError("march: ray index / SH records of the request do not match the points")
        sh_rec, n_rec = _lib.ptr(ml.sh_rec, "sh_rec"), ml.sh_rec.shape[0]
    elif tuple(ml.sh_c.shape) != (n, 16):
        raise ValueError("march: SH rows of the request do not match the points")
    f = dict(device=dev, dtype=torch.float32)
    raw = torch.empty(n, 4, **f)
    if n == 0:
        return raw
    pts = inputs.detach().float().contiguous()
    weights = _weights_struct(fn.mlp_weights())
    m = min(n, ml.max_points)
    (feat, w, fdt), keep = feature_buffer(req, L * m, dev), torch.empty(m, device=dev, dtype=torch.bool)
    for s0 in range(0, n, m):
        k = min(m, n - s0)
        embed_fn.encode_into(pts[s0:s0 + k], feat[:L * k * w], w, w * k, keep[:k], half=req.half, packed=req.packed)
        mlp_forward(req, _lib.ptr(feat, "feat", fdt), w * k, None if by_ray else _lib.ptr_at(ml.sh_c, 16 * s0, "sh_c"),
                    _lib.ptr(keep, "keep", torch.bool), k, weights, _lib.ptr_at(raw, 4 * s0, "raw"), None,
                    (_lib.ptr_at(ml.ray_c, s0, "ray_c", torch.int32), sh_rec, n_rec) if by_ray else None)
    return raw


def _run_network_packed_grad(inputs, fn, embed_fn, req):
    """run_network_packed under gradients (march_grad): the list in slices of at most max_points points,
    each its own application of field.PackedFieldFn with its own saved features; the raws are concatenated. An empty
    list is one application on no points, which launches nothing and keeps raw attached to the graph."""
    from .field import PackedFieldFn
    ml = req.march
    if req.bf16 or req.half or req.packed:
        what = "table_precision" if req.half else "feature_precision" if req.packed else "mlp_precision"
        raise ValueError(f"{what}: forward-only (call under torch.no_grad(); {NOT_IN_TRAINING[what]})")
    n = inputs.shape[0]
    if tuple(ml.sh_c.shape) != (n, 16):
        raise ValueError("march: SH rows of the request do not match the points")
    pts, sh_c = inputs.detach().float().contiguous(), ml.sh_c.detach().float().contiguous()
    params = (*embed_fn.tables(), *fn.mlp_weights())
    m = max(1, min(n, ml.max_points))
    parts = [PackedFieldFn.apply(pts[s0:s0 + m], sh_c[s0:s0 + m], embed_fn, fn, *params)
             for s0 in range(0, max(n, 1), m)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def _run_network_packed_dev(inputs, fn, embed_fn, req):
    """run_network_packed for a device-sized list (march_sizes="device"): inputs [capacity, 3] of which
    the first *ml.total rows are points -> raw [capacity, 4] with those rows written and the others left as allocated.
    ceil(capacity / max_points) slices, a number the host knows; slice s covers clamp(total - s m, 0, m) points, read
    by the kernels (the _dev entries), so an empty slice is launched and does nothing. No host read."""
    from .field import _weights_struct
    ml = req.march
    cap, dev, L = inputs.shape[0], inputs.device, embed_fn.n_levels
    if not (req.bf16 and req.packed):
        raise ValueError("march: a device-sized list needs the bf16 MLP on packed bf16 features")
    if (cap != ml.capacity or tuple(ml.ray_c.shape) != (cap,) or ml.sh_rec.dim() != 2 or ml.sh_rec.shape[1] != 40
            or ml.total.dtype != torch.int32 or ml.total.numel() != 1):
        raise ValueError("march: ray index / SH records / total of the request do not match the points")
    raw = torch.empty(cap, 4, device=dev, dtype=torch.float32)
    if cap == 0:
        return raw
    sh_rec, n_rec = _lib.ptr(ml.sh_rec, "sh_rec"), ml.sh_rec.shape[0]
    total = _lib.ptr(ml.total, "total", torch.int32)
    pts = inputs.detach().float().contiguous()
    weights = _weights_struct(fn.mlp_weights())
    m = min(cap, ml.max_points)
    feat, keep = torch.empty(L, m, device=dev, dtype=torch.int32), torch.empty(m, device=dev, dtype=torch.bool)
    for s0 in range(0, cap, m):
        k = min(m, cap - s0)
        embed_fn.encode_into(pts[s0:s0 + k], feat, 1, m, keep, half=req.half, packed=True, count=(ml.total, s0))
        _lib.call("nerf_mlp_fwd_bf16_pkbf_rays_dev", _lib.ptr(feat, "feat", torch.int32), 1, m, sh_rec,
                  _lib.ptr_at(ml.ray_c, s0, "ray_c", torch.int32), n_rec, _lib.ptr(keep, "keep", torch.bool), total, s0,
                  k, weights, _lib.ptr_at(raw, 4 * s0, "raw"), _lib.stream())
    return raw


def run_network_sparse(inputs, viewdirs, fn, embed_fn, embeddirs_fn, req):
    """run_network (field.py) for a FieldRequest whose `what` is set: inputs [R, S, 3], viewdirs [R, 3] ->
    raw [R, S, 4] with the field evaluated at the kept samples only and zero rows elsewhere (a march's list goes to
    run_network_packed). Without early termination the call is one slab through req.grid.compact; with it, slabs of
    req.early's size front to back, nerf_ert_advance between them, and req.stop receives the stops."""
    if req.march is not None:
        return run_network_packed(inputs, viewdirs, fn, embed_fn, embeddirs_fn, req)
    from .field import _point_order, _weights_struct
    what = req.what
    _begin_field_call(what, inputs.dim() == 3, "inputs [R, S, 3]", viewdirs, fn, embed_fn, embeddirs_fn)
    R, S = inputs.shape[0], inputs.shape[1]
    P, dev, L = R * S, inputs.device, embed_fn.n_levels
    if 16 * (P + 32) >= 2 ** 31:
        raise ValueError(f"{what}: {P} points per field call exceed the MLP's 32-bit row indexing; use a smaller chunk")
    if req.early is not None:
        z, rays_d, eps, K = req.early
        if tuple(z.shape) != (R, S) or tuple(rays_d.shape) != (R, 3):
            raise ValueError("early_stop: z / rays_d of the request do not match the points")
    pts = inputs.detach().reshape(-1, 3).float().contiguous()
    sh_rays = getattr(viewdirs, "_nerf_sh", None)
    viewdirs = viewdirs.detach().float().contiguous()
    if sh_rays is not None:
        viewdirs._nerf_sh = sh_rays
    f, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    raw = torch.empty(P, 4, **f)
    weights = _weights_struct(fn.mlp_weights())

    _, w, fdt = feature_buffer(req, 0, dev)   # elements per (point, level) entry of the call's feature buffers

    def field(n, rows, pts_c, sh_c, feat, keep):
        """The field at the n compacted points; rows of raw `rows` receive the results."""
        embed_fn.encode_into(pts_c, feat, w, w * n, keep, half=req.half, packed=req.packed)
        mlp_forward(req, _lib.ptr(feat, "feat", fdt), w * n, _lib.ptr(sh_c, "sh_c"),
                    _lib.ptr(keep, "keep", torch.bool), n, weights, _lib.ptr(raw, "raw"), _point_order((rows, 0, 0)))

    if req.early is None:
        # one slab, no alive flags: the grid's own compaction, every buffer sized exactly after the count
        rows, pts_c, sh_c = req.grid.compact(pts, viewdirs, S, raw)
        n = rows.shape[0]
        if n > 0:
            field(n, rows, pts_c, sh_c, feature_buffer(req, L * n, dev)[0], torch.empty(n, device=dev, dtype=torch.bool))
        return raw.reshape(R, S, 4)

    z, rays_d = z.detach().float().contiguous(), rays_d.detach().float().contiguous()
    grid = req.grid
    if grid is not None:
        bmin, bmax, res, bits = grid._bmin, grid._bmax, grid.resolution, grid._bits()
    else:
        bmin, bmax, res, bits = embed_fn._meta["bmin"], embed_fn._meta["bmax"], 1, None   # the encoder's own box
    tau_max = tau_max_of(eps)
    tau = torch.zeros(R, **f)
    alive = torch.ones(R, device=dev, dtype=torch.uint8)
    stop = torch.full((R,), S, **i32)
    # scratch of the worst-case slab (every candidate kept), once per field call
    cap = R * min(K, S)
    count = torch.empty(1, **i32)
    ws = torch.empty(int(_lib.load().nerf_ert_compact_workspace_bytes(cap)) // 4, **i32)
    rows, pts_c, sh_c = torch.empty(cap, **i32), torch.empty(cap, 3, **f), torch.empty(cap, 16, **f)
    feat, keep = feature_buffer(req, L * cap, dev)[0], torch.empty(cap, device=dev, dtype=torch.bool)
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
            field(n, rows, pts_c[:n], sh_c, feat[:L * n * w], keep[:n])
        evaluated += n
        if s1 < S:
            _lib.call("nerf_ert_advance", _lib.ptr(raw, "raw"), _lib.ptr(z, "z"), _lib.ptr(rays_d, "rays_d"), R, S,
                      s0, s1, tau_max, _lib.ptr(tau, "tau"), _lib.ptr(alive, "alive", torch.uint8),
                      _lib.ptr(stop, "stop", torch.int32), _lib.stream())
    _LAST["counts"] = (evaluated, P)
    req.stop = stop
    return raw.reshape(R, S, 4)
