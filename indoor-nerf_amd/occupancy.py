"""Occupancy grid of the scene box: empty-space skipping for forward-only rendering.

A density bitfield over the scene box, built from the trained field (OccupancyGrid.update), and the
field call render_rays makes with one (sparse_field.run_network_sparse): the kept samples — inside the box and in
an occupied cell — are compacted in ascending order (csrc/sparse_points.hip), hash-encoded and run through
the MLP, whose results land in their rows of raw; every skipped sample gets an all-zero raw row.
Compositing gives a sample with relu(sigma) = 0 weight 0 exactly, so skipping a sample the dense path
would have given relu(sigma) = 0 changes nothing, and skipping any other equals masking sigma there.

    grid = OccupancyGrid(args.bounding_box)              # after training / loading a checkpoint
    grid.update(render_kwargs_test["embed_fn"], [render_kwargs_test["network_fn"],
                                                 render_kwargs_test["network_fine"]])
    render_kwargs_test["occupancy"] = grid                # render / render_path skip empty space

Forward-only: no gradients, no raw noise, no normals head, no A-CAQ (render_rays and
run_network_sparse raise ValueError otherwise). The grid is not used in training and is not stored
in checkpoints.
"""
import numpy as np
import torch

from . import _lib
from .hashgrid import HashEmbedder, _bbox_floats

MAX_RESOLUTION = 1024   # res^3 cell ids fit 32 bits (csrc/occupancy.hip)


def _check_modules(embed_fn, fn, what="occupancy"):
    """The field the occupancy kernels can run: fp32 tables and plain MLP weights."""
    from .field import NeRFSmall
    if not isinstance(embed_fn, HashEmbedder) or not isinstance(fn, NeRFSmall):
        raise ValueError(f"{what}: needs the fused field modules (HashEmbedder + NeRFSmall), got "
                         f"{type(embed_fn).__name__} + {type(fn).__name__}")
    if embed_fn.use_quantization or fn.use_quantization:
        raise ValueError(f"{what}: A-CAQ quantizers are not supported (fp32 tables and weights only: the "
                         "activation calibration depends on which points come first)")


MAX_MARCH_SAMPLES = 4096   # lattice samples per ray of a march (csrc/march.hip)


def check_march_samples(K, what):
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= MAX_MARCH_SAMPLES:
        raise ValueError(f"{what}: march_samples must be an integer in 1..{MAX_MARCH_SAMPLES}, got {K!r}")
    return int(K)


def _packed_rows(rays, method):
    """Packed ray rows as OccupancyGrid.`method` takes them (fp32, contiguous, detached), or ValueError."""
    if not torch.is_tensor(rays) or rays.dim() != 2 or rays.shape[1] not in (8, 11):
        raise ValueError(f"OccupancyGrid.{method}: rays must be packed rows [R, 8] or [R, 11] (o, d, near, far"
                         f"[, viewdir]), got {tuple(rays.shape) if torch.is_tensor(rays) else type(rays).__name__}")
    return rays.detach().float().contiguous()


class OccupancyGrid:
    """Density bitfield over `bounding_box`: resolution^3 cells, cell (ix, iy, iz) = bit
    (ix*res + iy)*res + iz (csrc/occupancy.hip has the cell rule). A new grid is empty."""

    def __init__(self, bounding_box, resolution=128, device=None):
        res = int(resolution)
        if not 1 <= res <= MAX_RESOLUTION:
            raise ValueError(f"OccupancyGrid: resolution must be 1..{MAX_RESOLUTION}, got {resolution}")
        bmin, bmax = _bbox_floats(bounding_box)
        self.bounding_box = bounding_box
        self.resolution = res
        self.n_cells = res ** 3
        self.n_words = (self.n_cells + 31) // 32
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._bmin, self._bmax = _lib.host_f32(bmin), _lib.host_f32(bmax)
        self.bits = torch.zeros(self.n_words, dtype=torch.int32, device=self.device)
        # (points evaluated, points total) of the last field call. The first is an int, or, after a device-sized march
        # (DESIGN.md §23), a list of int32 [1] device views into the lists' offsets that last_counts() sums and replaces
        self._last = (0, 0)

    def _bits(self, t=None):
        return _lib.ptr(self.bits if t is None else t, "occupancy bits", torch.int32)

    # ---- bitfield <-> bool[res, res, res] ---------------------------------------------------
    def set_mask(self, mask):
        """Set the grid from a bool [res, res, res] array or tensor (True = occupied)."""
        m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
        res = self.resolution
        if m.shape != (res, res, res):
            raise ValueError(f"OccupancyGrid.set_mask: mask must be [{res}, {res}, {res}], got {tuple(m.shape)}")
        flat = np.zeros(32 * self.n_words, np.uint8)
        flat[:self.n_cells] = m.reshape(-1).astype(bool)
        words = np.packbits(flat, bitorder="little").view("<u4").astype(np.uint32)
        self.bits.copy_(torch.from_numpy(words.view(np.int32)))

    def mask(self):
        """The grid as a bool [res, res, res] tensor on its device."""
        words = self.bits.cpu().numpy().view(np.uint32).astype("<u4")
        flat = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.n_cells]
        res = self.resolution
        return torch.from_numpy(flat.astype(bool).reshape(res, res, res)).to(self.device)

    def occupied_fraction(self):
        return float(self.mask().float().mean())

    def last_counts(self):
        """(points evaluated, points total) of the most recent field call through this grid. After a device-sized
        march the evaluated count is still in device memory, one int32 element per list: it is read
        here, once, when it is asked for."""
        n, total = self._last
        if not isinstance(n, int):
            n = int(torch.cat([c.reshape(1) for c in n]).sum().item())
            self._last = (n, total)
        return self._last

    # ---- kernels ------------------------------------------------------------------------------
    def query(self, pts):
        """bool [...]: the point of pts [..., 3] is inside the box and its cell is occupied."""
        p = pts.detach().reshape(-1, 3).float().contiguous()
        out = torch.empty(p.shape[0], dtype=torch.bool, device=p.device)
        _lib.call("nerf_occ_query", _lib.ptr(p, "pts"), p.shape[0], self._bmin, self._bmax, self.resolution,
                  self._bits(), _lib.ptr(out, "out", torch.bool), _lib.stream())
        return out.reshape(pts.shape[:-1])

    def cell_points(self, cell_begin, n_cells, samples_per_cell, seed):
        """[n_cells, samples_per_cell, 3]: the builder's sample positions of cells [cell_begin, +n_cells)
        (sample 0 the centre, the others uniform in the cell; the same for any chunking)."""
        pts = torch.empty(n_cells, samples_per_cell, 3, device=self.device, dtype=torch.float32)
        _lib.call("nerf_occ_cell_points", self._bmin, self._bmax, self.resolution, int(cell_begin), int(n_cells),
                  int(samples_per_cell), int(seed), 0, _lib.ptr(pts, "pts"), _lib.stream())
        return pts

    def update(self, embed_fn, networks, sigma_thresh=0.0, samples_per_cell=8, dilate=1, seed=0,
               chunk_cells=1 << 17):
        """Rebuild the grid from the field: a cell is occupied when sigma > sigma_thresh at any of its
        samples_per_cell positions under any of `networks` (a NeRFSmall or a list: network_fn and
        network_fine union into one grid), then dilated `dilate` times by one cell. Walks the cells in
        chunks of chunk_cells (a multiple of 64; ~1.3 KB of scratch per cell at 8 samples)."""
        from .field import NeRFSmall, _weights_struct
        nets = [networks] if isinstance(networks, NeRFSmall) else [n for n in networks if n is not None]
        nets = [n for i, n in enumerate(nets) if all(n is not m for m in nets[:i])]
        for net in nets:
            _check_modules(embed_fn, net)
        if not nets:
            raise ValueError("OccupancyGrid.update: no network")
        if chunk_cells < 64 or chunk_cells % 64:
            raise ValueError(f"OccupancyGrid.update: chunk_cells must be a positive multiple of 64, got {chunk_cells}")
        spc, res, dev = int(samples_per_cell), self.resolution, self.device
        L = embed_fn.n_levels
        view = torch.tensor([[0.0, 0.0, 1.0]], device=dev)      # sigma does not depend on the view direction
        with torch.no_grad():
            self.bits.zero_()
            for c0 in range(0, self.n_cells, chunk_cells):
                nc = min(chunk_cells, self.n_cells - c0)
                n = nc * spc
                pts = self.cell_points(c0, nc, spc, seed).view(n, 3)
                feat = torch.empty(L, n, 2, device=dev, dtype=torch.float32)
                keep = torch.empty(n, device=dev, dtype=torch.bool)
                embed_fn.encode_into(pts, feat, 2, 2 * n, keep)
                raw = torch.empty(n, 4, device=dev, dtype=torch.float32)
                for net in nets:
                    _lib.call("nerf_mlp_fwd", _lib.ptr(feat, "feat"), 2, 2 * n, None, 0, _lib.ptr(view, "viewdirs"), n,
                              _lib.ptr(keep, "keep", torch.bool), n, _weights_struct(net.mlp_weights()),
                              _lib.ptr(raw, "raw"), None, _lib.stream())
                    _lib.call("nerf_occ_mark", _lib.ptr(raw, "raw"), res, c0, nc, spc, float(sigma_thresh),
                              self._bits(), _lib.stream())
            for _ in range(int(dilate)):
                out = torch.empty_like(self.bits)
                _lib.call("nerf_occ_dilate", self._bits(), res, self._bits(out), _lib.stream())
                self.bits = out
        return self

    def compact(self, pts, viewdirs, samples_per_ray, raw):
        """The kept points of a field call over pts [P, 3] (point p on ray p // samples_per_ray):
        (rows int32 [n] ascending, pts_c [n, 3], sh_c [n, 16]); the rows of raw [P, 4] of the skipped
        points are zeroed. One host read (the count) between the two launches sizes the outputs."""
        P, dev = pts.shape[0], pts.device
        sh_rays = getattr(viewdirs, "_nerf_sh", None)
        i32 = dict(device=dev, dtype=torch.int32)
        count = torch.empty(1, **i32)
        ws = torch.empty(int(_lib.load().nerf_occ_compact_workspace_bytes(P)) // 4, **i32)

        def run(stages, cap, rows, pts_c, sh_c):
            _lib.call("nerf_occ_compact", _lib.ptr(pts, "pts"), P, _lib.ptr(sh_rays, "sh_rows", allow_none=True),
                      None if sh_rays is not None else _lib.ptr(viewdirs, "viewdirs"), samples_per_ray,
                      self._bmin, self._bmax, self.resolution, self._bits(), stages, cap,
                      _lib.ptr(rows, "rows", torch.int32, True), _lib.ptr(count, "count", torch.int32),
                      _lib.ptr(pts_c, "pts_c", allow_none=True), _lib.ptr(sh_c, "sh_c", allow_none=True),
                      _lib.ptr(raw, "raw"), _lib.ptr(ws, "workspace", torch.int32), ws.numel() * 4, _lib.stream())
        run(1, 0, None, None, None)
        n = int(count.item())
        f = dict(device=dev, dtype=torch.float32)
        rows, pts_c, sh_c = torch.empty(n, **i32), torch.empty(n, 3, **f), torch.empty(n, 16, **f)
        if P > 0:
            run(2, n, rows if n else None, pts_c if n else None, sh_c if n else None)
        self._last = (n, P)
        return rows, pts_c, sh_c

    # ---- per-ray sample bounds (csrc/ray_span.hip) --------------------------------
    def _span(self, rays):
        rays = _packed_rows(rays, "ray_span")
        R, C, dev = rays.shape[0], rays.shape[1], rays.device
        hit = torch.empty(R, dtype=torch.bool, device=dev)
        span = torch.empty(R, 2, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(_lib.load().nerf_ray_span_workspace_bytes(R)) // 4, dtype=torch.int32, device=dev)
        _lib.call("nerf_ray_span", _lib.ptr(rays, "rays"), R, C, self._bmin, self._bmax, self.resolution, self._bits(),
                  _lib.ptr(hit, "hit", torch.bool), _lib.ptr(span, "span"), _lib.ptr(count, "count", torch.int32),
                  _lib.ptr(ws, "workspace", torch.int32), ws.numel() * 4, _lib.stream())
        return rays, hit, span, count, ws

    def ray_span(self, rays):
        """Where along each packed ray row [R, 8 or 11] (o, d, near, far[, viewdir]) there is anything:
        (hit bool [R], span float32 [R, 2]). hit: the ray crosses an occupied cell inside [near, far];
        span: from the first to the last such cell, widened by pad and clipped to [near, far]
        ([near, far] itself for a missed ray)."""
        _, hit, span, _, _ = self._span(rays)
        return hit, span

    def bound_rays(self, rays):
        """ray_span and the hit rays compacted: (hit [R], span [R, 2], rows int32 [n] ascending,
        rays_c [n, C] = the hit rows with columns 6 and 7 replaced by their spans). One host read (the
        count) sizes the outputs."""
        rays, hit, span, count, ws = self._span(rays)
        R, C, dev = rays.shape[0], rays.shape[1], rays.device
        n = int(count.item()) if R > 0 else 0
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        rays_c = torch.empty(n, C, dtype=torch.float32, device=dev)
        if n > 0:
            _lib.call("nerf_ray_span_gather", _lib.ptr(rays, "rays"), R, C, _lib.ptr(hit, "hit", torch.bool),
                      _lib.ptr(span, "span"), n, _lib.ptr(rows, "rows", torch.int32), _lib.ptr(rays_c, "rays_c"),
                      _lib.ptr(ws, "workspace", torch.int32), ws.numel() * 4, _lib.stream())
        return hit, span, rows, rays_c

    # ---- grid ray marching (csrc/march.hip) ----------------------------------------
    @staticmethod
    def _jitter_args(jitter):
        """The uniforms of a jittered walk as the nerf_jitter_ entries take them: jitter = (u float32
        [R, K] or None, seed, offset, d_rng or None), the sampler's four."""
        u, seed, off, rng = jitter
        return _lib.ptr(u, "u", allow_none=True), int(seed), int(off), rng

    def _march_count(self, rays, K, k0=None, k1=None, alive=None, dirs=True, sized="host", jitter=None):
        """nerf_march_count over packed rows -> (rays, t, counts [R], offsets [R + 1], rays_d [R, 3], n). With a
        lattice range [k0, k1) (and alive, uint8 [R], or None for every ray): nerf_slab_march_count over that range
        of the rays alive. dirs=False: rays_d is not written (None). sized="device" (DESIGN.md §23):
        n is the device element offsets[R:R + 1], int32 [1], and the host reads nothing. jitter (the
        whole lattice, host-sized): nerf_jitter_march_count with these uniforms (_jitter_args)."""
        from .render import _linspace
        if jitter is not None and (k0 is not None or sized == "device"):
            raise ValueError("OccupancyGrid.march: a jittered walk has no slab and no device-sized entries")
        rays = _packed_rows(rays, "march")
        K = check_march_samples(K, "OccupancyGrid.march")
        R, C, dev = rays.shape[0], rays.shape[1], rays.device
        if R * K > 2 ** 31 - 1:
            raise ValueError(f"OccupancyGrid.march: {R} rays x {K} samples exceed 2^31 - 1; use a smaller chunk")
        i32 = dict(device=dev, dtype=torch.int32)
        t = _linspace(K, dev)
        counts, offsets = torch.empty(R, **i32), torch.zeros(R + 1, **i32) if R == 0 else torch.empty(R + 1, **i32)
        rays_d = torch.empty(R, 3, device=dev, dtype=torch.float32) if dirs else None
        n = 0
        if R > 0:
            ws = torch.empty(int(_lib.load().nerf_march_workspace_bytes(R)) // 4, **i32)
            name, slab, uniforms = "nerf_march_count", (), ()
            if k0 is not None:
                name, slab = "nerf_slab_march_count", (int(k0), int(k1), _lib.ptr(alive, "alive", torch.uint8, True))
            if jitter is not None:
                name, uniforms = "nerf_jitter_march_count", self._jitter_args(jitter)
            _lib.call(name, _lib.ptr(rays, "rays"), R, C, _lib.ptr(t, "t"), K, *slab, self._bmin, self._bmax,
                      self.resolution, self._bits(), _lib.ptr(counts, "counts", torch.int32),
                      _lib.ptr(offsets, "offsets", torch.int32), _lib.ptr(rays_d, "rays_d", allow_none=True),
                      _lib.ptr(ws, "workspace", torch.int32), ws.numel() * 4, *uniforms, _lib.stream())
            if sized != "device":
                n = int(offsets[R].item())     # one 4-byte host read sizes the list
        if sized == "device":
            n = offsets[R:R + 1]
        return rays, t, counts, offsets, rays_d, n

    def _march_write(self, rays, t, K, counts, offsets, n, sh, k0=None, k1=None, index=False, jitter=None):
        """nerf_march_write of the list _march_count sized; with the same [k0, k1): nerf_slab_march_write.
        index: the nerf_rays_ write; the fourth result is then ray_c int32 [n], the row of each
        entry's ray in `rays`, and no SH row is formed. n a device element (_march_count sized="device", DESIGN.md
        §23): the list is allocated at its capacity R (k1 - k0), the worst case, and the write is told that capacity
        in place of the count: the kernel bounds its stores by the capacity and takes every position from counts and
        offsets, so entries [0, *n) are written exactly as in the host-sized call and nothing beyond them."""
        R, C, dev = rays.shape[0], rays.shape[1], rays.device
        f = dict(device=dev, dtype=torch.float32)
        if torch.is_tensor(n):
            n = R * ((K if k1 is None else int(k1)) - (0 if k0 is None else int(k0)))
        pts_c, z_c, dist_c = torch.empty(n, 3, **f), torch.empty(n, **f), torch.empty(n, **f)
        if index:
            last = torch.empty(n, device=dev, dtype=torch.int32)
            last_ptr = _lib.ptr(last, "ray_c", torch.int32)
        else:
            last = torch.empty(n, 16, **f) if sh else None
            last_ptr = _lib.ptr(last, "sh_c", allow_none=True)
        if n > 0 and jitter is not None:
            _lib.call("nerf_jitter_march_write", _lib.ptr(rays, "rays"), R, C, _lib.ptr(t, "t"), K, self._bmin,
                      self._bmax, self.resolution, self._bits(), _lib.ptr(counts, "counts", torch.int32),
                      _lib.ptr(offsets, "offsets", torch.int32), n, n, _lib.ptr(pts_c, "pts_c"), _lib.ptr(z_c, "z_c"),
                      _lib.ptr(dist_c, "dist_c"), None if index else last_ptr, last_ptr if index else None,
                      *self._jitter_args(jitter), _lib.stream())
        elif n > 0:
            name, slab = ("nerf_march_write", ()) if k0 is None else ("nerf_slab_march_write", (int(k0), int(k1)))
            _lib.call(name.replace("nerf_", "nerf_rays_") if index else name, _lib.ptr(rays, "rays"), R, C, _lib.ptr(t, "t"), K, *slab,
                      self._bmin, self._bmax, self.resolution, self._bits(), _lib.ptr(counts, "counts", torch.int32),
                      _lib.ptr(offsets, "offsets", torch.int32), n, n, _lib.ptr(pts_c, "pts_c"), _lib.ptr(z_c, "z_c"),
                      _lib.ptr(dist_c, "dist_c"), last_ptr, _lib.stream())
        return pts_c, z_c, dist_c, last

    @staticmethod
    def _ray_sh_records(rays):
        """nerf_ray_sh_records: the SH record [R, 40] of every packed ray row [R, 11]."""
        R = rays.shape[0]
        rec = torch.empty(R, 40, device=rays.device, dtype=torch.float32)
        if R > 0:
            _lib.call("nerf_ray_sh_records", _lib.ptr(rays, "rays"), R, rays.shape[1], _lib.ptr(rec, "sh_rec"),
                      _lib.stream())
        return rec

    def march(self, rays, K):
        """The samples of packed ray rows [R, 8 or 11] that lie in occupied cells, out of K lattice samples per
        ray at the coarse sampler's unperturbed depths: (counts int32 [R], offsets int32 [R + 1], pts_c [n, 3],
        z_c [n], dist_c [n], sh_c [n, 16] or None for rows without view directions). Ray r owns entries
        [offsets[r], offsets[r + 1]) in ascending depth; dist_c is the distance to the next lattice sample
        (1e10 after the last). One host read (the list's length) sizes the outputs."""
        rays, t, counts, offsets, _, n = self._march_count(rays, K)
        K = int(K)
        pts_c, z_c, dist_c, sh_c = self._march_write(rays, t, K, counts, offsets, n, rays.shape[1] == 11)
        self._last = (n, rays.shape[0] * K)
        return counts, offsets, pts_c, z_c, dist_c, sh_c
