"""nerf_packed_composite_bwd (csrc/march_bwd.hip) against the float64 reference of tests/march_ref.py
(needs an MI355X).

One wave handles one ray in tiles of 64 entries; the carries of 64 tiles fit one register, and a longer segment is
walked in super-blocks of 64 tiles. The list (march_ref.main_inputs) has 13 rays, which is not a multiple of the four
of a block, with segments of 0, 1, 2, 63, 64, 65, 129, 300, 0, 4096, 4097, 8200 and 0 entries: the empty rays first,
in the middle and last, 4097 one tile past a full register, 8200 three super-blocks with a ragged tail. Every
gradient buffer starts as a sentinel, so an entry the kernel leaves out, or writes where it should not, shows.

Bar: the project's bar for the compositing backward, rtol 1e-3 and atol 1e-5 (test_gpu_composite_widths.py), with
every upstream gradient together and each alone, white background on and off. test_march_grad_cpu.py asserts on
these inputs that no ray's reference gradient hides under the atol."""
import numpy as np
import pytest
import torch

import march_ref as mr

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _dev(a, gpu):
    return None if a is None else torch.tensor(np.asarray(a)).to(gpu)      # a copy: the cached inputs are read-only


def _backward(gpu, d, white, which, n_points=None, rows=None):
    """The entry with the upstream gradients named in `which` (the rest NULL) on a sentinel-filled graw of `rows`
    rows, told that the list has n_points entries."""
    from indoor_nerf_amd import _lib
    n = d["raw"].shape[0]
    n_points = n if n_points is None else n_points
    raw, z, dist, off, rd = (_dev(d[k], gpu) for k in ("raw", "z", "dist", "offsets", "rays_d"))
    gs = [_dev(d[k], gpu) if k in which else None for k in mr.GRAD_NAMES]
    graw = torch.full((n if rows is None else rows, 4), SENTINEL, device=gpu, dtype=torch.float32)
    _lib.call("nerf_packed_composite_bwd", _lib.ptr(raw), _lib.ptr(z), _lib.ptr(dist), _lib.ptr(off, "off", torch.int32),
              _lib.ptr(rd), off.shape[0] - 1, n_points, int(white), *[_lib.ptr(g, allow_none=True) for g in gs],
              _lib.ptr(graw), _lib.stream())
    torch.cuda.synchronize()
    return graw.cpu().numpy()


def _check_grad(got, want, tag):
    err = np.abs(got.astype(np.float64) - want)
    print(f"{tag}: worst err / bar {float(np.nanmax(err / (1e-5 + 1e-3 * np.abs(want)))):.3f}, max |graw| "
          f"{float(np.abs(want).max()):.3e}")
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-5, err_msg=tag)


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("which", mr.GRAD_SETS, ids=["all"] + [s[0] for s in mr.GRAD_SETS[1:]])
def test_backward_vs_fp64(nerf, gpu, which, white):
    want, _ = mr.reference(which, white)
    got = _backward(gpu, mr.main_inputs(), white, which)
    off = mr.main_inputs()["offsets"]
    for r, S in enumerate(mr.LENGTHS):
        if S:
            e = np.abs(got[off[r]:off[r + 1]].astype(np.float64) - want[off[r]:off[r + 1]])
            bar = 1e-5 + 1e-3 * np.abs(want[off[r]:off[r + 1]])
            print(f"  S={S}: worst err / bar {float((e / bar).max()):.3f}")
    _check_grad(got, want, "+".join(which))


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
def test_dead_rays(nerf, gpu, white):
    """A ray without a positive sigma (an exact 0 and a -0.0 among them): every sigma gradient is exactly 0 (and,
    its weights being 0, every colour gradient too). A ray whose first sample is opaque: the bar, and finite."""
    d = mr.dead_inputs()
    off = d["offsets"]
    want, _ = mr.reference(mr.DEAD_GRADS, white, True)
    got = _backward(gpu, d, white, mr.DEAD_GRADS)
    assert (got[off[0]:off[1], 3] == 0).all() and (got[off[0]:off[1]] == 0).all()
    assert np.isfinite(got).all()
    _check_grad(got, want, "dead")


def test_repeatable_and_no_stray_writes(nerf, gpu):
    """Two launches on the same inputs give equal bits; rows of d_graw outside every segment keep the sentinel: in
    front of the first segment (offsets[0] > 0), in the capacity tail between offsets[R] and n_points, and beyond
    n_points."""
    d = mr.main_inputs()
    a = _backward(gpu, d, True, mr.GRAD_NAMES)
    b = _backward(gpu, d, True, mr.GRAD_NAMES)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert (a != SENTINEL).all()          # every row of this list lies in a segment
    # a sub-list: rays of 65, 129 and 0 entries placed at rows [7, 201) of a list told to have 221 entries, in a
    # buffer of 237 rows
    off = d["offsets"]
    lo, hi = int(off[5]), int(off[7])
    pad = 7
    sub = {k: np.concatenate([np.zeros((pad,) + d[k].shape[1:], np.float32), d[k][lo:hi],
                              np.zeros((36,) + d[k].shape[1:], np.float32)]) for k in ("raw", "z", "dist", "g_weights")}
    sub["offsets"] = (np.array([off[5], off[6], off[7], off[7]]) - lo + pad).astype(np.int32)
    for k in ("rays_d", "g_rgb", "g_disp", "g_acc", "g_depth"):
        sub[k] = np.concatenate([d[k][5:7], d[k][:1]])
    n_seg = hi - lo
    got = _backward(gpu, sub, True, mr.GRAD_NAMES, n_points=pad + n_seg + 20, rows=pad + n_seg + 36)
    assert (got[:pad] == SENTINEL).all() and (got[pad + n_seg:] == SENTINEL).all()
    want, _ = mr.reference(mr.GRAD_NAMES, True)
    _check_grad(got[pad:pad + n_seg], want[lo:hi], "sub-list")
    assert np.array_equal(got[pad:pad + n_seg].view(np.int32), a[lo:hi].view(np.int32))     # the same rays, moved
    # offsets past the list are clamped into it: the last ray is cut at n_points, nothing is written behind it
    cut = dict(sub, offsets=(sub["offsets"] + np.array([0, 0, 1000, 2000])).astype(np.int32))
    got = _backward(gpu, cut, True, ("g_rgb", "g_acc"), n_points=pad + 100, rows=pad + n_seg + 36)
    assert (got[:pad] == SENTINEL).all() and (got[pad + 100:] == SENTINEL).all() and (got[pad:pad + 100] != SENTINEL).all()


@pytest.mark.parametrize("K", [192, 300])
def test_against_the_dense_kernel(nerf, gpu, K):
    """A packed list scattered into [R, K, 4] with all-zero rows at the skipped samples (weight 0 exactly) is the dense
    compositing's input: nerf_composite_bwd on it agrees with the packed entry at the kept rows within the same bar.
    No claim of bit equality is made (the fp64 scans associate differently); the count is printed."""
    from indoor_nerf_amd import _lib
    rng = np.random.default_rng(K)
    R = 9
    keep = rng.random((R, K)) < 0.4
    keep[0] = False                       # an empty ray
    keep[1] = True                        # every sample kept
    keep[2, :] = False
    keep[2, K - 1] = True                 # only the last lattice sample: dist 1e10
    z = np.sort(rng.uniform(2.0, 6.0, (R, K)), -1).astype(np.float32)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((R, 1), 1e10, np.float32)], -1).astype(np.float32)
    raw = (2.0 * rng.standard_normal((R, K, 4))).astype(np.float32)
    raw[:, ::5, 3] = rng.uniform(0.3, 0.6, raw[:, ::5, 3].shape).astype(np.float32)
    raw[2, K - 1, 3] = 0.5                # ... with a positive sigma, so that the ray's depth is a number
    raw[~keep] = 0.0
    g_w =rng.standard_normal((R, K)).astype(np.float32)
    counts = keep.sum(-1)
    d = dict(raw=raw[keep], z=z[keep], dist=dist[keep], offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
             rays_d=rng.standard_normal((R, 3)).astype(np.float32), g_weights=g_w[keep])
    up = mr._upstream(rng, R, 1)
    live = counts > 0                     # a ray without samples has NaN depth in the dense kernel: no depth gradient
    for k in ("g_rgb", "g_disp", "g_acc", "g_depth"):
        d[k] = up[k]
    d["g_depth"] = np.where(live, d["g_depth"], 0).astype(np.float32)
    d["g_disp"] = np.where(live, d["g_disp"], 0).astype(np.float32)
    got = _backward(gpu, d, True, mr.GRAD_NAMES)
    t = lambda a: torch.tensor(a).to(gpu)  # noqa: E731
    graw = torch.full((R, K, 4), SENTINEL, device=gpu, dtype=torch.float32)
    raw_d, z_d, rd_d = t(raw), t(z), t(d["rays_d"])
    gs = dict(g_rgb=t(d["g_rgb"]), g_disp=t(d["g_disp"]), g_acc=t(d["g_acc"]), g_weights=t(g_w), g_depth=t(d["g_depth"]))
    _lib.call("nerf_composite_bwd", _lib.ptr(raw_d), 4, _lib.ptr(z_d), _lib.ptr(rd_d), None, R, K, 1,
              _lib.ptr(gs["g_rgb"]), _lib.ptr(gs["g_disp"]), _lib.ptr(gs["g_acc"]), _lib.ptr(gs["g_weights"]),
              _lib.ptr(gs["g_depth"]), None, None, _lib.ptr(graw), _lib.stream())
    torch.cuda.synchronize()
    dense = graw.cpu().numpy()[keep]
    print(f"K={K}: {int((dense.view(np.int32) != got.view(np.int32)).sum())} of {dense.size} entries not bit-identical")
    _check_grad(got, dense.astype(np.float64), f"dense K={K}")
    want, _ = mr.composite_grad(d["raw"], d["z"], d["dist"], d["rays_d"], d["offsets"], True,
                                {k: d[k] for k in mr.GRAD_NAMES})
    _check_grad(got, want.numpy(), f"fp64 K={K}")
