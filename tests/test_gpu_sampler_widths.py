"""nerf_sample_fine / nerf_sample_pdf / nerf_composite_sample_fine (csrc/sampling.hip) with given uniforms against the
float64 inverse CDF of tests/composite_ref.py (needs an MI355X).

build_cdf hands each lane per = ceil((S - 2) / 64) contiguous weights: S = 3 .. 256 at both edges of per = 1 .. 4.
sample_fine_ray sorts the N importance samples in registers (P2 <= 128: one or two elements per lane), in LDS, or,
where S + P2 > 1024 (S = 256, N = 700), takes the rank sort. The weights are uniform in [0.1, 1], so every bin
carries at least 6.5e-4 of the mass (test_composite_ref_cpu.py) and sample_pdf's `denom < 1e-5 -> 1` jump cannot fire:
every sample must meet isclose(rtol 1e-5, atol 1e-5) against float64 (the float32 oracle stays within 7.1e-6), the
merged depths must be torch.sort(cat(z, samples)) bit for bit, z_std within rtol 1e-5 of the float64 reference, and
the points o + d * z as in test_sample_fine_merge_vs_torch_sort. Outputs start as NaN.
"""
import numpy as np
import pytest
import torch

import composite_ref as cr

pytestmark = pytest.mark.gpu

R = 9


def _dev(a, gpu):
    return None if a is None else torch.tensor(np.asarray(a)).to(gpu)      # a copy: the cached inputs are read-only


def _nan(shape, gpu):
    return torch.full(shape, float("nan"), device=gpu, dtype=torch.float32)


def _check_samples(got, want, tag):
    got = got.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"{tag}: worst sample err {float(err.max()):.3e}, worst err / bar "
          f"{float((err / (1e-5 + 1e-5 * np.abs(want))).max()):.3f}")
    bad = ~np.isclose(got, want, rtol=1e-5, atol=1e-5)
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} samples off the float64 inverse CDF"


def _check_merge(rays, z, samples, z_fine, pts, z_std, want_std, tag):
    want = torch.sort(torch.cat([z, samples], -1), -1).values
    assert torch.equal(z_fine, want), f"{tag}: merged depths"
    want_pts = rays[:, None, 0:3] + rays[:, None, 3:6] * want[..., None]
    torch.testing.assert_close(pts, want_pts, rtol=1e-6, atol=1e-6)
    got_std = z_std.cpu().numpy()
    print(f"{tag}: z_std worst rel err {float(np.max(np.abs(got_std - want_std) / np.maximum(want_std, 1e-30))):.3e}")
    np.testing.assert_allclose(got_std, want_std, rtol=1e-5, err_msg=f"{tag}: z_std")


@pytest.mark.parametrize("S,N", cr.sampler_cases(), ids=[f"S{S}-N{N}-{cr.sort_path(S, N)}" for S, N in cr.sampler_cases()])
def test_sample_fine_vs_fp64(nerf, gpu, S, N):
    from indoor_nerf_amd import _lib
    d = cr.sampler_inputs(S, N)
    want, _, want_std = (t.numpy() for t in cr.sample_fine(d["z"], d["w"], d["u"]))
    rays, z, w, u = (_dev(d[k], gpu) for k in ("rays", "z", "w", "u"))
    z_fine, pts, z_std, samples = _nan((R, S + N), gpu), _nan((R, S + N, 3), gpu), _nan((R,), gpu), _nan((R, N), gpu)
    _lib.call("nerf_sample_fine", _lib.ptr(rays), 11, _lib.ptr(z), _lib.ptr(w), R, S, N, 0, None, _lib.ptr(u), 0, 0, None,
              _lib.ptr(z_fine), _lib.ptr(pts), _lib.ptr(z_std), _lib.ptr(samples), _lib.stream())
    torch.cuda.synchronize()
    _check_samples(samples, want, "sample_fine")
    _check_merge(rays, z, samples, z_fine, pts, z_std, want_std, "sample_fine")
    # the stand-alone sampler on the same bins and weights
    bins = (0.5 * (z[:, 1:] + z[:, :-1])).contiguous()
    inner = w[:, 1:-1].contiguous()
    alone = _nan((R, N), gpu)
    _lib.call("nerf_sample_pdf", _lib.ptr(bins), S - 1, _lib.ptr(inner), S - 2, R, S - 1, N, 0, None, _lib.ptr(u), 0, 0,
              None, _lib.ptr(alone), _lib.stream())
    torch.cuda.synchronize()
    _check_samples(alone, want, "sample_pdf")


@pytest.mark.parametrize("S,N", cr.FUSED_CASES)
def test_composite_sample_fine_vs_fp64_chain(nerf, gpu, S, N):
    """The coarse pass's one launch against the float64 chain: composite, then sample_pdf on weights[1:-1] (the
    medium is thin, so every bin of that pdf carries mass: composite_ref.fused_inputs)."""
    from indoor_nerf_amd import _lib
    d = cr.fused_inputs(S, N)
    comp = cr.composite(d["raw"], d["z"], d["rays_d"], None, True)
    want, _, want_std = (t.numpy() for t in cr.sample_fine(d["z"], comp[3], d["u"]))
    raw, z, rd, rays, u = (_dev(d[k], gpu) for k in ("raw", "z", "rays_d", "rays", "u"))
    shapes = dict(rgb=(R, 3), disp=(R,), acc=(R,), weights=(R, S), depth=(R,), entropy=(R,))
    out = {n: _nan(s, gpu) for n, s in shapes.items()}
    z_fine, pts, z_std, samples = _nan((R, S + N), gpu), _nan((R, S + N, 3), gpu), _nan((R,), gpu), _nan((R, N), gpu)
    _lib.call("nerf_composite_sample_fine", _lib.ptr(raw), 4, _lib.ptr(z), _lib.ptr(rd), None, R, S, 1,
              *[_lib.ptr(out[n]) for n in shapes], None, _lib.ptr(rays), 11, N, 0, None, _lib.ptr(u), 0, 0, None,
              _lib.ptr(z_fine), _lib.ptr(pts), _lib.ptr(z_std), _lib.ptr(samples), None, None, None, None, _lib.stream())
    torch.cuda.synchronize()
    for n, ref in zip(shapes, comp):
        np.testing.assert_allclose(out[n].cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-5, err_msg=n)
    _check_samples(samples, want, "fused")
    _check_merge(rays, z, samples, z_fine, pts, z_std, want_std, "fused")
