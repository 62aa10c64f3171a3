"""CPU-only: the jittered grid march (render march_jitter=). The two entries of csrc/march.hip are
declared in include/nerf_hip.h, bound in _lib with the declared argument types and exported by the built library
(ABI 12, additive); their argument checks run on the host; the keyword's refusals are raised, each by its
sentence, before anything is launched (the tensors live on the CPU here); and without the keyword perturb > 0 is
refused as it was."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_forward_only_guards import field_modules, refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, WRITE = "nerf_jitter_march_count", "nerf_jitter_march_write"
GRID = object()      # check_march_jitter only asks whether march= was given
UNIFORMS = ["const float* d_u", "uint64_t seed", "uint64_t offset", "const uint64_t* d_rng"]
PERTURB = "render_rays: march needs perturb == 0 (the lattice is the unperturbed coarse sampling)"


def declared_args(txt, name):
    body = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", txt, flags=re.M | re.S).group(1)
    return [" ".join(a.split()) for a in body.split(",")]


def ctype_of(arg):
    """The ctypes type _lib binds for a declared argument."""
    import indoor_nerf_amd._lib as L
    kind = arg.rsplit(" ", 1)[0]
    if kind == "const float*" and arg.rsplit(" ", 1)[1] in ("bbox_min", "bbox_max"):
        return L.c_f32p
    if kind.endswith("*"):
        return L.c_vp
    return {"int": L.c_int, "int64_t": L.c_i64, "uint64_t": L.c_u64, "size_t": ctypes.c_size_t}[kind]


# ---------------------------------------------------------------- the entries
def test_entries_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert sorted(re.findall(r"^\s*int\s+(nerf_jitter_\w+)\s*\(", txt, flags=re.M)) == [COUNT, WRITE]
    count, write = declared_args(txt, COUNT), declared_args(txt, WRITE)
    # the plain entries' arguments, then (the write: d_ray_c and) the sampler's four, then the stream
    plain_count, plain_write = declared_args(txt, "nerf_march_count"), declared_args(txt, "nerf_march_write")
    assert count == plain_count[:-1] + UNIFORMS + ["void* stream"]
    assert write == plain_write[:-1] + ["int32_t* d_ray_c"] + UNIFORMS + ["void* stream"]
    for name, args in ((COUNT, count), (WRITE, write)):
        assert name in L.exported_symbols()
        assert L.SIGNATURES[name] == [ctype_of(a) for a in args], name
    assert L.SIGNATURES[COUNT][:-5] == L.SIGNATURES["nerf_march_count"][:-1]
    assert L.SIGNATURES[WRITE][:-6] == L.SIGNATURES["nerf_march_write"][:-1]
    lib = nerf.load_library()
    for name in (COUNT, WRITE):
        assert hasattr(lib, name), f"libnerfhip.so does not export {name}"
        assert getattr(lib, name).argtypes == L.SIGNATURES[name]
    assert lib.nerf_abi_version() == 12          # additive entries


def _drivers():
    import indoor_nerf_amd._lib as L
    lo, hi = L.host_f32([-1, -1, -1]), L.host_f32([1, 1, 1])
    fake = ctypes.c_void_p(1 << 20)

    def count(R=8, C=11, K=64, p=fake, ws=fake, ws_bytes=4, u=None, rng=None):
        L.call(COUNT, p, R, C, p, K, lo, hi, 4, p, p, p, p, ws, ws_bytes, u, 5, 7, rng, None)

    def write(R=8, C=11, K=64, p=fake, n=8, cap=8, sh=fake, ray=None, u=None, rng=None):
        L.call(WRITE, p, R, C, p, K, lo, hi, 4, p, p, p, n, cap, p, p, p, sh, ray, u, 5, 7, rng, None)

    return count, write, fake, lo, hi


def test_argument_checks(nerf):
    """Validation happens before any launch (no GPU is touched): the checks of nerf_march_count and nerf_march_write,
    and exactly one of the SH rows and the ray indices."""
    nerf.load_library()
    count, write, fake, _, _ = _drivers()
    for fn in (count, write):
        for K in (0, 4097):
            with pytest.raises(RuntimeError, match=f"jitter_march_.*: n_samples {K} \\(1..4096\\)"):
                fn(K=K)
        with pytest.raises(RuntimeError, match="jitter_march_.*: ray rows of 9 columns \\(8 or 11\\)"):
            fn(C=9)
        with pytest.raises(RuntimeError, match="n_rays -1"):
            fn(R=-1)
        with pytest.raises(RuntimeError, match="use a smaller chunk"):
            fn(R=1 << 19, K=4096)
        with pytest.raises(RuntimeError, match="null arg"):
            fn(p=None)
        with pytest.raises(RuntimeError, match="pair must be 8-B aligned"):
            fn(rng=ctypes.c_void_p((1 << 20) + 4))
    with pytest.raises(RuntimeError, match="workspace 4 B < 8 B"):
        count(R=4097)
    one = "jitter_march_write: exactly one of sh_c \\(SH rows\\) and ray_c \\(ray indices\\) must be given"
    with pytest.raises(RuntimeError, match=one):
        write(sh=fake, ray=fake)
    with pytest.raises(RuntimeError, match=one):
        write(sh=None, ray=None)
    with pytest.raises(RuntimeError, match=one):
        write(sh=None, ray=None, n=0, cap=0)           # also for an empty list: the call names its kind of list
    with pytest.raises(RuntimeError, match="jitter_march_write: capacity 7 below the count 8"):
        write(cap=7)
    with pytest.raises(RuntimeError, match="count 513 of 512 lattice samples"):
        write(n=513, cap=513)
    with pytest.raises(RuntimeError, match="11 columns"):
        write(C=8)                                      # SH rows of rays without view directions
    with pytest.raises(RuntimeError, match="null arg"):
        write(C=8, sh=None, ray=fake, p=None)           # rows of 8 columns pass the checks with a ray index


def test_empty_calls_accept_null_buffers(nerf):
    """No rays: nothing is launched and NULL buffers are accepted, neither list among them; an empty list to write
    launches nothing either."""
    import indoor_nerf_amd._lib as L
    nerf.load_library()
    _, _, fake, lo, hi = _drivers()
    for C in (8, 11):
        L.call(COUNT, None, 0, C, None, 64, lo, hi, 4, None, None, None, None, None, 0, None, 0, 0, None, None)
        L.call(WRITE, None, 0, C, None, 64, lo, hi, 4, None, None, None, 0, 0, None, None, None, None, None, None, 0, 0,
               None, None)
        L.call(WRITE, None, 8, C, None, 64, lo, hi, 4, None, None, None, 0, 0, None, None, None, None, fake, None, 0, 0,
               None, None)


# ---------------------------------------------------------------- the keyword
def test_signatures(nerf):
    from indoor_nerf_amd import model, occupancy, sparse_field
    assert inspect.signature(nerf.render_rays).parameters["march_jitter"].default is False
    assert list(inspect.signature(sparse_field.check_march_jitter).parameters) == \
        ["value", "march", "stop", "march_sizes", "prefix"]
    for fn in (occupancy.OccupancyGrid._march_count, occupancy.OccupancyGrid._march_write):
        assert inspect.signature(fn).parameters["jitter"].default is None
    # nothing new through field_options; the training path takes the keyword in its render keywords
    assert "march_jitter" not in inspect.signature(sparse_field.field_options).parameters
    assert sparse_field.FieldOptions._fields == ("bf16", "half", "packed", "by_ray", "stop")
    for name, fn in inspect.getmembers(model, inspect.isfunction):
        assert "march_jitter" not in inspect.signature(fn).parameters, name


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_check_march_jitter(prefix):
    from indoor_nerf_amd import sparse_field
    check = sparse_field.check_march_jitter
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            for march in (None, GRID):
                for stop in (None, (1e-3, 128)):
                    for sizes in (None, "host", "device"):
                        assert check(False, march, stop, sizes, prefix) is False      # the call without it
                for bad in (None, 1, 0, "yes", 1.0, np.True_):
                    assert refusal(check, bad, march, None, None, prefix) == \
                        f"{prefix}: march_jitter must be a bool, got {bad!r}"
            assert check(True, GRID, None, None, prefix) is True and check(True, GRID, None, "host", prefix) is True
            assert refusal(check, True, None, None, None, prefix) == \
                f"{prefix}: march_jitter=True needs march= (the jitter is that of a grid march's lattice)"
            assert refusal(check, True, GRID, (1e-3, 128), None, prefix) == \
                (f"{prefix}: march_jitter=True does not combine with march_stop= (the slab walk has no jittered "
                 "entries)")
            assert refusal(check, True, GRID, None, "device", prefix) == \
                (f"{prefix}: march_jitter=True does not combine with march_sizes='device' (the device-sized path has "
                 "no jittered entries)")


def _cpu_call(nerf):
    box = (torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]))
    grid = nerf.OccupancyGrid(box, resolution=2, device="cpu")
    emb, net, _, _ = field_modules()
    return grid, dict(network_fn=net, network_query_fn=None, N_samples=4, embed_fn=emb)


def test_render_rays_and_render_refuse_before_any_launch(nerf):
    grid, common = _cpu_call(nerf)
    rays = torch.zeros(4, 11)
    calls = ((nerf.render_rays, (rays,), "render_rays"), (nerf.render, (2, 2, None), "render"))
    device = dict(march_sizes="device", march_sh="rays", mlp_precision="bf16", feature_precision="bf16")
    for fn, args, prefix in calls:
        for grad in (torch.no_grad, torch.enable_grad):
            with grad():
                assert refusal(fn, *args, march_jitter=True, **common) == \
                    f"{prefix}: march_jitter=True needs march= (the jitter is that of a grid march's lattice)"
                for bad in (1, None, "yes"):
                    assert refusal(fn, *args, march_jitter=bad, march=grid, **common) == \
                        f"{prefix}: march_jitter must be a bool, got {bad!r}"
                assert refusal(fn, *args, march_jitter=True, march=grid, march_stop=1e-3, **common) == \
                    (f"{prefix}: march_jitter=True does not combine with march_stop= (the slab walk has no jittered "
                     "entries)")
        with torch.no_grad():
            assert refusal(fn, *args, march_jitter=True, march=grid, **device, **common) == \
                (f"{prefix}: march_jitter=True does not combine with march_sizes='device' (the device-sized path has "
                 "no jittered entries)")
    o, d = torch.zeros(4, 3), torch.tensor([[0.0, 0.0, -1.0]]).repeat(4, 1)
    with torch.no_grad():
        for perturb in (0.0, 1.0):
            assert refusal(nerf.render, 2, 2, np.eye(3), rays=(o, d), ndc=False, march=grid, march_jitter=True,
                           ray_bounds=grid, perturb=perturb, **common) == \
                ("render: march_jitter=True does not combine with ray_bounds= (a bounded ray's lattice has no jittered "
                 "entries)")


def test_the_other_refusals_are_unchanged(nerf):
    """Without the keyword, and with march_jitter=False, perturb > 0 is refused by the sentence it had; with the
    keyword lindisp stays refused, gradients need march_grad, and a captured step refuses the march."""
    from indoor_nerf_amd.graphs import GraphedTrainStep
    grid, common = _cpu_call(nerf)
    rays = torch.zeros(4, 11)
    with torch.no_grad():
        for over in ({}, dict(march_jitter=False)):
            assert refusal(nerf.render_rays, rays, march=grid, perturb=1.0, **over, **common) == PERTURB
        for perturb in (0.0, 1.0):
            assert refusal(nerf.render_rays, rays, march=grid, march_jitter=True, perturb=perturb, lindisp=True,
                           **common) == "render_rays: march needs lindisp=False (the lattice is linear in depth)"
            assert "march needs raw_noise_std == 0" in refusal(nerf.render_rays, rays, march=grid, march_jitter=True,
                                                               perturb=perturb, raw_noise_std=1.0, **common)
    with torch.enable_grad():
        assert refusal(nerf.render_rays, rays, march=grid, march_jitter=True, perturb=1.0, **common) == \
            "render_rays: march is forward-only (call under torch.no_grad(); rays are not marched in training)"
        assert refusal(nerf.render_rays, rays, march=grid, march_jitter=True, march_grad=True, perturb=1.0,
                       march_sh="rays", **common) == \
            "render_rays: march_sh is forward-only (call under torch.no_grad(); the backward reads per-point SH rows)"
    kw = dict(common, march=grid, march_grad=True, march_jitter=True, perturb=1.0)
    assert refusal(GraphedTrainStep, None, None, kw, None, None) == \
        ("GraphedTrainStep: march_grad cannot be captured (the list length of a grid march is read on the host; use "
         "train_step)")
