"""CPU-only: training through the grid march (render march_grad=). The float64 restatement of the
packed compositing (march_ref.py) against the project's reference; the condition under which the atol of the kernel
test (test_gpu_march_bwd.py) hides nothing, asserted on that test's own inputs; nerf_packed_composite_bwd declared,
bound and exported, with its host argument checks; and the refusals of march_grad, word for word, on CPU tensors:
each is raised before anything could be launched."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import composite_ref as cr
import march_ref as mr

from test_forward_only_guards import field_modules, refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "nerf_packed_composite_bwd"
GRID = object()      # check_march_grad only asks whether march= was given
FORWARD_ONLY = "march is forward-only (call under torch.no_grad(); rays are not marched in training)"


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 300])
@pytest.mark.parametrize("white", [False, True])
def test_restatement_matches_the_dense_reference(S, white):
    """With dist the z difference and 1e10 for the last sample, one segment is one dense row of raw2outputs:
    float64 against float64 (composite_ref.composite_grad), outputs and gradient."""
    rng = np.random.default_rng(S)
    raw = (2.0 * rng.standard_normal((S, 4))).astype(np.float32)
    raw[0, 3] = abs(raw[0, 3]) + 0.1
    z = np.sort(rng.uniform(2.0, 6.0, S)).astype(np.float32)
    dist = np.concatenate([z[1:] - z[:-1], np.float32([1e10])]).astype(np.float32)
    d = rng.standard_normal(3).astype(np.float32)
    g = dict(g_rgb=rng.standard_normal((1, 3)).astype(np.float32), g_disp=rng.standard_normal(1).astype(np.float32),
             g_acc=rng.standard_normal(1).astype(np.float32), g_depth=rng.standard_normal(1).astype(np.float32),
             g_weights=rng.standard_normal(S).astype(np.float32))
    got, out = mr.composite_grad(raw, z, dist, d, None, white, g)
    want, ref = cr.composite_grad(raw[None], z[None], d[None], None, white, dict(g, g_weights=g["g_weights"][None]))
    # the packed distance is the float32 difference the dense reference forms in float64 from the same float32 z:
    # z[1:] - z[:-1] of two float32 values within a factor 2 of each other is exact in float32 (Sterbenz) unless it
    # underflows, and these lie in [2, 6]
    for a, b, name in zip(out, (ref[0], ref[1], ref[2], ref[3], ref[4]), ("rgb", "disp", "acc", "weights", "depth")):
        np.testing.assert_allclose(a.numpy().reshape(-1), b.numpy().reshape(-1), rtol=1e-12, atol=0, err_msg=name)
    np.testing.assert_allclose(got.numpy(), want[0].numpy(), rtol=1e-12, atol=1e-300)


def test_restatement_with_offsets_is_the_segments():
    """A list with offsets is its segments one by one; an empty segment takes no part."""
    d = mr.main_inputs()
    off = d["offsets"]
    which = {k: d[k] for k in mr.GRAD_NAMES}
    got, out = mr.reference(mr.GRAD_NAMES, True)
    for r in (1, 3, 7):
        b, e = off[r], off[r + 1]
        one = {k: (v[b:e] if k == "g_weights" else v[r:r + 1]) for k, v in which.items()}
        g1, o1 = mr.composite_grad(d["raw"][b:e], d["z"][b:e], d["dist"][b:e], d["rays_d"][r], None, True, one)
        assert np.array_equal(got[b:e], g1.numpy())
        assert np.array_equal(out[0][r], o1[0].numpy()[0]) and np.array_equal(out[3][b:e], o1[3].numpy())
    for r in (0, 8, 12):      # the empty rays
        assert off[r] == off[r + 1] and np.isnan(out[4][r]) and out[2][r] == 0 and (out[0][r] == 1).all()


# ---------------------------------------------------------------- the kernel test's inputs
def test_inputs_are_what_the_kernel_test_says():
    d = mr.main_inputs()
    off = d["offsets"]
    assert len(mr.LENGTHS) == 13 and mr.LENGTHS == (0, 1, 2, 63, 64, 65, 129, 300, 0, 4096, 4097, 8200, 0)
    assert tuple(np.diff(off)) == mr.LENGTHS and off[-1] == d["raw"].shape[0] == sum(mr.LENGTHS)
    for r, S in enumerate(mr.LENGTHS):
        z, dist = d["z"][off[r]:off[r + 1]], d["dist"][off[r]:off[r + 1]]
        if S:
            assert (np.diff(z) >= 0).all() and z.min() >= 2 and z.max() <= 6
            assert np.array_equal(dist[:-1], z[1:] - z[:-1]) and dist[-1] in (np.float32(1e10), np.float32(0.01))
            if r in mr.UNIFORM_SIGMA:
                s = d["raw"][off[r]:off[r + 1], 3]
                assert s.min() >= 0.3 and s.max() <= 0.6
    lasts = {float(d["dist"][off[r + 1] - 1]) for r, S in enumerate(mr.LENGTHS) if S}
    assert lasts == {float(np.float32(1e10)), float(np.float32(0.01))}


@pytest.mark.parametrize("white", [False, True])
def test_the_atol_of_the_kernel_test_hides_nothing(white):
    """test_gpu_march_bwd.py compares at rtol 1e-3, atol 1e-5. On its inputs with every upstream gradient together,
    every ray with a segment has max |graw_ref| >= 1e-3, a hundred times the atol, so no ray's gradient sits under
    the atol as a whole; and every such ray has acc > 0, so its depth and disp gradients are finite. (With g_depth or
    g_disp ALONE a one-sample ray has depth = z_0 whatever sigma is: its gradient is zero as a real number, and the
    sets with one gradient alone are covered by the list-wide maximum below.)"""
    d = mr.main_inputs()
    off = d["offsets"]
    live = np.diff(off) > 0
    g, out = mr.reference(mr.GRAD_NAMES, white)
    assert np.isfinite(g).all()
    worst = mr.ray_max(g, off)
    print("max |graw_ref| per ray:", " ".join(f"{v:.2e}" for v in worst))
    assert (worst[live] >= 1e-3).all()
    assert (out[2][live] > 0).all()       # acc
    for which in mr.GRAD_SETS[1:]:
        ga, _ = mr.reference(which, white)
        assert np.isfinite(ga).all() and np.abs(ga).max() >= 1e-3, which


def test_dead_rays_are_dead():
    """The first dead ray has no positive sigma (one exact 0 and one -0.0 among them): its reference gradient is
    exactly zero in every channel. The other's first sample is opaque."""
    d = mr.dead_inputs()
    off = d["offsets"]
    s0 = d["raw"][off[0]:off[1], 3]
    assert (s0 <= 0).all() and s0[5] == 0 and not np.signbit(s0[5]) and s0[66] == 0 and np.signbit(s0[66])
    for white in (False, True):
        g, out = mr.reference(mr.DEAD_GRADS, white, True)
        assert (g[off[0]:off[1]] == 0).all() and out[2][0] == 0
        assert out[3][off[2]] == 1.0 and out[2][2] >= 1.0          # w_0 = alpha_0 = 1
        assert np.isfinite(g).all() and mr.ray_max(g, off)[1] >= 1e-3


# ---------------------------------------------------------------- the entry
def test_entry_declared_bound_and_exported(nerf):
    import indoor_nerf_amd._lib as L
    txt = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert re.findall(r"^\s*int\s+(nerf_packed_\w+)\s*\(", txt, flags=re.M) == [ENTRY]
    assert ENTRY in L.exported_symbols() and len(L.SIGNATURES[ENTRY]) == 15
    lib = nerf.load_library()
    assert hasattr(lib, ENTRY), f"libnerfhip.so does not export {ENTRY}"
    assert lib.nerf_abi_version() == 12          # an additive entry
    assert os.path.exists(os.path.join(ROOT, "indoor-nerf_amd", "csrc", "march_bwd.hip"))


def test_entry_argument_checks(nerf):
    """Validation happens before any launch (no GPU is touched)."""
    import indoor_nerf_amd._lib as L
    nerf.load_library()
    fake = ctypes.c_void_p(1 << 20)

    def bwd(R=8, n=8, raw=fake, z=fake, dist=fake, off=fake, d=fake, graw=fake):
        L.call(ENTRY, raw, z, dist, off, d, R, n, 0, None, None, None, None, None, graw, None)

    with pytest.raises(RuntimeError, match="packed_composite_bwd: n_rays -1"):
        bwd(R=-1)
    with pytest.raises(RuntimeError, match="packed_composite_bwd: n_points -1"):
        bwd(n=-1)
    for name in ("raw", "z", "dist", "off", "d", "graw"):
        with pytest.raises(RuntimeError, match="packed_composite_bwd: null arg"):
            bwd(**{name: None})
    # no rays, or no points: nothing is launched and NULL buffers are accepted
    L.call(ENTRY, None, None, None, None, None, 0, 0, 0, None, None, None, None, None, None, None)
    L.call(ENTRY, None, None, None, None, None, 0, 8, 1, None, None, None, None, None, None, None)
    L.call(ENTRY, None, None, None, None, None, 8, 0, 1, None, None, None, None, None, None, None)


# ---------------------------------------------------------------- the keyword
def test_signature(nerf):
    p = inspect.signature(nerf.render_rays).parameters
    assert p["march_grad"].default is False and p["march"].default is None
    import importlib
    field, render = (importlib.import_module("indoor_nerf_amd." + m) for m in ("field", "render"))
    assert issubclass(field.PackedFieldFn, torch.autograd.Function)
    assert issubclass(render.MarchCompositeFn, torch.autograd.Function)


@pytest.mark.parametrize("prefix", ["render_rays", "render"])
def test_check_march_grad(prefix):
    check = sparse_field_check()
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            for march in (None, GRID):
                for stop in (None, (1e-3, 128)):
                    assert check(False, march, stop, prefix) is False      # the call without it: nothing to refuse
                for bad in (None, 1, 0, "yes", 1.0, np.True_):
                    assert refusal(check, bad, march, None, prefix) == f"{prefix}: march_grad must be a bool, got {bad!r}"
            assert check(True, GRID, None, prefix) is True
            assert refusal(check, True, None, None, prefix) == \
                f"{prefix}: march_grad=True needs march= (the gradients are those of a grid march)"
            assert refusal(check, True, GRID, (1e-3, 128), prefix) == \
                (f"{prefix}: march_grad=True does not combine with march_stop= (the slabs' carried state has no "
                 "backward)")


def sparse_field_check():
    from indoor_nerf_amd import sparse_field
    return sparse_field.check_march_grad


def _cpu_call(nerf):
    box = (torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]))
    grid = nerf.OccupancyGrid(box, resolution=2, device="cpu")
    emb, net, _, _ = field_modules()
    return grid, dict(network_fn=net, network_query_fn=None, N_samples=4, embed_fn=emb)


def test_render_rays_and_render_refuse_before_any_launch(nerf):
    """Both entry points check march_grad on their own keywords, after the forward-only keywords' checks and before
    they touch the rays: the refusals fire on CPU tensors, under gradients or not."""
    grid, common = _cpu_call(nerf)
    rays = torch.zeros(4, 11)
    calls = ((nerf.render_rays, (rays,), "render_rays"), (nerf.render, (2, 2, None), "render"))
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            for fn, args, prefix in calls:
                assert refusal(fn, *args, march_grad=True, **common) == \
                    f"{prefix}: march_grad=True needs march= (the gradients are those of a grid march)"
                assert refusal(fn, *args, march_grad=1, march=grid, **common) == \
                    f"{prefix}: march_grad must be a bool, got 1"
                assert refusal(fn, *args, march_grad=True, march=grid, march_stop=1e-3, **common) == \
                    (f"{prefix}: march_grad=True does not combine with march_stop= (the slabs' carried state has no "
                     "backward)")


def test_forward_only_refusals_are_unchanged(nerf):
    """march= without march_grad under gradients refuses with the sentence it had, at both levels, and so does
    march_grad=False; the forward-only companions refuse first with their own sentences; render refuses retraw."""
    from indoor_nerf_amd import sparse_field
    grid, common = _cpu_call(nerf)
    rays = torch.zeros(4, 11)
    with torch.enable_grad():
        for over in ({}, dict(march_grad=False)):
            assert refusal(nerf.render_rays, rays, march=grid, **over, **common) == f"render_rays: {FORWARD_ONLY}"
        for kw, what, reason in ((dict(march_sh="rays"), "march_sh", "the backward reads per-point SH rows"),
                                 (dict(mlp_precision="bf16"), "mlp_precision",
                                  "the backward recomputes the forward in fp32"),
                                 (dict(table_precision="fp16"), "table_precision",
                                  "the backward scatters into the fp32 tables"),
                                 (dict(mlp_precision="bf16", feature_precision="bf16"), "mlp_precision",
                                  "the backward recomputes the forward in fp32"),
                                 (dict(march_sizes="device", march_sh="rays", mlp_precision="bf16",
                                       feature_precision="bf16"), "march_sh", "the backward reads per-point SH rows")):
            for fn, args, prefix in ((nerf.render_rays, (rays,), "render_rays"), (nerf.render, (2, 2, None), "render")):
                assert refusal(fn, *args, march=grid, march_grad=True, **kw, **common) == \
                    f"{prefix}: {what} is forward-only (call under torch.no_grad(); {reason})"
        o, d = torch.zeros(4, 3), torch.tensor([[0.0, 0.0, -1.0]]).repeat(4, 1)
        assert refusal(nerf.render, 2, 2, np.eye(3), rays=(o, d), ndc=False, march=grid, march_grad=True,
                       ray_bounds=grid, **common) == \
            "render: ray_bounds is forward-only (call under torch.no_grad(); rays are not bounded in training)"
        # the field call: a list without the permission refuses as before; the permission travels on the list
        emb, net, _, sh = field_modules()
        pts, dirs = torch.zeros(5, 3), torch.zeros(2, 3)
        req = sparse_field.FieldRequest(march=sparse_field.MarchList(torch.zeros(5, 16), 1000))
        assert refusal(sparse_field.run_network_packed, pts, dirs, net, emb, sh, req) == \
            "march: forward-only (call under torch.no_grad(); rays are not marched in training)"
    assert sparse_field.NOT_IN_TRAINING["march"] == "rays are not marched in training"
    assert sparse_field.MarchList(torch.zeros(5, 16), 1000).grad is False
    assert sparse_field.MarchList(torch.zeros(5, 16), 1000, grad=True).grad is True
    assert refusal(sparse_field.MarchList, None, 1000, ray_c=torch.zeros(5, dtype=torch.int32),
                   sh_rec=torch.zeros(2, 40), grad=True) == \
        "march: a list under gradients carries SH rows (the backward reads per-point SH rows)"
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            assert refusal(nerf.render, 2, 2, np.eye(3), rays=(o, d), ndc=False, march=grid, march_grad=True,
                           retraw=True, N_samples=4) == \
                ("render: retraw is not available with march (the packed entries of several chunks do not "
                 "concatenate; call render_rays on one chunk)")


def test_graphed_step_refuses_at_construction(nerf):
    from indoor_nerf_amd.graphs import GraphedTrainStep
    grid, common = _cpu_call(nerf)
    kw = dict(common, march=grid, march_grad=True)
    assert refusal(GraphedTrainStep, None, None, kw, None, None) == \
        ("GraphedTrainStep: march_grad cannot be captured (the list length of a grid march is read on the host; use "
         "train_step)")
