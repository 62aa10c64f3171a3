"""The float64 references of tests/composite_ref.py against the golden vectors and the float32 oracle, and the
properties of the seeded cases that test_gpu_composite_widths.py and test_gpu_sampler_widths.py rely on, asserted on
the references alone (no GPU)."""
import numpy as np
import torch

import composite_ref as cr
from test_gpu_parity import _check_pdf_samples

NAMES = ["rgb", "disp", "acc", "weights", "depth", "entropy"]


def test_reference_reproduces_composite_golden(golden, oracle):
    """f7_composite (the reference's own raw2outputs, float32) at the bars of test_oracle_golden.test_composite."""
    g = golden("f7_composite")
    for S in (64, 192):
        for white in (0, 1):
            tag = f"S{S}_w{white}"
            out = cr.composite(g[f"raw_{tag}"], g[f"z_{tag}"], g[f"d_{tag}"], None, bool(white))
            for n, v in zip(NAMES, out):
                np.testing.assert_allclose(v.numpy(), g[f"{n}_{tag}"], rtol=1e-5, atol=1e-6, equal_nan=True,
                                           err_msg=f"{n} {tag}")
            grads = dict(g_rgb=g[f"g_rgb_{tag}"], g_disp=g[f"g_disp_{tag}"], g_acc=g[f"g_acc_{tag}"],
                         g_weights=g[f"g_w_{tag}"], g_depth=g[f"g_depth_{tag}"], g_entropy=g[f"g_ent_{tag}"])
            graw, _ = cr.composite_grad(g[f"braw_{tag}"], g[f"bz_{tag}"], g[f"bd_{tag}"], None, bool(white), grads)
            np.testing.assert_allclose(graw.numpy(), g[f"draw_{tag}"], rtol=1e-4, atol=1e-6, err_msg=f"grad {tag}")
    noise = oracle.pytest_uniforms(g["raw_noise"].shape[:2]) * 1.0
    out = cr.composite(g["raw_noise"], g["z_noise"], g["d_noise"], noise, False)
    for n, v in zip(NAMES, out):
        np.testing.assert_allclose(v.numpy(), g[f"{n}_noise"], rtol=1e-5, atol=1e-6, err_msg=n)


def test_reference_reproduces_pdf_golden(golden, oracle):
    g = golden("f8_pdf")
    R = g["bins"].shape[0]
    det = cr.sample_pdf(g["bins"], g["weights"], torch.linspace(0.0, 1.0, steps=128).expand(R, 128))
    _check_pdf_samples(det.numpy(), g["det"], g["weights"])
    rand = cr.sample_pdf(g["bins"], g["weights"], oracle.pytest_uniforms((R, 128)))
    _check_pdf_samples(rand.numpy(), g["rand_pytest"], g["weights"])


def test_reference_in_float32_is_the_oracle(oracle):
    """At float32 the restatement is oracle.composite bit for bit (S = 100, noise, white background), forward and
    raw gradient: only the eps of the clamp separates the two, and float32's is the one the restatement keeps."""
    d = cr.composite_inputs(100, 9, 4, 1, 1)
    raw = torch.tensor(d["raw"]).requires_grad_(True)
    want = oracle.composite(raw, torch.tensor(d["z"]), torch.tensor(d["rays_d"]), torch.tensor(d["noise"]), True)
    grads = {n: d[n] for n in cr.GRAD_NAMES if d[n] is not None}
    sum((o * torch.tensor(d[n])).sum() for o, n in zip(want, cr.GRAD_NAMES)).backward()
    graw, got = cr.composite_grad(d["raw"], d["z"], d["rays_d"], d["noise"], True, grads, torch.float32)
    for n, a, b in zip(NAMES, got, want):
        np.testing.assert_array_equal(a.numpy(), b.detach().numpy(), err_msg=n)
    np.testing.assert_array_equal(graw.numpy(), raw.grad.numpy())
    # ... and in float64 it is another function than the oracle's: the oracle's eps follows the dtype
    w = torch.zeros(1, 4, dtype=torch.float64)
    w[0, 0] = 1e-9
    p = cr.entropy_probs(w)
    ours = -(torch.log(p.clamp(min=cr.EPS32, max=1 - cr.EPS32)) * p).sum()
    eps64 = torch.finfo(torch.float64).eps
    theirs = -(torch.log(p.clamp(min=eps64, max=1 - eps64)) * p).sum()
    assert abs(float(ours - theirs)) > 1e-9


def test_reference_handles_one_sample():
    """S = 1: the one delta is 1e10, so a positive sigma is opaque (w = 1, depth = z) and a non-positive one leaves
    acc = 0 and a NaN depth; oracle.composite returns empty tensors here."""
    raw = np.array([[[0.3, -1.0, 2.0, 0.7]], [[0.3, -1.0, 2.0, -0.7]]], np.float32)
    z = np.array([[2.5], [3.5]], np.float32)
    rgb, disp, acc, w, depth, ent, normal = cr.composite(raw, z, np.ones((2, 3), np.float32), None, True)
    assert w.shape == (2, 1) and normal is None
    np.testing.assert_allclose(w.numpy(), [[1.0], [0.0]])
    np.testing.assert_allclose(depth.numpy(), [2.5, np.nan], equal_nan=True)
    np.testing.assert_allclose(disp.numpy(), [0.4, np.nan], equal_nan=True)
    np.testing.assert_allclose(rgb[0].numpy(), 1 / (1 + np.exp(-raw[0, 0, :3].astype(np.float64))), rtol=1e-12)
    np.testing.assert_allclose(rgb[1].numpy(), [1.0, 1.0, 1.0])
    graw, _ = cr.composite_grad(raw, z, np.ones((2, 3), np.float32), None, True, dict(g_rgb=np.ones((2, 3), np.float32)))
    assert np.isfinite(graw.numpy()).all() and (graw.numpy()[1] == 0).all()


def test_reference_normals():
    d = cr.composite_inputs(63, 9, 7, 0, 1)
    out = cr.composite(d["raw"], d["z"], d["rays_d"], d["noise"], False)
    nraw = (out[3][..., None] * torch.tensor(d["raw"][..., 4:7]).double()).sum(-2)
    np.testing.assert_allclose(out[6].numpy(), torch.nn.functional.normalize(nraw, dim=-1, eps=1e-12).numpy(), rtol=1e-12)


def test_cases_cover_every_dispatch_shape():
    cases = cr.composite_cases()
    template = {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}       # NERF_COMPOSITE_DISPATCH
    lo, hi = {}, {}
    for S in cr.WIDTHS:
        K = template[(S + 63) // 64]
        lo[K], hi[K] = min(lo.get(K, S), S), max(hi.get(K, S), S)
    assert lo == {1: 1, 2: 65, 3: 129, 4: 193, 6: 257, 8: 385} and hi == {1: 64, 2: 128, 3: 192, 4: 256, 6: 384, 8: 512}
    assert {(S + 63) // 64 for S in cr.WIDTHS} >= {5, 6}
    assert {template[(c[0] + 63) // 64] for c in cases if c[2] == 7} == {1, 2, 3, 4, 6, 8}
    assert {(c[3], c[4]) for c in cases if c[1] == 9 and c[2] == 4} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    main = [c for c in cases if c[1] == 9 and c[2] == 4]
    assert sum(c[4] for c in main) * 2 == len(main) and sum(c[3] for c in main) * 2 == len(main)
    assert len({cr.case_seed(*c) for c in cases}) == len(cases)
    pairs = cr.sampler_cases()
    assert {S for S, _ in pairs} == set(cr.SAMPLER_S) and {N for _, N in pairs} == set(cr.SAMPLER_N)
    assert {(S - 2 + 63) // 64 for S in cr.SAMPLER_S} == {1, 2, 3, 4}
    for per in (1, 2, 3, 4):      # every width of build_cdf meets every sort path that fits beside it
        paths = {cr.sort_path(S, N) for S, N in pairs if (S - 2 + 63) // 64 == per}
        assert paths >= {"reg1", "reg2", "lds"}, (per, paths)
    assert cr.sort_path(256, 700) == "rank" and (256, 700) in pairs
    assert all(3 <= S <= 256 and S + N <= cr.MAX_MERGED for S, N in pairs + list(cr.FUSED_CASES))


def test_cases_stay_off_the_references_own_jumps():
    """Where the reference itself is discontinuous a one-ulp difference decides the branch, so no bar can hold there:
    no ray of any case has 1 - acc within 20 % of the entropy clamp's 1e-6, and every bin of every sampler case
    carries far more than the 1e-5 of sample_pdf's denominator rule."""
    for case in cr.composite_cases():
        _, out = cr.composite_reference(*case, ("g_entropy",))
        assert (np.abs((1 - out[2]) - 1e-6) > 0.2e-6).all(), case
    for S in cr.EDGE_WIDTHS:
        _, out = cr.edge_reference(S, ("g_entropy",))
        assert (np.abs((1 - out[2]) - 1e-6) > 0.2e-6).all(), S
    for S, N in cr.sampler_cases():
        d = cr.sampler_inputs(S, N)
        assert float(cr.bin_mass(d["w"][:, 1:-1]).min()) >= cr.MIN_BIN_MASS, (S, N)
    for S, N in cr.FUSED_CASES:
        d = cr.fused_inputs(S, N)
        w = cr.composite(d["raw"], d["z"], d["rays_d"])[3]
        assert float(cr.bin_mass(w[:, 1:-1]).min()) >= cr.MIN_BIN_MASS, (S, N)
        assert (np.diff(d["z"], axis=-1) > 0).all()


def test_float32_oracle_meets_the_sampler_bar():
    """The float32 restatement stays within 7.1e-6 of the float64 inverse CDF on these cases (the bar is
    isclose(rtol 1e-5, atol 1e-5), at least 3e-5 for depths in [2, 6])."""
    worst = 0.0
    for S, N in cr.sampler_cases():
        d = cr.sampler_inputs(S, N)
        s64 = cr.sample_fine(d["z"], d["w"], d["u"])[0]
        s32 = cr.sample_fine(d["z"], d["w"], d["u"], torch.float32)[0]
        worst = max(worst, float((s32.double() - s64).abs().max()))
    assert worst <= 1e-5, worst


def test_edge_batch_is_what_it_says():
    for S in cr.EDGE_WIDTHS:
        d = cr.edge_batch(S)
        graw, (rgb, disp, acc, w, depth, ent, _) = cr.edge_reference(S, ("g_rgb",))
        assert (d["raw"][0, :, 3] <= 0).all() and acc[0] == 0 and (w[0] == 0).all()
        assert np.isnan(depth[0]) and np.isnan(disp[0]) and (graw[0, :, 3] == 0).all()
        assert np.isfinite(graw).all() and np.isfinite(depth[1:]).all()
        assert w[1, 0] > 1 - 1e-12 and w[1, 1:].max() < 1e-9               # opaque at the first sample
        assert 1 - acc[2] < 1e-6 and np.count_nonzero(w[2] > 1e-3) > 3     # dense, over several samples
        dz = np.diff(d["z"][3])
        assert (dz == 0).sum() >= S // 2 and (w[3, :-1][dz == 0] == 0).all()


def test_entropy_yardstick():
    """The float32 oracle's worst entropy ratio is the recorded one (the GPU bar is four times it; float32 CPU kernels
    differ a little between processors, so within a quarter above and a half below) and next to nothing is excluded."""
    worst, share, ratios = cr.entropy_oracle_worst()
    print({k: f"{v:.3e}" for k, v in ratios.items()}, worst, share)
    assert 0.5 * cr.ENT_ORACLE_WORST <= worst <= 1.25 * cr.ENT_ORACLE_WORST, worst
    assert share <= cr.ENT_EXCLUDED_MAX
