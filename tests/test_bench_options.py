"""bench.py's run shape (host only, no GPU): a plain run keeps to the headline — the legs that take
runs of their own (per-kernel timing, fresh rays, CPU baseline) are on only with --full — and
--dump-outputs writes the step's returns and the MLP state as bounded float32 arrays."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_extra_legs(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full) == (7, 3, False)
    assert not a.profile_kernels and not a.fresh_rays and a.no_cpu_baseline
    assert a.dump_outputs is None


def test_full_run_keeps_the_legs_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and a.profile_kernels and a.fresh_rays and not a.no_cpu_baseline
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--profile-kernels", "0", "--fresh-rays", "0")
    assert a.full and not a.profile_kernels and not a.fresh_rays and a.no_cpu_baseline


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def _state(seed):
    g = torch.Generator().manual_seed(seed)
    mlp = [torch.rand(5, 3, generator=g).requires_grad_(True), torch.rand(4, generator=g).requires_grad_(True)]
    for p in mlp:
        p.grad = torch.rand(p.shape, generator=g)
    return mlp


def test_dump_outputs_train(tmp_path):
    mlp = _state(0)
    bench.dump_outputs(str(tmp_path / "a"), "train", torch.tensor(0.25), torch.tensor(6.0), mlp, {})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["loss.npy", "mlp_grads.npy", "mlp_params.npy", "psnr.npy"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_MAX_BYTES
    assert got["loss"].tolist() == [0.25] and got["psnr"].tolist() == [6.0]
    np.testing.assert_array_equal(got["mlp_params"], torch.cat([p.detach().reshape(-1) for p in mlp]).numpy())
    np.testing.assert_array_equal(got["mlp_grads"], torch.cat([p.grad.reshape(-1) for p in mlp]).numpy())
    # before the first backward there are no gradients to write
    for p in mlp:
        p.grad = None
    bench.dump_outputs(str(tmp_path / "b"), "train", torch.tensor(0.25), torch.tensor(6.0), mlp, {})
    assert sorted(os.listdir(tmp_path / "b")) == ["loss.npy", "mlp_params.npy", "psnr.npy"]


def test_snapshot_and_restore_state_in_place():
    """The state the dump's replayed steps start from: parameters, buffers and the embedder's call count
    as before the first step, RAdam's moments zero and its step counts 0 — at the same addresses."""
    import types
    net = torch.nn.Linear(3, 2)
    emb = torch.nn.Embedding(4, 2)
    emb.register_buffer("scale", torch.ones(2))
    emb.current_step = 500
    kw = {"network_fn": net, "network_fine": None, "embed_fn": emb}
    params = list(net.parameters()) + list(emb.parameters())
    opt = types.SimpleNamespace(state={})
    snap = bench.snapshot_state(kw, params)
    want = [p.detach().clone() for p in params]
    ptrs = [p.data_ptr() for p in params]
    with torch.no_grad():
        for p in params:
            p.add_(1.0)
            opt.state[p] = {"step": 7, "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)}
        emb.scale.mul_(3.0)
    emb.current_step = 520
    moments = [(s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()) for s in opt.state.values()]
    bench.restore_state(snap, kw, params, opt)
    for p, w, ptr in zip(params, want, ptrs):
        assert torch.equal(p, w) and p.data_ptr() == ptr
    assert torch.equal(emb.scale, torch.ones(2)) and emb.current_step == 500
    for s, (pm, pv) in zip(opt.state.values(), moments):
        assert s["step"] == 0 and not s["exp_avg"].any() and not s["exp_avg_sq"].any()
        assert (s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()) == (pm, pv)


def test_dump_outputs_render_and_bound(tmp_path):
    maps = dict(rgb=torch.rand(9, 3), depth=torch.rand(9), acc=torch.rand(9).double())
    bench.dump_outputs(str(tmp_path / "r"), "render", maps["rgb"].mean(), maps["rgb"].mean(), [], maps)
    assert sorted(os.listdir(tmp_path / "r")) == ["acc.npy", "depth.npy", "rgb.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "r" / "rgb.npy"), maps["rgb"].numpy())
    assert np.load(tmp_path / "r" / "acc.npy").dtype == np.float32
    big = dict(rgb=torch.zeros(bench.DUMP_MAX_BYTES // 4 + 1))
    with pytest.raises(RuntimeError, match="exceed"):
        bench.dump_outputs(str(tmp_path / "big"), "render", None, None, [], big)
    assert not os.path.exists(tmp_path / "big")
