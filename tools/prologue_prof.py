#!/usr/bin/env python3
"""Share of the weight-image prologue in a block's lifetime, MLP forward and backward (diagnostic library built with
-DNERF_X6_PROLOGUE_PROF: tools/build_variant.py NAME -DNERF_X6_PROLOGUE_PROF, run with NERF_HIP_LIB=<that library>).
The lego step's launches: the training forward (nerf_mlp_fwd_h3 with the saved-h3 buffer, per-ray SH records) at
262,144 and 786,432 points and the batched backward of both nets on the saved h3. Per launch, over its blocks: the
cycles from kernel entry to the prologue's barrier, the block's lifetime, their ratio, and the same in microseconds
(the blocks' own 100 MHz real-time stamps give the cycle length). JSON out: argv[1] (and stdout)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import indoor_nerf_amd as nerf  # noqa: E402
from indoor_nerf_amd import _lib  # noqa: E402

N_BLOCKS, N_FIELDS = 512, 5


def read_stamps(lib):
    buf = (ctypes.c_ulonglong * (2 * N_BLOCKS * N_FIELDS))()
    assert lib.nerf_x6_prologue_prof(buf) == 0
    return np.frombuffer(buf, dtype=np.uint64).reshape(2, N_BLOCKS, N_FIELDS).astype(np.int64)


def summary(rec, event_us):
    rec = rec[rec[:, 2] > 0]
    pro, life = rec[:, 1] - rec[:, 0], rec[:, 2] - rec[:, 0]
    us_per_cycle = float((rec[:, 4] - rec[:, 3]).sum()) / 100.0 / max(float(life.sum()), 1.0)
    t0 = rec[:, 3].min()
    return {"blocks": int(rec.shape[0]), "prologue_cycles_median": int(np.median(pro)),
            "prologue_cycles_p95": int(np.percentile(pro, 95)), "lifetime_cycles_median": int(np.median(life)),
            "prologue_share_of_block_lifetime": round(float(pro.sum()) / max(float(life.sum()), 1.0), 4),
            "us_per_cycle": round(us_per_cycle, 6), "prologue_us_median": round(float(np.median(pro)) * us_per_cycle, 2),
            "lifetime_us_median": round(float(np.median(life)) * us_per_cycle, 2),
            # blocks of a second wave (the grid exceeds what is resident at once) start late
            "block_start_us_max": round(float((rec[:, 3] - t0).max()) / 100.0, 2),
            "launch_event_us_median": round(float(np.median(event_us)), 1)}


def make_net(P, spr, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    net = nerf.NeRFSmall(2, 64, 15, 3, 64, 32, 16).to(dev)
    R = P // spr
    k = dict(P=P, spr=spr, ws=[p.detach() for p in net.mlp_weights()])
    k["feat"] = (torch.randn(16, P, 2, device=dev, generator=g) * 0.3).contiguous()
    rays = torch.cat([torch.zeros(R, 8, device=dev),
                      torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=-1)], 1).contiguous()
    k["rec"] = torch.empty(R, 40, device=dev)
    _lib.call("nerf_ray_sh_records", _lib.ptr(rays), R, 11, _lib.ptr(k["rec"]), _lib.stream())
    k["keep"] = (torch.rand(P, device=dev, generator=g) > 0.05).contiguous()
    k["graw"] = torch.randn(P, 4, device=dev, generator=g).contiguous()
    k["raw"], k["dfeat"] = torch.empty(P, 4, device=dev), torch.empty(16, P, 2, device=dev)
    k["h3"] = torch.empty(int(_lib.load().nerf_mlp_h3_bytes(P)) // 4, device=dev)
    k["grads"] = [torch.zeros_like(w) for w in k["ws"]]
    k["w"] = _lib.MlpWeights(*[_lib.ptr(t).value for t in k["ws"]])
    return k


def forward(k):
    _lib.call("nerf_mlp_fwd_h3", _lib.ptr(k["feat"]), 2, 2 * k["P"], _lib.ptr(k["rec"]), 0, None, k["spr"],
              _lib.ptr(k["keep"], dtype=torch.bool), k["P"], ctypes.byref(k["w"]), _lib.ptr(k["raw"]), None, None, None,
              0, None, _lib.ptr(k["h3"]), _lib.stream())


def bwd_job(k):
    j = _lib.MlpBwdJob()
    j.feat, j.feat_stride_point, j.feat_stride_level = _lib.ptr(k["feat"]), 2, 2 * k["P"]
    j.dfeat_stride_point, j.dfeat_stride_level = 2, 2 * k["P"]
    j.sh, j.sh_stride, j.samples_per_ray = _lib.ptr(k["rec"]), 0, k["spr"]
    j.keep, j.n_points, j.weights = _lib.ptr(k["keep"], dtype=torch.bool), k["P"], k["w"]
    j.graw, j.dfeat, j.h3 = _lib.ptr(k["graw"]), _lib.ptr(k["dfeat"]), _lib.ptr(k["h3"])
    j.grads = _lib.MlpGrads(*[_lib.ptr(t).value for t in k["grads"]])
    return j


def timed(lib, fn, kernel, reps=7):
    ev, times, last = [torch.cuda.Event(enable_timing=True) for _ in range(2)], [], None
    for _ in range(reps):
        read_stamps(lib)   # reset
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3)
        last = read_stamps(lib)[kernel]
    return summary(last, times[2:])


def main():
    dev = torch.device("cuda:0")
    lib = _lib.load()
    if not hasattr(lib, "nerf_x6_prologue_prof"):
        raise SystemExit("this library was not built with -DNERF_X6_PROLOGUE_PROF (see the module docstring)")
    lib.nerf_x6_prologue_prof.restype = ctypes.c_int
    lib.nerf_x6_prologue_prof.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
    torch.manual_seed(0)
    fine, coarse = make_net(4096 * 192, 192, 1, dev), make_net(4096 * 64, 64, 2, dev)
    out = {"lib": os.environ.get("NERF_HIP_LIB", "default"), "device": torch.cuda.get_device_name(0)}
    out["fwd_262144"] = timed(lib, lambda: forward(coarse), 0)
    out["fwd_786432"] = timed(lib, lambda: forward(fine), 0)
    arr = (_lib.MlpBwdJob * 2)(bwd_job(fine), bwd_job(coarse))
    out["bwd_batch_786432_262144"] = timed(lib, lambda: _lib.call("nerf_mlp_bwd_batch", arr, 2, None, 0, _lib.stream()), 1)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fp:
            json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
