#!/usr/bin/env python3
"""Timing of the batched MLP backward (nerf_mlp_bwd_batch) on the lego step's two nets: the fine
(4096 x 192 points) and the coarse (4096 x 64) net in one launch, HIP-event median per launch, plus a
checksum of every output (dfeat of both nets, the ten weight gradients) so that builds can be told to
compute the same thing; and of the MLP forward at the step's two point counts (262,144 and 786,432), the
fp32-accurate kernel (nerf_mlp_fwd) and the bf16 one (nerf_mlp_fwd_bf16) alternating, where the
library has it. A/B of library builds: run once per build with NERF_HIP_LIB=<path>
(tools/build_variant.py). JSON out.

--feature-precision: only the A/B of the bf16 forward on fp32 features (nerf_mlp_fwd_bf16) against the same forward on
packed bf16 words (nerf_mlp_fwd_bf16_pkbf), real features of the lego hash configuration: at 262,144
points with the features hot (written once, the two launches alternate) and at 6,291,456 points with them not
resident in cache (each timed launch follows an encode launch of that size into its buffer: 805 MB of fp32
features, 403 MB of words). Median and min in us per launch, the ratio of the medians, whether raw has the same bits.
--counter-run (with --feature-precision): a few launch pairs and nothing else, to run under the profiler's counter
collection on its own. --out FILE also writes the JSON.

--march-sh: only the A/B of the three forwards on per-point SH rows (nerf_mlp_fwd_ord, nerf_mlp_fwd_bf16,
nerf_mlp_fwd_bf16_pkbf at sh_stride 16) against the same forwards reading one SH record per ray through a ray index
(nerf_mlp_fwd_rays, nerf_mlp_fwd_bf16_rays, nerf_mlp_fwd_bf16_pkbf_rays), segments of 49 consecutive
points per ray, at the same two point counts and cache states as --feature-precision. --counter-run applies.

--device-sized: only the A/B of nerf_mlp_fwd_bf16_pkbf_rays against nerf_mlp_fwd_bf16_pkbf_rays_dev,
which reads its point count on the device: count n in a capacity of n and of 4 n, and a count of 0, at 262,144,
786,432 and 6,291,456 points, features hot."""
import argparse
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


def make_job(P, spr, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    net = nerf.NeRFSmall(2, 64, 15, 3, 64, 32, 16).to(dev)
    feat = (torch.randn(16, P, 2, device=dev, generator=g) * 0.3).contiguous()
    vd = torch.nn.functional.normalize(torch.randn(P // spr, 3, device=dev, generator=g), dim=-1).contiguous()
    keep = (torch.rand(P, device=dev, generator=g) > 0.05).contiguous()
    graw = torch.randn(P, 4, device=dev, generator=g).contiguous()
    dfeat = torch.empty_like(feat)
    ws = [p.detach() for p in net.mlp_weights()]
    grads = [torch.zeros_like(w) for w in ws]
    j = _lib.MlpBwdJob()
    j.feat, j.feat_stride_point, j.feat_stride_level = _lib.ptr(feat), 2, 2 * P
    j.viewdirs, j.samples_per_ray = _lib.ptr(vd), spr
    j.keep = _lib.ptr(keep, dtype=torch.bool)
    j.n_points = P
    w = _lib.MlpWeights()
    gs = _lib.MlpGrads()
    for name, t, gt in zip(("w0", "w1", "c0", "c1", "c2"), ws, grads):
        setattr(w, name, _lib.ptr(t).value)
        setattr(gs, name, _lib.ptr(gt).value)
    j.weights, j.grads = w, gs
    j.graw, j.dfeat = _lib.ptr(graw), _lib.ptr(dfeat)
    return j, dict(feat=feat, vd=vd, keep=keep, graw=graw, dfeat=dfeat, ws=ws, grads=grads)


def forward_ab(jobs, dev, rounds=5, per_round=20):
    """Per point count: the x6 and the bf16 forward launch (view directions, keep flags, level-major features),
    alternating launch by launch between device events after a warm-up of both: median and min in us, the ratio of
    the medians, and the largest |raw difference| of the two kernels on the job's data."""
    out = {}
    if not hasattr(_lib.load(), "nerf_mlp_fwd_bf16"):
        return out
    for j, k, spr in jobs:
        P = k["feat"].shape[1]
        raws = {"x6": torch.empty(P, 4, device=dev), "bf16": torch.empty(P, 4, device=dev)}
        front = (_lib.ptr(k["feat"]), 2, 2 * P, None, 0, _lib.ptr(k["vd"]), spr, _lib.ptr(k["keep"], dtype=torch.bool), P,
                 ctypes.byref(j.weights))
        fns = {"x6": lambda: _lib.call("nerf_mlp_fwd", *front, _lib.ptr(raws["x6"]), None, _lib.stream()),
               "bf16": lambda: _lib.call("nerf_mlp_fwd_bf16", *front, _lib.ptr(raws["bf16"]), None, _lib.stream())}
        ts = {name: [] for name in fns}
        for _ in range(rounds):
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(per_round):
                for name, fn in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ts[name].append(e0.elapsed_time(e1))
        row = {name + "_us_median": round(float(np.median(v)) * 1e3, 1) for name, v in ts.items()}
        row.update({name + "_us_min": round(float(np.min(v)) * 1e3, 1) for name, v in ts.items()})
        row["x6_over_bf16"] = round(float(np.median(ts["x6"]) / np.median(ts["bf16"])), 3)
        row["max_abs_raw_diff"] = float((raws["x6"] - raws["bf16"]).abs().max())
        out[str(P)] = row
    return out


def packed_ab(dev, counter_run=False, rounds=5, per_round=20):
    """The --feature-precision table: see the module docstring."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from tables import blender_bbox
    lo, hi = blender_bbox()
    emb = nerf.HashEmbedder((torch.from_numpy(lo), torch.from_numpy(hi)), finest_resolution=1024).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    net = nerf.NeRFSmall(2, 64, 15, 3, 64, 32, 16).to(dev)
    w = _lib.MlpWeights(*[_lib.ptr(p.detach()).value for p in net.mlp_weights()])
    with torch.no_grad():
        for e in emb.embeddings:
            e.weight.copy_((torch.rand(e.weight.shape, device=dev, generator=g) * 2 - 1) * 0.05)
    L = emb.n_levels
    out = {}
    for R, S, cold in ((4096, 64, False), (32768, 192, True)):
        P = R * S
        o = 4.0 * torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=-1)
        d = torch.nn.functional.normalize(-o + 0.8 * torch.randn(R, 3, device=dev, generator=g), dim=-1)
        t = torch.linspace(2.0, 6.0, S, device=dev)
        pts = (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3).contiguous()
        feat, words = torch.empty(L, P, 2, device=dev), torch.empty(L, P, device=dev, dtype=torch.int32)
        keep = torch.empty(P, device=dev, dtype=torch.bool)
        raws = {"bf16": torch.empty(P, 4, device=dev), "bf16:pkbf": torch.empty(P, 4, device=dev)}
        back = (None, 0, _lib.ptr(d), S, _lib.ptr(keep, dtype=torch.bool), P, ctypes.byref(w))
        with torch.no_grad():
            enc = {"bf16": lambda: emb.encode_into(pts, feat, 2, 2 * P, keep),
                   "bf16:pkbf": lambda: emb.encode_into(pts, words, 1, P, keep, packed=True)}
        fns = {"bf16": lambda: _lib.call("nerf_mlp_fwd_bf16", _lib.ptr(feat), 2, 2 * P, *back, _lib.ptr(raws["bf16"]),
                                         None, _lib.stream()),
               "bf16:pkbf": lambda: _lib.call("nerf_mlp_fwd_bf16_pkbf", _lib.ptr(words, dtype=torch.int32), 1, P, *back,
                                              _lib.ptr(raws["bf16:pkbf"]), None, _lib.stream())}
        with torch.no_grad():
            for name in fns:
                enc[name]()
                fns[name]()
            torch.cuda.synchronize()
            if counter_run:
                for _ in range(3):
                    for name in fns:
                        if cold:
                            enc[name]()
                        fns[name]()
                torch.cuda.synchronize()
                continue
            ts = {name: [] for name in fns}
            for _ in range(rounds):
                for fn in fns.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                for _ in range(per_round if not cold else max(4, per_round // 2)):
                    for name, fn in fns.items():
                        if cold:      # the features written by a preceding encode of this size, as in a frame
                            enc[name]()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        torch.cuda.synchronize()
                        ts[name].append(e0.elapsed_time(e1))
        row = {name + "_us_median": round(float(np.median(v)) * 1e3, 1) for name, v in ts.items()}
        row.update({name + "_us_min": round(float(np.min(v)) * 1e3, 1) for name, v in ts.items()})
        row["bf16_over_bf16:pkbf"] = round(float(np.median(ts["bf16"]) / np.median(ts["bf16:pkbf"])), 3)
        row["features"] = "written by a preceding encode launch" if cold else "hot"
        row["feature_bytes"] = {"bf16": feat.numel() * 4, "bf16:pkbf": words.numel() * 4}
        row["raw_same_bits"] = bool(torch.equal(raws["bf16"].view(torch.int32), raws["bf16:pkbf"].view(torch.int32)))
        out[str(P)] = row
    return out


def march_sh_ab(dev, counter_run=False, rounds=5, per_round=20, segment=49):
    """The --march-sh table: see the module docstring."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from tables import blender_bbox
    lo, hi = blender_bbox()
    emb = nerf.HashEmbedder((torch.from_numpy(lo), torch.from_numpy(hi)), finest_resolution=1024).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    net = nerf.NeRFSmall(2, 64, 15, 3, 64, 32, 16).to(dev)
    w = _lib.MlpWeights(*[_lib.ptr(p.detach()).value for p in net.mlp_weights()])
    with torch.no_grad():
        for e in emb.embeddings:
            e.weight.copy_((torch.rand(e.weight.shape, device=dev, generator=g) * 2 - 1) * 0.05)
    L = emb.n_levels
    out = {}
    for R, S, cold in ((4096, 64, False), (32768, 192, True)):
        P = R * S
        o = 4.0 * torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=-1)
        d = torch.nn.functional.normalize(-o + 0.8 * torch.randn(R, 3, device=dev, generator=g), dim=-1)
        t = torch.linspace(2.0, 6.0, S, device=dev)
        pts = (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3).contiguous()
        n_rays = -(-P // segment)
        ray_of = (torch.arange(P, device=dev) // segment).to(torch.int32)
        views = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev, generator=g), dim=-1)
        rays = torch.cat([torch.zeros(n_rays, 8, device=dev), views], 1).contiguous()
        rec = torch.empty(n_rays, 40, device=dev)
        _lib.call("nerf_ray_sh_records", _lib.ptr(rays), n_rays, 11, _lib.ptr(rec), _lib.stream())
        sh_c = rec[ray_of.long(), :16].contiguous()
        feat, words = torch.empty(L, P, 2, device=dev), torch.empty(L, P, device=dev, dtype=torch.int32)
        keep = torch.empty(P, device=dev, dtype=torch.bool)
        kp, wp = _lib.ptr(keep, dtype=torch.bool), ctypes.byref(w)
        rows_view = (_lib.ptr(sh_c), 16, None, 1, kp, P, wp)
        rays_view = (_lib.ptr(rec), _lib.ptr(ray_of, dtype=torch.int32), n_rays, kp, P, wp)
        fp, wdp = (_lib.ptr(feat), 2, 2 * P), (_lib.ptr(words, dtype=torch.int32), 1, P)
        raws = {}

        def fn(entry, front, view, tail):
            raws[entry] = torch.empty(P, 4, device=dev)
            return lambda: _lib.call(entry, *front, *view, _lib.ptr(raws[entry]), *tail, _lib.stream())
        fns = {"nerf_mlp_fwd_ord": fn("nerf_mlp_fwd_ord", fp, rows_view, (None, None, None, 0, None)),
               "nerf_mlp_fwd_rays": fn("nerf_mlp_fwd_rays", fp, rays_view, ()),
               "nerf_mlp_fwd_bf16": fn("nerf_mlp_fwd_bf16", fp, rows_view, (None,)),
               "nerf_mlp_fwd_bf16_rays": fn("nerf_mlp_fwd_bf16_rays", fp, rays_view, ()),
               "nerf_mlp_fwd_bf16_pkbf": fn("nerf_mlp_fwd_bf16_pkbf", wdp, rows_view, (None,)),
               "nerf_mlp_fwd_bf16_pkbf_rays": fn("nerf_mlp_fwd_bf16_pkbf_rays", wdp, rays_view, ())}
        with torch.no_grad():
            encode = {False: lambda: emb.encode_into(pts, feat, 2, 2 * P, keep),
                      True: lambda: emb.encode_into(pts, words, 1, P, keep, packed=True)}
            enc = {name: encode["pkbf" in name] for name in fns}
            for name in fns:
                enc[name]()
                fns[name]()
            torch.cuda.synchronize()
            if counter_run:
                for _ in range(3):
                    for name in fns:
                        if cold:
                            enc[name]()
                        fns[name]()
                torch.cuda.synchronize()
                continue
            ts = {name: [] for name in fns}
            for _ in range(rounds):
                for f in fns.values():
                    for _ in range(3):
                        f()
                torch.cuda.synchronize()
                for _ in range(per_round if not cold else max(4, per_round // 2)):
                    for name, f in fns.items():
                        if cold:      # the features written by a preceding encode of this size, as in a frame
                            enc[name]()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        torch.cuda.synchronize()
                        ts[name].append(e0.elapsed_time(e1))
        row = {name + "_us_median": round(float(np.median(v)) * 1e3, 1) for name, v in ts.items()}
        row.update({name + "_us_min": round(float(np.min(v)) * 1e3, 1) for name, v in ts.items()})
        for twin in ("nerf_mlp_fwd_ord", "nerf_mlp_fwd_bf16", "nerf_mlp_fwd_bf16_pkbf"):
            by_ray = twin.replace("_ord", "") + "_rays"
            row[f"{twin}_over_{by_ray}"] = round(float(np.median(ts[twin]) / np.median(ts[by_ray])), 3)
            row[f"{by_ray}_raw_same_bits"] = bool(torch.equal(raws[twin].view(torch.int32), raws[by_ray].view(torch.int32)))
        row["features"] = "written by a preceding encode launch" if cold else "hot"
        row["sh_bytes"] = {"rows": sh_c.numel() * 4, "index + records": ray_of.numel() * 4 + rec.numel() * 4}
        out[str(P)] = row
    return out


def device_sized_ab(dev, rounds=5, per_round=20, segment=49):
    """The --device-sized table: nerf_mlp_fwd_bf16_pkbf_rays at n points against
    nerf_mlp_fwd_bf16_pkbf_rays_dev at count n in a capacity of n and of 4 n, and a launch whose count is 0, at 262,144,
    786,432 and 6,291,456 points (features hot), alternating after a warm-up; host-sized twice (the run's spread)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from hash_fwd_ab import ab_row, alternate      # the alternation protocol and the row, shared with that tool
    from tables import blender_bbox
    lo, hi = blender_bbox()
    emb = nerf.HashEmbedder((torch.from_numpy(lo), torch.from_numpy(hi)), finest_resolution=1024).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    net = nerf.NeRFSmall(2, 64, 15, 3, 64, 32, 16).to(dev)
    w = _lib.MlpWeights(*[_lib.ptr(p.detach()).value for p in net.mlp_weights()])
    with torch.no_grad():
        for e in emb.embeddings:
            e.weight.copy_((torch.rand(e.weight.shape, device=dev, generator=g) * 2 - 1) * 0.05)
    L = emb.n_levels
    out = {}
    for R, S in ((4096, 64), (4096, 192), (32768, 192)):
        n = R * S
        o = 4.0 * torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=-1)
        d = torch.nn.functional.normalize(-o + 0.8 * torch.randn(R, 3, device=dev, generator=g), dim=-1)
        t = torch.linspace(2.0, 6.0, S, device=dev)
        pts = (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3).contiguous()
        n_rays = -(-n // segment)
        ray_of = torch.zeros(4 * n, device=dev, dtype=torch.int32)
        ray_of[:n] = (torch.arange(n, device=dev) // segment).to(torch.int32)
        views = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev, generator=g), dim=-1)
        rays = torch.cat([torch.zeros(n_rays, 8, device=dev), views], 1).contiguous()
        rec = torch.empty(n_rays, 40, device=dev)
        _lib.call("nerf_ray_sh_records", _lib.ptr(rays), n_rays, 11, _lib.ptr(rec), _lib.stream())
        words = {c: torch.zeros(L, c, device=dev, dtype=torch.int32) for c in (n, 4 * n)}
        keep = torch.ones(4 * n, device=dev, dtype=torch.bool)
        with torch.no_grad():
            emb.encode_into(pts, words[n], 1, n, keep, packed=True)
        words[4 * n][:, :n] = words[n]
        total, zero = (torch.tensor([v], device=dev, dtype=torch.int32) for v in (n, 0))
        raws = {k: torch.zeros(4 * n, 4, device=dev) for k in ("host", "dev")}
        kp, wp, rp = _lib.ptr(keep, dtype=torch.bool), ctypes.byref(w), _lib.ptr(ray_of, dtype=torch.int32)

        def host():
            _lib.call("nerf_mlp_fwd_bf16_pkbf_rays", _lib.ptr(words[n], dtype=torch.int32), 1, n, _lib.ptr(rec), rp, n_rays,
                      kp, n, wp, _lib.ptr(raws["host"]), _lib.stream())

        def device(cap, count=total):
            _lib.call("nerf_mlp_fwd_bf16_pkbf_rays_dev", _lib.ptr(words[cap], dtype=torch.int32), 1, cap, _lib.ptr(rec), rp,
                      n_rays, kp, _lib.ptr(count, dtype=torch.int32), 0, cap, wp, _lib.ptr(raws["dev"]), _lib.stream())

        fns = {"host": host, "host again": host, "dev capacity n": lambda: device(n),
               "dev capacity 4n": lambda: device(4 * n), "dev empty, capacity n": lambda: device(n, zero)}
        host()
        device(4 * n)
        torch.cuda.synchronize()
        same = bool(torch.equal(raws["host"][:n].view(torch.int32), raws["dev"][:n].view(torch.int32)))
        row = ab_row(alternate(fns, rounds, per_round))
        row["dev_raw_same_bits"] = same
        out[str(n)] = row
        del words, raws
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-sized", action="store_true")
    ap.add_argument("--march-sh", action="store_true")
    ap.add_argument("--feature-precision", action="store_true")
    ap.add_argument("--counter-run", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.feature_precision or a.march_sh or a.device_sized:
        report = {"device": torch.cuda.get_device_name(0)}
        if a.device_sized:
            report["device_sized_ab"] = device_sized_ab(dev)
        elif a.march_sh:
            report["march_sh_ab"] = march_sh_ab(dev, a.counter_run)
        else:
            report["packed_ab"] = packed_ab(dev, a.counter_run)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fp:
                json.dump(report, fp, indent=1)
        print(json.dumps(report))
        return
    torch.manual_seed(0)
    jf, kf = make_job(4096 * 192, 192, 1, dev)
    jc, kc = make_job(4096 * 64, 64, 2, dev)
    arr = (_lib.MlpBwdJob * 2)(jf, jc)
    det = int(os.environ.get("NERF_DET", "0"))
    ws = torch.empty(int(_lib.load().nerf_mlp_bwd_det_workspace_bytes()) // 4, device=dev) if det else None

    def run():
        _lib.call("nerf_mlp_bwd_batch", arr, 2, _lib.ptr(ws, allow_none=True), 0 if ws is None else ws.numel() * 4,
                  _lib.stream())

    for k in (kf, kc):
        for t in k["grads"]:
            t.zero_()
    run()
    torch.cuda.synchronize()
    check = {"dfeat_f": float(kf["dfeat"].double().abs().sum()), "dfeat_c": float(kc["dfeat"].double().abs().sum()),
             "grads": [float(t.double().sum()) for k in (kf, kc) for t in k["grads"]]}
    def timed(fn):
        ts = []
        for rnd in range(5):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
        return ts

    # forward of the fine net (the lego step's larger MLP forward launch)
    raw = torch.empty(kf["feat"].shape[1], 4, device=dev)
    w = jf.weights

    def fwd():
        _lib.call("nerf_mlp_fwd", _lib.ptr(kf["feat"]), 2, 2 * raw.shape[0], None, 0, _lib.ptr(kf["vd"]), 192,
                  _lib.ptr(kf["keep"], dtype=torch.bool), raw.shape[0], ctypes.byref(w), _lib.ptr(raw), None,
                  _lib.stream())

    fwd()
    torch.cuda.synchronize()
    check["raw"] = float(raw.double().abs().sum())
    ts = timed(run)
    tf = timed(fwd)
    fwd_ab = forward_ab(((jf, kf, 192), (jc, kc, 64)), dev)
    print(json.dumps({"lib": os.environ.get("NERF_HIP_LIB", "default"), "us_median": round(float(np.median(ts)) * 1e3, 1),
                      "us_min": round(float(np.min(ts)) * 1e3, 1), "fwd_us_median": round(float(np.median(tf)) * 1e3, 1),
                      "fwd_us_min": round(float(np.min(tf)) * 1e3, 1), "det": det, "check": check,
                      "fwd_ab": fwd_ab}))

if __name__ == "__main__":
    main()
