#!/usr/bin/env python3
"""Per-launch A/B of the hash-encoding forward on fp32 tables (nerf_hash_encode_fwd) and on their fp16 image
(nerf_hash_encode_fwd_half): the lego configuration (16 levels, 2^19 entries, finest resolution 1024),
level-major features and keep flags, at 262,144 (4096 rays x 64 samples), 786,432 (4096 x 192) and 6,291,456
(32768 x 192) points, consecutive points being consecutive samples of a ray through the box as in the renderer. The two
launches alternate between device events after a warm-up of both (tables hot): median and min in us per launch, the
ratio of the medians, and whether the fp16 launch gives the fp32 launch's bits on the rounded tables.

--variant NAME=LIB (repeatable): the fp16 launch of another build of the library (tools/build_variant.py) joins the
alternation in the same process, as "fp16:NAME".
--feature-precision: the packed bf16 launches of both table formats (nerf_hash_encode_fwd_pkbf,
nerf_hash_encode_fwd_half_pkbf) join the alternation as "fp32:pkbf" and "fp16:pkbf": the ratio of each
unpacked launch's median to its packed twin's, and whether the words are the rounded features.
--device-sized: instead of the above, the packed launch on fp32 tables sized on the device
(nerf_hash_encode_fwd_pkbf_dev) against the host-sized one at the same count n, in the same alternation:
the default grid at capacity n and 4 n, the grid caps --max-blocks (default 256,512,1024,2048,4096,8192) at capacity n,
and a launch whose count is 0; medians, ratios to the host-sized launch, and whether the words are the same bits.
--counter-run: a few launches of each and nothing else, to run under the profiler's counter collection on its own
(no tracing beside it):  rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d DIR -o t -- \\
    python tools/hash_fwd_ab.py --counter-run
--counters FILE: summarise that run's t_counter_collection.csv into L2 hit rates per kernel and grid.
JSON out (--out FILE also writes it)."""
import argparse
import collections
import csv
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SHAPES = ((4096, 64), (4096, 192), (32768, 192))
KERNELS = ("hash_encode_fwd_pair_kernel", "hash_encode_fwd_half_pair_kernel", "hash_tables_to_half_kernel",
           "hash_encode_fwd_pkbf_kernel<false>", "hash_encode_fwd_pkbf_kernel<true>")


def counters(path):
    """L2 hits, misses and hit rate per launch of the hash forward kernels, by grid size (one per point count)."""
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"].split("(")[0].replace("void ", "")
        name = next((n for n in sorted(KERNELS, key=len, reverse=True) if n in k), None)
        if name is None:
            continue
        grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
        acc[(name, int(grid) if str(grid).isdigit() else grid)][r["Counter_Name"]].append(float(r["Counter_Value"]))
    out = []
    for (name, grid), d in sorted(acc.items(), key=lambda kv: (str(kv[0][1]).zfill(12), kv[0][0])):
        h = sum(d.get("TCC_HIT_sum", [0])) / max(1, len(d.get("TCC_HIT_sum", [0])))
        m = sum(d.get("TCC_MISS_sum", [0])) / max(1, len(d.get("TCC_MISS_sum", [0])))
        out.append({"kernel": name, "grid_size": grid, "launches": max(len(v) for v in d.values()),
                    "l2_hits": round(h), "l2_misses": round(m), "l2_hit_rate": round(h / (h + m), 4) if h + m else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB")
    ap.add_argument("--feature-precision", action="store_true")
    ap.add_argument("--device-sized", action="store_true")
    ap.add_argument("--max-blocks", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--counter-run", action="store_true")
    ap.add_argument("--counters", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.counters:
        report = {"l2_counters": counters(a.counters)}
    elif a.device_sized:
        report = run_device_sized(a)
    else:
        report = run(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            json.dump(report, fp, indent=1)
    print(json.dumps(report))


def run(a):
    import numpy as np
    import torch

    import indoor_nerf_amd as nerf
    from indoor_nerf_amd import _lib
    from tables import blender_bbox

    if not torch.cuda.is_available():
        raise SystemExit("hash_fwd_ab: needs a GPU (a time measured elsewhere says nothing)")
    dev = torch.device("cuda:0")
    lo, hi = blender_bbox()
    emb = nerf.HashEmbedder((torch.from_numpy(lo), torch.from_numpy(hi)), finest_resolution=1024).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for e in emb.embeddings:
            e.weight.copy_((torch.rand(e.weight.shape, device=dev, generator=g) * 2 - 1) * 0.05)
        twin = [e.weight.half().float() for e in emb.embeddings]
    meta, L = emb._meta, emb.n_levels
    image = emb.half_tables()
    tabs = _lib.ptr_array(emb.tables())
    twin_ptrs = _lib.ptr_array(twin)
    variants = {}
    for spec in a.variant:      # another build's entry, bound like _lib binds its own
        name, path = spec.split("=", 1)
        fn = getattr(ctypes.CDLL(os.path.abspath(path)), "nerf_hash_encode_fwd_half")
        fn.argtypes, fn.restype = _lib.SIGNATURES["nerf_hash_encode_fwd_half"], ctypes.c_int
        variants[name] = fn
    report = {"device": torch.cuda.get_device_name(0), "n_levels": L, "log2_T": meta["log2_T"], "points": {}}
    for R, S in SHAPES:
        P = R * S
        o = 4.0 * torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=-1)
        d = torch.nn.functional.normalize(-o + 0.8 * torch.randn(R, 3, device=dev, generator=g), dim=-1)
        t = torch.linspace(2.0, 6.0, S, device=dev)
        pts = (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3).contiguous()
        feat = {k: torch.empty(L, P, 2, device=dev) for k in ["fp32", "fp16", "twin"] + ["fp16:" + v for v in variants]}
        keep = {k: torch.empty(P, device=dev, dtype=torch.bool) for k in feat}

        packed = ["fp32:pkbf", "fp16:pkbf"] if a.feature_precision else []
        words = {k: torch.empty(L, P, device=dev, dtype=torch.int32) for k in packed}
        keep.update({k: torch.empty(P, device=dev, dtype=torch.bool) for k in packed})

        def launch_pk(kind, name, tables):
            _lib.call(name, _lib.ptr(pts), P, meta["bmin"], meta["bmax"], meta["res"], L, meta["log2_T"], tables,
                      _lib.ptr(words[kind], dtype=torch.int32), 1, P, _lib.ptr(keep[kind], dtype=torch.bool),
                      _lib.stream())

        def launch(kind, name, tables):
            _lib.call(name, _lib.ptr(pts), P, meta["bmin"], meta["bmax"], meta["res"], L, meta["log2_T"], tables,
                      _lib.ptr(feat[kind]), 2, 2 * P, _lib.ptr(keep[kind], dtype=torch.bool), _lib.stream())

        fns = {"fp32": lambda: launch("fp32", "nerf_hash_encode_fwd", tabs),
               "fp16": lambda: launch("fp16", "nerf_hash_encode_fwd_half", _lib.ptr(image, dtype=torch.uint8))}
        def variant_launch(vname):
            rc = variants[vname](_lib.ptr(pts), P, meta["bmin"], meta["bmax"], meta["res"], L, meta["log2_T"],
                                 _lib.ptr(image, dtype=torch.uint8), _lib.ptr(feat["fp16:" + vname]), 2, 2 * P,
                                 _lib.ptr(keep["fp16:" + vname], dtype=torch.bool), _lib.stream())
            if rc != 0:
                raise RuntimeError(f"variant {vname}: code {rc}")

        for vname in variants:
            fns["fp16:" + vname] = (lambda v=vname: variant_launch(v))
        if packed:
            fns["fp32:pkbf"] = lambda: launch_pk("fp32:pkbf", "nerf_hash_encode_fwd_pkbf", tabs)
            fns["fp16:pkbf"] = lambda: launch_pk("fp16:pkbf", "nerf_hash_encode_fwd_half_pkbf",
                                                 _lib.ptr(image, dtype=torch.uint8))
        if a.counter_run:
            for _ in range(4):
                for fn in fns.values():
                    fn()
            torch.cuda.synchronize()
            continue
        launch("twin", "nerf_hash_encode_fwd", twin_ptrs)
        ts = {name: [] for name in fns}
        for _ in range(a.rounds):
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.per_round):
                for name, fn in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ts[name].append(e0.elapsed_time(e1))
        row = {name + "_us_median": round(float(np.median(v)) * 1e3, 1) for name, v in ts.items()}
        row.update({name + "_us_min": round(float(np.min(v)) * 1e3, 1) for name, v in ts.items()})
        row["fp32_over_fp16"] = round(float(np.median(ts["fp32"]) / np.median(ts["fp16"])), 3)
        for vname in variants:
            row[f"fp16_over_fp16:{vname}"] = round(float(np.median(ts["fp16"]) / np.median(ts["fp16:" + vname])), 3)
            row[f"fp16:{vname}_same_bits"] = bool(torch.equal(feat["fp16:" + vname].view(torch.int32),
                                                              feat["fp16"].view(torch.int32)))
        for kind in packed:
            base = kind.split(":")[0]
            row[f"{base}_over_{kind}"] = round(float(np.median(ts[base]) / np.median(ts[kind])), 3)
            ref = feat[base].to(torch.bfloat16).contiguous().view(torch.int32).reshape(L, P)
            row[f"{kind}_words_are_the_rounded_features"] = bool(torch.equal(words[kind], ref)
                                                                 and torch.equal(keep[kind], keep[base]))
        row["inside_box"] = round(float(keep["fp16"].float().mean()), 4)
        row["fp16_equals_fp32_on_rounded_tables"] = bool(
            torch.equal(feat["fp16"].view(torch.int32), feat["twin"].view(torch.int32))
            and torch.equal(keep["fp16"], keep["twin"]))
        row["max_abs_diff_vs_fp32_tables"] = float((feat["fp16"] - feat["fp32"]).abs().max())
        report["points"][str(P)] = row
    if not a.counter_run:       # the conversion launch itself (64 MiB read, 32 MiB written)
        ts = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.call("nerf_hash_tables_to_half", tabs, L, meta["log2_T"], _lib.ptr(image, dtype=torch.uint8), _lib.stream())
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        report["tables_to_half_us_median"] = round(float(np.median(ts)) * 1e3, 1)
    return report


def alternate(fns, rounds, per_round):
    """run()'s protocol: per round three warm-up launches of each, then per_round timed launches of each in turn
    -> {name: [ms]}."""
    import torch
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
    return ts


def ab_row(ts, base="host"):
    """alternate()'s times as a table row: median and min in us per launch, and each median over `base`'s."""
    import numpy as np
    row = {name + "_us_median": round(float(np.median(v)) * 1e3, 1) for name, v in ts.items()}
    row.update({name + "_us_min": round(float(np.min(v)) * 1e3, 1) for name, v in ts.items()})
    row.update({f"{name}_over_{base}": round(float(np.median(v) / np.median(ts[base])), 3) for name, v in ts.items()
                if name != base})
    return row


def run_device_sized(a):
    import numpy as np
    import torch

    import indoor_nerf_amd as nerf
    from indoor_nerf_amd import _lib
    from tables import blender_bbox

    if not torch.cuda.is_available():
        raise SystemExit("hash_fwd_ab: needs a GPU (a time measured elsewhere says nothing)")
    dev = torch.device("cuda:0")
    lo, hi = blender_bbox()
    emb = nerf.HashEmbedder((torch.from_numpy(lo), torch.from_numpy(hi)), finest_resolution=1024).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for e in emb.embeddings:
            e.weight.copy_((torch.rand(e.weight.shape, device=dev, generator=g) * 2 - 1) * 0.05)
    meta, L = emb._meta, emb.n_levels
    tabs = _lib.ptr_array(emb.tables())
    caps = [int(c) for c in a.max_blocks.split(",")]
    report = {"device": torch.cuda.get_device_name(0), "n_levels": L, "log2_T": meta["log2_T"], "points": {}}
    for R, S in SHAPES:
        n = R * S
        o = 4.0 * torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=-1)
        d = torch.nn.functional.normalize(-o + 0.8 * torch.randn(R, 3, device=dev, generator=g), dim=-1)
        t = torch.linspace(2.0, 6.0, S, device=dev)
        pts = torch.zeros(4 * n, 3, device=dev)
        pts[:n] = (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3)
        total, zero = (torch.tensor([v], device=dev, dtype=torch.int32) for v in (n, 0))
        words = {k: torch.zeros(L * 4 * n, device=dev, dtype=torch.int32) for k in ("host", "dev")}
        keep = torch.empty(4 * n, device=dev, dtype=torch.bool)
        back = lambda k, sl: (_lib.ptr(words[k], dtype=torch.int32), 1, sl, _lib.ptr(keep, dtype=torch.bool), _lib.stream())  # noqa: E731
        box = (meta["bmin"], meta["bmax"], meta["res"], L, meta["log2_T"], tabs)

        def host():
            _lib.call("nerf_hash_encode_fwd_pkbf", _lib.ptr(pts), n, *box, *back("host", n))

        def device(cap, max_blocks=0, count=total):
            _lib.call("nerf_hash_encode_fwd_pkbf_dev", _lib.ptr(pts), _lib.ptr(count, dtype=torch.int32), 0, cap,
                      max_blocks, *box, *back("dev", cap))

        fns = {"host": host, "host again": host, "dev capacity n": lambda: device(n),
               "dev capacity 4n": lambda: device(4 * n), "dev empty, capacity n": lambda: device(n, 0, zero)}
        for c in caps:
            fns[f"dev capacity n, max_blocks {c}"] = (lambda c=c: device(n, c))
        host()
        device(n)
        torch.cuda.synchronize()
        same = bool(torch.equal(words["host"][:L * n], words["dev"][:L * n]))
        row = ab_row(alternate(fns, a.rounds, a.per_round))
        row["dev_words_are_the_host_words"] = same
        report["points"][str(n)] = row
        del words, pts, keep
    return report


if __name__ == "__main__":
    main()
