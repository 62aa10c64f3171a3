#!/usr/bin/env python3
"""Bitwise comparison of two library builds on the hash backward's run-merge cases.
  bin_scan_bitwise.py dump OUT.npz      deterministic table gradients (levels 16 and 1024, T = 2^19) of every point
                                        set of tests/bin_scan_cases.py and of hash_bwd_ref.run_points, with the library
                                        NERF_HIP_LIB names (default: the tree's)
  bin_scan_bitwise.py compare A.npz B.npz [BENCH_DUMP_A BENCH_DUMP_B]
                                        one line per array: identical, or the number of differing words; the optional
                                        directories are two `bench.py --deterministic 1 --dump-outputs` dumps
Exit status 1 when anything differs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]


def dump(out):
    import torch
    import bin_scan_cases as bs
    import hash_bwd_ref as hb
    from tables import blender_bbox
    from indoor_nerf_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lo, hi = blender_bbox()
    levels, T = (16.0, 1024.0), 19
    sets = {f"runs_{n}": bs.run_set(n)[0] for n in bs.RUN_LENGTHS}
    sets["run_points"] = hb.run_points(int(lib.nerf_hash_bwd_chunk_points()))[0]
    arrays = {}
    for k, (name, x) in enumerate(sets.items()):
        P = len(x)
        d = hb.random_grads(len(levels), P, seed=300 + k, decades=3.0)
        xt, dt = torch.from_numpy(x).to(dev), torch.from_numpy(d).to(dev)
        g = [torch.zeros(1 << T, 2, device=dev) for _ in levels]
        nbytes = int(lib.nerf_hash_encode_bwd_workspace_bytes(len(levels), T, P, 1))
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
        _lib.call("nerf_hash_encode_bwd_ws", _lib.ptr(xt), P, _lib.host_f32(lo), _lib.host_f32(hi), _lib.host_f32(levels),
                  len(levels), T, _lib.ptr(dt), 2, 2 * P, _lib.ptr_array(g), 1, _lib.ptr(ws, dtype=torch.uint8), nbytes,
                  _lib.stream())
        torch.cuda.synchronize()
        for lvl, t in enumerate(g):
            arrays[f"{name}_level{lvl}"] = t.cpu().numpy()
    np.savez_compressed(out, **arrays)
    print(f"{len(arrays)} arrays from {_lib.LIB_PATH} -> {out}")


def _line(name, a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return f"{name} shapes differ {a.shape} {b.shape}", 1
    n = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    nz = int((a != 0).sum())
    return f"{name} {a.shape} " + ("identical" if n == 0 else f"{n} words differ") + f" ({nz} nonzero)", int(n != 0)


def compare(args):
    bad = 0
    a, b = np.load(args[0]), np.load(args[1])
    assert sorted(a.files) == sorted(b.files)
    for k in sorted(a.files):
        s, e = _line(k, a[k], b[k])
        print(s)
        bad += e
    if len(args) == 4:
        for f in sorted(os.listdir(args[2])):
            if f.endswith(".npy"):
                s, e = _line(f, np.load(os.path.join(args[2], f)), np.load(os.path.join(args[3], f)))
                print(s)
                bad += e
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2:]))
