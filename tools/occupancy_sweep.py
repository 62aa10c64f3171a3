"""Measurement (GPU box): OccupancyGrid.update's sigma_thresh and dilate on the trained two-sphere
scene (tools/render_time.py's trained_scene): per setting the occupied fraction, the build time, and for
the held-out and the novel rays of tests/test_gpu_converge.py the PSNR difference to the dense render
and the share of the fine pass's points that were evaluated. Also the quantiles of raw sigma at the cell
centres of both networks (how much of the box the field has learnt to be empty).

usage: python tools/occupancy_sweep.py [--iters 300] [--out bench_out/occupancy_sweep.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_time as rt  # noqa: E402
from tables import convergence_rays  # noqa: E402  (render_time puts tests/golden on sys.path)

nerf = rt.nerf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--out", default="bench_out/occupancy_sweep.json")
    a = ap.parse_args()
    bbox, emb, coarse, fine, kw = rt.trained_scene(a.iters)
    gpu = torch.device("cuda:0")
    _, ev, nv = convergence_rays()
    sets = {"eval": [torch.from_numpy(x).to(gpu) for x in ev], "novel": [torch.from_numpy(x).to(gpu) for x in nv]}

    def psnr(o, d, t, **over):
        with torch.no_grad():
            out = nerf.render(800, 800, None, rays=(o, d), **dict(kw, **over))[0]
        return float(-10 * torch.log10(((out - t) ** 2).mean()))

    dense = {k: psnr(*v) for k, v in sets.items()}
    grid = nerf.OccupancyGrid(bbox, device=gpu)
    sigma = {}
    with torch.no_grad():
        pts = grid.cell_points(0, grid.n_cells // 8, 1, 0)
        view = torch.zeros(pts.shape[0], 3, device=gpu)
        view[:, 2] = 1
        qs = [0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99]
        for name, net in (("coarse", coarse), ("fine", fine)):
            s = kw["network_query_fn"](pts, view, net)[..., 3].reshape(-1)
            q = torch.quantile(s[:1000000], torch.tensor(qs, device=gpu))
            sigma[name] = {"quantiles": dict(zip(map(str, qs), [float(v) for v in q])),
                           "share_positive": float((s > 0).float().mean())}
    rows = []
    for th in (0.0, 0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0):
        for dil in (0, 1, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grid.update(emb, [coarse, fine], sigma_thresh=th, dilate=dil)
            torch.cuda.synchronize()
            r = {"thresh": th, "dilate": dil, "occupied": grid.occupied_fraction(),
                 "build_ms": 1e3 * (time.perf_counter() - t0)}
            for k, v in sets.items():
                p = psnr(*v, occupancy=grid)
                n, P = grid.last_counts()
                r[k + "_dpsnr"], r[k + "_fine_share"] = p - dense[k], n / P
            rows.append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump({"dense": dense, "sigma_at_cell_centres": sigma, "rows": rows}, fp, indent=1)


if __name__ == "__main__":
    main()
