#!/usr/bin/env python3
"""
bench_points_gradient.py -- times deform_grid_coordinates_gradient (forward direction) and deform_points_gradient
(inverse direction, the solved positions handed in: the gradient's own three launches, no second solve) on float64
points, with device events after warm-up, next to the calls they differentiate at the same N (the yardstick:
deform_grid_coordinates / deform_points):

    2-D   N = 2^16, 2^20, 2^24 points      256^2, 1024^2, 4096^2 extent, a 5^2 grid and a 64^2 grid
    3-D   the same N                       32x32x64, 64x128x128, 256^3 extent, a 5^3 grid

    python tools/bench_points_gradient.py [--iters N] [--max-log2 K] [--out profiles/points_gradient_bench.txt]

One JSON line per case: mean / min call time in microseconds of the public calls (the control grid's prefilter, the
transposed prefilter and the results' allocation included), the gradient's time over its yardstick's, and nanoseconds
per point.  The 5^n grids keep the gradient's cells in LDS; the 64^2 grid (8192 values) puts them in global memory.
The displacement is sigma = extent / 40 per control spacing of the 5^n grid (a mild, invertible field).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import elasticdeform_amd as ed  # noqa: E402

SHAPES = {
    2: {16: (256, 256), 20: (1024, 1024), 24: (4096, 4096)},
    3: {16: (32, 32, 64), 20: (64, 128, 128), 24: (256, 256, 256)},
}


def time_call(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.mean(times)), float(np.min(times))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--out", default=None)
    p.add_argument("--max-log2", type=int, default=24, help="largest N = 2^k to run")
    args = p.parse_args()
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = []
    for n in (2, 3):
        grids = [(5,) * n] + ([(64, 64)] if n == 2 else [])
        for k, shape in SHAPES[n].items():
            if k > args.max_log2:
                continue
            N = 1 << k
            ext = torch.tensor([s - 1.0 for s in shape], dtype=torch.float64, device="cuda")
            P = torch.rand((N, n), dtype=torch.float64, device="cuda", generator=gen) * ext
            G = torch.randn((N, n), dtype=torch.float64, device="cuda", generator=gen)
            for ncp in grids:
                sigma = min(shape) / 40.0 * 4.0 / (max(ncp) - 1)
                D = torch.from_numpy(rng.standard_normal((n,) + ncp) * sigma).cuda()
                Q, ok = ed.deform_points(P, D, shape, return_converged=True)
                res = {"naxis": n, "points": N, "extent": list(shape), "grid": list(ncp),
                       "solved": round(float(ok.double().mean()), 6)}
                fwd, fwd_min = time_call(lambda: ed.deform_grid_coordinates(P, D, shape), args.iters)
                inv, inv_min = time_call(lambda: ed.deform_points(P, D, shape), args.iters)
                gf, gf_min = time_call(lambda: ed.deform_grid_coordinates_gradient(P, G, D, shape), args.iters)
                gi, gi_min = time_call(lambda: ed.deform_points_gradient(P, G, D, shape, positions=Q), args.iters)
                res.update(forward_us=round(fwd, 1), forward_min_us=round(fwd_min, 1),
                           inverse_us=round(inv, 1), inverse_min_us=round(inv_min, 1),
                           forward_gradient_us=round(gf, 1), forward_gradient_min_us=round(gf_min, 1),
                           inverse_gradient_us=round(gi, 1), inverse_gradient_min_us=round(gi_min, 1),
                           forward_gradient_vs_forward=round(gf / fwd, 2),
                           inverse_gradient_vs_inverse=round(gi / inv, 2),
                           forward_gradient_ns_per_point=round(gf * 1e3 / N, 3),
                           inverse_gradient_ns_per_point=round(gi * 1e3 / N, 3))
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
                del Q
            del P, G
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
