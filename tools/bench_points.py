#!/usr/bin/env python3
"""
bench_points.py -- times deform_grid_coordinates (forward) and deform_points (inverse) on float64 points, with
device events after warm-up, next to deform_grid on a float32 volume of as many voxels (order 3, mirror: the
yardstick -- the image call does per voxel what the forward map does per point, plus the interpolation):

    2-D   N = 2^16, 2^20, 2^24 points      256^2, 1024^2, 4096^2 volume, 5^2 grid
    3-D   the same N                       32x32x64, 64x128x128, 256^3 volume, 5^3 grid

    python tools/bench_points.py [--iters N] [--out profiles/points_bench.txt]

One JSON line per case: mean / min call time in microseconds (the public call: the control grid's prefilter and the
result's allocation included), the ratio to the yardstick, nanoseconds per point, and for the inverse the Newton
steps the points needed -- from calls with max_iter = 1, 2, ... on the smallest N: the share solved within k steps.
The displacement is sigma = extent / 40 on every axis (a mild, invertible field: every point is solved).
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


def steps_needed(P, D, shape, upto=12):
    """share of the points solved within k Newton steps, k = 1 .. (until all are)"""
    shares = []
    for k in range(1, upto + 1):
        _, ok = ed.deform_points(P, D, shape, max_iter=k, return_converged=True)
        shares.append(round(float(ok.double().mean()), 4))
        if shares[-1] == 1.0:
            break
    return shares


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
        for k, shape in SHAPES[n].items():
            if k > args.max_log2:
                continue
            N = 1 << k
            assert int(np.prod(shape)) == N
            D = torch.from_numpy(rng.standard_normal((n,) + (5,) * n) * (min(shape) / 40.0)).cuda()
            ext = torch.tensor([s - 1.0 for s in shape], dtype=torch.float64, device="cuda")
            P = torch.rand((N, n), dtype=torch.float64, device="cuda", generator=gen) * ext
            X = torch.rand(shape, dtype=torch.float32, device="cuda", generator=gen)
            res = {"naxis": n, "points": N, "volume": list(shape)}
            image, image_min = time_call(lambda: ed.deform_grid(X, D, order=3, mode="mirror"), args.iters)
            fwd, fwd_min = time_call(lambda: ed.deform_grid_coordinates(P, D, shape), args.iters)
            jac, jac_min = time_call(lambda: ed.deform_grid_coordinates(P, D, shape, jacobian=True), args.iters)
            inv, inv_min = time_call(lambda: ed.deform_points(P, D, shape), args.iters)
            _, ok = ed.deform_points(P, D, shape, return_converged=True)
            res.update(deform_grid_us=round(image, 1), deform_grid_min_us=round(image_min, 1),
                       forward_us=round(fwd, 1), forward_min_us=round(fwd_min, 1),
                       forward_jacobian_us=round(jac, 1), forward_jacobian_min_us=round(jac_min, 1),
                       inverse_us=round(inv, 1), inverse_min_us=round(inv_min, 1),
                       forward_vs_deform_grid=round(fwd / image, 3), inverse_vs_deform_grid=round(inv / image, 3),
                       inverse_vs_forward=round(inv / fwd, 2),
                       forward_ns_per_point=round(fwd * 1e3 / N, 3), inverse_ns_per_point=round(inv * 1e3 / N, 3),
                       solved=round(float(ok.double().mean()), 6))
            if k == min(SHAPES[n]):
                res["solved_within_k_steps"] = steps_needed(P, D, shape)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            del P, X
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
