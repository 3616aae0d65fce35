#!/usr/bin/env python3
"""
sample_bench.py -- times a sampled loss on a deformed image, value and gradients, with device events after warm-up:
N = 2^12, 2^15, 2^18 uniformly random positions in a 128^3 float32 volume, control grid 5^3 (float64, sigma 5), mode
'nearest', tensors resident.

    (a) sample        deform_grid_sample + deform_grid_sample_gradient + deform_grid_sample_points_gradient, order 3
                      and order 1 (the volume's prefilter included: it is part of the public call)
    (b) what there was before:
        order 1       deform_grid_coordinates + torch.nn.functional.grid_sample (bilinear, align_corners=True,
                      padding_mode='border') with its autograd (the gradients of the volume and of the coordinates) +
                      deform_grid_coordinates_gradient
        order 3       the full-volume deform_grid + deform_grid_gradient + deform_grid_displacement_gradient

    python tools/sample_bench.py [--iters N] [--repeats R] [--points 4096 32768 262144] [--out profiles/sample_points.txt]

A repeat times consecutive calls between two events -- at least `iters` of them and enough for `window-ms` of work per
window --; the repeats of the routes alternate, and a line reports the median and the spread (min, max) of the repeats
in microseconds per call.  One JSON line per N.
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


def window_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=25.0)
    p.add_argument("--repeats", type=int, default=21)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--points", type=int, nargs="+", default=[2 ** 12, 2 ** 15, 2 ** 18])
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench.py needs a GPU: there is nothing to time without one")
    size = args.size
    shape = (size,) * 3
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    D = torch.from_numpy(rng.standard_normal((3, 5, 5, 5)) * 5.0).cuda()
    X = torch.rand(shape, dtype=torch.float32, device="cuda", generator=gen)
    dY = torch.randn(shape, dtype=torch.float32, device="cuda", generator=gen)
    scale = torch.tensor([2.0 / (size - 1)] * 3, dtype=torch.float64, device="cuda")
    lines = []

    def full_volume():
        ed.deform_grid(X, D, order=3, mode="nearest")
        ed.deform_grid_gradient(dY, D, order=3, mode="nearest")
        ed.deform_grid_displacement_gradient(X, dY, D, order=3, mode="nearest")

    for N in args.points:
        q = torch.rand((N, 3), dtype=torch.float64, device="cuda", generator=gen) * (size - 1)
        dV = torch.randn((N,), dtype=torch.float32, device="cuda", generator=gen)

        def sample(order):
            ed.deform_grid_sample(X, q, D, order=order, mode="nearest")
            ed.deform_grid_sample_gradient(dV, q, D, shape, order=order, mode="nearest")
            ed.deform_grid_sample_points_gradient(X, dV, q, D, order=order, mode="nearest")

        def composition():
            r = ed.deform_grid_coordinates(q, D, shape)
            # grid_sample wants (x, y, z) in [-1, 1], float32, and a (1, C, D, H, W) volume
            r = r.detach().requires_grad_()
            grid = (r * scale - 1.0).flip(-1).to(torch.float32).reshape(1, 1, 1, N, 3)
            x = X.reshape((1, 1) + shape).requires_grad_()
            v = torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=True)
            dx, dr = torch.autograd.grad(v.reshape(N), (x, r), dV)
            ed.deform_grid_coordinates_gradient(q, dr, D, shape)

        calls = {"sample_order3": lambda: sample(3), "sample_order1": lambda: sample(1),
                 "coordinates_grid_sample_order1": composition, "full_volume_order3": full_volume}
        # the two order-1 routes agree inside the volume (float32 coordinates on the composition's side)
        v1 = ed.deform_grid_sample(X, q, D, order=1, mode="nearest")
        r = ed.deform_grid_coordinates(q, D, shape)
        grid = (r * scale - 1.0).flip(-1).to(torch.float32).reshape(1, 1, 1, N, 3)
        v2 = torch.nn.functional.grid_sample(X.reshape((1, 1) + shape), grid, mode="bilinear", padding_mode="border",
                                             align_corners=True).reshape(N)
        diff = float((v1 - v2).abs().max())
        for fn in calls.values():                                # warm-up: code objects, workspaces, plans
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        iters = {k: max(args.iters, min(2000, int(np.ceil(args.window_ms * 1e3 / window_us(fn, args.iters)))))
                 for k, fn in calls.items()}
        times = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, fn in calls.items():
                times[k].append(window_us(fn, iters[k]))
        res = {"volume": list(shape), "grid": [5, 5, 5], "points": N, "calls_per_window": iters,
               "repeats": args.repeats, "max_abs_difference_order1_routes": diff}
        for k, t in times.items():
            res[k + "_us"] = round(float(np.median(t)), 1)
            res[k + "_min_max_us"] = [round(float(min(t)), 1), round(float(max(t)), 1)]
        res["sample_not_slower_than_composition_order1"] = bool(
            res["sample_order1_us"] <= res["coordinates_grid_sample_order1_us"])
        res["full_volume_over_sample_order3"] = round(res["full_volume_order3_us"] / res["sample_order3_us"], 2)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
