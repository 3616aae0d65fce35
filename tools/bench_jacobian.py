#!/usr/bin/env python3
"""
bench_jacobian.py -- times det J on the voxel lattice, with device events after warm-up, at 128^3 and 256^3 on a 5^3
float64 control grid:

    (a) jacobian            deform_grid_jacobian
    (b) coordinates_det     the route there was before: deform_grid_coordinates on the voxel lattice with
                            jacobian=True, then torch.linalg.det (the lattice of positions is built once, outside the
                            timed window)
    (c) jacobian_gradient   deform_grid_jacobian_gradient (displacement and inverse map, one call)
    (d) deform_grid         deform_grid on a float32 volume of the shape, order 3, mirror: a yardstick only

    python tools/bench_jacobian.py [--iters N] [--repeats R] [--sizes 128 256] [--out profiles/jacobian_bench.txt]

Every figure is the public call (the control grid's prefilter and the result's allocation included).  A repeat times
consecutive calls between two events -- at least `iters` of them and enough for `window-ms` of work per window --; the
repeats of (a) .. (d) alternate, and a line reports the median and the spread (min, max) of the repeats in
microseconds per call.  `--wide 8 16 64` also times (a) and (c) on 5 x 5 x N grids (other strides of the dense rows in
LDS; with 64 points the gradient's units reach a window of the last axis and the forward runs per voxel).  One JSON line per size; `a_not_slower_than_b` is the
acceptance of the row contraction.
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
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--window-ms", type=float, default=25.0)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    p.add_argument("--wide", type=int, nargs="*", default=[], help="also time (a) and (c) on 5 x 5 x N grids")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jacobian.py needs a GPU: there is nothing to time without one")
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = []
    for size in args.sizes:
        shape = (size,) * 3
        D = torch.from_numpy(rng.standard_normal((3, 5, 5, 5)) * (size / 40.0)).cuda()
        axes = [torch.arange(size, dtype=torch.float64, device="cuda")] * 3
        lattice = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
        X = torch.rand(shape, dtype=torch.float32, device="cuda", generator=gen)
        g = torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)

        def route_b():
            _, J = ed.deform_grid_coordinates(lattice, D, shape, jacobian=True)
            return torch.linalg.det(J)

        calls = {
            "jacobian": lambda: ed.deform_grid_jacobian(D, shape),
            "coordinates_det": route_b,
            "jacobian_gradient": lambda: ed.deform_grid_jacobian_gradient(g, D, shape),
            "deform_grid": lambda: ed.deform_grid(X, D, order=3, mode="mirror"),
        }
        # the two routes agree (the bound of tests/test_jacobian.py is tighter; this guards the comparison)
        diff = float((calls["jacobian"]() - route_b().reshape(shape)).abs().max())
        for fn in calls.values():                                # warm-up: code objects, workspaces, plans
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # calls per window: at least --iters, and enough of them for --window-ms of work (a short window times the
        # clock and the scheduler)
        iters = {k: max(args.iters, min(2000, int(np.ceil(args.window_ms * 1e3 / window_us(fn, args.iters)))))
                 for k, fn in calls.items()}
        times = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, fn in calls.items():
                times[k].append(window_us(fn, iters[k]))
        res = {"volume": list(shape), "grid": [5, 5, 5], "calls_per_window": iters, "repeats": args.repeats,
               "max_abs_difference_a_b": diff}
        for k, t in times.items():
            res[k + "_us"] = round(float(np.median(t)), 1)
            res[k + "_min_max_us"] = [round(float(min(t)), 1), round(float(max(t)), 1)]
        res["b_over_a"] = round(res["coordinates_det_us"] / res["jacobian_us"], 2)
        res["a_not_slower_than_b"] = bool(res["jacobian_us"] <= res["coordinates_det_us"])
        res["jacobian_ns_per_voxel"] = round(res["jacobian_us"] * 1e3 / size ** 3, 4)
        res["jacobian_gradient_ns_per_voxel"] = round(res["jacobian_gradient_us"] * 1e3 / size ** 3, 4)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        for ncp in args.wide:
            # a fine last grid axis: the forward's row contraction up to 56 points, its per-voxel route beyond; the
            # gradient's units reach a window of the axis
            Dw = torch.from_numpy(rng.standard_normal((3, 5, 5, ncp)) * (size / 40.0 * 4.0 / (ncp - 1))).cuda()
            wide = {"jacobian": lambda: ed.deform_grid_jacobian(Dw, shape),
                    "jacobian_gradient": lambda: ed.deform_grid_jacobian_gradient(g, Dw, shape)}
            for fn in wide.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            it = {k: max(args.iters, min(2000, int(np.ceil(args.window_ms * 1e3 / window_us(fn, args.iters)))))
                  for k, fn in wide.items()}
            tw = {k: [] for k in wide}
            for _ in range(args.repeats):
                for k, fn in wide.items():
                    tw[k].append(window_us(fn, it[k]))
            resw = {"volume": list(shape), "grid": [5, 5, ncp], "calls_per_window": it, "repeats": args.repeats}
            for k, t in tw.items():
                resw[k + "_us"] = round(float(np.median(t)), 1)
                resw[k + "_min_max_us"] = [round(float(min(t)), 1), round(float(max(t)), 1)]
            lines.append(json.dumps(resw))
            print(lines[-1], flush=True)
        del lattice, X, g
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
