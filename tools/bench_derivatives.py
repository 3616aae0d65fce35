#!/usr/bin/env python3
"""
bench_derivatives.py -- times the coordinate map's derivatives at sampled positions, with device events after warm-up,
for 2^12 .. 2^18 uniform positions in a 128^3 frame on a 5^3 float64 control grid:

    (a) derivatives             deform_grid_derivatives (r, J, H)
    (b) derivatives_no_hessian  deform_grid_derivatives(hessian=False) (r, J)
    (c) derivatives_gradient    deform_grid_derivatives_gradient with all three cotangents (points, displacement and
                                inverse map, one call)
    (d) coordinates             deform_grid_coordinates(jacobian=True): the same r and J from the call there was
    (e) coordinates_gradient    deform_grid_coordinates_gradient: the adjoint of r alone
    (f) jacobian_lattice        deform_grid_jacobian + deform_grid_jacobian_gradient on the whole 128^3 lattice: what a
                                regulariser cost before it could be sampled (once per run, it does not depend on N)

    python tools/bench_derivatives.py [--iters N] [--repeats R] [--log2 12 .. 18] [--out profiles/derivatives_points.txt]

Every figure is the public call on device tensors (the control grid's prefilter and the results' allocation included).
A repeat times consecutive calls between two events -- at least `iters` of them and enough for `window-ms` of work per
window --; the repeats of the calls alternate, and a line reports the median and the spread (min, max) of the repeats in
microseconds per call.  One JSON line per number of points.
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


def measure(calls, args):
    """{name: (median, min, max) us per call}, {name: calls per window}"""
    for fn in calls.values():                                    # warm-up: code objects, workspaces, plans
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    iters = {k: max(args.iters, min(2000, int(np.ceil(args.window_ms * 1e3 / window_us(fn, args.iters)))))
             for k, fn in calls.items()}
    times = {k: [] for k in calls}
    for _ in range(args.repeats):
        for k, fn in calls.items():
            times[k].append(window_us(fn, iters[k]))
    return {k: (float(np.median(t)), float(min(t)), float(max(t))) for k, t in times.items()}, iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--window-ms", type=float, default=25.0)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--log2", type=int, nargs="+", default=list(range(12, 19)))
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_derivatives.py needs a GPU: there is nothing to time without one")
    size = args.size
    shape = (size,) * 3
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    D = torch.from_numpy(rng.standard_normal((3, 5, 5, 5)) * (size / 40.0)).cuda()
    lines = []

    g = torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)
    lattice, it = measure({"jacobian": lambda: ed.deform_grid_jacobian(D, shape),
                           "jacobian_gradient": lambda: ed.deform_grid_jacobian_gradient(g, D, shape)}, args)
    res = {"volume": list(shape), "grid": [5, 5, 5], "lattice": True, "calls_per_window": it, "repeats": args.repeats}
    for k, t in lattice.items():
        res[k + "_us"] = round(t[0], 1)
        res[k + "_min_max_us"] = [round(t[1], 1), round(t[2], 1)]
    res["jacobian_lattice_us"] = round(lattice["jacobian"][0] + lattice["jacobian_gradient"][0], 1)
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    del g

    for e in args.log2:
        N = 1 << e
        q = torch.rand((N, 3), dtype=torch.float64, device="cuda", generator=gen) * (size - 1)
        u = torch.randn((N, 3), dtype=torch.float64, device="cuda", generator=gen)
        A = torch.randn((N, 3, 3), dtype=torch.float64, device="cuda", generator=gen)
        G = torch.randn((N, 3, 3, 3), dtype=torch.float64, device="cuda", generator=gen)
        calls = {
            "derivatives": lambda: ed.deform_grid_derivatives(q, D, shape),
            "derivatives_no_hessian": lambda: ed.deform_grid_derivatives(q, D, shape, hessian=False),
            "derivatives_gradient": lambda: ed.deform_grid_derivatives_gradient(q, D, shape, u, A, G),
            "coordinates": lambda: ed.deform_grid_coordinates(q, D, shape, jacobian=True),
            "coordinates_gradient": lambda: ed.deform_grid_coordinates_gradient(q, u, D, shape),
        }
        # the two forwards agree bit for bit (tests/test_derivatives.py asserts it; this guards the comparison)
        same = bool(torch.equal(calls["derivatives"]().jacobian, calls["coordinates"]()[1]))
        times, it = measure(calls, args)
        res = {"points": N, "volume": list(shape), "grid": [5, 5, 5], "calls_per_window": it, "repeats": args.repeats,
               "jacobian_bits_equal": same}
        for k, t in times.items():
            res[k + "_us"] = round(t[0], 1)
            res[k + "_min_max_us"] = [round(t[1], 1), round(t[2], 1)]
        res["forward_plus_backward_us"] = round(times["derivatives"][0] + times["derivatives_gradient"][0], 1)
        res["lattice_over_sampled"] = round((lattice["jacobian"][0] + lattice["jacobian_gradient"][0])
                                            / (times["derivatives"][0] + times["derivatives_gradient"][0]), 2)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
