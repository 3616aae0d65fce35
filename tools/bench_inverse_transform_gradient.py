#!/usr/bin/env python3
"""
bench_inverse_transform_gradient.py -- times the gradient of deform_grid_inverse with respect to the deformation (ONE
library call for the displacement's and the inverse map's gradient: deform_grid.py _inverse_transform_gradient)
against deform_grid_inverse and deform_grid_inverse_gradient on the same arguments (5^3 control grid, sigma 5, order 3,
mode 'mirror'), with device events after warm-up:

    float32 128^3, float32 4 channels x 128^3, float32 256^3, float64 128^3

    python tools/bench_inverse_transform_gradient.py [--iters N] [--repeats R]
                                                     [--out profiles/inverse_transform_gradient_bench.txt]

Every variant is timed `repeats` times, alternating between the variants, each time over `iters` back-to-back calls
between two device events; one JSON line per variant: the median per-call time in microseconds, the smallest and the
largest of the repeats.  The tensors live on the device; a call is the host path of the public calls (the control
grid's prefilter, the volume's prefilter, the results' allocation, the transposed grid prefilter included).

A last line per shape relates the three: the new call's time over the forward's (whose cost is the solve this call
repeats) and over the image adjoint's, and the bytes of the fp64 u and q rows it writes and reads back
(2 x naxis x 8 bytes per voxel, once each way).  The per-channel increment is the 4-channel line against the
1-channel one.  There is no pass mark.

    --trace-only   one warm-up and `iters` calls of the new call on float32 128^3 and nothing else: the workload of a
                   kernel trace of its own (the share of points_grad_scatter).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import importlib  # noqa: E402

import elasticdeform_amd as ed  # noqa: E402

api = importlib.import_module("elasticdeform_amd.deform_grid")      # (the module, not the function)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def transform_gradient(Y, dZ, D, k):
    """the displacement's and the inverse map's gradient in one library call, as autograd's backward asks for them"""
    return api._inverse_transform_gradient(Y, dZ, D, k["order"], k["mode"], None, k.get("prefilter", True),
                                           k.get("axis"), None, None, None, 32, 1e-9, False, True, True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5, help="calls per timed window")
    p.add_argument("--repeats", type=int, default=21, help="timed windows per variant (median and spread)")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None)
    p.add_argument("--trace-only", action="store_true")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inverse_transform_gradient.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(0)
    D = torch.from_numpy(rng.standard_normal((3, 5, 5, 5)) * 5.0).cuda()
    S128, S256 = (128, 128, 128), (256, 256, 256)
    kw = dict(order=3, mode="mirror")

    def volume(shape, dtype):
        return torch.from_numpy(rng.uniform(0, 1, shape).astype(dtype)).cuda()

    if args.trace_only:
        Y, dZ = volume(S128, np.float32), volume(S128, np.float32)
        for _ in range(1 + args.iters):
            transform_gradient(Y, dZ, D, kw)
        torch.cuda.synchronize()
        return

    # name -> (Y, dZ: no crop, so both have the shape of X; deformed shape; keywords)
    shapes = {
        "128": (volume(S128, np.float32), volume(S128, np.float32), S128, kw),
        "128_4ch": (volume((4,) + S128, np.float32), volume((4,) + S128, np.float32), S128, dict(kw, axis=(1, 2, 3))),
        "256": (volume(S256, np.float32), volume(S256, np.float32), S256, kw),
        "128_f64": (volume(S128, np.float64), volume(S128, np.float64), S128, kw),
    }
    variants = {}
    for name, (Y, dZ, S, k) in shapes.items():
        variants["inverse_" + name] = lambda Y=Y, k=k: ed.deform_grid_inverse(Y, D, tuple(Y.shape), **k)
        variants["inverse_gradient_" + name] = lambda dZ=dZ, k=k: ed.deform_grid_inverse_gradient(dZ, D, **k)
        variants["inverse_transform_gradient_" + name] = lambda Y=Y, dZ=dZ, k=k: transform_gradient(Y, dZ, D, k)
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():           # alternating: drift hits every variant alike
            times[name].append(timed(fn, args.iters))
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    lines = []
    for name, ts in times.items():
        lines.append(json.dumps({
            "variant": name, "grid": [5, 5, 5], "sigma": 5.0, "order": 3, "mode": "mirror",
            "median_us": round(med[name], 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
            "iters": args.iters, "repeats": args.repeats}))
        print(lines[-1], flush=True)
    for name, (Y, dZ, S, k) in shapes.items():
        fwd, adj, new = (med[v + name] for v in ("inverse_", "inverse_gradient_", "inverse_transform_gradient_"))
        row_bytes = int(np.prod(S)) * 2 * 3 * 8
        lines.append(json.dumps({
            "shape": name, "dtype": str(Y.dtype).replace("torch.", ""),
            "transform_gradient_over_inverse": round(new / fwd, 3),
            "transform_gradient_over_inverse_gradient": round(new / adj, 3), "excess_over_inverse_us": round(new - fwd, 1),
            "row_bytes": row_bytes, "workspace_MB": round(row_bytes / 1e6, 1)}))
        print(lines[-1], flush=True)
    lines.append(json.dumps({
        "per_channel_increment_us": {v: round((med[v + "_128_4ch"] - med[v + "_128"]) / 3.0, 1)
                                     for v in ("inverse", "inverse_gradient", "inverse_transform_gradient")}}))
    print(lines[-1], flush=True)
    lines.append(json.dumps({"device": torch.cuda.get_device_name(0)}))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
