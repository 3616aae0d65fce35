#!/usr/bin/env python3
"""
bench_inverse.py -- times deform_grid_inverse on a float32 128^3 volume (5^3 control grid, sigma 5, order 3, mode
'mirror'), with device events after warm-up, next to the two existing pieces it fuses:

    (a) inverse          deform_grid_inverse(Y, D, shape)                 solve per voxel + gather, one kernel
    (b) points           deform_points(lattice, D, shape)                 the solve alone: float64 lattice in (24 B per
                                                                          voxel), float64 positions out (24 B)
    (c) forward exact    deform_grid(Y, D) under set_arithmetic('exact')  the reference-order gather alone (its
                                                                          coordinate is a spline evaluation, no solve)

and deform_grid_inverse on 256^3 and on a 4-channel 128^3 volume (the solve is shared by the channels).

    python tools/bench_inverse.py [--iters N] [--repeats R] [--out profiles/inverse_bench.txt]

Every variant is timed `repeats` times, alternating between the variants, each time over `iters` back-to-back calls
between two device events; one JSON line per variant: the median per-call time in microseconds, the smallest and the
largest of the repeats.  The tensors live on the device; a call is the public call (the prefilter of the volume and of
the control grid and the result's allocation included); "inverse_128_no_prefilter" leaves the volume's prefilter out.
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


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def forward_exact(Y, D):
    ed.set_arithmetic("exact")
    try:
        return ed.deform_grid(Y, D, order=3, mode="mirror")
    finally:
        ed.set_arithmetic("auto")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5, help="calls per timed window")
    p.add_argument("--repeats", type=int, default=21, help="timed windows per variant (median and spread)")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inverse.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(0)
    D = torch.from_numpy(rng.standard_normal((3, 5, 5, 5)) * 5.0).cuda()
    S128, S256 = (128, 128, 128), (256, 256, 256)
    Y128 = torch.from_numpy(rng.uniform(0, 1, S128).astype(np.float32)).cuda()
    Y256 = torch.from_numpy(rng.uniform(0, 1, S256).astype(np.float32)).cuda()
    Y4 = torch.from_numpy(rng.uniform(0, 1, (4,) + S128).astype(np.float32)).cuda()
    lattice = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64, device="cuda") for s in S128],
                                         indexing="ij"), dim=-1).reshape(-1, 3)
    kw = dict(order=3, mode="mirror")
    Yf = Y128                        # (taken as spline coefficients: the time does not depend on the values)
    variants = {
        "inverse_128": lambda: ed.deform_grid_inverse(Y128, D, S128, **kw),
        "inverse_128_with_valid": lambda: ed.deform_grid_inverse(Y128, D, S128, return_valid=True, **kw),
        "inverse_128_no_prefilter": lambda: ed.deform_grid_inverse(Yf, D, S128, prefilter=False, **kw),
        "points_128": lambda: ed.deform_points(lattice, D, S128),
        "forward_exact_128": lambda: forward_exact(Y128, D),
        "inverse_256": lambda: ed.deform_grid_inverse(Y256, D, S256, **kw),
        "inverse_128_4ch": lambda: ed.deform_grid_inverse(Y4, D, (4,) + S128, axis=(1, 2, 3), **kw),
    }
    _, valid = ed.deform_grid_inverse(Y128, D, S128, return_valid=True, **kw)
    _, ok = ed.deform_points(lattice, D, S128, return_converged=True)
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
            "variant": name, "grid": [5, 5, 5], "sigma": 5.0, "order": 3, "mode": "mirror", "dtype": "float32",
            "median_us": round(med[name], 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
            "iters": args.iters, "repeats": args.repeats}))
        print(lines[-1], flush=True)
    lines.append(json.dumps({
        "inverse_128_over_points_plus_forward_exact": round(med["inverse_128"] / (med["points_128"]
                                                                                  + med["forward_exact_128"]), 3),
        "inverse_128_4ch_over_4x_inverse_128": round(med["inverse_128_4ch"] / (4 * med["inverse_128"]), 3),
        "inverse_256_over_8x_inverse_128": round(med["inverse_256"] / (8 * med["inverse_128"]), 3),
        "valid_share_128": round(float(valid.double().mean()), 4), "solved_share_128": round(float(ok.double().mean()), 6),
        "device": torch.cuda.get_device_name(0)}))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
