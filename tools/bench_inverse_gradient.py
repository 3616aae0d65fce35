#!/usr/bin/env python3
"""
bench_inverse_gradient.py -- times deform_grid_inverse_gradient against deform_grid_inverse on the same arguments (5^3
control grid, sigma 5, order 3, mode 'mirror'), with device events after warm-up:

    float32 128^3, float32 4 channels x 128^3, float32 256^3, float64 128^3

and, on float32 128^3, both calls with prefilter=False (the kernels without the volume's filter passes).

    python tools/bench_inverse_gradient.py [--iters N] [--repeats R] [--out profiles/inverse_gradient_bench.txt]

Every variant is timed `repeats` times, alternating between the variants, each time over `iters` back-to-back calls
between two device events; one JSON line per variant: the median per-call time in microseconds, the smallest and the
largest of the repeats.  The tensors live on the device; a call is the public call (the control grid's prefilter, the
volume's prefilter -- transposed for the gradient -- and the result's allocation, zeroed for the gradient, included).

A last line per shape relates the two: the gradient's time over the forward's, the bytes its float atomics add
(solved voxels x 64 taps x channels x element size), the time those bytes take at 1.3 TB/s, the chip-wide rate of
4-byte float atomics, and the gradient's excess over the forward.  There is no pass mark.
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

ATOMIC_RATE = 1.3e12        # bytes per second, 4-byte float atomics in contiguous wave instructions


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5, help="calls per timed window")
    p.add_argument("--repeats", type=int, default=21, help="timed windows per variant (median and spread)")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inverse_gradient.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(0)
    D = torch.from_numpy(rng.standard_normal((3, 5, 5, 5)) * 5.0).cuda()
    S128, S256 = (128, 128, 128), (256, 256, 256)
    kw = dict(order=3, mode="mirror")

    def volume(shape, dtype):
        return torch.from_numpy(rng.uniform(0, 1, shape).astype(dtype)).cuda()

    # name -> (array in the frame of Y and of X alike: no crop, deformed shape, keywords)
    shapes = {
        "128": (volume(S128, np.float32), S128, kw),
        "128_4ch": (volume((4,) + S128, np.float32), S128, dict(kw, axis=(1, 2, 3))),
        "256": (volume(S256, np.float32), S256, kw),
        "128_f64": (volume(S128, np.float64), S128, kw),
        "128_no_prefilter": (volume(S128, np.float32), S128, dict(kw, prefilter=False)),
    }
    variants, solved = {}, {}
    for name, (V, S, k) in shapes.items():
        variants["inverse_" + name] = lambda V=V, k=k: ed.deform_grid_inverse(V, D, tuple(V.shape), **k)
        variants["inverse_gradient_" + name] = lambda V=V, k=k: ed.deform_grid_inverse_gradient(V, D, **k)
        if S not in solved:
            # the solved voxels, as the forward marks them: in 'mirror' exactly they have taps
            ones = torch.ones(S, dtype=torch.float32, device="cuda")
            Z = ed.deform_grid_inverse(ones, D, S, order=1, mode="mirror", cval=0.0)
            solved[S] = int((Z != 0).sum())
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
    for name, (V, S, k) in shapes.items():
        fwd, grad = med["inverse_" + name], med["inverse_gradient_" + name]
        channels = int(V.numel() // int(np.prod(S)))
        atomic_bytes = solved[S] * 64 * channels * V.element_size()
        lines.append(json.dumps({
            "shape": name, "dtype": str(V.dtype).replace("torch.", ""), "gradient_over_inverse": round(grad / fwd, 3),
            "excess_us": round(grad - fwd, 1), "atomic_bytes": atomic_bytes,
            "atomic_us_at_1.3TBps": round(atomic_bytes / ATOMIC_RATE * 1e6, 1),
            "atomic_GBps_over_whole_call": round(atomic_bytes / grad * 1e-3, 1),
            "solved_share": round(solved[S] / float(np.prod(S)), 6)}))
        print(lines[-1], flush=True)
    lines.append(json.dumps({"device": torch.cuda.get_device_name(0)}))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
