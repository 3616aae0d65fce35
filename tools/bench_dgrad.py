#!/usr/bin/env python3
"""
bench_dgrad.py -- times deform_grid_displacement_gradient against deform_grid and deform_grid_gradient on the
same arguments, with device events after warm-up, and the gradient with respect to the affine part: affine only
(deform_grid_affine_gradient) and combined (displacement and affine from one library call):

    cfg2   256^3 float32, 5^3 grid, sigma 5, order 3, mirror
    cfg3   128^3 float32, same grid
    2d     512^2 float32, 5^2 grid

    python tools/bench_dgrad.py [--iters N] [--out profiles/dgrad_bench.txt] [--affine]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_dgrad.py --iters 5 --trace

Prints one line per case (mean / min call time in microseconds) and, for the displacement gradient's row
kernel, the bytes and operations it needs by shape (HBM vs VALU bound).
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
import importlib  # noqa: E402

_dg = importlib.import_module("elasticdeform_amd.deform_grid")

CASES = {
    "cfg2": ((256, 256, 256), (5, 5, 5)),
    "cfg3": ((128, 128, 128), (5, 5, 5)),
    "2d": ((512, 512), (5, 5)),
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


def model(shape, ncp, order=3):
    """bytes / operations of the row kernel by shape: every voxel reads dY (4 B) and (order+1)^n taps of C,
    which reach HBM about once (the source box of a row stays in L2); fp64 work per voxel: coordinates,
    weights and their derivatives, 4 x naxis taps of Q; fp32 tap work: 2 FMA per tap innermost."""
    n = len(shape)
    vox = float(np.prod(shape))
    taps = (order + 1) ** n
    hbm = vox * (4 + 4)
    fp32 = vox * (2 * taps + 3 * (order + 1) ** (n - 1))
    fp64 = vox * (n * 80 + 4 * n * 2)
    return dict(voxels=vox, hbm_bytes=hbm, fp32_flops=2 * fp32, fp64_flops=2 * fp64,
                hbm_us_at_8TBs=hbm / 8e12 * 1e6, fp32_us_at_157TF=2 * fp32 / 157e12 * 1e6,
                fp64_us_at_79TF=2 * fp64 / 78.6e12 * 1e6)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--out", default=None)
    p.add_argument("--trace", action="store_true", help="a short run for rocprofv3 (no model lines)")
    p.add_argument("--affine", action="store_true",
                   help="displacement-only vs affine-only vs combined (profiles/agrad_bench.txt)")
    args = p.parse_args()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    lines = []
    for name, (shape, ncp) in CASES.items():
        X = torch.rand(shape, device="cuda", dtype=torch.float32)
        dY = torch.rand(shape, device="cuda", dtype=torch.float32)
        D = torch.from_numpy(rng.standard_normal((len(shape),) + ncp) * 5).cuda()
        kw = dict(order=3, mode="mirror")
        res = {"case": name, "shape": list(shape), "grid": list(ncp)}
        n = len(shape)
        A = np.concatenate([np.eye(n) + 0.01 * rng.standard_normal((n, n)), 0.3 * rng.standard_normal((n, 1))], 1)
        akw = dict(kw, affine=A)
        cases = (("deform_grid", lambda: ed.deform_grid(X, D, **kw)),
                 ("deform_grid_gradient", lambda: ed.deform_grid_gradient(dY, D, **kw)),
                 ("displacement_gradient", lambda: ed.deform_grid_displacement_gradient(X, dY, D, **kw)))
        if args.affine:
            cases = (("displacement_gradient", lambda: ed.deform_grid_displacement_gradient(X, dY, D, **akw)),
                     ("affine_gradient", lambda: ed.deform_grid_affine_gradient(X, dY, D, **akw)),
                     ("combined", lambda: _dg._transform_gradient(X, dY, D, want_disp=True, want_map=True, **akw)))
        for label, fn in cases:
            mean, best = time_call(fn, args.iters)
            res[label + "_us"] = round(mean, 1)
            res[label + "_min_us"] = round(best, 1)
        if args.affine:
            res["affine_vs_displacement"] = round(res["affine_gradient_us"] / res["displacement_gradient_us"], 3)
            res["combined_vs_displacement"] = round(res["combined_us"] / res["displacement_gradient_us"], 3)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            continue
        res["ratio_vs_deform_grid"] = round(res["displacement_gradient_us"] / res["deform_grid_us"], 2)
        if not args.trace:
            res["model"] = {k: (round(v, 1) if isinstance(v, float) else v) for k, v in model(shape, ncp).items()}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
