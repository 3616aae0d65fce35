#!/usr/bin/env python3
"""
bench_labels.py -- times deform_grid_labels on a 128^3 uint8 label map (5^3 control grid, sigma 5, mode 'nearest'), with
device events after warm-up, next to the two things a user can write without it:

    (a) labels      deform_grid_labels(L, D)                                       one gather pass over the integer map
    (b) one-hot C   C calls of deform_grid on float32 one-hot channels, order 1, and a running argmax in torch, for
                    C = 4 and C = 16 (the channels are built outside the timed region: only the resampling counts)
    (c) order 0     deform_grid(L, D, order=0)                                     the nearest source voxel

    python tools/bench_labels.py [--iters N] [--repeats R] [--out profiles/labels_bench.txt]

Every variant is timed `repeats` times, alternating between the variants, each time over `iters` back-to-back calls
between two device events; one JSON line per variant: the median per-call time in microseconds, the smallest and the
largest of the repeats, and the ratio to (a).  The tensors live on the device; a call is the public call (the control
grid's prefilter and the result's allocation included).
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

SHAPE = (128, 128, 128)


def one_hot_argmax(channels, D):
    """what a user writes today: deform every class channel with order 1, keep the running argmax"""
    best = label = None
    for c, ch in enumerate(channels):
        s = ed.deform_grid(ch, D, order=1, mode="nearest")
        if best is None:
            best, label = s, torch.zeros(s.shape, dtype=torch.uint8, device=s.device)
        else:
            upd = s > best
            label = torch.where(upd, torch.full_like(label, c), label)
            best = torch.where(upd, s, best)
    return label


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
    p.add_argument("--iters", type=int, default=20, help="calls per timed window")
    p.add_argument("--repeats", type=int, default=7, help="timed windows per variant (median and spread)")
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_labels.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(0)
    D = torch.from_numpy(rng.standard_normal((3, 5, 5, 5)) * 5.0).cuda()
    variants = {}
    maps = {}
    for C in (4, 16):
        maps[C] = torch.from_numpy(rng.integers(0, C, SHAPE).astype(np.uint8)).cuda()
        channels = [(maps[C] == c).to(torch.float32) for c in range(C)]
        variants["one_hot_C%d" % C] = lambda ch=channels: one_hot_argmax(ch, D)
        variants["labels_C%d" % C] = lambda L=maps[C]: ed.deform_grid_labels(L, D, mode="nearest")
    variants["labels_with_weight_C4"] = lambda: ed.deform_grid_labels(maps[4], D, mode="nearest", return_weight=True)
    variants["order0_C4"] = lambda: ed.deform_grid(maps[4], D, order=0, mode="nearest")
    # the one-hot route computes the same thing (float32 scores instead of float64 ones: a near tie may differ)
    same = float((one_hot_argmax([(maps[4] == c).to(torch.float32) for c in range(4)], D)
                  == ed.deform_grid_labels(maps[4], D, mode="nearest")).double().mean())
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():           # alternating: drift hits every variant alike
            times[name].append(timed(fn, args.iters))
    base = float(np.median(times["labels_C4"]))
    lines = []
    for name, ts in times.items():
        lines.append(json.dumps({
            "variant": name, "shape": list(SHAPE), "grid": [5, 5, 5], "sigma": 5.0, "mode": "nearest",
            "median_us": round(float(np.median(ts)), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
            "vs_labels_C4": round(float(np.median(ts)) / base, 3), "iters": args.iters, "repeats": args.repeats}))
        print(lines[-1], flush=True)
    lines.append(json.dumps({"one_hot_C4_agrees_with_labels": round(same, 6), "device": torch.cuda.get_device_name(0)}))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
