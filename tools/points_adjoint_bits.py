"""
Bits of the point adjoints: a fixed, seeded list of small calls whose sums go through the fixed-point reduction of
csrc/ed_points_grad.h, every output array saved, so that two builds of the library can be compared bit for bit.  The
outputs do not depend on the order of the points or on how they are dealt to workgroups, so the comparison is exact, NaN
patterns included.

    python tools/points_adjoint_bits.py --out new.npz                       # the library of this tree
    python tools/points_adjoint_bits.py --lib /path/to/libedhip.so --out old.npz
    python tools/points_adjoint_bits.py --compare old.npz new.npz [--report profiles/points_adjoint_refactor_bits.txt]

One process per library.  The cases:
    points_{fwd,inv}_{n}d_{lds,global}_{f32,f64}   deform_grid_coordinates_gradient / deform_points_gradient, 1 to 4
                                                   axes, a grid staged in LDS and one above kPointsLdsValues values
                                                   (1-3 axes), float32 and float64 positions
    points_{fwd,inv}_batch2                        their batch forms, two samples
    jet_{u,A,G,all}_{n}d_{lds,global}              deform_grid_derivatives_gradient, each cotangent alone and all three
    inverse_{disp,affine}_{2,3}d                   deform_grid_inverse_displacement_gradient / _affine_gradient
    sample_coordinate                              deform_grid_sample_coordinate_gradient
    overflow_{points,jet}                          the library entries on one point at (100, 0.5) with the cotangent
                                                   (4e307, 0) and, as a second sample, (1, 0): a bound that overflows
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# deformed extents and control grid per number of axes: staged in LDS / more than 7680 values
SHAPES = {1: ((500,), (9,)), 2: ((30, 34), (5, 6)), 3: ((20, 24, 32), (4, 5, 6)), 4: ((8, 9, 10, 11), (3, 3, 4, 3))}
GLOBAL = {1: ((9000,), (7700,)), 2: ((70, 70), (64, 64)), 3: ((16, 16, 16), (14, 14, 14))}


def _arrays(result):
    """the arrays of a result (an array, a tensor, or a tuple of them with None for what is absent), by position"""
    import torch
    if not isinstance(result, tuple):
        result = (result,)
    out = {}
    for i, v in enumerate(result):
        if v is None:
            continue
        out[str(i)] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    return out


def _overflow(ed, entry, u0):
    """tests/test_points_gradient.py / test_derivatives_gradient.py: the library entry itself on the prefiltered grid"""
    import torch
    api = importlib.import_module("elasticdeform_amd.deform_grid")
    from elasticdeform_amd import _lib
    nb = len(u0)
    P = torch.from_numpy(np.random.default_rng(11).random((2, 4, 4)) - 0.5).cuda().repeat(nb, 1, 1, 1)
    q = torch.tensor([[100.0, 0.5]], dtype=torch.float64).cuda().repeat(nb, 1, 1)
    u = torch.tensor([[[v, 0.0]] for v in u0], dtype=torch.float64).cuda()
    rows, dP = torch.full_like(q, 7.0), torch.full_like(P, 7.0)
    dK = torch.full((nb, 2, 3), 7.0, dtype=torch.float64).cuda()
    d = api._desc_sample0
    tail = (*d(P), (8, 8), None, None, *d(rows), *d(dP), *d(dK), 0, api._stream(q.device))
    if entry == "points":
        _lib.deform_points_gradient(0, nb, *d(q), *d(u), None, 0, *tail)
    else:
        _lib.deform_points_derivatives_gradient(nb, *d(q), *d(u), None, 0, None, 0, *tail)
    torch.cuda.synchronize()
    return rows, dP, dK


def run():
    import elasticdeform_amd as ed
    rng = np.random.default_rng(2024)
    out = {}

    def keep(name, result):
        for k, v in _arrays(result).items():
            out["%s--%s" % (name, k)] = v

    def points_of(I, count, dtype=np.float64):
        return (rng.random((count, len(I))) * (np.asarray(I) + 4.0) - 2.0).astype(dtype)

    for table, tag in ((SHAPES, "lds"), (GLOBAL, "global")):
        for n, (I, ncp) in table.items():
            D = rng.standard_normal((n,) + ncp) * 1.5
            kw = dict(crop=tuple(slice(1, s - 1) for s in I)) if n <= 3 else {}
            if n == 2:
                kw["rotate"] = 12.0
            for dtype, dname in ((np.float32, "f32"), (np.float64, "f64")):
                q = points_of(I, 1000 if n <= 3 else 257, dtype)
                u = rng.standard_normal(q.shape).astype(dtype)
                keep("points_fwd_%dd_%s_%s" % (n, tag, dname), ed.deform_grid_coordinates_gradient(q, u, D, I, **kw))
                # (the inverse direction: the positions given, so that no solve stands between the call and its bits)
                keep("points_inv_%dd_%s_%s" % (n, tag, dname),
                     ed.deform_points_gradient(q, u, 0.2 * D, I, positions=q, **kw))
            if n <= 3:
                q = points_of(I, 1000 if tag == "lds" else 257)
                u, A, G = (rng.standard_normal(q.shape + (n,) * k) for k in range(3))
                for which, cot in (("u", dict(d_coordinates=u)), ("A", dict(d_jacobian=A)), ("G", dict(d_hessian=G)),
                                   ("all", dict(d_coordinates=u, d_jacobian=A, d_hessian=G))):
                    keep("jet_%s_%dd_%s" % (which, n, tag), ed.deform_grid_derivatives_gradient(q, D, I, **cot, **kw))
    I, ncp = SHAPES[3]
    Db = rng.standard_normal((2, 3) + ncp)
    qb = np.stack([points_of(I, 513), points_of(I, 513)])
    ub = rng.standard_normal(qb.shape)
    keep("points_fwd_batch2", ed.deform_grid_coordinates_gradient_batch(qb, ub, Db, I))
    keep("points_inv_batch2", ed.deform_points_gradient_batch(qb, ub, 0.2 * Db, I, positions=qb))
    for n in (2, 3):
        I, ncp = SHAPES[n]
        D = rng.standard_normal((n,) + ncp)
        Y = rng.random(I)
        dZ = rng.standard_normal(I)
        keep("inverse_disp_%dd" % n, ed.deform_grid_inverse_displacement_gradient(Y, dZ, D, order=3, mode="mirror"))
        keep("inverse_affine_%dd" % n, ed.deform_grid_inverse_affine_gradient(Y, dZ, D, order=3, mode="mirror",
                                                                             affine=np.eye(n + 1)[:n]))
    I, ncp = SHAPES[3]
    X = rng.random(I)
    q = points_of(I, 1000)
    keep("sample_coordinate", ed.deform_grid_sample_coordinate_gradient(X, rng.standard_normal(q.shape[0]), q,
                                                                        rng.standard_normal((3,) + ncp), order=3))
    keep("overflow_points", _overflow(ed, "points", [4e307, 1.0]))
    keep("overflow_jet", _overflow(ed, "jet", [4e307, 1.0]))
    return out


def compare(old_path, new_path, report):
    old, new = np.load(old_path), np.load(new_path)
    cases = sorted({k.split("--")[0] for k in list(old.files) + list(new.files)})
    lines, bad = [], 0
    for case in cases:
        keys = sorted(k for k in set(old.files) | set(new.files) if k.split("--")[0] == case)
        same = all(k in old.files and k in new.files and old[k].dtype == new[k].dtype and old[k].shape == new[k].shape
                   and old[k].tobytes() == new[k].tobytes() for k in keys)
        nans = sum(int(np.isnan(new[k]).sum()) for k in keys if k in new.files and new[k].dtype.kind == "f")
        lines.append("%-32s %d arrays, %d NaN   result bit-equal to parent: %s" % (case, len(keys), nans,
                                                                                 "YES" if same else "NO"))
        bad += not same
    lines.append("%d cases, %d differ" % (len(cases), bad))
    print("\n".join(lines))
    if report:
        with open(report, "a") as f:
            f.write("\n".join(lines) + "\n")
    return bad


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib", default=None, help="another build of libedhip.so to load instead of this tree's")
    p.add_argument("--out", default=None)
    p.add_argument("--compare", nargs=2, default=None)
    p.add_argument("--report", default=None, help="--compare: append the lines to this file")
    args = p.parse_args()
    if args.compare:
        sys.exit(1 if compare(args.compare[0], args.compare[1], args.report) else 0)
    if args.lib:
        from elasticdeform_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    out = run()
    np.savez(args.out, **out)
    print("%d arrays of %d cases -> %s" % (len(out), len({k.split("--")[0] for k in out}), args.out))


if __name__ == "__main__":
    main()
