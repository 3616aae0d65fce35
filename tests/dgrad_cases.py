"""
The case table of tests/test_dgrad_routes.py (GPU) and the error bound of its float64 comparison; the host file
tests/test_dgrad_reference_host.py evaluates the same table through the reference alone.  Not a test module.

Every case is one call of deform_grid_displacement_gradient / deform_grid_affine_gradient on the smallest shape
that reaches one launch shape of deform_dgrad.hip (see `why`).  dY is standard normal, the displacement standard
normal times `sigma`, the volumes are smooth (`_volume`).
"""
import math

import numpy as np

MODES = ["constant", "nearest", "mirror", "reflect", "wrap"]


def _c(name, shape, ncp, why, order=3, mode="mirror", sigma=2.0, **extra):
    return dict(name=name, shape=tuple(shape), ncp=tuple(ncp), why=why, order=order, mode=mode, sigma=sigma, **extra)


def _table():
    t = [
        _c("block128", (5, 100), (3, 5), "block 128, second wave partly filled"),
        _c("block256", (5, 200), (3, 4), "block 256, one partial chunk", mode="reflect"),
        _c("one_chunk", (4, 256), (3, 5), "exactly one chunk", mode="wrap"),
        _c("two_chunks", (4, 512), (3, 5), "exactly two chunks", mode="nearest"),
        _c("empty_waves", (4, 300), (3, 5), "two chunks, waves 1 to 3 of the last chunk empty", mode="constant"),
        _c("one_voxel_chunk", (3, 513), (3, 4), "three chunks, one voxel in the last"),
    ]
    for nl in (16, 17, 33, 100, 128):
        t.append(_c("K%d" % (2 * nl), (4, 300), (3, nl), "band class K = naxis * ncp_last", mode=MODES[nl % 5]))
    t.append(_c("K255_3d", (4, 5, 70), (3, 3, 85), "K = 255 with three axes", sigma=1.0))
    for ncp in ((4, 1), (4, 2), (4, 3), (1, 5), (2, 5)):
        t.append(_c("folded_%dx%d" % ncp, (6, 300), ncp, "1 to 3 control points: every tap window folds",
                    mode=MODES[sum(ncp) % 5]))
    t += [
        _c("contract130", (130, 20), (4, 4), "contracted axis longer than 64: two lane iterations and a tail"),
        _c("contract_3d", (65, 70, 12), (3, 4, 3), "two contractions, the early continue, nouter > 1", mode="reflect",
           sigma=0.3),
        _c("affine_2wg", (257, 9), (4, 3), "affine reduce: 2 workgroups, 1 row in the second", mode="nearest"),
        _c("affine_store", (129, 128, 6), (8, 8, 3), "affine store: more than 64 partials", order=1, sigma=0.5),
        _c("crop_affine", (10, 400), (3, 6), "crop offset and affine on a chunked row", crop=((2, 8), (37, 390)),
           affine=True),
    ]
    for order in range(1, 6):
        for mode in MODES:
            t.append(_c("modes_o%d_%s" % (order, mode), (6, 300), (3, 5), "every order and mode on a chunked row",
                        order=order, mode=mode, modes_case=True, sigma=3.0))
    for order in range(1, 6):
        t.append(_c("3d_o%d" % order, (4, 5, 140), (3, 3, 4), "3-D, block 256", order=order, mode=MODES[order % 5],
                    sigma=0.7))
    for order in range(1, 6):
        t.append(_c("1d_K5_o%d" % order, (700,), (5,), "1-D generic kernel, chunked", order=order,
                    mode=MODES[order % 5], sigma=4.0))
        t.append(_c("1d_K200_o%d" % order, (700,), (200,), "1-D generic kernel, chunked, K = 200", order=order,
                    mode=MODES[(order + 2) % 5], sigma=1.0, reseed=int(order == 1)))
    for order in range(1, 6):
        t.append(_c("4d_o%d" % order, (3, 4, 3, 70), (2, 3, 2, 4), "4 axes (generic kernel)", order=order,
                    mode=MODES[(order + 1) % 5], sigma=0.1))
    t += [
        _c("5d_o3", (3, 4, 3, 3, 4), (2,) * 5, "5 axes", order=3, sigma=0.01, ramp=True),
        _c("6d_o2", (3, 3, 4, 3, 3, 4), (2,) * 6, "6 axes", order=2, mode="reflect", sigma=0.002, ramp=True),
        _c("7d_o1", (3, 3, 3, 4, 3, 3, 3), (2,) * 7, "7 axes", order=1, mode="wrap", sigma=2e-6, ramp=True),
        _c("two_inputs_channels", (5, 300), (3, 5), "second input accumulates; a channel step axis",
           order=[3, 1], mode=["mirror", "nearest"], nin=2, channels=3),
        _c("batch_row", (4, 300), (3, 5), "batch of 3, chunked row", batch=3),
        _c("batch_contract", (65, 70, 12), (3, 4, 3), "batch of 3, two contractions", batch=3, mode="reflect",
           sigma=0.3),
        _c("batch_one_launch", (40, 130), (60, 40), "batch of 3 in one launch (a grid too large for the library's own "
           "prefilter): blockIdx.y > 0, the grid filter outside the call", batch=3, sigma=1.0),
        _c("float32_grid", (4, 300), (3, 5), "float32 displacement grid", grid32=True),
    ]
    for shape, ncp, sigma in (((4, 300), (3, 5), 2.0), ((4, 5, 140), (3, 3, 4), 0.7), ((700,), (5,), 4.0),
                              ((3, 4, 3, 70), (2, 3, 2, 4), 0.1)):
        for order in range(1, 6):
            t.append(_c("float32_%dd_o%d" % (len(shape), order), shape, ncp, "float32 volumes and dY", order=order,
                        mode=MODES[(order + len(shape)) % 5], sigma=sigma, f32=True))
    for i, case in enumerate(t):
        case["seed"] = 5000 + i + 1000 * case.get("reseed", 0)      # (reseed: the first seed broke the host condition)
    return t


CASES = _table()
F64_CASES = [c for c in CASES if not c.get("f32")]
F32_CASES = [c for c in CASES if c.get("f32")]


def _volume(rng, shape, ramp):
    """six random plane waves of 5 to 12 samples per period plus a trace of white noise: every sample differs, and the
    prefiltered coefficients do not cancel inside a tap window (white noise through the order-5 prefilter alternates
    in sign, and the tap-level scale S of the bound is then thousands of times the gradient).  `ramp`: also a slope
    of 1 along every axis, which no wave undoes -- the derivative has one sign (see `make`)."""
    o = np.indices(shape).astype(np.float64)
    X = 0.001 * rng.standard_normal(shape)
    if ramp:
        X += (o - o.mean(axis=tuple(range(1, o.ndim)), keepdims=True)).sum(0)
    # (along an axis shorter than 16 samples the waves are 3 to 6 times the axis long: a faster one is all
    # high frequency for the mirror prefilter there)
    lo = np.array([5.0 if m >= 16 else 3.0 * m for m in shape])
    for _ in range(6):
        f = 2 * np.pi / rng.uniform(lo, 2.4 * lo) * rng.choice([-1.0, 1.0], len(shape))
        X += (0.04 if ramp else 1.0) * rng.uniform(0.5, 1.0) * np.cos(np.tensordot(f, o, axes=1) + rng.uniform(0, 2 * np.pi))
    return X


def make(case):
    """(X, dY, D, kw) of a case as NumPy arrays; with `batch` every array has the batch axis in front"""
    rng = np.random.default_rng(case["seed"])
    shape, n = case["shape"], len(case["shape"])
    B = (case["batch"],) if case.get("batch") else ()
    full = B + shape + ((case["channels"],) if case.get("channels") else ())
    crop = case.get("crop")
    out = B + (tuple(b - a for a, b in crop) if crop else shape) + full[len(B) + n:]
    dt = np.float32 if case.get("f32") else np.float64
    # 5 to 7 axes with 2 control points each: the transposed grid filter is [[2, -1], [-1, 2]] per axis and S_D grows
    # by 3 per axis while a gradient of random signs does not -- there the volume rises along every axis and dY is
    # positive, so that the voxels' terms add up
    ramp = bool(case.get("ramp"))
    X = [_volume(rng, full, ramp).astype(dt) for _ in range(case.get("nin", 1))]
    dY = [rng.standard_normal(out) for _ in X]
    dY = [((np.abs(y) + 0.1) if ramp else y).astype(dt) for y in dY]
    D = rng.standard_normal(B + (n,) + case["ncp"]) * case["sigma"]
    if case.get("grid32"):
        D = D.astype(np.float32)
    kw = dict(order=case["order"], mode=case["mode"])
    if crop:
        kw["crop"] = tuple(slice(a, b) for a, b in crop)
    if case.get("affine"):
        kw["affine"] = np.concatenate([np.eye(n) + 0.04 * rng.standard_normal((n, n)),
                                       0.6 * rng.standard_normal((n, 1))], 1)
    if case.get("channels"):
        kw["axis"] = tuple(range(n))
    if len(X) == 1:
        X, dY = X[0], dY[0]
    return X, dY, D, kw


# ---- the float64 bound ---------------------------------------------------------------------------------------------

def rounding_counts(case, cmax, dmax):
    """(c_D, c_K): the factors of 2^-53 * S_D and 2^-53 * S_K that bound |kernel - reference| in float64.

    Derived from the summation structure in the header of deform_dgrad.hip (first order in u = 2^-53; a sum of terms
    added along a path of d additions is off by at most d u times the sum of their absolute values, a product of k
    rounded factors by k u), NOT from what the kernel returns.  n axes, order p, row length L, block = 64 / 128 / 256,
    K = n ncp_last, G = voxel groups per wave (the largest power of two with G K <= 64).

    kernel, per result
      weights        a closed form is at most 12 operations (order 5 Horner); a tap's product has n of them   12 n
      tap products   C times n weights                                                                        n
      tap sum        2 and 3 axes: the separable tree, (p + 1) additions and one product per axis             n (p + 2)
                     1 and 4..7 axes: one running sum over all taps                                           (p + 1)^n
      steps, inputs  dY times the sum, one addition per step and input                                        1 + steps
      band           the b weight (12), its product with g, a running sum over the group's 64 / G voxels      13 + 64 / G
      chunks         one addition per chunk of the row                                                        ceil(L / block)
      waves, groups  a running sum over block / 64 waves times G groups                                       (block / 64) G
      contraction    per axis d < n - 1: the coefficient (12 + 3), its product, the lane loop
                     ceil(L_d / 64), the tree of 6                                                            22 + ceil(L_d / 64)
      grid filter    per grid axis: the transposed recursion, two passes of 2 roundings per sample whose errors
                     decay with the pole |z| = 0.268 (gain 1 / (1 - |z|) per pass, 8 in all), the gain factor
                     and the boundary sum over the axis                                                       9 + ncp_d
      inverse map    instead of band .. grid filter: the butterfly (6), g times o (1), the chunks, the waves,
                     o_l times S0 (1), the second butterfly (6), its 4 waves, the store's lane loop and
                     butterfly                                                            18 + chunks + waves + ceil(rows / 256 / 64) + 6
    reference      its weights (de Boor, 4 p operations each), the same running sum over the taps, and its
                   contractions as matrix products (counted as a running sum over a block of 32 per axis)     4 p n + (p + 1)^n + 32 n

    conditioning of the coordinate.  The weights are functions of m_h = map(c_h), and the kernel rounds c_h (the
    reference forms it with a 64-bit significand, 2^-11 of that, and rounds m - tap once: 4 u).  Without an affine o
    and the offset are exact integers: one rounding in the sum with the displacement and one in the fold of the
    boundary map (`c + period`; the other folds subtract numbers on c's own grid and are exact); with an affine n
    products and n additions more: 2 n + 2.  Each is at most u / 2 times the power of two above `cmax`.  The
    displacement sum_j P beta is a running sum of 4^(n-1) terms whose weights are n - 1 rounded products of closed
    forms (8 each), then 4 terms with a weight of 8: off by at most (4^(n-1) + 8 n + 4) u `dmax`, dmax the largest
    sum_j |P| beta (the cubic weights are non-negative).  A shift dm of the coordinate moves the derivative weights
    by |w''| dm, sum_t |w''_t| <= 4 against sum_t |w'_t| >= 1, and the value weights of each other axis by |w'| dm,
    sum_t |w'_t| <= 2 against sum_t w_t = 1: (4 + 2 (n - 1)) dm relative to the tap-level scale.
    """
    n = len(case["shape"])
    shape = tuple(b - a for a, b in case["crop"]) if case.get("crop") else case["shape"]
    ncp = case["ncp"]
    p = max(case["order"]) if isinstance(case["order"], list) else case["order"]
    L = shape[-1]
    block = 256 if L > 128 else (128 if L > 64 else 64)
    K = n * ncp[-1]
    G = 1
    while G < 64 and 2 * G * K <= 64:
        G *= 2
    steps = case.get("nin", 1) * case.get("channels", 1)
    taps = n * (p + 2) if n in (2, 3) else (p + 1) ** n
    chunks = -(-L // block)
    waves = block // 64
    voxel = 12 * n + n + taps + 1 + steps
    ref = 4 * p * n + (p + 1) ** n + 32 * n
    c_d = voxel + 13 + 64 // G + chunks + waves * G + ref
    rows = 1
    for d in range(n - 1):
        c_d += 22 + -(-shape[d] // 64)
        rows *= shape[d]
    for d in range(n):
        c_d += 9 + ncp[d]
    c_k = voxel + 18 + chunks + waves + -(-(-(-rows // 256)) // 64) + 6 + ref
    mag = 2.0 ** math.ceil(math.log2(max(cmax, 1.0)))
    dm = (2 * n + 2 if case.get("affine") else 2) * mag / 2 + (4 ** (n - 1) + 8 * n + 4) * dmax + 4
    if np.finfo(np.longdouble).nmant < 63:
        dm *= 2                           # (no extended precision here: the reference rounds its coordinates too)
    cond = (4 + 2 * (n - 1)) * dm
    return c_d + cond, c_k + cond


U = 2.0 ** -53
