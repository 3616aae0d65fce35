"""
Plain float64 reference of the B-spline prefilter (mirror boundary) and of its transpose.  TEST INFRASTRUCTURE ONLY:
NumPy, no recursion, no code shared with the kernels.

The prefilter of order p turns samples x into coefficients c with  sum_k b_p[k] c[i - k] = x[i],  b_p the B-spline of
order p sampled at the integers, c extended beyond the line by mirroring about its end samples (c[-j] = c[j],
c[n-1+j] = c[n-1-j]) -- scipy.ndimage.spline_filter1d(mode='mirror').  So with the n x n matrix

    B[i, fold(i + k)] += b_p[k],     fold = the mirror index map with period 2n - 2,

the forward filter is  F = B^-1  and its transpose (the reference's NI_SplineFilter1DGrad)  F^T = B^-T.  B is
diagonally dominant (condition number below 8 for every order), so the dense inverse is good to a few ulp.

    forward(x, order, axis) / transpose(x, order, axis)   one axis of an array
    windowed(x, window, axes, order, transpose)           the chain on the contiguous copy x[window], the rest untouched
    tap_range(c, order)                                   first tap index of a coordinate, order + 1 taps
    alternating_eigenvalue(order)                         F (-1)^i = lambda (-1)^i, from the poles
"""
import functools

import numpy as np

# B-spline of order p at the integers 0, 1, 2 (symmetric)
SAMPLES = {2: (3.0 / 4.0, 1.0 / 8.0),
           3: (2.0 / 3.0, 1.0 / 6.0),
           4: (115.0 / 192.0, 19.0 / 96.0, 1.0 / 384.0),
           5: (11.0 / 20.0, 13.0 / 60.0, 1.0 / 120.0)}

# the poles (Unser, Aldroubi, Eden 1993): roots inside the unit circle of the sampled B-spline's z-transform
POLES = {2: (np.sqrt(8.0) - 3.0,),
         3: (np.sqrt(3.0) - 2.0,),
         4: (np.sqrt(664.0 - np.sqrt(438976.0)) + np.sqrt(304.0) - 19.0,
             np.sqrt(664.0 + np.sqrt(438976.0)) - np.sqrt(304.0) - 19.0),
         5: (np.sqrt(67.5 - np.sqrt(4436.25)) + np.sqrt(26.25) - 6.5,
             np.sqrt(67.5 + np.sqrt(4436.25)) - np.sqrt(26.25) - 6.5)}


def mirror_fold(i, n):
    """index i of the mirror-extended line of n >= 2 samples -> index inside it"""
    period = 2 * n - 2
    i = np.abs(np.asarray(i)) % period
    return np.where(i >= n, period - i, i)


def interpolation_matrix(n, order):
    """B (n x n): coefficients -> samples, mirror boundary"""
    if n < 2:
        raise ValueError("lines of at least 2 samples")
    b = SAMPLES[order]
    B = np.zeros((n, n))
    rows = np.arange(n)
    for k in range(-(len(b) - 1), len(b)):
        np.add.at(B, (rows, mirror_fold(rows + k, n)), b[abs(k)])
    return B


@functools.lru_cache(maxsize=128)
def filter_matrix(n, order):
    """F = B^-1 (n x n, float64; read-only, shared)"""
    F = np.linalg.inv(interpolation_matrix(n, order))
    F.setflags(write=False)
    return F


def _apply(M, x, axis):
    x = np.asarray(x, dtype=np.float64)
    return np.moveaxis(np.tensordot(M, x, axes=([1], [axis])), 0, axis)


def forward(x, order, axis=-1):
    """scipy.ndimage.spline_filter1d(x, order, axis, mode='mirror') in float64"""
    x = np.asarray(x, dtype=np.float64)
    if order < 2:
        return x.copy()
    return _apply(filter_matrix(x.shape[axis], order), x, axis)


def transpose(x, order, axis=-1):
    """the adjoint of forward() along `axis` in float64"""
    x = np.asarray(x, dtype=np.float64)
    if order < 2:
        return x.copy()
    return _apply(filter_matrix(x.shape[axis], order).T, x, axis)


def window_slices(window):
    return tuple(slice(int(w0), int(w1)) for w0, w1 in window)


def windowed(x, window, axes, order, transpose_=False):
    """The filter chain over `axes` applied to the contiguous copy x[window] -- lines of the window's length, its ends
    the filter's boundaries -- written back into a float64 copy of x; everything outside the window is x's own.
    window: (w0, w1) per dimension of x."""
    out = np.array(x, dtype=np.float64)
    sl = window_slices(window)
    sub = np.ascontiguousarray(out[sl])
    for a in axes:
        sub = transpose(sub, order, a) if transpose_ else forward(sub, order, a)
    out[sl] = sub
    return out


def tap_range(c, order):
    """First tap index of source coordinate(s) c for spline order 0..5; the taps are first .. first + order.
    The rule of the interpolation's window (oracle/ed_oracle.c window_start): odd orders centre on floor(c), even orders
    on the nearest sample."""
    c = np.asarray(c, dtype=np.float64)
    base = np.floor(c) if order & 1 else np.floor(c + 0.5)
    return base.astype(np.int64) - order // 2


def alternating_eigenvalue(order):
    """(-1)^i is mirror-symmetric about every sample, so it is an eigenvector of B and of F:
    F (-1)^i = prod over the poles ((1 - z) / (1 + z))^2 (-1)^i  (the filter's gain at the Nyquist frequency)."""
    lam = 1.0
    for z in POLES[order]:
        lam *= ((1.0 - z) / (1.0 + z)) ** 2
    return lam
