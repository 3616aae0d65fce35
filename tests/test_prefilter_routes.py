"""
Whole-array prefilter passes (edhip_spline_filter1d, default arithmetic) at every line length where the launcher changes
its route, against the fp64 reference of tests/prefilter_reference.py.  Tolerances are those of
test_fast_prefilter_kernels: 2e-6 / 4e-6 of the result's scale for float32 orders 2-3 / 4-5, 1e-13 for float64.

The route table, derived from launch_spline_filter_fast and launch_line_tiles (spline_fast.hip) with the project's
constants kB = kK = 32 (block, warm-up), kBlock = 256 (threads), kTileLdsBudget = 80 KiB = 81920 bytes; n = line
length, nb = ceil(n / 32) blocks, T = element size, VN = 16 / T.  A change of a constant moves a row of this table, and
ROUTES below -- the same table as data, from which the test lengths are taken -- has to move with it.

  every axis kind
    n < 64                      exact kernel (spline_filter.hip)           `fp.len < 64` -> not supported by the fast path
    float64, orders 4 / 5       exact kernel at every length               `fp.in_dtype != EDHIP_F32` in the cascade
    float32, orders 4 / 5       two one-pole passes on the routes below;   `fp.len > 576`
                                n <= 576: second pass in place on the output, n >= 577: through a workspace temporary

  contiguous axis (lines along the last dimension): tile of R lines, pitch = 64 + 32 nb + VN (+ 1 scalar) elements,
  R halves from 32 while `R * nb > kBlock` or `1024 + R * pitch * T > 81920`; R < 8 -> no tile
    float32   64 ..  256        tile, R = 32      32 nb <= 256 <=> nb <= 8      (LDS: 1024 + 32 * 324 * 4 = 42496, never binds)
             257 ..  512        tile, R = 16      16 nb <= 256 <=> nb <= 16
             513 .. 1024        tile, R = 8        8 nb <= 256 <=> nb <= 32
            1025 ..             block-recompute kernel (lane = line, unit stride)
    float64   64 ..  224        tile, R = 32      LDS: 32 * pitch * 8 <= 80896 <=> pitch <= 316 <=> nb <= 7
                                                  (nb = 8: 1024 + 32 * 322 * 8 = 83456 > 81920)
             225 ..  512        tile, R = 16      16 nb <= 256 <=> nb <= 16     (LDS: pitch <= 632 <=> nb <= 17, does not bind)
             513 .. 1024        tile, R = 8        8 nb <= 256 <=> nb <= 32     (LDS: pitch <= 1264 <=> nb <= 37, does not bind)
            1025 ..             block-recompute kernel

  strided axis (lines across rows; the column axis is the unit-stride one): tile of 64 + 32 nb rows of C columns,
  CW = 256 / T columns (64 float32, 32 float64), i.e. 256-byte rows for either type
    columns > CW / 2,  64 .. 256    tile, C = CW      (64 + 32 nb) * 256 <= 81920 <=> nb <= 8
    columns > CW / 2, 257 .. 576    tile, C = CW / 2  (64 + 32 nb) * 128 <= 81920 <=> nb <= 18
    columns <= CW / 2, 64 .. 576    tile, C = CW / 2  `outer_len[cax] <= C / 2`: 32 columns float32, 16 float64
                      577 ..        block-recompute kernel (lane = line, strided)

Out of place the block-recompute kernels split a line into segments, in place they do not: both are run everywhere.
The chosen kernel is not observed at run time; the table stands in for it.  (tests/test_prefilter_window.py pins the
two ends of the tile routes -- contiguous 1024 / 1025, strided 576 / 577 -- through the windowed call, which only the
tile kernels serve.)
"""
import importlib

import numpy as np
import pytest

import prefilter_reference as pref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from elasticdeform_amd import _lib  # noqa: E402

FTYPE = {"float32": np.float32, "float64": np.float64}
VN = {"float32": 4, "float64": 2}
CW = {"float32": 64, "float64": 32}

# (dtype, axis kind) -> [(first length, last length or None, route)], the table above
ROUTES = {
    ("float32", "contiguous"): [(1, 63, "exact"), (64, 256, "tile R=32"), (257, 512, "tile R=16"),
                                (513, 1024, "tile R=8"), (1025, None, "block-recompute")],
    ("float64", "contiguous"): [(1, 63, "exact"), (64, 224, "tile R=32"), (225, 512, "tile R=16"),
                                (513, 1024, "tile R=8"), (1025, None, "block-recompute")],
    ("float32", "strided"): [(1, 63, "exact"), (64, 256, "tile C=CW"), (257, 576, "tile C=CW/2"),
                             (577, None, "block-recompute")],
    ("float64", "strided"): [(1, 63, "exact"), (64, 256, "tile C=CW"), (257, 576, "tile C=CW/2"),
                             (577, None, "block-recompute")],
}
TEMPORARY_ABOVE = 576      # float32 orders 4 / 5: `fp.len > 576`


def _boundary_lengths(dtype, kind):
    """the last length of every route and the first of the next, plus both sides of the orders-4/5 temporary"""
    ns = set()
    for first, last, _ in ROUTES[(dtype, kind)]:
        ns.add(first)
        if last is not None:
            ns.add(last)
    ns.discard(1)
    ns.update((TEMPORARY_ABOVE, TEMPORARY_ABOVE + 1))
    return sorted(ns)


def _route(dtype, kind, n):
    for first, last, name in ROUTES[(dtype, kind)]:
        if n >= first and (last is None or n <= last):
            return name
    raise AssertionError(n)


def _tol(dtype, order):
    return 1e-13 if dtype == "float64" else (2e-6 if order < 4 else 4e-6)


def _env():
    dgm = importlib.import_module("elasticdeform_amd.deform_grid")
    dev = torch.device("cuda", torch.cuda.current_device())
    return dgm, dev, torch.cuda.current_stream(dev).cuda_stream


def _filter(xd, axis, order, transpose, inplace, out=None):
    dgm, dev, stream = _env()
    if inplace:
        out = xd.clone() if out is None else out
        _lib.spline_filter1d(dgm._desc(out), dgm._desc(out), axis, order, transpose, _lib.FLAG_AUTO, stream)
    else:
        out = torch.full_like(xd, float("nan")) if out is None else out
        _lib.spline_filter1d(dgm._desc(xd), dgm._desc(out), axis, order, transpose, _lib.FLAG_AUTO, stream)
    return out


def _want(x, order, axis, transpose):
    x = np.asarray(x, dtype=np.float64)
    return pref.transpose(x, order, axis) if transpose else pref.forward(x, order, axis)


def _compare(got, want, tol, what, scale=None):
    scale = np.abs(want).max() if scale is None else scale
    err = np.abs(got.astype(np.float64) - want).max()
    print("%s: err %.3e of scale (bound %.1e)" % (what, err / scale, tol))
    assert err <= tol * scale, (what, err / scale)


def _shape(kind, n, other):
    return ((other, n), 1) if kind == "contiguous" else ((n, other), 0)


def _all_passes(x, axis, dtype, what, orders=(2, 3, 4, 5)):
    """forward and transpose, out of place and in place, against the fp64 reference"""
    _, dev, _ = _env()
    xd = torch.from_numpy(x).to(dev) if isinstance(x, np.ndarray) else x
    xh = xd.cpu().numpy()
    for order in orders:
        for transpose in (0, 1):
            want = _want(xh, order, axis, transpose)
            for inplace in (False, True):
                got = _filter(xd, axis, order, transpose, inplace).cpu().numpy()
                _compare(got, want, _tol(dtype, order), what + (order, transpose, inplace))
    np.testing.assert_array_equal(xd.cpu().numpy(), xh)       # the input of an out-of-place pass is not written


def _cases():
    out = []
    for (dtype, kind) in sorted(ROUTES):
        for n in _boundary_lengths(dtype, kind):
            out.append(pytest.param(dtype, kind, n, id="%s-%s-%d-%s" % (dtype, kind, n, _route(dtype, kind, n).replace(" ", ""))))
    return out


@pytest.mark.parametrize("dtype,kind,n", _cases())
def test_both_sides_of_every_route_boundary(dtype, kind, n):
    rng = np.random.default_rng(n)
    shape, axis = _shape(kind, n, 40)            # 40 lines / 40 columns (> CW / 2 for either type: the full-width tile)
    x = rng.standard_normal(shape).astype(FTYPE[dtype])
    _all_passes(x, axis, dtype, (dtype, kind, n, _route(dtype, kind, n)))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_column_rule_of_the_strided_tiles(dtype):
    """`outer_len[cax] <= C / 2`: CW / 2 columns (32 float32 / 16 float64) take the half-width tile, one vector more
    the full-width one; on either side of n = 256 as well, where the full-width tile ends anyway"""
    half = CW[dtype] // 2
    for n in (96, 256, 257):
        for cols in (half - VN[dtype], half, half + VN[dtype], half + 1):
            x = np.random.default_rng(cols).standard_normal((n, cols)).astype(FTYPE[dtype])
            _all_passes(x, 0, dtype, (dtype, "columns", n, cols), orders=(3, 5))
    # the column axis need not be the only outer axis
    x = np.random.default_rng(1).standard_normal((3, 96, half)).astype(FTYPE[dtype])
    _all_passes(x, 1, dtype, (dtype, "columns", x.shape), orders=(2,))
    x = np.random.default_rng(2).standard_normal((3, 96, half + VN[dtype])).astype(FTYPE[dtype])
    _all_passes(x, 1, dtype, (dtype, "columns", x.shape), orders=(2,))


# ---- alignment -------------------------------------------------------------------------------------------------------

def _off_by_one_element(shape, dtype, dev, rng):
    """a dense tensor whose base pointer is one element (4 / 8 bytes) off 16-byte alignment"""
    n = int(np.prod(shape))
    big = torch.zeros(n + 8, dtype=getattr(torch, dtype), device=dev)
    assert big.data_ptr() % 16 == 0
    v = big[1:1 + n].view(shape)
    v.copy_(torch.from_numpy(rng.standard_normal(shape).astype(FTYPE[dtype])))
    assert v.data_ptr() % 16 == (4 if dtype == "float32" else 8)
    return v


@pytest.mark.parametrize("kind,n", [("contiguous", 96), ("contiguous", 1028), ("strided", 96), ("strided", 320),
                                    ("strided", 580)])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_misaligned_and_ragged_layouts(dtype, kind, n):
    """what sends a pass to the scalar (`aligned16 == false` / non-vector) kernels: a base pointer off 16-byte
    alignment (input, output, both, in place), a last extent that is no multiple of the vector width, outer / axis
    strides that are none (a sliced view) -- a tile length and a block-recompute length of each axis kind"""
    _, dev, _ = _env()
    rng = np.random.default_rng(n)
    vn = VN[dtype]
    shape, axis = _shape(kind, n, 24)
    what = (dtype, kind, n)
    # base pointer: one side off, both sides off, in place
    v = _off_by_one_element(shape, dtype, dev, rng)
    xh = v.cpu().numpy()
    xa = torch.from_numpy(xh).to(dev)
    for order in (2, 3, 5):
        for transpose in (0, 1):
            want = _want(xh, order, axis, transpose)
            out = _filter(v, axis, order, transpose, False, out=torch.full_like(xa, float("nan")))
            _compare(out.cpu().numpy(), want, _tol(dtype, order), what + ("input misaligned", order, transpose))
            out = _off_by_one_element(shape, dtype, dev, rng)
            _filter(xa, axis, order, transpose, False, out=out)
            _compare(out.cpu().numpy(), want, _tol(dtype, order), what + ("output misaligned", order, transpose))
            out = _off_by_one_element(shape, dtype, dev, rng)
            _filter(v, axis, order, transpose, False, out=out)
            _compare(out.cpu().numpy(), want, _tol(dtype, order), what + ("both misaligned", order, transpose))
            out.copy_(v)
            _filter(out, axis, order, transpose, True, out=out)
            _compare(out.cpu().numpy(), want, _tol(dtype, order), what + ("misaligned, in place", order, transpose))
    np.testing.assert_array_equal(v.cpu().numpy(), xh)
    # last extent no multiple of the vector width
    if kind == "contiguous":
        ragged = sorted({(24, n + 1), (24, n + vn - 1)})
    else:
        ragged = sorted({(n, 24 + 1), (n, 24 + vn - 1)})
    for shp in ragged:
        x = rng.standard_normal(shp).astype(FTYPE[dtype])
        _all_passes(x, axis, dtype, what + ("ragged", shp), orders=(3, 4))
    # a sliced view: the last extent is a multiple, the row stride is not
    base = torch.from_numpy(rng.standard_normal((shape[0], shape[1] + 1)).astype(FTYPE[dtype])).to(dev)
    view = base[:, :shape[1]]
    assert view.stride(0) % vn == 1 and not view.is_contiguous()
    xh = view.cpu().numpy()
    for order in (3, 4):
        for transpose in (0, 1):
            want = _want(xh, order, axis, transpose)
            got = _filter(view, axis, order, transpose, False, out=torch.full_like(torch.from_numpy(xh).to(dev), float("nan")))
            _compare(got.cpu().numpy(), want, _tol(dtype, order), what + ("view -> dense", order, transpose))
            keep = base.clone()
            inpl = keep[:, :shape[1]]
            _filter(inpl, axis, order, transpose, True, out=inpl)
            _compare(inpl.cpu().numpy(), want, _tol(dtype, order), what + ("view in place", order, transpose))
            # the column the view leaves out is not part of the array
            np.testing.assert_array_equal(keep[:, shape[1]].cpu().numpy(), base[:, shape[1]].cpu().numpy())


# ---- structured inputs -----------------------------------------------------------------------------------------------

def _structured_lengths(dtype, kind):
    first_block = [first for first, last, name in ROUTES[(dtype, kind)] if name == "block-recompute"][0]
    return (64, 65, 96, 97, 576, first_block)


@pytest.mark.parametrize("kind", ["contiguous", "strided"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_unit_impulses_next_to_the_ends_of_a_line(dtype, kind):
    """impulses at 0, 1, 2, n-3, n-2, n-1 and mid-line: the causal initialisation (forward: the mirror image of the
    line's start) and the transpose's folded tails are all there is to see; absolute tolerance, the response is O(1)"""
    _, dev, _ = _env()
    for n in _structured_lengths(dtype, kind):
        pos = [0, 1, 2, n - 3, n - 2, n - 1, n // 2, n // 3]
        lines = np.zeros((40, n), dtype=FTYPE[dtype])
        for j in range(40):
            lines[j, pos[j % len(pos)]] = 1.0 if j < 24 else -2.5
        x = lines if kind == "contiguous" else np.ascontiguousarray(lines.T)
        axis = 1 if kind == "contiguous" else 0
        xd = torch.from_numpy(x).to(dev)
        for order in (2, 3, 4, 5):
            for transpose in (0, 1):
                want = _want(x, order, axis, transpose)
                for inplace in (False, True):
                    got = _filter(xd, axis, order, transpose, inplace).cpu().numpy()
                    _compare(got, want, _tol(dtype, order), (dtype, kind, n, "impulses", order, transpose, inplace),
                             scale=max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("kind", ["contiguous", "strided"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_constant_and_alternating_lines(dtype, kind):
    """The forward filter of a constant is that constant (the gain is normalised): 4 ulp in float32, 1e-14 in float64.
    (Measured on the MI355X, either axis kind, every length here: float32 0 / 1 / 3 / 4 ulp for orders 2 / 3 / 4 / 5 --
    the two float32 passes of order 5 use the whole bound -- and at most 1.3e-15 in float64.)
    (-1)^i is the mirror filter's other eigenvector, eigenvalue prod ((1 - z) / (1 + z))^2 over the poles: against the
    fp64 reference (and the closed form to the same tolerance)."""
    _, dev, _ = _env()
    ftype = FTYPE[dtype]
    for n in _structured_lengths(dtype, kind):
        values = np.array([1.0, -3.7, 0.001953125, 1000.5] * 10)            # one per line
        const = np.repeat(values[:, None], n, axis=1).astype(ftype)
        alt = (values[:, None] * (-1.0) ** np.arange(n)[None, :]).astype(ftype)
        axis = 1 if kind == "contiguous" else 0
        if kind == "strided":
            const, alt = np.ascontiguousarray(const.T), np.ascontiguousarray(alt.T)
        cd, ad = torch.from_numpy(const).to(dev), torch.from_numpy(alt).to(dev)
        # per element: 4 ulp of the constant (float32) / 1e-14 of it (float64)
        bound = 4 * np.spacing(np.abs(const)).astype(np.float64) if dtype == "float32" else 1e-14 * np.abs(const)
        for order in (2, 3, 4, 5):
            for inplace in (False, True):
                got = _filter(cd, axis, order, 0, inplace).cpu().numpy()
                err = np.abs(got.astype(np.float64) - const.astype(np.float64))
                print("%s: constant line, worst error %.2f of its bound" %
                      ((dtype, kind, n, order, inplace), (err / bound).max()))
                assert (err <= bound).all(), (dtype, kind, n, order, inplace, (err / bound).max())
                got = _filter(ad, axis, order, 0, inplace).cpu().numpy()
                want = pref.forward(alt, order, axis)
                _compare(got, want, _tol(dtype, order), (dtype, kind, n, "alternating", order, inplace))
                _compare(got, pref.alternating_eigenvalue(order) * alt.astype(np.float64), _tol(dtype, order),
                         (dtype, kind, n, "alternating, closed form", order, inplace))


def _adjoint_cases():
    out = []
    for (dtype, kind) in sorted(ROUTES):
        for first, last, name in ROUTES[(dtype, kind)]:
            n = first + 1 if last is None else last      # the far end of each route (the exact kernel: n = 63)
            out.append(pytest.param(dtype, kind, n, id="%s-%s-%d-%s" % (dtype, kind, n, name.replace(" ", ""))))
        if kind == "strided":                            # the half-width tile by the column rule
            out.append(pytest.param(dtype, "strided-narrow", 200, id="%s-strided-200-tileC=CW/2-by-columns" % dtype))
    return out


@pytest.mark.parametrize("dtype,kind,n", _adjoint_cases())
def test_adjointness_on_every_route(dtype, kind, n):
    """<F x, y> = <x, F^T y> line by line, the dot products in fp64.  Either side carries at most n products with an
    error of tol * scale of the filtered factor each: the bound is tol * n * (max|F x| max|y| + max|x| max|F^T y|)."""
    _, dev, _ = _env()
    rng = np.random.default_rng(n)
    other = CW[dtype] // 2 if kind == "strided-narrow" else 40
    shape, axis = _shape("contiguous" if kind == "contiguous" else "strided", n, other)
    x = rng.standard_normal(shape).astype(FTYPE[dtype])
    y = rng.standard_normal(shape).astype(FTYPE[dtype])
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    for order in (2, 3, 4, 5):
        for inplace in (False, True):
            Fx = _filter(xd, axis, order, 0, inplace).cpu().numpy().astype(np.float64)
            Fty = _filter(yd, axis, order, 1, inplace).cpu().numpy().astype(np.float64)
            a = np.sum(Fx * y64, axis=axis)
            b = np.sum(x64 * Fty, axis=axis)
            bound = _tol(dtype, order) * n * (np.abs(Fx).max() * np.abs(y64).max() + np.abs(x64).max() * np.abs(Fty).max())
            print("%s: adjointness, worst %.3e of the bound" % ((dtype, kind, n, order, inplace), np.abs(a - b).max() / bound))
            assert np.abs(a - b).max() <= bound, (dtype, kind, n, order, inplace, np.abs(a - b).max(), bound)
