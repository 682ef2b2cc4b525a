"""Line-by-line, element-by-element checks of the sweep kernels (helper module of test_linewise_host.py / test_gpu_linewise.py).

The reference is a dense long-double product with the Chebyshev-Gauss-Lobatto differentiation matrix D (or the interior
block L = (D D)[1:n, 1:n] of its square), built here from the closed formula.  The bar is componentwise: for every element

    |y_i - truth_i| <= (K + 8) 2^-53 B_i,      B_i = 1/2 sum_j (|M_ij| + |M_i,m-j|) (|x_j| + |x_m-j|),   m = rows - 1,

K = points of the line.  B_i dominates sum_j |M_ij||x_j| and the same sum of the even / odd split
(sum_j |E_ij||e_j| + |O_ij||o_j| with E, O = (M_ij +- M_i,m-j) / 2, e, o = x_j +- x_m-j), so it does not depend on how a route
orders or splits the sum.  Roundings counted (first order, Higham's gamma_k): one per matrix entry (long double -> double), one
for e / o, at most K for the multiply-add chain in any order, two for the recombination, one for alpha, one for an accumulate
operand: K + 6 <= K + 8.  With an accumulator |acc_i| is added to B_i.  B_i = 0 demands y_i == 0 exactly."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
PI_L = LD(4) * np.arctan(LD(1))            # pi to the last bit of the long-double format


# ----------------------------------------------------------------------------------------------
# matrices
# ----------------------------------------------------------------------------------------------
_D, _L = {}, {}


def _sin_half(k, n):
    """sin(k pi / 2n) for integer k in [-2n, 2n], long double; the argument is folded into [0, pi/2] first so that the rounding
    of pi is never amplified (sin(pi - t) = sin t)."""
    k = np.asarray(k)
    sgn = np.where(k < 0, -1, 1)
    a = np.abs(k)
    a = np.where(a > n, 2 * n - a, a)
    return sgn * np.sin(PI_L * a.astype(LD) / LD(2 * n))


def dense_D(P):
    """The differentiation matrix of the degree-n interpolant on x_i = cos(i pi / n), n = P - 1, in long double:
    D_ij = (c_i / c_j) (-1)^(i+j) / (x_i - x_j), c_0 = c_n = 2, else 1, with x_i - x_j = -2 sin((i+j) pi/2n) sin((i-j) pi/2n);
    D_ii = -x_i / (2 sin^2(i pi / n)), D_00 = (2 n^2 + 1) / 6 = -D_nn."""
    if P in _D:
        return _D[P]
    n = P - 1
    i = np.arange(P)
    I, J = np.meshgrid(i, i, indexing="ij")
    c = np.where((i == 0) | (i == n), LD(2), LD(1))
    dx = LD(-2) * _sin_half(I + J, n) * _sin_half(I - J, n)
    dx[i, i] = LD(1)
    D = (c[:, None] / c[None, :]) * np.where((I + J) & 1, LD(-1), LD(1)) / dx
    s = _sin_half(2 * i, n)                                    # sin(i pi / n)
    s[0] = s[n] = LD(1)
    # cos(i pi / n) = sin((n - 2i) pi / 2n): the same folding
    D[i, i] = -_sin_half(n - 2 * i, n) / (LD(2) * s * s)
    D[0, 0] = (LD(2) * n * n + LD(1)) / LD(6)
    D[n, n] = -D[0, 0]
    _D[P] = D
    return D


def dense_L(P):
    """(D D)[1:n, 1:n], the second derivative of a line of P points with zero end values at its P - 2 interior points."""
    if P not in _L:
        D = dense_D(P)
        _L[P] = np.ascontiguousarray(np.dot(D, D)[1:P - 1, 1:P - 1])
    return _L[P]


# ----------------------------------------------------------------------------------------------
# truth and bound
# ----------------------------------------------------------------------------------------------
def truth(M, x, axis, lines=None):
    """M applied along `axis` of x in long double.  lines: flat indices (C order of the shape without `axis`) of the lines to
    compute; the result is then (rows, len(lines))."""
    if lines is not None:
        xl = take_lines(x, axis, lines).astype(LD)
        return np.dot(M, xl)
    y = np.tensordot(M, np.asarray(x).astype(LD), axes=([1], [axis]))
    return np.moveaxis(y, 0, axis)


def bound(M, x, axis, lines=None):
    """The componentwise weight B (module docstring), double."""
    A = np.abs(np.asarray(M, dtype=np.float64))
    A = 0.5 * (A + A[:, ::-1])
    if lines is not None:
        ax = np.abs(take_lines(x, axis, lines))
        return A @ (ax + ax[::-1])
    ax = np.abs(np.asarray(x, dtype=np.float64))
    ax = ax + np.flip(ax, axis)
    with np.errstate(invalid="ignore"):                         # (isolation runs never come here; inf * 0 cannot arise for finite x)
        return np.moveaxis(np.tensordot(A, ax, axes=([1], [axis])), 0, axis)


def take_lines(x, axis, lines):
    """(points, len(lines)) array of whole lines of x along `axis`."""
    x = np.asarray(x)
    xm = np.moveaxis(x, axis, 0).reshape(x.shape[axis], -1)
    return xm[:, np.asarray(lines)]


def worst(y, t, B):
    """(ratio, flat index) of the worst |y - t| / (2^-53 B) over the arrays; an element with B == 0 counts as 0 if y == 0 exactly
    and as inf otherwise."""
    y = np.asarray(y)
    err = np.abs(y.astype(LD) - t).astype(np.float64)
    B = np.asarray(B, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(B > 0, err / (U53 * B), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), k


def check(y, t, B, cap, what=""):
    """Asserts the bar; returns the worst ratio.  The message names the element."""
    r, k = worst(y, t, B)
    idx = tuple(int(v) for v in np.unravel_index(k, np.shape(y)))
    assert r <= cap, "%s: |y - truth| = %.3g x 2^-53 B at %s (cap %g; y = %r, truth = %r, B = %.3e)" % (
        what, r, idx, cap, float(np.asarray(y).reshape(-1)[k]), float(np.asarray(t).reshape(-1)[k]), float(np.asarray(B).reshape(-1)[k]))
    return r, idx


# ----------------------------------------------------------------------------------------------
# inputs: every generator returns an array of `shape` whose lines run along `axis`
# ----------------------------------------------------------------------------------------------
def _lineshape(shape, axis):
    s = list(shape)
    s[axis] = 1
    return s


def nlines(shape, axis):
    return int(np.prod(shape)) // shape[axis]


def noise(shape, axis, seed):
    return np.random.default_rng(seed).standard_normal(shape)


def scale_exponents(shape, axis, seed):
    """The per-line decimal exponent of `scaled`, integers in [-100, 100], shape with 1 along `axis`."""
    return np.random.default_rng(seed + 1).integers(-100, 101, size=_lineshape(shape, axis))


def scaled(shape, axis, seed):
    return np.random.default_rng(seed).standard_normal(shape) * 10.0 ** scale_exponents(shape, axis, seed)


def impulse(shape, axis, seed=0):
    """Line l (C order of the other indices) holds a single 1.0 at row (l + seed) mod K."""
    K = shape[axis]
    L = nlines(shape, axis)
    x = np.zeros((K, L))
    x[(np.arange(L) + seed) % K, np.arange(L)] = 1.0
    rest = [s for k, s in enumerate(shape) if k != axis]
    return np.ascontiguousarray(np.moveaxis(x.reshape([K] + rest), 0, axis))


def alternating(shape, axis, seed):
    """x_j = (-1)^j times a per-line N(0,1) constant: the largest outputs D can produce."""
    sg = np.where(np.arange(shape[axis]) & 1, -1.0, 1.0).reshape([shape[axis] if k == axis else 1 for k in range(len(shape))])
    return sg * np.random.default_rng(seed).standard_normal(_lineshape(shape, axis)) * np.ones(shape)


def constant(shape, axis, seed):
    """Constant lines: the null space of D."""
    return np.random.default_rng(seed).standard_normal(_lineshape(shape, axis)) * np.ones(shape)


def sparse_positions(L, seed, tile=32):
    """Line indices of the noise lines of `sparse_lines`: first, last, both sides of the first tile boundary that exists, and
    three seeded ones."""
    pos = {0, L - 1}
    for t in (tile, 64, 128):
        if t < L:
            pos.update((t - 1, t))
    pos.update(int(v) for v in np.random.default_rng(seed + 2).integers(0, L, size=3))
    return sorted(pos)


def sparse_lines(shape, axis, seed):
    K = shape[axis]
    L = nlines(shape, axis)
    x = np.zeros((K, L))
    pos = sparse_positions(L, seed)
    x[:, pos] = np.random.default_rng(seed).standard_normal((K, len(pos)))
    rest = [s for k, s in enumerate(shape) if k != axis]
    return np.ascontiguousarray(np.moveaxis(x.reshape([K] + rest), 0, axis))


GENERATORS = {"noise": noise, "scaled": scaled, "impulse": impulse, "alternating": alternating, "constant": constant,
              "sparse": sparse_lines}


# ----------------------------------------------------------------------------------------------
# plain double products the host test feeds through the bar (what an IEEE implementation gives)
# ----------------------------------------------------------------------------------------------
def product_double(M, x, axis):
    Md = np.asarray(M, dtype=np.float64)
    return np.moveaxis(np.tensordot(Md, np.asarray(x, dtype=np.float64), axes=([1], [axis])), 0, axis)


def product_evenodd(M, x, axis, sym):
    """The even / odd split of csrc/diffmat.cpp in double: E, O rounded once from long double, e = x_j + x_m-j, o = x_j - x_m-j,
    y_i = (E e)_i + (O o)_i, y_m-i = +-((E e)_i - (O o)_i)."""
    K = M.shape[0]
    m, H = K - 1, (K + 1) // 2
    E = ((M[:H, :H] + M[:H, ::-1][:, :H]) / 2).astype(np.float64)
    O = ((M[:H, :H] - M[:H, ::-1][:, :H]) / 2).astype(np.float64)
    if K & 1:
        E[:, H - 1] = np.asarray(M[:H, H - 1], dtype=np.float64)
        O[:, H - 1] = 0.0
    xm = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    xr = xm[::-1]
    e, o = xm[:H] + xr[:H], xm[:H] - xr[:H]
    if K & 1:
        e[H - 1] = xm[H - 1]
    a = np.tensordot(E, e, axes=([1], [0]))
    b = np.tensordot(O, o, axes=([1], [0]))
    y = np.empty_like(xm)
    y[:H] = a + b
    lo = (a - b) if sym else (b - a)
    y[m - np.arange(H)] = np.where((2 * np.arange(H) == m).reshape([H] + [1] * (xm.ndim - 1)), y[:H], lo)
    return np.moveaxis(y, 0, axis)


# ----------------------------------------------------------------------------------------------
# subsets of whole lines at full size (a condition the tests assert, not a measurement)
# ----------------------------------------------------------------------------------------------
def line_subset(shape, axis, seed, frac=0.02):
    """Sorted flat line indices (C order of the shape without `axis`) containing: the first and last 128 lines; for each
    non-transform index its first two and last two values crossed with a seeded sample of everything else; one full interior
    plane per non-transform axis; a seeded random sample; then topped up so that at least `frac` of the lines and every residue of
    the line index modulo 128 are covered."""
    rest = [s for k, s in enumerate(shape) if k != axis]
    L = int(np.prod(rest))
    rng = np.random.default_rng(seed)
    idx = np.arange(L).reshape(rest)
    sel = set(range(min(128, L))) | set(range(max(0, L - 128), L))
    for a, s in enumerate(rest):
        edge = sorted({0, min(1, s - 1), max(s - 2, 0), s - 1})
        sub = np.take(idx, edge, axis=a).reshape(-1)
        sel.update(int(v) for v in sub[rng.random(sub.size) < 0.25])
        sel.update(int(v) for v in np.take(idx, edge, axis=a).reshape(len(edge), -1)[:, :4].reshape(-1))
        if s > 2:
            sel.update(int(v) for v in np.take(idx, int(rng.integers(1, s - 1)), axis=a).reshape(-1))
    want = int(np.ceil(frac * L))
    sel.update(int(v) for v in rng.integers(0, L, size=want))
    for r in range(min(128, L)):                                # every residue of the line index modulo 128, in the interior too
        c = np.arange(r, L, 128)
        sel.add(int(c[rng.integers(0, c.size)]))
    return np.array(sorted(sel), dtype=np.int64)


def subset_coverage(lines, L):
    """(fraction of the L lines, number of residues modulo 128 present)."""
    lines = np.asarray(lines)
    return lines.size / float(L), np.unique(lines % 128).size


def plane_subset(n0, seed):
    """Indices along the outermost interior dimension for the EllipticOp subsets: first two, last two, two seeded interior ones."""
    rng = np.random.default_rng(seed)
    inner = rng.choice(np.arange(2, n0 - 2), size=2, replace=False) if n0 > 5 else []
    return np.array(sorted({0, 1, n0 - 2, n0 - 1} | {int(v) for v in inner}), dtype=np.int64)


# ----------------------------------------------------------------------------------------------
# the constant-coefficient elliptic operator: V = -sum_k L_k U on the interior tensor
# ----------------------------------------------------------------------------------------------
def elliptic_truth_bound(dims, U, planes=None):
    """(truth, B, factor) of MatMult_Elliptic at eta = 1 on the interior tensor U (shape dims - 2): truth = -sum_k L_k U in long
    double, B = sum_k B_k, factor = sum_k (K_k + 8) + d (one product per direction and d roundings for summing the terms).
    planes: indices along dimension 0 to restrict the output to."""
    d = len(dims)
    U = np.asarray(U, dtype=np.float64).reshape([p - 2 for p in dims])
    sel = slice(None) if planes is None else np.asarray(planes)
    t, B = None, None
    for k in range(d):
        Lk = dense_L(dims[k])
        if k == 0:
            tk, Bk = truth(Lk[sel], U, 0), bound_rows(Lk, sel, U)
        else:
            Us = U[sel]
            tk, Bk = truth(Lk, Us, k), bound(Lk, Us, k)
        t = tk if t is None else t + tk
        B = Bk if B is None else B + Bk
    return -t, B, sum(p - 2 + 8 for p in dims) + d


def bound_rows(M, sel, x):
    """bound(M, x, 0) restricted to the output rows sel."""
    A = np.abs(np.asarray(M, dtype=np.float64))
    A = 0.5 * (A + A[:, ::-1])[sel]
    ax = np.abs(np.asarray(x, dtype=np.float64))
    ax = ax + ax[::-1]
    return np.tensordot(A, ax, axes=([1], [0]))


def impulse_truth_bound(M, shape, axis, seed=0):
    """truth and bound of `impulse(shape, axis, seed)` without a product: line l is column j(l) = (l + seed) mod K of M (1.0 times
    an entry plus exact zeros), B_i = |M_ij| + |M_i,m-j|."""
    K = shape[axis]
    j = (np.arange(nlines(shape, axis)) + seed) % K
    A = np.abs(np.asarray(M, dtype=np.float64))
    rest = [s for k, s in enumerate(shape) if k != axis]
    t = np.moveaxis(np.asarray(M)[:, j].reshape([K] + rest), 0, axis)
    B = np.moveaxis((A[:, j] + A[:, K - 1 - j]).reshape([K] + rest), 0, axis)
    return t, B
