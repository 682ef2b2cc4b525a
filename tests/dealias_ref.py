"""Reference side of the dealiasing tests (helper module of test_dealias_host.py / test_gpu_dealias.py): numpy long-double
restatements of R, P and G, the long-double application of the library's DOUBLE host matrices (the `truth` of the per-element
bars), the componentwise weights B, and the chebmul / chebder truncations of separable series.

Per direction of n coarse and m fine points: R (m x n) Lagrange interpolation, P (n x m) = B_n T_m[0:n, :], G (m x n) = R D_n.

The bars (first order, in units of 2^-53 B; one K + 8 per line product of K points as in linewise.py, which already counts the
rounding of a matrix entry):
    multiply   cap = 2 sum_k (n_k + 8) + 1 + sum_k (m_k + 8),  B = (x|P|) ((x|R| |u|) o (x|R| |v|))
               -- the way up of each of the two operands, one rounding for the product, the way down;
    advect     cap + d,                                        B = (x|P|) sum_k (x|R| |vel_k|) o (|G_k| in direction k |c|)
               -- d products and d - 1 additions instead of one product."""
import numpy as np
from numpy.polynomial import chebyshev as npc

import __graft_entry__ as ge
import linewise as lw

sp = ge.load()
LD = np.longdouble
U53 = 2.0 ** -53


def _cos_table(rows, cols, N):
    """cos(pi j k / N), j < rows, k < cols, long double, with j k reduced modulo 2N and folded into 0..N in integers."""
    j, k = np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64)
    r = (j[:, None] * k[None, :]) % (2 * N)
    r = np.where(r > N, 2 * N - r, r)
    m = N - 2 * r
    c = np.sign(m).astype(LD) * np.sin(lw.PI_L * np.abs(m).astype(LD) / LD(2 * N))
    c[m == 0] = 0
    return c


def R_ld(n, m):
    """Barycentric Lagrange interpolation from the n to the m CGL nodes, long double; shared nodes give exact unit rows."""
    ni, no = n - 1, m - 1
    j = np.arange(n, dtype=np.int64)

    def diff(i, a, jj, b):      # x_i (grid of a intervals) - x_jj (grid of b intervals) from the half-angles
        den = LD(2 * a * b)
        return -2 * np.sin(lw.PI_L * (i * b + jj * a).astype(LD) / den) * np.sin(lw.PI_L * (i * b - jj * a).astype(LD) / den)

    dd = diff(j[:, None], ni, j[None, :], ni)
    np.fill_diagonal(dd, 1)
    w = 1 / np.prod(dd, axis=1)
    R = np.zeros((m, n), dtype=LD)
    for i in range(m):
        hit = np.nonzero(i * ni == j * no)[0]
        if len(hit):
            R[i, hit[0]] = 1
            continue
        c = w / diff(np.int64(i), no, j, ni)
        R[i] = c / c.sum()
    return R


def P_ld(n, m, rows=None):
    """rows: only these rows (the long-double product is the cost at large n)."""
    rows = np.arange(n) if rows is None else np.asarray(rows)
    if m == n:
        return np.eye(n, dtype=LD)[rows]
    M = m - 1
    B = _cos_table(n, n, n - 1)                                  # B_n[i][k] = T_k(x_i)
    c = np.ones(m, dtype=LD); c[0] = c[M] = 2
    T = LD(2) / (LD(M) * c[:n, None] * c[None, :]) * _cos_table(n, m, M)      # T_m[k][j], k < n
    return np.dot(B[rows], np.asfortranarray(T))


def G_ld(n, m, rows=None):
    rows = np.arange(m) if rows is None else np.asarray(rows)
    return np.dot(R_ld(n, m)[rows], np.asfortranarray(lw.dense_D(n)))


_mats = {}


def mats(n, m):
    """The library's double (R, P, G) of one direction."""
    if (n, m) not in _mats:
        _mats[(n, m)] = tuple(sp.dealias_matrix(n, w, m) for w in "RPG")
    return _mats[(n, m)]


def fine_dims(dims):
    return tuple((3 * n + 1) // 2 for n in dims)


def apply(M, x, axis, dtype=LD):
    """M along `axis` of x (axis 0 of x is the field index; directions are axes 1 ..)."""
    y = np.tensordot(np.asarray(M).astype(dtype), np.asarray(x).astype(dtype), axes=([1], [axis]))
    return np.moveaxis(y, 0, axis)


def lift(dims, fine, x, g=-1, absolute=False):
    """(x R_k) x, direction g through G; absolute: |matrices| |x| in double (the weight), else long double (the truth)."""
    dt = np.float64 if absolute else LD
    y = np.abs(x) if absolute else x
    for k, (n, m) in enumerate(zip(dims, fine)):
        A = mats(n, m)[2 if k == g else 0]
        y = apply(np.abs(A) if absolute else A, y, k + 1, dt)
    return y


def lower(dims, fine, p, absolute=False):
    dt = np.float64 if absolute else LD
    y = p
    for k, (n, m) in enumerate(zip(dims, fine)):
        A = mats(n, m)[1]
        y = apply(np.abs(A) if absolute else A, y, k + 1, dt)
    return y


def cap_multiply(dims, fine):
    return 2 * sum(n + 8 for n in dims) + 1 + sum(m + 8 for m in fine)


def multiply_truth_bound(dims, fine, u, v):
    """u, v: (nfields,) + dims.  Long-double truth of the double matrices and the weight B."""
    t = lower(dims, fine, lift(dims, fine, u) * lift(dims, fine, v))
    B = lower(dims, fine, lift(dims, fine, u, absolute=True) * lift(dims, fine, v, absolute=True), absolute=True)
    return t, B


def advect_truth_bound(dims, fine, vel, c):
    """vel: (d,) + dims, c: (nfields,) + dims."""
    d = len(dims)
    V, Va = lift(dims, fine, vel), lift(dims, fine, vel, absolute=True)
    s = sum(V[k][None] * lift(dims, fine, c, g=k) for k in range(d))
    sa = sum(Va[k][None] * lift(dims, fine, c, g=k, absolute=True) for k in range(d))
    return lower(dims, fine, s), lower(dims, fine, sa, absolute=True)


def nodes(n):
    return np.cos(np.pi * np.arange(n) / (n - 1))


def separable(dims, coef):
    """prod_k series_k(x_k) on the grid: coef[k] holds direction k's Chebyshev coefficients."""
    out = np.ones(())
    for n, a in zip(dims, coef):
        out = np.multiply.outer(out, npc.chebval(nodes(n), a))
    return out


def trunc_mul(a, b, n):
    p = npc.chebmul(a, b)[:n]
    return np.pad(p, (0, n - len(p)))
