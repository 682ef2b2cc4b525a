"""The truth the cheb_points_* tests compare against: the barycentric nearest-node formula of include/chebhip.h restated in numpy
long double on the double node table cgl_nodes(n), with the operations in the order of the host twin (sum in ascending j)."""
import numpy as np

import __graft_entry__ as ge

sp = ge.load()
LD = np.longdouble
U = 2.0 ** -53
TINY = 2.0 ** -1022


def lam(n):
    """Bound of the Lebesgue constant of n CGL points."""
    return 1.0 + 2.0 / np.pi * np.log(n)


def cap1(n):
    return (1.0 + lam(n)) * n + 8.0


def cap(dims):
    return sum(cap1(n) for n in dims)


def rows_ld(n, x):
    """(len(x), n) long-double rows; NaN rows for non-finite coordinates, exact unit rows on nodes."""
    xn = sp.cgl_nodes(n).astype(LD)
    x = np.asarray(x, dtype=np.float64).ravel()
    fin = np.isfinite(x)
    xt = np.where(fin, x, 0.0).astype(LD)
    N, m = n - 1, x.size
    d = xt[:, None] - xn[None, :]
    s = np.argmin(np.abs(d), axis=1)                     # the first minimum: the lowest index on a tie
    ar = np.arange(m)
    ds = d[ar, s]
    j = np.arange(n)
    h = np.where((j == 0) | (j == N), LD(0.5), LD(1))
    sign = np.where((j[None, :] - s[:, None]) & 1, LD(-1), LD(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = sign * h[None, :] / h[s][:, None] * (ds[:, None] / d)
    r[ar, s] = 1
    tot = np.zeros(m, dtype=LD)
    for c in range(n):
        tot = tot + r[:, c]
    l = r / tot[:, None]
    on = ds == 0
    l[on] = 0
    l[on, s[on]] = 1
    l[~fin] = np.nan
    return l


def values_ld(dims, nf, u, rows):
    """(value, B) of the points whose rows (one (npts, n_k) long-double array per direction) are given: value[f][p] in long double,
    B[f][p] = sum prod |l| |u| in double."""
    dims = tuple(dims)
    npts = rows[0].shape[0]
    t = rows[0] @ np.moveaxis(u.reshape((nf,) + dims).astype(LD), 1, 0).reshape(dims[0], -1)          # [p][f, rest]
    b = np.abs(rows[0]).astype(np.float64) @ np.abs(np.moveaxis(u.reshape((nf,) + dims), 1, 0).reshape(dims[0], -1))
    t = t.reshape((npts, nf) + dims[1:])
    b = b.reshape((npts, nf) + dims[1:])
    for k in range(len(dims) - 1, 0, -1):                # the later directions, last first: [p][f, ..., i_k] . l_k[p][i_k]
        t = np.einsum("p...i,pi->p...", t, rows[k])
        b = np.einsum("p...i,pi->p...", b, np.abs(rows[k]).astype(np.float64))
    return t.T, b.T
