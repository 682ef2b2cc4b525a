"""The truth and the bar the cheb_points_spread tests share (the CPU model of tests/test_spread_host.py and the device tests of
tests/test_gpu_spread.py), on top of tests/points_ref.py.

Truth: g[f][i] = sum_p s[f][p] prod_k l_k,p[i_k] in numpy long double with the rows of points_ref.rows_ld (with delta: divided by
the product of the double Clenshaw-Curtis weights, in long double).

Bar, U = 2^-53:  |g_i - truth_i| <= cap U B_i,  B_i = sum_p |s_p| prod_k |l_k,p[i_k]|  (with delta: B_i / W_i),
    cap(dims, npts) = sum_k (Lambda(n_k) n_k + 8) + d + npts      (+ d + 1 with delta)
Per row entry Lambda n + 3 -- three roundings (two differences and a quotient) and the normalising sum of n terms amplified by the
Lebesgue constant, as for eval -- of which the bar keeps eval's Lambda n + 8; d products ((s l_1) .. l_{d-1} and the product with
direction 0's entry); npts additions in any order.  With delta the kernel multiplies by d inverse weights, each rounded once: 2 d
roundings, which the d + 1 of the bar and the 5 spare roundings per direction cover.

The float64 model restates the device algorithm in numpy: rows by the nearest-node formula in double (sum in ascending j), the
image ((s l_1) l_2 ..) l_{d-1}, then the points added one after the other."""
import numpy as np

import points_ref as pref

sp = pref.sp
LD = np.longdouble
U = pref.U


def cap(dims, npts, delta=False):
    d = len(dims)
    return sum(pref.lam(n) * n + 8.0 for n in dims) + d + npts + (d + 1 if delta else 0)


def rows_all_ld(dims, pts):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, len(dims))
    return [pref.rows_ld(n, pts[:, k]) for k, n in enumerate(dims)]


def outer(rows):
    """L[p][i] = prod_k rows[k][p][i_k], i row-major: (npts, prod(dims)) in the rows' type."""
    L = rows[0]
    for r in rows[1:]:
        L = (L[:, :, None] * r[:, None, :]).reshape(L.shape[0], -1)
    return L


def weights_ld(dims):
    """prod_k w_k[i_k], flat, long double products of the double weights."""
    return outer([sp.cc_weights(n).astype(LD)[None, :] for n in dims])[0]


def truth(dims, s, L, delta=False):
    """(truth (nf, prod(dims)) long double, B (nf, prod(dims)) double) for strengths s (nf, npts) and L = outer(rows_all_ld) (or its
    leading npts rows)."""
    s = np.asarray(s, dtype=np.float64)
    npts = s.shape[1]
    N = int(np.prod(dims))
    if npts == 0:
        return np.zeros((s.shape[0], N), dtype=LD), np.zeros((s.shape[0], N))
    with np.errstate(invalid="ignore", over="ignore"):
        t = s.astype(LD) @ L[:npts]
        b = (np.abs(s).astype(LD) @ np.abs(L[:npts]))
        if delta:
            W = weights_ld(dims)
            t, b = t / W, b / W
    return t, b.astype(np.float64)


def worst_ratio(g, t, B, c):
    """max |g - t| / (c U B) over the elements (0 / 0 = 0; anything / 0 = inf)."""
    err = np.abs(np.asarray(g).reshape(t.shape).astype(LD) - t).astype(np.float64)
    bar = c * U * B
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


# ---- the float64 model of the device algorithm ----------------------------------------------------------------------------------
def rows_f64(n, x):
    """The value rows of k_points_rows in numpy double (the sum in ascending j)."""
    xn = sp.cgl_nodes(n)
    x = np.asarray(x, dtype=np.float64).ravel()
    N, m = n - 1, x.size
    d = x[:, None] - xn[None, :]
    s = np.argmin(np.abs(d), axis=1)
    ar = np.arange(m)
    ds = d[ar, s]
    j = np.arange(n)
    h = np.where((j == 0) | (j == N), 0.5, 1.0)
    ihs = np.where((s == 0) | (s == N), 2.0, 1.0)
    sign = np.where((j[None, :] - s[:, None]) & 1, -1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (sign * h[None, :]) * ihs[:, None] * (ds[:, None] / d)
    r[ar, s] = 1.0
    tot = np.zeros(m)
    for c in range(n):
        tot = tot + r[:, c]
    l = r / tot[:, None]
    on = ds == 0
    l[on] = 0.0
    l[on, s[on]] = 1.0
    return l


def spread_model(dims, s, pts, delta=False):
    """The device algorithm in double: (nf, prod(dims))."""
    dims = tuple(dims)
    s = np.asarray(s, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, len(dims))
    rows = [rows_f64(n, pts[:, k]) for k, n in enumerate(dims)]
    nf, npts = s.shape
    N = int(np.prod(dims))
    g = np.zeros((nf, dims[0], N // dims[0]))
    for p in range(npts):
        X = s[:, p][:, None]                                         # ((s l_1) l_2 ..) l_{d-1}
        for k in range(1, len(dims)):
            X = (X[:, :, None] * rows[k][p][None, None, :]).reshape(nf, -1)
        g = g + rows[0][p][None, :, None] * X[:, None, :]
    if delta:
        iw = [(LD(1) / sp.cc_weights(n).astype(LD)).astype(np.float64) for n in dims]
        wl = np.ones(1)
        for k in range(len(dims) - 1, 0, -1):
            wl = (iw[k][:, None] * wl[None, :]).reshape(-1)
        g = (g * iw[0][None, :, None]) * wl[None, None, :]
    return g.reshape(nf, N)


def eval_model(dims, u, pts):
    """Evaluation in double with the same rows, direction 0 first: (nf, npts)."""
    dims = tuple(dims)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, len(dims))
    rows = [rows_f64(n, pts[:, k]) for k, n in enumerate(dims)]
    nf = u.size // int(np.prod(dims))
    t = np.einsum("pi,fi...->pf...", rows[0], u.reshape((nf,) + dims))
    for k in range(len(dims) - 1, 0, -1):
        t = np.einsum("p...i,pi->p...", t, rows[k])
    return t.T
