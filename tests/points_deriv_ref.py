"""The truth and the bars the derivative-at-points tests share (tests/test_points_deriv_host.py on the CPU,
tests/test_gpu_points_deriv.py on the device), on top of tests/points_ref.py and tests/spread_ref.py.

Truth: the derivative rows of include/chebhip.h in numpy long double on the double node table cgl_nodes(n) (sums in ascending j),
  c_j = w_j / w_s,  q_j = c_j / d_j,  r_j = q_j d_s  (j != s),  R = 1 + sum r,  Q2 = sum q_k / d_k,  T = sum q_k (x_s - x_k) / d_k
  l'_j = (q_j / R) ((1 + d_s^2 Q2) / R - d_s / d_j),   l'_s = -T / R^2
and the majorant a_j >= |l'_j| the errors are relative to (every sum replaced by the sum of absolute values):
  a_j = (|q_j| / |R|) ((1 + d_s^2 sum |q_k / d_k|) / |R| + |d_s / d_j|),   a_s = sum |q_k (x_s - x_k) / d_k| / R^2

cap1d(n) = 2 (n + 2) Lambda(n) + n + 16 bounds an entry's error in units of U a_j.  The count, for j != s (l'_s needs less):
  q_j                      2   (the difference d_j, the quotient)
  q_j / R                  1 + (n + 2) Lambda: R is a sum of n terms of 3 roundings each (d_j, d_s / d_j or q_j, the product),
                               n - 1 additions in any order, so |dR| <= (n + 2) U sum |r|, and sum |r| / |R| = sum |l| <= Lambda
  1 + d_s^2 Q2             3 (d_s twice, the square) + 1 (the product) + 1 (the addition) + (n + 2) for Q2: terms of 4 roundings
                               (q_k: 2, d_k, the quotient) and n - 2 additions
  (..) / R                 1 + (n + 2) Lambda
  d_s / d_j                3, no more than the first term's share, which the majorant adds to it
  the difference, product  2
in all 2 (n + 2) Lambda + n + 13; 3 more for the terms of second order.  A direction's share of a result's bar is cap1d(n) plus the
contraction's n + 5 of points_ref.cap1 (cap1 = Lambda n + 3 for an entry, n + 5 for the contraction)."""
import numpy as np

import points_ref as pref

sp = pref.sp
LD = np.longdouble
U = pref.U


def cap1d(n):
    return 2.0 * (n + 2) * pref.lam(n) + n + 16.0


def cap(dims, deriv=None, scaled=False):
    """The bar of eval / eval_grid / eval_grad in units of U B': cap1 per value direction, cap1d + n + 5 per derivative direction,
    one more rounding where a scale multiplies."""
    deriv = deriv or (0,) * len(dims)
    return sum(cap1d(n) + n + 5.0 if a else pref.cap1(n) for n, a in zip(dims, deriv)) + (1.0 if scaled else 0.0)


def spread_cap(dims, npts, deriv=None, delta=False):
    """spread_ref.cap with the derivative directions' entry terms: Lambda n + 8 becomes cap1d(n) + 5."""
    deriv = deriv or (0,) * len(dims)
    d = len(dims)
    return sum(cap1d(n) + 5.0 if a else pref.lam(n) * n + 8.0 for n, a in zip(dims, deriv)) + d + npts + (d + 1 if delta else 0)


def _parts(n, x, T=LD):
    """The pieces of the formula in type T, sums left to the caller: (s, ds, d, q (0 at s), diff x_s - x_j, finite mask)."""
    xn = sp.cgl_nodes(n).astype(T)
    x = np.asarray(x, dtype=np.float64).ravel()
    fin = np.isfinite(x)
    xt = np.where(fin, x, 0.0).astype(T)
    N, m = n - 1, x.size
    d = xt[:, None] - xn[None, :]
    s = np.argmin(np.abs(d), axis=1)                     # the first minimum: the lowest index on a tie
    ar = np.arange(m)
    ds = d[ar, s]
    j = np.arange(n)
    h = np.where((j == 0) | (j == N), T(0.5), T(1))
    c = np.where((j[None, :] - s[:, None]) & 1, T(-1), T(1)) * h[None, :] / h[s][:, None]
    dd = d.copy()
    dd[ar, s] = 1                                        # (never used: q is 0 there)
    q = c / dd
    q[ar, s] = 0
    diff = xn[s][:, None] - xn[None, :]
    return s, ds, dd, q, diff, fin


def _asc(a):
    """Row sums in ascending j."""
    t = np.zeros(a.shape[0], dtype=a.dtype)
    for c in range(a.shape[1]):
        t = t + a[:, c]
    return t


def _desc(a):
    return _asc(a[:, ::-1])


def drows(n, x, T=LD, total=_asc, fault=None):
    """(l' (len(x), n), majorant a (len(x), n)) in type T; NaN rows for non-finite coordinates.  total: the row sum.  fault plants
    an error for the tests that must see one: "end" (an end weight not halved), "drop" (one term missing from l'_s), "sign" (the
    sign of d_s / d_j)."""
    s, ds, d, q, diff, fin = _parts(n, x, T)
    m = len(s)
    ar = np.arange(m)
    if fault == "end":
        q = q.copy()
        q[:, 0] = np.where(s == 0, q[:, 0], 2 * q[:, 0])
    R = 1 + total(q * ds[:, None])
    Q2 = total(q / d)
    tt = q * diff / d
    if fault == "drop":
        tt = tt.copy()
        tt[ar, (s + 1) % n] = 0
    Tt = total(tt)
    dsd = ds[:, None] / d
    g0 = (1 + ds * ds * Q2) / R
    lp = q / R[:, None] * (g0[:, None] + dsd if fault == "sign" else g0[:, None] - dsd)
    lp[ar, s] = -Tt / (R * R)
    A = np.abs(q) / np.abs(R)[:, None] * (((1 + ds * ds * total(np.abs(q / d))) / np.abs(R))[:, None] + np.abs(dsd))
    A[ar, s] = total(np.abs(tt)) / (R * R)
    lp[~fin] = np.nan
    A[~fin] = np.nan
    return lp, A


def drows_ld(n, x):
    return drows(n, x)


def rows_kinds(dims, pts, deriv):
    """Per direction the long-double rows (l or l') and their magnitudes (|l| or the majorant a, double) of the points pts."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, len(dims))
    rows, mags = [], []
    for k, n in enumerate(dims):
        if deriv[k]:
            l, a = drows_ld(n, pts[:, k])
            rows.append(l); mags.append(a.astype(np.float64))
        else:
            l = pref.rows_ld(n, pts[:, k])
            rows.append(l); mags.append(np.abs(l).astype(np.float64))
    return rows, mags


def first_products(dims, nf, u, row0, mag0):
    """Direction 0 of values_ld, the expensive part, so that the components of a gradient can share it: (t, b) as [p][f, rest]."""
    dims = tuple(dims)
    x = np.moveaxis(u.reshape((nf,) + dims), 1, 0).reshape(dims[0], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = row0 @ x.astype(LD)
        b = mag0 @ np.abs(x)
    npts = row0.shape[0]
    return t.reshape((npts, nf) + dims[1:]), b.reshape((npts, nf) + dims[1:])


def later_products(t, b, rows, mags):
    """The later directions of values_ld, last first: (value[f][p] long double, B'[f][p] double)."""
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(rows) - 1, 0, -1):
            t = np.einsum("p...i,pi->p...", t, rows[k])
            b = np.einsum("p...i,pi->p...", b, mags[k])
    return t.T, b.T


def values_ld(dims, nf, u, rows, mags):
    """points_ref.values_ld with mixed row kinds: value[f][p] = sum prod rows u in long double, B'[f][p] = sum prod mags |u|."""
    t, b = first_products(dims, nf, u, rows[0], mags[0])
    return later_products(t, b, rows, mags)


def worst(out, value, B, c):
    """max |out - value| / (c U B) (0 / 0 = 0, anything / 0 = inf; NaN where both are NaN counts as 0)."""
    out = np.asarray(out).reshape(value.shape)
    both = np.isnan(out) & np.isnan(value.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(out.astype(LD) - value).astype(np.float64)
        r = np.where((err == 0) | both, 0.0, err / (c * U * B))
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0
