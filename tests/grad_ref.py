"""Long-double truth and bars for ChebGrad and ChebLayout (helper module of test_grad_host.py / test_gpu_grad.py /
test_gpu_layout.py), built on linewise.py.

Linear operators.  Every output is a list of terms factor * M_k u_j (M = D, or D D for the Laplacian), added in a fixed order.
With the per-element weight B of linewise.bound, |factor| B_t bounds one term's sweep error in units of (n_t + 8) 2^-53, and the
T - 1 additions each round a partial sum that sum_t B_t bounds, so

    |out - truth| <= 2^-53 W,      W = (max_t n_t + 8 + T) sum_t B_t.

A direction of more than 256 points of the Laplacian is two D sweeps: its term enters W as (2 (n + 8) + T) s^2 |D| (|D| |u|)
instead (the first sweep's error carried through the second, plus the second's own).  `terms(op, d)` is the table of the
operators; `derivs` computes D_k u_j and its weight once, so that every first-order operator and every scale shares one product.

Invariants.  `invariants(G)` evaluates the table of include/chebhip.h in long double and returns, per name, (value, A, T): A is
the formula with every term taken non-negative and the bar is (T + 4) 2^-53 A."""
import numpy as np

import linewise as lw

LD = np.longdouble
U = 2.0 ** -53
NAMES = ("div", "vort2", "strain2", "gamma", "q", "norm2")           # the order of the CHEB_INV_* bits


def npairs(d):
    return [(c, k) for c in range(d) for k in range(c, d)]


def terms(op, d):
    """Per output of ONE vector (one scalar for grad / laplacian) the list of (direction k, input component j, sign factor f,
    scale power): the term f * s_k^power * M_k u_j."""
    if op == "grad":
        return [[(k, 0, 1.0)] for k in range(d)]
    if op == "tensor":
        return [[(k, c, 1.0)] for c in range(d) for k in range(d)]
    if op == "div":
        return [[(k, k, 1.0) for k in range(d)]]
    if op == "curl":
        if d == 2:
            return [[(0, 1, 1.0), (1, 0, -1.0)]]
        assert d == 3
        return [[((i + 1) % 3, (i + 2) % 3, 1.0), ((i + 2) % 3, (i + 1) % 3, -1.0)] for i in range(3)]
    if op == "strain":
        return [[(c, c, 1.0)] if c == k else [(k, c, 0.5), (c, k, 0.5)] for c, k in npairs(d)]
    raise ValueError(op)


def fields_in(op, d):
    return 1 if op in ("grad", "laplacian") else d


def derivs(dims, x):
    """x: (nf, *dims).  (t, B) with t[j][k] = D_k x[j] in long double and B[j][k] its weight (double)."""
    t = [[lw.truth(lw.dense_D(n), x[j], k) for k, n in enumerate(dims)] for j in range(x.shape[0])]
    B = [[lw.bound(lw.dense_D(n), x[j], k) for k, n in enumerate(dims)] for j in range(x.shape[0])]
    return t, B


def first_order(op, dims, scale, dv, nunits):
    """(truth, W) of `op` for nunits vectors (scalars for grad) from derivs' tables dv: arrays (nunits * outputs, *dims)."""
    t, B = dv
    d = len(dims)
    s = [1.0] * d if scale is None else [float(v) for v in scale]
    per = fields_in(op, d)
    tt, WW = [], []
    for v in range(nunits):
        for out in terms(op, d):
            tr = np.zeros(dims, dtype=LD)
            Bs = np.zeros(dims)
            for k, j, f in out:
                tr = tr + LD(f) * LD(s[k]) * t[v * per + j][k]
                Bs = Bs + abs(f * s[k]) * B[v * per + j][k]
            tt.append(tr)
            WW.append((max(dims[k] for k, _, _ in out) + 8 + len(out)) * Bs)
    return np.stack(tt), np.stack(WW)


_DD = {}


def dense_DD(n):
    """D D on all n points in long double (dense_L's construction without the cut)."""
    if n not in _DD:
        D = lw.dense_D(n)
        _DD[n] = np.dot(D, D)
    return _DD[n]


def laplacian(dims, scale, x):
    """(truth, W) of sum_k s_k^2 d_k^2 x[f]; x: (nf, *dims)."""
    d = len(dims)
    s = [1.0] * d if scale is None else [float(v) for v in scale]
    live = [k for k in range(d) if dims[k] > 2]
    T = sum(1 if dims[k] <= 256 else 2 for k in live)
    one = [k for k in live if dims[k] <= 256]
    nmax = max([dims[k] for k in one], default=0)
    tr = np.zeros(x.shape, dtype=LD)
    W = np.zeros(x.shape)
    for k in live:
        n, a = dims[k], s[k] * s[k]
        if n <= 256:
            M = dense_DD(n)
            tr = tr + LD(a) * lw.truth(M, x, k + 1)
            W = W + (nmax + 8 + T) * a * lw.bound(M, x, k + 1)
        else:
            D = lw.dense_D(n)
            tr = tr + LD(a) * lw.truth(D, lw.truth(D, x, k + 1), k + 1)
            W = W + (2 * (n + 8) + T) * a * lw.bound(D, lw.bound(D, x, k + 1), k + 1)
    return tr, W


def invariants(G):
    """G: (d, d, ...) one vector's tensor.  {name: (value in long double, A in double, T)}."""
    d = G.shape[0]
    g = np.asarray(G).astype(LD)
    z = np.zeros(g.shape[2:], dtype=LD)
    div, adiv, sd, so, vo, nr = z, z, z, z, z, z
    for c in range(d):
        div = div + g[c, c]
        adiv = adiv + np.abs(g[c, c])
        sd = sd + g[c, c] * g[c, c]
    for c in range(d):
        for k in range(c + 1, d):
            vo = vo + (g[k, c] - g[c, k]) ** 2
            so = so + (g[c, k] + g[k, c]) ** 2
    for c in range(d):
        for k in range(d):
            nr = nr + g[c, k] * g[c, k]
    st = sd + LD(0.5) * so
    f = lambda a: np.asarray(a, dtype=np.float64)
    Tv, Ts = d * (d - 1) // 2, d * (d + 1) // 2
    return {"div": (div, f(adiv), d), "vort2": (vo, f(vo), Tv), "strain2": (st, f(st), Ts), "gamma": (LD(0.5) * st, f(LD(0.5) * st), Ts),
            "q": (LD(0.25) * vo - LD(0.5) * st, f(LD(0.25) * vo + LD(0.5) * st), Tv + Ts), "norm2": (nr, f(nr), d * d)}


def ratio(y, t, W):
    """Worst |y - t| / (2^-53 W) over the arrays (linewise.worst): at most 1 when the bar holds."""
    return lw.worst(y, t, W)[0]


# ----------------------------------------------------------------------------------------------
# ChebLayout: the boolean interior mask, and the maps it implies
# ----------------------------------------------------------------------------------------------
def interior_mask(dims):
    m = np.zeros(dims, dtype=bool)
    m[tuple(slice(1, n - 1) for n in dims)] = True
    return m


def layout_map(dims):
    """The table of cheb_layout_*: interior nodes numbered row-major from 0, boundary nodes -1 - (row-major number)."""
    inside = interior_mask(dims).ravel()
    m = np.empty(inside.size, dtype=np.int64)
    m[inside] = np.arange(inside.sum())
    m[~inside] = -1 - np.arange((~inside).sum())
    return m.reshape(dims)


def unpack(dims, ncomp, xi, si, oi, xb, sb, ob):
    """The numpy scatter: (ncomp, *dims) from the interleaved interior array xi and the compact boundary array xb (None: zeros)."""
    inside = interior_mask(dims).ravel()
    out = np.zeros((ncomp, inside.size))
    for c in range(ncomp):
        if xi is not None:
            out[c, inside] = np.asarray(xi).reshape(-1, si)[:, oi + c]
        if xb is not None:
            out[c, ~inside] = np.asarray(xb).reshape(-1, sb)[:, ob + c]
    return out.reshape((ncomp,) + tuple(dims))
