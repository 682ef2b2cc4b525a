"""Periodic (Fourier) directions restated in NumPy long double (helper module of test_periodic_host.py / test_gpu_periodic.py).

Conventions: n nodes x_j = -1 + 2 j / n; D_F = pi D_theta with D_theta[i][j] = 1/2 (-1)^(i-j) cot(pi (i-j) / n) for even
n, 1/2 (-1)^(i-j) / sin(pi (i-j) / n) for odd n; the second derivative is D_F D_F; the modes of -D_F D_F in the parity layout about
the flip j -> n-1-j (which reflects x about c = -1/n).  Every sine takes its argument as an integer multiple of pi / n, reduced in
integers and folded into [0, pi/2].  The `planted` arguments build the three wrong matrices the host tests must catch."""
import numpy as np

import linewise as lw

LD = np.longdouble
PI_L = lw.PI_L
U53 = lw.U53


def sin_pi(m, n):
    """sin(pi m / n) for integer arrays m, long double."""
    m = np.asarray(m, dtype=np.int64)
    r = np.mod(m, 2 * n)
    sg = np.where(r >= n, -1, 1)
    r = np.where(r >= n, r - n, r)
    r = np.where(2 * r > n, n - r, r)
    v = np.sin(PI_L * r.astype(LD) / LD(n))
    v = np.where(r == 0, LD(0), np.where(2 * r == n, LD(1), v))
    return sg * v


def cos_pi(m, n):
    return sin_pi(2 * np.asarray(m, dtype=np.int64) + n, 2 * n)


def nodes(n, planted=False):
    """x_j = -1 + 2 j / n; planted: the grid with a duplicated end point, -1 + 2 j / (n - 1)."""
    j = np.arange(n).astype(LD)
    return LD(-1) + LD(2) * j / LD(n - 1 if planted else n)


def diff_matrix(n, order=1, planted=None):
    """D_F (order 1) or D_F D_F (order 2) in long double.  planted = "cot": the even-n formula whatever n is; "textbook": for
    order 2 the textbook second-derivative matrix instead of the product."""
    i = np.arange(n)
    m = i[:, None] - i[None, :]
    s = sin_pi(m, n)
    s[i, i] = LD(1)
    sg = np.where(m & 1, LD(-1), LD(1))
    if n % 2 == 0 or planted == "cot":
        D = LD(0.5) * sg * cos_pi(m, n) / s
    else:
        D = LD(0.5) * sg / s
    D[i, i] = LD(0)
    D = PI_L * D
    if order == 1:
        return D
    if planted == "textbook":
        # theta-derivative matrices, Trefethen / Canuto: even n: -(-1)^m / (2 sin^2(m pi / n)), diagonal -n^2 / 12 - 1 / 6;
        # odd n: -(-1)^m cos(m pi / n) / (2 sin^2(m pi / n)), diagonal -(n^2 - 1) / 12
        if n % 2 == 0:
            D2 = -sg / (LD(2) * s * s)
            D2[i, i] = -(LD(n) * n / LD(12) + LD(1) / LD(6))
        else:
            D2 = -sg * cos_pi(m, n) / (LD(2) * s * s)
            D2[i, i] = -(LD(n) * n - LD(1)) / LD(12)
        return PI_L * PI_L * D2
    return np.dot(D, D)


def modes(n):
    """[(k, kind)] per coefficient position, kind "cos" / "sin" / "nyquist" (the docstring of sp.fourier_modes)."""
    K = (n - 1) // 2
    out = [None] * n
    out[0] = (0, "cos")
    for k in range(1, K + 1):
        out[k] = (k, "cos")
        out[n - k if n & 1 else n - 1 - k] = (k, "sin")
    if n % 2 == 0:
        out[n - 1] = (n // 2, "nyquist")
    return out


def mode_vector(n, k, kind):
    """Mode (k, kind) at the nodes with amplitude 1, long double: cos / sin (pi k (x_j - c)) = cos / sin (pi k (2 j + 1 - n) / n)."""
    j = np.arange(n)
    if kind == "nyquist":
        return np.where(j & 1, LD(-1), LD(1))
    a = k * (2 * j + 1 - n)
    return cos_pi(a, n) if kind == "cos" else sin_pi(a, n)


def modal_matrix(n, which):
    """B ("backward": column p = mode p) or T = B^-1 ("forward": row p = mode p times 1/n for the constant and the Nyquist vector,
    2/n otherwise), long double."""
    B = np.stack([mode_vector(n, k, kind) for k, kind in modes(n)], axis=1)
    if which == "backward":
        return B
    w = np.array([LD(1) if (kind == "nyquist" or k == 0) else LD(2) for k, kind in modes(n)]) / LD(n)
    return (B * w[None, :]).T


def line(n, scale=1.0):
    """(S, Sinv, lam) of -scale^2 D_F D_F in long double."""
    lam = np.array([LD(0) if (kind == "nyquist" or k == 0) else (PI_L * LD(k) * LD(scale)) ** 2 for k, kind in modes(n)])
    return modal_matrix(n, "backward"), modal_matrix(n, "forward"), lam


def ulps(a, t):
    """|a - t| in units of the spacing of doubles at a (a: double array, t: long double)."""
    a = np.asarray(a, dtype=np.float64)
    sp = np.spacing(np.abs(a))
    return float((np.abs(a.astype(LD) - t) / sp.astype(LD)).max())


# ----------------------------------------------------------------------------------------------
# handles with periodic directions: lines, layouts, operators
# ----------------------------------------------------------------------------------------------
def bc_entries(bc, periodic):
    """HelmholtzSolver's bc list: "periodic" on the flagged directions, bc[k] (default "dirichlet") elsewhere."""
    return ["periodic" if p else ("dirichlet" if bc is None else bc[k]) for k, p in enumerate(periodic)]


def lines(sp, dims, periodic, bc=None, scale=None):
    """Per direction (S, Sinv, lam) in double, from the library's host accessors (fdm_ref.lines with periodic directions)."""
    out = []
    for k, n in enumerate(dims):
        s = 1.0 if scale is None else float(scale[k])
        if periodic[k]:
            out.append(sp.fourier_line(n, s))
        else:
            out.append(tuple(sp.helmholtz_line_box(n, "dirichlet" if bc is None else bc[k], s)[:3]))
    return out


def unknown_shape(dims, periodic):
    return tuple(n if p else n - 2 for n, p in zip(dims, periodic))


def unknown_slices(periodic):
    return tuple(slice(None) if p else slice(1, -1) for p in periodic)


def dmat(sp, n, per, order=1):
    """The matrix a ChebGrad direction applies, long double: the uploaded Fourier matrix (rounded once by the library) or the
    closed-form CGL matrix of linewise / grad_ref."""
    if per:
        return sp.fourier_diff_matrix(n, order).astype(LD)
    D = lw.dense_D(n)
    return D if order == 1 else np.dot(D, D)


def derivs(sp, dims, periodic, x):
    """grad_ref.derivs with periodic directions: (t, B), t[j][k] = D_k x[j] in long double and its linewise weight."""
    t = [[lw.truth(dmat(sp, n, periodic[k]), x[j], k) for k, n in enumerate(dims)] for j in range(x.shape[0])]
    B = [[lw.bound(dmat(sp, n, periodic[k]), x[j], k) for k, n in enumerate(dims)] for j in range(x.shape[0])]
    return t, B


def laplacian(sp, dims, periodic, scale, x):
    """(truth, W) of sum_k s_k^2 M_k x[f], M = D D (CGL, n > 2) or D_F D_F; x: (nf, *dims); grad_ref.laplacian's bar."""
    d = len(dims)
    s = [1.0] * d if scale is None else [float(v) for v in scale]
    live = [k for k in range(d) if dims[k] > 2]
    T = len(live)
    nmax = max([dims[k] for k in live], default=0)
    tr = np.zeros(x.shape, dtype=LD)
    W = np.zeros(x.shape)
    for k in live:
        a = s[k] * s[k]
        M = dmat(sp, dims[k], periodic[k], 2)
        tr = tr + LD(a) * lw.truth(M, x, k + 1)
        W = W + (nmax + 8 + T) * a * lw.bound(M, x, k + 1)
    return tr, W


def wall_rows(sp, dims, periodic, bc, scale):
    """Per wall direction the two long-double rows of alpha u + beta s du/dnu at index 0 and n-1 (outward: +D at 0, -D at n-1);
    None on a periodic direction."""
    rows = []
    for k, n in enumerate(dims):
        if periodic[k]:
            rows.append(None)
            continue
        a0, b0, a1, b1 = sp.bc_array(["dirichlet" if bc is None else bc[k]], 1)
        s = LD(1.0 if scale is None else float(scale[k]))
        D = lw.dense_D(n)
        r0 = LD(b0) * s * D[0].copy()
        r0[0] += LD(a0)
        r1 = -LD(b1) * s * D[n - 1].copy()
        r1[n - 1] += LD(a1)
        rows.append((r0, r1))
    return rows


def boundary_mask(dims, periodic):
    """True at the nodes that are end nodes of some wall direction: the nodes of the compact boundary array g, row-major."""
    m = np.zeros(dims, dtype=bool)
    for k, n in enumerate(dims):
        if periodic[k]:
            continue
        idx = [slice(None)] * len(dims)
        for e in (0, n - 1):
            idx[k] = e
            m[tuple(idx)] = True
    return m
