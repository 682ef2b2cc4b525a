"""Reference side of the periodic toolbox tests (test_periodic_toolbox_host.py / test_gpu_periodic_toolbox.py): NumPy
long-double restatements of the formulas, the truths and the derived bars.  On top of periodic_ref.py (sin_pi / cos_pi with their
arguments reduced in integers), dealias_ref.py, project_ref.py, points_ref.py and points_deriv_ref.py.

Conventions: n nodes x_j = -1 + 2 j / n, period 2, K = floor(n / 2).  The interpolant of n periodic values is sum_j u_j r_j(x),
    n odd:   r_j(x) = (1/n) [1 + 2 sum_{k=1}^{K} cos pi k (x - x_j)]
    n even:  r_j(x) = (1/n) [1 + 2 sum_{k=1}^{K-1} cos pi k (x - x_j) + cos pi K (x - x_j)]
which equals the barycentric form r_j ~ (-1)^j cot(pi (x - x_j) / 2) (n even), (-1)^j / sin(pi (x - x_j) / 2) (n odd).

Dealiasing matrices (m >= n fine nodes y_i = -1 + 2 i / m), every cosine the integer multiple 2 k a of pi / (n m):
    R[i][j] = r_j(y_i), a = i n - j m (a fine node that is a coarse node: the exact unit row);   G = R D_F;
    P[i][j] = (1/m) [1 + 2 sum_{k=1}^{K} cos pi k (x_i - y_j)], a = i m - j n; exact 0 where (2K + 1) a is a multiple of n m and a is
    not (the zeros of the Dirichlet kernel); m == n: the identity.
The sums run in ascending k from the 1, as the library's do, so the two agree to the rounding of the result.

The rows of k_points_frows and their bars.  U = 2^-53; the device's sinpi / cospi are taken at 2 ulp = 4 U.  With a = pi d_s / 2,
b = pi m / n (m = (s - j) mod n), S = sin a cos b + cos a sin b, C = cos a cos b - sin a sin b, Chat = |cos a cos b| + |sin a sin b|:
    d_s 0 (exact);  sin a 4;  cos a 4;  tan a 4 + 4 + 1 = 9;  table entries 1 each;  each product of S and C 4 + 1 + 1 = 6;
    S: 6 (|t1| + |t2|) + |S| <= 19 |S| since |t1| + |t2| <= 3 |S| (|tan a / tan b| <= 1/2);  C: 6 Chat + |C| <= 7 Chat
    n odd:   e = +-sin a / S                 4 + 19 + 1 = 24 |e|     n even:  e = +-tan a (C / S)             9 + 27 + 1 = 37 ehat
             p = +-h cos a / S               4 + 19 + 3 = 26 |p|              p = +-h (C / S) / cos^2 a        27 + 9 + 3 = 39 phat
             f = -+h sin a C / S^2           4 + 7 + 1 + 39 + 3 = 54 fhat     f = -+h tan a / S^2              9 + 39 + 3 = 51 |f|
    with ehat = |tan a| Chat / |S| (even; |e| odd), phat = h Chat / (|S| cos^2 a) (even; |p| odd), fhat = h |sin a| Chat / S^2 (odd; |f|
    even).  C_E = 37, C_P = 39, C_F = 54 bound both parities.  A row's sums have at most ceil(n / G) + log2 G <= A = 10 additions.
    value    r_j = e_j / R:  |dr_j| <= U [C_E ehat_j / |R| + |r_j| ((C_E + A) Rhat / |R| + 1)] <= CAP_ROWS U M_j,
             M_j = (ehat_j / |R|) (Rhat / |R|), Rhat = 1 + sum ehat, CAP_ROWS = 2 C_E + A + 1 + 3 (second order) = 88
    deriv    r'_j = (f_j R + p_j - e_j F) / R^2, r'_s = -(P + F) / R^2:  with Nhat_j = fhat_j Rhat + phat_j + ehat_j Fhat (Nhat_s =
             Phat + Fhat): the numerator (C_F + C_E + A + 3) Nhat, R^2 and the quotient (2 (C_E + A) Rhat / |R| + 2) |r'|, so
             |dr'_j| <= CAP_DROWS U M'_j, M'_j = (Nhat_j / R^2) (Rhat / |R|), CAP_DROWS = 54 + 37 + 10 + 3 + 94 + 2 + 4 = 204
d_s is the device's: the wrapped coordinate minus the DOUBLE node fourier_nodes(n)[s], an exact difference; the rows are those of
the point x_s + d_s with x_s the exact node, i.e. of x moved by the node's rounding (at most 2^-54).  The truth is the same closed
form in long double from that d_s."""
import numpy as np

import dealias_ref as dr
import linewise as lw
import periodic_ref as pr
import points_ref as pref

sp = dr.sp
LD = np.longdouble
PI_L = lw.PI_L
U = 2.0 ** -53

C_E, C_P, C_F, A_SUM = 37.0, 39.0, 54.0, 10.0
CAP_ROWS = 2 * C_E + A_SUM + 1 + 3
CAP_DROWS = C_F + C_E + A_SUM + 3 + 2 * (C_E + A_SUM) + 2 + 4


# ----------------------------------------------------------------------------------------------
# dealiasing matrices
# ----------------------------------------------------------------------------------------------
def fine_size(n):
    return 3 * (n // 2) + 1


def _cos_table(nm):
    """cos(2 pi t / nm), t = 0 .. nm - 1: every cosine of R and P once (cos_pi reduces its argument in integers, so the entry of
    t = k a mod nm is the cosine of 2 k a pi / nm bit for bit)."""
    return pr.cos_pi(2 * np.arange(nm, dtype=np.int64), nm)


def R_ld(n, m):
    K = n // 2
    Kfull = K if n & 1 else K - 1
    i, j = np.arange(m, dtype=np.int64), np.arange(n, dtype=np.int64)
    a = i[:, None] * n - j[None, :] * m
    tab = _cos_table(n * m)
    s = np.ones((m, n), dtype=LD)
    for k in range(1, Kfull + 1):
        s = s + LD(2) * tab[(k * a) % (n * m)]
    if n % 2 == 0:
        s = s + tab[(K * a) % (n * m)]
    R = s / LD(n)
    for r in range(m):
        if (r * n) % m == 0:
            R[r] = 0
            R[r, r * n // m] = 1
    return R


def P_ld(n, m, planted=None):
    """planted = "half": the Nyquist wavenumber K of an even n with half weight (the interpolant's weight, wrong for P)."""
    if m == n:
        return np.eye(n, dtype=LD)
    K = n // 2
    i, j = np.arange(n, dtype=np.int64), np.arange(m, dtype=np.int64)
    a = i[:, None] * m - j[None, :] * n
    tab = _cos_table(n * m)
    s = np.ones((n, m), dtype=LD)
    for k in range(1, K + 1):
        w = LD(1) if (planted == "half" and n % 2 == 0 and k == K) else LD(2)
        s = s + w * tab[(k * a) % (n * m)]
    P = s / LD(m)
    if planted is None:
        P[(a % (n * m) != 0) & (((2 * K + 1) * a) % (n * m) == 0)] = 0
    return P


def G_ld(n, m):
    return np.dot(R_ld(n, m), pr.diff_matrix(n))


def mode(n, k, kind, x):
    """cos / sin (pi k (x + 1)) at the points x (long double); the Nyquist vector of an even n is kind "cos", k = n / 2."""
    t = PI_L * LD(k) * (np.asarray(x, dtype=LD) + LD(1))
    return np.cos(t) if kind == "cos" else np.sin(t)


def exact_cut(n, ku, kindu, kv, kindv):
    """The truncation to |k| <= K of the product of two modes, at the coarse nodes: the product's two wavenumbers ku +- kv, each
    kept if at most K.  At K itself (even n) the coarse grid sees cos pi K (x + 1) = (-1)^j and no sine."""
    K = n // 2
    x = pr.nodes(n)
    # cos a cos b = (cos(a-b) + cos(a+b)) / 2, sin a sin b = (cos(a-b) - cos(a+b)) / 2, sin a cos b = (sin(a+b) + sin(a-b)) / 2
    if kindu == "cos" and kindv == "cos":
        terms = [(abs(ku - kv), "cos", 0.5), (ku + kv, "cos", 0.5)]
    elif kindu == "sin" and kindv == "sin":
        terms = [(abs(ku - kv), "cos", 0.5), (ku + kv, "cos", -0.5)]
    else:
        ks, kc = (ku, kv) if kindu == "sin" else (kv, ku)
        terms = [(ks + kc, "sin", 0.5), (abs(ks - kc), "sin", 0.5 if ks >= kc else -0.5)]
    out = np.zeros(n, dtype=LD)
    for k, kind, c in terms:
        if k <= K:
            out = out + LD(c) * mode(n, k, kind, x)
    return out


def mats(n, m, periodic):
    """The library's double (R, P, G) of one direction."""
    if not periodic:
        return dr.mats(n, m)
    return tuple(sp.dealias_matrix(n, w, m, periodic=True) for w in "RPG")


def default_fine(dims, periodic):
    return tuple(fine_size(n) if p else (3 * n + 1) // 2 for n, p in zip(dims, periodic))


def lift(dims, fine, periodic, x, g=-1, absolute=False):
    dt = np.float64 if absolute else LD
    y = np.abs(x) if absolute else x
    for k, (n, m) in enumerate(zip(dims, fine)):
        Am = mats(n, m, periodic[k])[2 if k == g else 0]
        y = dr.apply(np.abs(Am) if absolute else Am, y, k + 1, dt)
    return y


def lower(dims, fine, periodic, p, absolute=False):
    dt = np.float64 if absolute else LD
    y = p
    for k, (n, m) in enumerate(zip(dims, fine)):
        Am = mats(n, m, periodic[k])[1]
        y = dr.apply(np.abs(Am) if absolute else Am, y, k + 1, dt)
    return y


def multiply_truth_bound(dims, fine, periodic, u, v):
    """dealias_ref.multiply_truth_bound with the matrices of each direction's basis; the cap is dealias_ref.cap_multiply (the count
    of roundings does not depend on what the matrices hold)."""
    t = lower(dims, fine, periodic, lift(dims, fine, periodic, u) * lift(dims, fine, periodic, v))
    B = lower(dims, fine, periodic, lift(dims, fine, periodic, u, absolute=True) * lift(dims, fine, periodic, v, absolute=True), absolute=True)
    return t, B


def advect_truth_bound(dims, fine, periodic, vel, c):
    d = len(dims)
    V, Va = lift(dims, fine, periodic, vel), lift(dims, fine, periodic, vel, absolute=True)
    s = sum(V[k][None] * lift(dims, fine, periodic, c, g=k) for k in range(d))
    sa = sum(Va[k][None] * lift(dims, fine, periodic, c, g=k, absolute=True) for k in range(d))
    return lower(dims, fine, periodic, s), lower(dims, fine, periodic, sa, absolute=True)


# ----------------------------------------------------------------------------------------------
# rows at arbitrary points
# ----------------------------------------------------------------------------------------------
def wrap(x):
    x = np.asarray(x, dtype=LD)
    return x - LD(2) * np.rint(LD(0.5) * x)


def cosine_rows(n, x, deriv=False):
    """The host twins' formula: the cosine sums of r_j (or r_j') with t = wrap(x) - x_j, k t reduced modulo 2, ascending k."""
    K = n // 2
    Kfull = K if n & 1 else K - 1
    x = np.asarray(x, dtype=np.float64).ravel()
    fin = np.isfinite(x)
    xr = wrap(np.where(fin, x, 0.0))
    j = np.arange(n)
    dj = xr[:, None] - ((2 * j - n).astype(LD) / LD(n))[None, :]
    acc = np.zeros(dj.shape, dtype=LD) if deriv else np.ones(dj.shape, dtype=LD)

    def cs(k):
        r = np.fmod(LD(k) * dj, LD(2))
        return np.cos(PI_L * r), np.sin(PI_L * r)
    for k in range(1, Kfull + 1):
        c, s = cs(k)
        acc = acc + (LD(-2) * (PI_L * LD(k)) * s if deriv else LD(2) * c)
    if n % 2 == 0:
        c, s = cs(K)
        acc = acc + (-(PI_L * LD(K)) * s if deriv else c)
    out = acc / LD(n)
    out[~fin] = np.nan
    return out


def _closed(n, x):
    """The pieces of the closed form in long double: (s, ds, e, p, f, ehat, phat, fhat, finite mask); the entries at s are 0."""
    x = np.asarray(x, dtype=np.float64).ravel()
    fin = np.isfinite(x)
    xr = wrap(np.where(fin, x, 0.0))
    c = np.rint((xr + LD(1)) * LD(n) / LD(2)).astype(np.int64)              # 0 .. n; n is node 0 one period on
    xn = np.append(sp.fourier_nodes(n), 1.0).astype(LD)                      # the double nodes; node 0 one period on is +1
    ds = xr - xn[c]                                                           # exact
    s = c % n
    j = np.arange(n)
    m = (s[:, None] - j[None, :]) % n
    sb, cb = pr.sin_pi(m, n), pr.cos_pi(m, n)
    a = PI_L * ds / LD(2)
    sa, ca = np.sin(a)[:, None], np.cos(a)[:, None]
    sg = np.where(m & 1, LD(-1), LD(1))
    S = sa * cb + ca * sb
    Cc = ca * cb - sa * sb
    Ch = np.abs(ca * cb) + np.abs(sa * sb)
    S[np.arange(len(s)), s] = 1                                               # (never used)
    h = PI_L / LD(2)
    if n & 1:
        e, p, f = sg * sa / S, h * sg * ca / S, -h * sg * sa * Cc / (S * S)
        eh, ph, fh = np.abs(e), np.abs(p), h * np.abs(sa) * Ch / (S * S)
    else:
        ta = sa / ca
        e, p, f = sg * ta * Cc / S, h * sg * (Cc / S) / (ca * ca), -h * sg * ta / (S * S)
        eh, ph, fh = np.abs(ta) * Ch / np.abs(S), h * Ch / (np.abs(S) * ca * ca), np.abs(f)
    ar = np.arange(len(s))
    for q in (e, p, f, eh, ph, fh):
        q[ar, s] = 0
    return s, ds, e, p, f, eh, ph, fh, fin


def rows_ld(n, x):
    """(rows (len(x), n) long double, majorant M double): the value rows and the weight of their bar CAP_ROWS U M."""
    s, ds, e, p, f, eh, ph, fh, fin = _closed(n, x)
    ar = np.arange(len(s))
    e[ar, s] = 1
    eh[ar, s] = 1
    R, Rh = e.sum(axis=1), eh.sum(axis=1)
    r = e / R[:, None]
    M = (eh / np.abs(R)[:, None]) * (Rh / np.abs(R))[:, None]
    on = ds == 0
    r[on] = 0
    r[on, s[on]] = 1
    r[~fin] = np.nan
    M[~fin] = np.nan
    return r, M.astype(np.float64)


def drows_ld(n, x):
    """(derivative rows, majorant M'), bar CAP_DROWS U M'."""
    s, ds, e, p, f, eh, ph, fh, fin = _closed(n, x)
    ar = np.arange(len(s))
    R, Rh = 1 + e.sum(axis=1), 1 + eh.sum(axis=1)
    F, Fh, P, Ph = f.sum(axis=1), fh.sum(axis=1), p.sum(axis=1), ph.sum(axis=1)
    num = f * R[:, None] + p - e * F[:, None]
    nh = fh * Rh[:, None] + ph + eh * Fh[:, None]
    num[ar, s] = -(P + F)
    nh[ar, s] = Ph + Fh
    d = num / (R * R)[:, None]
    M = nh / (R * R)[:, None] * (Rh / np.abs(R))[:, None]
    d[~fin] = np.nan
    M[~fin] = np.nan
    return d, M.astype(np.float64)


def bary_rows(n, x):
    """The barycentric cot / csc form itself, normalised by its sum (finite x off the nodes), long double."""
    x = np.asarray(x, dtype=np.float64).ravel()
    xr = wrap(x)
    j = np.arange(n)
    t = PI_L * (xr[:, None] - ((2 * j - n).astype(LD) / LD(n))[None, :]) / LD(2)
    sg = np.where(j & 1, LD(-1), LD(1))[None, :]
    w = sg / np.sin(t) if n & 1 else sg * np.cos(t) / np.sin(t)
    return w / w.sum(axis=1)[:, None]


def rows_kinds(dims, periodic, pts, deriv):
    """points_deriv_ref.rows_kinds with periodic directions: per direction (rows long double, magnitudes double, cap of an entry)."""
    import points_deriv_ref as pdr
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, len(dims))
    rows, mags, caps = [], [], []
    for k, n in enumerate(dims):
        if periodic[k]:
            l, a = (drows_ld if deriv[k] else rows_ld)(n, pts[:, k])
            rows.append(l); mags.append(a); caps.append((CAP_DROWS if deriv[k] else CAP_ROWS) + n + 5.0)
        elif deriv[k]:
            l, a = pdr.drows_ld(n, pts[:, k])
            rows.append(l); mags.append(a.astype(np.float64)); caps.append(pdr.cap1d(n) + n + 5.0)
        else:
            l = pref.rows_ld(n, pts[:, k])
            rows.append(l); mags.append(np.abs(l).astype(np.float64)); caps.append(pref.cap1(n))
    return rows, mags, caps


def grid_nodes(n, periodic):
    return sp.fourier_nodes(n) if periodic else sp.cgl_nodes(n)


def quad_weights(n, periodic):
    return np.full(n, 2.0 / n) if periodic else sp.cc_weights(n)


# ----------------------------------------------------------------------------------------------
# projection: the divergence of the result in long double and its bar (project_ref.div_ratio on the solver's geometry)
# ----------------------------------------------------------------------------------------------
def out_weights(dims, periodic, scale, u, phi):
    s = [1.0] * len(dims) if scale is None else [float(v) for v in scale]
    t, W = [], []
    for k, n in enumerate(dims):
        D = pr.dmat(sp, n, periodic[k])
        t.append(np.asarray(u[k]).astype(LD) - LD(s[k]) * lw.truth(D, phi, k))
        W.append((n + 8) * (s[k] * lw.bound(D, phi, k) + np.abs(u[k])))
    return np.stack(t), np.stack(W)


def dropped_modes(dims, periodic):
    """The right eigenvectors of the dropped modes of a singular channel handle on the unknown nodes: constant along every wall
    direction, and per periodic direction the constant or, for an even extent, the Nyquist vector: 2^e vectors, e the number of
    periodic directions of even extent (one vector, the constant, when there is none)."""
    import itertools
    shape = pr.unknown_shape(dims, periodic)
    even = [k for k, n in enumerate(dims) if periodic[k] and n % 2 == 0]
    out = []
    for pick in itertools.product((0, 1), repeat=len(even)):
        v = np.ones(shape)
        for k, on in zip(even, pick):
            if on:
                sh = [1] * len(dims)
                sh[k] = dims[k]
                v = v * np.where(np.arange(dims[k]) & 1, -1.0, 1.0).reshape(sh)
        out.append(v.reshape(-1))
    return np.stack(out, axis=1)


def div_ratio(dims, periodic, scale, u, phi, out, eps, spread):
    """project_ref.div_ratio with each direction's own matrix, over the UNKNOWN nodes (every node of a periodic direction, the
    interior of a wall one).  spread (walls only in the wall directions, the handle singular): the divergence is free along the
    dropped modes -- what is held to the bar is its distance from their span (dropped_modes; the least-squares remainder).  With
    the constant alone that is project_ref's max - min <= bar, i.e. each value within bar / 2 of the constant; the projector onto
    2^e orthogonal +-1 vectors has infinity norm at most 2^e, so a divergence within bar / 2 of the span leaves a remainder of at
    most (1 + 2^e) bar / 2, which is the bar used."""
    d = len(dims)
    s = [1.0] * d if scale is None else [float(v) for v in scale]
    inner = pr.unknown_slices(periodic)
    _, W = out_weights(dims, periodic, scale, u, phi)
    dv = np.zeros(dims, dtype=LD)
    rnd = np.zeros(dims)
    Bu = np.zeros(dims)
    dd = 0.0
    for k, n in enumerate(dims):
        D = pr.dmat(sp, n, periodic[k])
        dv = dv + LD(s[k]) * lw.truth(D, out[k], k)
        rnd = rnd + s[k] * np.moveaxis(np.tensordot(np.abs(D.astype(np.float64)), U * W[k], axes=([1], [k])), 0, k)
        Bu = Bu + s[k] * lw.bound(D, u[k], k)
        D2 = pr.dmat(sp, n, periodic[k], 2).astype(np.float64)
        dd += s[k] * s[k] * float(np.abs(D2).sum(axis=1).max())
    rnd = rnd + U * (max(dims) + 8 + d) * Bu
    bar = eps * dd + float(rnd[inner].max())
    dv = dv[inner]
    if not spread:
        return float(np.abs(dv).max()) / bar
    Q = dropped_modes(dims, periodic).astype(LD)
    flat = dv.reshape(-1)
    rem = flat - np.dot(Q, np.dot(Q.T, flat) / LD(flat.size))
    return float(np.abs(rem).max()) / (bar * (1 + Q.shape[1]) / 2)


def face_table(dims, periodic):
    """Per compact boundary node 2 k + end of the highest WALL direction in which it is an end node, row-major boundary order."""
    idx = np.indices(dims)
    code = np.full(dims, -1, dtype=np.int64)
    for k, n in enumerate(dims):
        if periodic[k]:
            continue
        code[idx[k] == 0] = 2 * k
        code[idx[k] == n - 1] = 2 * k + 1
    return code[pr.boundary_mask(dims, periodic)]


_records = {}


def record(name, ratio, cap=None):
    """Keeps the worst ratio per bar; written by the GPU suite's last test."""
    old = _records.get(name, (0.0, cap))
    _records[name] = (max(old[0], float(ratio)), cap)


def records():
    return dict(_records)
