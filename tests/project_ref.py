"""numpy model and bars of the box Helmholtz solve and of ChebProject (helper module of test_project_host.py /
test_gpu_project.py).

The model.  D is the float64 differentiation matrix of tests/test_gpu_helmholtz_bc.py (`cheb_d`).  A direction of scale s with
ends (alpha, beta) has the line of DESIGN 10c for the ends (alpha, beta s), its operator and lift times s^2 (`scaled_line`).
`dense_helmholtz` solves the eliminated interior system with np.linalg.solve and rebuilds the boundary direction by direction;
sigma = 0 with alpha = 0 everywhere is singular and the system is bordered with the left null vector (the Kronecker product of the
lines' left null vectors) and the constant vector, which is the solver's rule (no component of the solution along the dropped
mode, that part of the right-hand side discarded).  `face_table` is the edge rule: a boundary node takes the condition of the
highest direction in which it is an end node.  `project` composes divergence, right-hand sides, solve and gradient.

The bars (one definition for the model on the CPU and for the library on the GPU).
  out      |out_k - (u_k - s_k D_k phi)| <= (n_k + 8) 2^-53 (s_k B(D_k, phi) + |u_k|) element by element, truth and B in
           long double from the phi that came back (linewise.py's bar with an accumulator).
  eps      1e-9 max|phi|: the loosest bar the tests of solve_full hold that solve to; every property bar below is this error of
           phi carried through the operator that follows it, plus the rounding of the sweeps where the property passes through them.
  div      sum_k s_k D_k out_k at the interior nodes in long double.  out = u - G phi + delta with |delta_k| <= 2^-53 W_k (the out
           bar), and phi solves the collocation problem for the divergence the library computed, which is within
           2^-53 (max n + 8 + d) sum_k s_k B(D_k, u_k) of div u (grad_ref.py).  So
             |div out (- c)| <= eps sum_k s_k^2 ||(DD)_k||_inf + max_i [sum_k s_k |D_k| 2^-53 W_k + 2^-53 (max n + 8 + d) sum_k s_k B(D_k, u_k)]_i.
           With an open face the bound is on the divergence, with walls only on its spread max - min (the constant c is free).
  normal   |+-out_k - flux| <= eps s_k ||D_k||_inf at every node that takes a wall's condition, k that wall's direction.
  idem     |P(P u) - P u| <= eps max_k s_k ||D_k||_inf, eps of the first call.
  grad     |P(grad psi)| <= eps max_k s_k ||D_k||_inf at every node, eps of that call.  psi is N(0,1) at the nodes and 0 at the
           nodes that take an OPEN face's condition: phi = 0 there, so phi = psi (and a zero result) needs psi = 0 there."""
import numpy as np

import linewise as lw

LD = np.longdouble
U53 = 2.0 ** -53
WALL, OPEN = (0.0, 1.0), (1.0, 0.0)          # (alpha, beta) of phi's condition


def cheb_d(P):
    n = P - 1
    i = np.arange(P)
    I, J = np.meshgrid(i, i, indexing="ij")
    c = np.where((i == 0) | (i == n), 2.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dx = -2.0 * np.sin(np.pi * (I + J) / (2 * n)) * np.sin(np.pi * (I - J) / (2 * n))
        D = (c[:, None] / c[None, :]) * (-1.0) ** (I + J) / dx
        s = np.sin(np.pi * i / n)
        dg = -np.cos(np.pi * i / n) / (2.0 * s * s)
    dg[0] = (2.0 * n * n + 1.0) / 6.0
    dg[n] = -dg[0]
    D[i, i] = dg
    return D


def scaled_line(P, e4, s=1.0):
    """(A~, Q, L, Binv) of a line of P points, ends e4 = (alpha_first, beta_first, alpha_last, beta_last), scale s:
    B_row = [a0 e_0 + b0 s D_0; a1 e_n - b1 s D_n], Q = -B_BB^-1 B_BI, A~ = -s^2 ((DD)_II + (DD)_IB Q), L = s^2 (DD)_IB B_BB^-1."""
    a0, b0, a1, b1 = e4
    n = P - 1
    D = cheb_d(P)
    DD = D @ D
    B = np.vstack([b0 * s * D[0], -b1 * s * D[n]])
    B[0, 0] += a0
    B[1, n] += a1
    b00, b01, b10, b11 = B[0, 0], B[0, n], B[1, 0], B[1, n]
    # the 2 x 2 inverse in closed form: np.linalg.inv pivots once beta s |D_n0| > alpha and then loses cond(B_BB) ~ s n^2 units
    Binv = np.array([[b11, -b01], [-b10, b00]]) / (b00 * b11 - b01 * b10)
    Q = -Binv @ B[:, 1:n]
    DDib = DD[1:n][:, [0, n]]
    return s * s * (-DD[1:n, 1:n] - DDib @ Q), Q, s * s * (DDib @ Binv), Binv


def boundary_mask(dims):
    m = np.ones(dims, dtype=bool)
    m[tuple(slice(1, -1) for _ in dims)] = False
    return m


def interior(a, dims):
    """The interior values of one full-grid field, flat."""
    return np.asarray(a).reshape(dims)[tuple(slice(1, -1) for _ in dims)].ravel()


def face_grid(dims):
    """Per node 2 k + end of the face whose condition it takes (k the highest direction in which it is an end node; end 0 is
    index 0), -1 at interior nodes."""
    idx = np.indices(dims)
    code = np.full(dims, -1, dtype=np.int64)
    for k, n in enumerate(dims):                 # ascending: the highest direction writes last
        code[idx[k] == 0] = 2 * k
        code[idx[k] == n - 1] = 2 * k + 1
    return code


def face_table(dims):
    """face_grid at the boundary nodes, in row-major boundary order: the table of cheb_project_faces_host."""
    return face_grid(dims)[boundary_mask(dims)]


def kinds_of(bc, d):
    """[(first, last)] * d of 'wall' / 'open' from ChebProject's bc (None: walls)."""
    if bc is None:
        return [("wall", "wall")] * d
    return [(e, e) if isinstance(e, str) else tuple(e) for e in bc]


def ends_of(kinds):
    """HelmholtzSolver's bc of phi: (0, 1) at a wall, (1, 0) at an open face."""
    return [tuple(WALL if e == "wall" else OPEN for e in pair) for pair in kinds]


def scales(scale, d):
    return [1.0] * d if scale is None else [float(v) for v in scale]


def apply(M, x, axis):
    return np.moveaxis(np.tensordot(M, x, axes=([1], [axis])), 0, axis)


def dense_helmholtz(dims, bc_ends, scale, sigma, f_int, g):
    """(sigma - sum_k s_k^2 d_k^2) u = f at the interior nodes, alpha u + beta s_k du/dnu = g at the boundary nodes (edge rule),
    by a dense solve.  bc_ends: per direction ((a0, b0), (a1, b1)).  Returns the full-grid u."""
    d = len(dims)
    s = scales(scale, d)
    Ms = [P - 2 for P in dims]
    lines = [scaled_line(P, bc_ends[k][0] + bc_ends[k][1], s[k]) for k, P in enumerate(dims)]
    Gn = int(np.prod(Ms))
    A = sigma * np.eye(Gn)
    for k in range(d):
        mats = [np.eye(m) for m in Ms]
        mats[k] = lines[k][0]
        K = mats[0]
        for Mk in mats[1:]:
            K = np.kron(K, Mk)
        A += K
    Gf = np.zeros(dims)
    Gf[boundary_mask(dims)] = g
    rhs = np.asarray(f_int, dtype=np.float64).reshape(Ms).copy()
    inner = [slice(1, -1)] * d
    for k in range(d):
        Lk = lines[k][2]
        for e, idx in enumerate((0, -1)):
            sl = list(inner); sl[k] = idx
            rhs += np.moveaxis(np.multiply.outer(Lk[:, e], Gf[tuple(sl)]), 0, k)
    singular = sigma == 0.0 and all(a == 0.0 for pair in bc_ends for a, _ in pair)
    if singular:
        w = np.ones(1)
        for k in range(d):
            uu, _, _ = np.linalg.svd(lines[k][0])
            w = np.kron(w, uu[:, -1])                # left null vector of the line: A~^T w = 0
        Ab = np.zeros((Gn + 1, Gn + 1))
        Ab[:Gn, :Gn] = A
        Ab[:Gn, Gn] = 1.0                            # the constants: the null space of A
        Ab[Gn, :Gn] = w / np.abs(w).max()
        u = np.linalg.solve(Ab, np.append(rhs.ravel(), 0.0))[:Gn]
    else:
        u = np.linalg.solve(A, rhs.ravel())
    U = np.zeros(dims)
    U[tuple(inner)] = u.reshape(Ms)
    for k in range(d):
        _, Q, _, Bi = lines[k]
        sl = tuple([slice(None)] * (k + 1) + [slice(1, -1)] * (d - k - 1))
        V = np.moveaxis(U[sl], k, -1).copy()
        Gd = np.moveaxis(Gf[sl], k, -1)
        end = V[..., 1:-1] @ Q.T + Gd[..., [0, -1]] @ Bi.T
        V[..., 0], V[..., -1] = end[..., 0], end[..., 1]
        U[sl] = np.moveaxis(V, -1, k)
    return U


def boundary_data(dims, kinds, u, flux=None):
    """g of the solver for ONE vector u (d, *dims): per boundary node of face (k, e), +u_k (e = 0) or -u_k (e = 1), minus the flux if
    one is given, at a wall; 0 at an open face.  Values are moved and negated, the flux is one subtraction: the bits k_project_rhs
    writes."""
    d = len(dims)
    mask = boundary_mask(dims)
    code = face_table(dims)
    g = np.zeros(code.size)
    for k in range(d):
        uk = np.asarray(u[k]).reshape(dims)[mask]
        for e in range(2):
            sel = code == 2 * k + e
            if kinds[k][e] == "wall":
                g[sel] = uk[sel] if e == 0 else -uk[sel]
                if flux is not None:
                    g[sel] = g[sel] - np.asarray(flux)[sel]
            elif kinds[k][e] != "open":
                raise ValueError(kinds[k][e])
    return g


def project(dims, bc, scale, u, flux=None):
    """(out, phi) of ONE vector u (d, *dims) in float64 numpy: the dense model of ChebProject.project."""
    d = len(dims)
    s = scales(scale, d)
    kinds = kinds_of(bc, d)
    u = np.asarray(u, dtype=np.float64).reshape((d,) + tuple(dims))
    Ds = [cheb_d(n) for n in dims]
    div = sum(s[k] * apply(Ds[k], u[k], k) for k in range(d))
    phi = dense_helmholtz(dims, ends_of(kinds), scale, 0.0, -interior(div, dims), boundary_data(dims, kinds, u, flux))
    out = np.stack([u[k] - s[k] * apply(Ds[k], phi, k) for k in range(d)])
    return out, phi


# ----------------------------------------------------------------------------------------------
# the bars (module docstring); every function returns value / bar, at most 1 when the bar holds
# ----------------------------------------------------------------------------------------------
def norm_inf(M):
    return float(np.abs(np.asarray(M, dtype=np.float64)).sum(axis=1).max())


def d_norms(dims, scale):
    """(s_k ||D_k||_inf per k, sum_k s_k^2 ||(DD)_k||_inf)."""
    s = scales(scale, len(dims))
    Ds = [lw.dense_D(n) for n in dims]
    return [s[k] * norm_inf(Ds[k]) for k in range(len(dims))], sum(s[k] * s[k] * norm_inf(np.dot(Ds[k], Ds[k])) for k in range(len(dims)))


def out_weights(dims, scale, u, phi):
    """(truth, W) of out_k = u_k - s_k D_k phi: long double, and the weight of the per-element bar 2^-53 W."""
    s = scales(scale, len(dims))
    t, W = [], []
    for k, n in enumerate(dims):
        D = lw.dense_D(n)
        t.append(np.asarray(u[k]).astype(LD) - LD(s[k]) * lw.truth(D, phi, k))
        W.append((n + 8) * (s[k] * lw.bound(D, phi, k) + np.abs(u[k])))
    return np.stack(t), np.stack(W)


def out_ratio(dims, scale, u, phi, out):
    t, W = out_weights(dims, scale, u, phi)
    return lw.worst(out, t, W)[0]


def div_ratio(dims, scale, u, phi, out, eps, spread):
    """Interior divergence of `out` in long double against the div bar; spread: max - min instead of max |.|."""
    d = len(dims)
    s = scales(scale, d)
    inner = tuple(slice(1, -1) for _ in dims)
    _, W = out_weights(dims, scale, u, phi)
    dv = np.zeros(dims, dtype=LD)
    rnd = np.zeros(dims)
    Bu = np.zeros(dims)
    for k, n in enumerate(dims):
        D = lw.dense_D(n)
        dv = dv + LD(s[k]) * lw.truth(D, out[k], k)
        rnd = rnd + s[k] * apply(np.abs(D.astype(np.float64)), U53 * W[k], k)
        Bu = Bu + s[k] * lw.bound(D, u[k], k)
    rnd = rnd + U53 * (max(dims) + 8 + d) * Bu
    bar = eps * d_norms(dims, scale)[1] + float(rnd[inner].max())
    dv = dv[inner]
    val = float(dv.max() - dv.min()) if spread else float(np.abs(dv).max())
    return val / bar


def normal_ratio(dims, kinds, scale, out, flux, eps):
    """Worst |normal component - flux| / (eps s_k ||D_k||_inf) over the nodes that take a wall's condition."""
    sD, _ = d_norms(dims, scale)
    mask = boundary_mask(dims)
    code = face_table(dims)
    fl = np.zeros(code.size) if flux is None else np.asarray(flux)
    worst = 0.0
    for k in range(len(dims)):
        ok = np.asarray(out[k]).reshape(dims)[mask]
        for e in range(2):
            sel = code == 2 * k + e
            if kinds[k][e] == "wall" and sel.any():
                nrm = ok[sel] if e == 0 else -ok[sel]
                worst = max(worst, float(np.abs(nrm - fl[sel]).max()) / (eps * sD[k]))
    return worst


def node_ratio(dims, scale, diff, eps):
    """max |diff| / (eps max_k s_k ||D_k||_inf): the bar of idempotence and of projected gradients."""
    return float(np.abs(diff).max()) / (eps * max(d_norms(dims, scale)[0]))


def psi_field(dims, kinds, seed):
    """N(0,1) at the nodes, 0 at the nodes that take an open face's condition."""
    psi = np.random.default_rng(seed).standard_normal(dims)
    code = face_grid(dims)
    for k in range(len(dims)):
        for e in range(2):
            if kinds[k][e] == "open":
                psi[code == 2 * k + e] = 0.0
    return psi
