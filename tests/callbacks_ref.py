"""Element-by-element checks of the Stokes and Jacobian callbacks (helper module of test_callbacks_host.py and
test_gpu_callbacks.py): a NumPy long-double twin of the truths and weights of oracle/cheb_oracle.c (orc_stokes_truth,
orc_stokes_function_truth, orc_elliptic_truth, orc_elliptic_function_truth), plain double restatements of the operators, the
caps, the input families and the impulse positions.

The bar, for every output element:   |y_i - truth_i| <= cap 2^-53 W_i,   W_i = 0 demands y_i == 0 exactly.

W is the truth's own evaluation with every factor replaced by its absolute value and every line product by the symmetrised
weight of linewise.bound, x -> 1/2 (|D| + |D| flip)(|x| + flip |x|), which dominates the plain product, the even / odd split
product and (|D D| <= |D||D|) a product with the rounded D D matrices of the uniform-viscosity route.  The extrapolated
pressure's weight is built from |D| and the |Lagrange weights| separately, so it bounds the folded matrix and the
faces-then-sweep form alike.  For `function`, W is the weight of the operator linearised about the state the call leaves
(S0 = s), applied to |xL| with the Dirichlet values, plus |force|: to first order delta tau = eta delta s + eta' s (s : delta s).

The caps: roundings counted to first order, K = the longest line, d = dimensions.
  gradient G_j = D_j u                       K + 8     (linewise.py: matrix entry, e / o, K multiply-adds, recombination, alpha)
  node loop, relative to the stress weight:
    s = (G_jk + G_kj) / 2                    1         (the halving is exact)
    z = S0 : s                               d^2       (d^2 products, d^2 - 1 additions: at most d^2 per term in any order)
    eta' S0_jk z                             2
    eta s_jk  (+ eta' S0_jk z)               1         (the product is the shorter branch; one rounding for the sum)
                                             = d^2 + 4
  divergence -sum_j D_j tau_jk               K + 8 + d (d sweeps, d roundings to add their terms)
  + D_k p_ext, - force                       2         (the pressure's own chain -- K + 2 for the face values, K + 8 for the
                                                        sweep -- is shorter than the viscous one and sits on its own weight;
                                                        folded into the stress it costs the one subtraction counted here)
  velocity rows:   cap_v = 2 (K + 8) + d^2 + d + 6     (2 K + 34 for d = 3, 2 K + 28 for d = 2)
  pressure rows:   cap_p = K + 8 + d                   (the trace of the gradient)
`function` adds the rheology: gamma = s : s / 2 carries the gradient's error through the linearised weight (above) and
d^2 + 1 roundings of its own; q = eps + gamma / gamma0 two; eta = B q^p one and the device pow's POW_ULPS; eta' = B p / gamma0
(q^p / q) four and POW_ULPS.  On the residual they act through eta s_jk:  cap_fn = cap_v + d^2 + 4 + POW_ULPS.
  strain:  (K + 10) 2^-53 of its own symmetrised weight (gradient + symmetrisation + 1 spare).
  eta, eta': relative.  With wgamma = sum_jk |s_jk| ws_jk:  dq = ((K + 9) wgamma + (d^2 + 1) gamma) / gamma0 + 2 q  (units of
    2^-53), |d eta| / |eta| <= |p| dq / q + 1 + POW_ULPS,  |d eta'| / |eta'| <= (|p| + 1) dq / q + 4 + POW_ULPS.
POW_ULPS is the one measured number: the ROCm installation carries no documented bound for double pow, so the allowance is
twice the worst error seen against powl on the q values of these tests, rounded up to an integer
(test_gpu_callbacks.py::test_device_pow_ulps measures it: 1.32 ulps on an MI355X, hence 3).
The scalar operator: gradient K + 8; flux eta g_k + eta' u g0_k: 4; divergence K + 8 + d:  cap_e = 2 (K + 8) + d + 4;
`function` adds eta = 1 + gamma u^2 (3) and - b (1): cap_e + 4; with a general exponent eta = 1 + gamma pow(u, e): + POW_ULPS."""
import numpy as np

import linewise as lw

LD = np.longdouble
U53 = lw.U53
POW_ULPS = 3


# ----------------------------------------------------------------------------------------------
# caps
# ----------------------------------------------------------------------------------------------
def cap_v(dims, fn=False, power=False):
    K, d = max(dims), len(dims)
    return 2 * (K + 8) + d * d + d + 6 + ((d * d + 4 + (POW_ULPS if power else 0)) if fn else 0)


def cap_p(dims):
    return max(dims) + 8 + len(dims)


def cap_strain(dims):
    return max(dims) + 10


def cap_e(dims, fn=False, power=False):
    return 2 * (max(dims) + 8) + len(dims) + 4 + ((4 + (POW_ULPS if power else 0)) if fn else 0)


def eta_bounds(dims, rheology, tr):
    """Relative bounds (units of 2^-53) of eta and eta' from the dict of orc.stokes_function_truth."""
    kind, B, n, eps, g0 = rheology
    d, K = len(dims), max(dims)
    s = tr["strain"].reshape(d, -1, d)
    gam = 0.5 * (s * s).sum(axis=(0, 2))
    q = eps + gam / g0
    pw = abs((1.0 - n) / (2.0 * n))
    dq = ((K + 9) * tr["wgamma"] + (d * d + 1) * gam) / g0 + 2 * q
    return pw * dq / q + 1 + POW_ULPS, (pw + 1) * dq / q + 4 + POW_ULPS


# ----------------------------------------------------------------------------------------------
# grid helpers (layouts of oracle/cheb_oracle.h: full global vector [v_0 .. v_{d-1}, p] per interior node)
# ----------------------------------------------------------------------------------------------
def inner(dims):
    return tuple(slice(1, -1) for _ in dims)


def idims(dims):
    return tuple(p - 2 for p in dims)


def sizes(dims):
    """(N, I, g, dv)"""
    d, N, I = len(dims), int(np.prod(dims)), int(np.prod(idims(dims)))
    return N, I, (d + 1) * I, d * (N - I)


def boundary_mask(dims):
    m = np.ones(dims, dtype=bool)
    m[inner(dims)] = False
    return m


_WEXT = {}


def ext_weights(P):
    """Lagrange weights of the interior nodes of a line of P points at its two ends, long double, from the product formula
    l_j(x_e) = prod_{m != j} (x_e - x_m) / (x_j - x_m) with every difference as a product of two folded sines."""
    if P not in _WEXT:
        n = P - 1
        j = np.arange(1, n)

        def diff(a, b):                                          # x_a - x_b
            return LD(-2) * lw._sin_half(a + b, n) * lw._sin_half(a - b, n)
        w = np.zeros((2, P), dtype=LD)
        for e, a in enumerate((0, n)):
            for jj in j:
                m = j[j != jj]
                w[e, jj] = np.prod(diff(a, m) / diff(jj, m))
        _WEXT[P] = (w[0], w[1])
    return _WEXT[P]


def _local(dims, x, dirichlet, T):
    d = len(dims)
    X = np.asarray(x).reshape(-1, d + 1)
    u = np.zeros(tuple(dims) + (d,), dtype=T)
    u[inner(dims)] = X[:, :d].reshape(idims(dims) + (d,))
    if dirichlet is not None:
        u[boundary_mask(dims)] = np.asarray(dirichlet).reshape(-1, d)
    p = np.zeros(dims, dtype=T)
    p[inner(dims)] = X[:, d].reshape(idims(dims))
    return u, p


def _state(dims, eta, deta, S0, T):
    d = len(dims)
    e = np.ones(dims, dtype=T) if eta is None else np.asarray(eta).reshape(dims).astype(T)
    de = np.zeros(dims, dtype=T) if deta is None else np.asarray(deta).reshape(dims).astype(T)
    S = np.zeros((d,) + tuple(dims) + (d,), dtype=T) if S0 is None else np.asarray(S0).reshape((d,) + tuple(dims) + (d,)).astype(T)
    return e, de, S


def prod_ld(M, x, axis):
    return lw.truth(M, x, axis)


def prod_double(M, x, axis):
    return lw.product_double(M, x, axis)


def prod_evenodd(M, x, axis):
    return lw.product_evenodd(M, x, axis, False)


# ----------------------------------------------------------------------------------------------
# the Stokes operator: one statement for the long-double twin (T = LD, prod_ld) and the double restatements
# ----------------------------------------------------------------------------------------------
def stokes_apply(dims, x, eta=None, deta=None, S0=None, dirichlet=None, force=None, rheology=None, prod=prod_ld, T=LD,
                 mats=None, fault=None):
    """Returns (y, state): y the full global result, state = (eta, eta', strain (d, N * d)) for `function` (rheology given:
    StokesFunction; else the Jacobian apply with the given state).  fault: (name, ...) plants one of the defects of
    test_callbacks_host.py."""
    d = len(dims)
    fault = fault or (None,)
    D = mats if mats is not None else [lw.dense_D(P) for P in dims]
    u, p = _local(dims, x, dirichlet, T)
    if fault[0] == "dirichlet":                                  # the boundary node fault[1] holds the value of the boundary node fault[2]
        u[fault[1]] = u[fault[2]]
    for k in range(d):
        w0, w1 = (w.astype(T) for w in ext_weights(dims[k]))
        pin = p[inner(dims)]
        e0 = np.tensordot(w0[1:-1], pin, axes=([0], [k]))
        e1 = np.tensordot(w1[1:-1], pin, axes=([0], [k]))
        if fault[0] == "face" and fault[1] == k:
            e0[fault[2]] *= (1 + fault[3])
        ix = list(inner(dims))
        ix[k] = 0
        p[tuple(ix)] = e0
        ix[k] = -1
        p[tuple(ix)] = e1
    G = [prod(D[j], u, j) for j in range(d)]
    s = [[0.5 * (G[j][..., k] + G[k][..., j]) for k in range(d)] for j in range(d)]
    div = sum(G[k][..., k] for k in range(d))
    state = None
    if rheology is not None:
        kind, B, n, eps, g0 = rheology
        gam = sum(0.5 * (s[j][k] * s[j][k]) for j in range(d) for k in range(d))
        if kind == 1:
            pw = (T(1) - T(n)) / (T(2) * T(n))
            q = T(eps) + gam / T(g0)
            qp = np.power(q, pw)
            e = T(B) * qp
            de = T(B) * pw / T(g0) * (np.power(q, pw - T(1)) if T is LD else qp / q)
        else:
            e, de = np.ones(dims, dtype=T), np.zeros(dims, dtype=T)
        tau = [[e * s[j][k] for k in range(d)] for j in range(d)]
        state = (e.ravel(), de.ravel(), np.stack([np.stack(s[j], axis=-1).reshape(-1) for j in range(d)]))
    else:
        e, de, S = _state(dims, eta, deta, S0, T)
        z = sum(s[j][k] * S[j][..., k] for j in range(d) for k in range(d))
        tau = [[e * s[j][k] + de * S[j][..., k] * z for k in range(d)] for j in range(d)]
        if fault[0] == "drop":                                   # the eta' S0 z term of tau[j][k] dropped at one node
            _, j, k, node = fault
            tau[j][k][node] = (e * s[j][k])[node]
        if fault[0] == "transpose":                              # tau[j][k] and tau[k][j] exchanged at one node
            _, j, k, node = fault
            a, b = tau[j][k][node], tau[k][j][node]
            tau[j][k][node], tau[k][j][node] = b, a
    yv = -sum(prod(D[j], np.stack(tau[j], axis=-1), j) for j in range(d))
    for k in range(d):
        yv[..., k] += prod(D[k], p, k)
    I = int(np.prod(idims(dims)))
    Y = np.empty((I, d + 1), dtype=T)
    Y[:, :d] = yv[inner(dims)].reshape(I, d)
    Y[:, d] = div[inner(dims)].reshape(I)
    if fault[0] == "prow":
        Y[fault[1], d] *= (1 + fault[2])
    if force is not None:
        Y -= np.asarray(force).reshape(I, d + 1).astype(T)
    return Y.reshape(-1), state


def stokes_weight(dims, x, eta=None, deta=None, S0=None, dirichlet=None, force=None):
    """(W, ws, wgamma): the weight of stokes_apply's result (global size, double), the strain's own weight (d, N * d) and
    sum_jk |S0_jk| ws_jk (N)."""
    d = len(dims)
    D = [lw.dense_D(P) for P in dims]
    u, p = _local(dims, x, dirichlet, np.float64)
    au, ap = np.abs(u), np.abs(p)
    for k in range(d):
        w0, w1 = (np.abs(w.astype(np.float64)) for w in ext_weights(dims[k]))
        pin = ap[inner(dims)]
        ix = list(inner(dims))
        ix[k] = 0
        ap[tuple(ix)] = np.tensordot(w0[1:-1], pin, axes=([0], [k]))
        ix[k] = -1
        ap[tuple(ix)] = np.tensordot(w1[1:-1], pin, axes=([0], [k]))
    WG = [lw.bound(D[j], au, j) for j in range(d)]
    ws = [[0.5 * (WG[j][..., k] + WG[k][..., j]) for k in range(d)] for j in range(d)]
    e, de, S = _state(dims, eta, deta, S0, np.float64)
    wz = sum(np.abs(S[j][..., k]) * ws[j][k] for j in range(d) for k in range(d))
    wtau = [np.stack([np.abs(e) * ws[j][k] + np.abs(de) * np.abs(S[j][..., k]) * wz for k in range(d)], axis=-1) for j in range(d)]
    wv = sum(lw.bound(D[j], wtau[j], j) for j in range(d))
    for k in range(d):
        wv[..., k] += lw.bound(D[k], ap, k)
    wp = sum(WG[k][..., k] for k in range(d))
    I = int(np.prod(idims(dims)))
    W = np.empty((I, d + 1))
    W[:, :d] = wv[inner(dims)].reshape(I, d)
    W[:, d] = wp[inner(dims)].reshape(I)
    if force is not None:
        W += np.abs(np.asarray(force, dtype=np.float64).reshape(I, d + 1))
    return W.reshape(-1), np.stack([np.stack(ws[j], axis=-1).reshape(-1) for j in range(d)]), wz.reshape(-1)


def stokes_function_weight(dims, x, dirichlet, force, state):
    """The weight of `function`: that of the operator linearised about the state it leaves."""
    e, de, s = (np.asarray(a, dtype=np.float64) for a in state)
    return stokes_weight(dims, x, e, de, s, dirichlet, force)


# ----------------------------------------------------------------------------------------------
# the scalar operator
# ----------------------------------------------------------------------------------------------
def _local_scalar(dims, U, dirichlet, T):
    u = np.zeros(dims, dtype=T)
    u[inner(dims)] = np.asarray(U).reshape(idims(dims))
    if dirichlet is not None:
        u[boundary_mask(dims)] = np.asarray(dirichlet).reshape(-1)
    return u


def elliptic_apply(dims, U, eta=None, deta=None, g0=None, dirichlet=None, b=None, gamma=None, exponent=2.0, prod=prod_ld, T=LD):
    """(V, state): MatMult_Elliptic with the given state, or (gamma given) FormFunction with state = (eta, eta', gradu (d, N))."""
    d = len(dims)
    D = [lw.dense_D(P) for P in dims]
    u = _local_scalar(dims, U, dirichlet, T)
    g = [prod(D[k], u, k) for k in range(d)]
    state = None
    if gamma is not None:
        if exponent == 2.0:
            e, de = T(1) + T(gamma) * u * u, T(2) * T(gamma) * u
        else:
            e, de = T(1) + T(gamma) * np.power(u, T(exponent)), T(exponent) * T(gamma) * np.power(u, T(exponent) - T(1))
        f = [e * g[k] for k in range(d)]
        state = (e.ravel(), de.ravel(), np.stack([g[k].ravel() for k in range(d)]))
    else:
        e = np.ones(dims, dtype=T) if eta is None else np.asarray(eta).reshape(dims).astype(T)
        de = np.zeros(dims, dtype=T) if deta is None else np.asarray(deta).reshape(dims).astype(T)
        G0 = np.zeros((d,) + tuple(dims), dtype=T) if g0 is None else np.asarray(g0).reshape((d,) + tuple(dims)).astype(T)
        f = [e * g[k] + de * u * G0[k] for k in range(d)]
    V = -sum(prod(D[k], f[k], k) for k in range(d))
    V = V[inner(dims)].reshape(-1)
    if b is not None:
        V = V - np.asarray(b).reshape(-1).astype(T)
    return V, state


def elliptic_weight(dims, U, eta=None, deta=None, g0=None, dirichlet=None, b=None):
    """(W, wgrad (d, N))"""
    d = len(dims)
    D = [lw.dense_D(P) for P in dims]
    au = np.abs(_local_scalar(dims, U, dirichlet, np.float64))
    wg = [lw.bound(D[k], au, k) for k in range(d)]
    e = np.ones(dims) if eta is None else np.abs(np.asarray(eta, dtype=np.float64).reshape(dims))
    de = np.zeros(dims) if deta is None else np.abs(np.asarray(deta, dtype=np.float64).reshape(dims))
    G0 = np.zeros((d,) + tuple(dims)) if g0 is None else np.abs(np.asarray(g0, dtype=np.float64).reshape((d,) + tuple(dims)))
    W = sum(lw.bound(D[k], e * wg[k] + de * au * G0[k], k) for k in range(d))[inner(dims)].reshape(-1)
    if b is not None:
        W = W + np.abs(np.asarray(b, dtype=np.float64).reshape(-1))
    return W, np.stack([w.ravel() for w in wg])


# ----------------------------------------------------------------------------------------------
# the bar
# ----------------------------------------------------------------------------------------------
def rows(dims, y):
    """(velocity rows (I, d), pressure rows (I,)) of a full global vector."""
    d = len(dims)
    Y = np.asarray(y).reshape(-1, d + 1)
    return Y[:, :d], Y[:, d]


def check_stokes(dims, y, t, W, what, fn=False, power=False):
    """Asserts the bar on the velocity rows and on the pressure rows of a full global vector separately; returns
    [("v", ratio, index, cap), ("p", ...)]."""
    yv, yp = rows(dims, y)
    tv, tp = rows(dims, t)
    wv, wp = rows(dims, W)
    cv, cp = cap_v(dims, fn, power), cap_p(dims)
    rv, iv = lw.check(yv, tv, wv, cv, what + " velocity rows")
    rp, ip = lw.check(yp, tp, wp, cp, what + " pressure rows")
    return [("v", rv, iv, cv), ("p", rp, ip, cp)]


def worst_stokes(dims, y, t, W):
    """The two worst ratios without asserting."""
    yv, yp = rows(dims, y)
    tv, tp = rows(dims, t)
    wv, wp = rows(dims, W)
    return lw.worst(yv, tv, wv)[0], lw.worst(yp, tp, wp)[0]


def exact_zero(dims, t, W):
    """The truth of an input in the operator's null space ([0; constant]) is exactly 0; the long-double evaluation leaves its
    own rounding, at most (2 K + 40) 2^-64 W.  Asserts that and returns the exact truth."""
    assert np.all(np.abs(t) <= (2 * max(dims) + 40) * 2.0 ** -64 * W)
    return np.zeros_like(t)


def check_relative(y, t, bound_units, what):
    """|y - t| <= bound_units 2^-53 |t| per element (eta, eta'); returns the worst |y - t| / (2^-53 |t| bound)."""
    err = np.abs(np.asarray(y).astype(LD) - np.asarray(t).astype(LD)).astype(np.float64)
    lim = U53 * np.abs(np.asarray(t, dtype=np.float64)) * bound_units
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    k = int(np.argmax(r))
    assert r.reshape(-1)[k] <= 1.0, "%s: error %.3g of its bound at %d (y = %r, truth = %r)" % (
        what, r.reshape(-1)[k], k, float(np.asarray(y).reshape(-1)[k]), float(np.asarray(t).reshape(-1)[k]))
    return float(r.reshape(-1)[k]), k


# ----------------------------------------------------------------------------------------------
# states and inputs.  Every input is an interior (global) vector.
# ----------------------------------------------------------------------------------------------
STATES = ("default", "eta", "full")


def stokes_state(dims, name, seed=7):
    """(eta, eta', S0) of the three states of the tests; None = the handle's default.  S0 is symmetric (the ABI's contract)."""
    d, N = len(dims), int(np.prod(dims))
    rng = np.random.default_rng(seed)
    if name == "default":
        return None, None, None
    eta = np.exp(rng.uniform(np.log(0.5), np.log(10.0), N))
    if name == "eta":
        return eta, None, None
    deta = rng.standard_normal(N)
    S = rng.standard_normal((d, N, d))
    S = 0.5 * (S + S.transpose(2, 1, 0))
    return eta, deta, S.reshape(d, N * d)


def noise(dims, seed):
    return np.random.default_rng(seed).standard_normal(sizes(dims)[2])


def block_v(dims, seed):
    x = noise(dims, seed).reshape(-1, len(dims) + 1)
    x[:, -1] = 0.0
    return x.reshape(-1)


def block_p(dims, seed):
    x = noise(dims, seed).reshape(-1, len(dims) + 1)
    x[:, :-1] = 0.0
    return x.reshape(-1)


def node_scaled(dims, seed):
    """noise x 10^k per node, k uniform in -30 .. 30 (the linear callbacks only)."""
    x = noise(dims, seed).reshape(-1, len(dims) + 1)
    k = np.random.default_rng(seed + 1).integers(-30, 31, size=(x.shape[0], 1))
    return (x * 10.0 ** k).reshape(-1)


def constant_pressure(dims, seed):
    """[0; c]: the truth is exactly 0 while W is not."""
    x = np.zeros((sizes(dims)[1], len(dims) + 1))
    x[:, -1] = np.random.default_rng(seed).standard_normal()
    return x.reshape(-1)


def impulse_positions(dims, tile=16):
    """Interior nodes (full-grid indices) for the impulses: the first and last interior node of every direction (through the
    grid's first and last interior node); nodes on the contiguous lines (last index fastest, numbered over the full grid) on
    either side of the line numbers 15/16, 31/32 and 63/64 -- where such a line lies on the boundary (the whole first plane
    does when the middle extent exceeds 64) the first interior line with the same number modulo 64, i.e. the same place in its
    tile of 16, 32 or 64 lines; one on the last interior line, which feeds the stress on the last, partial tile of lines."""
    d = len(dims)
    first, last = tuple(1 for _ in dims), tuple(p - 2 for p in dims)
    pos = {first, last}
    for k in range(d):
        a, b = list(first), list(last)
        a[k], b[k] = dims[k] - 2, 1
        pos.update((tuple(a), tuple(b)))
    ldims = dims[:-1]
    nl = int(np.prod(ldims))
    mid = max(1, dims[-1] // 2)
    for L in (15, 16, 31, 32, 63, 64):
        while L < nl:
            ix = np.unravel_index(L, ldims)
            if all(0 < i < p - 1 for i, p in zip(ix, ldims)):
                pos.add(tuple(int(i) for i in ix) + (mid,))
                break
            L += 64
    pos.add(last[:-1] + (mid,))
    return sorted(pos)


def impulse(dims, node, comp):
    """The interior vector with a single 1.0: component comp (d = the pressure) of the interior node with full-grid index node."""
    x = np.zeros(idims(dims) + (len(dims) + 1,))
    x[tuple(i - 1 for i in node) + (comp,)] = 1.0
    return x.reshape(-1)
