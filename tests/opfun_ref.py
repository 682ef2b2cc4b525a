"""numpy model and bars of ChebOpFun (helper module of test_opfun_host.py / test_gpu_opfun.py).

The model.  A direction's S, S^-1 and lam are the float64 matrices the device holds (sp.helmholtz_line for a handle without bc,
sp.helmholtz_line_box otherwise).  The eigenvalue sum of a mode is formed as the kernel forms it: sigma is added to direction 0's
eigenvalues first, then s = ((l_0[i_0] + l_1[i_1]) + l_2[i_2]) + ... left to right in float64 (`eigen_sum`).  Weights are the host
twin's (sp.opfun_weight: long double, rounded once).  `model` evaluates y_o = S [sum_t c_t w_t .* (S^-1 x_{i_t})] with the tensor
products in np.longdouble (`prec` = np.float64: the same in float64, the stand-in for the device on the CPU).

The bars (one definition for the float64 model on the CPU and for the library on the GPU), U = 2^-53:
  weight   |w - twin| <= (K_kind + kappa) U |twin|, kappa = tau s for exp and 0 otherwise; where |twin| < 2^-1022 the bar is
           2^-1022 absolute.  K_kind counts the roundings of csrc/opfun_fn.h and the twin's own (see K below); HIP documents
           exp, expm1 and pow as 1 ulp, i.e. 2 U relative.
  field    |y - model| <= U [(sum_k 2 (M_k + 8) + T) B + B'] element by element, M_k = n_k - 2, T the output's number of terms,
           B = |S| (sum_t |c_t w_t| .* |S^-1| |x_{i_t}|) with every matrix replaced by its absolute value, B' the same with each
           |w_t| multiplied by (K_kind + kappa): 2 d line products of M_k terms each (linewise.py's (M + 8) U per product), T
           products and sums in the mixing kernel, and the weights' own error.
  norm     |y - model|_2 <= 1e-10 |model|_2: the project's normwise bar for every sweep route."""
import numpy as np

import __graft_entry__ as ge

sp = ge.load()

LD = np.longdouble
U = 2.0 ** -53
TINY = 2.0 ** -1022
NORM_BAR = 1e-10
KINDS = ("one", "inv", "res", "exp", "phi1", "phi2", "phi3", "pow")
PHI_SERIES = 2.0            # csrc/opfun_fn.h: |z| <= 2 the nested series of phi_2, phi_3, beyond it the recurrence

# K_kind, in U: the roundings of csrc/opfun_fn.h plus 1 wherever the function rounds at all, because the twin the device is
# compared with is itself a rounded double (up to 1 U from the exact value, so two faithful results can differ by 2 U).
# z = -tau s is rounded once: 1 U in z, which a function g passes on times |z g'(z) / g(z)|.  That factor is < 1 for every phi_k at
# z <= 0 and equals tau s for exp: the kappa of the bar.
K = {
    "one": 0,     # the constant 1
    "inv": 2,     # one division: 1; twin: 1
    "res": 3,     # fma(tau, s, p): 1 (one rounding of the exact p + tau s, also where the two cancel); the division: 1; twin: 1
    "exp": 3,     # exp: 2 (1 ulp); twin: 1
    "phi1": 5,    # z: 1; expm1: 2 (1 ulp); the division: 1; twin: 1
    # series (|z| <= 2): level j of 1 + z/(k+j) (1 + ...) has 3 roundings (the constant 1/(k+j), its product with z, the fma) and
    # passes the error e_{j+1} of the level below on times |a_j r_{j+1}| / r_j <= 0.76 (z = -2, k = 2, j = 1: 0.433 / 0.567;
    # 0.54, 0.43, 0.33, .. for j = 2, 3, 4 and smaller for |z| < 2 or k = 3): e_0 <= 1 + 0.76 (2 + e_1), e_1 <= 1 + 0.54 (2 + e_2),
    # e_2 <= 1 + 0.43 (2 + e_3), e_3 <= 1 + 0.33 (2 + 2) -> e_0 <= 5.3; the factor 1/2 is exact; z: 1; twin: 1 -> 7.3.
    # recurrence (|z| > 2): phi_1 with its 3 U (z apart) times phi_1 / (1 - phi_1) <= 0.76 at z = -2, falling beyond: 2.3; the
    # subtraction 1, the division 1 -> 4.3; z: 1; twin: 1 -> 6.3.  The larger branch, rounded up:
    "phi2": 8,
    # series: e_0 <= 4.4 (k = 3: the ratios are 0.60, 0.47, 0.38, ..); the constant 1/6 and its product: 1.5; z: 1; twin: 1 -> 7.9.
    # recurrence: phi_2 with its 4.3 U times phi_2 / (1/2 - phi_2) <= 1.31 at z = -2, falling beyond: 5.7; the subtraction (exact
    # for phi_2 in [1/4, 1]) 1; the division 1 -> 7.7; z: 1; twin: 1 -> 9.7.  Rounded up:
    "phi3": 10,
    "pow": 3,     # pow: 2 (1 ulp); twin: 1
}


def kappa(kind, tau, s):
    return np.abs(tau * np.asarray(s, dtype=np.float64)) if kind == "exp" else np.zeros(np.shape(s))


def weight_bar(kind, tau, s, twin):
    """The weight bar for device values of f(s) against the twin's."""
    twin = np.abs(np.asarray(twin, dtype=np.float64))
    return np.where(twin < TINY, TINY, (K[kind] + kappa(kind, tau, s)) * U * twin)


def lines(dims, bc=None, scale=None):
    """[(S, Sinv, lam)] per direction in float64: the matrices of the handle ChebOpFun(dims, bc=bc, scale=scale)."""
    out = []
    for k, P in enumerate(dims):
        if bc is None:
            out.append(sp.helmholtz_line(P))
        else:
            out.append(sp.helmholtz_line_box(P, bc[k], 1.0 if scale is None else scale[k])[:3])
    return out


def eigen_sum(ln, sigma=0.0):
    """s of every mode, shape (M_0, .., M_{d-1}), in the kernel's association: ((sigma + l_0) + l_1) + ..., float64."""
    s = ln[0][2] + np.float64(sigma)
    for k in range(1, len(ln)):
        s = s[..., None] + ln[k][2]
    return s


def along(A, x, k):
    """A applied along axis k + 1 of the stacked fields x (nf, M_0, .., M_{d-1}), in the precision of the operands."""
    return np.moveaxis(np.tensordot(A, x, axes=(1, k + 1)), 0, k + 1)


def to_modes(ln, x, prec=LD, absolute=False):
    y = np.abs(x).astype(prec) if absolute else x.astype(prec)
    for k, (S, Si, lam) in enumerate(ln):
        y = along((np.abs(Si) if absolute else Si).astype(prec), y, k)
    return y


def to_nodes(ln, c, prec=LD, absolute=False):
    y = c
    for k in range(len(ln) - 1, -1, -1):
        S = ln[k][0]
        y = along((np.abs(S) if absolute else S).astype(prec), y, k)
    return y


def term_weights(terms, s):
    """Per term the twin's weights over the modes (float64)."""
    return [sp.opfun_weight(kind, tau, par, s) for (o, i, kind, c, tau, par) in terms]


def model(dims, terms, x, nout, sigma=0.0, bc=None, scale=None, prec=LD, ln=None):
    """(y, bar): y (nout, G) the model in `prec`; bar (nout, G) the field bar of the same call (float64).  x: (nin, G)."""
    ln = lines(dims, bc, scale) if ln is None else ln
    M = tuple(n - 2 for n in dims)
    s = eigen_sum(ln, sigma)
    xs = np.asarray(x, dtype=np.float64).reshape((-1,) + M)
    c = to_modes(ln, xs, prec)
    ca = to_modes(ln, xs, LD, absolute=True)
    ws = term_weights(terms, s)
    acc = np.zeros((nout,) + M, dtype=prec)
    B = np.zeros((nout,) + M, dtype=LD)
    Bp = np.zeros((nout,) + M, dtype=LD)
    T = np.zeros(nout)
    for (o, i, kind, coef, tau, par), w in zip(terms, ws):
        acc[o] = acc[o] + (prec(coef) * w.astype(prec)) * c[i]
        aw = np.abs(coef * w).astype(LD)
        B[o] += aw * ca[i]
        Bp[o] += aw * (K[kind] + kappa(kind, tau, s)) * ca[i]
        T[o] += 1
    y = to_nodes(ln, acc, prec)
    B = to_nodes(ln, B, LD, absolute=True)
    Bp = to_nodes(ln, Bp, LD, absolute=True)
    lines_k = sum(2 * (m + 8) for m in M)
    bar = U * ((lines_k + T).reshape((nout,) + (1,) * len(M)) * B + Bp)
    return y.reshape(nout, -1), np.asarray(bar, dtype=np.float64).reshape(nout, -1)


def modal_apply(ln, W, x, prec=LD):
    """S (W .* S^-1 x) for one weight array W over the modes and stacked fields x (nf, G)."""
    M = W.shape
    c = to_modes(ln, np.asarray(x, dtype=np.float64).reshape((-1,) + M), prec)
    return to_nodes(ln, W.astype(prec) * c, prec).reshape(c.shape[0], -1)


def modal_bound(ln, Wabs, x):
    """|S| (Wabs .* |S^-1| |x|): what a relative perturbation of the weights can move, element by element."""
    M = Wabs.shape
    ca = to_modes(ln, np.asarray(x, dtype=np.float64).reshape((-1,) + M), LD, absolute=True)
    return np.asarray(to_nodes(ln, Wabs.astype(LD) * ca, LD, absolute=True), dtype=np.float64).reshape(ca.shape[0], -1)


def check(y, ref, bar, what=""):
    """Asserts the field bar element by element and the normwise bar; returns (worst ratio to the field bar, normwise error)."""
    y = np.asarray(y, dtype=np.float64).reshape(np.shape(ref))
    err = np.abs(y.astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(err == 0, 0.0, np.asarray(err / bar, dtype=np.float64))))
    nref = float(np.sqrt(np.sum(np.asarray(ref, dtype=LD) ** 2)))
    nerr = float(np.sqrt(np.sum(err ** 2))) / nref if nref > 0 else float(np.max(err))
    assert np.all(np.isfinite(y)), "%s: non-finite values" % what
    assert ratio <= 1.0, "%s: worst element at %.3g of the field bar" % (what, ratio)
    assert nerr <= NORM_BAR, "%s: normwise error %.3g" % (what, nerr)
    return ratio, nerr
