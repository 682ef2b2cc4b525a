"""The fast-diagonalisation solve restated in NumPy (helper module of test_fdm_host.py / test_gpu_fdm.py).

    z = (S_0 x .. x S_{d-1}) diag(1 / (sigma + l_i + l_j + ..)) (S_0^-1 x .. x S_{d-1}^-1) (r / eta)

on nf stacked interior fields, an array of shape (nf, M_0, .., M_{d-1}).  The line matrices are the library's own, in double, as its
host accessors give them (`lines`): the device's matrices up to the one rounding per entry that the bar of linewise.py counts.
`truth` is the chain in long double.  Two double restatements calibrate the bar of the whole solve: `chain(.., "plain")` (dense
products, divisions) and `chain(.., "evenodd")` (the device's algebra: parity-split products, multiplications by reciprocals).
Each STEP of the solve is a line product with a pointwise factor and gets the derived componentwise bar of linewise.py
(`step_truth_bound`, `step_cap`):

    plain transform                      K + 8             (linewise.py; K = points of the line)
    division by eta on the load          + 2               the reciprocal and the multiply; B on |x / eta|
    modal scaling on the store           + d + 2           d - 1 additions, sigma, the reciprocal and the multiply; B times |w|
    the scaling pass alone               d + 2             against |x| |w|
    the one-launch z solve               2 (K + 8) + d + 2 against |S|_s (|w| |S^-1|_s |x|) along the line"""
import numpy as np

import linewise as lw

LD = np.longdouble
U53 = lw.U53


def lines(sp, kind, dims, bc=None, scale=None):
    """Per direction (S, Sinv, lam) in double.  kind "fd": the three-point line of the preconditioner; "spectral": the collocation
    line; with bc (a HelmholtzSolver's, one entry per direction) the line with its ends eliminated, on a box of `scale`."""
    out = []
    for k, P in enumerate(dims):
        if bc is not None:
            out.append(tuple(sp.helmholtz_line_box(P, bc[k], 1.0 if scale is None else scale[k])[:3]))
        elif kind == "fd":
            out.append(sp.fdpc_line(P))
        else:
            out.append(sp.helmholtz_line(P))
    return out


def parity_ok(bc_k):
    """Whether a direction's modes use the parity layout: both ends carry the same condition."""
    if bc_k is None or isinstance(bc_k, str):
        return True
    b = tuple(bc_k)
    if len(b) == 2 and all(isinstance(e, (int, float)) for e in b):
        return True
    return b[0] == b[1]


def interior(full, dims):
    """The interior nodes of a full-grid array (prod(dims) values), shape dims - 2: plain slicing."""
    a = np.asarray(full).reshape(dims)
    return np.ascontiguousarray(a[tuple(slice(1, p - 1) for p in dims)])


def _shape(k, d, n):
    return [1] + [n if j == k else 1 for j in range(d)]


def weight_sum(L, sigma, dtype):
    """sigma + sum_k lam_k on the modal grid, shape (1, M_0, .., M_{d-1}); in double with the device's association: sigma rides on
    dimension 0's eigenvalues, then the directions in ascending order."""
    d = len(L)
    s = (np.asarray(L[0][2], dtype=dtype) + dtype(sigma)).reshape(_shape(0, d, L[0][2].size))
    for k in range(1, d):
        s = s + np.asarray(L[k][2], dtype=dtype).reshape(_shape(k, d, L[k][2].size))
    return s


def weights(L, sigma, dtype=np.float64, recip=True):
    """1 / weight_sum, 0 where the sum is exactly 0 (the dropped mode of a singular solve).  recip = False returns the sum itself
    with 1 in place of an exact 0 and the mask of those places: for the restatement that divides."""
    s = weight_sum(L, sigma, dtype)
    zero = s == 0
    safe = np.where(zero, dtype(1), s)
    if recip:
        return np.where(zero, dtype(0), dtype(1) / safe)
    return safe, zero


def _apply(M, x, axis):
    return np.moveaxis(np.tensordot(M, x, axes=([1], [axis])), 0, axis)


def truth(r, L, sigma=0.0, eta=None):
    """The whole solve in long double.  eta: interior viscosity, shape (M_0, .., M_{d-1}), or None."""
    t = np.asarray(r).astype(LD)
    if eta is not None:
        t = t * (LD(1) / np.asarray(eta).astype(LD))[None]
    for k, (S, Si, lam) in enumerate(L):
        t = _apply(Si.astype(LD), t, k + 1)
    t = t * weights(L, sigma, LD)
    for k, (S, Si, lam) in enumerate(L):
        t = _apply(S.astype(LD), t, k + 1)
    return t


def forward_eo(Si, x, axis):
    """S^-1 along `axis` by the parity split of the raw forward transform: even modes (positions p < H) from e = x_j + x_m-j, the
    q-th odd mode (position m - q) from o = x_j - x_m-j; the middle point of an odd line is its own mirror."""
    M = Si.shape[0]
    m, H = M - 1, (M + 1) // 2
    xm = np.moveaxis(x, axis, 0)
    xr = xm[::-1]
    e, o = xm[:H] + xr[:H], xm[:H] - xr[:H]
    if M & 1:
        e[H - 1] = xm[H - 1]
    c = np.empty_like(xm)
    c[:H] = np.tensordot(Si[:H, :H], e, axes=([1], [0]))
    nq = M - H
    if nq:
        c[m - np.arange(nq)] = np.tensordot(Si[m - np.arange(nq), :nq], o[:nq], axes=([1], [0]))
    return np.moveaxis(c, 0, axis)


def backward_eo(S, c, axis):
    """S along `axis` from coefficients in the parity layout: x_i = a_i + b_i, x_m-i = a_i - b_i with a from the even modes and b
    from the odd ones."""
    M = S.shape[0]
    m, H = M - 1, (M + 1) // 2
    nq = M - H
    cm = np.moveaxis(c, axis, 0)
    a = np.tensordot(S[:H, :H], cm[:H], axes=([1], [0]))
    b = np.tensordot(S[:H, m - np.arange(nq)], cm[m - np.arange(nq)], axes=([1], [0])) if nq else np.zeros_like(a)
    x = np.empty_like(cm)
    x[:H] = a + b
    i = np.arange(nq)
    x[m - i] = a[:nq] - b[:nq]
    return np.moveaxis(x, 0, axis)


def chain(r, L, sigma=0.0, eta=None, how="plain", parity=None, hook=None, w=None, einv=None):
    """The solve in double; returns (z, stages) with stages a list of (name, k, input, output) per step, the steps of the device:
    "over_eta" (k = None), "forward", "scale", "backward".  how = "plain": dense products, r / eta and t / sum; "evenodd": the
    parity-split products (directions with parity[k] false: dense) and multiplications by fl(1 / eta) and fl(1 / sum).
    hook(name, k, out) -> out lets a test plant a fault after a step; w / einv replace the weights (the reciprocal for "evenodd",
    the divisor for "plain") and 1 / eta."""
    d = len(L)
    parity = [True] * d if parity is None else parity
    eo = how == "evenodd"
    hook = hook or (lambda name, k, a: a)
    stages = []
    t = np.array(r, dtype=np.float64)
    if eta is not None or einv is not None:
        x = t
        if einv is not None:
            t = x * einv[None]
        elif eo:
            t = x * (1.0 / np.asarray(eta, dtype=np.float64))[None]
        else:
            t = x / np.asarray(eta, dtype=np.float64)[None]
        t = hook("over_eta", None, t)
        stages.append(("over_eta", None, x, t))
    for k, (S, Si, lam) in enumerate(L):
        x = t
        t = forward_eo(Si, x, k + 1) if eo and parity[k] else _apply(Si, x, k + 1)
        t = hook("forward", k, t)
        stages.append(("forward", k, x, t))
    x = t
    if eo:
        t = x * (weights(L, sigma) if w is None else w)
    else:
        if w is None:
            s, zero = weights(L, sigma, recip=False)
            t = np.where(zero, 0.0, x / s)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(w == 0, 0.0, x / w)
    t = hook("scale", d - 1, t)
    stages.append(("scale", d - 1, x, t))
    for k in range(d - 1, -1, -1):
        S = L[k][0]
        x = t
        t = backward_eo(S, x, k + 1) if eo and parity[k] else _apply(S, x, k + 1)
        t = hook("backward", k, t)
        stages.append(("backward", k, x, t))
    return t, stages


# ----------------------------------------------------------------------------------------------
# the steps: truth, componentwise weight B and cap
# ----------------------------------------------------------------------------------------------
def step_cap(mode, K, d):
    return {"forward": K + 8, "backward": K + 8, "forward_over_eta": K + 8 + 2, "forward_scaled": K + 8 + d + 2, "scale": d + 2,
            "zsolve": 2 * (K + 8) + d + 2}[mode]


def step_truth_bound(mode, k, x, L, sigma=0.0, eta=None, lines=None):
    """(truth in long double, B in double) of one step along direction k on x (nf, M_0, .., M_{d-1}).
    lines: flat indices (C order of the shape without direction k, stacked fields included) of the lines to compute; truth and B
    are then (points, len(lines)) arrays, as linewise.take_lines lays the lines out -- the same arithmetic on those lines alone."""
    S, Si, lam = L[k]
    ax = k + 1
    x = np.asarray(x, dtype=np.float64)
    wl = wd = einv = None
    if mode == "forward_over_eta":
        einv = np.broadcast_to((LD(1) / np.asarray(eta).astype(LD))[None], x.shape)
    if mode in ("scale", "forward_scaled", "zsolve"):
        wl = np.broadcast_to(weights(L, sigma, LD), x.shape)
        wd = np.broadcast_to(np.abs(weights(L, sigma)), x.shape)
    if lines is not None:                              # every operand as (points, lines); the products then run along axis 0
        x = lw.take_lines(x, ax, lines)
        einv, wl, wd = (None if a is None else lw.take_lines(a, ax, lines) for a in (einv, wl, wd))
        ax = 0
    if mode == "forward":
        return lw.truth(Si.astype(LD), x, ax), lw.bound(Si, x, ax)
    if mode == "backward":
        return lw.truth(S.astype(LD), x, ax), lw.bound(S, x, ax)
    if mode == "forward_over_eta":
        xe = x.astype(LD) * einv
        return lw.truth(Si.astype(LD), xe, ax), lw.bound(Si, np.abs(xe).astype(np.float64), ax)
    if mode == "scale":
        return x.astype(LD) * wl, np.abs(x) * wd
    if mode == "forward_scaled":
        return lw.truth(Si.astype(LD), x, ax) * wl, lw.bound(Si, x, ax) * wd
    if mode == "zsolve":
        c = lw.truth(Si.astype(LD), x, ax) * wl
        return lw.truth(S.astype(LD), c, ax), lw.bound(S, lw.bound(Si, x, ax) * wd, ax)
    raise ValueError(mode)


def sample_lines(shape, k, seed, tile=32, extra=192):
    """Sorted flat line indices (linewise.take_lines order for direction k of a (nf, M_0, .., M_{d-1}) array) on which a large case
    checks a step: the first and the last line, both sides of every boundary between stacked fields with the whole tile of `tile`
    lines that straddles it, the last (partial) tile, both sides of the first tile boundaries, and `extra` seeded ones."""
    nl = int(np.prod(shape)) // shape[k + 1]
    per = nl // shape[0]
    sel = {0, nl - 1}
    for f in range(1, shape[0]):
        t0 = (f * per // tile) * tile
        sel.update(range(t0, min(t0 + tile, nl)))
        sel.update((f * per - 1, f * per))
    sel.update(range(((nl - 1) // tile) * tile, nl))
    for t in (tile, 2 * tile, 4 * tile):
        if t < nl:
            sel.update((t - 1, t))
    sel.update(int(v) for v in np.random.default_rng(seed).integers(0, nl, size=extra))
    return np.array(sorted(sel), dtype=np.int64)


def stage_checks(stages, L, sigma, eta):
    """The restatement's own steps as (mode, k, input, output) in the vocabulary of the device's steps: its separate division by
    eta is folded into the first forward transform's input."""
    out, pend = [], None
    for name, k, x, y in stages:
        if name == "over_eta":
            pend = x
        elif name == "forward" and pend is not None:
            out.append(("forward_over_eta", k, pend, y))
            pend = None
        else:
            out.append((name, k, x, y))
    return out


def errors(y, t):
    """Per stacked field (max|y - t| / max|t|, ||y - t||_2 / ||t||_2), computed in long double; a NaN anywhere gives inf."""
    y = np.asarray(y).astype(LD).reshape(t.shape[0], -1)
    tt = t.reshape(t.shape[0], -1)
    e = np.abs(y - tt)
    out = []
    for f in range(tt.shape[0]):
        if not np.all(np.isfinite(e[f].astype(np.float64))):
            out.append((np.inf, np.inf))
            continue
        out.append((float(e[f].max() / np.abs(tt[f]).max()), float(np.sqrt((e[f] * e[f]).sum()) / np.sqrt((tt[f] * tt[f]).sum()))))
    return out


def node_scaled(shape, seed):
    """Noise scaled per node by 10^k, k uniform in -30 .. 30."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 31, size=shape)
