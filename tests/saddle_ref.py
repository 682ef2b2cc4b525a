"""The Stokes block preconditioners of csrc/saddle.hip (stokes_saddle_apply) restated in NumPy (helper module of test_saddle_host.py
and test_gpu_saddle_steps.py), composed from the pieces the suite already holds to a truth: krylov_ref.fgmres (the driver, with the
device's clamp and estimated last column), fdm_ref.truth / fdm_ref.chain (P_1^-1 (r / eta) on the library's own line matrices),
oracle_lib.stokes_truth (the long-double operator) and oracle_lib.fd_matrix (the stencil of MatVVPC).

`apply` is written from the reference's block formulas (stokes.C:1712, 1745, 1770, 1795), the KSP roles those of stokes.C:328-341:

  KSPVelocity, KSPSchurVelocity   fgmres on MatVV, right-preconditioned by MatVVPC; restart 30, zero guess, atol 1e-50, (max_it, rtol)
                                  from cfg; max_it = 0: one MatVVPC solve.
  KSPSchur                        fgmres without a preconditioner on y = P (eta .* (S x)), S x = -PV (svel_solve (VP x)), after the
                                  right-hand side is replaced by P (eta .* b); max(m_schur, 1) iterations; P = I - 1 1^T / n; eta at
                                  the interior nodes, 1 with schur_jacobi off.
  pressure                        made zero-mean once more at the end, for every kind.
  MatVVPC, pc_sweeps = 0          z = P_1^-1 (r / eta) per component: fdm_ref on fdm_ref.lines(sp, "fd", dims).
  MatVVPC, pc_sweeps = s          fgmres on the stencil matrix oracle_lib.fd_matrix(dims, eta) (the same matrix for every component;
                                  ONE solve on the d stacked components, as fdpc_apply runs it), restart s, max_it s, rtol 1e-12,
                                  atol 1e-300, right-preconditioned by the chain above.

Vectors are node-major throughout (the device's component-major layout inside an apply changes the order of its inner products
only, which is what the two restatements differ in anyway).

Three instances per case (`truth_ops`, `oracle_ops`):

  truth          dense long-double blocks whose columns are oracle_lib.stokes_truth on unit vectors (every entry correct to one
                 rounding), fdm_ref.truth, long-double Krylov with dot_ld;
  restatement A  oracle_lib.stokes_mult_vv / stokes_divergence / stokes_mult_vp in mode DIRECT, chain(.., "plain"), dot_pairwise;
  restatement B  the same in mode FAST, chain(.., "evenodd"), dot_strided.

The bar is krylov_ref.solve_ratios, separately on the velocity and on the pressure part: the device's max-norm and 2-norm error
against the truth at most MARGIN = 16 times the larger error of A and B (`part_ratios`).  The large shape has no dense truth: there
the device's difference from A is held to 16 |A - B| (`pair_ratios`).

The iteration counts (velocity iterations summed over the applies of KSPVelocity, Schur iterations: stokes_saddle_iterations) must
equal the truth's.  That is robust where no residual norm that an inner solve compared with its tolerance lies within a factor
GAP = 1.25 of it, on either side (`gap`): asserted for every case of the tables on the host.

The zero-mean bar.  y_p = fl(p - m), m = fl(fl(sum p) / n).  A term of the sum meets T_mean = trips + 8 + 8 roundings -- its thread's
running sum over the grid-stride trips of k_mean_partial (256 x 256 = 65 536 elements per trip), the 8 levels of the block's tree,
the 8 levels of the tree over the 256 partials in k_mean_subtract -- then the division and, per element, the subtraction.  p itself
is a combination of Krylov vectors that were each made zero-mean, so m is of the order of u mean|p| and what it adds to |p| beside
|y| is of second order:  |mean(y_p)| <= (T_mean + 2) u mean|y_p|   (`mean_bar`; 0 for one pressure unknown, where p - p / 1 == 0).

The planted faults (FAULTS) are the slips the suite could not see before: each is one line of `apply`.  Fault d (the mean left in
KSPSchur's right-hand side) cannot show in a result at a fixed number of iterations: S 1 = 0 and every Krylov vector is made
zero-mean, so the constant part of b only sits in the residual, untouched, and is removed from the result at the end.  It shows
where the solve ends on its relative tolerance -- the constant enters |b| and can never be reduced -- which is why the tolerance
cases (C7) carry a pressure mean in their right-hand side (`case_rhs`)."""
import numpy as np

import fdm_ref as fr
import krylov_ref as kr
import oracle_lib as orc

LD = np.longdouble
U53 = kr.U53
MARGIN = kr.MARGIN
GAP = 1.25
MEAN_RB, MEAN_RT = 256, 256

DEFAULT = dict(vel=(4, 1e-5), schur=(3, 1e-5), svel=(0, 1e-5), schur_jacobi=True, pc_sweeps=0)

FAULTS = {"a": "Jacobi scaling by 1 / eta",
          "b": "Jacobi scaling dropped while schur_jacobi is on",
          "c": "the mean not removed inside schur_apply",
          "d": "the mean not removed from the right-hand side",
          "e": "p0 <- p0 + x_p",
          "f": "type 0: y_v <- v1 at the end instead of +=",
          "g": "type 3 taking x_p after it was overwritten",
          "h": "MatVVPC without the division by eta",
          "i": "velocity limit 3 for 4",
          "j": "Schur limit 2 for 3",
          "k": "velocity read component-major where it is node-major",
          "l": "the mean taken over the first 65 536 entries only"}


def config(**kw):
    c = dict(DEFAULT)
    c.update(kw)
    return c


def idims(dims):
    return tuple(p - 2 for p in dims)


def split(x, d):
    X = np.asarray(x).reshape(-1, d + 1)
    return np.ascontiguousarray(X[:, :d]).ravel(), np.ascontiguousarray(X[:, d])


def merge(v, p, d):
    return np.concatenate([np.asarray(v).reshape(-1, d), np.asarray(p)[:, None]], axis=1).ravel()


# ----------------------------------------------------------------------------------------------
# the operators behind one small interface
# ----------------------------------------------------------------------------------------------
class Ops:
    """MatVV / PV / VP on node-major vectors in `dt`, the interior viscosity, and the two pieces of MatVVPC:
    fdm(rc, over_eta) on a component-major array (d, M_0, .., M_{d-1}), and stencil(X) = P X on a (G, d) array."""

    def __init__(self, dims, dt, vv, pv, vp, eta_int, fdm, stencil):
        self.dims, self.d, self.dt = tuple(dims), len(dims), dt
        self.I = int(np.prod(idims(dims)))
        self.vv, self.pv, self.vp, self.fdm, self.stencil = vv, pv, vp, fdm, stencil
        self.eta_int = np.asarray(eta_int, dtype=dt).ravel()


def _state(dims, state):
    N = int(np.prod(dims))
    eta, deta, strain = state if state is not None else (None, None, None)
    return (np.ones(N) if eta is None else np.asarray(eta, dtype=np.float64).ravel()), deta, strain


def _stencil(dims, eta, dt):
    P = orc.fd_matrix(dims, eta)
    if dt is LD:
        Pd = np.asarray(P.todense()).astype(LD)
        return lambda X: Pd @ X
    return lambda X: P @ X


def dense_blocks(dims, state, workers=8):
    """(VV, PV, VP) in long double: the columns of the linearised operator on unit vectors, by the long-double oracle (a column per
    call, the calls spread over `workers` threads: the oracle keeps no state between calls and ctypes releases the interpreter)."""
    from concurrent.futures import ThreadPoolExecutor
    d = len(dims)
    eta, deta, strain = _state(dims, state)
    I = int(np.prod(idims(dims)))
    g = (d + 1) * I
    K = np.empty((g, g))

    def columns(w):
        e = np.zeros(g)
        for j in range(w, g, workers):
            e[j] = 1.0
            K[:, j] = orc.stokes_truth(dims, e, eta, deta, strain)[0]
            e[j] = 0.0
    orc.stokes_truth(dims, np.zeros(g), eta, deta, strain)          # binds the library before the threads start
    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(columns, range(workers)))
    iv = np.arange(g).reshape(I, d + 1)[:, :d].ravel()
    ip = np.arange(g).reshape(I, d + 1)[:, d]
    return K[np.ix_(iv, iv)].astype(LD), K[np.ix_(ip, iv)].astype(LD), K[np.ix_(iv, ip)].astype(LD)


def truth_ops(sp, dims, state=None, blocks=None):
    eta = _state(dims, state)[0]
    VV, PV, VP = blocks if blocks is not None else dense_blocks(dims, state)
    L = fr.lines(sp, "fd", dims)
    ei = fr.interior(eta, dims)
    return Ops(dims, LD, lambda v: VV @ v, lambda v: PV @ v, lambda p: VP @ p, ei,
               lambda rc, over_eta=True: fr.truth(rc, L, 0.0, ei if over_eta else None), _stencil(dims, eta, LD))


def oracle_ops(sp, dims, state=None, mode=orc.DIRECT, how="plain", nthreads=1):
    eta, deta, strain = _state(dims, state)
    L = fr.lines(sp, "fd", dims)
    ei = fr.interior(eta, dims)
    return Ops(dims, np.float64,
               lambda v: orc.stokes_mult_vv(dims, v, eta=eta, deta=deta, strain=strain, mode=mode, nthreads=nthreads),
               lambda v: orc.stokes_divergence(dims, v, mode=mode, nthreads=nthreads),
               lambda p: orc.stokes_mult_vp(dims, p, mode=mode, nthreads=nthreads), ei,
               lambda rc, over_eta=True: fr.chain(rc, L, 0.0, ei if over_eta else None, how)[0], _stencil(dims, eta, np.float64))


# ----------------------------------------------------------------------------------------------
# the apply
# ----------------------------------------------------------------------------------------------
def remove_mean(p, first=None):
    """p - mean(p); first: the mean's sum runs over that many leading entries only (fault l)."""
    p = np.asarray(p)
    if p.size == 0:
        return p.copy()
    s = p[:first].sum() if first is not None else p.sum()
    return p - s / p.dtype.type(p.size)


def apply(ops, x, kind, cfg, dt=np.float64, dot=kr.dot_pairwise, fault=None):
    """stokes_saddle_apply in dt arithmetic.  Returns dict(y, its = (velocity, Schur), hist = [(solve name, tol, [residual norms])])."""
    d, I = ops.d, ops.I
    m_vel, rtol_vel = cfg["vel"]
    m_schur, rtol_schur = cfg["schur"]
    m_svel, rtol_svel = cfg["svel"]
    if fault == "i" and m_vel > 0:
        m_vel -= 1
    if fault == "j":
        m_schur -= 1
    sweeps = cfg["pc_sweeps"]
    its = [0, 0]
    hist = []
    zero_v = np.zeros(I * d, dtype=dt)

    def note(name, out):
        hist.append((name, out["tol"], list(out["hist"])))
        return out

    def fdm_cm(rc):                          # (d, G) component-major -> the same shape
        return ops.fdm(rc.reshape((d,) + idims(ops.dims)), fault != "h").reshape(d, I)

    def pc(r):                               # MatVVPC solve, node-major in and out
        rc = np.ascontiguousarray(r.reshape(I, d).T)
        if sweeps == 0:
            z = fdm_cm(rc)
        else:
            out = note("pc", kr.fgmres(lambda v: ops.stencil(v.reshape(d, I).T).T.reshape(-1), lambda v: fdm_cm(v.reshape(d, I)).reshape(-1),
                                       rc.reshape(-1), None, sweeps, sweeps, rtol=1e-12, atol=1e-300, dt=dt, dot=dot))
            z = out["x"].reshape(d, I)
        return np.ascontiguousarray(z.T).reshape(-1)

    def vsolve(b, m, rtol, name):
        if I == 0:
            return zero_v, 0
        if m == 0:
            return pc(b), 0
        out = note(name, kr.fgmres(ops.vv, pc, b, None, 30, m, rtol=rtol, atol=1e-50, dt=dt, dot=dot))
        return out["x"], out["its"]

    def vel_solve(b):
        z, n = vsolve(b, m_vel, rtol_vel, "vel")
        its[0] += n
        return z

    def eta_scale(p):
        if not cfg["schur_jacobi"] or fault == "b":
            return p
        return p / ops.eta_int if fault == "a" else ops.eta_int * p

    def schur_apply(p):
        y = eta_scale(-ops.pv(vsolve(ops.vp(p), m_svel, rtol_svel, "svel")[0]))
        return y if fault == "c" else remove_mean(y)

    def schur_solve(b):
        b = eta_scale(b)
        if fault != "d":
            b = remove_mean(b)
        out = note("schur", kr.fgmres(schur_apply, None, b, None, 30, max(m_schur, 1), rtol=rtol_schur, atol=1e-50, dt=dt, dot=dot))
        its[1] += out["its"]
        return out["x"]

    xv, xp = split(np.asarray(x, dtype=dt), d)
    if fault == "k":
        xv = np.ascontiguousarray(xv.reshape(I, d).T).reshape(-1)
    if kind == 0:                            # block LU (stokes.C:1712)
        v1 = vel_solve(xv)
        p0 = ops.pv(v1)
        p0 = p0 + xp if fault == "e" else xp - p0
        p1 = schur_solve(p0)
        v2 = vel_solve(-ops.vp(p1))
        yv = v2 if fault == "f" else v1 + v2
    elif kind == 1:                          # block upper triangular (stokes.C:1745)
        p1 = schur_solve(xp)
        yv = vel_solve(xv - ops.vp(p1))
    elif kind == 2:                          # block diagonal (stokes.C:1770)
        yv = vel_solve(xv)
        p1 = schur_solve(xp)
    else:                                    # block lower triangular (stokes.C:1795)
        yv = vel_solve(xv)
        p0 = ops.pv(yv)
        if fault == "g":
            xp = p0                          # x_p read after p0 was written over it
        p0 = p0 + xp if fault == "e" else xp - p0
        p1 = schur_solve(p0)
    yp = remove_mean(p1)
    return dict(y=merge(yv, yp, d), its=tuple(its), hist=hist)


# ----------------------------------------------------------------------------------------------
# the bars
# ----------------------------------------------------------------------------------------------
def part_ratios(y, y_ld, y_rest, d):
    """krylov_ref.solve_ratios on the velocity and on the pressure part: dict(v_max, v_2, p_max, p_2)."""
    out = {}
    for name, k in (("v", 0), ("p", 1)):
        r = kr.solve_ratios(split(y, d)[k], split(y_ld, d)[k], [split(q, d)[k] for q in y_rest])
        out[name + "_max"], out[name + "_2"] = r
    return out


def pair_ratios(y, ya, yb, d):
    """The large shape: |y - A| over MARGIN |A - B|, max-norm and 2-norm, per part."""
    out = {}
    for name, k in (("v", 0), ("p", 1)):
        a = split(ya, d)[k].astype(LD)
        e, w = np.abs(split(y, d)[k].astype(LD) - a), np.abs(split(yb, d)[k].astype(LD) - a)
        out[name + "_max"] = kr.ratio(e.max(), LD(MARGIN) * w.max())
        out[name + "_2"] = kr.ratio(np.sqrt((e * e).sum()), LD(MARGIN) * np.sqrt((w * w).sum()))
    return out


def gap(hist):
    """The smallest factor by which a residual norm of any inner solve misses its tolerance, max(r / tol, tol / r) minimised over
    the histories; inf where there is none.  A case's iteration counts are a property of the method where this exceeds GAP."""
    g = np.inf
    for name, tol, rs in hist:
        for r in rs:
            r, tol = LD(r), LD(tol)
            if r == 0 or tol == 0:
                continue
            g = min(g, float(max(r / tol, tol / r)))
    return g


def t_mean(n):
    return max(1, -(-n // (MEAN_RB * MEAN_RT))) + 8 + 8


def mean_bar(yp):
    """The bound on |mean(y_p)| of the module docstring."""
    yp = np.asarray(yp, dtype=LD)
    if yp.size <= 1:
        return LD(0)
    return LD((t_mean(yp.size) + 2) * U53) * np.abs(yp).mean()


def mean_of(yp):
    yp = np.asarray(yp, dtype=LD)
    return abs(yp.mean()) if yp.size else LD(0)


# ----------------------------------------------------------------------------------------------
# states, right-hand sides and the case tables
# ----------------------------------------------------------------------------------------------
STATES = ("unit", "variable", "jacobian")


def make_state(dims, name, seed):
    """(eta, eta', strain) on the full grid, None = the handle's default.  variable: eta log-uniform on [0.5, 10].  jacobian: the same
    eta, a random symmetric strain S of unit size and eta' = -c eta / (eps + gamma), gamma = S : S / 2, eps = 1e-2, c uniform on
    (0, 1/3]: what the power law eta = B (eps + gamma)^((1 - n) / 2 n) gives for exponents n up to 3 (stokes.C:700-716).  The tensor
    eta I + eta' S (x) S then keeps eigenvalues >= eta / 3: MatVV stays positive definite, as in a Newton step."""
    d, N = len(dims), int(np.prod(dims))
    rng = np.random.default_rng(seed)
    if name == "unit":
        return None
    eta = np.exp(rng.uniform(np.log(0.5), np.log(10.0), N))
    if name == "variable":
        return eta, None, None
    S = rng.standard_normal((d, N, d))
    S = 0.5 * (S + S.transpose(2, 1, 0))
    gamma = 0.5 * (S * S).sum(axis=(0, 2))
    deta = -rng.uniform(1e-3, 1.0 / 3.0, N) * eta / (1e-2 + gamma)
    return eta, deta, S.reshape(d, N * d)


def rhs(dims, seed, pmean=0.0):
    """Noise; pmean is added to the pressure part."""
    d = len(dims)
    x = np.random.default_rng(seed).standard_normal((d + 1) * int(np.prod(idims(dims))))
    x.reshape(-1, d + 1)[:, d] += pmean
    return x


def case_rhs(c, base):
    """C7's right-hand side carries a pressure mean of 3: the constant is no part of the Schur system (S 1 = 0, and the Krylov
    vectors are made zero-mean), so a mean left in KSPSchur's right-hand side changes nothing but the norm its relative tolerance
    is taken from -- visible only where a solve ends on its tolerance, and only with a mean that weighs beside the rest."""
    return rhs(c[0], case_seed(c, base) + 1, 3.0 if c[3] == "C7" else 0.0)


SMALL = [(3, 3), (4, 3), (11, 9), (12, 11), (9, 9, 7), (10, 9, 8), (6, 70), (5, 4, 70), (5, 131)]
LARGE = (43, 42, 44)
CONFIG_SHAPES = [(10, 9, 8), (5, 4, 70)]

# C7: an inner solve that ends on its tolerance inside the limit.  Each tolerance is the geometric mean of the truth's relative
# residuals at two consecutive iterations (to four digits), the iterations chosen so that the gap condition holds for every inner
# solve of the case; (dims, kind, state) -> (tau_v, tau_s), with the truth's counts and gap.  State `unit` throughout: with the
# random viscosity of the other two states the velocity solves lose 15 % of the residual per iteration or less, and no tolerance
# keeps a factor 1.25 from two consecutive residuals; at eta == 1 they lose a factor 3 (velocity) and 1.7 .. 1.9 (Schur).
C7_TOL = {
    ((10, 9, 8), 0, "unit"): (0.003341, 0.003111),   # counts (11, 12), gap 1.36
    ((10, 9, 8), 3, "unit"): (0.001118, 0.003111),   # counts (7, 12), gap 1.36
    ((5, 4, 70), 0, "unit"): (0.01098, 0.01082),     # counts (9, 7), gap 1.50
    ((5, 4, 70), 3, "unit"): (0.02766, 0.01082),     # counts (5, 7), gap 1.50
}

CONFIGS = {
    "C1": config(),
    "C2": config(svel=(2, 1e-5)),
    "C3": config(schur_jacobi=False),
    "C4": config(pc_sweeps=2),
    "C5": config(),                          # option saddle_node_major = 1 at create
    "C6": config(vel=(0, 1e-5), schur=(1, 1e-5)),
}
# the state of C2 .. C7 per (configuration, shape index, kind): `variable` wherever the Jacobi scaling or pc_sweeps is the point
# (with eta == 1 the scaling is invisible); across C2 .. C7 every (shape, kind) pair meets every state
CONFIG_STATE = {
    "C2": {(0, 0): "jacobian", (0, 3): "variable", (1, 0): "unit", (1, 3): "jacobian"},
    "C3": {(0, 0): "variable", (0, 3): "variable", (1, 0): "variable", (1, 3): "jacobian"},
    "C4": {(0, 0): "variable", (0, 3): "jacobian", (1, 0): "variable", (1, 3): "variable"},
    "C5": {(0, 0): "unit", (0, 3): "jacobian", (1, 0): "variable", (1, 3): "unit"},
    "C6": {(0, 0): "variable", (0, 3): "unit", (1, 0): "jacobian", (1, 3): "variable"},
    "C7": {(0, 0): "unit", (0, 3): "unit", (1, 0): "unit", (1, 3): "unit"},
}


def case_config(c):
    dims, kind, state, name = c
    if name == "C7":
        tv, ts = C7_TOL[(dims, kind, state)]
        return config(vel=(30, tv), schur=(30, ts))
    return CONFIGS[name]


def cases():
    """(dims, kind, state, configuration name): C1 on every small shape, kind and state; C2 .. C7 on the two configuration shapes,
    kinds 0 and 3."""
    out = [(dims, kind, state, "C1") for dims in SMALL for kind in range(4) for state in STATES]
    for name in ("C2", "C3", "C4", "C5", "C6", "C7"):
        for (si, kind), state in sorted(CONFIG_STATE[name].items()):
            out.append((CONFIG_SHAPES[si], kind, state, name))
    return out


LARGE_CASES = [(LARGE, 0, "variable", "C1"), (LARGE, 2, "variable", "C1")]


def case_id(c):
    dims, kind, state, name = c
    return "%s-k%d-%s-%s" % ("x".join(map(str, dims)), kind, state, name)


def case_seed(c, base):
    """One seed per (shape, state): the state is shared by the kinds and configurations of a shape, the right-hand side too."""
    dims, kind, state, name = c
    return base + 1000 * STATES.index(state) + sum((i + 1) * p for i, p in enumerate(dims))


_BLOCKS = {}
_REF = {}


def reference(sp, c, base, state=None):
    """dict(x, state, cfg, ld, rest) of a case, computed once and left unchanged.  state: the doubles the device holds (read back
    from the handle); None: make_state's."""
    if c not in _REF:
        dims, kind, sname, name = c
        seed = case_seed(c, base)
        st = make_state(dims, sname, seed) if state is None else state
        cfg = case_config(c)
        x = case_rhs(c, base)
        key = (dims, sname)
        if key not in _BLOCKS:
            _BLOCKS[key] = dense_blocks(dims, st)
        ld = apply(truth_ops(sp, dims, st, _BLOCKS[key]), x.astype(LD), kind, cfg, LD, kr.dot_ld)
        rest = [apply(oracle_ops(sp, dims, st, orc.DIRECT, "plain"), x, kind, cfg, np.float64, kr.dot_pairwise),
                apply(oracle_ops(sp, dims, st, orc.FAST, "evenodd"), x, kind, cfg, np.float64, kr.dot_strided)]
        _REF[c] = dict(x=x, state=st, cfg=cfg, ld=ld, rest=rest)
    return _REF[c]
