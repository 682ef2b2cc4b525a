"""The restarted flexible GMRES of csrc/krylov.hip restated in NumPy (helper module of test_krylov_host.py and
test_gpu_krylov_steps.py): the long-double truth of one Gram-Schmidt step and of a whole solve, the derived bars, two double
restatements that differ only in summation order, the planted faults, and the test operators.

A solve is observed through its callbacks (the operator, the preconditioner, the reduction): they see the exact bits of every basis
vector V_0 .. V_j, of z_j = M v_j and of w = A z_j, so every step has a local truth and no error propagates into its bar.

Counts (u = 2^-53; every count is the largest number of roundings one term of the sum can meet, the kernel's addition order is fixed):

  T_dot   a dot product:  trips of the grid-stride loop per thread (RB ST = 262 144 elements per trip, or that many PAIRS on the
          16-byte route, which then adds its two half-sums: + 1)  +  6 shuffle levels  +  16 wave sums  +  the finish  +  1 product.
          finish: gs_row_sums 4 + 6 (one-reduction step), the serial 256-term sum of k_orth_update (three-launch step, one rank),
          k_rows_finish 6 + 4 (three-launch step with a reduction callback; also the second stage of every norm).
          dev_norm (k_multidot, 256 threads): trips of 65 536 + 6 + 4 + (6 + 4) + 1.
  dots    |hcol_i - d_i| <= T_dot u E_i,  E_i = sum_e |V_ie w_e|;   the same for w.w and for nsq against sum_e V_{j+1,e}^2.
  stored  V_{j+1} = f (w - sum_i c_i V_i): a term meets its product, up to k = j + 1 subtractions and the scaling by f: (k + 2), one
          more for a fused / unfused product: (k + 3) B_e, B_e = |w_e| + sum |c_i| |V_ie|.  c_i = d_i / rn_i^2 carries the error of
          d_i (T_dot E_i), two divisions, and the device's rn_i^2 = fl(sqrt(nsq))^2: nsq's own T_dot and the square root twice
          (T_dot + 2, relative to |d_i| <= E_i):  T_c = 2 T_dot + 4.  On the three-launch step rn == 1 and T_c = T_dot.
          The scale f is the solver's own business: the bar is taken against phi u with phi the best-fit scalar (V_{j+1}.u) / (u.u).
  first   V_0 = r (1 / |r|): |r|^2 with T_dot (halved by the root), the root, the reciprocal, the product: <= T_dot + 3.
  norm    three-launch step: |V_{j+1}| = 1 up to nsq's T_dot / 2, the root, the reciprocal and the product: <= T_dot + 3.
  eigen   b an eigenvector: x = (g_0 / R_00) V_0: the Givens quotient and product, the triangular solve's quotient, the axpy's
          product, V_0's reciprocal and product on top of one dot product: T_dot + 6.

A reduction callback that doubles the sums in place is two ranks holding identical halves (`dup` = 2): the truth is the same
algorithm with every inner product doubled."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
RB, RT, ST, KB = 256, 256, 1024, 8
MARGIN = 16.0
DBL_MAX = 1.7976931348623157e308


# ----------------------------------------------------------------------------------------------
# counts
# ----------------------------------------------------------------------------------------------
def trips(n, per, v2=False):
    """Additions a thread's partial sum goes through: one per grid-stride trip, one more where two half-sums are joined."""
    m = n // 2 if v2 else n
    return max(1, -(-m // per)) + (1 if v2 else 0)


def t_dot(n, kind):
    v2 = n % 2 == 0
    if kind == "gs":              # k_gs_dots / k_gs_update, finished by gs_row_sums
        return trips(n, RB * ST, v2) + 6 + 16 + (4 + 6) + 1
    if kind == "three":           # k_multidot_grouped, finished by the serial sum of k_orth_update
        return trips(n, RB * ST, v2) + 6 + 16 + 256 + 1
    if kind == "three_reduce":    # k_multidot_grouped, finished by k_rows_finish
        return trips(n, RB * ST, v2) + 6 + 16 + (6 + 4) + 1
    if kind == "three_nsq":       # k_orth_update's squares (8-byte loads), finished by k_givens_scale / k_rows_finish
        return trips(n, RB * ST) + 6 + 16 + (6 + 4) + 1
    if kind == "norm":            # dev_norm
        return trips(n, RB * RT) + 6 + 4 + (6 + 4) + 1
    raise ValueError(kind)


def step_counts(n, exact, reduce):
    """(T_dot of the dots, T_dot of the stored vector's squares, T_c)."""
    if not exact:
        t = t_dot(n, "gs")
        return t, t, 2 * t + 4
    t = t_dot(n, "three_reduce" if reduce else "three")
    return t, t_dot(n, "three_nsq"), t


def ratio(err, bar):
    """max err / bar; an error where the bar is 0, or a non-finite error, is inf."""
    err = np.atleast_1d(np.asarray(err, dtype=LD)).ravel()
    bar = np.atleast_1d(np.asarray(bar, dtype=LD)).ravel()
    if err.size == 0:
        return 0.0
    r = np.full(err.shape, np.inf)
    r[err == 0] = 0.0
    ok = np.isfinite(err.astype(np.float64)) & (bar > 0) & (err != 0)
    r[ok] = (err[ok] / bar[ok]).astype(np.float64)
    return float(r.max())


# ----------------------------------------------------------------------------------------------
# one step
# ----------------------------------------------------------------------------------------------
def step_truth(VL, wl, exact, dup=1, aV=None):
    """VL: (k, n) long double, the stored basis (aV: its absolute values, where the caller keeps them); wl: (n,) long double.
    Sums are over the local entries (one rank's half)."""
    aV, aw = np.abs(VL) if aV is None else aV, np.abs(wl)
    d = (VL * wl).sum(axis=1)
    E = (aV * aw).sum(axis=1)
    ww = (wl * wl).sum()
    nv2 = (VL * VL).sum(axis=1)                 # rn_i^2 = dup nv2_i
    if exact:
        c, ec = LD(dup) * d, LD(dup) * E        # rn == 1
    else:
        c, ec = d / nv2, E / nv2                # dup d_i / (dup nv2_i)
    u = wl - (c[:, None] * VL).sum(axis=0)
    B = aw + (np.abs(c)[:, None] * aV).sum(axis=0)
    Cw = (ec[:, None] * aV).sum(axis=0)
    return dict(d=d, E=E, ww=ww, c=c, u=u, B=B, C=Cw)


def stored_ratio(vnext, t, k, T_c):
    """(ratio of the stored-vector bar, phi)."""
    vn = np.asarray(vnext, dtype=LD)
    uu = (t["u"] * t["u"]).sum()
    if not uu > 0:
        return (0.0 if not np.any(vn) else np.inf), LD(0)
    phi = (vn * t["u"]).sum() / uu
    if not (phi > 0 and np.isfinite(np.float64(phi))):
        return np.inf, phi
    bar = phi * LD(U53) * (LD(k + 3) * t["B"] + LD(T_c) * t["C"])
    return ratio(np.abs(vn - phi * t["u"]), bar), phi


def check_trace(tr, b, exact, dup=1, reduce=False):
    """Every step bar on every accepted iteration of a recorded solve.  tr: dict(bnsq, cycles=[dict(ax, rnsq, steps=[dict(v, w, hcol,
    nsq)])]) -- ax the recorded A x of the cycle's residual evaluation (None: r = b), hcol / nsq / bnsq / rnsq the local sums a
    reduction callback saw (None: not observed).  Returns the worst ratio per bar."""
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    T_d, T_n, T_c = step_counts(n, exact, reduce)
    T_0 = t_dot(n, "norm")
    out = dict(first=0.0, stored=0.0, dots=0.0, nsq=0.0, norm=0.0, rnorm=0.0)

    def worse(key, v):
        out[key] = max(out[key], v)
    if tr.get("bnsq") is not None:
        s = (b.astype(LD) ** 2).sum()
        worse("rnorm", ratio(abs(LD(tr["bnsq"]) - s), T_0 * LD(U53) * s))
    for cyc in tr["cycles"]:
        steps = cyc["steps"]
        r = (b if cyc["ax"] is None else b - np.asarray(cyc["ax"], dtype=np.float64)).astype(LD)   # the device's own subtraction
        rr = (r * r).sum()
        if cyc.get("rnsq") is not None:
            worse("rnorm", ratio(abs(LD(cyc["rnsq"]) - rr), T_0 * LD(U53) * rr))
        if not steps:
            continue
        rnorm = np.sqrt(LD(dup) * rr)
        worse("first", ratio(np.abs(steps[0]["v"].astype(LD) - r / rnorm), LD((T_0 + 3) * U53) * np.abs(r) / rnorm))
        VL, aV = np.empty((len(steps), n), dtype=LD), np.empty((len(steps), n), dtype=LD)
        for j, s in enumerate(steps):
            VL[j] = s["v"]
            aV[j] = np.abs(VL[j])
            t = step_truth(VL[:j + 1], s["w"].astype(LD), exact, dup, aV[:j + 1])
            if s.get("hcol") is not None:
                h = np.asarray(s["hcol"], dtype=LD)
                worse("dots", ratio(np.abs(h[:j + 1] - t["d"]), LD(T_d * U53) * t["E"]))
                if not exact:
                    worse("dots", ratio(abs(h[j + 1] - t["ww"]), LD(T_d * U53) * t["ww"]))
            if j + 1 < len(steps):
                vn = steps[j + 1]["v"]
                q, phi = stored_ratio(vn, t, j + 1, T_c)
                worse("stored", q)
                v2 = (vn.astype(LD) ** 2).sum()
                if exact:
                    worse("norm", ratio(abs(np.sqrt(LD(dup) * v2) - 1), LD((T_n + 3) * U53)))
                elif s.get("nsq") is not None:
                    worse("nsq", ratio(abs(LD(s["nsq"]) - v2), LD(T_n * U53) * v2))
    return out


# ----------------------------------------------------------------------------------------------
# the whole solve
# ----------------------------------------------------------------------------------------------
def dot_ld(a, c):
    return (a * c).sum()


def dot_pairwise(a, c):
    return np.sum(a * c)


def dot_strided(a, c, lanes=256):
    """The device's shape: `lanes` running sums over a stride, added sequentially, then the lanes pairwise."""
    p = a * c
    pad = (-p.size) % lanes
    if pad:
        p = np.concatenate([p, np.zeros(pad, dtype=p.dtype)])
    return p.reshape(-1, lanes).sum(axis=0).sum() if p.size else p.dtype.type(0)


def dot_reversed(a, c):
    """Pairwise from the far end.  (The caps count the depth of the device's order: a benign order is another one of bounded depth; a
    strictly sequential sum of n terms is not held to them.)"""
    return np.sum((a * c)[::-1].copy())


FAULTS = {"a": "the dots skip the last element of an odd n",
          "b": "the dots skip everything past the first grid-stride trip",
          "c": "c_i = d_i / rn_i",
          "d": "x += V y where x += Z y is due",
          "e": "the w.w row taken from the previous iteration when j + 1 is a multiple of 8",
          "f": "the reduce result ignored"}


def fgmres(A, M, b, x0, restart, max_it, rtol=1e-300, atol=1e-50, exact=False, dup=1, dt=np.float64, dot=dot_pairwise, fault=None,
           trip=None, trace=False):
    """chebhip_fgmres_solve in `dt` arithmetic: the one-reduction classical Gram-Schmidt with carried rn (exact: the three-launch
    step), the clamp of e2 at 1e-12 w.w, the estimated h_{j+1,j} on a cycle's last column, the Givens solve, x += Z y.
    A(x) and M(v) work in dt; x0 None is the zero guess that is never stored.  fault: a key of FAULTS (trip: elements of fault b's
    first trip).  Returns dict(x, its, reason, rnorm, last_est, trace, tol, hist): hist holds every residual norm the solve compared
    with tol, in order (a cycle's start residual, then one per column)."""
    b = np.asarray(b, dtype=dt)
    n, m = b.size, restart
    one, zero, D = dt(1), dt(0), dt(dup)

    def dotf(a, c):
        if fault == "a" and n & 1:
            a, c = a[:-1], c[:-1]
        if fault == "b":
            a, c = a[:trip], c[:trip]
        return dt(dot(a, c)) if a.size else zero

    def finite_pos(v):
        return v > 0 and v <= DBL_MAX
    bnsq = dotf(b, b)
    bnorm = np.sqrt(D * bnsq)
    tol = max(dt(rtol) * bnorm, dt(atol))
    x = None if x0 is None else np.array(x0, dtype=dt)
    its, reason, first, rnorm, last_est = 0, 0, True, zero, False
    tr = dict(bnsq=bnsq, cycles=[])
    hist = []
    while True:
        ax = rnsq = None
        if first and x is None:
            beta, r = bnorm, b
        else:
            ax = A(x if x is not None else np.zeros(n, dtype=dt))
            r = b - ax
            rnsq = dotf(r, r)
            beta = np.sqrt(D * rnsq)
        first = False
        rnorm = beta
        hist.append(beta)
        cyc = dict(ax=ax, rnsq=rnsq, steps=[])
        tr["cycles"].append(cyc)
        if not beta == beta:
            reason = -9
            break
        if beta <= tol:
            reason = 3 if beta <= atol else 2
            break
        if its >= max_it:
            reason = -3
            break
        V, Z, rn = [r * (one / beta)], [], [one]
        H = np.zeros((m + 1, m), dtype=dt)
        cs, sn, g = np.zeros(m, dtype=dt), np.zeros(m, dtype=dt), np.zeros(m + 1, dtype=dt)
        g[0] = beta
        kk, stop, ww_prev = 0, False, zero
        for j in range(m):
            if its + j >= max_it or stop:
                break
            z = M(V[j]) if M is not None else V[j]
            Z.append(z)
            w = np.array(A(z), dtype=dt)
            use_next = j + 1 < m and its + j + 1 < max_it
            st = dict(v=V[j], z=z, w=w.copy(), hcol=None, nsq=None)
            cyc["steps"].append(st)
            loc = np.array([dotf(V[i], w) for i in range(j + 1)], dtype=dt)
            if not exact:
                wwl = dotf(w, w)
                if fault == "e" and (j + 1) % KB == 0:
                    wwl = ww_prev
                ww_prev = wwl
                st["hcol"] = np.append(loc, wwl)
                Dh = one if fault == "f" else D
                hc, ww = Dh * loc, Dh * wwl
                h = hc / np.array(rn, dtype=dt)
                coef = h if fault == "c" else h / np.array(rn, dtype=dt)
                ssq = zero
                for i in range(j + 1):
                    ssq = ssq + h[i] * h[i]
                e2 = ww - ssq
                if not e2 >= dt(1.0e-12) * ww:
                    e2 = dt(1.0e-12) * ww
                f = one / np.sqrt(e2) if finite_pos(e2) else zero
                if use_next:
                    xw = w
                    for i in range(j + 1):
                        xw = xw - coef[i] * V[i]
                    xw = xw * f
                    nl = dotf(xw, xw)
                    st["nsq"] = nl
                    rr = np.sqrt(D * nl)
                    rn.append(rr if finite_pos(rr) else one)
                    hn = rr / f if f > 0 else (zero if ww == 0 else dt(np.nan))
                    V.append(xw)
                else:
                    hn = one / f if f > 0 else (zero if ww == 0 else dt(np.nan))
            else:
                st["hcol"] = loc
                h = (one if fault == "f" else D) * loc
                xw = w
                for i in range(j + 1):
                    xw = xw - h[i] * V[i]
                nl = dotf(xw, xw)
                st["nsq"] = nl
                hn = np.sqrt(D * nl)
                if use_next:
                    V.append(xw * (one / hn if finite_pos(hn) else zero))
            col = np.append(h, hn)
            for i in range(j):
                t = cs[i] * col[i] + sn[i] * col[i + 1]
                col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
                col[i] = t
            den = np.hypot(col[j], col[j + 1])
            if den == 0 or not den == den:
                res = dt(np.nan)
            else:
                c_, s_ = col[j] / den, col[j + 1] / den
                cs[j], sn[j] = c_, s_
                col[j], col[j + 1] = den, zero
                g[j + 1] = -s_ * g[j]
                g[j] = c_ * g[j]
                res = abs(g[j + 1])
            H[:j + 2, j] = col
            if not res == res:
                reason, kk, stop = -9, j, True
            else:
                kk, rnorm = j + 1, res
                hist.append(res)
                if res <= tol or its + kk >= max_it:
                    stop = True
        last_est = (not exact) and kk > 0 and not (kk < m and its + kk < max_it)
        its += kk
        if kk > 0:
            y = np.zeros(kk, dtype=dt)
            for i in range(kk - 1, -1, -1):
                s = g[i]
                for q in range(i + 1, kk):
                    s = s - H[i, q] * y[q]
                y[i] = s / H[i, i]
            basis = V if (M is None or fault == "d") else Z
            s = np.zeros(n, dtype=dt) if x is None else x
            for q in range(kk):
                s = s + y[q] * basis[q]
            x = s
        if reason == -9:
            break
        if rnorm <= tol and not last_est:
            reason = 3 if rnorm <= atol else 2
            break
        if its >= max_it and not rnorm <= tol:
            reason = -3
            break
    if x is None:
        x = np.zeros(n, dtype=dt)
    return dict(x=x, its=its, reason=reason, rnorm=rnorm, last_est=last_est, trace=tr if trace else None, tol=tol, hist=hist)


def solve_ratios(x, x_ld, x_rest):
    """(max-norm, 2-norm) of |x - x_ld| over MARGIN times the larger error of the restatements."""
    x_ld = np.asarray(x_ld, dtype=LD)

    def errs(y):
        e = np.abs(np.asarray(y).astype(LD) - x_ld)
        if e.size == 0:
            return LD(0), LD(0)
        return e.max(), np.sqrt((e * e).sum())
    bars = [errs(y) for y in x_rest]
    e = errs(x)
    return tuple(ratio(e[i], LD(MARGIN) * max(q[i] for q in bars)) for i in (0, 1))


def scalar_ratio(v, v_ld, v_rest):
    return ratio(abs(LD(v) - LD(v_ld)), LD(MARGIN) * max(abs(LD(q) - LD(v_ld)) for q in v_rest))


def eigen_cap(n):
    return t_dot(n, "gs") + 6


# ----------------------------------------------------------------------------------------------
# the test operators: one formula, a NumPy (any precision) and a torch twin
# ----------------------------------------------------------------------------------------------
class Op:
    """A x = a (.) x + s roll(x, 1) + t roll(x, -q) with |s| + |t| = 0.4 min|a|.
    kind "std": a spread over a decade; "ill": a takes the four values 1, 1e2, 1e4, 1e6 at random places and s = t = 0 (the bound on
    |s| + |t| allows it): every Krylov space has four dimensions, so the fifth w of a run is parallel to the basis to rounding, e2
    clamps, and the vector stored then is scaled noise with rn far from 1; "circ": a constant (the constant vector is an eigenvector).
    prec None / "fixed" (a diagonal near 1 / a) / "vary" (a diagonal that changes with the call count)."""

    def __init__(self, n, seed, kind="std", prec=None, q=3):
        rng = np.random.default_rng(seed)
        self.n, self.q, self.kind, self.prec = n, q, kind, prec
        if kind == "ill":
            self.a = 10.0 ** (2.0 * rng.integers(0, 4, n))
            self.s, self.t = 0.0, 0.0
            self.dfix = np.ones(n)
        else:
            self.a = np.full(n, 2.5) if kind == "circ" else 10.0 ** rng.uniform(0.0, 1.0, n)
            amin = float(self.a.min()) if n else 1.0
            self.s, self.t = 0.25 * amin, -0.15 * amin
            self.dfix = 1.0 / (self.a * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, n)))
        self.P = 1.0 + 0.3 * rng.uniform(-1.0, 1.0, (3, n))
        self.calls = 0
        self._t = None

    def reset(self):
        self.calls = 0

    def A(self, x, dt=np.float64):
        return self.a.astype(dt) * x + dt(self.s) * np.roll(x, 1) + dt(self.t) * np.roll(x, -self.q)

    def M(self, v, dt=np.float64):
        d = self.dfix.astype(dt)
        if self.prec == "vary":
            d = d * self.P[self.calls % 3].astype(dt)
        self.calls += 1
        return d * v

    def callables(self, dt):
        """(A, M) for fgmres in dt arithmetic, the call count reset."""
        self.reset()
        return (lambda x: self.A(x, dt)), ((lambda v: self.M(v, dt)) if self.prec else None)

    # the torch twin (device tensors)
    def _dev(self):
        if self._t is None:
            import torch
            self._t = dict(a=torch.from_numpy(self.a).cuda(), dfix=torch.from_numpy(self.dfix).cuda(), P=torch.from_numpy(self.P).cuda())
        return self._t

    def A_torch(self, x):
        import torch
        T = self._dev()
        return T["a"] * x + self.s * torch.roll(x, 1) + self.t * torch.roll(x, -self.q)

    def M_torch(self, v):
        T = self._dev()
        d = T["dfix"]
        if self.prec == "vary":
            d = d * T["P"][self.calls % 3]
        self.calls += 1
        return d * v


def rhs(gen, n, seed):
    rng = np.random.default_rng(seed)
    if gen == "normal":
        return rng.standard_normal(n)
    if gen == "scaled":
        return rng.standard_normal(n) * 10.0 ** rng.integers(-30, 31, size=n)
    if gen == "impulse":
        b = np.zeros(n)
        if n:
            b[max(n - 2, 0)] = 1.75           # near the end: past the first grid-stride trip of a long vector, and the rolls wrap
        return b
    if gen == "const":
        return np.full(n, 0.7)
    raise ValueError(gen)


def reference_solves(op, b, x0, restart, max_it, exact, dup, rtol=1e-300):
    """(long-double solve, [two double restatements]) of one case."""
    A, M = op.callables(LD)
    ld = fgmres(A, M, np.asarray(b, dtype=LD), None if x0 is None else np.asarray(x0, dtype=LD), restart, max_it, rtol=rtol, exact=exact,
                dup=dup, dt=LD, dot=dot_ld)
    rest = []
    for dot in (dot_pairwise, dot_strided):
        A, M = op.callables(np.float64)
        rest.append(fgmres(A, M, b, x0, restart, max_it, rtol=rtol, exact=exact, dup=dup, dot=dot, trace=True))
    return ld, rest


# ----------------------------------------------------------------------------------------------
# the cases: (class, n, restart, max_it, exact, reduce, prec, x_nonzero, generator)
# ----------------------------------------------------------------------------------------------
# reduce: None, "double" (the callback doubles the sums: two ranks with identical halves) or "ident" (a communicator of one rank).
# Restarts 5, 8, 9, 17, 30 meet the KB = 8 row groups (the w.w row alone in a group at j + 1 = 8, 16, 24), the k % 4 tails of the update
# loops and the second trip of gs_row_sums (more than 16 rows); 256 is the limit of GsShared.  max_it ends a solve at the end of a cycle,
# inside one (an estimated last column), and after two or more.  262 921 / 530 434 are the smallest odd / even n with a second
# grid-stride trip (8-byte loads: 262 144 elements per trip; 16-byte loads: 262 144 pairs).
# Tiny sizes: the three-launch step only where the iteration limit stays below n (at the n-th column the new vector is rounding noise
# around 0 and whether the solve reports breakdown or the limit is not a property of the method).
CASES = [
    ("tiny", 0, 1, 2, 0, "double", None, 0, "normal"),
    ("tiny", 0, 2, 2, 1, "ident", "fixed", 0, "normal"),
    ("tiny", 1, 1, 1, 0, "ident", "vary", 0, "normal"),
    ("tiny", 1, 2, 1, 0, None, None, 0, "normal"),
    ("tiny", 2, 1, 2, 0, None, "fixed", 1, "normal"),
    ("tiny", 2, 2, 2, 0, "double", "vary", 0, "normal"),
    ("tiny", 2, 1, 1, 1, None, None, 0, "normal"),
    ("tiny", 2, 2, 1, 1, "double", "fixed", 0, "normal"),
    ("tiny", 3, 1, 3, 0, None, None, 1, "normal"),
    ("tiny", 3, 2, 3, 0, "ident", "fixed", 0, "scaled"),
    ("tiny", 3, 2, 2, 1, "double", "fixed", 0, "normal"),
    ("tiny", 3, 1, 2, 1, None, "vary", 1, "normal"),
    ("small", 259, 256, 256, 0, None, "fixed", 0, "normal"),
    ("small", 258, 256, 259, 0, "double", None, 0, "normal"),
    ("small", 259, 256, 256, 1, "double", "vary", 1, "scaled"),
    ("small", 258, 256, 256, 1, None, "fixed", 0, "const"),
    ("small", 259, 256, 256, 0, "ident", "vary", 0, "impulse"),
    ("small", 258, 256, 259, 1, "ident", None, 1, "normal"),
    ("medium", 4097, 5, 10, 0, None, None, 0, "normal"),
    ("medium", 4098, 5, 13, 0, "double", "fixed", 1, "scaled"),
    ("medium", 4097, 8, 8, 0, None, "vary", 0, "impulse"),
    ("medium", 4098, 8, 16, 0, "double", None, 0, "const"),
    ("medium", 4097, 8, 19, 1, "ident", "fixed", 1, "normal"),
    ("medium", 4097, 9, 9, 1, None, "fixed", 0, "normal"),
    ("medium", 4098, 9, 12, 1, "double", "vary", 1, "normal"),
    ("medium", 4097, 9, 12, 0, "ident", None, 0, "normal"),
    ("medium", 4097, 9, 12, 0, None, None, 0, "normal"),
    ("medium", 4097, 17, 17, 0, "double", "fixed", 0, "normal"),
    ("medium", 4098, 17, 20, 0, None, "vary", 1, "scaled"),
    ("medium", 4097, 17, 34, 1, "double", None, 0, "impulse"),
    ("medium", 4098, 17, 17, 1, "ident", "vary", 0, "normal"),
    ("medium", 4098, 17, 17, 1, None, "vary", 0, "normal"),
    ("medium", 4098, 30, 30, 0, None, "fixed", 0, "normal"),
    ("medium", 4097, 30, 33, 0, "double", "vary", 1, "const"),
    ("medium", 4098, 30, 30, 1, None, None, 0, "scaled"),
    ("medium", 4097, 30, 64, 1, "double", "fixed", 0, "normal"),
    ("big", 262921, 9, 9, 0, None, "fixed", 0, "normal"),
    ("big", 262921, 9, 10, 1, "double", None, 1, "scaled"),
    ("big", 530434, 9, 10, 0, "double", "vary", 0, "normal"),
    ("big", 530434, 9, 9, 1, None, "fixed", 1, "impulse"),
    ("big", 530434, 9, 10, 0, "ident", None, 0, "const"),
    ("big", 262921, 9, 10, 1, "ident", "vary", 0, "normal"),
]
# The clamping operator: only the step bars apply.  Zero initial guess only: the stored-vector bar takes the scale from a best fit, which
# presumes that the error of u is small beside u in every block of a; a start residual b - A x0 spread over 10^6 breaks that presumption
# at the step after a clamped one (the restatements themselves then sit at 0.3 ... 3 of the bar), and says nothing about the kernel.
ILL_CASES = [
    ("ill", 4097, 9, 9, 0, None, None, 0, "normal"),
    ("ill", 4098, 17, 17, 0, "double", None, 0, "normal"),
]


def case_id(c):
    cls, n, r, mi, exact, red, prec, xnz, gen = c
    return "%s-n%d-r%d-it%d-%s-%s-M%s-x%d-%s" % (cls, n, r, mi, "three" if exact else "one", red or "noreduce", prec or "none", xnz, gen)


def case_route(c):
    """The name of a case's route in profiles/krylov/ratios.txt."""
    cls, n, r, mi, exact, red, prec, xnz, gen = c
    v2 = n % 2 == 0
    return "%s | %s | %s, %d trip%s | %s" % ("three-launch" if exact else "one-reduction", {None: "no reduce", "double": "reduce x2", "ident": "reduce id"}[red],
                                            "16-byte" if v2 else "8-byte", trips(n, RB * ST, v2) - v2, "s" if trips(n, RB * ST, v2) - v2 > 1 else "", cls)


def case_setup(c, seed, n=None):
    """(op, b, x0) of a case; n overrides the size (the host tests run the same cases at reduced n)."""
    cls, n0, r, mi, exact, red, prec, xnz, gen = c
    n = n0 if n is None else n
    op = Op(n, seed, kind="ill" if cls == "ill" else "std", prec=prec)
    b = rhs(gen, n, seed + 1)
    x0 = np.random.default_rng(seed + 2).standard_normal(n) * (np.abs(b).max() if n else 1.0) if xnz else None
    return op, b, x0
