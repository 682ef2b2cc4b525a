"""The variable-coefficient Helmholtz operator restated in NumPy long double (helper module of test_varhelm_host.py /
test_gpu_varhelm.py).  No dense matrix except `dense`, for the tiny grids of the solve tests.

Definition.  For unknowns x (interior nodes of a wall direction, all nodes of a periodic one, row-major, fields
stacked), boundary data g (compact: row-major over the end nodes of the wall directions) and full-grid fields kappa, c:
  1. on every line of a wall direction k the two end values are Q_k x_line + Binv_k (g_first, g_last), Q_k and Binv_k the DOUBLES
     sp.helmholtz_line_box(P_k, ends_k, s_k) returns;
  2. y = c x + sum_k (-s_k^2) [D_k (kappa . D_k W)] at the unknown nodes, D the CGL matrix (lw.dense_D) on a wall direction and D_F
     (periodic_ref.diff_matrix) on a periodic one, both long double, s_k^2 exact.
Direction k reads face values of direction k only, on lines whose other indices are unknown nodes: the truth is formed on exactly
those lines, so edges and corners do not exist here.

Bar.  |y_i - truth_i| <= cap 2^-53 A_i with A the definition with every factor replaced by its absolute value and every line
product by the symmetrised weight lw.bound (on faces |Q||x| + |Binv||g|).  Roundings counted to first order, K the points of the
longest line and M its unknowns:
    M + 2   the end values (an M-term sum in any order, the 2 x 2 data term and the sum of the two);
    K + 8   each of the two sweeps (linewise's count: matrix entries, even/odd split, the chain, recombination, alpha, accumulate);
    1       kappa times the gradient;
    1       fl(s_k s_k), the factor the route multiplies by;
    d - 1   accumulating the directions;
    2       c x and its sum with the rest (one if contracted);
    1       f minus that (the residual);
in all 2 (K + 8) + M + d + 6, taken at the direction that maximises 2 (K + 8) + M.  The long-line route (more than 256 points) adds
its K products in turn: K roundings, inside K + 8.  The cap is a count, never tuned to a measurement."""
import numpy as np

import linewise as lw
import periodic_ref as pr

LD = np.longdouble
U53 = lw.U53


class Problem:
    """Geometry, matrices and coefficients of one operator; kappa, c: full-grid arrays (c may be a scalar)."""

    def __init__(self, sp, dims, bc, scale=None, kappa=None, c=0.0):
        self.dims = tuple(int(p) for p in dims)
        d = self.d = len(self.dims)
        self.periodic, _, self.ends = sp.bc_split(bc, d)
        self.scale = tuple(1.0 for _ in dims) if scale is None else tuple(float(s) for s in scale)
        self.M = tuple(p if per else p - 2 for p, per in zip(self.dims, self.periodic))
        self.ushape = self.M
        self.G = int(np.prod(self.M))
        self.N = int(np.prod(self.dims))
        self.inner = tuple(slice(None) if per else slice(1, -1) for per in self.periodic)
        self.D = [pr.diff_matrix(p) if per else lw.dense_D(p) for p, per in zip(self.dims, self.periodic)]
        self.Q, self.Binv = [], []
        for k in range(d):
            if self.periodic[k]:
                self.Q.append(None); self.Binv.append(None)
                continue
            e = self.ends[k]
            _, _, _, Q, _, Bi = sp.helmholtz_line_box(self.dims[k], ((e[0], e[1]), (e[2], e[3])), self.scale[k])
            self.Q.append(Q); self.Binv.append(Bi)
        mask = np.zeros(self.dims, dtype=bool)
        for k in range(d):
            if not self.periodic[k]:
                ix = [slice(None)] * d
                ix[k] = [0, self.dims[k] - 1]
                mask[tuple(ix)] = True
        self.bmask = mask
        self.NB = int(mask.sum())
        self.kappa = np.ones(self.dims) if kappa is None else np.asarray(kappa, dtype=np.float64).reshape(self.dims)
        self.c = np.broadcast_to(np.asarray(c, dtype=np.float64), self.dims) if np.ndim(c) == 0 else np.asarray(c, dtype=np.float64).reshape(self.dims)
        self.cap = max(2 * (p + 8) + m for p, m in zip(self.dims, self.M)) + d + 6

    # lines of direction k: full along k, unknown nodes elsewhere
    def _lines(self, k):
        return tuple(slice(None) if m == k else self.inner[m] for m in range(self.d))

    def g_full(self, g):
        """The compact boundary data of ONE field on the full grid (zero elsewhere)."""
        out = np.zeros(self.dims)
        if g is not None:
            out[self.bmask] = np.asarray(g, dtype=np.float64).reshape(-1)
        return out

    def extend(self, X, gf, k, T=LD, absolute=False):
        """X (unknown shape) with direction k completed by its two end values; periodic: X itself."""
        if self.periodic[k]:
            return np.abs(X) if absolute else X
        Q, Bi = self.Q[k], self.Binv[k]
        gl = gf[self._lines(k)]
        g2 = np.stack([np.take(gl, 0, axis=k), np.take(gl, self.dims[k] - 1, axis=k)], axis=0)       # (2, other unknowns)
        if absolute:
            X, g2, Q, Bi = np.abs(X), np.abs(g2), np.abs(Q), np.abs(Bi)
        Xm = np.moveaxis(X, k, 0)
        ends = np.tensordot(Q.astype(T), Xm.astype(T), axes=([1], [0])) + np.tensordot(Bi.astype(T), g2.astype(T), axes=([1], [0]))
        W = np.concatenate([ends[:1], Xm.astype(T), ends[1:]], axis=0)
        return np.moveaxis(W, 0, k)

    def extend_full(self, x, g=None, T=np.float64):
        """The full grid of ONE field as solve_full builds it: wall directions ascending, direction k on the lines whose earlier
        indices are any and whose later ones are unknown nodes -- every boundary node is set once, by the highest direction in
        which it is an end node."""
        gf = self.g_full(g)
        U = np.asarray(x, dtype=np.float64).reshape(self.ushape).astype(T)
        for k in range(self.d):
            if self.periodic[k]:
                continue
            gl = gf[tuple(slice(None) if m <= k else self.inner[m] for m in range(self.d))]
            g2 = np.stack([np.take(gl, 0, axis=k), np.take(gl, self.dims[k] - 1, axis=k)], axis=0).astype(T)
            Um = np.moveaxis(U, k, 0)
            ends = np.tensordot(self.Q[k].astype(T), Um, axes=([1], [0])) + np.tensordot(self.Binv[k].astype(T), g2, axes=([1], [0]))
            U = np.moveaxis(np.concatenate([ends[:1], Um, ends[1:]], axis=0), 0, k)
        return U

    def _restrict(self, Y, k):
        return Y if self.periodic[k] else np.take(Y, np.arange(1, self.dims[k] - 1), axis=k)

    def apply(self, x, g=None, f=None, nfields=1):
        """(truth, A) of mult (f None) or residual, long double / double, flat over the stacked fields."""
        x = np.asarray(x, dtype=np.float64).reshape((nfields,) + self.ushape)
        gs = None if g is None else np.asarray(g, dtype=np.float64).reshape(nfields, self.NB)
        fs = None if f is None else np.asarray(f, dtype=np.float64).reshape((nfields,) + self.ushape)
        cI, ts, As = self.c[self.inner], [], []
        for j in range(nfields):
            X, gf = x[j], self.g_full(None if gs is None else gs[j])
            with np.errstate(invalid="ignore", over="ignore"):
                t = cI.astype(LD) * X.astype(LD)
                A = np.abs(cI) * np.abs(X)
                for k in range(self.d):
                    kap = self.kappa[self._lines(k)]
                    s2 = LD(self.scale[k]) * LD(self.scale[k])
                    W = self.extend(X, gf, k)
                    t = t - s2 * self._restrict(lw.truth(self.D[k], kap.astype(LD) * lw.truth(self.D[k], W, k), k), k)
                    Wa = self.extend(X, gf, k, np.float64, True)
                    A = A + float(s2) * self._restrict(lw.bound(self.D[k], np.abs(kap) * lw.bound(self.D[k], Wa, k), k), k)
                if fs is not None:
                    t = fs[j].astype(LD) - t
                    A = A + np.abs(fs[j])
            ts.append(t.reshape(-1)); As.append(A.reshape(-1))
        return np.concatenate(ts), np.concatenate(As)

    def dense(self):
        """(A, lift): the G x G matrix of mult and the function g -> -(operator at g)(0), long double; tiny grids only."""
        A = np.empty((self.G, self.G), dtype=LD)
        e = np.zeros(self.G)
        for j in range(self.G):
            e[j] = 1.0
            A[:, j] = self.apply(e)[0]
            e[j] = 0.0
        return A, (lambda g: -self.apply(np.zeros(self.G), g)[0])

    # ---- the route in plain double, with the faults the host test plants ----------------------------------------------------------
    def route_double(self, x, g=None, f=None, plant=None):
        """What an IEEE double implementation of the route gives for one field: end values, D (kappa . D W) per direction with the
        factor -fl(s s), accumulated in ascending order, then c x + sum and f - that.  plant: "kappa_face" (kappa of the neighbouring
        interior node at the first face of direction 0), "wrong_q" (direction 0's end values from direction 1's Q), "s_not_squared",
        "c_unrestricted" (c read with the unknown index on the full grid)."""
        X = np.asarray(x, dtype=np.float64).reshape(self.ushape)
        gf = self.g_full(g)
        acc = None
        for k in range(self.d):
            Dk = self.D[k].astype(np.float64)
            kap = self.kappa[self._lines(k)].copy()
            if plant == "kappa_face" and k == 0:
                kap[0] = kap[1]
            saveQ = self.Q[k]
            if plant == "wrong_q" and k == 0:
                self.Q[0] = self.Q[1]
            try:
                W = self.extend(X, gf, k, np.float64)
            finally:
                self.Q[k] = saveQ
            s2 = self.scale[k] if plant == "s_not_squared" else self.scale[k] * self.scale[k]
            T = -s2 * self._restrict(lw.product_double(Dk, kap * lw.product_double(Dk, W, k), k), k)
            acc = T if acc is None else acc + T
        cI = self.c[self.inner]
        if plant == "c_unrestricted":
            cI = self.c.reshape(-1)[:self.G].reshape(self.ushape)
        y = cI * X + acc
        if f is not None:
            y = np.asarray(f, dtype=np.float64).reshape(self.ushape) - y
        return y.reshape(-1)


def nodes(P, periodic):
    """The coordinates of one direction, double: cos(i pi / (P - 1)) or -1 + 2 j / P."""
    if periodic:
        return np.asarray(pr.nodes(P), dtype=np.float64)
    i = np.arange(P)
    return np.asarray(lw._sin_half(P - 1 - 2 * i, P - 1), dtype=np.float64)


def grid(dims, periodic):
    return np.meshgrid(*[nodes(p, per) for p, per in zip(dims, periodic)], indexing="ij")


def kappa_field(dims, periodic, amp=0.9, seed=None):
    """kappa = 1 + amp prod_k sin(2 x_k + 0.3 k) (contrast (1 + amp) / (1 - amp): 19 at 0.9); seed: scaled per node by 10^+-3."""
    k = np.ones(dims)
    for j, xk in enumerate(grid(dims, periodic)):
        k = k * np.sin(2.0 * xk + 0.3 * j)
    k = 1.0 + amp * k
    if seed is not None:
        k = k * 10.0 ** np.random.default_rng(seed).integers(-3, 4, size=dims)
    return k


def c_field(dims, periodic):
    """c = 2 + cos x_0"""
    return 2.0 + np.cos(grid(dims, periodic)[0])


def node_scaled(n, seed, span=30):
    r = np.random.default_rng(seed)
    return r.standard_normal(n) * 10.0 ** r.integers(-span, span + 1, size=n)
