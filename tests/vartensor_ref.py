"""The tensor mode of VarHelmholtz restated in NumPy long double (helper module of test_vartensor_host.py /
test_gpu_vartensor.py), on varhelm_ref.py and linewise.py.

Definition.  For the unknowns x and boundary data g of ONE field, the d (d + 1) / 2 full-grid fields K (diagonal first,
then the upper triangle row-major), the d fields v (or none) and c:
  1. W = the full-grid extension of x as the solve builds it (varhelm_ref.Problem.extend_full: wall directions ascending, every
     boundary node set once by the highest direction in which it is an end node), Q_k and Binv_k the library's DOUBLES;
  2. G_k = s_k D_k W on the whole grid, D the CGL matrix or D_F in long double, s_k exact;
  3. F_j = sum_k K_jk G_k and a = sum_k v_k G_k at every node;
  4. y = c x + a - sum_j s_j D_j F_j at the unknown nodes (f - that for the residual).
Unlike the scalar operator this one reads W on edges: F_j at a face node of direction j holds tangential derivatives G_k of W along
that face, and their lines end on the edge shared with a face of direction k.  Corners are never read.

Bar.  |y_i - truth_i| <= cap 2^-53 A_i, A the same evaluation with every factor replaced by its absolute value and every line
product by the symmetrised weight lw.bound.  The cap counts roundings to first order along the longest chain
    x -> edge value of W -> G_k on a face -> F_j on that face -> D_j F_j -> the sum -> c x + . -> f - .
with K the points of the longest line and M the most unknowns of a wall direction:
    w (M + 2)   the end values: an M-term sum in any order, the 2 x 2 data term and the sum of the two (varhelm_ref's count), once
                per stage of the extension the chain passes -- an edge value is the extension (direction k) of face values that
                are themselves an extension (direction j < k): w = 2 with two or more wall directions, 1 with one, 0 with none;
    K + 8       each of the two sweeps, the factor alpha = s_k and the accumulate operand inside (linewise's count);
    d           a flux term: one product and d - 1 fused multiply-adds;
    d           what the sum A goes through after a term has entered it: d - 1 later accumulations and the advective start;
    2           c x and its sum with the rest;
    1           f minus that;
in all cap = 2 (K + 8) + w (M + 2) + 2 d + 3.  With one wall direction this is 2 (K + 8) + M + 2 d + 5; the second (M + 2) is the
second stage of an edge value.  The cap is a count, never tuned to a measurement."""
import numpy as np

import linewise as lw
import varhelm_ref as vr

LD = np.longdouble
U53 = lw.U53


def tensor_order(d):
    return [(j, j) for j in range(d)] + [(j, k) for j in range(d) for k in range(j + 1, d)]


def minors_ok(K):
    """The library's test, per node: every entry finite and the leading principal minors > 0, in double.  K: (nK, *dims)."""
    K = np.asarray(K, dtype=np.float64)
    d = 2 if K.shape[0] == 3 else 3
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.all(np.isfinite(K), axis=0)
        if d == 2:
            k00, k11, k01 = K
            return ok & (k00 > 0) & (k00 * k11 - k01 * k01 > 0)
        k00, k11, k22, k01, k02, k12 = K
        det = k00 * (k11 * k22 - k12 * k12) - k01 * (k01 * k22 - k12 * k02) + k02 * (k01 * k12 - k11 * k02)
        return ok & (k00 > 0) & (k00 * k11 - k01 * k01 > 0) & (det > 0)


class TensorProblem(vr.Problem):
    """Geometry and matrices of varhelm_ref.Problem with K (nK, *dims), vel (d, *dims) or None, c (scalar or full grid)."""

    def __init__(self, sp, dims, bc, scale=None, K=None, vel=None, c=0.0):
        vr.Problem.__init__(self, sp, dims, bc, scale, None, c)
        d = self.d
        assert d in (2, 3)
        self.order = tensor_order(d)
        self.K = np.asarray(K, dtype=np.float64).reshape((len(self.order),) + self.dims)
        self.vel = None if vel is None else np.asarray(vel, dtype=np.float64).reshape((d,) + self.dims)
        self.kidx = {}
        for i, (j, k) in enumerate(self.order):
            self.kidx[(j, k)] = self.kidx[(k, j)] = i
        walls = [k for k in range(d) if not self.periodic[k]]
        self.cap = 2 * (max(self.dims) + 8) + min(2, len(walls)) * ((max(self.M[k] for k in walls) + 2) if walls else 0) + 2 * d + 3

    def kbar(self):
        t = self.K[0] + self.K[1]
        if self.d == 3:
            t = t + self.K[2]
        return t / float(self.d)

    def extend_full_abs(self, x, g=None):
        """extend_full with every factor replaced by its absolute value, double."""
        saveQ, saveB = self.Q, self.Binv
        self.Q = [None if Q is None else np.abs(Q) for Q in saveQ]
        self.Binv = [None if B is None else np.abs(B) for B in saveB]
        try:
            return self.extend_full(np.abs(np.asarray(x, dtype=np.float64)), None if g is None else np.abs(np.asarray(g, dtype=np.float64)))
        finally:
            self.Q, self.Binv = saveQ, saveB

    def apply(self, x, g=None, f=None, nfields=1):
        """(truth, A) of mult (f None) or residual, long double / double, flat over the stacked fields."""
        d = self.d
        x = np.asarray(x, dtype=np.float64).reshape((nfields,) + self.ushape)
        gs = None if g is None else np.asarray(g, dtype=np.float64).reshape(nfields, self.NB)
        fs = None if f is None else np.asarray(f, dtype=np.float64).reshape((nfields,) + self.ushape)
        cI, ts, As = self.c[self.inner], [], []
        s = [LD(v) for v in self.scale]
        for q in range(nfields):
            X, gq = x[q], None if gs is None else gs[q]
            with np.errstate(invalid="ignore", over="ignore"):
                W = self.extend_full(X, gq, LD)
                Wa = self.extend_full_abs(X, gq)
                G = [s[k] * lw.truth(self.D[k], W, k) for k in range(d)]
                Ga = [abs(self.scale[k]) * lw.bound(self.D[k], Wa, k) for k in range(d)]
                t = cI.astype(LD) * X.astype(LD)
                A = np.abs(cI) * np.abs(X)
                if self.vel is not None:
                    t = t + sum(self.vel[k].astype(LD) * G[k] for k in range(d))[self.inner]
                    A = A + sum(np.abs(self.vel[k]) * Ga[k] for k in range(d))[self.inner]
                for j in range(d):
                    F = sum(self.K[self.kidx[(j, k)]].astype(LD) * G[k] for k in range(d))
                    Fa = sum(np.abs(self.K[self.kidx[(j, k)]]) * Ga[k] for k in range(d))
                    t = t - (s[j] * lw.truth(self.D[j], F, j))[self.inner]
                    A = A + (abs(self.scale[j]) * lw.bound(self.D[j], Fa, j))[self.inner]
                if fs is not None:
                    t = fs[q].astype(LD) - t
                    A = A + np.abs(fs[q])
            ts.append(t.reshape(-1)); As.append(A.reshape(-1))
        return np.concatenate(ts), np.concatenate(As)

    # ---- an independent dense assembly (Kronecker products; tiny grids only) --------------------------------------------------------
    def _kron(self, mats):
        out = np.ones((1, 1), dtype=LD)
        for m in mats:
            out = np.kron(out, np.asarray(m, dtype=LD))
        return out

    def dense_kron(self):
        """(A, Bg): the G x G matrix of mult and the G x N matrix that takes boundary data on the full grid (g_full) to the
        operator's response to it, (operator at g)(x) = A x + Bg g_full; long double, assembled from Kronecker products of the line
        matrices -- no line product of this module or of linewise is used."""
        d, dims = self.d, self.dims
        cur = list(self.M)                                        # extents as the extension proceeds
        E = np.eye(self.G, dtype=LD)
        B = np.zeros((self.G, self.N), dtype=LD)
        for k in range(d):
            if self.periodic[k]:
                continue
            P, M = dims[k], self.M[k]
            T = np.zeros((P, M), dtype=LD)                        # [Q row 0; I; Q row 1]
            T[0], T[P - 1] = self.Q[k][0], self.Q[k][1]
            T[1:P - 1] = np.eye(M, dtype=LD)
            Tk = self._kron([np.eye(cur[m]) if m != k else T for m in range(d)])
            Z = np.zeros((P, P), dtype=LD)
            Z[0, 0], Z[0, P - 1], Z[P - 1, 0], Z[P - 1, P - 1] = self.Binv[k][0, 0], self.Binv[k][0, 1], self.Binv[k][1, 0], self.Binv[k][1, 1]
            cur[k] = P
            # the data: g_full on the grid whose directions <= k are complete and whose later ones hold the unknown nodes only
            S = self._kron([np.eye(dims[m])[slice(None) if (m <= k or self.periodic[m]) else slice(1, -1)] for m in range(d)])
            Zk = self._kron([np.eye(cur[m]) if m != k else Z for m in range(d)])
            E = np.dot(Tk, E)
            B = np.dot(Tk, B) + np.dot(Zk, S)
        Dk = [LD(self.scale[k]) * self._kron([np.eye(dims[m]) if m != k else self.D[k] for m in range(d)]) for k in range(d)]
        R = self._kron([np.eye(dims[m])[self.inner[m]] for m in range(d)])          # G x N: the unknown nodes
        L = np.zeros((self.N, self.N), dtype=LD)
        for j in range(d):
            Fj = sum(self.K[self.kidx[(j, k)]].reshape(-1, 1).astype(LD) * Dk[k] for k in range(d))
            L = L - np.dot(Dk[j], Fj)
        if self.vel is not None:
            L = L + sum(self.vel[k].reshape(-1, 1).astype(LD) * Dk[k] for k in range(d))
        RL = np.dot(R, L)
        A = np.dot(RL, E) + np.diag(self.c[self.inner].reshape(-1).astype(LD))
        return A, np.dot(RL, B)

    def dense_double(self):
        """The G x G matrix of mult in plain double for grids of a few thousand unknowns (3-D), where neither `dense` (one apply per
        column) nor `dense_kron` (N x N matrices) is affordable.  Term (j, k) is
            A[abc, ABC] = sum_pqr L0[a,p] L1[b,q] L2[c,r] C[p,q,r] R0[p,A] R1[q,B] R2[r,C],
        L_m = rows of the unknown nodes of (D_m if m == j else I), R_m = (D_m if m == k else I) T_m, T_m the extension of direction m;
        it is contracted one direction at a time (three matrix products).  T_0 x T_1 x T_2 is extend_full's sequence of stages (the
        stages act on different directions and commute), edge values included."""
        assert self.d == 3
        d, dims = 3, self.dims
        D = [self.scale[m] * self.D[m].astype(np.float64) for m in range(d)]
        T, Rw = [], []
        for m in range(d):
            if self.periodic[m]:
                T.append(np.eye(dims[m]))
            else:
                t = np.zeros((dims[m], self.M[m]))
                t[0], t[-1] = self.Q[m][0], self.Q[m][1]
                t[1:-1] = np.eye(self.M[m])
                T.append(t)
            Rw.append(np.eye(dims[m])[self.inner[m]])
        M0, M1, M2 = self.M

        def term(j, k, C, sign):
            pair = []
            for m in range(d):
                L = np.dot(Rw[m], D[m]) if m == j else Rw[m]
                R = np.dot(D[m], T[m]) if m == k else T[m]
                pair.append((L.T[:, :, None] * R[:, None, :]).reshape(dims[m], -1))       # [p, (a, A)]
            X = np.dot(pair[0].T, C.reshape(dims[0], -1)).reshape(M0 * M0, dims[1], dims[2])          # [(aA), q, r]
            X = np.einsum("xqr,qy->xyr", X, pair[1], optimize=True).reshape(-1, dims[2])              # [(aA)(bB), r]
            X = np.dot(X, pair[2]).reshape(M0, M0, M1, M1, M2, M2)                                    # [a A b B c C]
            return sign * X.transpose(0, 2, 4, 1, 3, 5).reshape(self.G, self.G)

        A = np.diag(self.c[self.inner].reshape(-1).astype(np.float64))
        for j in range(d):
            for k in range(d):
                A = A + term(j, k, self.K[self.kidx[(j, k)]], -1.0)
        if self.vel is not None:
            for k in range(d):
                A = A + term(None, k, self.vel[k], 1.0)
        return A

    # ---- the route in plain double, with the faults the host test plants ------------------------------------------------------------
    def route_double(self, x, g=None, f=None, plant=None):
        """What an IEEE double implementation of the route gives for one field.  plant: "k02_for_k12", "s_squared_cross" (the cross
        term j != k scaled by s_k s_k), "v_wrong_direction" (v_k times the gradient of direction k + 1), "k_face" (K of the
        neighbouring interior node on the first face of direction 0)."""
        d = self.d
        X = np.asarray(x, dtype=np.float64).reshape(self.ushape)
        W = self.extend_full(X, g, np.float64)
        D = [self.D[k].astype(np.float64) for k in range(d)]
        K = self.K.copy()
        if plant == "k_face":
            K[:, 0] = K[:, 1]
        if plant == "k02_for_k12":
            K[self.kidx[(1, 2)]] = K[self.kidx[(0, 2)]]
        D0 = [lw.product_double(D[k], W, k) for k in range(d)]
        G = [self.scale[k] * D0[k] for k in range(d)]
        acc = None
        if self.vel is not None:
            for k in range(d):
                term = self.vel[k] * G[(k + 1) % d if plant == "v_wrong_direction" else k]
                acc = term if acc is None else acc + term
        for j in range(d):
            F = None
            for k in range(d):
                Gk = self.scale[k] * self.scale[k] / self.scale[j] * D0[k] if (plant == "s_squared_cross" and j != k) else G[k]
                term = K[self.kidx[(j, k)]] * Gk
                F = term if F is None else F + term
            T = -self.scale[j] * lw.product_double(D[j], F, j)
            acc = T if acc is None else acc + T
        y = self.c[self.inner] * X + acc[self.inner]
        if f is not None:
            y = np.asarray(f, dtype=np.float64).reshape(self.ushape) - y
        return y.reshape(-1)


# ---- coefficients by construction -----------------------------------------------------------------------------------------------------
def rotating_tensor(dims, periodic, k=(1.0, 0.5, 2.0), amp=1.0):
    """K = R(theta(x)) diag(k_1, k_2[, k_3]) R(theta(x))^T in the order tensor_order(d), theta = amp (0.7 + sin(x_0 + 0.3) cos(0.8 x_last)).
    2-D: the plane rotation.  3-D: the rotation by theta about direction 1 (it mixes 0 and 2) after a fixed one by 0.6 about
    direction 2 (which brings in direction 1).  Positive definite with the eigenvalues k_i whatever theta is."""
    d = len(dims)
    X = vr.grid(dims, periodic)
    th = amp * (0.7 + np.sin(X[0] + 0.3) * np.cos(0.8 * X[-1]))
    c, s = np.cos(th), np.sin(th)
    one, zero = np.ones(dims), np.zeros(dims)
    if d == 2:
        R = [[c, -s], [s, c]]
    else:
        R1 = [[c, zero, -s], [zero, one, zero], [s, zero, c]]
        c2, s2 = np.cos(0.6), np.sin(0.6)
        R2 = [[c2 * one, -s2 * one, zero], [s2 * one, c2 * one, zero], [zero, zero, one]]
        R = [[sum(R1[i][m] * R2[m][j] for m in range(3)) for j in range(3)] for i in range(3)]
    return np.stack([sum(R[i][m] * k[m] * R[j][m] for m in range(d)) for i, j in tensor_order(d)])


def velocity_field(dims, periodic, amp=1.0):
    """v_k = amp cos(x_k + 0.5 k) sin(1.3 x_(k+1) + 0.2): smooth and O(1)."""
    d = len(dims)
    X = vr.grid(dims, periodic)
    return np.stack([amp * np.cos(X[k] + 0.5 * k) * np.sin(1.3 * X[(k + 1) % d] + 0.2) for k in range(d)])
