"""The deflated solve of a singular VarHelmholtz problem restated in NumPy (helper module of test_varhelm_singular_host.py,
test_gpu_varhelm_singular.py and test_gpu_project_variable.py).  Dense matrices: tiny grids only.

Definition.  A = varhelm_ref.Problem.dense() with c == 0 and every direction periodic or Neumann / Neumann; N = [z_1 .. z_q] the
null vectors of +-1 (sp.null_space: the constant, and (-1)^index in every subset of the even periodic directions), N^T N = G I;
Pi = I - N N^T / G.  The solve returns x with N^T x = 0 and Pi (b - A x) = 0: the bordered system [A N; N^T 0] [x; lam] = [b; 0].

Method.  Right-preconditioned GMRES on Pi A from Pi b, preconditioner r -> Pi H# (r / kappa), one last Pi on x.  H# is the direct
solve at kappa == 1 with its zero modes dropped, S L# S^-1 (`dropped_mode_solve`): its result differs from the bordered solve of the
kappa == 1 matrix by a null vector only (H maps their difference into span N, which meets the range of a diagonalisable H in 0
alone), so Pi H# is the leading block of that bordered inverse -- H# b itself is NOT orthogonal to N.

Bars (U = 2^-53, T = sum_depth(G) the depth of the fixed addition order of one of the projection's sums):
    bar 3   |z_j^T x| <= (T + q + 4) U sum |x_i|          T the sum, 1 the division by G, q the correction's terms and its
                                                           subtraction, 3 for sum |x| taken after the subtraction, not before
    bar 4   |x - x*| <= |B^-1_11| |Pi r| + |B^-1_12| |N^T x| + 16 U cond(B) max |x*|, from B [x - x*; lam - lam*] = [-Pi r; N^T x]
    bar 5   |defect - N^T r / G| <= (T + 2) U sum |r_i| / G   the sum, the division, the host's own rounding"""
import numpy as np

import varhelm_ref as vr

LD = np.longdouble
U = 2.0 ** -53


def sum_depth(G):
    """T: a thread's elements in turn (at most 2 ceil(G / 2^18): 512 blocks of 256 threads, pairs), the block's tree (8), the pair
    of block shares (1), the tree over them (8)."""
    return 2 * -(-int(G) // (1 << 18)) + 17


def null_matrix(sp, p):
    """N (G x q) of the problem's geometry."""
    return sp.null_space(p.dims, p.periodic).reshape(-1, p.G).T.copy()


def project(N, v, T=np.float64):
    """Pi v for one field, in T."""
    N, v = N.astype(T), np.asarray(v).astype(T)
    return v - N @ (N.T @ v) / T(N.shape[0])


def bordered(A, N):
    """B = [A N; N^T 0] in double, its inverse and its condition number."""
    G, q = N.shape
    B = np.zeros((G + q, G + q))
    B[:G, :G] = np.asarray(A, dtype=np.float64)
    B[:G, G:] = N
    B[G:, :G] = N.T
    return B, np.linalg.inv(B), np.linalg.cond(B)


def bordered_solve(A, N, b):
    """(x*, lam*) with one step of long-double refinement of NumPy's solve."""
    G, q = N.shape
    B = bordered(A, N)[0]
    rhs = np.concatenate([np.asarray(b, dtype=np.float64), np.zeros(q)])
    s = np.linalg.solve(B, rhs)
    BL = np.zeros((G + q, G + q), dtype=LD)
    BL[:G, :G] = A
    BL[:G, G:] = N
    BL[G:, :G] = N.T
    s = s + np.linalg.solve(B, (np.concatenate([np.asarray(b, dtype=LD), np.zeros(q, dtype=LD)]) - BL @ s.astype(LD)).astype(np.float64))
    return s[:G], s[G:]


def dropped_mode_solve(sp, p):
    """H#: the direct solve of the kappa == 1, c == 0 operator of the same geometry with its zero modes dropped, S L# S^-1 -- the
    function 1 / lambda (0 at lambda = 0) of the diagonalisable H, so it does not depend on the basis the eigenspaces are given in."""
    H = vr.Problem(sp, p.dims, p.bc_arg, p.scale, None, 0.0).dense()[0].astype(np.float64)
    lam, S = np.linalg.eig(H)
    inv = np.where(np.abs(lam) > 1e-9 * np.abs(lam).max(), 1.0 / np.where(lam == 0.0, 1.0, lam), 0.0)
    return ((S * inv) @ np.linalg.inv(S)).real


def problem(sp, dims, bc, scale=None, amp=0.9):
    per = sp.bc_split(bc, len(dims))[0]
    p = vr.Problem(sp, dims, bc, scale, vr.kappa_field(dims, per, amp) if amp else None, 0.0)
    p.bc_arg = bc
    return p


def deflated_gmres(A, N, Hs, kappa_u, b, rtol=1e-10, max_it=100, plant=None, x0=None):
    """The method in double, from the guess Pi x0: (x, iterations, converged, recurrence residual / |Pi b|).  plant: "ones_only" -- Pi built from the
    constant alone; "no_last_pi" -- the last projection left out."""
    A = np.asarray(A, dtype=np.float64)
    Np = N[:, :1] if plant == "ones_only" else N
    pi = lambda v: project(Np, v)
    M = lambda r: pi(Hs @ (r / kappa_u))
    pb = pi(np.asarray(b, dtype=np.float64))
    bnorm = np.linalg.norm(pb)
    xi = np.zeros_like(pb) if x0 is None else pi(np.asarray(x0, dtype=np.float64))
    r0 = pb if x0 is None else pb - pi(A @ xi)
    beta = np.linalg.norm(r0)
    V, Z = [r0 / beta], []
    H = np.zeros((max_it + 1, max_it))
    its, res = 0, beta / bnorm
    for j in range(max_it):
        Z.append(M(V[j]))
        w = pi(A @ Z[j])
        for i in range(j + 1):
            H[i, j] = V[i] @ w
            w = w - H[i, j] * V[i]
        H[j + 1, j] = np.linalg.norm(w)
        e1 = np.zeros(j + 2)
        e1[0] = beta
        y = np.linalg.lstsq(H[:j + 2, :j + 1], e1, rcond=None)[0]
        res = np.linalg.norm(e1 - H[:j + 2, :j + 1] @ y) / bnorm
        its = j + 1
        if res <= rtol or H[j + 1, j] == 0.0:
            break
        V.append(w / H[j + 1, j])
    x = xi + np.stack(Z[:its], axis=1) @ y
    if plant != "no_last_pi":
        x = pi(x)
    return x, its, res <= rtol, res


def bar3(x, G, q):
    return (sum_depth(G) + q + 4) * U * np.abs(x).sum()


def bar4(Binv, condB, N, pr, x, xstar):
    """The elementwise bound of |x - x*| for one field; pr = Pi r of the true residual."""
    G = N.shape[0]
    return np.abs(Binv[:G, :G]) @ np.abs(pr) + np.abs(Binv[:G, G:]) @ np.abs(N.T @ x) + 16.0 * U * condB * np.abs(xstar).max()


def bar5(r, G):
    return (sum_depth(G) + 2) * U * np.abs(r).sum() / G
