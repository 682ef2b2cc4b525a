"""cheb_helmholtz_line_bc_host: the spectral line operator with Neumann / Robin / mixed ends eliminated by their collocation rows
(csrc/diffmat.cpp: spec_line_bc), on the host (no device), against an independent numpy construction: the decomposition
A~ = S diag(lam) S^-1, the end-value map Q, the lift L, B_BB^-1, known smallest eigenvalues, the parity layout, and the
argument checks of the C ABI and of the Python wrapper."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge

sp = ge.load()
SIZES = (3, 4, 5, 8, 17, 64, 65, 129, 256, 258)
CONDS = {
    "neumann": "neumann",
    "robin11": (1.0, 1.0),
    "robin3_01": (3.0, 0.1),
    "dir_neu": ("dirichlet", "neumann"),
    "neu_dir": ("neumann", "dirichlet"),
    "robin21_neu": ((2.0, 1.0), "neumann"),
}


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def cheb_d(P):
    """Chebyshev differentiation matrix on x_i = cos(pi i / n) in float64, node differences from the half-angles."""
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


def ends(bc):
    return sp._bc_ends(bc)


def numpy_line(P, bc):
    """(A~, Q, L, Binv) built from a numpy D: B_row = [a0 e_0 + b0 D_0; a1 e_n - b1 D_n], Q = -B_BB^-1 B_BI,
    A~ = -(DD)_II - (DD)_IB Q, L = (DD)_IB B_BB^-1."""
    a0, b0, a1, b1 = ends(bc)
    n = P - 1
    D = cheb_d(P)
    DD = D @ D
    B = np.vstack([b0 * D[0], -b1 * D[n]])
    B[0, 0] += a0
    B[1, n] += a1
    Bbb = B[:, [0, n]]
    Binv = np.linalg.inv(Bbb)
    Q = -Binv @ B[:, 1:n]
    DDib = DD[1:n][:, [0, n]]
    A = -DD[1:n, 1:n] - DDib @ Q
    return A, Q, DDib @ Binv, Binv


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def test_dirichlet_bit_identical(L):
    for P in (3, 4, 5, 9, 10, 33, 66, 130, 131, 257, 258):
        M = P - 2
        S, Si, lam = sp.helmholtz_line(P)
        Sb, Sib, lamb, Q, Lf, Bi = sp.helmholtz_line_bc(P, "dirichlet")
        assert np.array_equal(S, Sb) and np.array_equal(Si, Sib) and np.array_equal(lam, lamb), P
        assert np.array_equal(Q, np.zeros((2, M))) and np.array_equal(Bi, np.eye(2))
        _, _, Ln, _ = numpy_line(P, "dirichlet")
        assert rel(Lf, Ln) <= 1e-13


@pytest.mark.parametrize("name", list(CONDS))
@pytest.mark.parametrize("P", SIZES)
def test_decomposition(L, P, name):
    bc = CONDS[name]
    M = P - 2
    A, Qn, Ln, Bn = numpy_line(P, bc)
    S, Si, lam, Q, Lf, Bi = sp.helmholtz_line_bc(P, bc)
    res = np.linalg.norm(A @ S - S * lam[None, :]) / max(np.linalg.norm(A) * np.linalg.norm(S), 1e-300)   # (P = 3 Neumann: A~ = 0)
    assert res <= 1e-13, res
    assert np.abs(S @ Si - np.eye(M)).max() <= 1e-13
    ev = np.sort(np.linalg.eigvals(A).real)
    assert np.abs(np.sort(lam) - ev).max() <= 1e-12 * np.abs(lam).max()
    assert np.all(lam >= 0.0)
    assert rel(Q, Qn) <= 1e-13 and rel(Lf, Ln) <= 1e-13 and rel(Bi, Bn) <= 1e-13


@pytest.mark.parametrize("P", (33, 34, 65, 130, 258))
def test_known_answers(L, P):
    M = P - 2
    S, Si, lam, *_ = sp.helmholtz_line_bc(P, "neumann")
    iz = int(np.argmin(np.abs(lam)))
    assert lam[iz] == 0.0
    col = S[:, iz]
    assert np.abs(col - col.mean()).max() <= 1e-12 * np.abs(col).max()
    assert np.sum(lam == 0.0) == 1
    _, _, lam, *_ = sp.helmholtz_line_bc(P, ("dirichlet", "neumann"))
    assert abs(lam.min() - (np.pi / 4) ** 2) <= 1e-12
    mu = 0.86                                       # mu tan(mu) = 1 (Newton)
    for _ in range(50):
        mu -= (mu * np.tan(mu) - 1.0) / (np.tan(mu) + mu / np.cos(mu) ** 2)
    _, _, lam, *_ = sp.helmholtz_line_bc(P, (1.0, 1.0))
    assert abs(lam.min() - mu * mu) <= 1e-12
    assert M == lam.size


@pytest.mark.parametrize("P", (5, 8, 17, 64, 65))
def test_parity_layout(L, P):
    M = P - 2
    m, H = M - 1, (M + 1) // 2
    for bc in ("neumann", (1.0, 1.0), (3.0, 0.1)):
        S, Si, lam, *_ = sp.helmholtz_line_bc(P, bc)
        for p in range(M):
            sg = 1.0 if p < H else -1.0             # position p < H: an even mode; M-1-q: the q-th odd one
            assert np.abs(S[::-1, p] - sg * S[:, p]).max() <= 1e-13 * np.abs(S[:, p]).max()
        assert np.all(np.diff(lam[:H]) > 0) and np.all(np.diff(lam[H:][::-1]) > 0)
    for bc in (("dirichlet", "neumann"), ((2.0, 1.0), "neumann")):
        S, Si, lam, *_ = sp.helmholtz_line_bc(P, bc)
        assert np.all(np.diff(lam) > 0)             # non-parity: ascending
        mixed = [p for p in range(M) if min(np.abs(S[::-1, p] - S[:, p]).max(), np.abs(S[::-1, p] + S[:, p]).max()) > 1e-6]
        assert mixed, "an asymmetric line has modes of no parity"


def test_argument_errors(L):
    M = 6
    buf = [np.empty(M * M), np.empty(M * M), np.empty(M), np.empty(2 * M), np.empty(2 * M), np.empty(4)]
    ptrs = [b.ctypes.data_as(C.POINTER(C.c_double)) for b in buf]
    bc = lambda *v: (C.c_double * 4)(*v)
    assert L.cheb_helmholtz_line_bc_host(8, bc(0, 1, 0, 1), *ptrs) == 0
    for bad in ((-1, 1, 0, 1), (0, -0.5, 0, 1), (0, 0, 0, 1), (1, 0, 0, 0), (float("nan"), 1, 0, 1), (0, float("inf"), 0, 1)):
        assert L.cheb_helmholtz_line_bc_host(8, bc(*bad), *ptrs) == 4, bad
    assert L.cheb_helmholtz_line_bc_host(2, bc(0, 1, 0, 1), *ptrs) == 1
    assert L.cheb_helmholtz_line_bc_host(259, bc(0, 1, 0, 1), *ptrs) == 4
    assert L.cheb_helmholtz_line_bc_host(8, None, *ptrs) == 4
    for bad in ((-1.0, 1.0), (0.0, 0.0), (float("nan"), 1.0), "robin", (1.0, 2.0, 3.0)):
        with pytest.raises((sp.ChebhipError, ValueError)):
            sp.helmholtz_line_bc(8, bad)
    with pytest.raises(sp.ChebhipError):
        sp.helmholtz_line_bc(2, "neumann")
    # create_bc refuses these before touching a device
    h = C.c_void_p()
    dims = (C.c_int * 2)(8, 8)
    good = [0.0, 1.0] * 4
    assert L.cheb_helmholtz_create_bc(2, dims, None, 0.0, 1, C.byref(h)) == 4
    assert L.cheb_helmholtz_create_bc(0, dims, (C.c_double * 8)(*good), 0.0, 1, C.byref(h)) == 3
    assert L.cheb_helmholtz_create_bc(2, dims, (C.c_double * 8)(*good), -1.0, 1, C.byref(h)) == 4
    assert L.cheb_helmholtz_create_bc(2, dims, (C.c_double * 8)(*good), 0.0, 17, C.byref(h)) == 4
    assert L.cheb_helmholtz_create_bc(2, dims, (C.c_double * 8)(*([0.0, 0.0] + good[2:])), 0.0, 1, C.byref(h)) == 4
    assert L.cheb_helmholtz_create_bc(2, (C.c_int * 2)(8, 2), (C.c_double * 8)(*good), 0.0, 1, C.byref(h)) == 1
    assert h.value is None
    # the Python wrapper: bc of the wrong length or form
    for bad in (["neumann"], ["neumann"] * 3, "neumann", [("neumann", "dirichlet", "neumann"), "neumann"], ["robin", "neumann"]):
        with pytest.raises(ValueError):
            sp.HelmholtzSolver((8, 8), bc=bad)
    assert sp.bc_array(["neumann", ("dirichlet", (2.0, 1.0))], 2) == [0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 2.0, 1.0]
