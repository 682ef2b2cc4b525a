"""cheb_helmholtz_line_host: the eigen-decomposition A_1 = S diag(lam) S^-1 of the spectral line operator
A_1 = -(D D)[1..n-1, 1..n-1] (csrc/diffmat.cpp: spec_line), on the host (no device), against numpy: residual, inverse,
eigenvalues, the smallest eigenvalue of -u'' on [-1, 1], the parity layout of the modes; argument errors."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge

sp = ge.load()
SIZES = (3, 4, 5, 10, 33, 34, 130, 256, 258)


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def cheb_d(P):
    """The Chebyshev collocation differentiation matrix on x_i = cos(pi i / n), float64, with the node differences taken from
    the half-angles (x_i - x_j = -2 sin((i+j) pi / 2n) sin((i-j) pi / 2n)) so that no entry loses digits to cancellation."""
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


def a1(P):
    D = cheb_d(P)
    return -(D @ D)[1:-1, 1:-1]


@pytest.mark.parametrize("P", SIZES)
def test_line_decomposition(L, P):
    S, Si, lam = sp.helmholtz_line(P)
    A = a1(P)
    M = P - 2
    assert S.shape == (M, M) and Si.shape == (M, M) and lam.shape == (M,)
    assert np.all(lam > 0)
    res = np.linalg.norm(A @ S - S * lam) / (np.linalg.norm(A) * np.linalg.norm(S))
    assert res <= 1e-12, res
    inv = np.linalg.norm(S @ Si - np.eye(M))
    assert inv <= 1e-12, inv
    ev = np.linalg.eigvals(A)
    assert np.abs(ev.imag).max() == 0.0
    ev = np.sort(ev.real)
    err = np.abs(np.sort(lam) - ev).max()
    assert err <= 1e-12 * ev.max(), (err, ev.max())
    if P >= 34:
        assert abs(lam.min() - np.pi ** 2 / 4) <= 1e-9, lam.min()
    # parity layout: columns p < ceil(M/2) even under i -> M-1-i, the rest odd; each class by ascending eigenvalue
    He = (M + 1) // 2
    R = np.arange(M)[::-1]
    assert np.array_equal(S[R, :He], S[:, :He])
    assert np.array_equal(S[R, He:], -S[:, He:])
    assert np.all(np.diff(lam[:He]) > 0) and np.all(np.diff(lam[He:][::-1]) > 0)
    # S^-1 rows carry the parity of their mode exactly (the raw-mode transforms rely on it)
    assert np.array_equal(Si[:He, R], Si[:He, :]) and np.array_equal(Si[He:, R], -Si[He:, :])


def test_line_smallest_eigenvalues(L):
    """The low modes of A_1 are those of -u'' on [-1, 1] with u(+-1) = 0: (k pi / 2)^2, resolved spectrally."""
    S, Si, lam = sp.helmholtz_line(66)
    low = np.sort(lam)[:8]
    ref = (np.arange(1, 9) * np.pi / 2) ** 2
    assert np.abs(low - ref).max() <= 1e-9 * ref.max()


def test_line_argument_errors(L):
    buf = np.empty(300 * 300)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.cheb_helmholtz_line_host(2, dp, dp, dp) == 1
    assert b"P >= 3" in L.chebhip_last_error()
    assert L.cheb_helmholtz_line_host(259, dp, dp, dp) == 4
    assert L.cheb_helmholtz_line_host(10, None, dp, dp) == 4
    assert L.cheb_helmholtz_line_host(10, dp, None, dp) == 4
    assert L.cheb_helmholtz_line_host(10, dp, dp, None) == 4
    with pytest.raises(sp.ChebhipError):
        sp.helmholtz_line(2)


def test_create_argument_errors_before_device(L):
    """cheb_helmholtz_create checks its arguments before any device use (no GPU needed); nothing is returned on error."""
    h = C.c_void_p()
    ints = lambda v: (C.c_int * len(v))(*v)
    assert L.cheb_helmholtz_create(0, ints([5]), 0.0, 1, C.byref(h)) == 3
    assert L.cheb_helmholtz_create(11, ints([5] * 11), 0.0, 1, C.byref(h)) == 3
    assert L.cheb_helmholtz_create(2, None, 0.0, 1, C.byref(h)) == 3
    assert L.cheb_helmholtz_create(2, ints([5, 5]), -1.0, 1, C.byref(h)) == 4
    assert L.cheb_helmholtz_create(2, ints([5, 5]), float("nan"), 1, C.byref(h)) == 4
    assert L.cheb_helmholtz_create(2, ints([5, 5]), float("inf"), 1, C.byref(h)) == 4
    assert L.cheb_helmholtz_create(2, ints([5, 5]), 0.0, 0, C.byref(h)) == 4
    assert L.cheb_helmholtz_create(2, ints([5, 5]), 0.0, 17, C.byref(h)) == 4
    assert L.cheb_helmholtz_create(2, ints([5, 2]), 0.0, 1, C.byref(h)) == 1
    assert L.cheb_helmholtz_create(2, ints([5, 259]), 0.0, 1, C.byref(h)) == 4
    assert L.cheb_helmholtz_create(2, ints([5, 5]), 0.0, 1, None) == 4
    assert h.value is None
    assert L.cheb_helmholtz_size(None) == -1
    assert L.cheb_helmholtz_solve(None, None, None, None) == 4
    assert L.cheb_helmholtz_destroy(None) == 4
    assert L.ell_pc_create_spectral(None, 0.0, C.byref(h)) == 4
