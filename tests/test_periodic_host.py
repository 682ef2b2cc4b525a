"""Host matrices of a periodic (Fourier) direction (csrc/diffmat.cpp) against NumPy long double (periodic_ref.py); no
device.

Entries: at most 1 ulp of the double from the closed form evaluated in NumPy long double (one rounding, plus the difference of two
long-double libm evaluations, which can move a tie).  Identities: in long double on the returned doubles, with bars
C n 2^-53 |.|.  C: tests/test_helmholtz_host.py allows spec_line a residual |A S - S Lambda|_F <= 1e-12 |A|_F |S|_F at every size up
to M = 256 unknowns, which at M = 256 is 1e-12 / (256 * 2^-53) = 35.2; C = 35 is taken at EVERY n here for the residual and the
derivative checks, so the closed form is held to what the eigensolver is allowed at its largest line and to less at every smaller
one.  The inverse checks are ABSOLUTE there, |S S^-1 - I|_F <= 1e-12 whatever n, and so they are here, for S S^-1 and for T B:
min(1e-12, C n 2^-53 |I|_F), |I|_F = sqrt(n) -- the eigensolver's figure where it is the smaller one (n >= 41) and the rounding
figure below that.  Three planted faults -- the textbook second-derivative
matrix, the even-n formula at odd n, nodes with a duplicated end point -- must each fail the test named for it."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import periodic_ref as pr

sp = ge.load()
LD = np.longdouble
SIZES = (2, 3, 4, 5, 8, 9, 16, 33, 64, 127, 256)
CBAR = 35.0


@pytest.fixture(scope="module", autouse=True)
def L():
    ge.build()
    return sp.lib()


def fro(a):
    a = np.asarray(a).astype(LD)
    return np.sqrt((a * a).sum())


def inverse_bar(n):
    """|S S^-1 - I|_F, |T B - I|_F: never looser than the absolute 1e-12 of tests/test_helmholtz_host.py (module docstring)."""
    return min(LD(1e-12), LD(CBAR * n * pr.U53) * np.sqrt(LD(n)))


def bar(n, *norms):
    b = LD(CBAR * n * pr.U53)
    for v in norms:
        b = b * v
    return b


# ---- the checks, as functions of the matrices: the library's must pass, a planted fault must fail ------------------------------
def derivative_defect(n, D, x):
    """Worst |D v - v'| / bar over the modes cos / sin (pi k (x + 1)), k < n / 2, sampled at the nodes x (long double):
    v' = -+ pi k sin / cos.  (The functions are evaluated at the nodes themselves, so a wrong grid shows.)"""
    D = np.asarray(D).astype(LD)
    worst = LD(0)
    for k in range(0, (n - 1) // 2 + 1):
        a = pr.PI_L * LD(k) * (x + LD(1))
        for v, dv in ((np.cos(a), -pr.PI_L * LD(k) * np.sin(a)), (np.sin(a), pr.PI_L * LD(k) * np.cos(a))):
            if fro(v) == 0:
                continue
            if fro(D) == 0:                                        # n = 2: D_F = 0 and only the constant is below n / 2
                worst = max(worst, LD(0) if fro(dv) == 0 else LD(np.inf))
                continue
            worst = max(worst, fro(np.dot(D, v) - dv) / bar(n, fro(D), fro(v)))
    return float(worst)


def second_derivative_defect(n, D, D2):
    """|D2 - D D| / bar: the second derivative is the square of the first (laplacian = div grad)."""
    D, D2 = np.asarray(D).astype(LD), np.asarray(D2).astype(LD)
    if fro(D) == 0:
        return float(fro(D2))
    return float(fro(D2 - np.dot(D, D)) / bar(n, fro(D), fro(D)))


def nyquist_defect(n, D):
    v = np.where(np.arange(n) & 1, LD(-1), LD(1))
    D = np.asarray(D).astype(LD)
    if fro(D) == 0:
        return 0.0
    return float(fro(np.dot(D, v)) / bar(n, fro(D), fro(v)))


# ---- entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_entries_within_one_ulp(n):
    for order in (1, 2):
        u = pr.ulps(sp.fourier_diff_matrix(n, order), pr.diff_matrix(n, order))
        print("n = %d order %d: %.3f ulp" % (n, order, u))
        assert u <= 1.0, (order, u)
    S, Si, lam = sp.fourier_line(n)
    St, Sit, lamt = pr.line(n)
    for name, a, t in (("S", S, St), ("Sinv", Si, Sit), ("lam", lam, lamt)):
        u = pr.ulps(a, t)
        assert u <= 1.0, (name, u)
    S2, Si2, lam2 = sp.fourier_line(n, 0.375)
    assert np.array_equal(S2, S) and np.array_equal(Si2, Si)
    assert pr.ulps(lam2, pr.line(n, 0.375)[2]) <= 1.0
    assert pr.ulps(sp.fourier_nodes(n), pr.nodes(n)) <= 1.0
    assert sp.fourier_modes(n) == pr.modes(n)


# ---- identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_first_derivative_of_trigonometric_modes(n):
    r = derivative_defect(n, sp.fourier_diff_matrix(n), sp.fourier_nodes(n).astype(LD))
    assert r <= 1.0, r
    assert np.all(np.diag(sp.fourier_diff_matrix(n)) == 0.0)


@pytest.mark.parametrize("n", [n for n in SIZES if n % 2 == 0])
def test_nyquist_vector_is_annihilated(n):
    assert nyquist_defect(n, sp.fourier_diff_matrix(n)) <= 1.0
    assert nyquist_defect(n, sp.fourier_diff_matrix(n, 2)) <= 1.0 or n == 2


@pytest.mark.parametrize("n", SIZES)
def test_second_derivative_is_the_square(n):
    r = second_derivative_defect(n, sp.fourier_diff_matrix(n), sp.fourier_diff_matrix(n, 2))
    assert r <= 1.0, r


@pytest.mark.parametrize("n", SIZES)
def test_line_decomposition(n):
    S, Si, lam = (a.astype(LD) for a in sp.fourier_line(n))
    A = -sp.fourier_diff_matrix(n, 2).astype(LD)
    if fro(A) > 0:
        r = fro(np.dot(A, S) - S * lam[None, :]) / bar(n, fro(A), fro(S))
        assert r <= 1.0, r
    else:
        assert np.all(lam == 0)
    r = fro(np.dot(S, Si) - np.eye(n)) / inverse_bar(n)
    assert r <= 1.0, r
    assert fro(np.dot(Si, S) - np.eye(n)) <= inverse_bar(n)


@pytest.mark.parametrize("n", SIZES)
def test_parity_bit_for_bit_and_mode_order(n):
    S, Si, lam = sp.fourier_line(n)
    He = (n + 1) // 2
    R = np.arange(n)[::-1]
    assert np.array_equal(S[R, :He], S[:, :He]) and np.array_equal(S[R, He:], -S[:, He:])
    assert np.array_equal(Si[:He, R], Si[:He, :]) and np.array_equal(Si[He:, R], -Si[He:, :])
    assert np.all(np.diff(lam[:He]) > 0) and np.all(np.diff(lam[He:][::-1]) > 0)          # each block by ascending eigenvalue
    for p, (k, kind) in enumerate(sp.fourier_modes(n)):
        assert (kind != "cos") == (p >= He)
        if kind == "nyquist" or k == 0:
            assert lam[p] == 0.0 and np.signbit(lam[p]) == False                       # exactly 0.0
        else:
            assert lam[p] > 0


@pytest.mark.parametrize("n", SIZES)
def test_modal_matrices_are_inverse_and_weights_integrate_modes(n):
    T, B = sp.fourier_modal_matrix(n, "forward").astype(LD), sp.fourier_modal_matrix(n, "backward").astype(LD)
    assert fro(np.dot(T, B) - np.eye(n)) <= inverse_bar(n)
    assert fro(np.dot(B, T) - np.eye(n)) <= inverse_bar(n)
    S, Si, _ = sp.fourier_line(n)
    assert np.array_equal(S, B.astype(np.float64)) and np.array_equal(Si, T.astype(np.float64))
    w = np.full(n, np.float64(LD(2) / LD(n))).astype(LD)           # the quadrature weight of a periodic direction
    got = np.dot(w, B)
    want = np.zeros(n, dtype=LD)
    want[0] = LD(2)                                                # 2 for the constant, 0 for every other mode
    assert np.all(np.abs(got - want) <= CBAR * n * pr.U53 * np.dot(np.abs(w), np.abs(B)))
    assert T[0].astype(np.float64).tolist() == [float(np.float64(LD(1) / LD(n)))] * n        # the constant's coefficient is the mean


def test_fourier_filter_gives_pairs_one_value():
    for n in (8, 9):
        s = sp.fourier_filter(n, lambda k: 1.0 / (1 + k))
        for p, (k, kind) in enumerate(sp.fourier_modes(n)):
            assert s[p] == 1.0 / (1 + k)


# ---- planted faults: each is caught by the test named above ---------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 16, 64))
def test_planted_textbook_second_derivative_is_caught(n):
    D = sp.fourier_diff_matrix(n)
    assert second_derivative_defect(n, D, pr.diff_matrix(n, 2)) <= 1.0
    assert second_derivative_defect(n, D, pr.diff_matrix(n, 2, planted="textbook")) > 1e6
    assert nyquist_defect(n, pr.diff_matrix(n, 2, planted="textbook")) > 1e6


@pytest.mark.parametrize("n", (3, 9, 33))
def test_planted_cot_at_odd_n_is_caught(n):
    x = pr.nodes(n)
    assert derivative_defect(n, pr.diff_matrix(n), x) <= 1.0
    assert derivative_defect(n, pr.diff_matrix(n, planted="cot"), x) > 1e6
    assert pr.ulps(sp.fourier_diff_matrix(n), pr.diff_matrix(n, planted="cot")) > 1e6


@pytest.mark.parametrize("n", (4, 9, 16))
def test_planted_duplicated_end_point_is_caught(n):
    D = sp.fourier_diff_matrix(n)
    assert derivative_defect(n, D, pr.nodes(n)) <= 1.0
    assert derivative_defect(n, D, pr.nodes(n, planted=True)) > 1e6
    assert pr.ulps(sp.fourier_nodes(n), pr.nodes(n, planted=True)) > 1e6


# ---- argument errors, all before any device use ---------------------------------------------------------------------------------
def test_argument_errors(L):
    buf = (C.c_double * 4)()
    ints = lambda v: (C.c_int * len(v))(*v)
    h = C.c_void_p()
    for call in (lambda n: L.cheb_fourier_nodes_host(n, buf), lambda n: L.cheb_fourier_diff_matrix_host(n, 1, buf),
                 lambda n: L.cheb_fourier_line_host(n, 1.0, buf, buf, buf), lambda n: L.cheb_fourier_modal_matrix_host(n, 0, buf),
                 lambda n: L.cheb_fourier_modes_host(n, ints([0] * 4), ints([0] * 4))):
        assert call(257) == 4 and b"at most 256" in L.chebhip_last_error()
        assert call(1) == 1 and b"at least 2" in L.chebhip_last_error()
    assert L.cheb_fourier_diff_matrix_host(2, 3, buf) == 4
    assert L.cheb_fourier_diff_matrix_host(2, 1, None) == 4
    assert L.cheb_fourier_line_host(2, 0.0, buf, buf, buf) == 4
    assert L.cheb_fourier_modal_matrix_host(2, 2, buf) == 4
    # the _basis entry points: the basis array NULL; a periodic direction of more than 256 points names the limit
    assert L.cheb_grad_create_basis(2, ints([8, 8]), None, None, C.byref(h)) == 4 and b"basis is NULL" in L.chebhip_last_error()
    assert L.cheb_modal_create_basis(2, ints([8, 8]), 1, None, C.byref(h)) == 4 and b"basis is NULL" in L.chebhip_last_error()
    assert L.cheb_helmholtz_create_basis(2, ints([8, 8]), None, None, None, 0.0, 1, C.byref(h)) == 4 and b"basis is NULL" in L.chebhip_last_error()
    assert L.cheb_grad_create_basis(2, ints([257, 8]), None, ints([1, 0]), C.byref(h)) == 4 and b"at most 256" in L.chebhip_last_error()
    assert L.cheb_modal_create_basis(2, ints([8, 257]), 1, ints([0, 1]), C.byref(h)) == 4 and b"at most 256" in L.chebhip_last_error()
    bc = (C.c_double * 8)(1, 0, 1, 0, 1, 0, 1, 0)
    assert L.cheb_helmholtz_create_basis(2, ints([257, 8]), ints([1, 0]), bc, None, 0.0, 1, C.byref(h)) == 4
    assert b"at most 256" in L.chebhip_last_error()
    assert L.cheb_helmholtz_create_basis(2, ints([8, 8]), ints([1, 2]), bc, None, 0.0, 1, C.byref(h)) == 4
    assert L.cheb_helmholtz_create_basis(2, ints([8, 8]), ints([1, 0]), None, None, 0.0, 1, C.byref(h)) == 4       # a wall needs its bc
    assert L.cheb_grad_create_basis(1, ints([8]), None, ints([2]), C.byref(h)) == 4
    assert h.value is None
    # a pair with one periodic end is refused
    with pytest.raises(sp.ChebhipError) as e:
        sp.HelmholtzSolver((8, 8), bc=[("periodic", "dirichlet"), "dirichlet"])
    assert e.value.code == 4 and "periodic" in str(e.value)
