"""Host side of the periodic toolbox (no device): the dealiasing matrices R, P, G and the interpolation / derivative rows
of a periodic direction against the NumPy long-double restatement of periodic_toolbox_ref.py, entry by entry to 1 ulp (the bar
test_periodic_host.py holds S and D_F to); the fine-size rule 3 floor(n/2) + 1 -- exact at the default, aliased one point below;
the planted faults each check must catch; argument errors of every new entry point."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import periodic_ref as pr
import periodic_toolbox_ref as tb

sp = ge.load()
LD = np.longdouble
SIZES = (2, 3, 4, 5, 8, 9, 16, 17, 64, 255, 256)


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def fine_sizes(n):
    K = n // 2
    return sorted({m for m in (n, 3 * K, 3 * K + 1, 2 * n) if m >= n})


def _pts(n):
    """The coordinates of the row tests: random in [-3, 3], nodes and nodes +- 2, mid-points, +-1, 1 ulp beside a node and a
    mid-point."""
    rng = np.random.default_rng(100 + n)
    xn = sp.fourier_nodes(n)
    mid = xn + 1.0 / n
    return np.concatenate([rng.uniform(-3, 3, 7), xn[:4], xn[:3] + 2, xn[-2:] - 2, mid[:3], [1.0, -1.0],
                           np.nextafter(xn[:2], 2), np.nextafter(mid[:2], -2)])


@pytest.mark.parametrize("n", SIZES)
def test_R_P_G_against_longdouble(L, n):
    for m in fine_sizes(n):
        R, P, G = (sp.dealias_matrix(n, w, m, periodic=True) for w in "RPG")
        assert R.shape == (m, n) and P.shape == (n, m) and G.shape == (m, n)
        for name, got, want in (("R", R, tb.R_ld(n, m)), ("P", P, tb.P_ld(n, m)), ("G", G, tb.G_ld(n, m))):
            u = pr.ulps(got, want)
            assert u <= 1.0, (name, n, m, u)
        PR = np.dot(P.astype(LD), R.astype(LD))
        assert np.abs(PR - np.eye(n)).max() <= 1e-14


@pytest.mark.parametrize("n", SIZES)
def test_interp_and_deriv_rows_against_longdouble(L, n):
    x = _pts(n)
    for deriv, fn in ((False, sp.interp_matrix), (True, sp.deriv_matrix)):
        got = fn(n, x, periodic=True)
        assert got.shape == (x.size, n)
        u = pr.ulps(got, tb.cosine_rows(n, x, deriv))
        assert u <= 1.0, (deriv, u)
    bad = sp.interp_matrix(n, [np.nan, np.inf, -np.inf, 0.25], periodic=True)
    assert np.isnan(bad[:3]).all() and np.isfinite(bad[3]).all()
    assert np.isnan(sp.deriv_matrix(n, [np.nan, np.inf], periodic=True)).all()


def test_default_size_is_3K_plus_1(L):
    for n in range(2, 257):
        assert sp.dealias_size(n, periodic=True) == 3 * (n // 2) + 1 == L.cheb_dealias_fine_size_basis(n, 1)
        assert L.cheb_dealias_fine_size_basis(n, 0) == sp.dealias_size(n)


def _worst_cut_error(n, m, P=None):
    """Worst error over every pair of modes of the grid of P ((R u) o (R v)) against the exact cut."""
    R = sp.dealias_matrix(n, "R", m, periodic=True).astype(LD)
    P = sp.dealias_matrix(n, "P", m, periodic=True).astype(LD) if P is None else P
    K = n // 2
    x = pr.nodes(n)
    modes = [(k, "cos") for k in range(K + 1)] + [(k, "sin") for k in range(1, (n - 1) // 2 + 1)]
    worst = 0.0
    for ku, cu in modes:
        for kv, cv in modes:
            got = np.dot(P, np.dot(R, tb.mode(n, ku, cu, x)) * np.dot(R, tb.mode(n, kv, cv, x)))
            worst = max(worst, float(np.abs(got - tb.exact_cut(n, ku, cu, kv, cv)).max()))
    return worst


@pytest.mark.parametrize("n", range(2, 18))
def test_default_size_is_exact_and_one_fewer_is_not(L, n):
    m = sp.dealias_size(n, periodic=True)
    assert _worst_cut_error(n, m) <= 1e-12
    if m - 1 >= n and n > 2:
        assert _worst_cut_error(n, m - 1) > 1e-4


@pytest.mark.parametrize("n", (4, 6, 8, 12, 16))
def test_planted_cgl_size_rule_aliases(L, n):
    """ceil(3n/2) = 3K for an even n: wavenumber 2K folds onto -K."""
    assert _worst_cut_error(n, (3 * n + 1) // 2) > 1e-4


@pytest.mark.parametrize("n", (4, 8, 16))
def test_nyquist_square_and_planted_half_weight(L, n):
    m = sp.dealias_size(n, periodic=True)
    R, P = (sp.dealias_matrix(n, w, m, periodic=True).astype(LD) for w in "RP")
    u = np.where(np.arange(n) & 1, LD(-1), LD(1))
    assert np.abs(np.dot(P, np.dot(R, u) ** 2) - LD(0.5)).max() <= 1e-15
    bad = tb.P_ld(n, m, planted="half")
    assert pr.ulps(P.astype(np.float64), bad) > 1e6
    assert _worst_cut_error(n, m, bad) > 1e-4


@pytest.mark.parametrize("n", SIZES)
def test_R_at_the_coarse_nodes_is_the_identity(L, n):
    assert np.array_equal(sp.dealias_matrix(n, "R", n, periodic=True), np.eye(n))
    assert np.array_equal(sp.dealias_matrix(n, "P", n, periodic=True), np.eye(n))
    assert np.array_equal(sp.dealias_matrix(n, "R", 2 * n, periodic=True)[::2], np.eye(n))
    assert pr.ulps(sp.dealias_matrix(n, "G", n, periodic=True), pr.diff_matrix(n)) <= 1.0


@pytest.mark.parametrize("n", SIZES)
def test_rows_agree_with_the_barycentric_form(L, n):
    """The cosine sums carry an absolute error of about K terms of 2^-63 each; the barycentric form divides by a sum of
    magnitude >= 1 / Lambda.  Bar: n 2^-58 absolute."""
    x = np.random.default_rng(7 + n).uniform(-3, 3, 16)
    got = sp.interp_matrix(n, x, periodic=True)
    assert np.abs(got - tb.bary_rows(n, x)).max() <= n * 2.0 ** -58 + 2.0 ** -52
    closed, _ = tb.rows_ld(n, x)
    # (the device's closed form measures x from the DOUBLE node: x moved by at most 2^-54, times |r'| <= pi n / 2)
    assert np.abs(got - closed).max() <= n * 2.0 ** -52
    if n & 1 and n > 3:
        # planted: the even-n (cot) weights on an odd n are another function
        j = np.arange(n)
        t = tb.PI_L * (tb.wrap(x)[:, None] - ((2 * j - n).astype(LD) / LD(n))[None, :]) / LD(2)
        w = np.where(j & 1, LD(-1), LD(1))[None, :] * np.cos(t) / np.sin(t)
        assert np.abs(got - w / w.sum(axis=1)[:, None]).max() > 1e-3


@pytest.mark.parametrize("n", (2, 4, 8, 16, 64, 256))
def test_deriv_rows_at_the_nodes_are_D_F(L, n):
    """Extents whose nodes are doubles.  Bar: the cosine sums' absolute error, about 6 n 2^-64, plus the rounding of the entry."""
    x = sp.fourier_nodes(n)
    D = pr.diff_matrix(n)
    sel = np.arange(0, n, max(1, n // 32))                      # (every node up to 32 of them, every 8th of 256)
    for shift in (0.0, 2.0, -4.0):
        got = sp.deriv_matrix(n, x[sel] + shift, periodic=True)
        assert np.all(np.abs(got - D[sel]) <= 8 * n * 2.0 ** -64 + 2.0 ** -53 * np.abs(D[sel]).astype(np.float64))
    dr_, _ = tb.drows_ld(n, x)
    # (the closed form in long double: the diagonal is minus a sum of n entries, each good to 2^-63 of itself)
    assert np.all(np.abs(dr_ - D) <= 2.0 ** -62 * (1 + np.abs(D).sum(axis=1)[:, None]))
    v, _ = tb.rows_ld(n, x + 2.0)
    assert np.array_equal(v.astype(np.float64), np.eye(n))


def test_planted_textbook_second_derivative():
    """The all-periodic projection on (4, 5): phi from sum_k (D_F D_F)_k phi = div u leaves div(u - grad phi) = 0 at every node;
    the textbook D^(2), which does not annihilate the Nyquist vector, does not."""
    dims = (4, 5)
    rng = np.random.default_rng(5)
    u = rng.standard_normal((2,) + dims)
    D = [sp.fourier_diff_matrix(n) for n in dims]

    def div_after(D2):
        Lap = np.kron(D2[0], np.eye(dims[1])) + np.kron(np.eye(dims[0]), D2[1])
        div = D[0] @ u[0] + u[1] @ D[1].T
        phi = np.linalg.lstsq(Lap, div.ravel(), rcond=1e-12)[0].reshape(dims)
        out = np.stack([u[0] - D[0] @ phi, u[1] - phi @ D[1].T])
        return float(np.abs(D[0] @ out[0] + out[1] @ D[1].T).max())

    assert div_after([sp.fourier_diff_matrix(n, 2) for n in dims]) <= 1e-12
    assert div_after([pr.diff_matrix(n, 2, planted="textbook").astype(np.float64) for n in dims]) > 1e-2


def test_face_table_on_the_solver_geometry(L):
    for dims, per in (((4, 5), (1, 0)), ((4, 5), (0, 1)), ((3, 4, 5), (0, 1, 0)), ((3, 2, 4), (0, 1, 0)), ((4, 3, 3, 5), (1, 0, 1, 0))):
        got = sp.project_faces(dims, periodic=per)
        assert np.array_equal(got, tb.face_table(dims, per)), (dims, per)
        assert got.size == pr.boundary_mask(dims, per).sum()
    assert sp.project_faces((4, 5), periodic=(1, 1)).size == 0
    assert np.array_equal(sp.project_faces((4, 5), periodic=(0, 0)), sp.project_faces((4, 5)))


def test_argument_errors(L):
    ints = lambda v: (C.c_int * len(v))(*v)
    h = C.c_void_p()
    buf = (C.c_double * 4096)()
    # NULL basis
    for rc in (L.cheb_dealias_create_basis(2, ints([4, 4]), None, None, 1, C.byref(h)),
               L.cheb_project_create_basis(2, ints([4, 4]), None, None, None, 1, C.byref(h)),
               L.cheb_opfun_create_basis(2, ints([4, 4]), None, None, None, 0.0, 1, 1, C.byref(h)),
               L.cheb_points_create_basis(2, ints([4, 4]), 1, None, C.byref(h)),
               L.cheb_project_faces_basis_host(2, ints([4, 4]), None, None)):
        assert rc == 4 and b"basis is NULL" in L.chebhip_last_error()
    # a basis value that is neither CGL nor Fourier
    bad = ints([0, 2])
    bc = (C.c_double * 8)(*([1.0, 0.0] * 4))
    assert L.cheb_dealias_create_basis(2, ints([4, 4]), None, bad, 1, C.byref(h)) == 4
    assert L.cheb_project_create_basis(2, ints([4, 4]), bad, None, None, 1, C.byref(h)) == 4
    assert L.cheb_opfun_create_basis(2, ints([4, 4]), bad, bc, None, 0.0, 1, 1, C.byref(h)) == 4
    assert L.cheb_points_create_basis(2, ints([4, 4]), 1, bad, C.byref(h)) == 4
    assert L.cheb_dealias_fine_size_basis(4, 2) == -1
    assert L.cheb_dealias_matrix_basis_host(4, 7, 0, 2, buf) == 4
    # the range of a periodic direction: 2 .. 256, the limit named
    per = ints([1, 0])
    for rc in (L.cheb_dealias_create_basis(2, ints([257, 4]), None, per, 1, C.byref(h)),
               L.cheb_project_create_basis(2, ints([257, 4]), per, None, None, 1, C.byref(h)),
               L.cheb_opfun_create_basis(2, ints([257, 4]), per, bc, None, 0.0, 1, 1, C.byref(h)),
               L.cheb_points_create_basis(2, ints([257, 4]), 1, per, C.byref(h)),
               L.cheb_dealias_matrix_basis_host(257, 400, 0, 1, buf),
               L.cheb_points_fourier_matrix_host(257, 1, buf, 0, buf)):
        assert rc == 4 and b"256" in L.chebhip_last_error()
    assert L.cheb_dealias_fine_size_basis(257, 1) == -1 and L.cheb_dealias_fine_size_basis(1, 1) == -1
    for rc in (L.cheb_dealias_create_basis(2, ints([1, 4]), None, per, 1, C.byref(h)),
               L.cheb_project_create_basis(2, ints([1, 4]), per, None, None, 1, C.byref(h)),
               L.cheb_opfun_create_basis(2, ints([1, 4]), per, bc, None, 0.0, 1, 1, C.byref(h)),
               L.cheb_points_create_basis(2, ints([1, 4]), 1, per, C.byref(h)),
               L.cheb_dealias_matrix_basis_host(1, 4, 0, 1, buf),
               L.cheb_points_fourier_matrix_host(1, 1, buf, 0, buf)):
        assert rc == 1
    # a wall direction keeps its own range: 2 points are fine for a periodic direction of ChebProject, not for a wall one
    assert L.cheb_project_create_basis(2, ints([4, 2]), per, None, None, 1, C.byref(h)) == 1
    assert L.cheb_project_faces_basis_host(2, ints([2, 4]), per, ints([0] * 4)) == 0
    # bc may be NULL only when every direction is periodic
    assert L.cheb_opfun_create_basis(2, ints([4, 4]), per, None, None, 0.0, 1, 1, C.byref(h)) == 4
    assert b"bc is NULL" in L.chebhip_last_error()
    assert L.cheb_dealias_matrix_basis_host(4, 3, 0, 1, buf) == 4 and L.cheb_dealias_matrix_basis_host(4, 7, 3, 1, buf) == 4
    assert L.cheb_dealias_matrix_basis_host(4, 7, 0, 1, None) == 4
    assert L.cheb_points_fourier_matrix_host(4, 1, buf, 2, buf) == 4 and L.cheb_points_fourier_matrix_host(4, -1, buf, 0, buf) == 4
    assert L.cheb_points_fourier_matrix_host(4, 1, None, 0, buf) == 4
    assert h.value is None
    # a direction is periodic as a whole
    with pytest.raises(sp.ChebhipError):
        sp.ChebProject((4, 4), bc=[("periodic", "wall"), "wall"])
    with pytest.raises(sp.ChebhipError):
        sp.ChebOpFun((4, 4), bc=[("periodic", "dirichlet"), "dirichlet"])
    with pytest.raises(ValueError):
        sp.ChebDealias((4, 4), periodic=(True,))
    with pytest.raises(ValueError):
        sp.ChebPoints((4, 4), periodic=(True, False, True))
    with pytest.raises(sp.ChebhipError):
        sp.dealias_size(257, periodic=True)
    with pytest.raises(sp.ChebhipError):
        sp.dealias_matrix(257, "R", 400, periodic=True)
