"""cheb_points_dmatrix_host and the CPU model of the derivative rows (tests/points_deriv_ref.py), no device: the host twin against
the numpy long-double formula, rows summing to zero, the differentiation matrix's rows on nodes, plain-double restatements in two
summation orders against the entry bar cap1d(n) U a_j, planted faults a normwise check lets through and the bar does not, the
truth against the derivative of Chebyshev series, the adjoint identity of spread and eval with derivative rows, argument errors."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import points_deriv_ref as dref
import points_ref as pref
import spread_ref as sref

sp = ge.load()
LD = np.longdouble
U = pref.U
SEED = 20240229
SIZES = (2, 3, 17, 64, 257, 1024)


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def coords(n):
    """200 uniform points, the nodes, their neighbours on both sides, node (1 - 1e-9)."""
    xn = sp.cgl_nodes(n)
    rng = np.random.default_rng(SEED + n)
    return np.concatenate([rng.uniform(-1, 1, 200), xn, np.nextafter(xn, 2.0), np.nextafter(xn, -2.0), xn * (1 - 1e-9)])


@pytest.mark.parametrize("n", SIZES)
def test_twin_rounded_once(L, n):
    """One rounding of the long-double entry: U |l'|, plus 2^-60 a for the long-double sums' own error where l'_s cancels."""
    x = np.concatenate([coords(n), [0.0, 5e-324, -5e-324, 1.5, -3.0]])
    R = sp.deriv_matrix(n, x)
    want, a = dref.drows_ld(n, x)
    assert R.shape == (x.size, n) and np.isfinite(R).all()
    assert (np.abs(R.astype(LD) - want) <= U * np.abs(want) + 2.0 ** -60 * a + pref.TINY).all()
    assert (a >= np.abs(want)).all()


@pytest.mark.parametrize("n", SIZES)
def test_rows_sum_to_zero(L, n):
    """The derivative of the interpolant of 1 is 0: within 1e-19 sum a for the long-double rows (the issue's CPU check), within
    the entries' bar, cap1d U sum a, for the rounded twin."""
    x = coords(n)
    want, a = dref.drows_ld(n, x)
    sa = a.sum(axis=1)
    assert (np.abs(want.sum(axis=1)) <= 1e-19 * n * sa).all()
    R = sp.deriv_matrix(n, x).astype(LD)
    assert (np.abs(R.sum(axis=1)) <= dref.cap1d(n) * U * sa).all()


@pytest.mark.parametrize("n", SIZES)
def test_on_node_rows_are_the_differentiation_matrix(L, n):
    """Closed form on the double nodes: D_sj = (c_s / c_j) (-1)^(s + j) / (x_s - x_j), c = 2 at both ends, D_ss = -sum D_sj."""
    xn = sp.cgl_nodes(n).astype(LD)
    j = np.arange(n)
    c = np.where((j == 0) | (j == n - 1), LD(2), LD(1))
    with np.errstate(divide="ignore"):
        D = (c[:, None] / c[None, :]) * np.where((j[:, None] + j[None, :]) & 1, LD(-1), LD(1)) / (xn[:, None] - xn[None, :])
    D[j, j] = 0
    A = np.abs(D)
    A[j, j] = A.sum(axis=1)
    D[j, j] = -D.sum(axis=1)
    R = sp.deriv_matrix(n, sp.cgl_nodes(n))
    assert (np.abs(R.astype(LD) - D) <= dref.cap1d(n) * U * A).all()
    want, a = dref.drows_ld(n, sp.cgl_nodes(n))
    assert (np.abs(want - D) <= 2.0 ** -58 * A).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_plain_double_restatements_pass_the_entry_bar(n, order):
    x = coords(n)
    want, a = dref.drows_ld(n, x)
    got, _ = dref.drows(n, x, T=np.float64, total=dref._asc if order == "ascending" else dref._desc)
    ratio = np.abs(got.astype(LD) - want) / (U * a)
    print("n = %d, %s: worst entry error %.3g U a (cap1d = %.0f)" % (n, order, float(ratio.max()), dref.cap1d(n)))
    assert (np.abs(got.astype(LD) - want) <= dref.cap1d(n) * U * a).all()


@pytest.mark.parametrize("fault", ["end", "drop", "sign"])
def test_planted_faults_pass_a_normwise_check_and_fail_the_bar(fault):
    """A field whose nodes differ by 10^200 and points 1e-12 .. 4e-12 from one node s hide each fault from a normwise comparison of
    the derivatives at the points: the doubled end weight and the term missing from l'_s only meet the nodes scaled by 1e-100
    (through R the end weight also moves every entry by about d_s / 2), and the wrong sign of d_s / d_j moves an entry by
    2 d_s / d_j <= 1e-10.  The entry bar sees all three: cap1d(17) U is 3e-14."""
    n, s = 17, 8
    rng = np.random.default_rng(SEED + 5)
    xn = sp.cgl_nodes(n)
    x = xn[s] + rng.uniform(1e-12, 4e-12, 200) * np.where(rng.integers(0, 2, 200) == 1, 1.0, -1.0)
    u = rng.standard_normal(n) * 1e100
    u[[0, s]] *= 1e-200
    want, a = dref.drows_ld(n, x)
    bad, _ = dref.drows(n, x, fault=fault)
    t, tb = want @ u.astype(LD), bad @ u.astype(LD)
    normwise = float(np.sqrt(((tb - t) ** 2).sum() / (t ** 2).sum()))
    assert normwise <= 1e-10
    assert not (np.abs(bad - want) <= dref.cap1d(n) * U * a).all()
    good, _ = dref.drows(n, x, T=np.float64)
    assert (np.abs(good.astype(LD) - want) <= dref.cap1d(n) * U * a).all()


# n = 2 and 3 have exact nodes (+-1, 0): what is left there is the long-double arithmetic, 1.7 and 3 units of 2^-64
MEASURED = {2: 0.000833, 3: 0.00148, 17: 0.391, 64: 6.26, 257: 59.7, 1024: 83.1}


@pytest.mark.parametrize("n", SIZES)
def test_truth_differentiates_chebyshev_series(n):
    """u = sum_{k <= n/2} a_k T_k sampled at the double nodes in long double; the truth rows applied to it against
    sum a_k k sin(k t) / sin(t), t = arccos x.  The weights (-1)^j are those of the exact nodes, so on the rounded table the formula
    is a rational interpolant that reproduces polynomials only up to the nodes' rounding: the distance is that term, not an error
    of the rows.  Measured with this seed in units of U sum a_j |u_j| (MEASURED below); the bar is 4 times that for other seeds."""
    rng = np.random.default_rng(SEED + 6 + n)
    deg = n // 2
    a = rng.standard_normal(deg + 1).astype(LD)
    k = np.arange(deg + 1, dtype=LD)
    xn = sp.cgl_nodes(n).astype(LD)
    u = np.cos(k[None, :] * np.arccos(xn)[:, None]) @ a
    x = rng.uniform(-0.99, 0.99, 200)
    th = np.arccos(x.astype(LD))
    want = (k[None, :] * np.sin(k[None, :] * th[:, None]) / np.sin(th)[:, None]) @ a
    rows, maj = dref.drows_ld(n, x)
    got = rows @ u
    ratio = float((np.abs(got - want) / (U * (maj @ np.abs(u)))).max())
    print("n = %d: worst distance %.3g U sum a |u|" % (n, ratio))
    assert ratio <= 4 * MEASURED[n]


@pytest.mark.parametrize("dims,nf,deriv", [((5,), 2, (1,)), ((4, 6), 3, (0, 1)), ((5, 4, 3), 2, (1, 1, 0)), ((5, 4, 3), 1, (0, 0, 0))])
@pytest.mark.parametrize("delta", [False, True])
def test_adjoint_identity_of_the_truths(dims, nf, deriv, delta):
    """<spread_deriv s, u> = <s, eval_deriv u> (with delta: the grid's inner product weighted by the Clenshaw-Curtis weights) for
    the long-double truths: both sides are the same sum of npts prod(dims) terms in two orders, so they agree within
    that many roundings of 2^-64 relative to the sum of the terms' magnitudes."""
    rng = np.random.default_rng(SEED + 7)
    npts, N = 23, int(np.prod(dims))
    pts = rng.uniform(-1, 1, (npts, len(dims)))
    pts[0] = [sp.cgl_nodes(n)[1] for n in dims]
    s = rng.standard_normal((nf, npts))
    u = rng.standard_normal(nf * N)
    rows, mags = dref.rows_kinds(dims, pts, deriv)
    Lm = sref.outer(rows)
    g, _ = sref.truth(dims, s, Lm, delta)
    w = sref.weights_ld(dims) if delta else np.ones(N, dtype=LD)
    lhs = (g * w[None, :] * u.reshape(nf, N).astype(LD)).sum()
    value, _ = dref.values_ld(dims, nf, u, rows, mags)
    rhs = (s.astype(LD) * value).sum()
    size = (np.abs(s).astype(LD) @ np.abs(Lm) * np.abs(u.reshape(nf, N))).sum()
    assert abs(lhs - rhs) <= (npts * N + 8) * 2.0 ** -64 * size


def test_nan_and_inf_rows(L):
    x = np.array([0.25, np.nan, -0.5, np.inf, 0.75, -np.inf])
    R = sp.deriv_matrix(9, x)
    assert np.isnan(R[[1, 3, 5]]).all()
    assert (R[[0, 2, 4]] == sp.deriv_matrix(9, x[[0, 2, 4]])).all()


def test_argument_errors(L):
    """Checked before any device use: the extent, the count, NULL arrays, NULL handles."""
    buf = (C.c_double * 8)()
    dp = C.POINTER(C.c_double)
    assert L.cheb_points_dmatrix_host(1, 1, C.cast(buf, dp), C.cast(buf, dp)) != 0
    assert L.cheb_points_dmatrix_host(1025, 1, C.cast(buf, dp), C.cast(buf, dp)) != 0
    assert L.cheb_points_dmatrix_host(4, -1, C.cast(buf, dp), C.cast(buf, dp)) == 4
    assert L.cheb_points_dmatrix_host(4, 0, None, None) == 0
    assert L.cheb_points_dmatrix_host(4, 1, None, C.cast(buf, dp)) == 4
    one = C.c_void_p(8)                                            # never dereferenced: the checks come first
    ints = (C.c_int * 3)(0, 1, 0)
    assert L.cheb_points_drows(None, 0, one, 1, one, None) == 4
    assert L.cheb_points_eval_deriv(None, one, one, 1, ints, one, None) == 4
    assert L.cheb_points_spread_deriv(None, one, one, 1, ints, one, 0, None) == 4
    assert L.cheb_points_eval_grid_deriv(None, one, one, ints, ints, one, None) == 4
    assert L.cheb_points_eval_grad(None, one, one, 1, None, 0, one, None) == 4
    with pytest.raises(sp.ChebhipError):
        sp.deriv_matrix(1, [0.0])
