"""cheb_points_spread without a device: the float64 model of the device algorithm (tests/spread_ref.py) stays within the derived bar
of the long-double truth, the model pair eval / spread satisfies the adjoint identity within the sum of both bars, and the library
exports the entry points, checks their arguments before any device use and knows the option points_spread_pass."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import points_ref as pref
import spread_ref as ref

sp = ge.load()
LD = np.longdouble
U = ref.U
SHAPES = [((2,), 5), ((7,), 3), ((12, 9), 130), ((10, 9, 8), 130), ((258, 6), 65), ((6, 5, 34), 257), ((33, 17, 16), 64), ((5, 4, 6, 5), 67)]
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def case(dims, npts, nf=2):
    """Points with half of each direction's coordinates on nodes or one ulp off them; strengths spread over 10^+-3."""
    rng = np.random.default_rng(20240229 + npts + sum(dims))
    pts = rng.uniform(-1.0, 1.0, (npts, len(dims)))
    for k, n in enumerate(dims):
        xn = sp.cgl_nodes(n)[rng.integers(0, n, npts)]
        kind = rng.integers(0, 6, npts)                              # 0: node, 1: one ulp above, 2: one ulp below, 3..5: uniform
        pts[:, k] = np.where(kind == 0, xn, np.where(kind == 1, np.nextafter(xn, 2.0), np.where(kind == 2, np.nextafter(xn, -2.0), pts[:, k])))
    s = rng.standard_normal((nf, npts)) * 10.0 ** rng.uniform(-3.0, 3.0, (nf, npts))
    return pts, s


@pytest.mark.parametrize("dims,npts", SHAPES, ids=ids)
@pytest.mark.parametrize("delta", [False, True], ids=["plain", "delta"])
def test_model_within_bar(L, dims, npts, delta):
    pts, s = case(dims, npts)
    Lo = ref.outer(ref.rows_all_ld(dims, pts))
    t, B = ref.truth(dims, s, Lo, delta)
    g = ref.spread_model(dims, s, pts, delta)
    c = ref.cap(dims, npts, delta)
    worst = ref.worst_ratio(g, t, B, c)
    print("%s x %d points%s: worst error %.3g U B, cap %.0f" % (ids(dims), npts, " (delta)" if delta else "", worst * c, c))
    assert worst <= 1.0


@pytest.mark.parametrize("dims,npts", SHAPES, ids=ids)
def test_model_adjoint_identity(L, dims, npts):
    """<eval(u), s> = <u, spread(s)> within the sum of eval's and spread's bars (both dot products in long double)."""
    pts, s = case(dims, npts)
    nf = s.shape[0]
    u = np.random.default_rng(7 + sum(dims)).standard_normal((nf, int(np.prod(dims))))
    e = ref.eval_model(dims, u.ravel(), pts)
    g = ref.spread_model(dims, s, pts)
    lhs = (e.astype(LD) * s.astype(LD)).sum(axis=1)
    rhs = (u.astype(LD) * g.astype(LD)).sum(axis=1)
    A = np.abs(ref.outer(ref.rows_all_ld(dims, pts))).astype(np.float64)
    mag = np.einsum("fp,pi,fi->f", np.abs(s), A, np.abs(u))          # sum_p |s_p| Be_p = sum_i |u_i| Bs_i
    bar = (pref.cap(dims) + ref.cap(dims, npts)) * U * mag
    print("%s: |lhs - rhs| / bar = %.3g" % (ids(dims), float((np.abs(lhs - rhs) / bar).max())))
    assert (np.abs(lhs - rhs) <= bar).all()


def test_model_nodes_are_exact(L):
    dims = (5, 4, 3)
    idx = np.array([[0, 0, 0], [4, 3, 2], [2, 1, 1], [2, 1, 1]])
    pts = np.stack([sp.cgl_nodes(n)[idx[:, k]] for k, n in enumerate(dims)], axis=1)
    s = np.array([[1.5, -2.25, 3e100, 1e100]])
    want = np.zeros(dims)
    np.add.at(want, tuple(idx.T), s[0])
    assert (ref.spread_model(dims, s, pts) == want.ravel()).all()


def test_entry_points_and_argument_errors(L):
    assert hasattr(L, "cheb_points_spread") and hasattr(L, "cheb_points_spread_pass")
    assert L.cheb_points_spread_pass(None) == -1
    assert L.cheb_points_spread(None, None, None, 1, None, 0, None) == 4
    assert b"NULL handle" in L.chebhip_last_error()
    assert L.cheb_points_spread(None, None, None, -1, None, 0, None) == 4
    one = C.c_void_p(8)                                              # never dereferenced: the checks come first
    assert L.cheb_points_spread(None, one, one, -1, one, 0, None) == 4
    assert "cheb_points_spread" in sp.ABI_SYMBOLS and "cheb_points_spread_pass" in sp.ABI_SYMBOLS


def test_option_is_known(L):
    assert "points_spread_pass" in sp.options()
    assert sp.get_option("points_spread_pass") == 0
    sp.set_option("points_spread_pass", 48)
    try:
        assert sp.get_option("points_spread_pass") == 48
    finally:
        sp.set_option("points_spread_pass", 0)
