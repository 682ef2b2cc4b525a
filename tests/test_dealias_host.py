"""cheb_dealias_fine_size / cheb_dealias_matrix_host on the host (no device): R is the resample matrix bit for bit; P = B_n T_m[0:n, :]
and G = R D_n agree with a numpy long-double restatement to 2^-52 of the largest entry of the row; P R = I; with m = ceil(3n/2) the
1-d product and a b' of random series are the chebmul truncations, with m - 1 they are not; argument errors."""
import ctypes as C

import numpy as np
import pytest
from numpy.polynomial import chebyshev as npc

import __graft_entry__ as ge
import dealias_ref as dr

sp = ge.load()
SIZES = (2, 3, 4, 5, 8, 17, 33, 64, 65, 129, 257, 682)
LD = np.longdouble
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def _rows_close(got, ref):
    return (np.abs(got.astype(LD) - ref).max(axis=1) <= EPS * np.abs(ref).max(axis=1)).all()


@pytest.mark.parametrize("n", SIZES)
def test_fine_size_and_R(L, n):
    m = sp.dealias_size(n)
    assert m == -(-3 * n // 2) and m - 1 > 1.5 * (n - 1) >= m - 2
    assert sp.dealias_matrix(n, "R").tobytes() == sp.resample_matrix(n, m).tobytes()
    m2 = min(2 * n, 1024)
    assert sp.dealias_matrix(n, "R", m2).tobytes() == sp.resample_matrix(n, m2).tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_P_and_G_against_longdouble(L, n):
    m = sp.dealias_size(n)
    R, P, G = dr.mats(n, m)
    assert R.shape == (m, n) and P.shape == (n, m) and G.shape == (m, n)
    # large n: the long-double reference products on every 16th row and the last two
    sub = lambda k: np.arange(k) if n <= 257 else np.unique(np.r_[0:k:16, k - 2, k - 1])
    assert _rows_close(P[sub(n)], dr.P_ld(n, m, sub(n)))
    assert _rows_close(G[sub(m)], dr.G_ld(n, m, sub(m)))
    PR = np.dot(P[sub(n)].astype(LD), np.asfortranarray(R.astype(LD)))
    assert np.abs(PR - np.eye(n, dtype=LD)[sub(n)]).max() <= 1e-14


@pytest.mark.parametrize("n", (2, 5, 64))
def test_unpadded_direction(L, n):
    assert np.array_equal(sp.dealias_matrix(n, "P", n), np.eye(n))
    assert np.array_equal(sp.dealias_matrix(n, "R", n), np.eye(n))
    assert _rows_close(sp.dealias_matrix(n, "G", n), dr.lw.dense_D(n))


def _series_case(n, m, seed):
    """(errors of the product and of a b' at m fine points, normwise relative to the chebmul truncations)."""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    x = dr.nodes(n)
    ua, ub = npc.chebval(x, a).astype(LD), npc.chebval(x, b).astype(LD)
    R, P, G = (A.astype(LD) for A in (sp.dealias_matrix(n, w, m) for w in "RPG"))
    got_mul = P @ ((R @ ua) * (R @ ub))
    got_adv = P @ ((R @ ua) * (G @ ub))
    ref_mul = npc.chebval(x, dr.trunc_mul(a, b, n))
    ref_adv = npc.chebval(x, dr.trunc_mul(a, npc.chebder(b), n))
    rel = lambda g, r: float(np.linalg.norm((g - r).astype(np.float64)) / np.linalg.norm(r))
    return rel(got_mul, ref_mul), rel(got_adv, ref_adv)


@pytest.mark.parametrize("n", SIZES)
def test_default_rule_is_the_chebmul_truncation(L, n):
    e_mul, e_adv = _series_case(n, sp.dealias_size(n), 1000 + n)
    assert e_mul <= 1e-10 and e_adv <= 1e-10, (e_mul, e_adv)


@pytest.mark.parametrize("n", (3, 5, 8, 17, 33, 65))
def test_one_point_fewer_aliases(L, n):
    """One fine point fewer: mode 2N of the product folds onto 2 (M - 1) - 2N <= N.  a b' has degree 2N - 1 only: for an odd n
    (M - 1 = 3N/2) its highest alias lands at N + 1 and it stays exact, for an even n (M - 1 = (3N - 1)/2) it lands on N."""
    e_mul, e_adv = _series_case(n, sp.dealias_size(n) - 1, 1000 + n)
    assert e_mul > 1e-3, e_mul
    if n % 2 == 0:
        assert e_adv > 1e-3, e_adv
    else:
        assert e_adv <= 1e-10, e_adv


def test_argument_errors(L):
    buf = (C.c_double * 64)()
    assert L.cheb_dealias_fine_size(1) == -1 and L.cheb_dealias_fine_size(1025) == -1
    assert L.cheb_dealias_fine_size(2) == 3 and L.cheb_dealias_fine_size(256) == 384 and L.cheb_dealias_fine_size(683) == 1025
    assert L.cheb_dealias_matrix_host(1, 3, 0, buf) == 1
    assert L.cheb_dealias_matrix_host(4, 1025, 0, None) == 4
    assert L.cheb_dealias_matrix_host(4, 3, 0, buf) == 4                       # m < n
    assert L.cheb_dealias_matrix_host(4, 6, 3, buf) == 4 and L.cheb_dealias_matrix_host(4, 6, -1, buf) == 4
    assert L.cheb_dealias_matrix_host(4, 6, 1, None) == 4
    h = C.c_void_p()
    ints = lambda v: (C.c_int * len(v))(*v)
    assert L.cheb_dealias_create(0, ints([4]), None, 1, C.byref(h)) == 3
    assert L.cheb_dealias_create(11, ints([4] * 11), None, 1, C.byref(h)) == 3
    assert L.cheb_dealias_create(2, ints([4, 1]), None, 1, C.byref(h)) == 1
    assert L.cheb_dealias_create(1, ints([683]), None, 1, C.byref(h)) == 4     # the 3/2 rule would need 1025 points
    assert b"682" in L.chebhip_last_error()
    assert L.cheb_dealias_create(2, ints([4, 4]), ints([6, 3]), 1, C.byref(h)) == 4   # a fine direction smaller than the coarse one
    assert L.cheb_dealias_create(2, ints([4, 4]), ints([6, 1025]), 1, C.byref(h)) == 4
    assert L.cheb_dealias_create(2, ints([4, 4]), None, 0, C.byref(h)) == 4
    assert L.cheb_dealias_create(2, ints([4, 4]), None, 17, C.byref(h)) == 4
    assert L.cheb_dealias_create(4, ints([682, 682, 682, 2]), None, 1, C.byref(h)) == 3
    assert L.cheb_dealias_create(1, ints([4]), None, 1, None) == 4
    assert h.value is None
    assert L.cheb_dealias_size(None) == -1 and L.cheb_dealias_work_bytes(None) == -1
    assert L.cheb_dealias_fine_dims(None, None) == 4 and L.cheb_dealias_reserve_advect(None) == 4
    assert L.cheb_dealias_multiply(None, None, None, None, None) == 4 and L.cheb_dealias_advect(None, None, None, None, None) == 4
    assert L.cheb_dealias_destroy(None) == 4
    with pytest.raises(ValueError):
        sp.dealias_matrix(4, "Q")
    with pytest.raises(sp.ChebhipError):
        sp.dealias_size(1)
    with pytest.raises(sp.ChebhipError):
        sp.dealias_matrix(4, "P", 3)
