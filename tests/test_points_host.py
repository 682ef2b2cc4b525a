"""cheb_nodes_host / cheb_points_matrix_host: the CGL node table and the barycentric interpolation rows of arbitrary coordinates,
on the host (no device), against the numpy long-double restatement of tests/points_ref.py: entries rounded once, row sums, exact
unit rows on nodes, finite rows next to nodes and at denormal coordinates, NaN isolation; argument errors of the whole cheb_points_*
family, which are checked before any device use."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import points_ref as ref

sp = ge.load()
SIZES = (2, 3, 5, 33, 256, 257, 1024)
LD = np.longdouble
U = ref.U
PI = LD(np.pi) + LD(1.2246467991473532e-16)       # pi to long double precision


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def coords(n):
    """Uniform points, the nodes, their neighbours on both sides, 0, the smallest denormal, the ends."""
    xn = sp.cgl_nodes(n)
    rng = np.random.default_rng(20240229 + n)
    return np.concatenate([rng.uniform(-1, 1, 40), xn, np.nextafter(xn, 2.0), np.nextafter(xn, -2.0), [0.0, 5e-324, -5e-324, 1.0, -1.0]])


@pytest.mark.parametrize("n", SIZES)
def test_nodes(L, n):
    x = sp.cgl_nodes(n)
    N = n - 1
    m = N - 2 * np.arange(n)
    want = np.sign(m).astype(LD) * np.sin(PI * np.abs(m).astype(LD) / LD(2 * N))
    assert (np.abs(x.astype(LD) - want) <= np.spacing(np.abs(x))).all()
    assert x[0] == 1.0 and x[N] == -1.0
    assert (x == -x[::-1]).all()
    if n % 2:
        assert x[N // 2] == 0.0 and not np.signbit(x[N // 2])
    assert (np.diff(x) < 0).all()


@pytest.mark.parametrize("n", SIZES)
def test_rows_rounded_once(L, n):
    x = np.concatenate([coords(n), [1.5, -3.0, 10.0]])             # the last three: extrapolation, by the same formula
    R = sp.interp_matrix(n, x)
    want = ref.rows_ld(n, x)
    assert np.isfinite(R).all()
    assert (np.abs(R.astype(LD) - want) <= U * np.abs(want) + ref.TINY).all()


@pytest.mark.parametrize("n", SIZES)
def test_row_sums_and_unit_rows(L, n):
    x = coords(n)
    R = sp.interp_matrix(n, x)
    assert np.isfinite(R).all()                                    # next to nodes, at 5e-324, at +-1
    sums = R.astype(LD).sum(axis=1)
    assert (np.abs(sums - 1) <= (n + 2) * U).all()
    xn = sp.cgl_nodes(n)
    E = sp.interp_matrix(n, xn)
    assert (E == np.eye(n)).all() and not np.signbit(E).any()
    if n % 2:                                                      # 5e-324 is not the middle node 0: its row is not the unit row's bits
        r = sp.interp_matrix(n, [5e-324])[0]
        assert r[(n - 1) // 2] == 1.0 and np.isfinite(r).all()


@pytest.mark.parametrize("n", SIZES)
def test_nan_and_inf_rows(L, n):
    x = np.array([0.25, np.nan, -0.5, np.inf, 0.75, -np.inf])
    R = sp.interp_matrix(n, x)
    assert np.isnan(R[[1, 3, 5]]).all()
    assert (R[[0, 2, 4]] == sp.interp_matrix(n, x[[0, 2, 4]])).all()


def test_argument_errors(L):
    buf = (C.c_double * 8)()
    h = C.c_void_p()
    ints = lambda v: (C.c_int * len(v))(*v)
    assert L.cheb_nodes_host(1, buf) == 1
    assert b"must be >= 2" in L.chebhip_last_error()
    assert L.cheb_nodes_host(1025, buf) == 4
    assert L.cheb_nodes_host(4, None) == 4
    assert L.cheb_points_matrix_host(1, 1, buf, buf) == 1
    assert L.cheb_points_matrix_host(1025, 1, buf, buf) == 4
    assert L.cheb_points_matrix_host(4, -1, buf, buf) == 4
    assert L.cheb_points_matrix_host(4, 1, None, buf) == 4
    assert L.cheb_points_matrix_host(4, 1, buf, None) == 4
    assert L.cheb_points_matrix_host(4, 0, None, None) == 0
    assert L.cheb_points_create(0, ints([4]), 1, C.byref(h)) == 3
    assert L.cheb_points_create(11, ints([4] * 11), 1, C.byref(h)) == 3
    assert L.cheb_points_create(2, None, 1, C.byref(h)) == 3
    assert L.cheb_points_create(2, ints([4, 4]), 0, C.byref(h)) == 4
    assert L.cheb_points_create(2, ints([4, 4]), 17, C.byref(h)) == 4
    assert L.cheb_points_create(2, ints([4, 1]), 1, C.byref(h)) == 1
    assert L.cheb_points_create(2, ints([4, 1025]), 1, C.byref(h)) == 4
    assert L.cheb_points_create(4, ints([1024, 1024, 1024, 2]), 1, C.byref(h)) == 3
    assert b"2^31" in L.chebhip_last_error()
    assert L.cheb_points_create(2, ints([4, 4]), 1, None) == 4
    assert h.value is None
    assert L.cheb_points_destroy(None) == 4
    assert L.cheb_points_chunk(None) == -1
    assert L.cheb_points_rows(None, 0, None, 1, None, None) == 4
    assert L.cheb_points_eval(None, None, None, 1, None, None) == 4
    assert L.cheb_points_grid_reserve(None, ints([1])) == 4
    assert L.cheb_points_eval_grid(None, None, None, ints([1]), None, None) == 4


def test_python_argument_errors(L):
    with pytest.raises(sp.ChebhipError) as e:
        sp.cgl_nodes(1)
    assert e.value.code == 1
    with pytest.raises(sp.ChebhipError) as e:
        sp.interp_matrix(1025, [0.0])
    assert e.value.code == 4
    assert sp.interp_matrix(7, []).shape == (0, 7)


def test_no_cpu_fallback(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    assert L.cheb_points_create(2, (C.c_int * 2)(8, 8), 1, C.byref(h)) == 5 and h.value is None
    assert b"no CPU fallback" in L.chebhip_last_error()
    with pytest.raises(sp.ChebhipError):
        sp.ChebPoints((8, 8))
