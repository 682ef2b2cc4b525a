"""cheb_resample_matrix_host: the Lagrange interpolation matrix between the node sets of two Chebyshev-Gauss-Lobatto grids, on
the host (no device), against a numpy long-double restatement of the barycentric formula; its exactness properties; argument
errors."""
import ctypes as C
import itertools

import numpy as np
import pytest

import __graft_entry__ as ge

sp = ge.load()
SIZES = (2, 3, 5, 16, 17, 64, 127, 256, 1024)
SETS = ("all", "interior")


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def _angles(n, nodes):
    """Grid indices of the stored nodes of a grid of n points."""
    return np.arange(1, n - 1) if nodes == "interior" else np.arange(n)


def _diff(i, m, j, n):
    """x_i - x_j for x_i = cos(pi i / m), x_j = cos(pi j / n), from the half-angles (no cancellation), long double."""
    den = np.longdouble(2 * m * n)
    pi = np.longdouble(np.pi) + np.longdouble(1.2246467991473532e-16)       # pi to long double precision
    return (-2 * np.sin(pi * (i * n + j * m) / den) * np.sin(pi * (i * n - j * m) / den)).astype(np.longdouble)


def reference(n_in, n_out, nodes_in, nodes_out):
    jin = _angles(n_in, nodes_in).astype(np.int64)
    iout = _angles(n_out, nodes_out).astype(np.int64)
    ni, no = n_in - 1, n_out - 1
    dd = _diff(jin[:, None], ni, jin[None, :], ni)
    np.fill_diagonal(dd, 1)
    w = 1 / np.prod(dd, axis=1)
    R = np.zeros((len(iout), len(jin)), dtype=np.longdouble)
    for t, i in enumerate(iout):
        hit = np.nonzero(i * ni == jin * no)[0]
        if len(hit):
            R[t, hit[0]] = 1
            continue
        c = w / _diff(i, no, jin, ni)
        R[t] = c / c.sum()
    return R


def valid(n, nodes):
    return n >= (3 if nodes == "interior" else 2)


CASES = [(a, b, s, t) for a, b in itertools.product(SIZES, SIZES) for s in SETS for t in SETS
         if valid(a, s) and valid(b, t) and (a <= 256 or b <= 256 or a == b)]


@pytest.mark.parametrize("n_in,n_out,nodes_in,nodes_out", CASES, ids=lambda v: str(v))
def test_matches_longdouble_barycentric(L, n_in, n_out, nodes_in, nodes_out):
    R = sp.resample_matrix(n_in, n_out, nodes_in, nodes_out)
    ref = reference(n_in, n_out, nodes_in, nodes_out)
    assert R.shape == ref.shape
    assert np.abs(R - ref.astype(np.float64)).max() <= 1e-15 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("n_in,n_out,nodes_in,nodes_out", CASES, ids=lambda v: str(v))
def test_reproduces_polynomials(L, n_in, n_out, nodes_in, nodes_out):
    """T_k of every degree k < (input nodes) is interpolated exactly, up to rounding: T_k(cos(pi j / m)) = cos(pi (k j mod 2m) / m),
    the angle reduced in integers so that the samples themselves are correctly rounded.  The bar is 1e-13, or 1e-15 times the
    Lebesgue constant max_t sum_s |R_ts| where that is larger: INTERIOR -> ALL extrapolates to x = +-1, and from 1022 interior nodes the
    end rows sum 1022 entries of size ~2 (the rounding of R alone then costs ~1e-13)."""
    R = sp.resample_matrix(n_in, n_out, nodes_in, nodes_out)
    T = lambda k, n, nodes: np.cos(np.pi * ((k * _angles(n, nodes)) % (2 * (n - 1))) / (n - 1))
    K = R.shape[1]
    tol = max(1e-13, 1e-15 * np.abs(R).sum(axis=1).max())
    for k in sorted({0, 1, 2, K // 2, K - 2, K - 1} & set(range(K))):
        assert np.abs(R @ T(k, n_in, nodes_in) - T(k, n_out, nodes_out)).max() <= tol, k


@pytest.mark.parametrize("n,nodes", [(n, s) for n in SIZES for s in SETS if valid(n, s)])
def test_equal_grids_give_identity(L, n, nodes):
    R = sp.resample_matrix(n, n, nodes, nodes)
    assert np.array_equal(R, np.eye(R.shape[0]))


@pytest.mark.parametrize("n_in,n_out,nodes_in,nodes_out", [(17, 33, "all", "all"), (33, 17, "all", "all"), (9, 17, "all", "interior"),
                                                           (17, 33, "interior", "interior"), (5, 257, "all", "all")])
def test_shared_nodes_are_exact_unit_rows(L, n_in, n_out, nodes_in, nodes_out):
    R = sp.resample_matrix(n_in, n_out, nodes_in, nodes_out)
    jin, iout = _angles(n_in, nodes_in), _angles(n_out, nodes_out)
    shared = 0
    for t, i in enumerate(iout):
        hit = np.nonzero(i * (n_in - 1) == jin * (n_out - 1))[0]
        if len(hit):
            e = np.zeros(len(jin)); e[hit[0]] = 1.0
            assert np.array_equal(R[t], e), (t, i)
            shared += 1
    assert shared >= min(len(jin), len(iout)) - 2


def test_argument_errors(L):
    """Checked before any device use: bad node sets / sizes give the documented codes, nothing is written."""
    buf = (C.c_double * 4)()
    assert L.cheb_resample_matrix_host(1, 0, 4, 0, buf) == 1                  # n < 2
    assert L.cheb_resample_matrix_host(4, 0, 2, 1, buf) == 1                  # INTERIOR needs n >= 3
    assert L.cheb_resample_matrix_host(4, 2, 4, 0, buf) == 4                  # no such node set
    assert L.cheb_resample_matrix_host(1025, 0, 4, 0, buf) == 4               # more than 1024 points
    assert L.cheb_resample_matrix_host(4, 0, 4, 0, None) == 4
    h = C.c_void_p()
    ints = lambda v: (C.c_int * len(v))(*v)
    assert L.cheb_resample_create(0, ints([4]), 0, ints([4]), 0, 1, C.byref(h)) == 3
    assert L.cheb_resample_create(11, ints([4] * 11), 0, ints([4] * 11), 0, 1, C.byref(h)) == 3
    assert L.cheb_resample_create(2, ints([4, 4]), 0, ints([4, 4]), 0, 5, C.byref(h)) == 4
    assert L.cheb_resample_create(2, ints([4, 4]), 0, ints([4, 4]), 0, 0, C.byref(h)) == 4
    assert L.cheb_resample_create(2, ints([4, 1]), 0, ints([4, 4]), 0, 1, C.byref(h)) == 1
    assert L.cheb_resample_create(2, ints([4, 4]), 1, ints([4, 2000]), 1, 1, C.byref(h)) == 4
    assert L.cheb_resample_create(3, ints([1024, 1024, 1024]), 0, ints([1024, 1024, 1024]), 0, 2, C.byref(h)) == 3   # 2^31 values
    assert L.cheb_resample_create(1, ints([4]), 0, ints([4]), 0, 1, None) == 4
    assert h.value is None
    assert L.cheb_resample_apply(None, None, None, None) == 4
    assert L.cheb_resample_destroy(None) == 4
    assert L.cheb_resample_size(None, 0) == -1
    with pytest.raises(ValueError):
        sp.resample_matrix(4, 4, "boundary", "all")
