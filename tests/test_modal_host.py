"""cheb_modal_matrix_host / _weights_host / _filter_matrix_host: the Chebyshev transform matrices, Clenshaw-Curtis weights and
filter matrices of one direction, on the host (no device), against a numpy long-double restatement of their closed forms with the
same integer reduction of the cosine argument; B T = I, the exactness of the quadrature, the filters; argument errors."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge

sp = ge.load()
SIZES = (2, 3, 4, 5, 16, 17, 33, 64, 65, 129, 256, 257, 1024)
LD = np.longdouble
PI = LD(np.pi) + LD(1.2246467991473532e-16)       # pi to long double precision
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


_cache = {}


def closed_form(n):
    """(T, B, w, zero mask) in long double: cos(pi j k / N) with j k reduced modulo 2N and folded into 0..N in integers, then
    cos(pi r / N) = sin(pi (N - 2r) / 2N)."""
    if n not in _cache:
        N = n - 1
        j = np.arange(n, dtype=np.int64)
        r = (j[:, None] * j[None, :]) % (2 * N)
        r = np.where(r > N, 2 * N - r, r)
        m = N - 2 * r
        cosm = np.sign(m).astype(LD) * np.sin(PI * np.abs(m).astype(LD) / LD(2 * N))
        cosm[m == 0] = 0
        c = np.ones(n, dtype=LD); c[0] = c[N] = 2
        T = LD(2) / (LD(N) * c[:, None] * c[None, :]) * cosm
        I = np.zeros(n, dtype=LD)
        I[0::2] = LD(2) / (LD(1) - j[0::2].astype(LD) ** 2)
        _cache[n] = (T, cosm, I @ T, (2 * j[:, None] * j[None, :]) % (2 * N) == N)
    return _cache[n]


def _close(got, ref):
    return np.abs(got.astype(LD) - ref).max() <= EPS * np.abs(ref).max()


@pytest.mark.parametrize("n", SIZES)
def test_entries_against_closed_form(L, n):
    T, B, w, zero = closed_form(n)
    Td, Bd, wd = sp.modal_matrix(n, "forward"), sp.modal_matrix(n, "backward"), sp.cc_weights(n)
    assert _close(Td, T) and _close(Bd, B) and _close(wd, w)
    assert (Td[zero] == 0.0).all() and (Bd[zero] == 0.0).all()
    assert Bd[0].tolist() == [1.0] * n and (Bd[:, 0] == 1.0).all()
    assert abs(wd.astype(LD).sum() - 2) <= 4 * 2.0 ** -53


@pytest.mark.parametrize("n", SIZES)
def test_product_and_exactness(L, n):
    Td, Bd, wd = sp.modal_matrix(n, "forward").astype(LD), sp.modal_matrix(n, "backward").astype(LD), sp.cc_weights(n).astype(LD)
    assert np.abs(np.dot(Bd, np.asfortranarray(Td)) - np.eye(n, dtype=LD)).max() <= 1e-15      # (columns contiguous: numpy's long double dot)
    x = closed_form(n)[1][:, 1] if n > 2 else np.array([1, -1], dtype=LD)       # T_1(x_j) = x_j
    p = np.ones(n, dtype=LD)
    for m in range(n):                                                           # degrees 0 .. N
        exact = LD(2) / (m + 1) if m % 2 == 0 else LD(0)
        assert abs(wd @ p - exact) <= 1e-14, (n, m)
        p = p * x


@pytest.mark.parametrize("n", SIZES)
def test_filters(L, n):
    assert np.array_equal(sp.filter_matrix(n, np.ones(n)), np.eye(n))
    T, B = closed_form(n)[:2]
    # large n: the long-double reference product on every 16th row and the last two (the library's own product is the cost there)
    rows = np.arange(n) if n <= 257 else np.unique(np.r_[0:n:16, n - 2, n - 1])
    for keep in sorted({1, (n + 1) // 2, n - 1} if n <= 257 else {1, n - 1}):
        sigma = sp.sharp_filter(n, keep)
        assert sigma.tolist() == [1.0] * keep + [0.0] * (n - keep)
        F = sp.filter_matrix(n, sigma)
        assert np.abs(F).max() <= 1.0 + EPS
        assert _close(F[rows], np.dot(B[rows, :keep], np.asfortranarray(T[:keep, :])))


def test_exp_filter():
    s = sp.exp_filter(17, order=8, alpha=36.0, cutoff=5)
    k = np.arange(17.0)
    assert (s[:6] == 1.0).all() and np.allclose(s[6:], np.exp(-36.0 * ((k[6:] - 5) / 11.0) ** 8), rtol=1e-15, atol=0)
    assert s[-1] == np.exp(-36.0) and (np.diff(s) <= 0).all()
    s = sp.exp_filter(9)
    assert s[0] == 1.0 and s[-1] == np.exp(-36.0)
    T, B = (a.astype(np.float64) for a in closed_form(9)[:2])
    assert np.abs(sp.filter_matrix(9, s) - B @ np.diag(s) @ T).max() <= 1e-15


def test_argument_errors(L):
    buf = (C.c_double * 16)()
    assert L.cheb_modal_matrix_host(1, 0, buf) == 1
    assert L.cheb_modal_matrix_host(1025, 0, None) == 4
    assert L.cheb_modal_matrix_host(4, 2, buf) == 4
    assert L.cheb_modal_matrix_host(4, 0, None) == 4
    assert L.cheb_modal_weights_host(1, buf) == 1 and L.cheb_modal_weights_host(4, None) == 4
    assert L.cheb_modal_filter_matrix_host(4, None, buf) == 4 and L.cheb_modal_filter_matrix_host(0, buf, buf) == 1
    h = C.c_void_p()
    ints = lambda v: (C.c_int * len(v))(*v)
    assert L.cheb_modal_create(0, ints([4]), 1, C.byref(h)) == 3
    assert L.cheb_modal_create(11, ints([4] * 11), 1, C.byref(h)) == 3
    assert L.cheb_modal_create(2, ints([4, 1]), 1, C.byref(h)) == 1
    assert L.cheb_modal_create(2, ints([4, 1025]), 1, C.byref(h)) == 4
    assert L.cheb_modal_create(2, ints([4, 4]), 0, C.byref(h)) == 4
    assert L.cheb_modal_create(2, ints([4, 4]), 17, C.byref(h)) == 4
    assert L.cheb_modal_create(4, ints([1024, 1024, 1024, 2]), 1, C.byref(h)) == 3
    assert h.value is None
    assert L.cheb_modal_size(None) == -1 and L.cheb_modal_spectrum_size(None) == -1
    assert L.cheb_modal_forward(None, None, None, None) == 4 and L.cheb_modal_integrate(None, None, None, None, None) == 4
    with pytest.raises(ValueError):
        sp.modal_matrix(4, "sideways")
    with pytest.raises(ValueError):
        sp.filter_matrix(4, np.ones(5))
