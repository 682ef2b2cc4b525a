"""cheb_reduce_weights_host (reduce_weights): the weight vectors of the partial contractions against the host builders they must
repeat bit for bit, against an independent long-double r(x)^T D, and on samples of T_k, whose derivative is known in closed form;
argument errors.  No device needed."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import linewise as lw
import points_ref as pref

sp = ge.load()
LD = np.longdouble
U = 2.0 ** -53
SIZES = [2, 3, 17, 64, 257, 1024]
XS = [0.3, -0.987654321, 1.0 - 2.0 ** -40, 1.25, -1.0, 0.0]


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("n", SIZES)
def test_integral_mean_node(n):
    w = sp.reduce_weights(n, "integral")
    assert (bits(w) == bits(sp.cc_weights(n))).all()
    assert (bits(sp.reduce_weights(n, "mean")) == bits(0.5 * w)).all()
    for j in sorted({0, 1, n // 2, n - 1}):
        e = np.zeros(n)
        e[j] = 1.0
        assert (bits(sp.reduce_weights(n, ("node", j))) == bits(e)).all()
        assert (bits(sp.reduce_weights(n, "node", j)) == bits(e)).all()


@pytest.mark.parametrize("n", SIZES)
def test_point_is_the_barycentric_row(n):
    for x in XS + [float("nan"), float("inf")]:
        assert (bits(sp.reduce_weights(n, ("point", x))) == bits(sp.interp_matrix(n, [x])[0])).all()
    assert np.isnan(sp.reduce_weights(n, ("point", float("nan")))).all()
    assert np.isnan(sp.reduce_weights(n, ("dpoint", float("-inf")))).all()


@pytest.mark.parametrize("n", SIZES)
def test_dnode_is_a_row_of_G(n):
    """dealias_matrix(n, "G", n) is I D formed in long double: row j of D, rounded once."""
    G = sp.dealias_matrix(n, "G", n)
    rows = range(n) if n <= 257 else sorted({0, 1, 2, n // 2, n - 2, n - 1})
    for j in rows:
        assert (bits(sp.reduce_weights(n, ("dnode", j))) == bits(G[j])).all()
    # a coordinate that is a node: the unit row times D
    xn = sp.cgl_nodes(n)
    for j in sorted({0, n // 2, n - 1}):
        assert (bits(sp.reduce_weights(n, ("dpoint", xn[j]))) == bits(G[j])).all()


@pytest.mark.parametrize("n", SIZES)
def test_dpoint_against_long_double(n):
    """|w - ref| <= U |ref| + (n + 8) 2^-63 sum_j |r_j| |D_jk|: ref = r(x)^T D from this suite's own long-double row
    (points_ref.rows_ld) and differentiation matrix (linewise.dense_D); one rounding to double, n + 8 long-double roundings."""
    D = lw.dense_D(n)
    for x in XS:
        r = pref.rows_ld(n, [x])[0]
        ref = r @ D
        mag = (np.abs(r) @ np.abs(D)).astype(np.float64)
        w = sp.reduce_weights(n, ("dpoint", x))
        err = np.abs(w.astype(LD) - ref).astype(np.float64)
        assert (err <= U * np.abs(ref).astype(np.float64) + (n + 8) * 2.0 ** -63 * mag).all(), (n, x)


@pytest.mark.parametrize("n", SIZES)
def test_derivative_of_T_k(n):
    """dnode and dpoint applied to the samples of T_k (k < n: the interpolant is T_k itself) give T_k'(x): k^2 at x = +1,
    (-1)^(k+1) k^2 at x = -1, k sin(k theta) / sin(theta) inside.  Bar: (n + 8) U sum |w_j| |T_k(x_j)| -- one rounding per weight,
    one per sample, n for the sum.  dnode takes every degree up to N.  dpoint interpolates on the DOUBLE node table, whose
    rounding (at most U |x_j| / 2 per node) moves the result by about sum_j |r_j| |T_k''(x_j)| U / 2, a term the bar does not
    count and that grows like k^4 towards the ends: it takes k <= 3, where |T_k''| <= 24 keeps that term below one unit of the
    bar, at coordinates in the middle and next to an end."""
    N = n - 1
    j = np.arange(n)
    ks = sorted({0, 1, 2, 3, N // 2, N - 1, N} & set(range(n)))
    theta_n = LD(4) * np.arctan(LD(1)) * j.astype(LD) / LD(N)
    for k in ks:
        samples = np.cos(LD(k) * theta_n)                      # T_k(x_j) = cos(k j pi / N), long double
        sd = samples.astype(np.float64)
        cases = [(("dnode", 0), LD(k) ** 2), (("dnode", N), LD(-1) ** (k + 1) * LD(k) ** 2)]
        for i in sorted({1, N // 2, N - 1} - {0, N}):
            if 0 < i < N:
                th = theta_n[i]
                cases.append((("dnode", i), LD(k) * np.sin(LD(k) * th) / np.sin(th)))
        for x in ((0.3, -0.7, -0.987654321) if k <= 3 else ()):
            th = np.arccos(LD(x))
            cases.append((("dpoint", x), LD(k) * np.sin(LD(k) * th) / np.sin(th)))
        for kind, want in cases:
            w = sp.reduce_weights(n, kind)
            got = (w.astype(LD) * sd.astype(LD)).sum()
            bar = (n + 8) * U * float((np.abs(w) * np.abs(sd)).sum())
            assert abs(float(got - want)) <= bar, (n, k, kind, float(got), float(want), bar)


def test_argument_errors():
    L = sp.lib()
    w = (C.c_double * 8)()
    assert L.cheb_reduce_weights_host(1, 0, 0.0, w) == 1                         # n < 2
    assert L.cheb_reduce_weights_host(1025, 0, 0.0, w) == 4
    assert L.cheb_reduce_weights_host(8, 0, 0.0, None) == 4
    assert L.cheb_reduce_weights_host(8, 6, 0.0, w) == 4 and b"CHEB_W" in L.chebhip_last_error()
    assert L.cheb_reduce_weights_host(8, -1, 0.0, w) == 4
    for kind in (2, 3):
        for j in (-1.0, 8.0, 2.5, float("nan")):
            assert L.cheb_reduce_weights_host(8, kind, j, w) == 4
        assert L.cheb_reduce_weights_host(8, kind, 7.0, w) == 0
    with pytest.raises(ValueError):
        sp.reduce_weights(8, "median")
    with pytest.raises(ValueError):
        sp.reduce_weights(8, "node")                                             # no index
    with pytest.raises(ValueError):
        sp.reduce_weights(8, "mean", 3)
    with pytest.raises(sp.ChebhipError):
        sp.reduce_weights(8, ("dnode", 8))
    h = C.c_void_p()
    ints = lambda v: (C.c_int * len(v))(*v)
    # checked before any device is touched
    assert L.cheb_reduce_create(2, ints([4, 4]), 1, ints([0, 0]), C.byref(h)) == 4 and b"contracted" in L.chebhip_last_error()
    assert L.cheb_reduce_create(2, ints([4, 4]), 1, None, C.byref(h)) == 4
    assert L.cheb_reduce_create(2, ints([4, 4]), 17, ints([1, 0]), C.byref(h)) == 4
    assert L.cheb_reduce_create(0, ints([4]), 1, ints([1]), C.byref(h)) == 3
    assert L.cheb_reduce_create(11, ints([2] * 11), 1, ints([1] * 11), C.byref(h)) == 3
    assert L.cheb_reduce_create(2, ints([4, 1]), 1, ints([1, 0]), C.byref(h)) == 1
    assert L.cheb_reduce_create(4, ints([1024, 1024, 1024, 2]), 1, ints([1, 0, 0, 0]), C.byref(h)) == 3
    assert h.value is None
    assert L.cheb_reduce_size(None, 0) == -1 and L.cheb_reduce_slices(None) == -1
    assert L.cheb_reduce_apply(None, None, None, None, None) == 4
    assert L.cheb_reduce_set_weights(None, 0, None) == 4 and L.cheb_reduce_destroy(None) == 4
