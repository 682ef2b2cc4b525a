"""ChebOpFun on the CPU: the host twin of the weight functions against mpmath, the identities of the phi functions,
the float64 numpy model against the long-double one within the bars of opfun_ref.py, operator identities in the model, and the
argument errors of every entry that needs no device."""
import ctypes as C

import mpmath
import numpy as np
import pytest

import opfun_ref as R

sp = R.sp
mpmath.mp.dps = 50

ERR_ARG = 4


def mp_phi(k, z):
    """phi_k(z) at 50 digits: the series where the recurrence would cancel."""
    z = mpmath.mpf(z)
    if z == 0:
        return 1 / mpmath.factorial(k)
    if abs(z) < 1:
        return mpmath.nsum(lambda j: z ** j / mpmath.factorial(j + k), [0, mpmath.inf])
    p = mpmath.expm1(z) / z
    for j in range(1, k):
        p = (p - 1 / mpmath.factorial(j)) / z
    return p


def mp_weight(kind, tau, par, s):
    s, tau, par = mpmath.mpf(float(s)), mpmath.mpf(float(tau)), mpmath.mpf(float(par))
    z = -tau * s
    if kind == "one":
        return mpmath.mpf(1)
    if kind == "inv":
        return 1 / s if s != 0 else mpmath.mpf(0)
    if kind == "res":
        den = par + tau * s
        return 1 / den if den != 0 else mpmath.mpf(0)
    if kind == "exp":
        return mpmath.exp(z)
    if kind == "pow":
        return (mpmath.mpf(1) if par == 0 else mpmath.mpf(0)) if s == 0 else s ** par
    return mp_phi(int(kind[3]), z)


def ulps(w, exact):
    """|w - exact| in units of the spacing of doubles at exact."""
    e = float(exact)
    return float(abs(mpmath.mpf(float(w)) - exact) / mpmath.mpf(float(np.spacing(abs(e)) if e != 0 else np.spacing(0.0))))


Z = np.concatenate([np.logspace(-30, np.log10(800.0), 2000), [0.0, 744.0, 744.44, 745.0, 745.13, 745.2, 746.0, 2.0, 1.0]])


@pytest.mark.parametrize("kind,tau,par", [("one", 0, 0), ("inv", 0, 0), ("res", 1.0, 1.0), ("res", 0.25, 3.0), ("exp", 1.0, 0),
                                           ("exp", 0.0, 0), ("phi1", 1.0, 0), ("phi2", 1.0, 0), ("phi3", 1.0, 0), ("phi2", 0.0, 0),
                                           ("pow", 0, 1.0), ("pow", 0, 0.5), ("pow", 0, -0.5), ("pow", 0, 2.0), ("pow", 0, 0.0)])
def test_weight_twin_against_mpmath(kind, tau, par):
    w = sp.opfun_weight(kind, tau, par, Z)
    worst = max(ulps(wi, mp_weight(kind, tau, par, zi)) for wi, zi in zip(w, Z))
    assert worst <= 1.0, "%s: %.3f ulp" % (kind, worst)


def test_weight_twin_special_values():
    assert sp.opfun_weight("inv", 0, 0, 0.0) == 0.0
    assert sp.opfun_weight("res", 2.0, -4.0, 2.0) == 0.0                    # p + tau s == 0
    assert sp.opfun_weight("exp", 3.0, 0, 0.0) == 1.0
    assert [sp.opfun_weight("phi%d" % k, 3.0, 0, 0.0) for k in (1, 2, 3)] == [1.0, 0.5, 1.0 / 6.0]
    assert sp.opfun_weight("pow", 0, 0.5, 0.0) == 0.0 and sp.opfun_weight("pow", 0, -1.0, 0.0) == 0.0
    assert sp.opfun_weight("pow", 0, 0.0, 0.0) == 1.0
    assert np.isnan(sp.opfun_weight("pow", 0, 2.0, -1.0)) and np.isnan(sp.opfun_weight("pow", 0, 0.5, -1.0))
    assert sp.opfun_weight("exp", 1.0, 0, 800.0) == 0.0 and 0.0 < sp.opfun_weight("exp", 1.0, 0, 745.0) < 2.0 ** -1022
    w = sp.opfun_weight("exp", 0.5, 0, np.ones((2, 3)))
    assert w.shape == (2, 3) and np.all(w == np.exp(-0.5))


def test_phi_recurrence_in_twin():
    """phi_k(z) = z phi_{k+1}(z) + 1/k!: each side's roundings, 3 U of the terms' magnitudes."""
    for tau in (1.0, 1e-3):
        z = -tau * Z
        f = [sp.opfun_weight("exp", tau, 0, Z)] + [sp.opfun_weight("phi%d" % k, tau, 0, Z) for k in (1, 2, 3)]
        fact = [1.0, 1.0, 0.5]
        for k in range(3):
            lhs = f[k].astype(R.LD)
            rhs = z.astype(R.LD) * f[k + 1].astype(R.LD) + R.LD(fact[k])
            bar = 3 * R.U * (np.abs(f[k]) + np.abs(z * f[k + 1]) + fact[k])
            assert np.all(np.abs(lhs - rhs) <= bar), "phi_%d" % k


SHAPES = [((10, 9, 8), None, None), ((34, 18, 10), None, None), ((130, 6), None, None), ((258, 6), None, None),
          ((20, 12, 9), ("neumann", ("dirichlet", "neumann"), (1.0, 0.5)), None),
          ((12, 9), ("neumann", "neumann"), (2.0, 0.5))]
KIND_ARGS = {"one": (0.0, 0.0), "inv": (0.0, 0.0), "res": (0.02, 1.5), "exp": (0.01, 0.0), "phi1": (0.01, 0.0), "phi2": (0.01, 0.0),
             "phi3": (0.01, 0.0), "pow": (0.0, 0.5)}


@pytest.mark.parametrize("dims,bc,scale", SHAPES)
def test_float64_model_within_bars(dims, bc, scale):
    rng = np.random.default_rng(7)
    ln = R.lines(dims, bc, scale)
    G = int(np.prod([n - 2 for n in dims]))
    x = rng.standard_normal((1, G))
    for kind in R.KINDS:
        tau, par = KIND_ARGS[kind]
        terms = [(0, 0, kind, 1.0, tau, par)]
        y, bar = R.model(dims, terms, x, 1, sigma=0.5, ln=ln)
        y64, _ = R.model(dims, terms, x, 1, sigma=0.5, ln=ln, prec=np.float64)
        R.check(y64, y, bar, "%s %s" % (dims, kind))


def test_float64_model_mixing():
    dims, rng = (10, 9, 8), np.random.default_rng(8)
    x = rng.standard_normal((3, 8 * 7 * 6))
    terms = [(0, 0, "exp", 1.0, 0.01, 0), (0, 1, "phi1", 0.01, 0.01, 0), (1, 2, "inv", -2.0, 0, 0), (1, 0, "exp", 0.5, 0.01, 0),
             (0, 2, "res", 3.0, 0.1, 1.0)]
    y, bar = R.model(dims, terms, x, 2)
    y64, _ = R.model(dims, terms, x, 2, prec=np.float64)
    R.check(y64, y, bar, "mixing")
    one = sum(R.model(dims, [(0, i, k, c, t, p)], x, 1)[0] for (o, i, k, c, t, p) in terms if o == 0)
    assert np.all(np.abs(one[0] - y[0]) <= bar[0])


@pytest.mark.parametrize("dims,bc", [((10, 9, 8), None), ((20, 12, 9), ("neumann", ("dirichlet", "neumann"), (1.0, 0.5)))])
def test_semigroup_and_phi1_identity(dims, bc):
    """e^(-t1 B) e^(-t2 B) = e^(-(t1 + t2) B) and phi_1(-t B) t B x = (I - e^(-t B)) x in the model.  Mode by mode the two sides
    differ by the weights' relative errors, (K + kappa) U each, so the fields differ by at most that through |S| .. |S^-1| |x|."""
    rng = np.random.default_rng(9)
    ln = R.lines(dims, bc)
    s = R.eigen_sum(ln)
    x = rng.standard_normal((1, s.size))
    t1, t2 = 0.003, 0.0045
    w1, w2, w12 = (sp.opfun_weight("exp", t, 0, s) for t in (t1, t2, t1 + t2))
    lhs = R.modal_apply(ln, w2, R.modal_apply(ln, w1, x))
    rhs = R.modal_apply(ln, w12, x)
    K = R.K["exp"]
    rel = (3 * K + 2 + 2 * (t1 + t2) * s) * R.U                           # three weights, the product, the sum t1 + t2
    bar = R.modal_bound(ln, np.abs(w12) * rel, x) + 2.0 ** -60 * R.modal_bound(ln, np.abs(w12), x) * sum(dims)
    assert np.all(np.abs(lhs - rhs) <= bar)
    t = 0.004
    p1, e = sp.opfun_weight("phi1", t, 0, s), sp.opfun_weight("exp", t, 0, s)
    lhs = R.modal_apply(ln, p1.astype(R.LD) * (R.LD(t) * s.astype(R.LD)), x)
    rhs = x.astype(R.LD) - R.modal_apply(ln, e, x)
    bar = R.modal_bound(ln, (R.K["phi1"] * np.abs(p1 * t * s) + (R.K["exp"] + t * s) * np.abs(e)) * R.U, x)
    bar += 2.0 ** -60 * sum(dims) * R.modal_bound(ln, np.ones_like(s), x)  # the long-double products themselves
    assert np.all(np.abs(lhs - rhs) <= bar)


def test_argument_errors_without_device():
    L = sp.lib()
    w = C.c_double()
    for kind, tau, par in ((3, -1.0, 0.0), (4, -1e-300, 0.0), (5, float("nan"), 0.0), (6, float("inf"), 0.0), (3, float("nan"), 0.0),
                           (2, float("nan"), 1.0), (2, 1.0, float("inf")), (7, 0.0, float("nan")), (8, 0.0, 0.0), (-1, 0.0, 0.0)):
        assert L.cheb_opfun_weight_host(kind, tau, par, 1.0, C.byref(w)) == ERR_ARG, (kind, tau, par)
        assert L.cheb_opfun_eval(kind, tau, par, None, 0, None, None) == ERR_ARG, (kind, tau, par)
    assert L.cheb_opfun_weight_host(3, 1.0, 0.0, 1.0, None) == ERR_ARG
    with pytest.raises(ValueError):
        sp.opfun_weight("sinh", 1.0, 0, 1.0)
    with pytest.raises(sp.ChebhipError):
        sp.opfun_weight("exp", -1.0, 0, np.ones(3))
    # what a kind does not read is not checked
    assert L.cheb_opfun_weight_host(1, float("nan"), float("nan"), 2.0, C.byref(w)) == 0 and w.value == 0.5
    good = (0, 0, "exp", 1.0, 0.1, 0.0)
    sp.opfun_check_terms(2, 3, [good, (2, 1, "pow", -1.0, 0.0, 0.5)])
    sp.opfun_check_terms(1, 1, [])
    sp.opfun_check_terms(1, 1, [good] * 32)
    for nin, nout, terms in ((1, 1, [good] * 33), (1, 1, [(1, 0, "exp", 1.0, 0.1, 0)]), (1, 1, [(-1, 0, "exp", 1.0, 0.1, 0)]),
                             (2, 1, [(0, 2, "exp", 1.0, 0.1, 0)]), (2, 1, [(0, -1, "exp", 1.0, 0.1, 0)]),
                             (1, 1, [(0, 0, "exp", 1.0, -0.1, 0)]), (1, 1, [(0, 0, "exp", float("nan"), 0.1, 0)]),
                             (1, 1, [(0, 0, 9, 1.0, 0.1, 0)]), (0, 1, []), (17, 1, []), (1, 0, []), (1, 17, [])):
        with pytest.raises(sp.ChebhipError) as e:
            sp.opfun_check_terms(nin, nout, terms)
        assert e.value.code == ERR_ARG
    h = C.c_void_p()
    ints = (C.c_int * 2)(6, 5)
    for nin, nout in ((0, 1), (17, 1), (1, 0), (1, 17)):
        assert L.cheb_opfun_create(2, ints, None, None, 0.0, nin, nout, C.byref(h)) == ERR_ARG
    sc = (C.c_double * 2)(1.0, 2.0)
    assert L.cheb_opfun_create(2, ints, None, sc, 0.0, 1, 1, C.byref(h)) == ERR_ARG          # scale without bc
    assert L.cheb_opfun_create(2, ints, None, None, 0.0, 1, 1, None) == ERR_ARG
    assert L.cheb_opfun_create(2, ints, None, None, -1.0, 1, 1, C.byref(h)) == ERR_ARG       # the solver's checks, before any device use
    assert L.cheb_opfun_create(11, (C.c_int * 11)(*[4] * 11), None, None, 0.0, 1, 1, C.byref(h)) == 3
    assert L.cheb_opfun_create(1, (C.c_int * 1)(259), None, None, 0.0, 1, 1, C.byref(h)) == ERR_ARG
    assert L.cheb_opfun_apply(None, None, None, None) == ERR_ARG and L.cheb_opfun_set_terms(None, 0, None) == ERR_ARG
    assert L.cheb_opfun_size(None, 0) == -1 and L.cheb_opfun_singular(None) == -1
