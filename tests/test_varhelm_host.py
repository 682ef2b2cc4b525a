"""VarHelmholtz on the host (no device): the long-double restatement varhelm_ref.py against itself and against the direct solve's
line matrices, the route in plain double under the per-element bar, planted faults that a normwise check passes and the bar
catches, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import linewise as lw
import varhelm_ref as vr

sp = ge.load()
LD = np.longdouble
SEED = 20261020

CASES = {
    "box3": ((5, 4, 6), ["dirichlet", "neumann", ("dirichlet", "neumann")], (0.5, 1.0, 2.0)),
    "robin2": ((9, 8), [((1.0, 2.0), (0.0, 1.0)), "dirichlet"], (1.0, 0.7)),
    "line": ((12,), [("neumann", (1.0, 0.5))], (1.3,)),
    "channel": ((8, 7, 6), ["periodic", "neumann", "periodic"], (0.5, 1.0, 2.0)),
    "per0": ((2, 5, 4), ["periodic", (1.0, 2.0), "dirichlet"], None),
}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ge.build()
    return sp.lib()


def problem(name, amp=0.9, c="field"):
    dims, bc, scale = CASES[name]
    per = sp.bc_split(bc, len(dims))[0]
    cc = vr.c_field(dims, per) if c == "field" else c
    return vr.Problem(sp, dims, bc, scale, vr.kappa_field(dims, per, amp), cc)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_assembly_matches_line_truth(name):
    """A x - lift(g) from the dense assembly equals the line-product truth of (operator at g)(x), to long-double rounding."""
    p = problem(name)
    rng = np.random.default_rng(SEED)
    x, g = rng.standard_normal(p.G), rng.standard_normal(p.NB)
    A, lift = p.dense()
    t, W = p.apply(x, g)
    err = np.abs(np.dot(A, x.astype(LD)) - lift(g) - t).astype(np.float64)
    assert np.all(err <= 2.0 ** -56 * np.maximum(W, np.abs(W).max() * 1e-3))


@pytest.mark.parametrize("name", ["box3", "robin2", "line"])
def test_unit_kappa_is_the_direct_solves_matrix(name):
    """kappa == 1, c == sigma: the assembled operator is sigma + sum_k A~_k, A~_k = S diag(lam) S^-1 of helmholtz_line_box."""
    dims, bc, scale = CASES[name]
    sigma = 0.75
    p = vr.Problem(sp, dims, bc, scale, None, sigma)
    A = p.dense()[0].astype(np.float64)
    d = len(dims)
    H = sigma * np.eye(p.G)
    for k in range(d):
        e = p.ends[k]
        S, Si, lam, _, _, _ = sp.helmholtz_line_box(dims[k], ((e[0], e[1]), (e[2], e[3])), p.scale[k])
        Ak = (S * lam) @ Si
        mats = [np.eye(m) for m in p.M]
        mats[k] = Ak
        full = mats[0]
        for m in mats[1:]:
            full = np.kron(full, m)
        H = H + full
    assert np.abs(A - H).max() <= 1e-11 * np.abs(H).max()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("inputs", ["noise", "scaled"])
def test_double_route_passes_the_cap(name, inputs):
    p = problem(name)
    rng = np.random.default_rng(SEED + 1)
    x = rng.standard_normal(p.G) if inputs == "noise" else vr.node_scaled(p.G, SEED + 2)
    g = rng.standard_normal(p.NB) if p.NB else None
    f = rng.standard_normal(p.G)
    for ff in (None, f):
        t, W = p.apply(x, g, ff)
        lw.check(p.route_double(x, g, ff), t, W, p.cap, "%s %s" % (name, "mult" if ff is None else "residual"))


def fault_problem(plant):
    """A setting in which the planted fault is small in norm (about 1e-11 of the result): coefficients, scales or end conditions that
    differ from their neighbours by that much."""
    dims = (6, 6, 5)
    eps = 2e-12 if plant == "wrong_q" else 4e-11          # (Q scales with beta times the entries of D, up to (2 n^2 + 1) / 6)
    bc = [(1.0, eps), "dirichlet", "neumann"] if plant == "wrong_q" else ["dirichlet", "neumann", ("dirichlet", "neumann")]
    scale = (1.0 + eps, 1.0, 1.0) if plant == "s_not_squared" else None
    per = (False,) * 3
    kap = 1.0 + eps * (vr.kappa_field(dims, per) - 1.0) if plant == "kappa_face" else vr.kappa_field(dims, per, 0.5)
    c = 2.0 + eps * (vr.c_field(dims, per) - 2.0) if plant == "c_unrestricted" else vr.c_field(dims, per)
    return vr.Problem(sp, dims, bc, scale, kap, c)


@pytest.mark.parametrize("plant", ["kappa_face", "wrong_q", "s_not_squared", "c_unrestricted"])
def test_planted_fault_passes_normwise_and_fails_the_bar(plant):
    p = fault_problem(plant)
    rng = np.random.default_rng(SEED + 3)
    x, g = rng.standard_normal(p.G), rng.standard_normal(p.NB)
    t, W = p.apply(x, g)
    good, bad = p.route_double(x, g), p.route_double(x, g, plant=plant)
    tn = np.linalg.norm(t.astype(np.float64))
    assert lw.worst(good, t, W)[0] <= p.cap
    assert np.linalg.norm(bad - t.astype(np.float64)) / tn < 1e-10, "the fault must be invisible to a normwise 1e-10 check"
    assert lw.worst(bad, t, W)[0] > p.cap, "the bar must catch %s" % plant


def test_cap_count():
    p = problem("box3")
    assert p.cap == 2 * (6 + 8) + 4 + 3 + 6
    p = problem("channel")
    assert p.cap == 2 * (8 + 8) + 8 + 3 + 6


def test_create_argument_errors(_lib):
    """The checks that run before any device use: they are the direct solve's."""
    L = _lib
    h = C.c_void_p()
    ints = lambda v: (C.c_int * len(v))(*v)
    dbl = lambda v: (C.c_double * len(v))(*v)
    dirichlet = [1.0, 0.0, 1.0, 0.0]
    assert L.cheb_varhelm_create(0, ints([4]), None, dbl(dirichlet), None, 1, C.byref(h)) == 3
    assert L.cheb_varhelm_create(1, ints([2]), None, dbl(dirichlet), None, 1, C.byref(h)) == 1
    assert L.cheb_varhelm_create(1, ints([259]), None, dbl(dirichlet), None, 1, C.byref(h)) == 4
    assert L.cheb_varhelm_create(1, ints([257]), ints([1]), None, None, 1, C.byref(h)) == 4
    assert L.cheb_varhelm_create(1, ints([8]), None, dbl(dirichlet), None, 17, C.byref(h)) == 4
    assert L.cheb_varhelm_create(1, ints([8]), None, dbl([0.0, 0.0, 1.0, 0.0]), None, 1, C.byref(h)) == 4
    assert L.cheb_varhelm_create(1, ints([8]), None, dbl(dirichlet), dbl([-1.0]), 1, C.byref(h)) == 4
    assert L.cheb_varhelm_create(1, ints([8]), None, None, None, 1, C.byref(h)) == 4
    assert L.cheb_varhelm_create(4, ints([258, 258, 258, 258]), None, dbl(dirichlet * 4), None, 1, C.byref(h)) == 3
    assert h.value is None
    for fn in (L.cheb_varhelm_size, L.cheb_varhelm_full_size, L.cheb_varhelm_boundary_size, L.cheb_varhelm_work_bytes):
        assert fn(None) == -1
    assert L.cheb_varhelm_mult(None, None, None, None) == 4
    assert L.cheb_varhelm_residual(None, None, None, None, None, None) == 4
    assert L.cheb_varhelm_precond(None, None, None, None) == 4
    assert L.cheb_varhelm_solve(None, None, None, None, 0, None, 1e-8, 0.0, 10, 30, None) == 4
    assert L.cheb_varhelm_set_coefficients(None, None, None, 0.0, None) == 4
    assert L.cheb_varhelm_destroy(None) == 4
    with pytest.raises(sp.ChebhipError):
        sp.VarHelmholtz((8, 8), bc=["dirichlet", ("periodic", "dirichlet")])
    with pytest.raises(ValueError):
        sp.VarHelmholtz((8, 8), bc=["dirichlet"])
