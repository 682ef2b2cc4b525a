"""The tensor mode of VarHelmholtz on the host (no device): the long-double line-product truth of vartensor_ref.py against an
independent dense assembly, the route in plain double under the per-element bar, four planted faults that a normwise check passes
and the bar catches, the closed form on a triply periodic grid, the null vectors of singular geometries, and the twin of the
library's positive-definiteness test."""
import numpy as np
import pytest

import __graft_entry__ as ge
import linewise as lw
import periodic_ref as pr
import varhelm_ref as vr
import vartensor_ref as vt

sp = ge.load()
LD = np.longdouble
SEED = 20261021

CASES = {
    "box3": ((5, 4, 6), ["dirichlet", "neumann", ("dirichlet", "neumann")], (0.5, 1.0, 2.0)),
    "robin3": ((4, 5, 4), [(1.0, 2.0), ("neumann", "dirichlet"), "dirichlet"], None),
    "robin2": ((9, 8), [((1.0, 2.0), (0.0, 1.0)), "dirichlet"], (1.0, 0.7)),
    "channel": ((8, 5, 6), ["periodic", "neumann", "periodic"], (0.5, 1.0, 2.0)),
    "per0": ((7, 5, 4), ["periodic", (1.0, 2.0), "dirichlet"], None),
    "one": ((3, 3, 3), ["dirichlet", "neumann", ("dirichlet", "neumann")], None),
}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ge.build()
    return sp.lib()


def problem(name, vel=True, c="field", k=(1.0, 0.5, 2.0)):
    dims, bc, scale = CASES[name]
    per = sp.bc_split(bc, len(dims))[0]
    cc = vr.c_field(dims, per) if c == "field" else c
    return vt.TensorProblem(sp, dims, bc, scale, vt.rotating_tensor(dims, per, k), vt.velocity_field(dims, per) if vel else None, cc)


def test_tensor_order_is_the_librarys():
    assert sp.tensor_order(3) == vt.tensor_order(3) == [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    assert sp.tensor_order(2) == vt.tensor_order(2) == [(0, 0), (1, 1), (0, 1)]


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("vel", [False, True], ids=["novel", "vel"])
def test_dense_assembly_matches_line_truth(name, vel):
    """A x + Bg g from the Kronecker assembly equals the line-product truth of (operator at g)(x), to long-double rounding."""
    p = problem(name, vel)
    rng = np.random.default_rng(SEED)
    x, g = rng.standard_normal(p.G), rng.standard_normal(p.NB)
    A, Bg = p.dense_kron()
    t, W = p.apply(x, g)
    y = np.dot(A, x.astype(LD)) + np.dot(Bg, p.g_full(g).reshape(-1).astype(LD))
    err = np.abs(y - t).astype(np.float64)
    assert np.all(err <= 2.0 ** -56 * np.maximum(W, np.abs(W).max() * 1e-3))
    # ... and the column-by-column assembly the solve tests use is the same matrix
    A2 = p.dense()[0]
    assert np.abs(A2 - A).max() <= 2.0 ** -56 * np.abs(A).max()


@pytest.mark.parametrize("name", ["box3", "robin3", "channel", "per0"])
def test_double_assembly_for_larger_grids_is_the_same_matrix(name):
    p = problem(name)
    A = p.dense_kron()[0]
    absA = np.abs(A).astype(np.float64)
    assert np.all(np.abs(p.dense_double() - A.astype(np.float64)) <= 64 * 2.0 ** -53 * (absA + absA.max() * 1e-2))


def test_identity_tensor_is_the_scalar_operator():
    """K = kappa I, no velocity: the tensor truth equals the scalar truth of varhelm_ref within both long-double evaluations' error."""
    dims, bc, scale = CASES["box3"]
    per = (False,) * 3
    kap = vr.kappa_field(dims, per, 0.5)
    K = np.stack([kap, kap, kap, 0 * kap, 0 * kap, 0 * kap])
    c = vr.c_field(dims, per)
    pt, ps = vt.TensorProblem(sp, dims, bc, scale, K, None, c), vr.Problem(sp, dims, bc, scale, kap, c)
    rng = np.random.default_rng(SEED + 9)
    x, g = rng.standard_normal(pt.G), rng.standard_normal(pt.NB)
    (tt, At), (ts, As) = pt.apply(x, g), ps.apply(x, g)
    assert np.all(np.abs(tt - ts).astype(np.float64) <= 2.0 ** -56 * (At + As))


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


def test_cap_count():
    assert problem("box3").cap == 2 * (6 + 8) + 2 * (4 + 2) + 6 + 3          # three wall directions: edge values have two stages
    assert problem("channel").cap == 2 * (8 + 8) + (3 + 2) + 6 + 3           # one wall direction: 2 (K + 8) + M + 2 d + 5
    assert problem("robin2").cap == 2 * (9 + 8) + 2 * (7 + 2) + 4 + 3
    dims = (8, 6, 4)
    per = (True,) * 3
    assert vt.TensorProblem(sp, dims, ["periodic"] * 3, None, vt.rotating_tensor(dims, per)).cap == 2 * (8 + 8) + 6 + 3


def fault_problem(plant):
    """A setting in which the planted fault is small in norm (about 1e-11 of the result): the two things the fault confuses
    differ by that much."""
    dims, per = (6, 6, 5), (False,) * 3
    bc = ["dirichlet", "neumann", ("dirichlet", "neumann")]
    eps = 4e-11
    bump = vr.kappa_field(dims, per) - 1.0
    K = vt.rotating_tensor(dims, per)
    vel = vt.velocity_field(dims, per)
    scale = None
    if plant == "k02_for_k12":
        K[5] = K[4] + eps * bump
    elif plant == "s_squared_cross":
        scale = (1.0 + eps, 1.0, 1.0)
    elif plant == "v_wrong_direction":
        vel = np.stack([vel[0], vel[0] + eps * bump, vel[0] - eps * bump])
    elif plant == "k_face":
        K = np.stack([np.full(dims, v) for v in (1.0, 1.5, 2.0, 0.2, -0.3, 0.1)]) + eps * bump
    assert np.all(vt.minors_ok(K))
    return vt.TensorProblem(sp, dims, bc, scale, K, vel, vr.c_field(dims, per))


@pytest.mark.parametrize("plant", ["k02_for_k12", "s_squared_cross", "v_wrong_direction", "k_face"])
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


@pytest.mark.parametrize("dims,m,scale", [((8, 6, 10), (1, 2, -3), (0.5, 1.0, 2.0)), ((12, 8), (3, -2), (1.0, 0.7)), ((9, 7, 5), (2, 1, 1), None)],
                         ids=["8x6x10", "12x8", "9x7x5"])
def test_closed_form_on_a_periodic_grid(dims, m, scale):
    """Constant K and v, u = sin(pi m . x) with a resolved wave vector: L u = (c + pi^2 (s o m)^T K (s o m)) u + pi (v . (s o m))
    cos(pi m . x) -- the sign and the scale of every cross term.  The input is u rounded to double, half a unit of A."""
    d = len(dims)
    per = (True,) * d
    order = vt.tensor_order(d)
    kval = {(0, 0): 1.5, (1, 1): 0.8, (2, 2): 2.0, (0, 1): 0.3, (0, 2): -0.4, (1, 2): 0.25}
    vval, c = (0.7, -1.1, 0.4)[:d], 0.6
    K = np.stack([np.full(dims, kval[jk]) for jk in order])
    assert np.all(vt.minors_ok(K))
    p = vt.TensorProblem(sp, dims, ["periodic"] * d, scale, K, np.stack([np.full(dims, v) for v in vval]), c)
    X = np.meshgrid(*[pr.nodes(n) for n in dims], indexing="ij")               # long double, exact nodes
    # sin / cos of pi times a rational: the argument reduced in integers first.  m . x = sum_k m_k (-1 + 2 j_k / n_k)
    ph = sum(LD(mk) * xk for mk, xk in zip(m, X))
    u, cu = np.sin(lw.PI_L * ph), np.cos(lw.PI_L * ph)
    sm = [LD(p.scale[k]) * LD(m[k]) for k in range(d)]
    quad = sum(LD(kval[(min(j, k), max(j, k))]) * sm[j] * sm[k] for j in range(d) for k in range(d))
    closed = (LD(c) + lw.PI_L ** 2 * quad) * u + lw.PI_L * sum(LD(v) * s for v, s in zip(vval, sm)) * cu
    x = u.astype(np.float64).reshape(-1)
    t, A = p.apply(x)
    # pi (m . x) reaches |m|_1 pi here: the long-double sine carries an absolute error of a few 2^-64 |argument|, far inside the bar
    r = lw.worst(closed.reshape(-1), t, A)[0]
    assert r <= p.cap, "closed form: %.3g x 2^-53 A (cap %d)" % (r, p.cap)
    assert np.abs(t).max() > 1.0


@pytest.mark.parametrize("dims,bc", [((8, 5, 6), ["periodic", "neumann", "periodic"]), ((5, 4, 6), ["neumann"] * 3),
                                     ((6, 4), ["periodic", "periodic"]), ((7, 5, 4), ["periodic", "neumann", "neumann"])],
                         ids=["channel", "neumann-box", "torus2", "odd-periodic"])
@pytest.mark.parametrize("vel", [False, True], ids=["novel", "vel"])
def test_null_vectors_are_annihilated(dims, bc, vel):
    """c == 0, every direction periodic or Neumann / Neumann: the +-1 vectors of cheb_varhelm_null_signs_host are in the null space of
    the dense tensor operator, with a velocity too -- every G_k of such a vector is zero up to the rounding of Q's doubles."""
    d = len(dims)
    per = sp.bc_split(bc, d)[0]
    p = vt.TensorProblem(sp, dims, bc, None, vt.rotating_tensor(dims, per), vt.velocity_field(dims, per) if vel else None, 0.0)
    A = p.dense_kron()[0]
    Z = sp.null_space(dims, per).reshape(-1, p.G)
    assert Z.shape[0] == 2 ** sum(1 for n, q in zip(dims, per) if q and n % 2 == 0)
    absA = np.abs(A).astype(np.float64).sum(axis=1)
    for z in Z:
        assert set(np.unique(z)) <= {-1.0, 1.0}
        assert np.all(np.abs(np.dot(A, z.astype(LD))).astype(np.float64) <= p.cap * 2.0 ** -53 * absA)
    # and nothing else: the rank deficiency is exactly the number of vectors
    sv = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    assert np.sum(sv <= 1e-10 * sv[0]) == Z.shape[0]


def test_minors_twin():
    dims, per = (5, 4, 6), (False,) * 3
    K = vt.rotating_tensor(dims, per, (1.0, 0.5, 10.0))
    assert np.all(vt.minors_ok(K))
    assert np.all(vt.minors_ok(vt.rotating_tensor((9, 8), (False, False), (0.5, 5.0))))
    # one node with det = -1e-3: diag(1, 1, t) with t = -1e-3 there
    bad = np.stack([np.ones(dims), np.ones(dims), np.ones(dims), np.zeros(dims), np.zeros(dims), np.zeros(dims)])
    bad[2, 2, 1, 3] = -1e-3
    ok = vt.minors_ok(bad)
    assert not ok[2, 1, 3] and ok.sum() == ok.size - 1
    # the same through the eigenvalues: the minors test is Sylvester's criterion
    full = np.array([[bad[vt.tensor_order(3).index((min(i, j), max(i, j)))][2, 1, 3] for j in range(3)] for i in range(3)])
    assert np.linalg.eigvalsh(full).min() < 0 and abs(np.linalg.det(full) + 1e-3) < 1e-15
    for v in (np.nan, np.inf):
        b = K.copy()
        b[4, 0, 0, 0] = v
        assert not vt.minors_ok(b)[0, 0, 0]
    b2 = vt.rotating_tensor((9, 8), (False, False))
    b2[2, 3, 3] = 5.0                                                            # K01^2 > K00 K11
    assert not vt.minors_ok(b2)[3, 3]
