"""The per-element bar of the Stokes and Jacobian callbacks (tests/callbacks_ref.py), checked on the CPU: the C truths and
weights of the oracle against their NumPy long-double twin and against what the tree already trusts; plain double
restatements of the operators through the bar (it is satisfiable); planted faults that the bar must catch and the normwise bar
(relerr < 1e-10) must miss (it is sharp).

Measured on the CPU (worst |y - truth| / (2^-53 W), velocity rows / pressure rows): plain double restatement 1.5 .. 13 / 1 .. 5,
even / odd restatement 1.5 .. 12 / 1 .. 5, against caps 62 .. 80 / 25 .. 30; the DIRECT oracle about 8."""
import os

import numpy as np
import pytest

import callbacks_ref as cb
import linewise as lw
import oracle_lib as orc
from conftest import relerr

LD = np.longdouble
SEED = 20240229
POWER = (1, 1.0, 3.0, 1e-2, 1.0)
ST_SHAPES = [(20, 17), (13, 11, 9), (14, 12, 9), (14, 12, 10)]            # the small shapes of test_gpu_callbacks.py
ELL_SHAPES = [(24, 20), (12, 11, 10), (33, 40)]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def close_to_rounded(c, t, W=None, K=0):
    """c is the long-double value t rounded once to double, up to the long-double rounding of two summation orders."""
    err = np.abs(c.astype(LD) - t).astype(np.float64)
    lim = 2.0 ** -53 * np.abs(t.astype(np.float64)) * (1 + 2.0 ** -8)
    if W is not None:
        lim = lim + (2 * K + 40) * 2.0 ** -63 * W
    assert np.all(err <= lim), float((err / np.maximum(lim, 1e-300)).max())


# ----------------------------------------------------------------------------------------------
# the C truth against the NumPy twin
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ST_SHAPES, ids=ids)
@pytest.mark.parametrize("state", cb.STATES)
def test_stokes_truth_c_vs_numpy(dims, state):
    eta, deta, S0 = cb.stokes_state(dims, state)
    rng = np.random.default_rng(SEED)
    N, I, g, dv = cb.sizes(dims)
    for x, dirichlet, force in ((cb.noise(dims, 1), None, None), (cb.node_scaled(dims, 2), None, None),
                                (cb.noise(dims, 3), rng.standard_normal(dv), rng.standard_normal(g))):
        y, W = orc.stokes_truth(dims, x, eta, deta, S0, dirichlet, force, nthreads=4)
        t, _ = cb.stokes_apply(dims, x, eta, deta, S0, dirichlet, force)
        Wn, _, _ = cb.stokes_weight(dims, x, eta, deta, S0, dirichlet, force)
        assert np.all(np.abs(W - Wn) <= 1e-12 * Wn)
        close_to_rounded(y, t, Wn, max(dims))


@pytest.mark.parametrize("dims", ST_SHAPES, ids=ids)
@pytest.mark.parametrize("rheology", [POWER, (0, 1.0, 1.0, 1.0, 1.0), (1, 1.3, 2.0, 1e-1, 0.7)], ids=["power", "linear", "power2"])
def test_stokes_function_truth_c_vs_numpy(dims, rheology):
    rng = np.random.default_rng(SEED + 1)
    N, I, g, dv = cb.sizes(dims)
    x, dirichlet, force = rng.standard_normal(g), rng.standard_normal(dv), rng.standard_normal(g)
    r = orc.stokes_function_truth(dims, x, dirichlet, force, rheology, nthreads=4)
    t, st = cb.stokes_apply(dims, x, dirichlet=dirichlet, force=force, rheology=rheology)
    Wn, ws, wg = cb.stokes_function_weight(dims, x, dirichlet, force, st)
    assert np.all(np.abs(r["W"] - Wn) <= 1e-12 * Wn)
    assert np.all(np.abs(r["wstrain"] - ws) <= 1e-12 * ws) and np.all(np.abs(r["wgamma"] - wg) <= 1e-12 * wg)
    close_to_rounded(r["y"], t, Wn, max(dims))
    close_to_rounded(r["eta"], st[0])
    close_to_rounded(r["deta"], st[1])
    close_to_rounded(r["strain"], st[2], ws, max(dims))


@pytest.mark.parametrize("dims", ELL_SHAPES, ids=ids)
def test_elliptic_truths_c_vs_numpy(dims):
    rng = np.random.default_rng(SEED + 2)
    N, G, Dn = orc.sizes(dims)
    d = len(dims)
    U, eta, deta, g0 = rng.standard_normal(G), np.exp(rng.uniform(-1, 1, N)), rng.standard_normal(N), rng.standard_normal((d, N))
    V, W = orc.elliptic_truth(dims, U, eta, deta, g0, nthreads=4)
    t, _ = cb.elliptic_apply(dims, U, eta, deta, g0)
    Wn, _ = cb.elliptic_weight(dims, U, eta, deta, g0)
    assert np.all(np.abs(W - Wn) <= 1e-12 * Wn)
    close_to_rounded(V, t, Wn, max(dims))
    b, dv = rng.standard_normal(G), rng.standard_normal(Dn)
    for U1, expo in ((U, 2.0), (1.0 + 0.5 * rng.random(G), 2.5)):
        dv1 = dv if expo == 2.0 else 1.0 + 0.5 * rng.random(Dn)
        r = orc.elliptic_function_truth(dims, U1, b, dv1, gamma=1.0, exponent=expo, nthreads=4)
        t, st = cb.elliptic_apply(dims, U1, dirichlet=dv1, b=b, gamma=1.0, exponent=expo)
        Wn, wg = cb.elliptic_weight(dims, U1, st[0].astype(np.float64), st[1].astype(np.float64), st[2].astype(np.float64), dv1, b)
        assert np.all(np.abs(r["W"] - Wn) <= 1e-12 * Wn) and np.all(np.abs(r["wgrad"] - wg) <= 1e-12 * wg)
        close_to_rounded(r["rhs"], t, Wn, max(dims))
        close_to_rounded(r["eta"], st[0])
        close_to_rounded(r["deta"], st[1])
        close_to_rounded(r["gradu"], st[2], wg, max(dims))


def test_extrapolation_weights_reproduce_polynomials():
    """Two statements of the Lagrange weights: the closed form in the C truth (through p = polynomial) and the product formula
    of callbacks_ref.ext_weights; both extrapolate polynomials of degree < P - 2 from the interior nodes to the ends."""
    for P in (3, 4, 9, 10, 17, 68, 130):
        n = P - 1
        xs = np.cos(lw.PI_L * np.arange(P) / n)
        w0, w1 = cb.ext_weights(P)
        for deg in range(0, min(P - 2, 6)):
            f = xs ** deg
            assert abs(np.dot(w0, f) - LD(1)) <= P * 2.0 ** -60 * np.dot(np.abs(w0), np.abs(f))
            assert abs(np.dot(w1, f) - LD(-1) ** deg) <= P * 2.0 ** -60 * np.dot(np.abs(w1), np.abs(f))


# ----------------------------------------------------------------------------------------------
# the C truth against what the tree already trusts
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ST_SHAPES + [(34, 9, 12)], ids=ids)
def test_stokes_truth_vs_direct_oracle(dims):
    rng = np.random.default_rng(SEED + 3)
    N, I, g, dv = cb.sizes(dims)
    eta, deta, S0 = cb.stokes_state(dims, "full")
    x, dirichlet, force = rng.standard_normal(g), rng.standard_normal(dv), rng.standard_normal(g)
    y, W = orc.stokes_truth(dims, x, eta, deta, S0, nthreads=4)
    yo = orc.stokes_mult(dims, x, eta, deta, S0, mode=orc.DIRECT)
    assert relerr(y, yo) <= 1e-12
    rv, rp = cb.worst_stokes(dims, yo, y, W)
    print("callback-host direct-oracle mult %s %.2f %.2f" % (ids(dims), rv, rp))
    r = orc.stokes_function_truth(dims, x, dirichlet, force, POWER, nthreads=4)
    yo, e, de, s = orc.stokes_function(dims, x, dirichlet, force, POWER, mode=orc.DIRECT)
    assert relerr(r["y"], yo) <= 1e-12 and relerr(r["eta"], e) <= 1e-12 and relerr(r["deta"], de) <= 1e-12
    assert relerr(r["strain"], s) <= 1e-12
    # the blocks: MatVV, MatPV and MatVP are rows of the truth on [v; 0] and [0; p]
    X = x.reshape(-1, len(dims) + 1)
    v, p = np.ascontiguousarray(X[:, :-1]).ravel(), np.ascontiguousarray(X[:, -1])
    tv, _ = orc.stokes_truth(dims, cb.block_v(dims, 0) * 0 + np.concatenate([X[:, :-1], 0 * X[:, -1:]], axis=1).ravel(), eta, deta, S0, nthreads=4)
    tp, _ = orc.stokes_truth(dims, np.concatenate([0 * X[:, :-1], X[:, -1:]], axis=1).ravel(), eta, deta, S0, nthreads=4)
    assert relerr(cb.rows(dims, tv)[0].ravel(), orc.stokes_mult_vv(dims, v, eta, deta, S0, mode=orc.DIRECT)) <= 1e-12
    assert relerr(cb.rows(dims, tv)[1], orc.stokes_divergence(dims, v, mode=orc.DIRECT)) <= 1e-12
    assert relerr(cb.rows(dims, tp)[0].ravel(), orc.stokes_mult_vp(dims, p, mode=orc.DIRECT)) <= 1e-12
    assert np.all(cb.rows(dims, tp)[1] == 0)


@pytest.mark.parametrize("dims", ELL_SHAPES, ids=ids)
def test_elliptic_truth_vs_direct_oracle_and_linewise(dims):
    rng = np.random.default_rng(SEED + 4)
    N, G, Dn = orc.sizes(dims)
    d = len(dims)
    U, eta, deta, g0 = rng.standard_normal(G), np.exp(rng.uniform(-1, 1, N)), rng.standard_normal(N), rng.standard_normal((d, N))
    V, W = orc.elliptic_truth(dims, U, eta, deta, g0, nthreads=4)
    assert relerr(V, orc.elliptic_mult(dims, U, eta, deta, g0, mode=orc.DIRECT)) <= 1e-12
    b, dv = rng.standard_normal(G), rng.standard_normal(Dn)
    r = orc.elliptic_function_truth(dims, U, b, dv, gamma=1.0, nthreads=4)
    ro, e, de, gu = orc.elliptic_function(dims, U, b, dv, gamma=1.0, mode=orc.DIRECT)
    assert relerr(r["rhs"], ro) <= 1e-12 and relerr(r["eta"], e) <= 1e-12 and relerr(r["deta"], de) <= 1e-12 and relerr(r["gradu"], gu) <= 1e-12
    # eta = 1: the constant-coefficient truth of linewise.py, -sum_k L_k U with L = (D D) interior.  D (D u) and (D D) u differ
    # by long-double rounding of sums whose terms W bounds; W dominates linewise's weight B
    V1, W1 = orc.elliptic_truth(dims, U, nthreads=4)
    t, B, _ = lw.elliptic_truth_bound(dims, U)
    assert np.all(W1 >= B.ravel() * (1 - 1e-12))
    err = np.abs(V1.astype(LD) - t.ravel()).astype(np.float64)
    assert np.all(err <= 2.0 ** -53 * np.abs(V1) * (1 + 2.0 ** -8) + (2 * max(dims) + 40) * 2.0 ** -63 * W1)


def _pl():
    PL = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analytic_powerlaw.npz"))
    B, n, eps, g0 = [float(v) for v in PL["rheology"]]
    return PL, (1, B, n, eps, g0), [tuple(int(v) for v in str(s).split("x")) for s in PL["cases"]]


def _pl_vectors(PL, dims):
    tag = "pl_" + "x".join(map(str, dims))
    V, Pp, Fv, dv = PL[tag + "_v"], PL[tag + "_p"], PL[tag + "_f"], PL[tag + "_div"]
    m = ~cb.boundary_mask(dims)
    return (np.concatenate([V[m], Pp[m][:, None]], axis=1).ravel(), np.concatenate([Fv[m], dv[m][:, None]], axis=1).ravel(),
            V[~m].ravel().copy())


def test_function_truth_at_the_50_digit_power_law_fixture():
    """The asserts of test_oracle_identities.py on the long-double truth: at the analytic fields of the fixture the residual is
    the truncation error and decays spectrally; eta, eta' and the strain equal their closed forms."""
    PL, rh, cases = _pl()
    for family in ([c for c in cases if len(c) == 2], [c for c in cases if len(c) == 3]):
        res = []
        for dims in family:
            xG, fG, dvals = _pl_vectors(PL, dims)
            r = orc.stokes_function_truth(dims, xG, dvals, fG, rh, nthreads=4)
            res.append(np.abs(r["y"]).max() / np.abs(fG).max())
        assert res[1] < res[0] * 2e-3 and res[2] < res[1] * 5e-3 and res[2] < 2e-7, res
    for dims in ((28, 26), (20, 18, 16)):
        d = len(dims)
        tag = "pl_" + "x".join(map(str, dims))
        xG, fG, dvals = _pl_vectors(PL, dims)
        r = orc.stokes_function_truth(dims, xG, dvals, fG, rh, nthreads=4)
        assert relerr(r["eta"], PL[tag + "_eta"].ravel()) < 1e-12 and relerr(r["deta"], PL[tag + "_deta"].ravel()) < 1e-12
        S = PL[tag + "_strain"].reshape(-1, d, d)
        for j in range(d):
            assert relerr(r["strain"][j].reshape(-1, d), S[:, j, :]) < 1e-12


# ----------------------------------------------------------------------------------------------
# the bar is satisfiable: plain double restatements pass every cap
# ----------------------------------------------------------------------------------------------
def _families(dims, linear):
    fam = [("noise", cb.noise(dims, 11)), ("block-v", cb.block_v(dims, 12)), ("block-p", cb.block_p(dims, 13)),
           ("constant-pressure", cb.constant_pressure(dims, 14))]
    if linear:
        fam.append(("node-scaled", cb.node_scaled(dims, 15)))
    return fam


@pytest.mark.parametrize("dims", ST_SHAPES, ids=ids)
@pytest.mark.parametrize("prod", [cb.prod_double, cb.prod_evenodd], ids=["plain", "evenodd"])
def test_double_restatement_of_the_stokes_callbacks_passes_every_cap(dims, prod):
    d = len(dims)
    N, I, g, dv = cb.sizes(dims)
    worst = [0.0, 0.0]
    for state in cb.STATES:
        eta, deta, S0 = cb.stokes_state(dims, state)
        inputs = _families(dims, True)
        for node in cb.impulse_positions(dims):
            inputs += [("impulse%s/%d" % (node, c), cb.impulse(dims, node, c)) for c in range(d + 1)]
        for name, x in inputs:
            y, _ = cb.stokes_apply(dims, x, eta, deta, S0, prod=prod, T=np.float64)
            t, W = orc.stokes_truth(dims, x, eta, deta, S0, nthreads=4)
            if name == "constant-pressure":
                t = cb.exact_zero(dims, t, W)
                assert W.max() > 0
            for rowk, r, idx, cap in cb.check_stokes(dims, y, t, W, "%s %s %s" % (ids(dims), state, name)):
                worst[rowk == "p"] = max(worst[rowk == "p"], r)
    rng = np.random.default_rng(SEED + 5)
    x, dirichlet, force = rng.standard_normal(g), rng.standard_normal(dv), rng.standard_normal(g)
    for rh in (POWER, (0, 1.0, 1.0, 1.0, 1.0)):
        y, st = cb.stokes_apply(dims, x, dirichlet=dirichlet, force=force, rheology=rh, prod=prod, T=np.float64)
        r = orc.stokes_function_truth(dims, x, dirichlet, force, rh, nthreads=4)
        for rowk, q, idx, cap in cb.check_stokes(dims, y, r["y"], r["W"], "%s function" % ids(dims), fn=True, power=rh[0] == 1):
            worst[rowk == "p"] = max(worst[rowk == "p"], q)
        for j in range(d):
            lw.check(st[2][j], r["strain"][j], r["wstrain"][j], cb.cap_strain(dims), "strain[%d]" % j)
        if rh[0] == 1:
            be, bde = cb.eta_bounds(dims, rh, r)
            cb.check_relative(st[0], r["eta"], be, "eta")
            cb.check_relative(st[1], r["deta"], bde, "eta'")
        # the Jacobian apply linearised about that state
        eta, deta, S0 = r["eta"], r["deta"], r["strain"]
        xv = cb.noise(dims, 16)
        y, _ = cb.stokes_apply(dims, xv, eta, deta, S0, prod=prod, T=np.float64)
        t, W = orc.stokes_truth(dims, xv, eta, deta, S0, nthreads=4)
        cb.check_stokes(dims, y, t, W, "%s linearised" % ids(dims))
    print("callback-host restatement %s %s velocity %.2f (cap %d) pressure %.2f (cap %d)" % (
        ids(dims), prod.__name__, worst[0], cb.cap_v(dims), worst[1], cb.cap_p(dims)))


@pytest.mark.parametrize("dims", ELL_SHAPES, ids=ids)
@pytest.mark.parametrize("prod", [cb.prod_double, cb.prod_evenodd], ids=["plain", "evenodd"])
def test_double_restatement_of_the_elliptic_callbacks_passes_every_cap(dims, prod):
    rng = np.random.default_rng(SEED + 6)
    N, G, Dn = orc.sizes(dims)
    d = len(dims)
    eta, deta, g0 = np.exp(rng.uniform(-1, 1, N)), rng.standard_normal(N), rng.standard_normal((d, N))
    worst = 0.0
    k = rng.integers(-30, 31, size=G)
    for name, U in (("noise", rng.standard_normal(G)), ("node-scaled", rng.standard_normal(G) * 10.0 ** k)):
        V, _ = cb.elliptic_apply(dims, U, eta, deta, g0, prod=prod, T=np.float64)
        t, W = orc.elliptic_truth(dims, U, eta, deta, g0, nthreads=4)
        worst = max(worst, lw.check(V, t, W, cb.cap_e(dims), "%s mult %s" % (ids(dims), name))[0])
    U, b, dv = rng.standard_normal(G), rng.standard_normal(G), rng.standard_normal(Dn)
    V, st = cb.elliptic_apply(dims, U, dirichlet=dv, b=b, gamma=1.0, prod=prod, T=np.float64)
    r = orc.elliptic_function_truth(dims, U, b, dv, gamma=1.0, nthreads=4)
    worst = max(worst, lw.check(V, r["rhs"], r["W"], cb.cap_e(dims, True), "%s function" % ids(dims))[0])
    for kk in range(d):
        lw.check(st[2][kk], r["gradu"][kk], r["wgrad"][kk], max(dims) + 8, "gradu[%d]" % kk)
    cb.check_relative(st[0], r["eta"], 3, "eta")
    cb.check_relative(st[1], r["deta"], 2, "eta'")
    print("callback-host restatement elliptic %s %s %.2f (cap %d)" % (ids(dims), prod.__name__, worst, cb.cap_e(dims)))


# ----------------------------------------------------------------------------------------------
# the bar is sharp: planted faults fail it and pass relerr < 1e-10
# ----------------------------------------------------------------------------------------------
def _fails_bar_passes_norm(dims, y_bad, t, W, fn=False, power=False):
    assert relerr(y_bad, t) < 1e-10, relerr(y_bad, t)
    with pytest.raises(AssertionError):
        cb.check_stokes(dims, y_bad, t, W, "planted fault", fn=fn, power=power)


def _small_nonlinear_state(dims, symmetric=True):
    """A state whose eta' S0 z term is 1e-9 of the stress, so that a defect in it at one node hides from the norm."""
    eta, deta, S0 = cb.stokes_state(dims, "full")
    d, N = len(dims), int(np.prod(dims))
    if not symmetric:
        S0 = np.random.default_rng(3).standard_normal((d, N * d))
    return eta, 1e-9 * deta, S0


DIMS = (14, 12, 10)


def test_fault_matrix_entry():
    """One entry of D_y off by 1e-12 of its size."""
    eta, deta, S0 = cb.stokes_state(DIMS, "full")
    x = cb.noise(DIMS, 21)
    t, W = orc.stokes_truth(DIMS, x, eta, deta, S0, nthreads=4)
    mats = [lw.dense_D(P).astype(np.float64) for P in DIMS]
    good, _ = cb.stokes_apply(DIMS, x, eta, deta, S0, prod=cb.prod_double, T=np.float64, mats=mats)
    cb.check_stokes(DIMS, good, t, W, "unplanted")
    mats[1] = mats[1].copy()
    mats[1][4, 5] *= 1 + 1e-12
    bad, _ = cb.stokes_apply(DIMS, x, eta, deta, S0, prod=cb.prod_double, T=np.float64, mats=mats)
    _fails_bar_passes_norm(DIMS, bad, t, W)


def test_fault_pressure_row():
    """One pressure row off by 0.1 %: rows that scale like n^2 |v| next to rows that scale like n^4 |v| in one norm.  The
    long lines of a 2-D grid put the row under 1e-10 of the norm, as 128^3 does in three dimensions."""
    dims = (320, 300)
    x = cb.noise(dims, 22)
    t, W = orc.stokes_truth(dims, x, nthreads=8)
    good, _ = cb.stokes_apply(dims, x, prod=cb.prod_double, T=np.float64)
    cb.check_stokes(dims, good, t, W, "unplanted")
    row = int(np.argmin(np.abs(cb.rows(dims, t)[1]) + 1e300 * (cb.rows(dims, t)[1] == 0)))
    bad, _ = cb.stokes_apply(dims, x, prod=cb.prod_double, T=np.float64, fault=("prow", row, 1e-3))
    assert bad.reshape(-1, 3)[row, 2] != good.reshape(-1, 3)[row, 2]
    _fails_bar_passes_norm(dims, bad, t, W)


def test_fault_folded_pressure_face_value():
    """The extrapolated face value of one z line off by 1e-9."""
    eta, deta, S0 = cb.stokes_state(DIMS, "full")
    x = cb.noise(DIMS, 23)
    t, W = orc.stokes_truth(DIMS, x, eta, deta, S0, nthreads=4)
    bad, _ = cb.stokes_apply(DIMS, x, eta, deta, S0, prod=cb.prod_double, T=np.float64, fault=("face", 2, (5, 4), 1e-9))
    _fails_bar_passes_norm(DIMS, bad, t, W)


def test_fault_dropped_nonlinear_term():
    """eta' S0_jk z dropped from one stress component at one node."""
    eta, deta, S0 = _small_nonlinear_state(DIMS)
    x = cb.noise(DIMS, 24)
    t, W = orc.stokes_truth(DIMS, x, eta, deta, S0, nthreads=4)
    good, _ = cb.stokes_apply(DIMS, x, eta, deta, S0, prod=cb.prod_double, T=np.float64)
    cb.check_stokes(DIMS, good, t, W, "unplanted")
    bad, _ = cb.stokes_apply(DIMS, x, eta, deta, S0, prod=cb.prod_double, T=np.float64, fault=("drop", 0, 1, (6, 5, 4)))
    _fails_bar_passes_norm(DIMS, bad, t, W)


def test_fault_transposed_stress_components():
    """tau_01 and tau_10 exchanged at one node.  The stress is symmetric only as far as S0 is; with eta' != 0 and an S0 that
    is not, the two slots differ by eta' z (S0_01 - S0_10), and a kernel that reads the wrong one is wrong by that."""
    eta, deta, S0 = _small_nonlinear_state(DIMS, symmetric=False)
    x = cb.noise(DIMS, 25)
    t, W = orc.stokes_truth(DIMS, x, eta, deta, S0, nthreads=4)
    good, _ = cb.stokes_apply(DIMS, x, eta, deta, S0, prod=cb.prod_double, T=np.float64)
    cb.check_stokes(DIMS, good, t, W, "unplanted")
    bad, _ = cb.stokes_apply(DIMS, x, eta, deta, S0, prod=cb.prod_double, T=np.float64, fault=("transpose", 0, 1, (6, 5, 4)))
    _fails_bar_passes_norm(DIMS, bad, t, W)


def test_fault_wrong_dirichlet_neighbour():
    """The interior node next to the corner reads, as its boundary neighbour in x, the Dirichlet value of the boundary node one
    step along z.  Boundary data 1 + 1e-11 noise: neighbouring values differ in the 11th digit."""
    N, I, g, dv = cb.sizes(DIMS)
    rng = np.random.default_rng(26)
    x, dirichlet, force = rng.standard_normal(g), 1.0 + 1e-11 * rng.standard_normal(dv), rng.standard_normal(g)
    r = orc.stokes_function_truth(DIMS, x, dirichlet, force, POWER, nthreads=4)
    good, _ = cb.stokes_apply(DIMS, x, dirichlet=dirichlet, force=force, rheology=POWER, prod=cb.prod_double, T=np.float64)
    cb.check_stokes(DIMS, good, r["y"], r["W"], "unplanted", fn=True, power=True)
    bad, _ = cb.stokes_apply(DIMS, x, dirichlet=dirichlet, force=force, rheology=POWER, prod=cb.prod_double, T=np.float64,
                             fault=("dirichlet", (0, 1, 1), (0, 1, 2)))
    _fails_bar_passes_norm(DIMS, bad, r["y"], r["W"], fn=True, power=True)


def test_impulse_positions_cover_what_they_name():
    for dims in ST_SHAPES + [(120, 121, 68), (98, 96, 130)]:
        pos = cb.impulse_positions(dims)
        assert all(all(0 < i < p - 1 for i, p in zip(n, dims)) for n in pos)
        for k in range(len(dims)):
            assert {n[k] for n in pos} >= {1, dims[k] - 2}
        if len(dims) == 3:
            lines = {(n[0] * dims[1] + n[1]) % 64 for n in pos}
            assert lines >= {15, 16, 31, 32, 63, 0}
