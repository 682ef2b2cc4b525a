"""Host side of the per-solve bar of the Stokes block preconditioners (saddle_ref.py; the device side is test_gpu_saddle_steps.py):
the restated apply against the dense block formulas, the gap condition that makes the inner iteration counts a property of the
method on every case of the tables, and planted faults in restatement A -- what the bar must catch.  No GPU."""
import numpy as np
import pytest

import __graft_entry__ as ge
import oracle_lib as orc
import krylov_ref as kr
import saddle_ref as sr
from conftest import relerr

sp = ge.load()
LD = np.longdouble
SEED = 20260101                # shared with test_gpu_saddle_steps.py: the same cases, states and right-hand sides
NT = 16


@pytest.fixture(scope="module", autouse=True)
def _built():
    ge.build()


def _dense(fn, nin, nout):
    A = np.empty((nout, nin)); e = np.zeros(nin)
    for j in range(nin):
        e[j] = 1.0; A[:, j] = fn(e); e[j] = 0.0
    return A


@pytest.mark.parametrize("dims", [(7, 6), (6, 5, 5)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("visc", ["unit", "variable"])
def test_converged_restatement_is_the_block_formula(dims, kind, visc):
    """With all inner solves converged (400, 1e-14 / 1e-13) the restatement is the block formula of its comment (stokes.C:1712, 1745,
    1770, 1795): the dense algebra and the 1e-8 of test_gpu_saddle.test_saddle_types_vs_dense."""
    d = len(dims)
    N, I, gv, gp, g, ndv = orc.stokes_sizes(dims)
    rng = np.random.default_rng(SEED)
    eta = np.ones(N) if visc == "unit" else np.exp(rng.uniform(np.log(0.5), np.log(10.0), N))
    x = rng.standard_normal(g)
    cfg = sr.config(vel=(400, 1e-14), schur=(400, 1e-13), svel=(400, 1e-14))
    y = sr.apply(sr.oracle_ops(sp, dims, (eta, None, None)), x, kind, cfg)["y"]
    VV = _dense(lambda e: orc.stokes_mult_vv(dims, e, eta=eta, mode=orc.DIRECT), gv, gv)
    VP = _dense(lambda e: orc.stokes_mult_vp(dims, e, mode=orc.DIRECT), gp, gv)
    PV = _dense(lambda e: orc.stokes_divergence(dims, e, mode=orc.DIRECT), gv, gp)
    S = -PV @ np.linalg.solve(VV, VP)
    Dm = np.diag(sr.fr.interior(eta, dims).ravel())
    Q = np.linalg.qr(np.eye(gp) - 1.0 / gp)[0][:, :gp - 1]             # orthonormal basis of the zero-mean subspace
    Sinv = Q @ np.linalg.solve(Q.T @ Dm @ S @ Q, Q.T @ Dm)
    xv, xp = sr.split(x, d)
    Ai = lambda b: np.linalg.solve(VV, b)
    if kind == 0:
        v1 = Ai(xv); p1 = Sinv @ (xp - PV @ v1); yv = v1 + Ai(-VP @ p1)
    elif kind == 1:
        p1 = Sinv @ xp; yv = Ai(xv - VP @ p1)
    elif kind == 2:
        yv = Ai(xv); p1 = Sinv @ xp
    else:
        yv = Ai(xv); p1 = Sinv @ (xp - PV @ yv)
    gv_, gp_ = sr.split(y, d)
    assert sr.mean_of(gp_) <= sr.mean_bar(gp_)
    assert relerr(gv_, yv) < 1e-8
    assert relerr(gp_, p1 - p1.mean()) < 1e-8


@pytest.mark.parametrize("c", sr.cases(), ids=sr.case_id)
def test_gap_condition_and_restatements(c):
    """No residual norm of any inner solve of the truth lies within a factor 1.25 of its tolerance: the iteration counts of the case
    are a property of the method, and the restatements reproduce them.  The restatements themselves sit at or below 1 / 16 of the
    bar by construction, and their pressure is zero-mean to the device's bar."""
    r = sr.reference(sp, c, SEED)
    d = len(c[0])
    g = sr.gap(r["ld"]["hist"])
    print(sr.case_id(c), "its", r["ld"]["its"], "gap %.3g" % g)
    assert g > sr.GAP, g
    for q in r["rest"]:
        assert q["its"] == r["ld"]["its"]
        got = sr.part_ratios(q["y"], r["ld"]["y"], [w["y"] for w in r["rest"]], d)
        assert all(v <= 1.0 / sr.MARGIN for v in got.values()), got
        yp =sr.split(q["y"], d)[1]
        assert sr.mean_of(yp) <= sr.mean_bar(yp)
    if c[0] == (3, 3):
        assert not np.any(sr.split(r["ld"]["y"], d)[1]) and r["ld"]["its"][1] == 0   # one pressure unknown: the zero-mean subspace is {0}


def test_c7_ends_on_its_tolerance_inside_the_limit():
    for c in sr.cases():
        if c[3] != "C7":
            continue
        r = sr.reference(sp, c, SEED)
        for name, tol, rs in r["ld"]["hist"]:
            assert len(rs) - 1 < 30 and rs[-1] <= tol and len(rs) > 3, (sr.case_id(c), name, len(rs))


def test_every_state_appears_on_every_shape_and_kind_of_the_configurations():
    """Across C2 .. C7 each (shape, kind) pair meets each of the three states at least once."""
    for key in sr.CONFIG_STATE["C2"]:
        assert {sr.CONFIG_STATE[n][key] for n in sr.CONFIG_STATE} == set(sr.STATES), key
    for n in ("C3", "C4"):                   # the Jacobi scaling / pc_sweeps are invisible with eta == 1
        assert "unit" not in sr.CONFIG_STATE[n].values()


@pytest.mark.parametrize("c", sr.LARGE_CASES, ids=sr.case_id)
def test_gap_condition_large(c):
    """The large shape has no dense truth: the gap condition on restatement A's histories, B's counts equal A's, and the two differ
    by rounding."""
    a, b = large_reference(c)
    g = sr.gap(a["hist"])
    print(sr.case_id(c), "its", a["its"], "gap %.3g" % g)
    assert g > sr.GAP and a["its"] == b["its"]
    assert relerr(b["y"], a["y"]) < 1e-12


_LARGE = {}


def large_reference(c):
    if c not in _LARGE:
        dims, kind, sname, name = c
        seed = sr.case_seed(c, SEED)
        st = sr.make_state(dims, sname, seed)
        x = sr.case_rhs(c, SEED)
        _LARGE[c] = (sr.apply(sr.oracle_ops(sp, dims, st, orc.DIRECT, "plain", NT), x, kind, sr.case_config(c), np.float64, kr.dot_pairwise),
                     sr.apply(sr.oracle_ops(sp, dims, st, orc.FAST, "evenodd", NT), x, kind, sr.case_config(c), np.float64, kr.dot_strided))
    return _LARGE[c]


# where a fault can show: the kinds that run the faulted line; a, b, h need a viscosity that varies
FAULT_KINDS = {"a": (0, 1, 2, 3), "b": (0, 1, 2, 3), "c": (0, 1, 2, 3), "d": (0, 1, 2, 3), "e": (0, 3), "f": (0,), "g": (3,),
               "h": (0, 1, 2, 3), "i": (0, 1, 2, 3), "j": (0, 1, 2, 3), "k": (0, 1, 2, 3)}
FAULT_SHAPES = [(11, 9), (10, 9, 8), (5, 4, 70)]


def fault_cases(fault):
    """Fault d shows only where KSPSchur ends on its tolerance (saddle_ref.case_rhs): the C7 cases."""
    if fault == "d":
        return [c for c in sr.cases() if c[3] == "C7"]
    return [(dims, kind, "variable", "C1") for dims in FAULT_SHAPES for kind in FAULT_KINDS[fault]]


@pytest.mark.parametrize("fault", sorted(FAULT_KINDS))
def test_the_bar_catches_planted_faults(fault):
    """Each fault planted in restatement A (default limits, variable viscosity) exceeds ratio 1 on the velocity or on the pressure
    part, on every shape and kind where it can show -- the cases test_gpu_saddle_steps.py runs on the device, so the same slip in
    saddle.hip turns those cases red."""
    for c in fault_cases(fault):
        dims, kind = c[0], c[1]
        r = sr.reference(sp, c, SEED)
        bad = sr.apply(sr.oracle_ops(sp, dims, r["state"]), r["x"], kind, r["cfg"], fault=fault)
        got = sr.part_ratios(bad["y"], r["ld"]["y"], [w["y"] for w in r["rest"]], len(dims))
        print("fault %s  %-24s v %.3g / %.3g  p %.3g / %.3g  its %s (truth %s)" % (fault, sr.case_id(c), got["v_max"], got["v_2"], got["p_max"],
                                                                             got["p_2"], bad["its"], r["ld"]["its"]))
        assert max(got["v_max"], got["p_max"]) > 1.0 and max(got["v_2"], got["p_2"]) > 1.0, (fault, sr.case_id(c), got)


def test_the_mean_bar_catches_a_mean_over_the_first_trip_only():
    """Fault l on the large shape's pressure vector alone: 68 880 > 256 x 256 entries, the mean's second grid-stride trip."""
    gp = int(np.prod(sr.idims(sr.LARGE)))
    assert gp > sr.MEAN_RB * sr.MEAN_RT
    p = np.random.default_rng(SEED + 5).standard_normal(gp)
    good, bad = sr.remove_mean(p), sr.remove_mean(p, first=sr.MEAN_RB * sr.MEAN_RT)
    print("fault l  mean / bar: unfaulted %.3g, faulted %.3g" % (float(sr.mean_of(good) / sr.mean_bar(good)), float(sr.mean_of(bad) / sr.mean_bar(bad))))
    assert sr.mean_of(good) <= sr.mean_bar(good)
    assert sr.mean_of(bad) > sr.mean_bar(bad)
    assert sr.t_mean(gp) == 2 + 16 and sr.t_mean(65536) == 1 + 16
