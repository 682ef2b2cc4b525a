"""The reference of the Krylov tests held to its own bars (krylov_ref.py), on the CPU: the cases of test_gpu_krylov_steps.py at reduced n.

  a. both double restatements of the solve pass every step bar on every case (their own observed sums included), end with the
     long-double solve's iteration count and reason, and define a whole-solve bar that is not degenerate;
  b. a different fixed summation order (pairwise from the far end) passes the same bars;
  c. each planted fault fails a bar (or ends the solve at another iteration count) on every case it can show on.  Whether the
     criterion the suite had before (the solve converges and its true residual is within 1.05 rtol |b|; here rtol 1e-8, restart 16,
     n = 257, the fixed preconditioner; the clean solve takes 11 iterations) would have let the fault through:

         a  dots skip the last element of an odd n             passes the old criterion, 11 iterations
         b  dots skip everything past the first trip            passes, 11 iterations
         c  c_i = d_i / rn_i                                    passes, 11 iterations (rn is 1 to rounding until e2 clamps)
         d  x += V y where x += Z y is due                      fails (reports convergence, the true residual is not)
         e  w.w of the previous iteration at j + 1 = 8, 16      passes, 11 iterations
         f  the reduced dots ignored                            passes, 80 iterations

     Five of six pass, one at seven times the iterations.  The stored-vector bar catches a, b, f, and c on the clamping operator;
     the whole-solve bar catches d, and e where the estimated last column of a cycle is the one with j + 1 a multiple of 8.

Worst ratios of the two restatements against the caps (every case): first vector 0.11, stored vector 0.69, observed dots 0.10, nsq 0.07,
|V| - 1 on the three-launch step 0.06, the norms' sums 0.10; the other summation order: 0.71 at most, 0.09 and 0.16 of the whole-solve
and residual bars."""
import numpy as np
import pytest

import krylov_ref as kr

LD = kr.LD
SEED = 20250301
HOST_N = {4097: 257, 4098: 258, 262921: 1031, 530434: 2050}
TRIP = 200                         # elements of the "first trip" of fault b at these sizes
ALL = kr.CASES + kr.ILL_CASES
_REF = {}


def setup(c):
    n = HOST_N.get(c[1], c[1])
    return kr.case_setup(c, SEED, n)


def reference(c):
    """(op, b, x0, long-double solve, [restatements]) of a case: computed once, shared, never changed."""
    if c not in _REF:
        op, b, x0 = setup(c)
        ld, rest = kr.reference_solves(op, b, x0, c[2], c[3], c[4], 2 if c[5] == "double" else 1)
        _REF[c] = (op, b, x0, ld, rest)
    return _REF[c]


def run(c, **kw):
    op, b, x0, ld, rest = reference(c)
    A, M = op.callables(np.float64)
    return kr.fgmres(A, M, b, x0, c[2], c[3], exact=c[4], dup=2 if c[5] == "double" else 1, trace=True, **kw)


def bars(c, q):
    """Every ratio of a solve q of case c: the step bars and (not on the clamping operator) the whole-solve bar."""
    op, b, x0, ld, rest = reference(c)
    out = kr.check_trace(q["trace"], b, c[4], 2 if c[5] == "double" else 1, bool(c[5]))
    if c[0] != "ill":
        out["solve_max"], out["solve_2"] = kr.solve_ratios(q["x"], ld["x"], [r["x"] for r in rest])
        if not ld["last_est"] and ld["its"] > 0:
            out["residual"] = kr.scalar_ratio(q["rnorm"], ld["rnorm"], [r["rnorm"] for r in rest])
    return out


@pytest.mark.parametrize("c", ALL, ids=kr.case_id)
def test_restatements_within_every_bar(c):
    op, b, x0, ld, rest = reference(c)
    n = b.size
    assert ld["its"] == (c[3] if n else 0) and ld["reason"] == (-3 if n else 3)
    for q in rest:
        assert (q["its"], q["reason"], q["last_est"]) == (ld["its"], ld["reason"], ld["last_est"])
        got = bars(c, q)
        assert all(v <= 1.0 for v in got.values()), got
    if n and c[0] != "ill":                       # the bar of the whole solve is a number, not 0 and not inf
        e = max(float(np.abs(q["x"].astype(LD) - ld["x"]).max()) for q in rest)
        assert 0.0 < e <= 1e-9 * float(np.abs(ld["x"]).max()), e


@pytest.mark.parametrize("c", [c for c in ALL if c[0] != "small"] + [kr.CASES[12]], ids=kr.case_id)
def test_another_fixed_summation_order_passes(c):
    got = bars(c, run(c, dot=kr.dot_reversed))
    assert all(v <= 1.0 for v in got.values()), got


def old_criterion(fault):
    """Would the suite's earlier check have passed a solver with this fault?  (converged, true residual <= 1.05 rtol |b|)"""
    n, rtol = 257, 1e-8
    op = kr.Op(n, SEED, prec="fixed")
    b = kr.rhs("normal", n, SEED + 1)
    A, M = op.callables(np.float64)
    q = kr.fgmres(A, M, b, None, 16, 2000, rtol=rtol, dup=2 if fault == "f" else 1, fault=fault, trip=TRIP)
    res = b.astype(LD) - op.A(q["x"].astype(LD), LD)
    ok = q["reason"] == 2 and float(np.sqrt((res * res).sum())) <= 1.05 * rtol * float(np.linalg.norm(b))
    return ok, q["its"]


# fault -> (the cases it can show on, the bars that must catch it)
FAULT_CASES = {
    "a": ([c for c in ALL if HOST_N.get(c[1], c[1]) % 2 == 1 and c[1] > 3 and c[0] != "small"], ("stored",)),
    "b": ([c for c in ALL if c[0] in ("medium", "big")], ("stored",)),
    "c": (kr.ILL_CASES, ("stored",)),
    "d": ([c for c in ALL if c[6] and c[0] in ("medium", "big")], ("solve_max", "solve_2")),
    "e": ([c for c in ALL if c[2] == 8 and not c[4]], ("solve_max", "solve_2")),
    "f": ([c for c in ALL if c[5] == "double" and c[0] in ("medium", "big", "ill")], ("stored",)),
}


@pytest.mark.parametrize("fault", sorted(kr.FAULTS))
def test_planted_fault_fails_a_bar(fault):
    cases, keys = FAULT_CASES[fault]
    assert cases
    for c in cases:                                # every case the fault can show on catches it, on the bar named for it
        q = run(c, fault=fault, trip=TRIP)
        got = bars(c, q)
        ld = reference(c)[3]
        stopped = (q["its"], q["reason"]) != (ld["its"], ld["reason"])      # (fault b on an impulse past the first trip: |b| = 0)
        assert stopped or any(got[k] > 1.0 for k in keys), (kr.case_id(c), got)
    passed_before, its = old_criterion(fault)
    print("fault %s (%s): old criterion %s, %d iterations" % (fault, kr.FAULTS[fault], "passes" if passed_before else "fails", its))
    if fault in "abc":
        assert passed_before                       # the gap: these cost iterations, not correctness


def test_clean_solver_meets_the_old_criterion():
    ok, its = old_criterion(None)
    assert ok and 0 < its < 100


def test_counts():
    """The counts the bars rest on, at the sizes of the route table."""
    assert kr.trips(262144, kr.RB * kr.ST) == 1 and kr.trips(262921, kr.RB * kr.ST) == 2
    assert kr.trips(524288, kr.RB * kr.ST, True) == 2 and kr.trips(530434, kr.RB * kr.ST, True) == 3      # pairs, + 1 for the half-sums
    assert kr.t_dot(4097, "gs") == 1 + 6 + 16 + 10 + 1 and kr.t_dot(4098, "gs") == 2 + 6 + 16 + 10 + 1
    assert kr.t_dot(4097, "three") == 1 + 6 + 16 + 256 + 1 and kr.t_dot(4097, "norm") == 1 + 6 + 4 + 10 + 1
    assert kr.step_counts(4097, False, False)[2] == 2 * 34 + 4 and kr.eigen_cap(4097) == 40
