"""The deflated solve of singular VarHelmholtz problems on the host (no device): the null vectors of
cheb_varhelm_null_signs_host against the rank deficiency of the dense operator, the refusal of more than three even periodic
directions, the NumPy restatement of the method against the bordered solve, two planted faults that pass "converged" and fail a
bar, and the rounding counts of the bars."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import varhelm_ref as vr
import varhelm_singular_ref as sr

sp = ge.load()
U = sr.U
SEED = 20261021

NEU = "neumann"
# (dims, bc, scale, q)
SHAPES = {
    "6x7x5": ((6, 7, 5), [NEU] * 3, None, 1),
    "8x7": ((8, 7), ["periodic", NEU], (0.5, 1.0), 2),
    "9x6": ((9, 6), ["periodic", NEU], None, 1),
    "4x6x6": ((4, 6, 6), ["periodic", "periodic", NEU], None, 4),
}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ge.build()
    return sp.lib()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_null_signs_against_the_dense_operator(name):
    dims, bc, scale, q = SHAPES[name]
    p = sr.problem(sp, dims, bc, scale)
    flags = sp.null_signs(p.dims, p.periodic)
    assert len(flags) == q and flags[0] == 0 and len(set(flags)) == q
    N = sr.null_matrix(sp, p)
    assert N.shape == (p.G, q) and np.array_equal(np.abs(N), np.ones((p.G, q)))
    assert np.array_equal(N.T @ N, p.G * np.eye(q)), "mutually orthogonal"
    # brute force: every product of (-1)^index over a subset of the even periodic directions, in the order of the subsets' bits
    even = [k for k in range(p.d) if p.periodic[k] and p.dims[k] % 2 == 0]
    idx = np.indices(p.M)
    for j in range(q):
        par = sum(idx[even[b]] for b in range(len(even)) if j >> b & 1)
        assert np.array_equal(N[:, j], ((-1.0) ** (par + np.zeros(p.M))).reshape(-1))
        assert flags[j] == sum(1 << even[b] for b in range(len(even)) if j >> b & 1)
    A = p.dense()[0]
    sv = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    assert int((sv <= 1e-9 * sv[0]).sum()) == q, "rank deficiency %d, expected %d" % ((sv <= 1e-9 * sv[0]).sum(), q)
    for j in range(q):                                           # |A z| at the operator's own rounding (the end values are doubles)
        t, W = p.apply(N[:, j])
        assert np.all(np.abs(t.astype(np.float64)) <= p.cap * U * W)


def test_more_than_three_even_periodic_directions_are_refused(_lib):
    L = _lib
    ints = lambda v: (C.c_int * len(v))(*v)
    flags = (C.c_int * 8)()
    assert L.cheb_varhelm_null_signs_host(4, ints([4, 6, 8, 4]), ints([1, 1, 1, 1]), flags) == -4
    assert b"more than three" in L.chebhip_last_error()
    assert L.cheb_varhelm_null_signs_host(5, ints([4, 6, 8, 5, 7]), ints([1, 1, 1, 1, 0]), flags) == 8      # an odd extent adds none
    assert [flags[j] for j in range(8)] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert L.cheb_varhelm_null_signs_host(3, ints([4, 6, 8]), None, flags) == 1 and flags[0] == 0
    assert L.cheb_varhelm_null_signs_host(0, ints([4]), None, flags) == -4
    assert L.cheb_varhelm_null_signs_host(1, None, None, flags) == -4
    assert L.cheb_varhelm_null_signs_host(1, ints([4]), None, None) == -4
    with pytest.raises(sp.ChebhipError) as e:
        sp.null_signs((4, 4, 4, 4, 5), (True, True, True, True, False))
    assert e.value.code == 4 and "more than three" in str(e.value)
    # the entry points that take a handle, without one
    assert L.cheb_varhelm_solve_deflated(None, None, None, None, 0, None, 1e-8, 0.0, 10, 30, None) == 4
    assert L.cheb_varhelm_remove_null(None, None, None, None) == 4
    assert L.cheb_varhelm_apply_deflated(None, None, None, None) == 4
    assert L.cheb_varhelm_precond_deflated(None, None, None, None) == 4
    assert L.cheb_varhelm_defect(None, None) == 4
    assert L.cheb_varhelm_null_count(None) == -1


def setup(name, amp=0.9, consistent=False):
    dims, bc, scale, q = SHAPES[name]
    p = sr.problem(sp, dims, bc, scale, amp)
    N = sr.null_matrix(sp, p)
    A = p.dense()[0]
    rng = np.random.default_rng(SEED)
    b = rng.standard_normal(p.G)
    if consistent:                                               # b in the range of A: the faulty projections still converge
        b = (A @ rng.standard_normal(p.G).astype(sr.LD)).astype(np.float64)
    return p, N, A, b


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("amp", [0.0, 0.9])
def test_method_against_the_bordered_solve(name, amp):
    p, N, A, b = setup(name, amp)
    q = N.shape[1]
    Hs = sr.dropped_mode_solve(sp, p)
    x, its, ok, res = sr.deflated_gmres(A, N, Hs, p.kappa[p.inner].reshape(-1), b)
    print("%s amp %.1f: %d iterations, recurrence residual %.2e" % (name, amp, its, res))
    assert ok and its <= (2 if amp == 0.0 else 100)
    r = (b.astype(sr.LD) - A @ x.astype(sr.LD)).astype(np.float64)
    pr, pb = sr.project(N, r), sr.project(N, b)
    assert np.linalg.norm(pr) <= 1.05e-10 * np.linalg.norm(pb)
    assert np.all(np.abs(N.T @ x) <= sr.bar3(x, p.G, q))
    B, Binv, cond = sr.bordered(A, N)
    xs, lam = sr.bordered_solve(A, N, b)
    assert np.all(np.abs(x - xs) <= sr.bar4(Binv, cond, N, pr, x, xs))
    assert np.all(np.abs(N.T @ r / p.G - lam) <= np.abs(Binv[p.G:, :p.G]) @ np.abs(pr) + 16.0 * U * cond * np.abs(lam).max() + sr.bar5(r, p.G))
    if amp == 0.0:                                               # kappa == 1: the preconditioner is the solve
        assert np.all(np.abs(x - sr.project(N, Hs @ b)) <= sr.bar4(Binv, cond, N, pr, x, xs))
        # Pi H# is the leading block of the bordered inverse; H# alone leaves a null-space part
        assert np.abs(sr.project(N, Hs) - Binv[:p.G, :p.G]).max() <= 1e-9 * np.abs(Binv).max()


@pytest.mark.parametrize("plant", ["ones_only", "no_last_pi"])
def test_planted_fault_converges_and_fails_a_bar(plant):
    name = "8x7" if plant == "ones_only" else "4x6x6"
    p, N, A, b = setup(name, consistent=True)
    q = N.shape[1]
    Hs = sr.dropped_mode_solve(sp, p)
    ku = p.kappa[p.inner].reshape(-1)
    # a warm start whose constant is far from 0 (a pressure of the step before): Pi x0 keeps a null-space part at the rounding of
    # |x0|, which only the last Pi, taken at the size of x, removes
    x0 = None if plant == "ones_only" else 1e6 + np.random.default_rng(SEED + 1).standard_normal(p.G)
    good = sr.deflated_gmres(A, N, Hs, ku, b, x0=x0)
    bad = sr.deflated_gmres(A, N, Hs, ku, b, plant=plant, x0=x0)
    assert good[2] and bad[2], "both report convergence"
    assert np.all(np.abs(N.T @ good[0]) <= sr.bar3(good[0], p.G, q))
    worst = (np.abs(N.T @ bad[0]) / sr.bar3(bad[0], p.G, q)).max()
    print("%s: |N^T x| at %.3g of bar 3" % (plant, worst))
    assert worst > 1.0, "bar 3 must catch %s" % plant


def test_cap_count():
    assert sr.sum_depth(1) == sr.sum_depth(1 << 18) == 2 + 17
    assert sr.sum_depth((1 << 18) + 1) == 4 + 17
    assert sr.sum_depth(68880) == 19 and sr.sum_depth(66 * 32 * 64) == 19
    x = np.ones(10)
    assert sr.bar3(x, 10, 4) == (19 + 4 + 4) * U * 10.0
    assert sr.bar5(x, 10) == (19 + 2) * U * 10.0 / 10
