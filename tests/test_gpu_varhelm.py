"""VarHelmholtz on the device against the long-double restatement varhelm_ref.py.

  mult / residual   per element under the bar cap 2^-53 A of varhelm_ref (cap = 2 (K + 8) + M + d + 6, a count) on the smallest shapes
                    that reach every route: the fused D(kappa D W) launch on lines of 2 .. 256 points (every matrix size class,
                    strided and contiguous, CGL and periodic), and the two-sweep route, which only the 258-point lines take: a
                    contiguous one with one field (6, 5, 258) and a strided one with three (4, 258, 3), whose launches read the
                    stacked kappa copies and the gradient work grid; mixed faces, scales, 1 / 3 / 16 stacked fields;
                    N(0,1), node-scaled, impulse and constant inputs; data given and None; c scalar, field and 0; 8-byte offsets.
  containment       a NaN / +Inf in one field leaves the other fields' bits alone; the same call gives the same bits, on another
                    stream too; a clean call after a NaN call gives a fresh handle's bits.
  identities        kappa == 1, c == sigma: mult under the bar, solve in at most 2 iterations, precond after mult and mult after
                    precond the identity, precond the bits of HelmholtzSolver(sigma).solve;
                    all-Dirichlet, unit scale, c = 0: EllipticOp.mult in the state eta = kappa, within the sum of both bars.
  solves            tiny shapes against the dense long-double assembly; refusals of singular problems; repeatability; x0.
  manufactured      u* of degree 2, kappa of degree 1 per wall direction, sin(pi x) on periodic ones: u* at every node.
  arguments         bad kappa / c, aliasing, wrong sizes, calls before set_coefficients.

Where VARHELM_RATIOS_OUT names a file the worst measured ratio per shape is written there (profiles/varhelm/ratios.txt)."""
import copy
import functools
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import callbacks_ref as cb
import linewise as lw
import varhelm_ref as vr

pytestmark = pytest.mark.gpu
sp = ge.load()
solve_mod = import_module(sp.__name__ + ".solve")
LD = np.longdouble
U = 2.0 ** -53
SEED = 20261020
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("VARHELM_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |y - truth| / (2^-53 A) per shape over its variants (tests/test_gpu_varhelm.py); cap = 2 (K + 8) + M + d + 6\n")
            for key in sorted(RATIOS):
                f.write("%-44s worst %8.3f  cap %4d\n" % (key, RATIOS[key][0], RATIOS[key][1]))


def dev(a, offset8=False):
    """A device copy; offset8: at an address that is 8 but not 16 bytes aligned."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if not offset8:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    t = buf[1:] if buf.data_ptr() % 16 == 0 else buf[:-1]
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 8
    return t


def new(n, offset8=False):
    return dev(np.full(int(n), np.nan), offset8)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


MIXED3 = ["dirichlet", "neumann", ("dirichlet", "neumann")]
ROBIN3 = [(1.0, 2.0), ("neumann", "dirichlet"), "dirichlet"]
# (dims, bc, scale, nfields)
BAR_CASES = [
    ((3, 3, 3), MIXED3, None, 16),
    ((5, 4, 6), ROBIN3, (0.5, 1.0, 2.0), 3),
    ((12,), [("neumann", (1.0, 0.5))], None, 16),
    ((9, 8), [((1.0, 2.0), (0.0, 1.0)), "dirichlet"], (0.5, 1.0), 3),
    ((66, 7, 9), MIXED3, None, 3),
    ((9, 130, 6), ROBIN3, (0.5, 1.0, 2.0), 1),
    ((6, 5, 258), MIXED3, None, 1),
    ((4, 258, 3), ROBIN3, (0.5, 1.0, 2.0), 3),
    ((34, 36, 40), MIXED3, (0.5, 1.0, 2.0), 1),
    ((34, 36, 40), ROBIN3, None, 3),
    ((2, 5, 4), ["periodic", (1.0, 2.0), ("dirichlet", "neumann")], None, 16),
    ((8, 7, 6), ["periodic", "neumann", "periodic"], (0.5, 1.0, 2.0), 3),
    ((256, 4, 3), ["periodic", "neumann", "dirichlet"], None, 1),
]
case_id = lambda c: "%s-%s-nf%d" % ("x".join(map(str, c[0])), "box" if c[2] else "cube", c[3])
# (x, g, kappa scaled per node, c, 8-byte offsets)
VARIANTS = [("noise", "given", False, "field", False), ("scaled", None, True, 1.5, False),
            ("impulse", "scaled", False, 0.0, True), ("constant", "given", True, "field", True)]


def make_inputs(p, nf, kind, gkind, seed):
    rng = np.random.default_rng(seed)
    n = nf * p.G
    if kind == "noise":
        x = rng.standard_normal(n)
    elif kind == "scaled":
        x = vr.node_scaled(n, seed + 1)
    elif kind == "impulse":
        x = np.zeros(n)
        x[(np.arange(nf) * p.G) + rng.integers(0, p.G, size=nf)] = 1.0
    else:
        x = np.repeat(rng.standard_normal(nf), p.G)
    g = None
    if p.NB and gkind == "given":
        g = rng.standard_normal(nf * p.NB)
    elif p.NB and gkind == "scaled":
        g = vr.node_scaled(nf * p.NB, seed + 2)
    f = rng.standard_normal(n) * (np.abs(x).max() if kind == "scaled" else 1.0)
    return x, g, f


def make_problem(dims, bc, scale, kscaled, c):
    per = sp.bc_split(bc, len(dims))[0]
    kap = vr.kappa_field(dims, per, 0.9, SEED + 5 if kscaled else None)
    return vr.Problem(sp, dims, bc, scale, kap, vr.c_field(dims, per) if isinstance(c, str) else c)


def set_coef(op, p, c):
    op.set_coefficients(dev(p.kappa), dev(p.c) if isinstance(c, str) else c)


@pytest.mark.parametrize("case", BAR_CASES, ids=case_id)
def test_mult_and_residual_under_the_bar(case):
    dims, bc, scale, nf = case
    op = sp.VarHelmholtz(dims, nf, bc=bc, scale=scale)
    worst = 0.0
    try:
        assert op.work_bytes() > 0
        for v, (kind, gkind, kscaled, c, off) in enumerate(VARIANTS):
            p = make_problem(dims, bc, scale, kscaled, c)
            assert (op.size, op.full_size, op.boundary_size) == (nf * p.G, nf * p.N, nf * p.NB)
            set_coef(op, p, c)
            x, g, f = make_inputs(p, nf, kind, gkind, SEED + 10 * v)
            xd, fd, gd = dev(x, off), dev(f, off), None if g is None else dev(g, off)
            y = host(op.mult(xd, new(op.size, off)))
            t, A = p.apply(x, None, None, nf)
            r = lw.worst(y, t, A)[0]
            print("%s %s mult: %.3f of cap %d" % (case_id(case), kind, r, p.cap))
            lw.check(y, t, A, p.cap, "mult %s" % kind)
            worst = max(worst, r)
            y = host(op.residual(xd, fd, gd, new(op.size, off)))
            t, A = p.apply(x, g, f, nf)
            r = lw.worst(y, t, A)[0]
            print("%s %s residual: %.3f of cap %d" % (case_id(case), kind, r, p.cap))
            lw.check(y, t, A, p.cap, "residual %s" % kind)
            worst = max(worst, r)
        RATIOS[case_id(case)] = (worst, p.cap)
    finally:
        op.destroy()


@pytest.mark.parametrize("case", [BAR_CASES[1], ((34, 36, 40), ROBIN3, None, 3), ((8, 7, 6), ["periodic", "neumann", "periodic"], (0.5, 1.0, 2.0), 3), ((4, 258, 3), ROBIN3, None, 3)], ids=case_id)
def test_containment_and_repeatability(case):
    dims, bc, scale, nf = case
    p = make_problem(dims, bc, scale, False, "field")
    x, g, f = make_inputs(p, nf, "noise", "given", SEED + 77)
    op, fresh = sp.VarHelmholtz(dims, nf, bc=bc, scale=scale), sp.VarHelmholtz(dims, nf, bc=bc, scale=scale)
    try:
        set_coef(op, p, "field"); set_coef(fresh, p, "field")
        xd, fd, gd = dev(x), dev(f), dev(g) if g is not None else None
        clean = host(fresh.residual(xd, fd, gd, new(op.size))).copy()
        clean_m = host(fresh.mult(xd, new(op.size))).copy()
        assert np.array_equal(host(op.residual(xd, fd, gd, new(op.size))), clean), "two handles, the same bits"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ys = op.residual(xd, fd, gd, new(op.size))
        side.synchronize()
        assert np.array_equal(host(ys), clean), "another stream, the same bits"
        for bad in (np.nan, np.inf):
            for j in sorted({0, nf - 1}):
                xb = x.copy()
                xb[j * p.G + p.G // 2] = bad
                y = host(op.residual(dev(xb), fd, gd, new(op.size))).reshape(nf, p.G)
                ym = host(op.mult(dev(xb), new(op.size))).reshape(nf, p.G)
                for q in range(nf):
                    if q != j:
                        assert np.array_equal(y[q], clean.reshape(nf, p.G)[q]) and np.array_equal(ym[q], clean_m.reshape(nf, p.G)[q])
                assert not np.all(np.isfinite(y[j]))
                assert np.array_equal(host(op.residual(xd, fd, gd, new(op.size))), clean), "a clean call after a NaN call"
                assert np.array_equal(host(op.mult(xd, new(op.size))), clean_m)
    finally:
        op.destroy(); fresh.destroy()


@pytest.mark.parametrize("dims", [(9, 8, 7), (6, 5, 98)], ids=lambda d: "x".join(map(str, d)))
def test_new_coefficients_give_a_fresh_handles_bits(dims):
    """set_coefficients on a handle that has already solved with another shift leaves nothing of the old one behind."""
    nf = 2
    p = make_problem(dims, MIXED3, None, False, "field")
    r = dev(np.random.default_rng(SEED + 88).standard_normal(nf * p.G))
    op, fresh = sp.VarHelmholtz(dims, nf, bc=MIXED3), sp.VarHelmholtz(dims, nf, bc=MIXED3)
    try:
        op.set_coefficients(dev(vr.kappa_field(dims, p.periodic, 0.5)), 3.0)
        op.precond(r, new(op.size)); op.mult(r, new(op.size))
        set_coef(op, p, "field"); set_coef(fresh, p, "field")
        assert op.sigma == fresh.sigma > 0.0
        assert np.array_equal(host(op.precond(r, new(op.size))), host(fresh.precond(r, new(op.size))))
        assert np.array_equal(host(op.mult(r, new(op.size))), host(fresh.mult(r, new(op.size))))
        # ... and equals a direct solve CREATED at that shift: at kappa == 1 the division is exact and precond is that solve
        sigma = 0.75
        hs = sp.HelmholtzSolver(dims, sigma, nfields=nf, bc=MIXED3)
        try:
            op.set_coefficients(dev(np.ones(dims)), sigma)
            assert op.sigma == sigma
            assert np.array_equal(host(op.precond(r, new(op.size))), host(hs.solve(r, new(op.size))))
        finally:
            hs.destroy()
    finally:
        op.destroy(); fresh.destroy()


# ---- identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((7, 6, 8), MIXED3, (0.5, 1.0, 2.0), 1), ((8, 7, 6), ["periodic", "neumann", "periodic"], None, 3)], ids=case_id)
def test_unit_kappa_is_the_direct_solve(case):
    dims, bc, scale, nf = case
    sigma = 0.75
    p = vr.Problem(sp, dims, bc, scale, None, sigma)
    op = sp.VarHelmholtz(dims, nf, bc=bc, scale=scale)
    try:
        op.set_coefficients(dev(p.kappa), sigma)
        assert op.sigma == sigma and not op.singular
        x, g, f = make_inputs(p, nf, "noise", "given", SEED + 31)
        xd = dev(x)
        y = op.mult(xd, new(op.size))
        t, A = p.apply(x, None, None, nf)
        lw.check(host(y), t, A, p.cap, "mult at kappa = 1")
        # precond after mult: z - x = [H^-1 on the device - H^-1](y) + H^-1 (y - truth).  The second term is within |H^-1| cap 2^-53 A;
        # the first is held to 16 x the largest error of NumPy's double dense solve of the same system (the margin of the solver's tests).
        z = host(op.precond(y, new(op.size))).reshape(nf, p.G)
        H = p.dense()[0].astype(np.float64)
        Hinv = np.abs(np.linalg.inv(H))
        for j in range(nf):
            xj = x.reshape(nf, p.G)[j]
            tj = t.reshape(nf, p.G)[j].astype(np.float64)
            e_np = np.abs(np.linalg.solve(H, tj) - xj).max()
            bound = Hinv @ (p.cap * U * A.reshape(nf, p.G)[j]) + 16.0 * e_np
            assert np.all(np.abs(z[j] - xj) <= bound), "precond(mult(x)) != x: worst %.3g of its bound" % (np.abs(z[j] - xj) / bound).max()
        # mult after precond: y - r = [mult on the device - A](z) + A (z - H^-1 r), z the device's precond(r).  The first term is the
        # operator's bar at z; the second is |A| times the solver's error, held to 16 x that of NumPy's dense solve (measured against a
        # long-double refinement of it): the sum of the two bars.
        rr = np.random.default_rng(SEED + 32).standard_normal(nf * p.G)
        zd = op.precond(dev(rr), new(op.size))
        y2 = host(op.mult(zd, new(op.size))).reshape(nf, p.G)
        t2, A2 = p.apply(host(zd), None, None, nf)
        Hld = p.dense()[0]
        absH = np.abs(H).sum(axis=1)
        for j in range(nf):
            rj = rr.reshape(nf, p.G)[j]
            z0 = np.linalg.solve(H, rj)
            zref = z0.astype(LD) + np.linalg.solve(H, (rj.astype(LD) - np.dot(Hld, z0.astype(LD))).astype(np.float64)).astype(LD)
            e_np = float(np.abs(z0.astype(LD) - zref).max())
            bound = p.cap * U * A2.reshape(nf, p.G)[j] + 16.0 * e_np * absH
            err = np.abs(y2[j] - rj)
            print("%s field %d: mult(precond(r)) - r worst %.3g of its bound" % (case_id(case), j, (err / bound).max()))
            assert np.all(err <= bound)
        xs = op.solve(dev(f), None if g is None else dev(g), rtol=1e-10, max_it=20)
        assert op.reason == 2 and op.iterations <= 2, (op.reason, op.iterations)
        r = p.apply(host(xs), g, f, nf)[0].astype(np.float64)
        b = p.apply(np.zeros(nf * p.G), g, f, nf)[0].astype(np.float64)
        assert np.linalg.norm(r) <= 1.05e-10 * np.linalg.norm(b)
    finally:
        op.destroy()


@pytest.mark.parametrize("dims", [(9, 8, 7), (34, 36, 40), (6, 130, 5)], ids=lambda d: "x".join(map(str, d)))
def test_agrees_with_elliptic_op(dims):
    """All-Dirichlet, unit scale, c = 0: MatMult_Elliptic in a state whose eta array is kappa."""
    d = len(dims)
    p = make_problem(dims, ["dirichlet"] * d, None, False, 0.0)
    x = np.random.default_rng(SEED + 41).standard_normal(p.G)
    op, ell = sp.VarHelmholtz(dims, 1), sp.EllipticOp(dims)
    try:
        op.set_coefficients(dev(p.kappa), 0.0)
        ell.set_state(0, p.kappa.reshape(-1))
        ell.set_state(1, np.zeros(p.N))
        for k in range(d):
            ell.set_state(2 + k, np.zeros(p.N))
        xd = dev(x)
        yv, ye = host(op.mult(xd, new(p.G))), host(ell.mult(xd, new(p.G)))
        _, A = p.apply(x)
        We = cb.elliptic_weight(dims, x, eta=p.kappa)[0]
        assert np.all(np.abs(yv - ye) <= U * (p.cap * A + cb.cap_e(dims) * We))
    finally:
        op.destroy(); ell.destroy()


# ---- solves -------------------------------------------------------------------------------------------------------------------------
SOLVE_CASES = [
    ((7, 6, 8), MIXED3, None, (0.0, "field")),
    ((8, 7, 6), ["periodic", "neumann", "periodic"], (0.5, 1.0, 2.0), ("field",)),
    ((9, 8), [((1.0, 2.0), (0.0, 1.0)), "dirichlet"], (1.0, 0.7), (0.0, "field")),
    ((12,), [("neumann", (1.0, 0.5))], (1.3,), (0.0, "field")),
    ((6, 7, 5), ["neumann"] * 3, None, ("field",)),
]
solve_id = lambda c: "x".join(map(str, c[0]))


@functools.lru_cache(maxsize=None)
def solve_setup(i, c):
    dims, bc, scale, _ = SOLVE_CASES[i]
    p = make_problem(dims, bc, scale, False, c)
    x, g, f = make_inputs(p, 1, "noise", "given", SEED + 50 + i)
    A, lift = p.dense()
    b = f.astype(LD) + lift(g)
    return p, g, f, A, b


@pytest.mark.parametrize("i", range(len(SOLVE_CASES)), ids=lambda i: solve_id(SOLVE_CASES[i]))
def test_solve_against_dense_truth(i):
    dims, bc, scale, cs = SOLVE_CASES[i]
    rtol = 1e-10
    for c in cs:
        p, g, f, A, b = solve_setup(i, c)
        op = sp.VarHelmholtz(dims, 1, bc=bc, scale=scale)
        try:
            set_coef(op, p, c)
            fd, gd = dev(f), dev(g)
            u = new(op.full_size)
            x = op.solve(fd, gd, u_full=u, rtol=rtol, max_it=200, restart=64)
            its = op.iterations
            print("%s c=%s: %d iterations, recurrence residual %.3e" % (solve_id(SOLVE_CASES[i]), c, its, op.residual_norm))
            assert op.reason == 2
            xh = host(x)
            r = p.apply(xh, g, f)[0].astype(np.float64)                       # f - (operator at g)(x), long double
            bn = np.linalg.norm(b.astype(np.float64))
            assert np.linalg.norm(r) <= 1.05 * rtol * bn, "true residual %.3e |b|" % (np.linalg.norm(r) / bn)
            assert its <= 100
            # against the dense solve: |x - A^-1 b| <= |A^-1| |r| elementwise
            A64 = A.astype(np.float64)
            xt = np.linalg.solve(A64, b.astype(np.float64))
            assert np.all(np.abs(xh - xt) <= np.abs(np.linalg.inv(A64)) @ np.abs(r) + 16.0 * U * np.linalg.cond(A64) * np.abs(xt).max())
            # the full grid: unknown nodes are x bit for bit, boundary nodes the extension of x
            uf = host(u).reshape(dims)
            assert np.array_equal(uf[p.inner].reshape(-1), xh)
            ue = p.extend_full(xh, g, LD)
            pa = copy.copy(p)                                                # the same extension with every factor's absolute value
            pa.Q = [None if Q is None else np.abs(Q) for Q in p.Q]
            pa.Binv = [None if B is None else np.abs(B) for B in p.Binv]
            Ba = pa.extend_full(np.abs(xh), np.abs(g))
            assert np.all(np.abs(uf - ue.astype(np.float64)) <= p.d * (max(p.M) + 2) * U * Ba), "the boundary nodes are the extension of x"
            # the same solve twice: the same bits; from the solution: no iteration
            x2 = op.solve(fd, gd, rtol=rtol, max_it=200, restart=64)
            assert np.array_equal(host(x2), xh) and op.iterations == its
            x3 = op.solve(fd, gd, x0=x, rtol=rtol, max_it=200, restart=64)
            assert op.iterations == 0 and op.reason == 2 and np.array_equal(host(x3), xh)
        finally:
            op.destroy()


@pytest.mark.parametrize("i", [1, 4], ids=lambda i: solve_id(SOLVE_CASES[i]))
def test_singular_solve_is_refused_and_mult_still_works(i):
    dims, bc, scale, _ = SOLVE_CASES[i]
    p = make_problem(dims, bc, scale, False, 0.0)
    x, g, f = make_inputs(p, 1, "noise", "given", SEED + 60 + i)
    op = sp.VarHelmholtz(dims, 1, bc=bc, scale=scale)
    try:
        op.set_coefficients(dev(p.kappa), 0.0)
        assert op.singular and op.sigma == 0.0
        with pytest.raises(sp.ChebhipError) as e:
            op.solve(dev(f), dev(g))
        assert e.value.code == 4 and "singular" in str(e.value)
        t, A = p.apply(x)
        lw.check(host(op.mult(dev(x), new(op.size))), t, A, p.cap, "mult of a singular problem")
        t, A = p.apply(x, g, f)
        lw.check(host(op.residual(dev(x), dev(f), dev(g), new(op.size))), t, A, p.cap, "residual of a singular problem")
        op.set_coefficients(dev(p.kappa), 1e-3)                              # the same handle with c > 0 solves
        assert not op.singular
        op.solve(dev(f), dev(g), rtol=1e-10, restart=64)
        assert op.reason == 2
    finally:
        op.destroy()


def test_operator_and_preconditioner_in_a_callers_fgmres():
    dims, bc, scale, _ = SOLVE_CASES[0]
    p, g, f, A, b = solve_setup(0, "field")
    op = sp.VarHelmholtz(dims, 1, bc=bc, scale=scale)
    ks = sp.Fgmres(op.size, restart=64, rtol=1e-10, atol=0.0, max_it=200)
    try:
        set_coef(op, p, "field")
        fd, gd = dev(f), dev(g)
        bd = op.residual(dev(np.zeros(p.G)), fd, gd, new(op.size))
        x = ks.solve(op, bd, new(op.size), M=op, m_entry="precond")
        xs = op.solve(fd, gd, rtol=1e-10, max_it=200, restart=64)
        assert ks.reason == 2 and ks.iterations == op.iterations
        assert np.array_equal(host(x), host(xs)), "solve is FGMRES on mult and precond, nothing else"
        # another restart length replaces the Krylov bases: one set at a time
        wb = op.work_bytes()
        op.solve(fd, gd, rtol=1e-10, max_it=200, restart=8)
        assert op.reason in (2, -3) and op.work_bytes() == wb - 2 * (64 - 8) * op.size * 8
    finally:
        ks.destroy(); op.destroy()


# ---- manufactured boundary-value problem ----------------------------------------------------------------------------------------------
def manufactured(p):
    """(u*, f, g) on the full grid: u* = prod_k p_k(x_k), kappa = prod_k q_k(x_k); wall: p = 1 + 0.3 x + 0.5 x^2, q = 1 + 0.4 x;
    periodic: p = 2 + sin(pi x), q = 1.  f = c u - sum_k s_k^2 (q_k p_k')' prod_{m != k} q_m p_m; g from the faces' conditions with
    the outward derivative (+d/dx at index 0, x = +1; -d/dx at the last index), at every boundary node from the highest direction
    in which it is an end node."""
    X = vr.grid(p.dims, p.periodic)
    P0, P1, P2, Q0, Q1 = [], [], [], [], []
    for k, x in enumerate(X):
        if p.periodic[k]:
            P0.append(2.0 + np.sin(np.pi * x)); P1.append(np.pi * np.cos(np.pi * x)); P2.append(-np.pi ** 2 * np.sin(np.pi * x))
            Q0.append(np.ones_like(x)); Q1.append(np.zeros_like(x))
        else:
            P0.append(1.0 + 0.3 * x + 0.5 * x * x); P1.append(0.3 + x); P2.append(np.ones_like(x))
            Q0.append(1.0 + 0.4 * x); Q1.append(0.4 * np.ones_like(x))
    u = np.prod(P0, axis=0)
    kappa = np.prod(Q0, axis=0)
    f = p.c * u
    for k in range(p.d):
        others = np.prod([Q0[m] * P0[m] for m in range(p.d) if m != k], axis=0) if p.d > 1 else 1.0
        f = f - p.scale[k] ** 2 * (Q1[k] * P1[k] + Q0[k] * P2[k]) * others
    gfull = np.zeros(p.dims)
    for k in range(p.d):                                                      # ascending: the highest direction writes last
        if p.periodic[k]:
            continue
        dudx = P1[k] * (np.prod([P0[m] for m in range(p.d) if m != k], axis=0) if p.d > 1 else 1.0)
        a0, b0, a1, b1 = p.ends[k]
        ix0, ix1 = [slice(None)] * p.d, [slice(None)] * p.d
        ix0[k], ix1[k] = 0, p.dims[k] - 1
        gfull[tuple(ix0)] = (a0 * u + b0 * p.scale[k] * dudx)[tuple(ix0)]
        gfull[tuple(ix1)] = (a1 * u - b1 * p.scale[k] * dudx)[tuple(ix1)]
    return u, kappa, f, gfull[p.bmask]


@pytest.mark.parametrize("i", [0, 1, 2], ids=lambda i: solve_id(SOLVE_CASES[i]))
def test_manufactured_solution_at_every_node(i):
    dims, bc, scale, _ = SOLVE_CASES[i]
    per = sp.bc_split(bc, len(dims))[0]
    p = vr.Problem(sp, dims, bc, scale, None, vr.c_field(dims, per))
    u, kappa, f, g = manufactured(p)
    p = vr.Problem(sp, dims, bc, scale, kappa, vr.c_field(dims, per))
    rtol = 1e-12
    # NumPy's double dense solve of the same system, extended to the full grid the same way
    A, lift = p.dense()
    A64 = A.astype(np.float64)
    b = (f[p.inner].reshape(-1).astype(LD) + lift(g)).astype(np.float64)
    e_np = np.abs(p.extend_full(np.linalg.solve(A64, b), g) - u).max()
    bound = 16.0 * e_np + rtol * np.linalg.norm(np.linalg.inv(A64), 2) * np.linalg.norm(b)
    uf, its = solve_mod.variable_diffusion(sp, dims, dev(kappa), dev(f), c=dev(p.c), bc=bc, g=dev(g), scale=scale, rtol=rtol, restart=64)
    err = np.abs(host(uf).reshape(dims) - u).max()
    print("%s: error %.3e, bound %.3e (NumPy's dense solve %.3e), %d iterations" % (solve_id(SOLVE_CASES[i]), err, bound, e_np, its))
    assert err <= bound
    assert 0 < its <= 100


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    dims, bc = (6, 5, 7), MIXED3
    p = make_problem(dims, bc, None, False, "field")
    op = sp.VarHelmholtz(dims, 2, bc=bc)
    try:
        n = op.size
        x, y = dev(np.ones(n)), new(n)
        for call in (lambda: op.mult(x, y), lambda: op.precond(x, y), lambda: op.solve(x), lambda: op.residual(x, x, None, y)):
            with pytest.raises(sp.ChebhipError) as e:
                call()
            assert e.value.code == 4 and "set_coefficients" in str(e.value)
        assert op.sigma == -1.0
        set_coef(op, p, "field")
        good = host(op.mult(x, new(n))).copy()
        for bad_k, bad_c in ((np.nan, None), (np.inf, None), (0.0, None), (-1.0, None), (None, -1e-300), (None, np.nan)):
            k, c = p.kappa.copy(), p.c.copy()
            if bad_k is not None:
                k[2, 1, 3] = bad_k
            if bad_c is not None:
                c[0, 0, 0] = bad_c
            with pytest.raises(sp.ChebhipError) as e:
                op.set_coefficients(dev(k), dev(c))
            assert e.value.code == 4
        for c in (-1.0, np.nan, np.inf):
            with pytest.raises(sp.ChebhipError):
                op.set_coefficients(dev(p.kappa), c)
        assert np.array_equal(host(op.mult(x, new(n))), good), "a refused set_coefficients leaves the handle as it was"
        buf = new(2 * n + op.boundary_size)
        for call in (lambda: op.mult(buf[:n], buf[n - 1:2 * n - 1]), lambda: op.mult(x, x), lambda: op.residual(x, buf[:n], None, buf[1:n + 1]),
                     lambda: op.residual(x, y, buf[:op.boundary_size], buf[:n])):
            with pytest.raises(sp.ChebhipError) as e:
                call()
            assert e.value.code == 4 and "alias" in str(e.value)
        big = dev(np.ones(n + op.full_size))
        with pytest.raises(sp.ChebhipError) as e:
            op.solve(big[:n], u_full=big[n - 1:n - 1 + op.full_size])
        assert e.value.code == 4 and "alias" in str(e.value)
        for call in (lambda: op.mult(x[:-1], y), lambda: op.mult(x, new(n + 1)), lambda: op.residual(x, x, new(3), y),
                     lambda: op.set_coefficients(dev(p.kappa)[:-1]), lambda: op.solve(x, u_full=new(n)), lambda: op.mult(x.cpu(), y),
                     lambda: op.mult(x.float(), y)):
            with pytest.raises(ValueError):
                call()
    finally:
        op.destroy()
    allp = sp.VarHelmholtz((8, 6), 1, bc=["periodic", "periodic"])
    try:
        assert allp.boundary_size == 0 and allp.size == allp.full_size
        allp.set_coefficients(dev(np.ones((8, 6))), 0.5)
        with pytest.raises(sp.ChebhipError):
            allp.residual(dev(np.ones(48)), dev(np.ones(48)), dev(np.ones(1)), new(48))
    finally:
        allp.destroy()
