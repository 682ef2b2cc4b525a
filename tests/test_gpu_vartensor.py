"""The tensor mode of VarHelmholtz on the device against the long-double restatement vartensor_ref.py.

  mult / residual   per element under the bar cap 2^-53 A of vartensor_ref (cap = 2 (K + 8) + w (M + 2) + 2 d + 3, a count), with and
                    without a velocity, c scalar, field and 0, N(0,1), node-scaled (10^+-30) and impulse inputs, data given and None,
                    8-byte offsets; on one unknown, on odd and even extents (odd stacked grids put every other field on an 8-byte
                    boundary), 2-D strided and contiguous 130-point lines, periodic directions and the 258-point lines.
  identity tensor   K = kappa I: mult within the sum of the tensor bar and the scalar bar; the solve in the scalar solve's iterations.
  containment       a NaN in one field leaves the other fields' bits; the same call, the same bits; set_tensor -> set_coefficients ->
                    set_tensor gives a fresh handle's bits in each mode; 8-byte-offset vectors give the aligned ones' bits.
  solves            at most 64 unknowns against the dense long-double assembly, anisotropy 10, with and without a velocity.
  manufactured      18 x 16 x 20, rotating K, a velocity, Dirichlet and Robin faces: u* at every node.
  singular          8 periodic x 9 Neumann x 6 periodic, c == 0: solve refuses, solve_deflated converges, bars 2 and 3 of DESIGN 10q.
  Fgmres            a caller's Fgmres on mult / precond gives solve's bits.
  arguments         d = 1 and 4, a node that is not positive definite, NaN in K and v, no K, mult before any setter.

Where VARTENSOR_RATIOS_OUT names a file the worst measured ratio per shape and the iteration counts are written there
(profiles/varhelm/tensor_ratios.txt)."""
import functools
import os
from importlib import import_module

import numpy as np
import pytest
import scipy.linalg
import torch

import __graft_entry__ as ge
import linewise as lw
import varhelm_ref as vr
import varhelm_singular_ref as sr
import vartensor_ref as vt

pytestmark = pytest.mark.gpu
sp = ge.load()
solve_mod = import_module(sp.__name__ + ".solve")
LD = np.longdouble
U = 2.0 ** -53
SEED = 20261021
RATIOS, NOTES = {}, []


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("VARTENSOR_RATIOS_OUT")
    if path and (RATIOS or NOTES):
        with open(path, "w") as f:
            f.write("# worst |y - truth| / (2^-53 A) per shape over its variants (tests/test_gpu_vartensor.py); cap = 2 (K + 8) + w (M + 2) + 2 d + 3\n")
            for key in sorted(RATIOS):
                f.write("%-44s worst %8.3f  cap %4d\n" % (key, RATIOS[key][0], RATIOS[key][1]))
            for line in NOTES:
                f.write(line + "\n")


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
ROBIN2 = [((1.0, 2.0), (0.0, 1.0)), ("dirichlet", "neumann")]
# (dims, bc, scale, nfields)
BAR_CASES = [
    ((3, 3, 3), MIXED3, None, 3),
    ((5, 4, 6), ROBIN3, (0.5, 1.0, 2.0), 3),
    ((5, 5, 7), MIXED3, None, 3),
    ((5, 4, 6), MIXED3, None, 1),
    ((34, 36, 40), MIXED3, (0.5, 1.0, 2.0), 1),
    ((8, 9, 6), ["periodic", (1.0, 2.0), "periodic"], (0.5, 1.0, 2.0), 3),
    ((7, 5, 4), ["periodic", "neumann", ("dirichlet", "neumann")], None, 1),
    ((9, 130), ROBIN2, (0.5, 1.0), 3),
    ((130, 9), ROBIN2, None, 1),
    ((6, 5, 258), MIXED3, None, 1),
    ((4, 258, 3), ROBIN3, (0.5, 1.0, 2.0), 3),
]
case_id = lambda c: "%s-%s-nf%d" % ("x".join(map(str, c[0])), "box" if c[2] else "cube", c[3])
# (x, g, velocity, c, 8-byte offsets)
VARIANTS = [("noise", "given", True, "field", False), ("scaled", None, False, 1.5, False),
            ("impulse", "scaled", True, 0.0, True), ("noise", "given", False, "field", True)]


def make_inputs(p, nf, kind, gkind, seed):
    rng = np.random.default_rng(seed)
    n = nf * p.G
    if kind == "noise":
        x = rng.standard_normal(n)
    elif kind == "scaled":
        x = vr.node_scaled(n, seed + 1)
    else:
        x = np.zeros(n)
        x[(np.arange(nf) * p.G) + rng.integers(0, p.G, size=nf)] = 1.0
    g = None
    if p.NB and gkind == "given":
        g = rng.standard_normal(nf * p.NB)
    elif p.NB and gkind == "scaled":
        g = vr.node_scaled(nf * p.NB, seed + 2)
    f = rng.standard_normal(n) * (np.abs(x).max() if kind == "scaled" else 1.0)
    return x, g, f


def make_problem(dims, bc, scale, vel, c, k=(1.0, 0.5, 2.0)):
    per = sp.bc_split(bc, len(dims))[0]
    return vt.TensorProblem(sp, dims, bc, scale, vt.rotating_tensor(dims, per, k), vt.velocity_field(dims, per) if vel else None,
                            vr.c_field(dims, per) if isinstance(c, str) else c)


def set_tensor(op, p, c):
    op.set_tensor(dev(p.K), dev(p.c) if isinstance(c, str) else c, None if p.vel is None else dev(p.vel))


@pytest.mark.parametrize("case", BAR_CASES, ids=case_id)
def test_mult_and_residual_under_the_bar(case):
    dims, bc, scale, nf = case
    op = sp.VarHelmholtz(dims, nf, bc=bc, scale=scale)
    worst = 0.0
    try:
        assert op.mode == 0
        wb0 = op.work_bytes()
        for v, (kind, gkind, vel, c, off) in enumerate(VARIANTS):
            p = make_problem(dims, bc, scale, vel, c)
            assert np.all(vt.minors_ok(p.K))
            assert (op.size, op.full_size, op.boundary_size) == (nf * p.G, nf * p.N, nf * p.NB)
            set_tensor(op, p, c)
            assert op.mode == 2
            # K and v once per handle, d gradient grids per field: made by the first set_tensor, then kept
            assert op.work_bytes() == wb0 + 8 * p.N * (len(p.order) + p.d + p.d * nf)
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


# ---- K = kappa I --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((7, 6, 8), MIXED3, (0.5, 1.0, 2.0), 1), ((8, 7, 6), ["periodic", (1.0, 2.0), "periodic"], None, 3),
                                  ((9, 8), ROBIN2, (1.0, 0.7), 1)], ids=case_id)
def test_identity_tensor_is_the_scalar_operator(case):
    dims, bc, scale, nf = case
    d = len(dims)
    per = sp.bc_split(bc, d)[0]
    kap, c = vr.kappa_field(dims, per, 0.5), vr.c_field(dims, per)
    K = np.stack([kap] * d + [np.zeros(dims)] * (d * (d - 1) // 2))
    pt, ps = vt.TensorProblem(sp, dims, bc, scale, K, None, c), vr.Problem(sp, dims, bc, scale, kap, c)
    x, g, f = make_inputs(pt, nf, "noise", "given", SEED + 21)
    op = sp.VarHelmholtz(dims, nf, bc=bc, scale=scale)
    try:
        xd, fd, gd = dev(x), dev(f), dev(g)
        op.set_coefficients(dev(kap), dev(c))
        assert op.mode == 1
        ys = host(op.mult(xd, new(op.size))).copy()
        op.solve(fd, gd, rtol=1e-10)
        its_s, sigma_s = op.iterations, op.sigma
        assert op.reason == 2
        op.set_tensor(dev(K), dev(c))
        assert op.mode == 2
        yt = host(op.mult(xd, new(op.size)))
        At, As = pt.apply(x, None, None, nf)[1], ps.apply(x, None, None, nf)[1]
        assert np.all(np.abs(yt - ys) <= U * (pt.cap * At + ps.cap * As)), "tensor and scalar mult differ by more than the sum of their bars"
        assert abs(op.sigma - sigma_s) <= 8 * U * sigma_s                     # kbar = (kappa + kappa [+ kappa]) / d: kappa to two roundings
        op.solve(fd, gd, rtol=1e-10)
        print("%s: %d iterations in the tensor mode, %d in the scalar mode" % (case_id(case), op.iterations, its_s))
        assert op.reason == 2 and abs(op.iterations - its_s) <= 1, (op.iterations, its_s)
    finally:
        op.destroy()


# ---- containment and repeatability ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((5, 4, 6), ROBIN3, (0.5, 1.0, 2.0), 3), ((5, 5, 7), MIXED3, None, 3), ((9, 130), ROBIN2, None, 3),
                                  ((4, 258, 3), ROBIN3, None, 3)], ids=case_id)
def test_containment_and_repeatability(case):
    dims, bc, scale, nf = case
    p = make_problem(dims, bc, scale, True, "field")
    x, g, f = make_inputs(p, nf, "noise", "given", SEED + 77)
    op, fresh = sp.VarHelmholtz(dims, nf, bc=bc, scale=scale), sp.VarHelmholtz(dims, nf, bc=bc, scale=scale)
    try:
        set_tensor(op, p, "field"); set_tensor(fresh, p, "field")
        xd, fd, gd = dev(x), dev(f), dev(g)
        clean = host(fresh.residual(xd, fd, gd, new(op.size))).copy()
        clean_m = host(fresh.mult(xd, new(op.size))).copy()
        assert np.array_equal(host(op.residual(xd, fd, gd, new(op.size))), clean), "two handles, the same bits"
        assert np.array_equal(host(op.residual(xd, fd, gd, new(op.size))), clean), "the same call, the same bits"
        assert np.array_equal(host(op.residual(dev(x, True), dev(f, True), dev(g, True), new(op.size, True))), clean), "8-byte offsets, the same bits"
        assert np.array_equal(host(op.mult(dev(x, True), new(op.size, True))), clean_m)
        for j in sorted({0, 1, nf - 1}):
            xb = x.copy()
            xb[j * p.G + p.G // 2] = np.nan
            y = host(op.residual(dev(xb), fd, gd, new(op.size))).reshape(nf, p.G)
            ym = host(op.mult(dev(xb), new(op.size))).reshape(nf, p.G)
            for q in range(nf):
                if q != j:
                    assert np.array_equal(y[q], clean.reshape(nf, p.G)[q]) and np.array_equal(ym[q], clean_m.reshape(nf, p.G)[q])
            assert not np.all(np.isfinite(y[j]))
            assert np.array_equal(host(op.residual(xd, fd, gd, new(op.size))), clean), "a clean call after a NaN call"
    finally:
        op.destroy(); fresh.destroy()


@pytest.mark.parametrize("dims", [(9, 8, 7), (6, 5, 98)], ids=lambda d: "x".join(map(str, d)))
def test_switching_modes_gives_a_fresh_handles_bits(dims):
    nf = 2
    p = make_problem(dims, MIXED3, None, True, "field")
    p2 = make_problem(dims, MIXED3, None, False, 3.0, (2.0, 1.0, 0.5))
    kap = vr.kappa_field(dims, p.periodic, 0.5)
    r = dev(np.random.default_rng(SEED + 88).standard_normal(nf * p.G))
    op, ft, fs = (sp.VarHelmholtz(dims, nf, bc=MIXED3) for _ in range(3))
    try:
        set_tensor(ft, p, "field")
        fs.set_coefficients(dev(kap), dev(p.c))
        ref = {}
        for name, h in (("tensor", ft), ("scalar", fs)):
            ref[name] = [host(h.mult(r, new(h.size))).copy(), host(h.precond(r, new(h.size))).copy(),
                         host(h.solve(r, rtol=1e-10, restart=20)).copy(), h.sigma, h.iterations]
        set_tensor(op, p2, 3.0)                                               # another tensor, without a velocity, first
        op.solve(r, rtol=1e-6, restart=20)
        for name in ("tensor", "scalar", "tensor"):
            if name == "tensor":
                set_tensor(op, p, "field")
            else:
                op.set_coefficients(dev(kap), dev(p.c))
            assert op.mode == (2 if name == "tensor" else 1) and op.sigma == ref[name][3]
            assert np.array_equal(host(op.mult(r, new(op.size))), ref[name][0]), name
            assert np.array_equal(host(op.precond(r, new(op.size))), ref[name][1]), name
            assert np.array_equal(host(op.solve(r, rtol=1e-10, restart=20)), ref[name][2]) and op.iterations == ref[name][4], name
    finally:
        op.destroy(); ft.destroy(); fs.destroy()


# ---- solves -------------------------------------------------------------------------------------------------------------------------
# (dims, bc, scale): at most 64 unknowns
SOLVE_CASES = [
    ((6, 5, 4), MIXED3, None),
    ((4, 5, 4), ["periodic", (1.0, 2.0), "periodic"], (0.5, 1.0, 2.0)),
    ((9, 8), ROBIN2, (1.0, 0.7)),
    ((6, 6, 5), ROBIN3, None),
]
solve_id = lambda c: "x".join(map(str, c[0]))


@functools.lru_cache(maxsize=None)
def solve_setup(i, vel):
    dims, bc, scale = SOLVE_CASES[i]
    p = make_problem(dims, bc, scale, vel, "field" if i % 2 else 0.0, (5.0, 0.5, 1.0))          # anisotropy 10
    assert p.G <= 64
    x, g, f = make_inputs(p, 1, "noise", "given", SEED + 50 + i)
    A, lift = p.dense()
    b = f.astype(LD) + lift(g)
    return p, g, f, A, b


@pytest.mark.parametrize("vel", [False, True], ids=["novel", "vel"])
@pytest.mark.parametrize("i", range(len(SOLVE_CASES)), ids=lambda i: solve_id(SOLVE_CASES[i]))
def test_solve_against_dense_truth(i, vel):
    dims, bc, scale = SOLVE_CASES[i]
    rtol = 1e-10
    p, g, f, A, b = solve_setup(i, vel)
    op = sp.VarHelmholtz(dims, 1, bc=bc, scale=scale)
    try:
        set_tensor(op, p, "field" if i % 2 else 0.0)
        fd, gd = dev(f), dev(g)
        u = new(op.full_size)
        x = op.solve(fd, gd, u_full=u, rtol=rtol, max_it=p.G, restart=p.G)          # full GMRES: it ends within G steps by construction
        its = op.iterations
        print("%s vel=%s: %d iterations of at most %d, recurrence residual %.3e" % (solve_id(SOLVE_CASES[i]), vel, its, p.G, op.residual_norm))
        NOTES.append("solve %-10s vel=%-5s anisotropy 10: %3d iterations (%d unknowns, full GMRES)" % (solve_id(SOLVE_CASES[i]), vel, its, p.G))
        assert op.reason == 2
        xh = host(x)
        r = p.apply(xh, g, f)[0].astype(np.float64)                           # f - (operator at g)(x), long double
        bn = np.linalg.norm(b.astype(np.float64))
        assert np.linalg.norm(r) <= 1.05 * rtol * bn, "true residual %.3e |b|" % (np.linalg.norm(r) / bn)
        A64 = A.astype(np.float64)
        xt = np.linalg.solve(A64, b.astype(np.float64))
        assert np.all(np.abs(xh - xt) <= np.abs(np.linalg.inv(A64)) @ np.abs(r) + 16.0 * U * np.linalg.cond(A64) * np.abs(xt).max())
        uf = host(u).reshape(dims)
        assert np.array_equal(uf[p.inner].reshape(-1), xh)
        ue, Ba = p.extend_full(xh, g, LD), p.extend_full_abs(xh, g)
        assert np.all(np.abs(uf - ue.astype(np.float64)) <= p.d * (max(p.M) + 2) * U * Ba), "the boundary nodes are the extension of x"
        x2 = op.solve(fd, gd, rtol=rtol, max_it=p.G, restart=p.G)
        assert np.array_equal(host(x2), xh) and op.iterations == its
    finally:
        op.destroy()


def test_operator_and_preconditioner_in_a_callers_fgmres():
    dims, bc, scale = SOLVE_CASES[0]
    p, g, f, A, b = solve_setup(0, True)
    op = sp.VarHelmholtz(dims, 1, bc=bc, scale=scale)
    ks = sp.Fgmres(op.size, restart=64, rtol=1e-10, atol=0.0, max_it=200)
    try:
        set_tensor(op, p, 0.0)
        fd, gd = dev(f), dev(g)
        bd = op.residual(dev(np.zeros(p.G)), fd, gd, new(op.size))
        x = ks.solve(op, bd, new(op.size), M=op, m_entry="precond")
        xs = op.solve(fd, gd, rtol=1e-10, max_it=200, restart=64)
        assert ks.reason == 2 and ks.iterations == op.iterations
        assert np.array_equal(host(x), host(xs)), "solve is FGMRES on mult and precond, nothing else"
    finally:
        ks.destroy(); op.destroy()


# ---- manufactured boundary-value problem ----------------------------------------------------------------------------------------------
def test_manufactured_solution_at_every_node():
    """u* = prod_k (1 + 0.3 x_k + 0.5 x_k^2) on 18 x 16 x 20 with Dirichlet and Robin faces: the faces' data g from u* and its exact
    derivative (degree 2: the grid differentiates it exactly), f = the long-double operator of u* -- K rotates with x, so K grad u*
    is no polynomial and f has no closed form the grid would reproduce; the discrete problem has the solution u* by construction.
    The bound is test_gpu_varhelm's: 16 x the error of NumPy's double dense solve of the same system, extended to the full grid the
    same way, plus what a residual of rtol |b| can move the solution by, rtol |A^-1|_2 |b|."""
    dims, bc, scale = (18, 16, 20), [(1.0, 2.0), ("dirichlet", (1.0, 0.5)), "dirichlet"], (1.0, 0.8, 1.25)
    p = make_problem(dims, bc, scale, True, "field", (1.0, 0.5, 2.0))
    X = vr.grid(dims, p.periodic)
    P0 = [1.0 + 0.3 * x + 0.5 * x * x for x in X]
    P1 = [0.3 + x for x in X]
    u = np.prod(P0, axis=0)
    gfull = np.zeros(dims)
    for k in range(3):                                                        # ascending: the highest direction writes last
        dudx = P1[k] * np.prod([P0[m] for m in range(3) if m != k], axis=0)
        a0, b0, a1, b1 = p.ends[k]
        ix0, ix1 = [slice(None)] * 3, [slice(None)] * 3
        ix0[k], ix1[k] = 0, dims[k] - 1
        gfull[tuple(ix0)] = (a0 * u + b0 * p.scale[k] * dudx)[tuple(ix0)]     # outward: +d/dx at index 0 (x = +1), -d/dx at the last
        gfull[tuple(ix1)] = (a1 * u - b1 * p.scale[k] * dudx)[tuple(ix1)]
    g = gfull[p.bmask]
    xstar = u[p.inner].reshape(-1)
    f = p.apply(xstar, g)[0].astype(np.float64)                               # (operator at g)(u*)
    rtol = 1e-12
    A64 = p.dense_double()
    b = (f.astype(LD) - p.apply(np.zeros(p.G), g)[0]).astype(np.float64)      # f + lift(g)
    lu = scipy.linalg.lu_factor(A64)
    e_np = np.abs(p.extend_full(scipy.linalg.lu_solve(lu, b), g) - u).max()
    v = np.ones(p.G) / np.sqrt(p.G)                                           # |A^-1|_2 by the power method on A^-T A^-1, from below;
    for _ in range(60):                                                       # 1.05: what sixty steps can still be short of it
        w = scipy.linalg.lu_solve(lu, scipy.linalg.lu_solve(lu, v), trans=1)
        nrm = np.linalg.norm(w)
        v = w / nrm
    ainv2 = 1.05 * np.sqrt(nrm)
    bound = 16.0 * e_np + rtol * ainv2 * np.linalg.norm(b)
    ffull = np.zeros(dims)
    ffull[p.inner] = f.reshape(p.ushape)
    uf, its = solve_mod.variable_diffusion(sp, dims, None, dev(ffull), c=dev(p.c), bc=bc, g=dev(g), scale=scale, rtol=rtol,
                                           tensor=dev(p.K), velocity=dev(p.vel))
    err = np.abs(host(uf).reshape(dims) - u).max()
    print("18x16x20: error %.3e, bound %.3e (dense solve %.3e, |A^-1|_2 %.3e), %d iterations" % (err, bound, e_np, ainv2, its))
    NOTES.append("manufactured 18x16x20, rotating K (1, 0.5, 2), velocity, rtol 1e-12, restart 30: %d iterations; error %.3e of bound %.3e" % (its, err, bound))
    assert err <= bound
    assert 0 < its <= 200


# ---- a singular problem -------------------------------------------------------------------------------------------------------------
def test_singular_problem_is_deflated():
    dims, bc, nf, rtol = (8, 9, 6), ["periodic", "neumann", "periodic"], 2, 1e-10
    p = make_problem(dims, bc, (0.5, 1.0, 2.0), True, 0.0)
    x0, g, f = make_inputs(p, nf, "noise", "given", SEED + 60)
    op = sp.VarHelmholtz(dims, nf, bc=bc, scale=p.scale)
    try:
        set_tensor(op, p, 0.0)
        assert op.singular and op.sigma == 0.0 and op.null_count == 4
        fd, gd = dev(f), dev(g)
        with pytest.raises(sp.ChebhipError) as e:
            op.solve(fd, gd)
        assert e.value.code == 4 and "singular" in str(e.value)
        x = op.solve_deflated(fd, gd, rtol=rtol, restart=60)
        print("8x9x6 singular: %d iterations" % op.iterations)
        NOTES.append("singular 8x9x6 (periodic, Neumann, periodic), velocity, rtol 1e-10, restart 60: %d iterations" % op.iterations)
        assert op.reason == 2
        N = sr.null_matrix(sp, p)
        q = N.shape[1]
        r = host(op.residual(x, fd, gd, new(op.size))).reshape(nf, p.G)
        b = host(op.residual(dev(np.zeros(op.size)), fd, gd, new(op.size))).reshape(nf, p.G)
        pr = np.stack([sr.project(N, r[j], LD) for j in range(nf)]).astype(np.float64)
        pb = np.stack([sr.project(N, b[j], LD) for j in range(nf)]).astype(np.float64)
        assert np.linalg.norm(pr) <= 1.05 * rtol * np.linalg.norm(pb)
        xh = host(x).reshape(nf, p.G)
        for j in range(nf):
            s = np.abs((N.T.astype(LD) @ xh[j].astype(LD)).astype(np.float64))
            assert np.all(s <= sr.bar3(xh[j], p.G, q)), "N^T x = 0 to the projection's bar"
        assert op.defect.shape == (nf, q)
    finally:
        op.destroy()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    dims, bc = (6, 5, 7), MIXED3
    p = make_problem(dims, bc, None, True, "field")
    op = sp.VarHelmholtz(dims, 2, bc=bc)
    try:
        n = op.size
        x = dev(np.ones(n))
        with pytest.raises(sp.ChebhipError) as e:
            op.mult(x, new(n))
        assert e.value.code == 4 and op.mode == 0
        with pytest.raises(sp.ChebhipError) as e:
            sp._chk(sp.lib().cheb_varhelm_set_tensor(op._h, None, None, None, 0.0, None))
        assert e.value.code == 4 and op.mode == 0
        kap = vr.kappa_field(dims, p.periodic, 0.5)
        for first in ("scalar", "tensor"):
            if first == "scalar":
                op.set_coefficients(dev(kap), dev(p.c))
            else:
                set_tensor(op, p, "field")
            good, sigma, mode = host(op.mult(x, new(n))).copy(), op.sigma, op.mode
            good_z = host(op.precond(x, new(n))).copy()
            for what in ("not spd", "minor2", "nan K", "inf K", "nan v", "nan c", "negative c", "no K"):
                K, v, c = p.K.copy(), p.vel.copy(), p.c.copy()
                if what == "not spd":
                    K[:, 2, 1, 3] = (1.0, 1.0, -1e-3, 0.0, 0.0, 0.0)
                elif what == "minor2":
                    K[3, 0, 0, 0] = 5.0
                elif what == "nan K":
                    K[5, 5, 4, 6] = np.nan
                elif what == "inf K":
                    K[0, 1, 1, 1] = np.inf
                elif what == "nan v":
                    v[1, 3, 2, 1] = np.nan
                elif what == "nan c":
                    c[0, 0, 0] = np.nan
                elif what == "negative c":
                    c[5, 4, 6] = -1e-300
                with pytest.raises(sp.ChebhipError) as e:
                    if what == "no K":
                        sp._chk(sp.lib().cheb_varhelm_set_tensor(op._h, None, dev(v).data_ptr(), None, 0.0, None))
                    else:
                        op.set_tensor(dev(K), dev(c), dev(v))
                assert e.value.code == 4, what
                assert op.mode == mode and op.sigma == sigma
                assert np.array_equal(host(op.mult(x, new(n))), good), "a refused set_tensor (%s) leaves the handle as it was" % what
                assert np.array_equal(host(op.precond(x, new(n))), good_z), what
            for cs in (-1.0, np.nan, np.inf):
                with pytest.raises(sp.ChebhipError):
                    op.set_tensor(dev(p.K), cs)
        for call in (lambda: op.set_tensor(dev(p.K)[:-1]), lambda: op.set_tensor(dev(p.K), 0.0, dev(p.vel)[:-1]),
                     lambda: op.set_tensor(dev(p.K).cpu())):
            with pytest.raises(ValueError):
                call()
    finally:
        op.destroy()
    for dims, bc in (((12,), [("neumann", (1.0, 0.5))]), ((4, 4, 4, 4), ["dirichlet"] * 4)):
        op = sp.VarHelmholtz(dims, 1, bc=bc)
        try:
            d = len(dims)
            op.set_coefficients(dev(np.ones(dims)), 1.0)
            good = host(op.mult(dev(np.ones(op.size)), new(op.size))).copy()
            with pytest.raises(sp.ChebhipError) as e:
                sp._chk(sp.lib().cheb_varhelm_set_tensor(op._h, dev(np.ones(d * (d + 1) // 2 * op.nodes)).data_ptr(), None, None, 1.0, None))
            assert e.value.code == 4 and "d = %d" % d in str(e.value)
            with pytest.raises(sp.ChebhipError):
                op.set_tensor(dev(np.ones(len(sp.tensor_order(d)) * op.nodes)), 1.0)
            assert op.mode == 1 and np.array_equal(host(op.mult(dev(np.ones(op.size)), new(op.size))), good)
        finally:
            op.destroy()
