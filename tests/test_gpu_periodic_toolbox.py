"""Periodic directions in ChebDealias, ChebProject, ChebOpFun and ChebPoints on the device against the long-double
truths and derived bars of periodic_toolbox_ref.py (its docstring states each count).  Shapes and masks are those of
test_gpu_periodic.py, so that the same routes are reached.  Every module also builds its all-zero-mask handle through the _basis
entry point and compares the bits with the old create call.  The worst measured ratio per bar goes to
profiles/periodic/toolbox_ratios.txt where PERIODIC_TOOLBOX_RATIOS_OUT names that file."""
import ctypes as C
import itertools
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import dealias_ref as dr
import linewise as lw
import opfun_ref as orf
import periodic_ref as pr
import periodic_toolbox_ref as tb
import points_deriv_ref as pdr
import points_ref as pref

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
LD = np.longdouble
U = 2.0 ** -53
SEED = 20261020


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("PERIODIC_TOOLBOX_RATIOS_OUT")
    if path and tb.records():
        with open(path, "w") as f:
            f.write("worst measured error / bar per check of tests/test_gpu_periodic_toolbox.py (at most 1 where the bar holds)\n")
            for name, (ratio, cap) in sorted(tb.records().items()):
                f.write("%-44s %.4f%s\n" % (name, ratio, "" if cap is None else "   (cap %g)" % cap))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().reshape(-1)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and v and isinstance(v[0], (int, np.integer)) else str(v)

SHAPES = [(8,), (9,), (2, 5), (16, 9), (12, 16), (16, 9, 12), (7, 6, 16), (6, 5, 96), (256, 4, 3)]
MASKS_3 = [(1, 0, 1), (0, 1, 0), (1, 1, 1), (0, 0, 1)]


def masks(d):
    return MASKS_3 if d == 3 else [m for m in itertools.product((0, 1), repeat=d) if any(m)]


GRID = [(dims, m) for dims in SHAPES for m in masks(len(dims))] + [((4, 5, 4, 6), (1, 0, 1, 0))]
# the solver's ranges: a wall direction needs an interior node
GRID_SOLVER = [(dims, m) for dims, m in GRID if all(n >= 3 for n, p in zip(dims, m) if not p)]
SCALE = {1: (0.75,), 2: (0.5, 2.0), 3: (0.5, 1.0, 2.0), 4: (0.5, 1.0, 2.0, 1.5)}


def basis_handle(obj, create, *args):
    """obj's handle replaced by one from the _basis entry point `create` (its out argument last)."""
    h = C.c_void_p()
    rc = create(*args, C.byref(h))
    assert rc == 0, sp.lib().chebhip_last_error()
    getattr(sp.lib(), obj._destroy)(obj._h)
    obj._h = h
    return obj


ints = lambda v: (C.c_int * len(v))(*[int(x) for x in v])


# =================================================================================================================================
# ChebDealias
# =================================================================================================================================
DEALIAS_GRID = GRID + [((8, 9), (1, 0)), ((9, 8), (1, 0))]


@pytest.mark.parametrize("dims,mask", DEALIAS_GRID, ids=ids)
def test_dealias_multiply_and_advect_per_element(dims, mask):
    d, nf = len(dims), 2
    h = sp.ChebDealias(dims, nf, periodic=mask)
    fine = tb.default_fine(dims, mask)
    assert h.fine == fine and h.periodic == tuple(bool(p) for p in mask)
    rng = np.random.default_rng(SEED + sum(dims))
    u, v, vel = rng.standard_normal((nf,) + dims), rng.standard_normal((nf,) + dims), rng.standard_normal((d,) + dims)
    ud, vd, veld = dev(u), dev(v), dev(vel)
    cap = dr.cap_multiply(dims, fine)
    got = host(h.multiply(ud, vd)).reshape(u.shape)
    t, B = tb.multiply_truth_bound(dims, fine, mask, u, v)
    r = lw.worst(got, t, cap * B)[0]
    tb.record("dealias multiply", r)
    print("%s %s multiply: %.3f of the bar (cap %d)" % (ids(dims), mask, r, cap))
    assert r <= 1.0, r
    gota = host(h.advect(veld, ud)).reshape(u.shape)
    t, B = tb.advect_truth_bound(dims, fine, mask, vel, u)
    ra = lw.worst(gota, t, (cap + d) * B)[0]
    tb.record("dealias advect", ra)
    print("%s %s advect: %.3f of the bar" % (ids(dims), mask, ra))
    assert ra <= 1.0, ra
    # the same bits from run to run
    assert np.array_equal(host(h.multiply(ud, vd)).reshape(u.shape), got)
    assert np.array_equal(host(h.advect(veld, ud)).reshape(u.shape), gota)
    # a NaN stays in the field it is in
    ub = u.copy()
    ub[0][tuple(n // 3 for n in dims)] = np.nan
    gb = host(h.multiply(dev(ub), vd)).reshape(u.shape)
    assert np.isnan(gb[0]).any() and np.array_equal(gb[1], got[1])
    h.destroy()


@pytest.mark.parametrize("dims", [(9,), (16, 9), (7, 6, 16)], ids=ids)
def test_dealias_all_zero_basis_is_the_old_handle(dims):
    d, nf = len(dims), 2
    rng = np.random.default_rng(SEED + 3)
    u, v, vel = dev(rng.standard_normal((nf,) + dims)), dev(rng.standard_normal((nf,) + dims)), dev(rng.standard_normal((d,) + dims))
    h0 = sp.ChebDealias(dims, nf)
    h1 = sp.ChebDealias(dims, nf, periodic=(0,) * d)          # (cheb_dealias_create_basis with an all-zero basis)
    assert h0.fine == h1.fine and h0.work_bytes() == h1.work_bytes()
    assert torch.equal(h0.multiply(u, v), h1.multiply(u, v))
    assert torch.equal(h0.advect(vel, u), h1.advect(vel, u))
    torch.cuda.synchronize()
    h0.destroy(); h1.destroy()


@pytest.mark.parametrize("n", [8, 9])
def test_dealias_modes_and_the_nyquist_square(n):
    """Single trigonometric modes give their product's cut; the bar's (K + 8) per line product already counts the rounding of a
    matrix entry, so the exact cut is held to the same cap."""
    h = sp.ChebDealias((n,), 1, periodic=(1,))
    m = h.fine[0]
    x = pr.nodes(n)
    cap = dr.cap_multiply((n,), (m,))
    K = n // 2
    pairs = [((3, "cos"), (2, "sin")), ((K, "cos"), (K, "cos")), ((K - 1, "sin"), (2, "cos")), ((1, "sin"), (K - 1, "sin"))]
    for (ku, cu), (kv, cv) in pairs:
        u, v = tb.mode(n, ku, cu, x).astype(np.float64)[None], tb.mode(n, kv, cv, x).astype(np.float64)[None]
        got = host(h.multiply(dev(u), dev(v))).reshape(1, n)
        _, B = tb.multiply_truth_bound((n,), (m,), (1,), u, v)
        # (the sampled modes are rounded doubles: one more rounding per operand)
        r = lw.worst(got, tb.exact_cut(n, ku, cu, kv, cv)[None], (cap + 2) * B)[0]
        tb.record("dealias single modes", r)
        assert r <= 1.0, (ku, cu, kv, cv, r)
    if n % 2 == 0:
        u = np.where(np.arange(n) & 1, -1.0, 1.0)[None]
        got = host(h.multiply(dev(u), dev(u))).reshape(1, n)
        _, B = tb.multiply_truth_bound((n,), (m,), (1,), u, u)
        assert np.all(np.abs(got - 0.5) <= cap * U * B)
    h.destroy()


def test_dealias_unpadded_periodic_direction():
    dims, mask, fine = (8, 9), (1, 0), (8, 14)
    h = sp.ChebDealias(dims, 1, fine=fine, periodic=mask)
    assert h.fine == fine
    rng = np.random.default_rng(SEED + 5)
    u, v, vel = rng.standard_normal((1,) + dims), rng.standard_normal((1,) + dims), rng.standard_normal((2,) + dims)
    cap = dr.cap_multiply(dims, fine)
    t, B = tb.multiply_truth_bound(dims, fine, mask, u, v)
    assert lw.worst(host(h.multiply(dev(u), dev(v))).reshape(u.shape), t, cap * B)[0] <= 1.0
    t, B = tb.advect_truth_bound(dims, fine, mask, vel, u)
    assert lw.worst(host(h.advect(dev(vel), dev(u))).reshape(u.shape), t, (cap + 2) * B)[0] <= 1.0
    h.destroy()


# =================================================================================================================================
# ChebProject
# =================================================================================================================================
def project_bc(dims, mask, open_face=None):
    bc = ["periodic" if p else "wall" for p in mask]
    if open_face is not None:
        bc[open_face] = ("open", "wall")
    return bc


def solver_bc(bc):
    one = lambda e: "neumann" if e == "wall" else "dirichlet"
    return [e if e == "periodic" else one(e) if isinstance(e, str) else (one(e[0]), one(e[1])) for e in bc]


def boundary_data(dims, mask, bc, u, flux):
    """g of the solver for ONE vector: +u_k at index 0, -u_k at index n-1 of the face's direction, minus the flux, 0 at an open face."""
    bm = pr.boundary_mask(dims, mask)
    code = tb.face_table(dims, mask)
    g = np.zeros(code.size)
    for k in range(len(dims)):
        if mask[k]:
            continue
        uk = u[k][bm]
        kinds = (bc[k], bc[k]) if isinstance(bc[k], str) else bc[k]
        for e in range(2):
            sel = code == 2 * k + e
            if kinds[e] == "wall":
                g[sel] = uk[sel] if e == 0 else -uk[sel]
                if flux is not None:
                    g[sel] = g[sel] - flux[sel]
    return g


PROJECT_CASES = [(dims, m, None) for dims, m in GRID_SOLVER] + [((16, 9, 12), (1, 0, 1), 1), ((12, 16), (1, 0), 1)]


@pytest.mark.parametrize("dims,mask,open_face", PROJECT_CASES, ids=ids)
def test_project(dims, mask, open_face):
    d = len(dims)
    scale = SCALE[d]
    bc = project_bc(dims, mask, open_face)
    inner = pr.unknown_slices(mask)
    for nvec in sorted({1, 16 // d}):
        h = sp.ChebProject(dims, nvec, bc, scale)
        N = int(np.prod(dims))
        G = int(np.prod(pr.unknown_shape(dims, mask)))
        assert (h.size, h.interior_size, h.boundary_size) == (N, G, N - G)
        assert h.periodic == tuple(bool(p) for p in mask) and h.singular == (open_face is None)
        rng = np.random.default_rng(SEED + sum(dims) + nvec)
        u = rng.standard_normal((nvec, d) + dims)
        flux = rng.standard_normal((nvec, N - G)) * 0.1 if N > G else None
        ud = dev(u)
        phid = torch.empty(nvec * N, dtype=torch.float64, device="cuda")
        fluxd = None if flux is None else dev(flux)
        outd = h.project(ud, phi=phid, flux=fluxd)
        out, phi = host(outd).reshape(u.shape), host(phid).reshape((nvec,) + dims)
        # phi is HelmholtzSolver.solve_full of the same right-hand side, bit for bit
        gh = sp.ChebGrad(dims, scale, periodic=mask)
        div = host(gh.div(ud)).reshape((nvec,) + dims)
        f = np.ascontiguousarray(-div[(slice(None),) + inner])
        hs = sp.HelmholtzSolver(dims, 0.0, nvec, bc=solver_bc(bc), scale=scale)
        g = None
        if N > G:
            g = np.stack([boundary_data(dims, mask, bc, u[v], None if flux is None else flux[v]) for v in range(nvec)])
        us = torch.empty(nvec * N, dtype=torch.float64, device="cuda")
        hs.solve_full(dev(f), None if g is None else dev(g), us)
        torch.cuda.synchronize()
        assert torch.equal(us, phid), "phi differs from solve_full in %d values" % int((us != phid).sum())
        hs.destroy(); gh.destroy()
        # the divergence of the result and the wall-normal velocity
        for v in range(nvec):
            eps = 1e-9 * float(np.abs(phi[v]).max())
            r = tb.div_ratio(dims, mask, scale, u[v], phi[v], out[v], eps, spread=open_face is None and not all(mask))
            tb.record("project div " + ("all periodic" if all(mask) else "channel" if open_face is None else "open face"), r)
            assert r <= 1.0, (v, r)
            if N > G:
                bm, code = pr.boundary_mask(dims, mask), tb.face_table(dims, mask)
                for k in range(d):
                    if mask[k]:
                        continue
                    sD = scale[k] * float(np.abs(lw.dense_D(dims[k]).astype(np.float64)).sum(axis=1).max())
                    kinds = (bc[k], bc[k]) if isinstance(bc[k], str) else bc[k]
                    for e in range(2):
                        sel = code == 2 * k + e
                        if kinds[e] == "wall" and sel.any():
                            nrm = out[v][k][bm][sel] * (1.0 if e == 0 else -1.0)
                            rn = float(np.abs(nrm - flux[v][sel]).max()) / (eps * sD)
                            tb.record("project wall-normal velocity", rn)
                            assert rn <= 1.0, (v, k, e, rn)
        # out is u; the same bits from run to run
        u2 = ud.clone()
        phi2 = torch.empty_like(phid)
        h.project(u2, out=u2, phi=phi2, flux=fluxd)
        torch.cuda.synchronize()
        assert torch.equal(u2.reshape(-1), outd.reshape(-1)) and torch.equal(phi2, phid)
        if all(mask):
            with pytest.raises(sp.ChebhipError):
                h.project(ud, flux=torch.zeros(1, dtype=torch.float64, device="cuda"))
        h.destroy()


@pytest.mark.parametrize("dims", [(9,), (16, 9), (7, 6, 16)], ids=ids)
def test_project_all_zero_basis_is_the_old_handle(dims):
    d = len(dims)
    sc = np.array(SCALE[d])
    u = dev(np.random.default_rng(SEED + 7).standard_normal((d,) + dims))
    h0 = sp.ChebProject(dims, 1, None, SCALE[d])
    h1 = basis_handle(sp.ChebProject(dims, 1, None, SCALE[d]), sp.lib().cheb_project_create_basis, d, ints(dims), ints([0] * d), None,
                      sc.ctypes.data_as(C.POINTER(C.c_double)), 1)
    p0, p1 = torch.empty(h0.size, dtype=torch.float64, device="cuda"), torch.empty(h0.size, dtype=torch.float64, device="cuda")
    o0, o1 = h0.project(u, phi=p0), h1.project(u, phi=p1)
    torch.cuda.synchronize()
    assert torch.equal(o0, o1) and torch.equal(p0, p1)
    assert np.array_equal(sp.project_faces(dims, periodic=(0,) * d), sp.project_faces(dims))
    h0.destroy(); h1.destroy()


# =================================================================================================================================
# ChebOpFun
# =================================================================================================================================
def opfun_model(dims, mask, bc, scale, sigma, terms, x, nout):
    """opfun_ref.model on the unknown layout of a handle with periodic directions: (y, bar)."""
    ln = pr.lines(sp, dims, mask, bc, scale)
    M = pr.unknown_shape(dims, mask)
    s = orf.eigen_sum(ln, sigma)
    xs = np.asarray(x, dtype=np.float64).reshape((-1,) + M)
    c = orf.to_modes(ln, xs, LD)
    ca = orf.to_modes(ln, xs, LD, absolute=True)
    ws = orf.term_weights(terms, s)
    acc = np.zeros((nout,) + M, dtype=LD)
    B = np.zeros((nout,) + M, dtype=LD)
    Bp = np.zeros((nout,) + M, dtype=LD)
    T = np.zeros(nout)
    for (o, i, kind, coef, tau, par), w in zip(terms, ws):
        acc[o] = acc[o] + (LD(coef) * w.astype(LD)) * c[i]
        aw = np.abs(coef * w).astype(LD)
        B[o] += aw * ca[i]
        Bp[o] += aw * (orf.K[kind] + orf.kappa(kind, tau, s)) * ca[i]
        T[o] += 1
    y = orf.to_nodes(ln, acc, LD)
    B = orf.to_nodes(ln, B, LD, absolute=True)
    Bp = orf.to_nodes(ln, Bp, LD, absolute=True)
    lines_k = sum(2 * (m + 8) for m in M)
    bar = U * ((lines_k + T).reshape((nout,) + (1,) * len(M)) * B + Bp)
    return y.reshape(nout, -1), np.asarray(bar, dtype=np.float64).reshape(nout, -1), ln, s


KIND_ARGS = {"exp": (1e-2, 0.0), "phi1": (1e-2, 0.0), "res": (0.05, 1.5), "pow": (0.0, 0.5)}


def opfun_bc(mask, wall="dirichlet"):
    return ["periodic" if p else wall for p in mask]


@pytest.mark.parametrize("dims,mask", GRID_SOLVER, ids=ids)
def test_opfun_kinds_and_mixing(dims, mask):
    d = len(dims)
    scale, sigma = SCALE[d], 0.3
    bc = opfun_bc(mask)
    G = int(np.prod(pr.unknown_shape(dims, mask)))
    h = sp.ChebOpFun(dims, 2, 1, sigma, bc=bc, scale=scale)
    assert h.size == 2 * G and h.out_size == G and h.full_size == int(np.prod(dims)) and not h.singular
    assert h.periodic == tuple(bool(p) for p in mask)
    x = np.random.default_rng(SEED + sum(dims)).standard_normal((2, G))
    xd = dev(x)
    wall = [None if p else "dirichlet" for p in mask]
    for kind, (tau, par) in KIND_ARGS.items():
        terms = [(0, 0, kind, 1.0, tau, par)]
        h.set_terms(terms)
        y = host(h.apply(xd))
        ref, bar, ln, s = opfun_model(dims, mask, wall, scale, sigma, terms, x, 1)
        ratio, nerr = orf.check(y, ref, bar, "%s %s %s" % (ids(dims), mask, kind))
        tb.record("opfun field bar", ratio)
    # a 2 -> 1 table against the two calls and the add
    terms = [(0, 0, "exp", 0.5, 1e-2, 0.0), (0, 1, "res", -2.0, 0.05, 1.5)]
    h.set_terms(terms)
    y = h.apply(xd)
    ref, bar, ln, s = opfun_model(dims, mask, wall, scale, sigma, terms, x, 1)
    orf.check(host(y), ref, bar, "mix")
    h1 = sp.ChebOpFun(dims, 1, 1, sigma, bc=bc, scale=scale)
    h1.set_terms([terms[0][:1] + (0,) + terms[0][2:]])
    a = host(h1.apply(xd[:G].clone()))
    h1.set_terms([(0, 0) + terms[1][2:]])
    b = host(h1.apply(xd[G:].clone()))
    assert np.all(np.abs(host(y) - (a + b)) <= 2.0 * bar.reshape(-1) + U * np.abs(a + b))
    # apply_full: the unknowns embedded, the wall ends from the homogeneous conditions; every direction periodic: apply itself
    yf = host(h.apply_full(xd)).reshape(dims)
    assert np.array_equal(yf[pr.unknown_slices(mask)].reshape(-1), host(y))
    if all(mask):
        assert np.array_equal(yf.reshape(-1), host(y))
    else:
        for k in range(d):
            if not mask[k]:
                idx = [slice(None)] * d
                for e in (0, dims[k] - 1):
                    idx[k] = e
                    assert np.all(yf[tuple(idx)] == 0.0)          # (Dirichlet walls: u_B = Q u_I = 0)
    h.destroy(); h1.destroy()


def same_route(dims, mask):
    """test_gpu_opfun.same_route on the unknown layout: the last direction's unknowns are even in number and its line a parity line
    (a periodic line is one, and so are equal ends)."""
    M = pr.unknown_shape(dims, mask)
    return M[-1] % 2 == 0


@pytest.mark.parametrize("dims,mask", [(dm, m) for dm, m in GRID_SOLVER if 2 <= len(dm) <= 3 and same_route(dm, m)], ids=ids)
def test_opfun_inv_is_the_solver(dims, mask):
    d, nf, sigma = len(dims), 2, 0.7
    bc = opfun_bc(mask, "neumann")
    G = int(np.prod(pr.unknown_shape(dims, mask)))
    x = dev(np.random.default_rng(SEED + 11).standard_normal(nf * G))
    old = sp.get_option("fdm_z_separate")
    sp.set_option("fdm_z_separate", 1)
    try:
        hs = sp.HelmholtzSolver(dims, sigma, nf, bc=bc, scale=SCALE[d])
        h = sp.ChebOpFun(dims, nf, nf, sigma, bc=bc, scale=SCALE[d])
        h.set_terms("inv")
        u = torch.empty_like(x)
        hs.solve(x, u)
        y = h.apply(x)
        torch.cuda.synchronize()
        assert torch.equal(y, u), "%d of %d values differ" % (int((y != u).sum()), y.numel())
        hs.destroy(); h.destroy()
    finally:
        sp.set_option("fdm_z_separate", old)


@pytest.mark.parametrize("dims,mask", [((8,), (1,)), ((9,), (1,)), ((12, 16), (1, 0)), ((16, 9, 12), (1, 0, 1))], ids=ids)
def test_opfun_eigenvectors(dims, mask):
    """The product of one mode per direction (a Fourier mode, a wall eigenvector) goes to f(s) times itself."""
    d = len(dims)
    scale, sigma = SCALE[d], 0.3
    bc = opfun_bc(mask)
    wall = [None if p else "dirichlet" for p in mask]
    ln = pr.lines(sp, dims, mask, wall, scale)
    M = pr.unknown_shape(dims, mask)
    pos = tuple(m // 3 + 1 if m > 2 else m - 1 for m in M)
    vec = np.ones(())
    for k in range(d):
        vec = np.multiply.outer(vec, ln[k][0][:, pos[k]])
    s = orf.eigen_sum(ln, sigma)[pos]
    h = sp.ChebOpFun(dims, 1, 1, sigma, bc=bc, scale=scale)
    for kind, (tau, par) in KIND_ARGS.items():
        terms = [(0, 0, kind, 1.0, tau, par)]
        h.set_terms(terms)
        y = host(h.apply(dev(vec)))
        ref, bar, _, _ = opfun_model(dims, mask, wall, scale, sigma, terms, vec.reshape(1, -1), 1)
        w = sp.opfun_weight(kind, tau, par, s)
        # the model is the bar's centre; f(s) v differs from it by the rounding of S S^-1 on v, which the same bar covers
        assert np.all(np.abs(y - ref.reshape(-1)) <= bar.reshape(-1))
        assert np.all(np.abs(y - w * vec.reshape(-1)) <= 2.0 * bar.reshape(-1)), kind
    h.destroy()


@pytest.mark.parametrize("dims", [(8,), (12, 16), (4, 6, 8)], ids=ids)
def test_opfun_singular_all_periodic(dims):
    """sigma = 0, every direction periodic, even extents: every product of a constant or a Nyquist vector per direction has s == 0
    and gets what the kinds give s == 0 on any singular handle: 0 from inv and pow, 1 from exp, 1/k! from phi_k."""
    d = len(dims)
    h = sp.ChebOpFun(dims, 1, 1, 0.0, bc=["periodic"] * d)
    assert h.singular and h.size == h.full_size
    expect = {"inv": 0.0, "pow": 0.0, "exp": 1.0, "phi1": 1.0, "phi2": 0.5, "one": 1.0}
    for choice in itertools.product((0, 1), repeat=d):
        vec = np.ones(())
        for k, n in enumerate(dims):
            vec = np.multiply.outer(vec, np.where(np.arange(n) & 1, -1.0, 1.0) if choice[k] else np.ones(n))
        xd = dev(vec)
        for kind, w in expect.items():
            terms = [(0, 0, kind, 1.0, 0.25, 0.5)]
            h.set_terms(terms)
            y = host(h.apply(xd))
            ref, bar, _, s = opfun_model(dims, (1,) * d, None, None, 0.0, terms, vec.reshape(1, -1), 1)
            assert np.all(np.abs(y - ref.reshape(-1)) <= bar.reshape(-1)), (choice, kind)
            assert np.all(np.abs(y - w * vec.reshape(-1)) <= 2.0 * bar.reshape(-1)), (choice, kind)
    assert int((s == 0.0).sum()) == 2 ** d                       # (exactly the products of zero modes)
    h.destroy()


@pytest.mark.parametrize("dims", [(9,), (16, 9)], ids=ids)
def test_opfun_all_zero_basis_is_the_old_handle(dims):
    d = len(dims)
    b = sp.bc_array(["neumann"] * d, d)
    sc = np.array(SCALE[d])
    h0 = sp.ChebOpFun(dims, 1, 1, 0.4, bc=["neumann"] * d, scale=SCALE[d])
    h1 = basis_handle(sp.ChebOpFun(dims, 1, 1, 0.4, bc=["neumann"] * d, scale=SCALE[d]), sp.lib().cheb_opfun_create_basis, d, ints(dims),
                      ints([0] * d), (C.c_double * len(b))(*b), sc.ctypes.data_as(C.POINTER(C.c_double)), 0.4, 1, 1)
    x = dev(np.random.default_rng(SEED + 13).standard_normal(h0.size))
    for h in (h0, h1):
        h.set_terms("exp", tau=0.01)
    assert torch.equal(h0.apply(x), h1.apply(x)) and torch.equal(h0.apply_full(x), h1.apply_full(x))
    torch.cuda.synchronize()
    h0.destroy(); h1.destroy()


# =================================================================================================================================
# ChebPoints
# =================================================================================================================================
def beside(x, to):
    """The neighbouring double of x towards `to`; of the node 0 a coordinate of 1e-300, whose row still has normal numbers (the
    bars count relative roundings, which subnormal entries do not have)."""
    return np.where(x == 0.0, np.copysign(1e-300, to), np.nextafter(x, to))


def row_points(n):
    rng = np.random.default_rng(100 + n)
    xn = sp.fourier_nodes(n)
    mid = xn + 1.0 / n
    return np.concatenate([rng.uniform(-3, 3, 40), xn, xn + 2, xn - 2, mid[: min(n, 8)], mid[: min(n, 8)] - 2, [1.0, -1.0, 3.0, 1e9 + 0.25],
                           beside(xn[: min(n, 6)], 2), beside(xn[: min(n, 6)], -2), np.nextafter(mid[: min(n, 6)], 2),
                           np.nextafter(mid[: min(n, 6)], -2), [np.nan, np.inf, -np.inf]])


@pytest.mark.parametrize("n", [2, 3, 8, 9, 65, 256])
def test_points_rows_and_derivative_rows(n):
    h = sp.ChebPoints((n,), 1, periodic=(1,))
    x = row_points(n)
    xd = dev(x)
    rows, drows = host(h.rows(0, xd)).reshape(-1, n), host(h.drows(0, xd)).reshape(-1, n)
    t, M = tb.rows_ld(n, x)
    r = pdr.worst(rows, t, M, tb.CAP_ROWS)
    tb.record("points value rows", r, tb.CAP_ROWS)
    td, Md = tb.drows_ld(n, x)
    rd = pdr.worst(drows, td, Md, tb.CAP_DROWS)
    tb.record("points derivative rows", rd, tb.CAP_DROWS)
    print("n = %d: value rows %.3f, derivative rows %.3f of the bar" % (n, r, rd))
    assert r <= 1.0 and rd <= 1.0, (r, rd)
    assert np.isnan(rows[-3:]).all() and np.isnan(drows[-3:]).all() and np.isfinite(rows[:-3]).all() and np.isfinite(drows[:-3]).all()
    # the doubles fourier_nodes(n), one period up and one down where that sum is exact: the unit row, bit for bit
    xn = sp.fourier_nodes(n)
    for shift in (0.0, 2.0, -2.0):
        ok = (xn + shift) - shift == xn
        got = host(h.rows(0, dev(xn + shift))).reshape(n, n)
        assert np.array_equal(got[ok], np.eye(n)[ok]), shift
    # the derivative rows at the nodes are D_F within the bar (through the truth above), and annihilate the Nyquist vector
    dn = host(h.drows(0, dev(xn))).reshape(n, n)
    tdn, Mdn = tb.drows_ld(n, xn)
    assert pdr.worst(dn, tdn, Mdn, tb.CAP_DROWS) <= 1.0
    if n % 2 == 0:
        ny = np.where(np.arange(n) & 1, -1.0, 1.0)
        assert np.all(np.abs(dn @ ny) <= tb.CAP_DROWS * U * (Mdn @ np.ones(n)) + U * n * np.abs(dn).sum(axis=1))
    # rows() and drows() with what = 3 inside eval_grad give the same bits from run to run
    assert np.array_equal(host(h.rows(0, xd)).reshape(-1, n), rows, equal_nan=True)
    h.destroy()


POINTS_CASES = [((8,), (1,)), ((9,), (1,)), ((8, 9), (1, 0)), ((8, 9), (0, 1)), ((9, 8), (1, 1)), ((6, 5, 9), (1, 0, 1)),
                ((4, 5, 4, 6), (1, 0, 1, 0))]


def case_points(dims, mask, npts, seed):
    rng = np.random.default_rng(seed)
    pts = np.empty((npts, len(dims)))
    for k, n in enumerate(dims):
        pts[:, k] = rng.uniform(-3, 3, npts) if mask[k] else rng.uniform(-1, 1, npts)
        nodes = tb.grid_nodes(n, mask[k])
        pts[:3, k] = nodes[[0, n // 2, n - 1]]
    return pts


@pytest.mark.parametrize("dims,mask", POINTS_CASES, ids=ids)
def test_points_eval_grad_grid_spread(dims, mask):
    d, nf, npts = len(dims), 2, 37
    h = sp.ChebPoints(dims, nf, periodic=mask)
    assert h.periodic == tuple(bool(p) for p in mask)
    rng = np.random.default_rng(SEED + sum(dims))
    u = rng.standard_normal((nf,) + dims)
    pts = case_points(dims, mask, npts, SEED + d)
    ud, pd = dev(u), dev(pts).reshape(npts, d)
    derivs = [None, tuple(1 if k == 0 else 0 for k in range(d)), tuple(1 if k == d - 1 else 0 for k in range(d))]
    for deriv in derivs:
        dv = deriv or (0,) * d
        rows, mags, caps = tb.rows_kinds(dims, mask, pts, dv)
        val, B = pdr.values_ld(dims, nf, u, rows, mags)
        got = host(h.eval(ud, pd, deriv=deriv))
        r = pdr.worst(got, val, B, sum(caps))
        tb.record("points eval", r)
        assert r <= 1.0, (deriv, r)
        assert np.array_equal(host(h.eval(ud, pd, deriv=deriv)), got)
        # spread: the transpose, g_i = sum_p s_p prod_k rows_k[p][i_k]
        for delta in (False, True):
            s = rng.standard_normal((nf, npts))
            L, La = rows[0], mags[0]
            for rr, ma in zip(rows[1:], mags[1:]):
                L = (L[:, :, None] * rr[:, None, :]).reshape(npts, -1)
                La = (La[:, :, None] * ma[:, None, :]).reshape(npts, -1)
            t = s.astype(LD) @ L
            b = np.abs(s) @ La
            capS = sum(c - (n + 5.0) + 5.0 if (mask[k] or dv[k]) else pref.lam(n) * n + 8.0 for k, (n, c) in enumerate(zip(dims, caps)))
            capS += d + npts + (d + 1 if delta else 0)
            if delta:
                W = np.ones(1, dtype=LD)
                for k, n in enumerate(dims):
                    W = (W[:, None] * tb.quad_weights(n, mask[k]).astype(LD)[None, :]).reshape(-1)
                t, b = t / W, (b / W).astype(np.float64)
            g = h.spread(dev(s).reshape(nf, npts), pd, delta=delta, deriv=deriv)
            rs = pdr.worst(host(g), t, b, capS)
            tb.record("points spread", rs)
            assert rs <= 1.0, (deriv, delta, rs)
            g2 = h.spread(dev(s).reshape(nf, npts), pd, out=g.clone(), accumulate=True, delta=delta, deriv=deriv)
            assert pdr.worst(host(g2), 2 * t, 2 * b, capS + 1) <= 1.0
    # eval_grad: every first derivative and the value, scaled
    scale = SCALE[d]
    gr = host(h.eval_grad(ud, pd, value=True, scale=scale))
    for c in range(d + 1):
        dv = tuple(1 if k == c else 0 for k in range(d))
        rows, mags, caps = tb.rows_kinds(dims, mask, pts, dv)
        val, B = pdr.values_ld(dims, nf, u, rows, mags)
        sc = scale[c] if c < d else 1.0
        r = pdr.worst(gr[:, c, :], val * LD(sc), B * abs(sc), sum(caps) + 1.0)
        tb.record("points eval_grad", r)
        assert r <= 1.0, (c, r)
    # eval_grid: one line product per direction
    m = [5 + k for k in range(d)]
    coords = [case_points((n,), (mask[k],), m[k], SEED + 31 + k)[:, 0] for k, n in enumerate(dims)]
    for deriv in (None, derivs[1]):
        dv = deriv or (0,) * d
        t, b, capg = u.astype(LD), np.abs(u), 0.0
        for k, n in enumerate(dims):
            rows, mags, caps = tb.rows_kinds((n,), (mask[k],), coords[k][:, None], (dv[k],))
            t = np.moveaxis(np.tensordot(rows[0], t, axes=([1], [k + 1])), 0, k + 1)
            b = np.moveaxis(np.tensordot(mags[0], b, axes=([1], [k + 1])), 0, k + 1)
            capg += caps[0] + 3.0
        got = host(h.eval_grid(ud, [dev(c) for c in coords], deriv=deriv))
        r = pdr.worst(got, t, b, capg)
        tb.record("points eval_grid", r)
        assert r <= 1.0, (deriv, r)
    h.destroy()


@pytest.mark.parametrize("dims,mask", [((8, 9), (1, 0)), ((16, 5, 4), (1, 0, 1))], ids=ids)
def test_points_node_values_nan_and_old_handle(dims, mask):
    d, nf = len(dims), 2
    rng = np.random.default_rng(SEED + 41)
    u = rng.standard_normal((nf,) + dims)
    h = sp.ChebPoints(dims, nf, periodic=mask)
    # every node, the periodic coordinates a period away: the field's bits
    grids = np.meshgrid(*[tb.grid_nodes(n, mask[k]) + (2.0 if mask[k] else 0.0) for k, n in enumerate(dims)], indexing="ij")
    pts = np.stack([g.reshape(-1) for g in grids], axis=1)
    got = host(h.eval(dev(u), dev(pts).reshape(-1, d)))
    assert np.array_equal(got, u.reshape(nf, -1))
    # a NaN or infinite coordinate poisons its point only
    bad = pts[:6].copy()
    bad[1, 0], bad[3, d - 1], bad[4, 0] = np.nan, np.inf, -np.inf
    gb = host(h.eval(dev(u), dev(bad).reshape(-1, d)))
    assert np.isnan(gb[:, [1, 3, 4]]).all() and np.array_equal(gb[:, [0, 2, 5]], got[:, [0, 2, 5]])
    # the all-zero mask through the _basis entry point: the old handle's bits
    h0, h1 = sp.ChebPoints(dims, nf), sp.ChebPoints(dims, nf, periodic=(0,) * d)
    p = dev(rng.uniform(-1, 1, (23, d))).reshape(23, d)
    assert torch.equal(h0.eval(dev(u), p), h1.eval(dev(u), p))
    assert torch.equal(h0.eval_grad(dev(u), p), h1.eval_grad(dev(u), p))
    s = dev(rng.standard_normal((nf, 23))).reshape(nf, 23)
    assert torch.equal(h0.spread(s, p, delta=True), h1.spread(s, p, delta=True))
    torch.cuda.synchronize()
    for x in (h, h0, h1):
        x.destroy()


@pytest.mark.parametrize("dims,mask", [((8,), (1,)), ((9, 6), (1, 0)), ((6, 5, 8), (1, 0, 1))], ids=ids)
def test_points_sources_integrate_to_point_values(dims, mask):
    """ChebModal(periodic).integrate(spread(delta=True), phi) = sum_p s_p phi(x_p) for phi in the grid's space: a trigonometric mode
    along a periodic direction, a polynomial along a wall one."""
    d, npts = len(dims), 11
    rng = np.random.default_rng(SEED + 51)
    pts = case_points(dims, mask, npts, SEED + 52)
    s = rng.standard_normal(npts)

    def phi(xs):
        out = np.ones(np.broadcast(*xs).shape, dtype=LD)
        for k, n in enumerate(dims):
            x = np.asarray(xs[k], dtype=LD)
            out = out * (np.cos(tb.PI_L * LD((n - 1) // 2) * (x + 1)) + LD(0.5) if mask[k] else x ** (n - 1) - LD(0.25) * x)
        return out

    grids = np.meshgrid(*[tb.grid_nodes(n, mask[k]) for k, n in enumerate(dims)], indexing="ij")
    pg = phi(grids).astype(np.float64)
    g = solve.point_sources(sp, dims, dev(pts).reshape(npts, d), dev(s), periodic=mask)
    hm = sp.ChebModal(dims, 1, periodic=mask)
    got = float(host(hm.integrate(g.reshape(-1), dev(pg)))[0])
    want = float((s.astype(LD) * phi([pts[:, k] for k in range(d)])).sum())
    rows, mags, caps = tb.rows_kinds(dims, mask, pts, (0,) * d)
    La = mags[0]
    for ma in mags[1:]:
        La = (La[:, :, None] * ma[:, None, :]).reshape(npts, -1)
    b = np.abs(s) @ La
    cap = sum(caps) + 2 * d + 1 + npts + int(np.prod(dims)) + 8 + d
    bar = cap * U * float((b * np.abs(pg).reshape(-1)).sum()) + 4 * U * abs(want)
    tb.record("points sources integrate", abs(got - want) / bar)
    assert abs(got - want) <= bar, (got, want, bar)
    hm.destroy()


# =================================================================================================================================
# the modules together on a channel
# =================================================================================================================================
def test_channel_step():
    dims, mask = (16, 17, 12), (1, 0, 1)
    d = 3
    rng = np.random.default_rng(SEED + 61)
    c = rng.standard_normal((1,) + dims)
    a = np.array([0.5, -1.25, 2.0])
    vel = np.broadcast_to(a[:, None, None, None], (d,) + dims).copy()
    hd = sp.ChebDealias(dims, 1, periodic=mask)
    got = host(hd.advect(dev(vel), dev(c))).reshape(dims)
    t, B = tb.advect_truth_bound(dims, hd.fine, mask, vel, c)
    tr = sum(LD(a[k]) * lw.truth(pr.dmat(sp, n, mask[k]), c[0], k) for k, n in enumerate(dims))
    cap = dr.cap_multiply(dims, hd.fine) + d
    r = lw.worst(got[None], tr[None], cap * B)[0]
    tb.record("channel advect = a . grad", r)
    assert r <= 1.0, r
    hd.destroy()
    # project, then read the projected field back at the nodes: its bits
    u = rng.standard_normal((d,) + dims)
    out, phi = solve.channel_project(sp, dims, dev(u), mask)
    hp = sp.ChebPoints(dims, d, periodic=mask)
    grids = np.meshgrid(*[tb.grid_nodes(n, mask[k]) for k, n in enumerate(dims)], indexing="ij")
    pts = np.stack([g.reshape(-1) for g in grids], axis=1)
    back = hp.eval(out.reshape(-1), dev(pts).reshape(-1, d))
    torch.cuda.synchronize()
    assert torch.equal(back.reshape(-1), out.reshape(-1))
    hp.destroy()
    # the wrappers pass the flags through
    plane = solve.sample_plane(sp, dims, out[0].reshape(-1), 1, 0.25, periodic=mask)
    assert tuple(plane.shape) == (1, dims[0], dims[2])
    A = solve.velocity_gradient(sp, dims, out.reshape(-1), dev(pts[:5]).reshape(5, d), periodic=mask)
    assert tuple(A.shape) == (5, d, d)
    v = solve.diffuse(sp, dims, out[0], 0.01, ["periodic", "dirichlet", "periodic"])
    assert tuple(v.shape) == dims and bool(torch.isfinite(v).all())
