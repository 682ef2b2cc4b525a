"""ChebProject(variable=True) on the device: out_k = u_k - kappa s_k d_k phi with phi from VarHelmholtz.solve_deflated.

Shapes: (7, 6, 8) walls; (8, 7, 6) periodic / wall / periodic on a box (two even periodic extents: q = 4); (6, 7) with one open
face (nonsingular); one and two vectors; kappa of contrast 19; flux None and given; rtol 1e-10, restart 64.

  1  the correction, given the device's phi: |out - (u - kappa s_k D_k phi)| <= (K + 8 + 3) U (|u| + kappa s_k B(D_k, phi)) per
     element, truth in long double -- one sweep (linewise's K + 8), kappa, the scale (inside the sweep's alpha), the subtraction;
  2  wall nodes: |+-out_k - flux| <= kappa s_k d (max M + 2) U Ba, Ba the extension with every factor's absolute value;
  3  the divergence of out in long double at the unknown nodes: with an open face |div out| <= 1.05 rtol |b| + |rnd|, with walls and
     periodic directions only the same for Pi div(out); rnd is the rounding of the chain, element by element: the correction's bar
     carried through sum_k s_k |D_k|, the library's divergence of u ((max n + 8 + d) U sum_k s_k B(D_k, u_k), grad_ref's count) and
     the residual's bar cap U A of varhelm_ref; `defect` against the null components of -div(out) within sum |rnd| / G + bar 5;
  4  kappa == 1 against ChebProject(variable=False).project: the potentials differ by bar 4 of varhelm_singular_ref (or by
     |A^-1| |r| with an open face) and by null vectors, whose gradient is zero;
  5  warm starts, in place, repeats, variable=False, arguments.

Where VARHELM_PROJECT_RATIOS_OUT names a file the worst measured ratio to each bar is written there (appended to
profiles/varhelm/singular_ratios.txt)."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import linewise as lw
import varhelm_ref as vr
import varhelm_singular_ref as sr

pytestmark = pytest.mark.gpu
sp = ge.load()
LD = np.longdouble
U = sr.U
SEED = 20261022
RTOL = 1e-10
OPTS = dict(rtol=RTOL, max_it=200, restart=64)

RATIOS = {}


def note(bar, case, ratio):
    RATIOS[(bar, case)] = max(RATIOS.get((bar, case), 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("VARHELM_PROJECT_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst measured / bar per case (tests/test_gpu_project_variable.py)\n")
            for key in sorted(RATIOS):
                f.write("%-28s %-24s %10.4f\n" % (key[0], key[1], RATIOS[key]))


# (dims, bc of ChebProject, scale)
CASES = [
    ((7, 6, 8), ["wall"] * 3, None),
    ((8, 7, 6), ["periodic", "wall", "periodic"], (0.5, 1.0, 2.0)),
    ((6, 7), ["wall", ("wall", "open")], (1.0, 0.7)),
]
case_id = lambda i: "x".join(map(str, CASES[i][0]))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def solver_bc(bc):
    """VarHelmholtz's bc of phi: Neumann at a wall, Dirichlet at an open face."""
    one = lambda e: {"wall": "neumann", "open": "dirichlet", "periodic": "periodic"}[e]
    return [one(e) if isinstance(e, str) else tuple(one(x) for x in e) for e in bc]


@functools.lru_cache(maxsize=None)
def setup(i, amp):
    dims, bc, scale = CASES[i]
    p = sr.problem(sp, dims, solver_bc(bc), scale, amp)
    kinds = [None if per else ((e, e) if isinstance(e, str) else tuple(e)) for e, per in zip(bc, p.periodic)]
    singular = all(k is None or k == ("wall", "wall") for k in kinds)
    N = sr.null_matrix(sp, p) if singular else None
    A = p.dense()[0]
    if singular:
        _, Binv, cond = sr.bordered(A, N)
    else:
        A64 = A.astype(np.float64)
        Binv, cond = np.linalg.inv(A64), np.linalg.cond(A64)
    face = np.full(p.dims, -1)
    face[p.bmask] = sp.project_faces(p.dims, p.periodic)
    return p, kinds, N, Binv, cond, face


def boundary_data(p, kinds, face, u, flux):
    """g of ONE vector u (d, *dims), compact: (+-u_k - flux) / kappa at the nodes of a wall, 0 at those of an open face -- the
    operations k_project_rhs performs, so the same bits."""
    code = face[p.bmask]
    g = np.zeros(p.NB)
    kap = p.kappa[p.bmask]
    for k in range(p.d):
        if kinds[k] is None:
            continue
        uk = u[k][p.bmask]
        for e in range(2):
            sel = code == 2 * k + e
            if kinds[k][e] == "wall":
                val = uk[sel] if e == 0 else -uk[sel]
                if flux is not None:
                    val = val - flux[sel]
                g[sel] = val / kap[sel]
    return g


def inputs(p, nvec, with_flux, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((nvec * p.d,) + p.dims)
    flux = 0.3 * rng.standard_normal((nvec, p.NB)) if with_flux else None
    return u, flux


def correction(p, u, phi):
    """(truth, W, cap per direction) of out_k = u_k - kappa s_k D_k phi for ONE vector."""
    t, W, caps = [], [], []
    for k in range(p.d):
        s = p.scale[k]
        t.append(u[k].astype(LD) - p.kappa.astype(LD) * LD(s) * lw.truth(p.D[k], phi, k))
        W.append(np.abs(u[k]) + p.kappa * s * lw.bound(p.D[k], phi, k))
        caps.append(p.dims[k] + 8 + 3)
    return t, W, caps


def divergence(p, out):
    """sum_k s_k D_k out_k of ONE vector at the unknown nodes, long double."""
    dv = np.zeros(p.dims, dtype=LD)
    for k in range(p.d):
        dv = dv + LD(p.scale[k]) * lw.truth(p.D[k], out[k], k)
    return dv[p.inner].reshape(-1)


def chain_rounding(p, u, phi, x, g, f):
    """rnd of the module docstring for ONE vector, at the unknown nodes."""
    _, W, caps = correction(p, u, phi)
    rnd = np.zeros(p.dims)
    Bu = np.zeros(p.dims)
    for k in range(p.d):
        Dk = np.abs(p.D[k].astype(np.float64))
        rnd = rnd + p.scale[k] * np.moveaxis(np.tensordot(Dk, caps[k] * U * W[k], axes=([1], [k])), 0, k)
        Bu = Bu + p.scale[k] * lw.bound(p.D[k], u[k], k)
    rnd = rnd + U * (max(p.dims) + 8 + p.d) * Bu
    return rnd[p.inner].reshape(-1) + p.cap * U * p.apply(x, g, f)[1]


def abs_extension(p, x, g):
    pa = copy.copy(p)
    pa.Q = [None if Q is None else np.abs(Q) for Q in p.Q]
    pa.Binv = [None if B is None else np.abs(B) for B in p.Binv]
    return pa.extend_full(np.abs(x), np.abs(g))


def wall_ratio(p, kinds, face, ov, fv, g, x):
    """Worst |+-out_k - flux| / (kappa s_k d (max M + 2) U Ba) over the nodes that take a wall's condition: the extension's bar
    times kappa s_k.  The library meets it because it takes the normal derivative at such a node from the condition that defines
    phi's end value there (k_project_wall_grad), not from the sweep, which would carry the end values' rounding through the row of
    D_k -- corner entry (2 n^2 + 1) / 6 -- and miss this bar by 1.2 - 7.8 times on these shapes."""
    d = p.d
    Ba = d * (max(p.M) + 2) * U * abs_extension(p, x, g)
    worst = 0.0
    for k in range(d):
        if kinds[k] is None:
            continue
        for e in range(2):
            sel = face == 2 * k + e
            if kinds[k][e] != "wall" or not sel.any():
                continue
            nrm = ov[k][sel] if e == 0 else -ov[k][sel]
            fl = 0.0 if fv is None else fv[sel[p.bmask]]
            worst = max(worst, float((np.abs(nrm - fl) / (p.kappa[sel] * p.scale[k] * Ba[sel])).max()))
    return worst


@pytest.mark.parametrize("with_flux", [False, True], ids=["noflux", "flux"])
@pytest.mark.parametrize("nvec", [1, 2])
@pytest.mark.parametrize("i", range(len(CASES)), ids=case_id)
def test_variable_projection(i, nvec, with_flux):
    p, kinds, N, Binv, cond, face = setup(i, 0.9)
    dims, bc, scale = CASES[i]
    d, G = p.d, p.G
    u_h, flux_h = inputs(p, nvec, with_flux, SEED + 10 * i + nvec)
    u, flux = cuda(u_h), None if flux_h is None else cuda(flux_h)
    P = sp.ChebProject(dims, nvec, bc, scale, variable=True)
    try:
        assert P.variable and P.singular == (N is not None) and (P.size, P.interior_size, P.boundary_size) == (p.N, G, p.NB)
        P.set_inverse_density(cuda(p.kappa).reshape(-1))
        q = 0 if N is None else N.shape[1]
        assert P.null_count == q
        phi = torch.full((nvec,) + dims, float("nan"), dtype=torch.float64, device="cuda")
        out = P.project(u, phi=phi, flux=flux, **OPTS)
        its = P.iterations
        assert P.reason == 2 and 0 < its <= 100, (P.reason, its)
        lam = P.defect
        assert lam.shape == (nvec, q)
        out_h, phi_h = host(out).copy(), host(phi).copy()
        assert np.array_equal(host(u), u_h), "the input is untouched"
        tag = "%s nvec %d %s" % (case_id(i), nvec, "flux" if with_flux else "noflux")
        dvs, rnds, bs = [], [], []
        for v in range(nvec):
            uv, ov, pv = u_h[v * d:(v + 1) * d], out_h[v * d:(v + 1) * d], phi_h[v]
            fv = None if flux_h is None else flux_h[v]
            # 1: the correction
            t, W, caps = correction(p, uv, pv)
            for k in range(d):
                r, _ = lw.check(ov[k], t[k], W[k], caps[k], "%s vector %d component %d" % (tag, v, k))
                print("%s vector %d component %d: correction at %.3f x 2^-53 W (cap %d)" % (tag, v, k, r, caps[k]))
                note("P1 correction", case_id(i), r / caps[k])
            # 2: the normal velocity at the nodes of a wall
            g = boundary_data(p, kinds, face, uv, fv)
            x = pv[p.inner].reshape(-1)
            worst = wall_ratio(p, kinds, face, ov, fv, g, x)
            print("%s vector %d: normal velocity at %.3f of the wall bar" % (tag, v, worst))
            note("P2 wall nodes", case_id(i), worst)
            assert worst <= 1.0
            # 3: the divergence
            f = -divergence(p, uv).astype(np.float64)
            dvs.append(divergence(p, ov)); rnds.append(chain_rounding(p, uv, pv, x, g, f))
            bs.append(p.apply(np.zeros(G), g, f)[0])
        dv, rnd, b = np.stack(dvs), np.stack(rnds), np.stack(bs)
        if N is not None:
            pdv = np.stack([sr.project(N, dv[v], LD) for v in range(nvec)]).astype(np.float64)
            pb = np.stack([sr.project(N, b[v], LD) for v in range(nvec)]).astype(np.float64)
        else:
            pdv, pb = dv.astype(np.float64), b.astype(np.float64)
        bar = 1.05 * RTOL * np.linalg.norm(pb) + np.linalg.norm(rnd)
        print("%s: |%sdiv out| = %.3e at %.3f of its bar (%d iterations)" % (tag, "Pi " if N is not None else "", np.linalg.norm(pdv), np.linalg.norm(pdv) / bar, its))
        note("P3 divergence", case_id(i), np.linalg.norm(pdv) / bar)
        assert np.linalg.norm(pdv) <= bar
        for v in range(nvec):
            if N is None:
                continue
            want = -(N.T.astype(LD) @ dv[v] / G).astype(np.float64)
            tol = np.abs(rnd[v]).sum() / G + sr.bar5(dv[v].astype(np.float64), G)
            print("%s vector %d: defect %s against -N^T div(out) / G at %.3f of its bar" % (tag, v, lam[v], (np.abs(lam[v] - want) / tol).max()))
            note("P3 defect", case_id(i), (np.abs(lam[v] - want) / tol).max())
            assert np.all(np.abs(lam[v] - want) <= tol)
        # 5: warm from the same input: no iteration, the same bits; in place; again
        phi2 = torch.empty_like(phi)
        out2 = P.project(u, phi=phi2, flux=flux, warm=True, **OPTS)
        assert P.iterations == 0 and P.reason == 2
        assert np.array_equal(host(out2), out_h) and np.array_equal(host(phi2), phi_h)
        u3, phi3 = u.clone(), torch.empty_like(phi)
        assert P.project(u3, out=u3, phi=phi3, flux=flux, **OPTS) is u3 and P.iterations == its
        assert np.array_equal(host(u3), out_h) and np.array_equal(host(phi3), phi_h)
        assert np.array_equal(host(P.project(u, flux=flux, **OPTS)), out_h)
    finally:
        P.destroy()


@pytest.mark.parametrize("i", range(len(CASES)), ids=case_id)
def test_unit_density_against_the_direct_projection(i):
    p, kinds, N, Binv, cond, face = setup(i, 0.0)
    dims, bc, scale = CASES[i]
    d, G, nvec = p.d, p.G, 2
    u_h, flux_h = inputs(p, nvec, True, SEED + 50 + i)
    u, flux = cuda(u_h), cuda(flux_h)
    Pv, Pc = sp.ChebProject(dims, nvec, bc, scale, variable=True), sp.ChebProject(dims, nvec, bc, scale)
    try:
        Pv.set_inverse_density(cuda(np.ones(dims)).reshape(-1))
        phiv, phic = torch.empty((nvec,) + dims, dtype=torch.float64, device="cuda"), torch.empty((nvec,) + dims, dtype=torch.float64, device="cuda")
        ov = host(Pv.project(u, phi=phiv, flux=flux, **OPTS)).copy()
        assert Pv.reason == 2 and Pv.iterations <= 2, (Pv.reason, Pv.iterations)
        oc = host(Pc.project(u, phi=phic, flux=flux)).copy()
        pv_h, pc_h = host(phiv), host(phic)
        for v in range(nvec):
            uv = u_h[v * d:(v + 1) * d]
            g = boundary_data(p, kinds, face, uv, flux_h[v])
            f = -divergence(p, uv).astype(np.float64)
            xv, xc = pv_h[v][p.inner].reshape(-1), pc_h[v][p.inner].reshape(-1)
            r = p.apply(xv, g, f)[0].astype(np.float64)
            if N is not None:
                dx = sr.bar4(Binv, cond, N, sr.project(N, r, LD).astype(np.float64), xv, xc)
            else:
                dx = np.abs(Binv) @ np.abs(r) + 16.0 * U * cond * np.abs(xc).max()
            # the unknowns' difference on the full grid (the extension with absolute values), then the extension's own rounding
            # on both potentials; what the potentials differ by along the null vectors has zero gradient
            dphi = abs_extension(p, dx, np.zeros(p.NB)) + 2 * d * (max(p.M) + 2) * U * abs_extension(p, np.maximum(np.abs(xv), np.abs(xc)), g)
            _, Wv, caps = correction(p, uv, pv_h[v])
            _, Wc, _ = correction(p, uv, pc_h[v])
            for k in range(d):
                Dk = np.abs(p.D[k].astype(np.float64))
                bar = p.scale[k] * np.moveaxis(np.tensordot(Dk, dphi, axes=([1], [k])), 0, k) + caps[k] * U * (Wv[k] + Wc[k])
                ratio = (np.abs(ov[v * d + k] - oc[v * d + k]) / bar).max()
                print("%s vector %d component %d: variable - direct at %.3f of its bar" % (case_id(i), v, k, ratio))
                note("P4 unit density", case_id(i), ratio)
                assert ratio <= 1.0
    finally:
        Pv.destroy(); Pc.destroy()


def test_constant_density_handles_are_todays():
    """variable=False: the potential is the composition divergence, right-hand sides, direct solve, bit for bit, and a variable
    handle beside it changes nothing."""
    i, nvec = 1, 2
    p, kinds, N, Binv, cond, face = setup(i, 0.0)
    dims, bc, scale = CASES[i]
    d = p.d
    u_h, flux_h = inputs(p, nvec, True, SEED + 70)
    u, flux = cuda(u_h), cuda(flux_h)
    Pc = sp.ChebProject(dims, nvec, bc, scale)
    phi = torch.empty((nvec,) + dims, dtype=torch.float64, device="cuda")
    before = host(Pc.project(u, phi=phi, flux=flux)).copy()
    Pv = sp.ChebProject(dims, nvec, bc, scale, variable=True)
    gr = sp.ChebGrad(dims, scale, p.periodic)
    hs = sp.HelmholtzSolver(dims, 0.0, nfields=nvec, bc=solver_bc(bc), scale=scale)
    try:
        Pv.set_inverse_density(cuda(vr.kappa_field(dims, p.periodic)).reshape(-1))
        Pv.project(u, flux=flux, **OPTS)
        assert not Pc.variable and Pc.null_count == 0 and Pc.defect.shape == (nvec, 0)
        phi2 = torch.empty_like(phi)
        assert np.array_equal(host(Pc.project(u, phi=phi2, flux=flux)), before) and torch.equal(phi2, phi)
        f = -gr.div(u).reshape((nvec,) + dims)[(slice(None),) + p.inner].contiguous().reshape(-1)
        g = np.stack([boundary_data(p, kinds, face, u_h[v * d:(v + 1) * d], flux_h[v]) for v in range(nvec)])   # (kappa == 1: x / 1 = x)
        ref = torch.empty(nvec * p.N, dtype=torch.float64, device="cuda")
        hs.solve_full(f, cuda(g).reshape(-1), ref)
        torch.cuda.synchronize()
        assert torch.equal(phi.reshape(-1), ref)
        with pytest.raises(sp.ChebhipError) as e:
            Pc.set_inverse_density(cuda(np.ones(dims)).reshape(-1))
        assert e.value.code == 4 and "create_variable" in str(e.value)
    finally:
        Pc.destroy(); Pv.destroy(); gr.destroy(); hs.destroy()


def test_project_velocity_passes_the_density_through():
    solve = __import__("importlib").import_module(sp.__name__ + ".solve")
    i = 2
    p, kinds, N, Binv, cond, face = setup(i, 0.9)
    dims, bc, scale = CASES[i]
    u = cuda(np.random.default_rng(SEED + 80).standard_normal((2 * p.d,) + dims))
    out, phi = solve.project_velocity(sp, dims, u, bc=bc, scale=scale, inverse_density=cuda(p.kappa), **OPTS)
    P = sp.ChebProject(dims, 2, bc, scale, variable=True)
    try:
        P.set_inverse_density(cuda(p.kappa).reshape(-1))
        phi2 = torch.empty_like(phi)
        out2 = P.project(u, phi=phi2, **OPTS)
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(phi, phi2)
    finally:
        P.destroy()
    with pytest.raises(ValueError):
        solve.project_velocity(sp, dims, u, bc=bc, scale=scale, rtol=1e-6)


def test_argument_errors():
    dims = (8, 7)
    P = sp.ChebProject(dims, 2, variable=True)
    try:
        N, NB = P.size, P.boundary_size
        u = cuda(np.random.default_rng(SEED + 90).standard_normal((4,) + dims))
        with pytest.raises(sp.ChebhipError) as e:
            P.project(u)
        assert e.value.code == 4 and "set_inverse_density" in str(e.value)
        kap = vr.kappa_field(dims, (False, False))
        for bad in (0.0, -1.0, np.nan, np.inf):
            k = kap.copy()
            k[3, 2] = bad
            with pytest.raises(sp.ChebhipError) as e:
                P.set_inverse_density(cuda(k).reshape(-1))
            assert e.value.code == 4
        with pytest.raises(sp.ChebhipError):
            P.project(u)                                             # a refused density leaves the handle without one
        P.set_inverse_density(cuda(kap).reshape(-1))
        good = host(P.project(u, **OPTS)).copy()
        k = kap.copy()
        k[0, 0] = -2.0
        with pytest.raises(sp.ChebhipError):
            P.set_inverse_density(cuda(k).reshape(-1))
        assert np.array_equal(host(P.project(u, **OPTS)), good), "a refused density leaves the earlier one in place"
        phi = torch.empty((2,) + dims, dtype=torch.float64, device="cuda")
        with pytest.raises(sp.ChebhipError) as e:
            P.project(u, restart=0)
        assert e.value.code == 4 and "restart" in str(e.value)
        L = sp.lib()
        p = lambda t: t.data_ptr()
        out = torch.empty_like(u)
        assert L.cheb_project_apply(P._h, p(u), None, p(phi), p(out), None) == 4, "a variable handle projects with apply_variable"
        assert L.cheb_project_apply_variable(P._h, p(u), None, p(u), p(out), 0, 1e-8, 0.0, 10, 30, None) == 4      # phi overlaps u
        assert L.cheb_project_apply_variable(None, p(u), None, p(phi), p(out), 0, 1e-8, 0.0, 10, 30, None) == 4
        assert L.cheb_project_set_inverse_density(None, p(u), None) == 4
        assert L.cheb_project_varhelm(None) is None
        with pytest.raises(AssertionError):
            P.set_inverse_density(cuda(kap).reshape(-1)[:-1])
    finally:
        P.destroy()
    allp = sp.ChebProject((8, 6), 1, ["periodic", "periodic"], variable=True)
    try:
        allp.set_inverse_density(cuda(vr.kappa_field((8, 6), (True, True))).reshape(-1))
        u = cuda(np.random.default_rng(SEED + 91).standard_normal((2, 8, 6)))
        with pytest.raises(sp.ChebhipError) as e:
            allp.project(u, flux=cuda(np.ones(1)))
        assert e.value.code == 4 and "periodic" in str(e.value)
        allp.project(u, **OPTS)
        assert allp.reason == 2 and allp.null_count == 4
    finally:
        allp.destroy()
