"""ChebProject and the box Helmholtz solve on the device (cheb_project_*, cheb_helmholtz_create_box).

The box solver against the dense scaled model of tests/project_ref.py, and bit for bit against today's handle where the scale
is 1.  The projection: phi is the composition ChebGrad.div -> face rule -> HelmholtzSolver.solve_full bit for bit (signs, faces,
flux, open faces, batch layout, without a tolerance); out within the per-element sweep bar of the phi that came back; in-place,
out-of-place and repeated calls give the same bits; interior divergence, wall-normal velocity, idempotence and projected
gradients within the bars project_ref.py derives from eps = 1e-9 max|phi|.  Every case prints its ratios value / bar
(profiles/project/ratios.txt)."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import project_ref as pr

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
ids = lambda d: "x".join(map(str, d))

SHAPES = [(9,), (12, 10), (8, 7, 6), (7, 6, 5, 6), (66, 12, 5), (20, 18, 16), (63, 64, 65), (130, 70), (258, 6)]
BOX = (0.5, 2.0, 1.25, 0.8)                     # the non-unit scale of a d-dimensional case: its first d values
FACES = ("walls", "open_first", "open_last")
CASES = [(dims, f, sc, 1) for dims in SHAPES for f in FACES for sc in (False, True)]
CASES += [((8, 7, 6), f, True, 2) for f in FACES] + [((20, 18, 16), f, sc, 2) for f, sc in (("walls", False), ("open_last", True))]


def faces_bc(d, faces):
    return {"walls": None, "open_first": [("open", "wall")] + ["wall"] * (d - 1), "open_last": ["wall"] * (d - 1) + [("wall", "open")]}[faces]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inner_of(t, dims):
    """The interior values of stacked full-grid fields (nf, *dims), as a contiguous (nf * G) tensor."""
    return t[(slice(None),) + tuple(slice(1, -1) for _ in dims)].contiguous().reshape(-1)


# ----------------------------------------------------------------------------------------------
# the box solver
# ----------------------------------------------------------------------------------------------
def box_bcs(d, kind):
    robin = [(1.0, 1.0), (3.0, 0.1), (2.0, 0.5), (0.5, 2.0)]
    if kind == "neumann":
        return ["neumann"] * d
    if kind == "robin":
        return [robin[k % 4] for k in range(d)]
    out = [((1.0, 1.0) if k % 2 else "neumann") for k in range(d)]
    k = {"mixed_first": 0, "mixed_last": d - 1}[kind]
    out[k] = ("dirichlet", "neumann") if k % 2 == 0 else ((2.0, 1.0), "neumann")
    return out


@pytest.mark.parametrize("kind,sigma", [("neumann", 1.0), ("robin", 0.0), ("mixed_first", 0.5), ("mixed_last", 0.0)])
@pytest.mark.parametrize("dims", [(9,), (12, 10), (8, 7, 6), (7, 6, 5, 6), (66, 12, 5)], ids=ids)
def test_box_solver_against_dense(dims, kind, sigma):
    d = len(dims)
    bc, scale = box_bcs(d, kind), BOX[:d]
    h = sp.HelmholtzSolver(dims, sigma, bc=bc, scale=scale)
    N, G = int(np.prod(dims)), int(np.prod([P - 2 for P in dims]))
    assert (h.size, h.full_size, h.boundary_size, h.singular, h.scale) == (G, N, N - G, False, scale)
    rng = np.random.default_rng(d * 5 + len(kind))
    f, g = rng.standard_normal(G), rng.standard_normal(N - G)
    b4 = sp.bc_array(bc, d)
    ends = [((b4[4 * k], b4[4 * k + 1]), (b4[4 * k + 2], b4[4 * k + 3])) for k in range(d)]
    ref = pr.dense_helmholtz(dims, ends, scale, sigma, f, g).ravel()
    u = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    h.solve_full(cuda(f), cuda(g), u)
    torch.cuda.synchronize()
    out = u.cpu().numpy()
    assert np.all(np.isfinite(out))
    err = np.linalg.norm(out - ref) / np.linalg.norm(ref)
    node = np.abs(out - ref).max() / np.abs(ref).max()
    print("box %s %s sigma %g: normwise %.3g (bar 1e-11), node by node %.3g (bar 1e-10)" % (ids(dims), kind, sigma, err, node))
    assert err <= 1e-11, err
    assert node <= 1e-10                                                  # edges and corners included
    # the convenience wrapper takes the scale through
    ff = np.zeros(dims); ff[tuple(slice(1, -1) for _ in dims)] = f.reshape([P - 2 for P in dims])
    u2 = solve.helmholtz_bvp(sp, dims, cuda(ff.ravel()), cuda(g), bc, sigma=sigma, scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(u2, u)
    h.destroy()


@pytest.mark.parametrize("dims", [(9,), (12, 10), (8, 7, 6), (66, 12, 5), (64, 64, 64)], ids=ids)
def test_box_unit_scale_is_todays_handle(dims):
    d = len(dims)
    bc = box_bcs(d, "mixed_last")
    h0 = sp.HelmholtzSolver(dims, 0.5, bc=bc)
    rng = np.random.default_rng(2)
    f, g = cuda(rng.standard_normal(h0.size)), cuda(rng.standard_normal(h0.boundary_size))
    u0 = torch.empty(h0.full_size, dtype=torch.float64, device="cuda")
    h0.solve_full(f, g, u0)
    hp = C.c_void_p()                                # scale NULL at the C entry
    b = sp.bc_array(bc, d)
    sp._chk(sp.lib().cheb_helmholtz_create_box(d, sp._ints(dims), (C.c_double * len(b))(*b), None, 0.5, 1, C.byref(hp)))
    un = torch.empty_like(u0)
    sp._chk(sp.lib().cheb_helmholtz_solve_bc(hp, f.data_ptr(), g.data_ptr(), un.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(un, u0)
    sp.lib().cheb_helmholtz_destroy(hp)
    h1 = sp.HelmholtzSolver(dims, 0.5, bc=bc, scale=(1.0,) * d)
    u1 = torch.empty_like(u0)
    h1.solve_full(f, g, u1)
    torch.cuda.synchronize()
    assert torch.equal(u1, u0)
    h0.destroy(); h1.destroy()


def test_box_equal_extents_different_scales():
    """Two directions of equal extent and equal ends but different scale are different lines: x and y swapped must swap the answer."""
    dims, bc = (10, 10), ["neumann", "neumann"]
    rng = np.random.default_rng(4)
    f, g = rng.standard_normal((8, 8)), rng.standard_normal(36)
    ref = pr.dense_helmholtz(dims, [(pr.WALL, pr.WALL)] * 2, (0.5, 2.0), 1.0, f.ravel(), g).ravel()
    h = sp.HelmholtzSolver(dims, 1.0, bc=bc, scale=(0.5, 2.0))
    u = torch.empty(100, dtype=torch.float64, device="cuda")
    h.solve_full(cuda(f.ravel()), cuda(g), u)
    torch.cuda.synchronize()
    assert np.abs(u.cpu().numpy() - ref).max() <= 1e-10 * np.abs(ref).max()
    h.destroy()


# ----------------------------------------------------------------------------------------------
# the projection
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,faces,scaled,nvec", CASES, ids=["%s-%s-%s-nv%d" % (ids(c[0]), c[1], "box" if c[2] else "unit", c[3]) for c in CASES])
def test_project(dims, faces, scaled, nvec):
    d = len(dims)
    scale = BOX[:d] if scaled else None
    bc = faces_bc(d, faces)
    kinds = pr.kinds_of(bc, d)
    N, G = int(np.prod(dims)), int(np.prod([n - 2 for n in dims]))
    NB = N - G
    rng = np.random.default_rng(d * 13 + len(faces) + 2 * scaled + nvec)
    u_h = rng.standard_normal((nvec * d,) + dims)
    flux_h = 0.3 * rng.standard_normal((nvec, NB)) if scaled else None           # a non-zero flux with every box case
    u = cuda(u_h)
    flux = None if flux_h is None else cuda(flux_h)

    P = sp.ChebProject(dims, nvec, bc, scale)
    assert (P.size, P.interior_size, P.boundary_size, P.singular) == (N, G, NB, faces == "walls")
    phi = torch.full((nvec,) + dims, float("nan"), dtype=torch.float64, device="cuda")
    out = P.project(u, phi=phi, flux=flux)
    torch.cuda.synchronize()
    assert torch.equal(u, cuda(u_h))                                           # the input is untouched
    out_h, phi_h = out.cpu().numpy(), phi.cpu().numpy()
    assert out.shape == (nvec * d,) + dims and np.all(np.isfinite(out_h)) and np.all(np.isfinite(phi_h))

    # phi is the composition, bit for bit
    gr = sp.ChebGrad(dims, scale)
    f = -inner_of(gr.div(u), dims)
    g = cuda(np.stack([pr.boundary_data(dims, kinds, u_h[v * d:(v + 1) * d], None if flux_h is None else flux_h[v]) for v in range(nvec)]))
    hs = sp.HelmholtzSolver(dims, 0.0, nfields=nvec, bc=pr.ends_of(kinds), scale=scale)
    assert hs.singular == P.singular
    ref = torch.empty(nvec * N, dtype=torch.float64, device="cuda")
    hs.solve_full(f, g.reshape(-1), ref)
    torch.cuda.synchronize()
    assert torch.equal(phi.reshape(-1), ref)
    hs.destroy()

    # in place, and again: the same bits
    u2, phi2 = u.clone(), torch.empty_like(phi)
    assert P.project(u2, out=u2, phi=phi2, flux=flux) is u2
    out3, phi3 = torch.empty_like(out), torch.empty_like(phi)
    P.project(u, out=out3, phi=phi3, flux=flux)
    torch.cuda.synchronize()
    assert torch.equal(u2, out) and torch.equal(phi2, phi) and torch.equal(out3, out) and torch.equal(phi3, phi)

    # idempotence and projected gradients (device work first, the bars below)
    again = P.project(out, flux=flux).cpu().numpy()
    psi_h = np.stack([pr.psi_field(dims, kinds, 100 + v) for v in range(nvec)])
    gphi = torch.empty_like(phi)
    gout = P.project(gr.grad(cuda(psi_h)), phi=gphi).cpu().numpy()
    gphi_h = gphi.cpu().numpy()
    P.destroy(); gr.destroy()

    tag = "%s nv %d %s scale %s" % (ids(dims), nvec, faces, "s" if scaled else "1")
    for v in range(nvec):
        uv, ov, pv = u_h[v * d:(v + 1) * d], out_h[v * d:(v + 1) * d], phi_h[v]
        fv = None if flux_h is None else flux_h[v]
        eps = 1e-9 * np.abs(pv).max()
        r = {"out": pr.out_ratio(dims, scale, uv, pv, ov),
             "div": pr.div_ratio(dims, scale, uv, pv, ov, eps, spread=faces == "walls"),
             "normal": pr.normal_ratio(dims, kinds, scale, ov, fv, eps),
             "idem": pr.node_ratio(dims, scale, again[v * d:(v + 1) * d] - ov, eps),
             "grad": pr.node_ratio(dims, scale, gout[v * d:(v + 1) * d], 1e-9 * np.abs(gphi_h[v]).max())}
        print("%s vector %d: %s of the bar" % (tag, v, ", ".join("%s %.3g" % kv for kv in r.items())))
        for name, val in r.items():
            assert val <= 1.0, (name, val)


def test_project_velocity_wrapper():
    dims, scale, bc = (12, 10), (1.0, 3.0), ["wall", ("wall", "open")]
    u = cuda(np.random.default_rng(8).standard_normal((4,) + dims))
    out, phi = solve.project_velocity(sp, dims, u, bc=bc, scale=scale)
    P = sp.ChebProject(dims, 2, bc, scale)
    phi2 = torch.empty(2, *dims, dtype=torch.float64, device="cuda")
    out2 = P.project(u, phi=phi2)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(phi, phi2)
    P.destroy()
    with pytest.raises(ValueError):
        solve.project_velocity(sp, dims, u[:3])


def test_argument_errors():
    L = sp.lib()
    dims = (8, 7)
    P = sp.ChebProject(dims, 2)
    N, NB = P.size, P.boundary_size
    buf = torch.zeros(2 * 2 * N + 2 * N + 2 * NB + 2 * 2 * N, dtype=torch.float64, device="cuda")
    u, phi, flux, out = buf[:4 * N], buf[4 * N:6 * N], buf[6 * N:6 * N + 2 * NB], buf[6 * N + 2 * NB:]
    p = lambda t: t.data_ptr()
    assert L.cheb_project_apply(P._h, p(u), p(flux), p(phi), p(out), None) == 0
    assert L.cheb_project_apply(P._h, p(u), None, p(phi), p(u), None) == 0                       # in place, no flux
    assert L.cheb_project_apply(None, p(u), None, p(phi), p(out), None) == 4
    assert L.cheb_project_apply(P._h, None, None, p(phi), p(out), None) == 4
    assert L.cheb_project_apply(P._h, p(u), None, None, p(out), None) == 4                       # phi is required
    assert L.cheb_project_apply(P._h, p(u), None, p(phi), None, None) == 4
    assert L.cheb_project_apply(P._h, p(u), None, p(phi), p(u) + 8, None) == 4                   # out overlaps u without being u
    assert L.cheb_project_apply(P._h, p(u), None, p(u), p(out), None) == 4                       # phi overlaps u
    assert L.cheb_project_apply(P._h, p(u), None, p(out), p(out), None) == 4                     # phi overlaps out
    assert L.cheb_project_apply(P._h, p(u), p(u), p(phi), p(out), None) == 4                     # flux overlaps u
    assert L.cheb_project_apply(P._h, p(u), p(phi), p(phi), p(out), None) == 4                   # flux overlaps phi
    assert L.cheb_project_apply(P._h, p(u), p(out), p(phi), p(out), None) == 4                   # flux overlaps out
    torch.cuda.synchronize()
    assert [L.cheb_project_size(P._h, w) for w in (0, 1, 2, 3, -1)] == [56, 30, 26, -1, -1] and L.cheb_project_singular(P._h) == 1
    for bad in (u[:-1], u.float(), u.cpu()):
        with pytest.raises(AssertionError):
            P.project(bad)
    with pytest.raises(AssertionError):
        P.project(u, flux=flux[:-1])
    P.destroy()
    for kw in (dict(dims=(8, 7, 6), nvec=6), dict(dims=(8, 2)), dict(dims=(8, 259)), dict(dims=(8, 7), scale=(1.0, 0.0)),
               dict(dims=(8, 7), scale=(1.0, float("inf"))), dict(dims=(8, 7), nvec=0)):
        with pytest.raises(sp.ChebhipError):
            sp.ChebProject(**kw)
    for kw in (dict(dims=(8, 7), bc=["wall"]), dict(dims=(8, 7), bc=["wall", "neumann"]), dict(dims=(8, 7), scale=(1.0,))):
        with pytest.raises(ValueError):
            sp.ChebProject(**kw)
    h = C.c_void_p()
    assert L.cheb_project_create(2, sp._ints(dims), sp._ints([0, 0, 0, 7]), None, 1, C.byref(h)) == 4 and h.value is None
    with pytest.raises(ValueError):
        sp.HelmholtzSolver(dims, scale=(1.0, 2.0))                                               # scale without bc
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver(dims, bc=["neumann", "neumann"], scale=(1.0, -2.0))
    Pn = sp.ChebProject(dims, bc=["open", "wall"])
    assert not Pn.singular
    Pn.destroy()
