"""Direct Helmholtz solves with Dirichlet, Neumann, Robin and mixed faces (cheb_helmholtz_create_bc / _solve_bc,
HelmholtzSolver(bc=...), solve.helmholtz_bvp): the all-Dirichlet handle against today's solver bit for bit, full-grid output
against a dense numpy Kronecker solve of the same discretisation (edges and corners by the edge rule of DESIGN 10c),
manufactured smooth solutions, the singular all-Neumann problem, batches, the interior route, FGMRES, argument errors."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
ids = lambda d: "x".join(map(str, d))


def cheb_d(P):
    n = P - 1
    i = np.arange(P)
    I, J = np.meshgrid(i, i, indexing="ij")
    c = np.where((i == 0) | (i == n), 2.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dx = -2.0 * np.sin(np.pi * (I + J) / (2 * n)) * np.sin(np.pi * (I - J) / (2 * n))
        D = (c[:, None] / c[None, :]) * (-1.0) ** (I + J) / dx
        s = np.sin(np.pi * i / n)
        dg = -np.cos(np.pi * i / n) / (2.0 * s * s)
    dg[0] = (2.0 * n * n + 1.0) / 6.0
    dg[n] = -dg[0]
    D[i, i] = dg
    return D


def numpy_line(P, e4):
    a0, b0, a1, b1 = e4
    n = P - 1
    D = cheb_d(P)
    DD = D @ D
    B = np.vstack([b0 * D[0], -b1 * D[n]])
    B[0, 0] += a0
    B[1, n] += a1
    Binv = np.linalg.inv(B[:, [0, n]])
    Q = -Binv @ B[:, 1:n]
    DDib = DD[1:n][:, [0, n]]
    return -DD[1:n, 1:n] - DDib @ Q, Q, DDib @ Binv, Binv


def bcs(d, kind):
    """Per-direction bc entries of a named configuration."""
    robin = [(1.0, 1.0), (3.0, 0.1), (2.0, 0.5), (0.5, 2.0)]
    if kind == "neumann":
        return ["neumann"] * d
    if kind == "robin":
        return [robin[k % 4] for k in range(d)]
    out = [((1.0, 1.0) if k % 2 else "neumann") for k in range(d)]
    k = {"mixed_first": 0, "mixed_middle": d // 2, "mixed_last": d - 1}[kind]
    out[k] = ("dirichlet", "neumann") if k % 2 == 0 else ((2.0, 1.0), "neumann")
    return out


def boundary_mask(dims):
    m = np.ones(dims, dtype=bool)
    m[tuple(slice(1, -1) for _ in dims)] = False
    return m


def lines_of(dims, bc):
    b = sp.bc_array(bc, len(dims))
    return [numpy_line(P, b[4 * k:4 * k + 4]) for k, P in enumerate(dims)]


def dense_solve(dims, bc, sigma, f_int, g):
    """The discretisation of DESIGN 10c by a dense solve: interior equations with the lifts, then the ordered extension."""
    d = len(dims)
    Ms = [P - 2 for P in dims]
    lines = lines_of(dims, bc)
    Gn = int(np.prod(Ms))
    A = sigma * np.eye(Gn)
    for k in range(d):
        mats = [np.eye(m) for m in Ms]
        mats[k] = lines[k][0]
        K = mats[0]
        for Mk in mats[1:]:
            K = np.kron(K, Mk)
        A += K
    Gf = np.zeros(dims)
    Gf[boundary_mask(dims)] = g
    rhs = f_int.reshape(Ms).copy()
    inner = [slice(1, -1)] * d
    for k in range(d):
        Lk = lines[k][2]
        for e, idx in enumerate((0, -1)):
            sl = list(inner); sl[k] = idx
            face = Gf[tuple(sl)]                                   # other indices interior
            rhs += np.moveaxis(np.multiply.outer(Lk[:, e], face), 0, k)
    u = np.linalg.solve(A, rhs.ravel())
    U = np.zeros(dims)
    U[tuple(inner)] = u.reshape(Ms)
    for k in range(d):
        _, Q, _, Bi = lines[k]
        sl = tuple([slice(None)] * (k + 1) + [slice(1, -1)] * (d - k - 1))
        V = np.moveaxis(U[sl], k, -1).copy()
        Gd = np.moveaxis(Gf[sl], k, -1)
        end = V[..., 1:-1] @ Q.T + Gd[..., [0, -1]] @ Bi.T
        V[..., 0], V[..., -1] = end[..., 0], end[..., 1]
        U[sl] = np.moveaxis(V, -1, k)
    return U


def manufactured(dims, bc, sigma):
    """u = prod_k cos(a_k x + b_k) exp(c_k x) on the full grid, f = sigma u - Laplace u, and g at each boundary node from the
    condition of the highest direction in which it is an end node."""
    d = len(dims)
    xs = [np.cos(np.pi * np.arange(P) / (P - 1)) for P in dims]
    a = [0.7 + 0.1 * k for k in range(d)]
    b = [0.3 * k for k in range(d)]
    c = 0.2
    phi = [np.cos(a[k] * xs[k] + b[k]) * np.exp(c * xs[k]) for k in range(d)]
    dphi = [(-a[k] * np.sin(a[k] * xs[k] + b[k]) + c * np.cos(a[k] * xs[k] + b[k])) * np.exp(c * xs[k]) for k in range(d)]
    d2phi = [((c * c - a[k] ** 2) * np.cos(a[k] * xs[k] + b[k]) - 2 * a[k] * c * np.sin(a[k] * xs[k] + b[k])) * np.exp(c * xs[k])
             for k in range(d)]

    def prod(fs):
        out = fs[0]
        for f in fs[1:]:
            out = np.multiply.outer(out, f)
        return out
    u = prod(phi)
    lap = sum(prod([d2phi[m] if m == k else phi[m] for m in range(d)]) for k in range(d))
    f = sigma * u - lap
    bb = sp.bc_array(bc, d)
    Gf = np.zeros(dims)
    for k in range(d):
        du = prod([dphi[m] if m == k else phi[m] for m in range(d)])
        a0, b0, a1, b1 = bb[4 * k:4 * k + 4]
        sl0 = tuple([slice(None)] * k + [0]); sl1 = tuple([slice(None)] * k + [-1])
        Gf[sl0] = a0 * u[sl0] + b0 * du[sl0]
        Gf[sl1] = a1 * u[sl1] - b1 * du[sl1]
    return u, f, Gf[boundary_mask(dims)]


def interior(a, dims):
    return a.reshape(dims)[tuple(slice(1, -1) for _ in dims)].ravel()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("dims", [(9,), (12, 10), (8, 7, 6), (66, 12, 5), (12,) * 5, (128, 128, 128)], ids=ids)
def test_dirichlet_handle_bit_identical(dims):
    h0 = sp.HelmholtzSolver(dims)
    h1 = sp.HelmholtzSolver(dims, bc=["dirichlet"] * len(dims))
    assert h1.size == h0.size and not h1.singular
    f = torch.from_numpy(np.random.default_rng(1).standard_normal(h0.size)).cuda()
    u0, u1 = torch.empty_like(f), torch.empty_like(f)
    h0.solve(f, u0); h1.solve(f, u1)
    torch.cuda.synchronize()
    assert torch.equal(u0, u1)
    h0.destroy(); h1.destroy()


DENSE = [(9,), (12, 10), (8, 7, 6), (7, 6, 5, 6), (66, 12, 5)]


@pytest.mark.parametrize("kind,sigma", [("neumann", 1.0), ("robin", 0.0), ("mixed_first", 0.5), ("mixed_middle", 0.0), ("mixed_last", 2.0)])
@pytest.mark.parametrize("dims", DENSE, ids=ids)
def test_against_dense(dims, kind, sigma):
    bc = bcs(len(dims), kind)
    h = sp.HelmholtzSolver(dims, sigma, bc=bc)
    N, G = int(np.prod(dims)), int(np.prod([P - 2 for P in dims]))
    assert (h.size, h.full_size, h.boundary_size, h.singular) == (G, N, N - G, False)
    rng = np.random.default_rng(len(dims) * 7 + len(kind))
    f, g = rng.standard_normal(G), rng.standard_normal(N - G)
    ref = dense_solve(dims, bc, sigma, f, g).ravel()
    u = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    h.solve_full(cuda(f), cuda(g), u)
    torch.cuda.synchronize()
    out = u.cpu().numpy()
    assert np.all(np.isfinite(out))
    err = np.linalg.norm(out - ref) / np.linalg.norm(ref)
    assert err <= 1e-11, err
    assert np.abs(out - ref).max() <= 1e-10 * np.abs(ref).max()          # node by node, edges and corners included
    h.destroy()


@pytest.mark.parametrize("dims,kind,sigma", [((40, 36), "mixed_last", 0.0), ((40, 36), "robin", 1.0), ((130, 70), "mixed_first", 0.0),
                                             ((130, 70), "neumann", 1.0), ((64, 64, 64), "mixed_middle", 0.0),
                                             ((70, 68, 40), "mixed_last", 1.0), ((70, 68, 40), "robin", 0.0),
                                             ((128, 128, 128), "neumann", 1.0), ((128, 128, 128), "mixed_last", 0.0)])
def test_manufactured(dims, kind, sigma):
    bc = bcs(len(dims), kind)
    uex, f, g = manufactured(dims, bc, sigma)
    h = sp.HelmholtzSolver(dims, sigma, bc=bc)
    u = torch.empty(h.full_size, dtype=torch.float64, device="cuda")
    h.solve_full(cuda(interior(f, dims)), cuda(g), u)
    torch.cuda.synchronize()
    err = np.abs(u.cpu().numpy() - uex.ravel()).max() / np.abs(uex).max()
    assert err <= 1e-9, err
    # the convenience wrapper: full-grid f (boundary entries ignored)
    fz = f.copy(); fz[boundary_mask(dims)] = 1e30
    u2 = solve.helmholtz_bvp(sp, dims, cuda(fz.ravel()), cuda(g), bc, sigma=sigma, solver=h)
    torch.cuda.synchronize()
    assert torch.equal(u2, u)
    h.destroy()


@pytest.mark.parametrize("dims", [(40, 36), (24, 20, 18)], ids=ids)
def test_singular_neumann(dims):
    bc = ["neumann"] * len(dims)
    uex, f, g = manufactured(dims, bc, 0.0)
    h = sp.HelmholtzSolver(dims, 0.0, bc=bc)
    assert h.singular
    u = torch.empty(h.full_size, dtype=torch.float64, device="cuda")
    h.solve_full(cuda(interior(f, dims)), cuda(g), u)
    torch.cuda.synchronize()
    out = u.cpu().numpy()
    diff = out - uex.ravel()
    assert np.abs(diff - diff.mean()).max() <= 1e-9 * np.abs(uex).max()
    # no component along the dropped mode: w . u_I = 0, w the product of the zero-mode rows of S^-1
    ui = interior(out, dims).reshape([P - 2 for P in dims])
    wn = 1.0
    for k, P in enumerate(dims):
        S, Si, lam, *_ = sp.helmholtz_line_bc(P, "neumann")
        iz = int(np.flatnonzero(lam == 0.0)[0])
        ui = np.tensordot(Si[iz], ui, axes=([0], [0]))
        wn *= np.linalg.norm(Si[iz])
    assert abs(float(ui)) <= 1e-12 * wn * np.linalg.norm(out), float(ui)
    h.destroy()
    h = sp.HelmholtzSolver(dims, 1.0, bc=bc)
    assert not h.singular
    h.destroy()
    h = sp.HelmholtzSolver(dims, 0.0, bc=["neumann"] * (len(dims) - 1) + [("neumann", (1.0, 1.0))])
    assert not h.singular
    h.destroy()


def test_batch_and_zero_data():
    dims, bc, nf = (24, 20, 18), bcs(3, "mixed_last"), 16
    hb = sp.HelmholtzSolver(dims, 0.5, nfields=nf, bc=bc)
    h1 = sp.HelmholtzSolver(dims, 0.5, bc=bc)
    rng = np.random.default_rng(5)
    f = cuda(rng.standard_normal(nf * h1.size)); g = cuda(rng.standard_normal(nf * h1.boundary_size))
    assert hb.full_size == nf * h1.full_size and hb.boundary_size == nf * h1.boundary_size
    ub = torch.empty(hb.full_size, dtype=torch.float64, device="cuda")
    hb.solve_full(f, g, ub)
    u1 = torch.empty(h1.full_size, dtype=torch.float64, device="cuda")
    for i in range(nf):
        h1.solve_full(f[i * h1.size:(i + 1) * h1.size].contiguous(), g[i * h1.boundary_size:(i + 1) * h1.boundary_size].contiguous(), u1)
        ref = ub[i * h1.full_size:(i + 1) * h1.full_size]
        assert float((ref - u1).norm() / u1.norm()) <= 1e-14
    ua, uz = torch.empty_like(ub), torch.empty_like(ub)
    hb.solve_full(f, None, ua)
    hb.solve_full(f, torch.zeros_like(g), uz)
    torch.cuda.synchronize()
    assert torch.equal(ua, uz)
    # the interior route (g = 0) is the interior of the full-grid one
    ui = torch.empty_like(f)
    hb.solve(f, ui)
    inner = ua.view(nf, *dims)[:, 1:-1, 1:-1, 1:-1].reshape(-1)
    assert torch.equal(ui, inner)
    hb.destroy(); h1.destroy()


def test_fgmres_preconditioner():
    dims, sigma = (20, 18, 16), 0.0
    bc = [(1.0, 1.0), "neumann", ("neumann", (2.0, 1.0))]
    h = sp.HelmholtzSolver(dims, sigma, bc=bc)
    Ms = [P - 2 for P in dims]
    As = []
    for P, e in zip(dims, bc):
        S, Si, lam, *_ = sp.helmholtz_line_bc(P, e)
        As.append(torch.from_numpy((S * lam[None, :]) @ Si).cuda())

    def A(x, y):
        X = x.view(*Ms)
        Y = sigma * X
        for k, Ak in enumerate(As):
            Y = Y + torch.movedim(torch.tensordot(Ak, X, dims=([1], [k])), 0, k)
        y.copy_(Y.reshape(-1))
    b = cuda(np.random.default_rng(3).standard_normal(h.size))
    x = torch.zeros_like(b)
    ks = sp.Fgmres(h.size, rtol=1e-12)
    ks.solve(A, b, x, M=h)
    torch.cuda.synchronize()
    assert ks.iterations <= 1, ks.iterations
    r = torch.empty_like(b)
    A(x, r)
    assert float((r - b).norm() / b.norm()) <= 1e-12
    ks.destroy(); h.destroy()


def test_argument_errors():
    L = sp.lib()
    h = sp.HelmholtzSolver((8, 7), bc=["neumann", ("dirichlet", (1.0, 1.0))])
    f = torch.zeros(h.size, dtype=torch.float64, device="cuda")
    g = torch.zeros(h.boundary_size, dtype=torch.float64, device="cuda")
    u = torch.zeros(h.full_size, dtype=torch.float64, device="cuda")
    assert L.cheb_helmholtz_solve_bc(h._h, None, g.data_ptr(), u.data_ptr(), None) == 4
    assert L.cheb_helmholtz_solve_bc(h._h, f.data_ptr(), g.data_ptr(), None, None) == 4
    assert L.cheb_helmholtz_solve_bc(None, f.data_ptr(), g.data_ptr(), u.data_ptr(), None) == 4
    assert L.cheb_helmholtz_solve_bc(h._h, u.data_ptr(), g.data_ptr(), u.data_ptr(), None) == 4       # u aliases f
    assert L.cheb_helmholtz_solve_bc(h._h, f.data_ptr(), u.data_ptr(), u.data_ptr(), None) == 4       # u aliases g
    assert L.cheb_helmholtz_full_size(None) == -1 and L.cheb_helmholtz_boundary_size(None) == -1 and L.cheb_helmholtz_singular(None) == -1
    for bad in ((f[:-1], g, u), (f, g[:-1], u), (f, g, u[:-1]), (f.float(), g, u), (f.cpu(), g, u)):
        with pytest.raises(ValueError):
            h.solve_full(*bad)
    h.destroy()
    h0 = sp.HelmholtzSolver((8, 7))
    with pytest.raises(ValueError):
        h0.solve_full(f, None, u)
    assert L.cheb_helmholtz_solve_bc(h0._h, f.data_ptr(), None, u.data_ptr(), None) == 4                # not a bc handle
    assert L.cheb_helmholtz_full_size(h0._h) == 56 and L.cheb_helmholtz_boundary_size(h0._h) == 56 - 30
    h0.destroy()
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver((8, 7), bc=["neumann", (-1.0, 1.0)])
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver((8, 7), sigma=-1.0, bc=["neumann", "neumann"])
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver((8, 259), bc=["neumann", "neumann"])
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver((8, 7), nfields=17, bc=["neumann", "neumann"])
    with pytest.raises(ValueError):
        sp.HelmholtzSolver((8, 7), bc=["neumann"])
    hp = C.c_void_p()
    assert L.cheb_helmholtz_create_bc(11, (C.c_int * 11)(*[4] * 11), (C.c_double * 44)(*[0.0, 1.0] * 22), 0.0, 1, C.byref(hp)) == 3
    assert hp.value is None
