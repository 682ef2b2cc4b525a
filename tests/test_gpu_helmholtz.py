"""Direct Chebyshev Poisson / Helmholtz solves by fast diagonalisation (cheb_helmholtz_*, ell_pc_create_spectral,
solve.poisson_solve): the exact inverse of MatMult_Elliptic at eta == 1 (shifted by sigma), batches and in-place solves, the
inhomogeneous Dirichlet problem of README:21 against its polynomial solution and against Newton-Krylov, and the spectral
preconditioner inside linear and nonlinear Newton solves."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import oracle_lib as orc

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")

SHAPES = [(9,), (12, 10), (8, 7, 6), (66, 12, 5), (130, 70), (131, 70), (258, 20), (70, 68, 40), (12,) * 5, (128, 128, 128)]
ids = lambda d: "x".join(map(str, d))


def interior_field(dims, kind, seed=0):
    """White noise, or a smooth (entire, non-polynomial) function sampled at the interior Gauss-Lobatto nodes, row-major."""
    if kind == "noise":
        G = int(np.prod([n - 2 for n in dims]))
        return np.random.default_rng(seed).standard_normal(G)
    grids = [np.cos(np.pi * np.arange(1, n - 1) / (n - 1)) for n in dims]
    X = np.meshgrid(*grids, indexing="ij")
    u = np.ones(X[0].shape)
    for k, x in enumerate(X):
        u = u * np.cos(0.7 * x + 0.3 * k) * np.exp(0.2 * x)
    return u.ravel()


def relerr(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_round_trip(dims, kind):
    op = sp.EllipticOp(dims)
    h = sp.HelmholtzSolver(dims)
    assert h.size == op.global_size
    u = torch.from_numpy(interior_field(dims, kind)).cuda()
    f = torch.empty_like(u)
    op.mult(u, f)
    x = torch.empty_like(u)
    h.solve(f, x)
    torch.cuda.synchronize()
    err = relerr(x, u)
    assert err <= 1e-10, err
    h.destroy(); op.destroy()


@pytest.mark.parametrize("sigma", [1.5, 1e3])
@pytest.mark.parametrize("dims", [(9,), (130, 70), (70, 68, 40), (12,) * 5, (66, 12, 5)], ids=ids)
def test_shifted_residual(dims, sigma):
    op = sp.EllipticOp(dims)
    h = sp.HelmholtzSolver(dims, sigma=sigma)
    f = torch.from_numpy(interior_field(dims, "noise", seed=3)).cuda()
    x = torch.empty_like(f)
    h.solve(f, x)
    r = torch.empty_like(f)
    op.mult(x, r)
    r.add_(x, alpha=sigma)
    torch.cuda.synchronize()
    err = relerr(r, f)
    assert err <= 1e-10, err
    h.destroy(); op.destroy()


@pytest.mark.parametrize("dims", [(9,), (12, 10), (130, 70), (70, 68, 40), (12,) * 5, (128, 128, 128)], ids=ids)
def test_batch_and_in_place(dims):
    G = int(np.prod([n - 2 for n in dims]))
    one = sp.HelmholtzSolver(dims, sigma=0.25)
    three = sp.HelmholtzSolver(dims, sigma=0.25, nfields=3)
    assert three.size == 3 * G
    f = torch.from_numpy(np.concatenate([interior_field(dims, "noise", seed=s) for s in range(3)])).cuda()
    ref = torch.empty_like(f)
    for i in range(3):
        one.solve(f[i * G:(i + 1) * G], ref[i * G:(i + 1) * G])
    u = torch.empty_like(f)
    three.solve(f, u)
    torch.cuda.synchronize()
    err = relerr(u, ref)
    assert err <= 1e-14, err
    print("%s: nfields = 3 vs three solves: %s" % (ids(dims), "same bits" if torch.equal(u, ref) else "rel.err %.1e" % err))
    g = f.clone()
    three.solve(g, g)                                                       # u == f
    torch.cuda.synchronize()
    assert torch.equal(g, u)
    one.destroy(); three.destroy()


def newton_fdpc(op, b, gamma, exponent):
    pc = sp.FdPc(op, sweeps=0)
    x = torch.zeros_like(b)
    its, kits, fn = solve.newton_krylov(sp, op, b, x, gamma, exponent, snes_rtol=1e-12, ksp_rtol=1e-12, ksp_restart=30,
                                        ksp_max_it=20000, M=pc, monitor=lambda i, f, k: pc.update())
    pc.destroy()
    return x, its, kits


@pytest.mark.parametrize("dims", [(12,) * 5, (32, 32, 32)], ids=ids)
def test_poisson_inhomogeneous_dirichlet(dims):
    """README:21's problem (-exact 2 at gamma = 0): u = prod_j x_j^(4+j) is a polynomial the grid resolves exactly."""
    u, u2, dv = orc.elliptic_exact(dims, 2)
    op = sp.EllipticOp(dims)
    op.set_dirichlet(dv)
    b = torch.from_numpy(u2).cuda()
    x = torch.empty_like(b)
    solve.poisson_solve(sp, op, b, x)
    torch.cuda.synchronize()
    ud = torch.from_numpy(u).cuda()
    err = relerr(x, ud)
    assert err <= 1e-10, err
    xn, its, kits = newton_fdpc(op, b, 0.0, 2.0)
    torch.cuda.synchronize()
    assert relerr(x, xn) <= 1e-10, (relerr(x, xn), its, kits)
    # a caller's solver, kept across calls: the same bits
    h = sp.HelmholtzSolver(dims)
    x2 = torch.empty_like(b)
    solve.poisson_solve(sp, op, b, x2, solver=h)
    torch.cuda.synchronize()
    assert torch.equal(x2, x)
    with pytest.raises(ValueError):
        solve.poisson_solve(sp, op, b, x2, sigma=1.0, solver=h)
    h.destroy(); op.destroy()


def test_poisson_zero_dirichlet_128():
    """-exact 1: u = prod_j (1 - x_j^2), zero Dirichlet values, resolved exactly.  The reference's forcing (elliptic.C:633-643)
    multiplies by 2 (1 - x_k^2) for every OTHER direction k, i.e. it is -Laplace(2^(d-2) u): at d = 3 the solution is 2 u."""
    dims = (128, 128, 128)
    u, u2, dv = orc.elliptic_exact(dims, 1)
    assert np.abs(dv).max() == 0.0
    op = sp.EllipticOp(dims)
    op.set_dirichlet(dv)
    b = torch.from_numpy(u2).cuda()
    x = torch.empty_like(b)
    solve.poisson_solve(sp, op, b, x)
    r = torch.empty_like(b)
    op.mult(x, r)
    torch.cuda.synchronize()
    err = relerr(x, 2.0 ** (len(dims) - 2) * torch.from_numpy(u).cuda())
    assert err <= 1e-10, err
    assert relerr(r, b) <= 1e-10
    op.destroy()


@pytest.mark.parametrize("dims", [(24, 24), (32, 32, 32)], ids=ids)
def test_linear_newton_spectral_pc(dims):
    """At gamma = 0 the spectral preconditioner is the exact inverse of the Jacobian: one Newton step, one or two FGMRES iterations."""
    u, u2, dv = orc.elliptic_exact(dims, 2)
    op = sp.EllipticOp(dims)
    op.set_dirichlet(dv)
    b = torch.from_numpy(u2).cuda()
    pc = sp.SpectralPc(op)
    x = torch.zeros_like(b)
    its, kits, fn = solve.newton_krylov(sp, op, b, x, 0.0, 2.0, M=pc, monitor=lambda i, f, k: pc.update())
    torch.cuda.synchronize()
    assert its == 1 and kits <= 3, (its, kits)
    assert relerr(x, torch.from_numpy(u).cuda()) <= 1e-10
    pc.destroy(); op.destroy()


@pytest.mark.parametrize("dims", [(16, 16, 16), (24, 24)], ids=ids)
def test_nonlinear_newton_spectral_pc(dims):
    """tests.sh's problem (-exact 0 -cos_scale 3 -gamma 4): the spectral preconditioner (after division by eta) against FdPc."""
    g, e = 4.0, 2.0
    u, u2, dv = orc.elliptic_exact(dims, 0, gamma=g, exponent=e, cos_scale=3.0)
    op = sp.EllipticOp(dims)
    op.set_dirichlet(dv)
    b = torch.from_numpy(u2).cuda()
    xf, its_f, kits_f = newton_fdpc(op, b, g, e)
    pc = sp.SpectralPc(op)
    x = torch.zeros_like(b)
    its, kits, fn = solve.newton_krylov(sp, op, b, x, g, e, snes_rtol=1e-12, ksp_rtol=1e-12, ksp_restart=30, ksp_max_it=20000,
                                        M=pc, monitor=lambda i, f, k: pc.update())
    torch.cuda.synchronize()
    print("%s gamma = 4: SpectralPc %d Newton / %d FGMRES iterations, FdPc %d / %d" % (ids(dims), its, kits, its_f, kits_f))
    assert relerr(x, xf) <= 1e-10, relerr(x, xf)
    pc.destroy(); op.destroy()


def test_helmholtz_as_fgmres_preconditioner():
    dims = (40, 30)
    op = sp.EllipticOp(dims)
    h = sp.HelmholtzSolver(dims)
    b = torch.from_numpy(interior_field(dims, "noise", seed=7)).cuda()
    x = torch.zeros_like(b)
    ks = sp.Fgmres(op.global_size, rtol=1e-12)
    ks.solve(op, b, x, M=h)
    torch.cuda.synchronize()
    assert ks.iterations <= 2, ks.iterations
    r = torch.empty_like(b)
    op.mult(x, r)
    assert relerr(r, b) <= 1e-11
    ks.destroy(); h.destroy(); op.destroy()


def test_argument_errors():
    L = sp.lib()
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver((8, 2))
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver((8, 8), sigma=-1.0)
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver((8, 8), nfields=17)
    h = sp.HelmholtzSolver((8, 8))
    t = torch.zeros(h.size, dtype=torch.float64, device="cuda")
    assert L.cheb_helmholtz_solve(h._h, None, t.data_ptr(), None) == 4
    assert L.cheb_helmholtz_solve(h._h, t.data_ptr(), None, None) == 4
    with pytest.raises(AssertionError):
        h.solve(torch.zeros(h.size + 1, dtype=torch.float64, device="cuda"), t)
    h.destroy()
    op = sp.EllipticOp((8, 8))
    with pytest.raises(sp.ChebhipError):
        sp.SpectralPc(op, sigma=float("nan"))
    pc = sp.SpectralPc(op)
    assert L.chebhip_fdpc_set_sweeps(pc._h, 1) == 4
    assert L.chebhip_fdpc_set_sweeps(pc._h, 0) == 0
    assert L.chebhip_fdpc_mult(pc._h, t.data_ptr(), torch.empty_like(t).data_ptr(), None) == 4
    pc.destroy(); op.destroy()
    slab = sp.EllipticOp((8, 8), slab=(0, 4), dim0=lambda *a: 0)
    hp = C.c_void_p()
    assert L.ell_pc_create_spectral(slab._h, 0.0, C.byref(hp)) == 4
    assert hp.value is None
    slab.destroy()
