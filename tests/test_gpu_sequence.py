"""Grid-sequenced Newton solves (solve.newton_krylov_sequenced / stokes_solve_sequenced): a coarse solve prolonged by
cheb_resample_* is the fine Newton starting point.  The fine result must be the direct fine solve's, reached in fewer Newton steps."""
import numpy as np
import pytest
import torch
from importlib import import_module

import __graft_entry__ as ge
import oracle_lib as orc

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
GAMMA, EXPO, COS = 4.0, 2.0, 3.0


def elliptic_level(dims):
    """tests.sh's problem: -exact 0 -cos_scale 3 -gamma 4 (inhomogeneous Dirichlet values)."""
    op = sp.EllipticOp(dims)
    u, u2, dv = orc.elliptic_exact(dims, 0, gamma=GAMMA, exponent=EXPO, cos_scale=COS)
    op.set_dirichlet(dv)
    return op, torch.from_numpy(u2).cuda(), dv


@pytest.mark.parametrize("coarse,fine", [((12, 12), (24, 24)), ((16, 16, 16), (32, 32, 32))], ids=["12x12-24x24", "16^3-32^3"])
def test_elliptic_sequenced_equals_direct(coarse, fine):
    kw = dict(ksp_rtol=1e-12, ksp_restart=30, ksp_max_it=20000)
    op, b, dv = elliptic_level(fine)
    pc = sp.FdPc(op, sweeps=0)
    xd = torch.zeros_like(b)
    its_d, _, fn_d = solve.newton_krylov(sp, op, b, xd, GAMMA, EXPO, snes_rtol=1e-10, M=pc, monitor=lambda i, f, k: pc.update(), **kw)
    pc.destroy()
    # the same absolute target on the fine level, |F| <= 1e-10 |b| (a relative one would ask more of the better start); |F|
    # weights the error of the start by ~n^4, so 12 -> 24 saves one Newton step, 16^3 -> 32^3 three
    f0 = float(b.norm())
    opc, bc, dvc = elliptic_level(coarse)
    pcs = [sp.FdPc(opc, sweeps=0), sp.FdPc(op, sweeps=0)]
    xs = torch.zeros_like(b)
    log = solve.newton_krylov_sequenced(sp, [(opc, bc, dvc, pcs[0]), (op, b, dv, pcs[1])], GAMMA, EXPO, x=xs, snes_rtol=1e-10,
                                        snes_atol=1e-10 * f0, monitor=lambda lev, i, f, k: pcs[lev].update(), **kw)
    torch.cuda.synchronize()
    assert len(log) == 2
    F = torch.empty_like(b)
    op.function(xs, b, F, GAMMA, EXPO)
    assert float(F.norm()) <= max(1e-10 * f0, fn_d)
    assert float((xs - xd).norm()) <= 1e-10 * float(xd.norm())
    assert log[1][0] < its_d, (log, its_d)
    for p in pcs:
        p.destroy()
    op.destroy(); opc.destroy()


def stokes_level(dims):
    st = sp.StokesOp(dims)
    U, U2, dv = orc.stokes_exact(dims, 2)
    st.set_dirichlet(dv); st.set_force(U2)
    return st, dv, U2


def _mean_free(x, d):
    """Velocity and the pressure with its mean removed (the pressure of an all-Dirichlet velocity problem is defined up to a constant)."""
    v = x.view(-1, d + 1).clone()
    v[:, d] -= v[:, d].mean()
    return v.view(-1)


def test_stokes_linear_sequenced_equals_direct():
    """-exact 2 is resolved to rounding on these grids, so the field U is the discrete solution: the sequenced solve must reach it to
    1e-10.  The direct solve from zero agrees to what its own tolerances leave (one Newton step at ksp_rtol 1e-12 of a residual
    ~10^4 times the sequenced start's: ~3e-9 measured), checked at 1e-8."""
    coarse, fine = (12, 12, 12), (24, 24, 24)
    st, dv, _ = stokes_level(fine)
    U = torch.from_numpy(orc.stokes_exact(fine, 2)[0]).cuda()
    xd = torch.zeros(st.global_size, dtype=torch.float64, device="cuda")
    F = torch.empty_like(xd)
    st.function(xd, F)
    # one absolute target for every solve: 1e-12 of the direct solve's initial residual (the sequenced start's is far smaller)
    kw = dict(snes_rtol=1e-12, snes_atol=1e-12 * float(F.norm()), ksp_rtol=1e-12, ksp_restart=60, ksp_max_it=400, max_linear_fail=3, snes_max_it=20)
    solve.stokes_solve(sp, st, xd, **kw)
    stc, dvc, _ = stokes_level(coarse)
    xs = torch.zeros_like(xd)
    log = solve.stokes_solve_sequenced(sp, [(stc, dvc), (st, dv)], x=xs, **kw)
    torch.cuda.synchronize()
    assert [row[5] for row in log] == [0, 1]                    # one stage: solved on both levels, coarsest first
    a, b, u = _mean_free(xs, 3), _mean_free(xd, 3), _mean_free(U, 3)
    assert float((a - u).norm()) <= 1e-10 * float(u.norm())
    assert float((a - b).norm()) <= 1e-8 * float(b.norm())
    st.destroy(); stc.destroy()


def test_stokes_power_law_sequenced_is_a_root_of_the_oracle_residual():
    """-exact 2 -rheology 1 -exponent 3 -eps 1e-2 -cont 2: stages 0-1 at 16^3, stage 2 at 32^3.  The final state is a root of the
    oracle's StokesFunction at 32^3 (as test_gpu_saddle.py's direct continuation), in fewer Newton steps at 32^3 than the direct solve."""
    coarse, fine = (16, 16, 16), (32, 32, 32)
    rheo = (1, 1.0, 3.0, 1e-2, 1.0)
    st, dv, U2 = stokes_level(fine)
    kw = dict(rheology=rheo, cont0=0, cont=2, snes_rtol=1e-8, snes_atol=1e-10 * np.linalg.norm(U2), ksp_rtol=1e-5, ksp_restart=60,
              ksp_max_it=200)
    xd = torch.zeros(st.global_size, dtype=torch.float64, device="cuda")
    direct = solve.stokes_solve(sp, st, xd, **kw)
    stc, dvc, _ = stokes_level(coarse)
    xs = torch.zeros_like(xd)
    log = solve.stokes_solve_sequenced(sp, [(stc, dvc), (st, dv)], [0, 0, 1], x=xs, **kw)
    torch.cuda.synchronize()
    assert [row[5] for row in log] == [0, 0, 1]
    assert [round(row[0], 4) for row in log] == [round(row[0], 4) for row in direct]
    F = orc.stokes_function(fine, xs.cpu().numpy(), dv, U2, rheology=rheo, mode=orc.FAST, nthreads=16)[0]
    assert np.linalg.norm(F) <= 1e-7 * np.linalg.norm(U2)
    assert sum(row[2] for row in log if row[5] == 1) < sum(row[2] for row in direct), (log, direct)
    st.destroy(); stc.destroy()


def test_sequenced_drivers_reject_bad_arguments():
    st, dv, _ = stokes_level((8, 8, 8))
    x = torch.zeros(st.global_size, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        solve.stokes_solve_sequenced(sp, [(st, dv)], [0, 1], rheology=(1, 1.0, 3.0, 1e-2, 1.0), cont=1, x=x)      # level out of range
    with pytest.raises(ValueError):
        solve.stokes_solve_sequenced(sp, [(st, dv)], x=x, dist=object())
    with pytest.raises(ValueError):
        solve.newton_krylov_sequenced(sp, [], x=x, dist=object())
    st.destroy()
