#!/usr/bin/env python3
"""Grid sequencing against the direct solve, in one process, alternating (direct, sequenced, direct, sequenced); the SECOND run of
each is reported, as bench.py's `solves` does (the first also pays a fresh process's one-off costs).  One Fgmres / preconditioner per
level, kept across the runs (the caller's KSP / PC objects).
  * config 5: power-law Stokes -exact 2 -rheology 1 -exponent 3 -eps 1e-4 -cont 4 at 128^3 (bench.py's settings), sequenced with
    stages 0-3 at 64^3 and stage 4 at 128^3;
  * elliptic 256^3, gamma 4, bench.py's manufactured problem, sequenced 64^3 -> 128^3 -> 256^3, every level to the direct solve's
    absolute target (snes_atol = 1e-10 |F(0)| of the 256^3 problem; snes_rtol 1e-10 as bench.py).
Prints one JSON line per problem: seconds, Newton and FGMRES iterations per level, the final |F| on the fine grid, and
|x_seq - x_direct| / |x_direct| (for Stokes also with the pressure means removed: the pressure is defined up to a constant)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from importlib import import_module
import __graft_entry__ as ge


def exact2(P):
    """StokesExact2 (stokes.C:1963-2012) on P^3 CGL points: state, force, Dirichlet values (as bench.py)."""
    c = np.cos(np.pi * np.arange(P) / (P - 1))
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    u = np.sin(0.5 * np.pi * X) * np.cos(0.5 * np.pi * Y); v = -np.cos(0.5 * np.pi * X) * np.sin(0.5 * np.pi * Y)
    val = np.stack([u, v, np.zeros_like(u), np.zeros_like(u)], axis=-1).reshape(-1, 4)
    idx = np.arange(P)
    bd1 = (idx == 0) | (idx == P - 1)
    bd = (bd1[:, None, None] | bd1[None, :, None] | bd1[None, None, :]).ravel()
    U = val[~bd]
    rhs = U.copy(); rhs[:, :2] *= (0.5 * np.pi) ** 2; rhs[:, 2:] = 0.0
    return U.ravel(), rhs.ravel(), np.ascontiguousarray(val[bd][:, :3]).ravel()


def smooth(P, d, seed):
    """bench.py's manufactured elliptic field (zero on the boundary), at the interior nodes of P^d."""
    x = np.cos(np.pi * np.arange(1, P - 1) / (P - 1))
    rng = np.random.default_rng(seed)
    f = np.ones((P - 2,) * d)
    for k in range(d):
        a, b = rng.random(2) + 0.5
        g = (1.0 - x * x) * (1.0 + 0.3 * np.cos(2.0 * a * x + b))
        f = f * g.reshape([-1 if j == k else 1 for j in range(d)])
    return f


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def stokes(sp, solve, Ps=(64, 128)):
    rheo, cont = (1, 1.0, 3.0, 1e-4, 1.0), 4
    kw = dict(rheology=rheo, cont0=0, cont=cont, snes_rtol=1e-8, ksp_rtol=1e-5, ksp_restart=60, ksp_max_it=200, max_linear_fail=3, snes_max_it=20)
    levels, kss, pcs = [], [], []
    for P in Ps:
        st = sp.StokesOp((P, P, P))
        U, U2, dv = exact2(P)
        st.set_dirichlet(dv); st.set_force(U2)
        levels.append((st, dv))
        kss.append(sp.Fgmres(st.global_size, restart=60, rtol=1e-5, max_it=200)); pcs.append(sp.StokesSaddlePc(st, 0))
    fine = levels[-1][0]
    xd = torch.zeros(fine.global_size, dtype=torch.float64, device="cuda"); xs = torch.zeros_like(xd)
    rec = {"problem": "config 5: Stokes -exact 2 power law (1, 1, 3, 1e-4, 1) cont %d at %d^3" % (cont, Ps[-1]),
           "sequenced_levels": ["%d^3" % P for P in Ps], "stage_level": solve.default_stage_level(cont + 1, len(Ps))}
    for rep in range(2):
        xd.zero_()
        td, logd = timed(lambda: solve.stokes_solve(sp, fine, xd, ks=kss[-1], pc=pcs[-1], **kw))
        ts, logs = timed(lambda: solve.stokes_solve_sequenced(sp, levels, None, x=xs, ks=kss, pc=pcs, **kw))
        rec.setdefault("seconds_first_run", {"direct": td, "sequenced": ts})
    rec["seconds"] = {"direct": td, "sequenced": ts}
    rec["speedup_direct_over_sequenced"] = td / ts
    rec["direct"] = {"newton_its": sum(r[2] for r in logd), "krylov_its": sum(r[3] for r in logd), "final_F": logd[-1][4],
                     "stages": [list(r) for r in logd]}
    rec["sequenced"] = {"per_level": {"%d^3" % Ps[l]: {"newton_its": sum(r[2] for r in logs if r[5] == l), "krylov_its": sum(r[3] for r in logs if r[5] == l)}
                                      for l in range(len(Ps))}, "final_F": logs[-1][4], "stages": [list(r) for r in logs]}
    F = torch.empty_like(xd)
    fine.set_rheology(*rheo); fine.function(xd, F); fd = float(F.norm())
    fine.function(xs, F); fs = float(F.norm())
    rec["fine_F_recomputed"] = {"direct": fd, "sequenced": fs}
    rec["rel_diff_seq_vs_direct"] = float((xs - xd).norm() / xd.norm())
    mf = lambda x: (lambda v: torch.cat([v[:, :3], (v[:, 3] - v[:, 3].mean())[:, None]], 1))(x.view(-1, 4))
    rec["rel_diff_seq_vs_direct_pressure_mean_removed"] = float((mf(xs) - mf(xd)).norm() / mf(xd).norm())
    for k in kss: k.destroy()
    for p in pcs: p.destroy()
    for st, _ in levels: st.destroy()
    return rec


def elliptic(sp, solve, Ps=(64, 128, 256)):
    kw = dict(snes_rtol=1e-10, ksp_rtol=1e-6, ksp_restart=30, ksp_max_it=300)
    levels, kss = [], []
    for P in Ps:
        op = sp.EllipticOp((P, P, P))
        dv = np.zeros(op.dirichlet_size); op.set_dirichlet(dv)
        us = torch.from_numpy(smooth(P, 3, 1).ravel()).cuda()
        b = torch.empty_like(us)
        op.function(us, None, b, 4.0, 2.0)
        levels.append([op, b, dv, None])
        kss.append(sp.Fgmres(op.global_size, restart=30, rtol=1e-6, max_it=300))
    op, b = levels[-1][0], levels[-1][1]
    F = torch.empty_like(b)
    op.function(torch.zeros_like(b), b, F, 4.0, 2.0)
    atol = 1e-10 * float(F.norm())
    xd = torch.zeros_like(b); xs = torch.zeros_like(b)
    rec = {"problem": "elliptic %d^3 gamma 4 (bench.py's manufactured problem)" % Ps[-1], "sequenced_levels": ["%d^3" % P for P in Ps],
           "snes_atol": atol}
    for rep in range(2):
        xd.zero_()
        pc = sp.FdPc(op, sweeps=0)
        td, (its, kits, fn) = timed(lambda: solve.newton_krylov(sp, op, b, xd, 4.0, 2.0, M=pc, monitor=lambda i, f, k: pc.update(), ks=kss[-1], **kw))
        pc.destroy()
        pcs = [sp.FdPc(l[0], sweeps=0) for l in levels]
        for l, p in zip(levels, pcs):
            l[3] = p
        ts, logs = timed(lambda: solve.newton_krylov_sequenced(sp, [tuple(l) for l in levels], 4.0, 2.0, x=xs, ks=kss, snes_atol=atol,
                                                               monitor=lambda lev, i, f, k: pcs[lev].update(), **kw))
        for p in pcs: p.destroy()
        rec.setdefault("seconds_first_run", {"direct": td, "sequenced": ts})
    rec["seconds"] = {"direct": td, "sequenced": ts}
    rec["speedup_direct_over_sequenced"] = td / ts
    rec["direct"] = {"newton_its": its, "krylov_its": kits, "final_F": fn}
    rec["sequenced"] = {"per_level": {"%d^3" % P: {"newton_its": r[0], "krylov_its": r[1], "final_F": r[2]} for P, r in zip(Ps, logs)},
                        "final_F": logs[-1][2]}
    rec["rel_diff_seq_vs_direct"] = float((xs - xd).norm() / xd.norm())
    for k in kss: k.destroy()
    for l in levels: l[0].destroy()
    return rec


def main():
    sp = ge.load()
    assert torch.cuda.is_available(), "sequence_bench needs a GPU"
    solve = import_module(sp.__name__ + ".solve")
    what = sys.argv[1:] or ["stokes", "elliptic"]
    for w in what:
        print(json.dumps({"stokes": stokes, "elliptic": elliptic}[w](sp, solve)), flush=True)


if __name__ == "__main__":
    main()
