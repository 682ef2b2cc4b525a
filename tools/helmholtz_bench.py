#!/usr/bin/env python3
"""Direct Poisson / Helmholtz solves by fast diagonalisation against the Krylov routes.
  1. cheb_helmholtz_solve at 128^3 and 256^3 beside FdPc(sweeps = 0).apply (the same launches with other matrices), device
     events, warm-up first;
  2. 256^3 gamma = 0: the linear solve on a random right-hand side, HelmholtzSolver against FGMRES(30) + FdPc to 1e-8 (the
     DESIGN 5.1 configuration), and poisson_solve against newton_krylov + FdPc on README:21's problem (-exact 2, inhomogeneous
     Dirichlet values), with the error against the analytic solution;
  3. 256^3 gamma = 4 (bench.py's manufactured problem, as tools/sequence_bench.py): Newton with SpectralPc against FdPc.
Prints one JSON line per part.  usage: helmholtz_bench.py [reps]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from importlib import import_module
import __graft_entry__ as ge
import oracle_lib as orc
sp = ge.load(); solve = import_module(sp.__name__ + ".solve")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def dev_us(fn, reps=REPS, warm=3):
    """Mean device time per call in microseconds (events around `reps` back-to-back calls), best of three rounds."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        best = us if best is None else min(best, us)
    return best


def wall_s(fn, reps=3):
    """Best wall time of `reps` runs (host synchronised around each), after one warm-up run."""
    fn(); torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


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


def part1():
    for P in (128, 256):
        dims = (P, P, P)
        op = sp.EllipticOp(dims)
        h = sp.HelmholtzSolver(dims)
        pc = sp.FdPc(op, sweeps=0); pc.update()
        r = torch.randn(op.global_size, dtype=torch.float64, device="cuda"); z = torch.empty_like(r)
        t_h = dev_us(lambda: h.solve(r, z))
        t_fd = dev_us(lambda: pc.apply(r, z))
        t_mv = dev_us(lambda: op.mult(r, z))
        print(json.dumps({"part": "solve vs FdPc(sweeps=0).apply", "dims": "%d^3" % P, "helmholtz_solve_us": round(t_h, 1),
                          "fdpc_apply_us": round(t_fd, 1), "ratio": round(t_h / t_fd, 3), "poisson_matvec_us": round(t_mv, 1)}), flush=True)
        pc.destroy(); h.destroy(); op.destroy()
        del r, z


def part2():
    P = 256
    dims = (P, P, P)
    op = sp.EllipticOp(dims); n = op.global_size
    # (a) random right-hand side, zero Dirichlet values: the DESIGN 5.1 solve
    b = torch.randn(n, dtype=torch.float64, device="cuda"); x = torch.empty_like(b)
    pc = sp.FdPc(op, sweeps=0); pc.update()
    ks = sp.Fgmres(n, restart=30, rtol=1e-8, max_it=200)
    t_k, _ = wall_s(lambda: ks.solve(op, b, x, M=pc))
    its = ks.iterations
    xk = x.clone()
    h = sp.HelmholtzSolver(dims)
    t_h, _ = wall_s(lambda: h.solve(b, x), reps=10)
    r = torch.empty_like(b); op.mult(x, r)
    res = float((r - b).norm() / b.norm())
    print(json.dumps({"part": "256^3 linear solve, random b", "fgmres_fdpc_1e-8_ms": round(t_k * 1e3, 2), "fgmres_its": its,
                      "helmholtz_ms": round(t_h * 1e3, 3), "speedup": round(t_k / t_h, 1), "helmholtz_rel_residual": res,
                      "rel_diff_vs_fgmres": float((x - xk).norm() / xk.norm())}), flush=True)
    ks.destroy(); del xk, r
    # (b) README:21's problem: -exact 2, inhomogeneous Dirichlet values, gamma = 0
    u, u2, dv = orc.elliptic_exact(dims, 2)
    op.set_dirichlet(dv)
    b = torch.from_numpy(u2).cuda(); ud = torch.from_numpy(u).cuda()
    t_p, _ = wall_s(lambda: solve.poisson_solve(sp, op, b, x, solver=h), reps=5)
    err_p = float((x - ud).norm() / ud.norm())
    kw = dict(snes_rtol=1e-10, ksp_rtol=1e-6, ksp_restart=30, ksp_max_it=300)
    xn = torch.zeros_like(b)
    def newton():
        xn.zero_()
        return solve.newton_krylov(sp, op, b, xn, 0.0, 2.0, M=pc, monitor=lambda i, f, k: pc.update(), **kw)
    t_n, (nits, kits, fn) = wall_s(newton)
    err_n = float((xn - ud).norm() / ud.norm())
    print(json.dumps({"part": "256^3 gamma 0 -exact 2 (inhomogeneous Dirichlet)", "poisson_solve_ms": round(t_p * 1e3, 3),
                      "newton_krylov_fdpc_ms": round(t_n * 1e3, 2), "newton_its": nits, "fgmres_its": kits, "speedup": round(t_n / t_p, 1),
                      "poisson_solve_err_vs_analytic": err_p, "newton_err_vs_analytic": err_n,
                      "rel_diff": float((x - xn).norm() / xn.norm())}), flush=True)
    pc.destroy(); h.destroy(); op.destroy()


def part3():
    P = 256
    dims = (P, P, P)
    op = sp.EllipticOp(dims)
    dv = np.zeros(op.dirichlet_size); op.set_dirichlet(dv)
    us = torch.from_numpy(smooth(P, 3, 1).ravel()).cuda()
    b = torch.empty_like(us)
    op.function(us, None, b, 4.0, 2.0)
    kw = dict(snes_rtol=1e-10, ksp_rtol=1e-6, ksp_restart=30, ksp_max_it=300)
    out = {"part": "256^3 gamma 4 Newton (bench.py's manufactured problem)", "settings": kw}
    xs = {}
    for name, mk in (("FdPc", lambda: sp.FdPc(op, sweeps=0)), ("SpectralPc", lambda: sp.SpectralPc(op))):
        pc = mk()
        x = torch.zeros_like(b)
        def run():
            x.zero_()
            return solve.newton_krylov(sp, op, b, x, 4.0, 2.0, M=pc, monitor=lambda i, f, k: pc.update(), **kw)
        t, (its, kits, fn) = wall_s(run, reps=2)
        xs[name] = x
        out[name] = {"seconds": round(t, 4), "newton_its": its, "fgmres_its": kits, "final_F": fn,
                     "err_vs_manufactured": float((x - us).norm() / us.norm())}
        pc.destroy()
    out["rel_diff"] = float((xs["SpectralPc"] - xs["FdPc"]).norm() / xs["FdPc"].norm())
    out["speedup_spectral_over_fd"] = round(out["FdPc"]["seconds"] / out["SpectralPc"]["seconds"], 2)
    print(json.dumps(out), flush=True)
    op.destroy()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS}), flush=True)
    part1()
    part2()
    part3()
