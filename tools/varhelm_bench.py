#!/usr/bin/env python3
"""VarHelmholtz timed next to its yardsticks, in one session: device events, 5 warm-up calls, REPS timed ones.
Per case (64^3, 128^3, 256^3 with Dirichlet walls, and one periodic-wall-periodic channel; 1 and 3 stacked fields), kappa = 1 + 0.9
prod_k sin(2 x_k + 0.3 k) (contrast 19), c = 0:
  mult          VarHelmholtz.mult                                   precond      VarHelmholtz.precond
  solve         one VarHelmholtz.solve to rtol 1e-8 (restart 30) of a N(0,1) right-hand side, with its iteration count
  elliptic      EllipticOp.mult in a state whose eta array is kappa (one field, walls only): the operator's yardstick
  solve_full    HelmholtzSolver.solve_full of the same handle arguments
and the solve's yardstick (iterations + 1) x (mult + solve_full).  Every timing carries chebhip_launch_count per call, which counts the
sweep, fused and pointwise launches but NOT the launches of the full-grid extension (k_bc_extend_col / _row, one per wall direction):
between walls mult runs 7 launches where the column says 4, and solve_full 3 more than its column.
Then the iteration counts of the solve for the contrasts 2, 19 and 199 with the built preconditioner H(mean(c / kappa))^-1 (r / kappa) and
with the alternative H(mean(c) / mean(kappa))^-1 r / mean(kappa), the latter through Fgmres with a Python preconditioner (its count does
not depend on how it is called).  Prints one JSON line per case.
The per-kernel split comes from a kernel-trace run of its own with fewer calls and one size:
  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/varhelm_bench.py 5 128 trace
usage: varhelm_bench.py [timed calls] [largest cube, default 256] [trace: that cube with one field only, no iteration table]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
NMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
TRACE = len(sys.argv) > 3 and sys.argv[3] == "trace"
WARM = 5


def dev_us(fn, reps=REPS, warm=WARM):
    L = sp.lib()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    c0 = L.chebhip_launch_count()
    fn()
    launches = L.chebhip_launch_count() - c0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 1), launches


def coords(dims, periodic):
    xs = [(-1.0 + 2.0 * np.arange(n) / n) if p else np.cos(np.pi * np.arange(n) / (n - 1)) for n, p in zip(dims, periodic)]
    return np.meshgrid(*xs, indexing="ij")


def kappa(dims, periodic, amp):
    k = np.ones(dims)
    for j, x in enumerate(coords(dims, periodic)):
        k = k * np.sin(2.0 * x + 0.3 * j)
    return 1.0 + amp * k


def case(dims, bc, nf):
    d = len(dims)
    per = sp.bc_split(bc, d)[0]
    op = sp.VarHelmholtz(dims, nf, bc=bc)
    kap = torch.from_numpy(kappa(dims, per, 0.9)).cuda().reshape(-1)
    op.set_coefficients(kap, 0.0)
    rng = np.random.default_rng(dims[0] + nf)
    x = torch.from_numpy(rng.standard_normal(op.size)).cuda()
    f = torch.from_numpy(rng.standard_normal(op.size)).cuda()
    y, u = torch.empty_like(x), torch.empty(op.full_size, dtype=torch.float64, device="cuda")
    row = {"dims": "x".join(map(str, dims)), "bc": "/".join(b if isinstance(b, str) else "mixed" for b in bc), "nfields": nf}
    row["mult_us"], row["mult_launches"] = dev_us(lambda: op.mult(x, y))
    row["precond_us"], row["precond_launches"] = dev_us(lambda: op.precond(x, y))
    op.solve(f, u_full=u, rtol=1e-8)                                   # warm-up: allocates the Krylov bases
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); op.solve(f, u_full=u, rtol=1e-8); e1.record(); torch.cuda.synchronize()
    row.update(solve_us=round(e0.elapsed_time(e1) * 1e3, 1), solve_iterations=op.iterations, solve_reason=op.reason, work_MB=round(op.work_bytes() / 2 ** 20, 1))
    hs = sp.HelmholtzSolver(dims, 0.0 if not all(per) else 1.0, nfields=nf, bc=bc)
    row["solve_full_us"], row["solve_full_launches"] = dev_us(lambda: hs.solve_full(f, None, u))
    hs.destroy()
    row["solve_yardstick_us"] = round((op.iterations + 1) * (row["mult_us"] + row["solve_full_us"]), 1)
    row["solve_over_yardstick"] = round(row["solve_us"] / row["solve_yardstick_us"], 3)
    if nf == 1 and not any(per):
        ell = sp.EllipticOp(dims)
        N = int(np.prod(dims))
        ell.set_state(0, kap.cpu().numpy()); ell.set_state(1, np.zeros(N))
        for k in range(d):
            ell.set_state(2 + k, np.zeros(N))
        row["elliptic_us"], row["elliptic_launches"] = dev_us(lambda: ell.mult(x, y))
        row["mult_over_elliptic"] = round(row["mult_us"] / row["elliptic_us"], 3)
        ell.destroy()
    op.destroy()
    print(json.dumps(row), flush=True)


def iterations(dims, bc, cval):
    d = len(dims)
    per = sp.bc_split(bc, d)[0]
    op = sp.VarHelmholtz(dims, 1, bc=bc)
    f = torch.from_numpy(np.random.default_rng(7).standard_normal(op.size)).cuda()
    row = {"dims": "x".join(map(str, dims)), "bc": "/".join(b if isinstance(b, str) else "mixed" for b in bc), "c": cval}
    inner = tuple(slice(None) if p else slice(1, -1) for p in per)
    for contrast, amp in ((2, 1.0 / 3.0), (19, 0.9), (199, 0.99)):
        kh = kappa(dims, per, amp)
        op.set_coefficients(torch.from_numpy(kh).cuda().reshape(-1), cval)
        xs = op.solve(f, rtol=1e-8)
        row["built_%d" % contrast] = op.iterations if op.reason == 2 else -op.iterations
        km = float(kh[inner].mean())
        hs = sp.HelmholtzSolver(dims, cval / km, bc=bc)
        ks = sp.Fgmres(op.size, restart=30, rtol=1e-8, atol=0.0, max_it=200)
        t = torch.empty_like(f)

        def M(r, z):
            torch.div(r, km, out=t)
            hs.solve(t, z)
        xa = torch.empty_like(f)
        ks.solve(op, f, xa, M=M)
        row["mean_kappa_%d" % contrast] = ks.iterations if ks.reason == 2 else -ks.iterations
        row["solutions_differ_%d" % contrast] = float((xa - xs).abs().max() / xs.abs().max())
        ks.destroy(); hs.destroy()
    op.destroy()
    print(json.dumps(row), flush=True)


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "timed_calls": REPS, "warm_up": WARM}), flush=True)
    walls = ["dirichlet"] * 3
    channel = ["periodic", "dirichlet", "periodic"]
    if TRACE:
        case((NMAX,) * 3, walls, 1)
        return
    for n in (64, 128, 256):
        if n > NMAX:
            continue
        for nf in (1, 3):
            case((n,) * 3, walls, nf)
    for nf in (1, 3):
        case((128, 130, 128), channel, nf)
    # iteration counts (negative: not converged within 200): walls and the channel, c = 0 and c = 1; mixed faces at 64^3
    for dims, bc in (((64,) * 3, walls), ((128,) * 3, walls), ((128, 130, 128), channel),
                     ((64,) * 3, ["dirichlet", "neumann", ("dirichlet", "neumann")])):
        for cval in (0.0, 1.0):
            iterations(dims, bc, cval)


if __name__ == "__main__":
    main()
