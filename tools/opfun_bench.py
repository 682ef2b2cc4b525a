#!/usr/bin/env python3
"""ChebOpFun.apply against HelmholtzSolver.solve and against compositions of one-field calls, on the cube at
128^3 and 256^3 with Dirichlet faces, and at 128^3 once more with Neumann faces (the bc lines), device events, 5 warm-up calls and
100 timed ones:
  inv      `inv` 1 -> 1 against HelmholtzSolver.solve of the same handle arguments, with the default options and with
           fdm_passes = 1 (the solver's separate scaling pass: the same launches as ChebOpFun, a lighter pointwise kernel)
  exp      `exp` 1 -> 1
  etd1     u+ = e^(-hB) u + h phi_1(-hB) N as ONE 2 -> 1 call against two 1 -> 1 calls and a torch add
  res3     1 / (p_f + tau_f B) on three fields with three (p, tau) in one call against three one-field solver handles
           (sigma_f = p_f / tau_f, and a torch scaling by 1 / tau_f)
Every line also carries the library's launches per call (chebhip_launch_count).  Prints one JSON line per case.  The per-kernel
split comes from a kernel-trace run of the same script with fewer calls:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/opfun_bench.py 5 opfun 256
usage: opfun_bench.py [timed calls] [opfun|all] [128|256|128n]   (opfun: only the ChebOpFun calls, for the trace; one case only)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 100
WHAT = sys.argv[2] if len(sys.argv) > 2 else "all"
CASE = sys.argv[3] if len(sys.argv) > 3 else None
WARM = 5
H = 1e-3


def dev_us(fn):
    """(mean device time per call in microseconds, library launches per call): events around REPS back-to-back calls."""
    L = sp.lib()
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    c0 = L.chebhip_launch_count()
    fn()
    launches = L.chebhip_launch_count() - c0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record(); torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / REPS, 1), launches


def solver_us(dims, bc, x, y, passes):
    old = sp.get_option("fdm_passes")
    sp.set_option("fdm_passes", passes)             # (read at create and per solve)
    try:
        hs = sp.HelmholtzSolver(dims, 0.0, 1, bc=bc)
        r = dev_us(lambda: hs.solve(x, y))
        hs.destroy()
    finally:
        sp.set_option("fdm_passes", old)
    return r


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "timed_calls": REPS, "warm_up": WARM}), flush=True)
    for n, bc in ((128, None), (256, None), (128, ("neumann",) * 3)):
        if CASE is not None and CASE != "%d%s" % (n, "" if bc is None else "n"):
            continue
        dims = (n,) * 3
        G = (n - 2) ** 3
        x = torch.from_numpy(np.random.default_rng(n).standard_normal(3 * G)).cuda()
        y = torch.empty_like(x)
        row = {"dims": "%d^3" % n, "faces": "dirichlet" if bc is None else "neumann", "MB_per_field": round(G * 8e-6, 1)}
        one = sp.ChebOpFun(dims, 1, 1, 0.0, bc=bc)
        one.set_terms("inv")
        row["inv_us"], row["inv_launches"] = dev_us(lambda: one.apply(x[:G], out=y[:G]))
        if WHAT == "all":
            row["solve_us"], row["solve_launches"] = solver_us(dims, bc, x[:G], y[:G], 0)
            row["solve_passes_us"], row["solve_passes_launches"] = solver_us(dims, bc, x[:G], y[:G], 1)
        one.set_terms("exp", tau=H)
        row["exp_us"], _ = dev_us(lambda: one.apply(x[:G], out=y[:G]))
        etd = sp.ChebOpFun(dims, 2, 1, 0.0, bc=bc)
        etd.set_terms([(0, 0, "exp", 1.0, H, 0.0), (0, 1, "phi1", H, H, 0.0)])
        row["etd1_us"], row["etd1_launches"] = dev_us(lambda: etd.apply(x[:2 * G], out=y[:G]))
        etd.destroy()
        if WHAT == "all":
            t = torch.empty(G, dtype=torch.float64, device="cuda")

            def two_calls():
                one.set_terms("exp", tau=H)
                one.apply(x[:G], out=y[:G])
                one.set_terms([(0, 0, "phi1", H, H, 0.0)])
                one.apply(x[G:2 * G], out=t)
                y[:G].add_(t)
            row["etd1_two_calls_us"], _ = dev_us(two_calls)
        one.destroy()
        pt = [(1.0, 1e-3), (1.5, 4e-3), (2.0, 2.5e-4)]
        res = sp.ChebOpFun(dims, 3, 3, 0.0, bc=bc)
        res.set_terms([(f, f, "res", 1.0, tau, p) for f, (p, tau) in enumerate(pt)])
        row["res3_us"], row["res3_launches"] = dev_us(lambda: res.apply(x, out=y))
        res.destroy()
        if WHAT == "all":
            hs = [sp.HelmholtzSolver(dims, p / tau, 1, bc=bc) for p, tau in pt]

            def three_solvers():
                for f, (p, tau) in enumerate(pt):
                    hs[f].solve(x[f * G:(f + 1) * G], y[f * G:(f + 1) * G])
                    y[f * G:(f + 1) * G].mul_(1.0 / tau)
            row["res3_three_solvers_us"], _ = dev_us(three_solvers)
            for h in hs:
                h.destroy()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
