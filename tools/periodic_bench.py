#!/usr/bin/env python3
"""Periodic directions beside walls, device events, warm-up first, both handles in the same process:
  1. a (periodic, wall, periodic) Helmholtz solve -- solve (unknown arrays) and solve_full with boundary data (lift + solve +
     extension: the k_bc_* kernels every boundary-condition handle runs) -- against the all-wall Dirichlet handle of the same dims;
  2. ChebGrad.laplacian with the same two periodic directions against the all-wall handle.
Every launch of the periodic handle should be the kernel the all-wall handle launches, on lines two points longer in the periodic
directions; a kernel-trace run of the same script shows whether it is:
  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/periodic_bench.py 5
Prints one JSON line per case.  A number for DESIGN, not a test.
usage: periodic_bench.py [reps]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
MASK = (True, False, True)


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


def helmholtz_us(dims, bc, sigma, rng):
    h = sp.HelmholtzSolver(dims, sigma, bc=bc)
    f = torch.from_numpy(rng.standard_normal(h.size)).cuda()
    g = torch.from_numpy(rng.standard_normal(h.boundary_size)).cuda()
    ui, u = torch.empty_like(f), torch.empty(h.full_size, dtype=torch.float64, device="cuda")
    out = (dev_us(lambda: h.solve(f, ui)), dev_us(lambda: h.solve_full(f, g, u)), h.size)
    h.destroy()
    return out


def laplacian_us(dims, periodic, rng):
    g = sp.ChebGrad(dims, periodic=periodic)
    s = torch.from_numpy(rng.standard_normal(g.N)).cuda()
    out = torch.empty_like(s)
    us = dev_us(lambda: g.laplacian(s, out=out))
    g.destroy()
    return us


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "periodic": MASK}), flush=True)
    rng = np.random.default_rng(0)
    for P in (64, 128, 256):
        dims = (P,) * 3
        for sigma in (0.0, 1.0):
            ws, wf, wn = helmholtz_us(dims, ["dirichlet"] * 3, sigma, rng)
            ps, pf, pn = helmholtz_us(dims, ["periodic" if p else "dirichlet" for p in MASK], sigma, rng)
            print(json.dumps({"dims": "%d^3" % P, "sigma": sigma, "wall_solve_us": round(ws, 1), "periodic_solve_us": round(ps, 1),
                              "solve_ratio": round(ps / ws, 3), "wall_full_us": round(wf, 1), "periodic_full_us": round(pf, 1),
                              "full_ratio": round(pf / wf, 3), "unknowns_ratio": round(pn / wn, 3)}), flush=True)
        wl, pl = laplacian_us(dims, None, rng), laplacian_us(dims, MASK, rng)
        print(json.dumps({"dims": "%d^3" % P, "wall_laplacian_us": round(wl, 1), "periodic_laplacian_us": round(pl, 1),
                          "laplacian_ratio": round(pl / wl, 3)}), flush=True)


if __name__ == "__main__":
    main()
