#!/usr/bin/env python3
"""Direct Helmholtz solves with Neumann / Robin / mixed faces, device events, warm-up first:
  1. full-grid solves (lift + fast-diagonalisation solve + extension, HelmholtzSolver.solve_full) at 128^3 and 256^3 for
     all-Neumann sigma = 1, Robin(1, 1) on every face, and one asymmetric last direction (Dirichlet / Neumann), each beside
     the Dirichlet interior solve (HelmholtzSolver(dims).solve) measured in the same process;
  2. the interior solve of each bc handle alone (solve: g = 0, no lift, no extension), which separates the line-transform
     cost from the two new memory-bound passes.
Prints one JSON line per case.  The lift / extension kernel times come from a kernel-trace run of the same script:
  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/helmholtz_bc_bench.py 5
usage: helmholtz_bc_bench.py [reps]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
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


CASES = [("neumann, sigma 1", ["neumann"] * 3, 1.0),
         ("robin(1,1), sigma 0", [(1.0, 1.0)] * 3, 0.0),
         ("neumann x2 + dirichlet/neumann last, sigma 0", ["neumann", "neumann", ("dirichlet", "neumann")], 0.0)]


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS}), flush=True)
    rng = np.random.default_rng(0)
    for P in (128, 256):
        dims = (P,) * 3
        h0 = sp.HelmholtzSolver(dims)
        f = torch.from_numpy(rng.standard_normal(h0.size)).cuda()
        u0 = torch.empty_like(f)
        dir_us = dev_us(lambda: h0.solve(f, u0))
        h0.destroy()
        for name, bc, sigma in CASES:
            h = sp.HelmholtzSolver(dims, sigma, bc=bc)
            g = torch.from_numpy(rng.standard_normal(h.boundary_size)).cuda()
            u = torch.empty(h.full_size, dtype=torch.float64, device="cuda")
            ui = torch.empty_like(f)
            full_us = dev_us(lambda: h.solve_full(f, g, u))
            interior_us = dev_us(lambda: h.solve(f, ui))
            print(json.dumps({"dims": "%d^3" % P, "bc": name, "full_solve_us": round(full_us, 1), "interior_solve_us": round(interior_us, 1),
                              "lift_plus_extend_us": round(full_us - interior_us, 1), "dirichlet_solve_us": round(dir_us, 1),
                              "ratio_vs_dirichlet": round(full_us / dir_us, 3)}), flush=True)
            h.destroy()


if __name__ == "__main__":
    main()
