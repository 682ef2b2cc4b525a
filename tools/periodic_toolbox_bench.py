#!/usr/bin/env python3
"""The toolbox on a channel: a (periodic, wall, periodic) handle of ChebDealias, ChebProject, ChebOpFun and
ChebPoints against the all-wall handle of the same dims, device events, warm-up first, both handles in the same process, at 64^3,
128^3 and 256^3 (a case whose buffers do not fit is reported as skipped).
  dealias   advect of 3 fields; the fine grids differ (3 floor(n/2) + 1 against ceil(3n/2) points), so the ratio of the fine-grid
            FLOP counts is printed beside the ratio of the times
  project   one projection of one velocity
  opfun     apply of "exp" on one field (unknown layout)
  points    eval of one chunk of scattered points, 3 fields
With --wall-only only the all-wall handles run (a tree from before the periodic toolbox can run the script that way).
Prints one JSON line per case.  A number for DESIGN, not a test.
usage: periodic_toolbox_bench.py [reps] [--wall-only]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(ARGS[0]) if ARGS else 10
WALL_ONLY = "--wall-only" in sys.argv
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


def rand(n, rng):
    return torch.from_numpy(rng.standard_normal(int(n))).cuda()


def dealias_case(dims, periodic, rng):
    kw = {} if periodic is None else {"periodic": periodic}
    h = sp.ChebDealias(dims, 3, **kw)
    N = int(np.prod(dims))
    vel, c, out = rand(3 * N, rng), rand(3 * N, rng), torch.empty(3 * N, dtype=torch.float64, device="cuda")
    us = dev_us(lambda: h.advect(vel, c, out=out))
    # line products of the way up (every operand image), direction l's pair products and the way down, 2 m n per line and direction
    fine = h.fine
    flops, cur = 0.0, list(dims)
    for k in range(3):
        flops += 2.0 * fine[k] * dims[k] * np.prod(cur) / cur[k]
        cur[k] = fine[k]
    h.destroy()
    return us, 2.0 * flops, fine


def project_case(dims, periodic, rng):
    bc = None if periodic is None else ["periodic" if p else "wall" for p in periodic]
    h = sp.ChebProject(dims, 1, bc)
    u = rand(3 * h.size, rng)
    out, phi = torch.empty_like(u), torch.empty(h.size, dtype=torch.float64, device="cuda")
    us = dev_us(lambda: h.project(u, out=out, phi=phi))
    h.destroy()
    return us


def opfun_case(dims, periodic, rng):
    bc = ["dirichlet"] * 3 if periodic is None else ["periodic" if p else "dirichlet" for p in periodic]
    h = sp.ChebOpFun(dims, 1, 1, 0.0, bc=bc)
    h.set_terms("exp", tau=1e-3)
    x = rand(h.size, rng)
    out = torch.empty_like(x)
    us = dev_us(lambda: h.apply(x, out=out))
    n = h.size
    h.destroy()
    return us, n


def points_case(dims, periodic, rng):
    kw = {} if periodic is None else {"periodic": periodic}
    h = sp.ChebPoints(dims, 3, **kw)
    npts = int(h.chunk)
    u = rand(h.size(), rng)
    pts = torch.from_numpy(rng.uniform(-1, 1, (npts, 3))).cuda()
    out = torch.empty((3, npts), dtype=torch.float64, device="cuda")
    us = dev_us(lambda: h.eval(u, pts, out=out))
    h.destroy()
    return us, npts


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": REPS, "periodic": MASK, "wall_only": WALL_ONLY}), flush=True)
    rng = np.random.default_rng(0)
    for P in (64, 128, 256):
        dims = (P,) * 3
        for name, case in (("dealias", dealias_case), ("project", project_case), ("opfun", opfun_case), ("points", points_case)):
            row = {"dims": "%d^3" % P, "module": name}
            try:
                w = case(dims, None, rng)
                p = None if WALL_ONLY else case(dims, MASK, rng)
            except sp.ChebhipError as e:
                row["skipped"] = str(e)
                print(json.dumps(row), flush=True)
                continue
            wu = w if isinstance(w, float) else w[0]
            row["wall_us"] = round(wu, 1)
            if p is not None:
                pu = p if isinstance(p, float) else p[0]
                row["periodic_us"] = round(pu, 1)
                row["ratio"] = round(pu / wu, 3)
            if name == "dealias":
                row["wall_fine"] = list(w[2])
                if p is not None:
                    row["periodic_fine"] = list(p[2])
                    row["flop_ratio"] = round(p[1] / w[1], 3)
            if name == "opfun" and p is not None:
                row["unknowns_ratio"] = round(p[1] / w[1], 3)
            if name == "points":
                row["points"] = w[1]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
