#!/usr/bin/env python3
"""Output bits of everything that goes through the full-grid kernels of the Helmholtz handles (the lift k_bc_lift,
the extension k_bc_extend_col / _row): HelmholtzSolver.solve_full with noise data, with signed powers of two
and with g = None, ChebOpFun.apply_full and ChebProject.project, on all-wall handles and on handles with periodic directions, once
as the library starts and once with the option general_kernels.  One line per case -- a shape and its periodic mask -- with one
SHA-256 over the output bytes of all its handles (1 and 3 fields, sigma 0 and 1.5, with and without scale), so a pair of runs stays
short enough to commit; --all prints a line per output as well, which is what to look at when two case lines differ.  Inputs from a
fixed NumPy seed.  The script compares nothing: run it on two builds of the library, each in a fresh process, and diff the outputs
    python tools/helmholtz_bits.py > new.txt
    CHEBHIP_LIB_PATH=/elsewhere/libchebhip.so python tools/helmholtz_bits.py > parent.txt
(profiles/helmholtz_bc/bits_parent.txt and bits_new.txt are such a pair).
usage: helmholtz_bits.py [--all]"""
import hashlib, itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
SEED = 20261020
ALL = "--all" in sys.argv[1:]
CASE = [None]                                    # the running hash of the case at hand

WALL_SHAPES = [(9,), (12, 10), (8, 7, 6), (66, 12, 5), (6, 5, 96), (256, 4, 3), (7, 6, 5, 6), (12,) * 5]
# the (dims, mask) pairs of tests/test_gpu_periodic.py's FULL: every mask with a periodic and a wall direction, and one d = 4 case
SHAPES_12 = [(8,), (9,), (16, 9), (12, 16)]
SHAPES_3 = [(16, 9, 12), (7, 6, 16), (6, 5, 96), (6, 66, 5), (256, 4, 3)]
MASKS_3 = [(1, 0, 1), (0, 1, 0), (1, 1, 1), (0, 0, 1)]
PERIODIC = [(dims, m) for dims in SHAPES_12 + SHAPES_3
            for m in (MASKS_3 if len(dims) == 3 else [m for m in itertools.product((0, 1), repeat=len(dims)) if any(m)])
            if not all(m) and all(n <= 256 for n, p in zip(dims, m) if p)] + [((4, 5, 4, 6), (1, 0, 1, 0))]
WALLS = ["dirichlet", "neumann", (1.0, 1.0), ("dirichlet", "neumann")]
FACES = ["wall", "open", ("wall", "open"), ("open", "wall")]
SCALE = {1: (0.75,), 2: (0.5, 2.0), 3: (0.5, 1.0, 2.0), 4: (0.5, 1.0, 2.0, 1.5), 5: (0.5, 1.0, 2.0, 1.5, 0.75)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().reshape(-1)


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def emit(tag, what, fn):
    line = "%s %s %s" % (tag, what, fn())
    CASE[0].update(line.encode())
    if ALL:
        print(line, flush=True)


def attempt(tag, what, fn, *args):
    try:
        fn(tag, *args)
    except (sp.ChebhipError, ValueError) as e:           # (a refusal is an output too: both builds must give the same one)
        emit(tag, what, lambda: "refused: %s" % e)


def helmholtz(tag, dims, bc, sigma, nf, scale, rng):
    h = sp.HelmholtzSolver(dims, sigma, nf, bc=bc, scale=scale)
    f = dev(rng.standard_normal(h.size))
    u = torch.empty(h.full_size, dtype=torch.float64, device="cuda")
    g = dev(rng.standard_normal(h.boundary_size))
    g2 = dev(rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], size=h.boundary_size))
    emit(tag, "solve_full noise", lambda: sha(h.solve_full(f, g, u)))
    emit(tag, "solve_full pow2", lambda: sha(h.solve_full(f, g2, u)))
    emit(tag, "solve_full none", lambda: sha(h.solve_full(f, None, u)))
    h.destroy()


def opfun(tag, dims, bc, sigma, nf, scale, rng):
    h = sp.ChebOpFun(dims, nf, nf, sigma, bc=bc, scale=scale)
    h.set_terms("exp", tau=0.01)
    x = dev(rng.standard_normal(h.size))
    emit(tag, "opfun apply_full", lambda: sha(h.apply_full(x)))
    h.destroy()


def project(tag, dims, faces, nvec, scale, rng):
    h = sp.ChebProject(dims, nvec, bc=faces, scale=scale)
    u = dev(rng.standard_normal(nvec * len(dims) * h.size)).reshape((nvec * len(dims),) + tuple(dims))
    flux = dev(rng.standard_normal(nvec * h.boundary_size))
    emit(tag, "project", lambda: sha(h.project(u, flux=flux)))
    h.destroy()


def main():
    cases = [(dims, (0,) * len(dims)) for dims in WALL_SHAPES] + PERIODIC
    for general in (0, 1):
        sp.set_option("general_kernels", general)
        for q, (dims, mask) in enumerate(cases):
            d = len(dims)
            CASE[0] = hashlib.sha256()
            wall = [WALLS[(q + k) % len(WALLS)] for k in range(d)]
            bc = ["periodic" if p else w for p, w in zip(mask, wall)]
            for nf, sigma, scaled in itertools.product((1, 3), (0.0, 1.5), (False, True)):
                scale = SCALE[d] if scaled else None
                tag = "general_kernels=%d %s mask=%s nf=%d sigma=%g scale=%s" % (
                    general, "x".join(map(str, dims)), "".join(map(str, mask)), nf, sigma, "box" if scaled else "none")
                rng = np.random.default_rng([SEED, q, nf, int(2 * sigma), int(scaled)])
                attempt(tag, "solve_full", helmholtz, dims, bc, sigma, nf, scale, rng)
                if any(mask):                            # (ChebOpFun and ChebProject take walls only)
                    continue
                attempt(tag, "opfun", opfun, dims, wall, sigma, nf, scale, rng)
                if sigma == 0.0 and nf * d <= 16:
                    attempt(tag, "project", project, dims, [FACES[(q + k) % len(FACES)] for k in range(d)], nf, scale, rng)
            print("general_kernels=%d %s mask=%s %s" % (general, "x".join(map(str, dims)), "".join(map(str, mask)), CASE[0].hexdigest()), flush=True)


if __name__ == "__main__":
    main()
