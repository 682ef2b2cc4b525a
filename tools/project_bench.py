#!/usr/bin/env python3
"""ChebProject.project against the composition a user of the library writes without it, on the cube at 128^3
and 256^3, one vector per call, walls everywhere, device events, 5 warm-up calls and 100 timed ones:
  project      div -> k_project_rhs -> solve -> one accumulating sweep per component, no temporaries beyond phi
  composition  ChebGrad.div, ChebLayout.pack of the interior, a torch gather of +-u_k at the boundary nodes (one index tensor and
               one sign tensor built once), a negation, HelmholtzSolver.solve_full, ChebGrad.grad into a d-field temporary, and
               the subtraction u - grad phi
both giving the same phi and, to the rounding of one subtraction against one accumulate, the same out (checked here).  Every line
also carries the library's launches per call (chebhip_launch_count; torch's own kernels of the composition are not counted).
Prints one JSON line per case.  The per-kernel split comes from a kernel-trace run of the same script with fewer calls:
  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/project_bench.py 5 project
usage: project_bench.py [timed calls] [project|composition|both]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 100
WHAT = sys.argv[2] if len(sys.argv) > 2 else "both"
WARM = 5


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
    return e0.elapsed_time(e1) * 1e3 / REPS, launches


def face_gather(dims):
    """(flat index into u (d, N), sign) per compact boundary node: g = sign * u.view(-1)[index] is the all-wall boundary data."""
    d, N = len(dims), int(np.prod(dims))
    code = sp.project_faces(dims).astype(np.int64)
    node = np.flatnonzero(sp.layout_map(dims).ravel() < 0)
    return torch.from_numpy((code >> 1) * N + node).cuda(), torch.from_numpy(np.where(code & 1, -1.0, 1.0)).cuda()


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "timed_calls": REPS, "warm_up": WARM}), flush=True)
    for n in (128, 256):
        dims = (n,) * 3
        d, N = 3, n ** 3
        u = torch.from_numpy(np.random.default_rng(n).standard_normal((d,) + dims)).cuda()
        row = {"dims": "%d^3" % n}
        phi, out = torch.empty((1,) + dims, dtype=torch.float64, device="cuda"), torch.empty_like(u)
        if WHAT in ("project", "both"):
            P = sp.ChebProject(dims)
            us, launches = dev_us(lambda: P.project(u, out=out, phi=phi))
            row.update(project_us=round(us, 1), project_launches=launches)
            P.destroy()
        if WHAT in ("composition", "both"):
            gr, lay = sp.ChebGrad(dims), sp.ChebLayout(dims)
            hs = sp.HelmholtzSolver(dims, 0.0, bc=["neumann"] * d)
            idx, sign = face_gather(dims)
            dv, f = torch.empty((1,) + dims, dtype=torch.float64, device="cuda"), torch.empty(hs.size, dtype=torch.float64, device="cuda")
            phi2, gp, out2 = torch.empty_like(phi), torch.empty_like(u), torch.empty_like(u)
            uf = u.view(-1)

            def composition():
                gr.div(u, out=dv)
                lay.pack(1, dv, xi=f)
                f.neg_()
                g = uf[idx] * sign
                hs.solve_full(f, g, phi2.view(-1))
                gr.grad(phi2, out=gp)
                torch.sub(u, gp, out=out2)
            us, launches = dev_us(composition)
            row.update(composition_us=round(us, 1), composition_library_launches=launches)
            if WHAT == "both":
                row.update(phi_equal=bool(torch.equal(phi, phi2)), out_max_diff=float((out - out2).abs().max()),
                           speedup=round(row["composition_us"] / row["project_us"], 3))
            gr.destroy(); lay.destroy(); hs.destroy()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
