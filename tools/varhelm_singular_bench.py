#!/usr/bin/env python3
"""The deflated solve and the variable-density projection timed next to their yardsticks, in one session:
device events around whole solves, 2 warm-up solves, REPS timed ones.  Cases: 64^3 and 128^3 between Neumann walls (q = 1) and a
128 x 130 x 128 channel periodic / wall / periodic (q = 4); kappa = 1 + 0.9 prod_k sin(2 x_k + 0.3 k) (contrast 19); one field.
  deflated      VarHelmholtz.solve_deflated with c = 0 to rtol 1e-8, restart 30: us per solve, iterations, us per iteration
  twin          the same handle's solve with c = 1e-3 (nonsingular, the code path of solve): the same three
  remove_null   one Pi alone (three launches), and its predicted share: a Pi moves 24 B per unknown (two reads, one write), an
                iteration runs two of them next to mult's 144 B per node -- 48 / 144 of mult's time if both ran at
                the same bandwidth
  mult          VarHelmholtz.mult, for that prediction
  project_var   ChebProject(variable=True).project at kappa of contrast 19 (its iterations) and at kappa == 1
  project       ChebProject.project (the direct solve) of the same grid and faces
Prints one JSON line per case.
usage: varhelm_singular_bench.py [timed solves, default 5] [largest cube, default 128]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
NMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 128
WARM = 2


def dev_us(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 1)


def kappa(dims, periodic, amp):
    xs = [(-1.0 + 2.0 * np.arange(n) / n) if p else np.cos(np.pi * np.arange(n) / (n - 1)) for n, p in zip(dims, periodic)]
    k = np.ones(dims)
    for j, x in enumerate(np.meshgrid(*xs, indexing="ij")):
        k = k * np.sin(2.0 * x + 0.3 * j)
    return 1.0 + amp * k


def case(dims, vbc, pbc):
    per = sp.bc_split(vbc, len(dims))[0]
    row = {"dims": "x".join(map(str, dims)), "bc": "/".join(vbc)}
    kap = torch.from_numpy(kappa(dims, per, 0.9)).cuda().reshape(-1)
    op = sp.VarHelmholtz(dims, 1, bc=vbc)
    rng = np.random.default_rng(dims[0])
    f = torch.from_numpy(rng.standard_normal(op.size)).cuda()
    y = torch.empty_like(f)
    op.set_coefficients(kap, 0.0)
    row["null_count"] = op.null_count
    row["deflated_us"] = dev_us(lambda: op.solve_deflated(f, rtol=1e-8))
    row.update(deflated_iterations=op.iterations, deflated_reason=op.reason, deflated_us_per_iteration=round(row["deflated_us"] / max(op.iterations, 1), 1))
    row["mult_us"] = dev_us(lambda: op.mult(f, y), 20, 5)
    row["remove_null_us"] = dev_us(lambda: op.remove_null(f, y), 20, 5)
    row["two_pi_over_mult_predicted"] = round(48.0 * op.size / (144.0 * op.full_size), 3)
    row["two_pi_over_mult_measured"] = round(2.0 * row["remove_null_us"] / row["mult_us"], 3)
    op.set_coefficients(kap, 1e-3)
    row["twin_us"] = dev_us(lambda: op.solve(f, rtol=1e-8))
    row.update(twin_iterations=op.iterations, twin_reason=op.reason, twin_us_per_iteration=round(row["twin_us"] / max(op.iterations, 1), 1))
    row["per_iteration_over_twin"] = round(row["deflated_us_per_iteration"] / row["twin_us_per_iteration"], 3)
    op.destroy()
    d = len(dims)
    u = torch.from_numpy(rng.standard_normal((d,) + dims)).cuda()
    out, phi = torch.empty_like(u), torch.empty((1,) + dims, dtype=torch.float64, device="cuda")
    pv = sp.ChebProject(dims, 1, pbc, variable=True)
    pv.set_inverse_density(kap)
    row["project_var_us"] = dev_us(lambda: pv.project(u, out=out, phi=phi, rtol=1e-8))
    row.update(project_var_iterations=pv.iterations, project_var_reason=pv.reason)
    pv.set_inverse_density(torch.ones_like(kap))
    row["project_var_unit_us"] = dev_us(lambda: pv.project(u, out=out, phi=phi, rtol=1e-8))
    row["project_var_unit_iterations"] = pv.iterations
    pv.destroy()
    pc = sp.ChebProject(dims, 1, pbc)
    row["project_us"] = dev_us(lambda: pc.project(u, out=out, phi=phi), 20, 5)
    pc.destroy()
    row["project_var_unit_over_project"] = round(row["project_var_unit_us"] / row["project_us"], 2)
    print(json.dumps(row), flush=True)


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "timed_solves": REPS, "warm_up": WARM}), flush=True)
    for n in (64, 128):
        if n <= NMAX:
            case((n,) * 3, ["neumann"] * 3, ["wall"] * 3)
    case((128, 130, 128), ["periodic", "neumann", "periodic"], ["periodic", "wall", "periodic"])


if __name__ == "__main__":
    main()
