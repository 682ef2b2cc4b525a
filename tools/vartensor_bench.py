#!/usr/bin/env python3
"""The tensor mode of VarHelmholtz timed next to the scalar mode of the SAME handle, in one session: device
events, 5 warm-up calls, REPS timed ones (tools/varhelm_bench.py's counts).
Per case (64^3, 128^3, 256^3 with Dirichlet walls; 1 and 3 stacked fields): `mult` in the scalar mode (kappa = 1 + 0.9 prod_k
sin(2 x_k + 0.3 k), c = 0), in the tensor mode without and with a velocity (K = R(theta(x)) diag(2, 1, 0.5) R^T), each with
chebhip_launch_count of one call (the extension's launches are not in that count) and the bytes per second it stands for by the
traffic count of DESIGN 10s, B per node and field: scalar 144, tensor 264, tensor with a velocity 304; then `precond` in both modes.
Then the iteration counts of `solve` to 1e-8 (restart 30, at most 200 iterations, N(0,1) right-hand side, c = 0) at 64^3 and 128^3
between walls and on the 128 x 130 x 128 (periodic, wall, periodic) channel, for the anisotropies k_1 / k_2 = 1, 10, 100 (K = R
diag(a, 1, 1) R^T with the rotating theta) and the cell Peclet numbers max|v| h / k_min = 0, 1, 10 (h the widest node spacing of the
grid, v = the smooth field of unit maximum scaled to that); a negative count is a solve that had not converged after that many
iterations.  Prints one JSON line per case.
The per-kernel split comes from a kernel-trace run of its own with fewer calls and one size:
  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/vartensor_bench.py 5 128 trace
usage: vartensor_bench.py [timed calls] [largest cube, default 256] [trace: that cube with one field only, no iteration table]"""
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
BYTES = {"scalar": 144, "tensor": 264, "tensor_vel": 304}


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


def spacing(dims, periodic):
    """The widest node spacing of the grid."""
    return max(2.0 / n if p else float(np.abs(np.diff(np.cos(np.pi * np.arange(n) / (n - 1)))).max()) for n, p in zip(dims, periodic))


def kappa(dims, periodic, amp):
    k = np.ones(dims)
    for j, x in enumerate(coords(dims, periodic)):
        k = k * np.sin(2.0 * x + 0.3 * j)
    return 1.0 + amp * k


def tensor(dims, periodic, k):
    """R diag(k) R^T in the order sp.tensor_order(3): R = the rotation by theta(x) = 0.7 + sin(x_0 + 0.3) cos(0.8 x_2) about
    direction 1 after a fixed one by 0.6 about direction 2."""
    X = coords(dims, periodic)
    th = 0.7 + np.sin(X[0] + 0.3) * np.cos(0.8 * X[2])
    c, s = np.cos(th), np.sin(th)
    c2, s2 = np.cos(0.6), np.sin(0.6)
    R = [[c * c2, -c * s2, -s], [s2 * np.ones(dims), c2 * np.ones(dims), np.zeros(dims)], [s * c2, -s * s2, c]]
    return np.stack([sum(R[i][m] * k[m] * R[j][m] for m in range(3)) for i, j in sp.tensor_order(3)])


def velocity(dims, periodic):
    X = coords(dims, periodic)
    v = np.stack([np.cos(X[k] + 0.5 * k) * np.sin(1.3 * X[(k + 1) % 3] + 0.2) for k in range(3)])
    return v / np.abs(v).max()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1)


def case(dims, bc, nf):
    per = sp.bc_split(bc, 3)[0]
    op = sp.VarHelmholtz(dims, nf, bc=bc)
    N = int(np.prod(dims))
    kap, K, v = cu(kappa(dims, per, 0.9)), cu(tensor(dims, per, (2.0, 1.0, 0.5))), cu(velocity(dims, per))
    rng = np.random.default_rng(dims[0] + nf)
    x = torch.from_numpy(rng.standard_normal(op.size)).cuda()
    y = torch.empty_like(x)
    row = {"dims": "x".join(map(str, dims)), "nfields": nf}
    for name in ("scalar", "tensor", "tensor_vel"):
        if name == "scalar":
            op.set_coefficients(kap, 0.0)
        else:
            op.set_tensor(K, 0.0, v if name == "tensor_vel" else None)
        us, launches = dev_us(lambda: op.mult(x, y))
        row["mult_%s_us" % name], row["mult_%s_launches" % name] = us, launches
        row["mult_%s_TBps" % name] = round(BYTES[name] * N * nf / us * 1e-6, 2)
        if name != "tensor":
            row["precond_%s_us" % name] = dev_us(lambda: op.precond(x, y))[0]
    row["tensor_over_scalar"] = round(row["mult_tensor_us"] / row["mult_scalar_us"], 2)
    row["tensor_vel_over_scalar"] = round(row["mult_tensor_vel_us"] / row["mult_scalar_us"], 2)
    row["work_MB"] = round(op.work_bytes() / 2 ** 20, 1)
    op.destroy()
    print(json.dumps(row), flush=True)


def iterations(dims, bc):
    per = sp.bc_split(bc, 3)[0]
    op = sp.VarHelmholtz(dims, 1, bc=bc)
    f = torch.from_numpy(np.random.default_rng(7).standard_normal(op.size)).cuda()
    h = spacing(dims, per)
    v1 = velocity(dims, per)
    for a in (1.0, 10.0, 100.0):
        K = cu(tensor(dims, per, (a, 1.0, 1.0)))
        row = {"dims": "x".join(map(str, dims)), "bc": "/".join(bc), "k1_over_k2": a, "h": round(h, 5)}
        for pe in (0.0, 1.0, 10.0):
            op.set_tensor(K, 0.0, None if pe == 0.0 else cu(v1 * (pe / h)))
            op.solve(f, rtol=1e-8, max_it=200, restart=30)
            row["peclet_%g" % pe] = op.iterations if op.reason == 2 else -op.iterations
        print(json.dumps(row), flush=True)
    op.destroy()


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "timed_calls": REPS, "warm_up": WARM, "bytes_per_node_and_field": BYTES}), flush=True)
    walls = ["dirichlet"] * 3
    if TRACE:
        case((NMAX,) * 3, walls, 1)
        return
    for n in (64, 128, 256):
        if n > NMAX:
            continue
        for nf in (1, 3):
            case((n,) * 3, walls, nf)
    for dims, bc in (((64,) * 3, walls), ((128,) * 3, walls), ((128, 130, 128), ["periodic", "dirichlet", "periodic"])):
        iterations(dims, bc)


if __name__ == "__main__":
    main()
