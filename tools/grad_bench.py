#!/usr/bin/env python3
"""Times ChebGrad (cheb_grad_*) and ChebLayout (cheb_layout_*) on the device: device events, 5 warm-up and 100 timed calls per case,
at 128^3 and 256^3 with three components.  Each operator, `invariants` with the full mask and `stokes_fields`, next to what a user
writes without them for the same result: one ChebPlan.mult per term plus torch arithmetic for the operators, the index tensors of
solve._node_split for the layout.  Every line also carries the sweep / kernel launches of one call (chebhip_launch_count).
usage: grad_bench.py [reps] [only]     (one JSON line per case to stdout; only: run the cases whose name contains it)"""
import json, os, sys
from importlib import import_module
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    only = sys.argv[2] if len(sys.argv) > 2 else ""
    sp = ge.load()
    solve = import_module(sp.__name__ + ".solve")
    assert torch.cuda.is_available(), "grad_bench needs a GPU"
    L = sp.lib()
    gen = torch.Generator(device="cuda").manual_seed(20261018)
    names = ("div", "vort2", "strain2", "gamma", "q", "norm2")
    for dims in ((128,) * 3, (256,) * 3):
        case = "x".join(map(str, dims))
        d, N = 3, dims[0] * dims[1] * dims[2]
        u = torch.randn(3 * N, dtype=torch.float64, device="cuda", generator=gen)
        g = sp.ChebGrad(dims)
        plans = [sp.ChebPlan((3,) + dims, k + 1) for k in range(3)]
        one = [sp.ChebPlan(dims, k) for k in range(3)]
        t = [torch.empty(3 * N, dtype=torch.float64, device="cuda") for _ in range(3)]      # D_k of the three components
        uc = [u[c * N:(c + 1) * N] for c in range(3)]
        s1 = [torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(6)]
        pair = lambda k, c: t[k][c * N:(c + 1) * N]                                        # d_k u_c after the batched plan

        def line(call, fn, **more):
            if only not in call:
                return
            c0 = L.chebhip_launch_count()
            fn()
            launches = L.chebhip_launch_count() - c0
            print(json.dumps(dict(case=case, call=call, us=round(timed(fn, reps), 2), launches=launches, reps=reps, **more)), flush=True)

        def sweeps():
            for k in range(3):
                plans[k].mult(u, t[k])

        outs = {op: torch.empty((n,) + dims, dtype=torch.float64, device="cuda") for op, n in
                (("grad", 9), ("div", 1), ("curl", 3), ("strain", 6), ("laplacian", 3), ("inv", 6))}
        line("grad", lambda: g.grad(u, outs["grad"]))
        line("plan_grad", sweeps)                      # (component-major instead of the tensor's layout: no transposition is timed)
        line("div", lambda: g.div(u, outs["div"]))

        def plan_div():
            for k in range(3):
                one[k].mult(uc[k], s1[k])
            return (s1[0] + s1[1]) + s1[2]
        line("plan_div", plan_div)
        line("curl", lambda: g.curl(u, outs["curl"]))

        def plan_curl():
            for i in range(3):
                a, b = (i + 1) % 3, (i + 2) % 3
                one[a].mult(uc[b], s1[2 * i]); one[b].mult(uc[a], s1[2 * i + 1])
            return [s1[2 * i] - s1[2 * i + 1] for i in range(3)]
        line("plan_curl", plan_curl)
        line("strain", lambda: g.strain(u, outs["strain"]))

        def plan_strain():
            sweeps()
            return [pair(c, c) if c == k else 0.5 * pair(k, c) + 0.5 * pair(c, k) for c in range(3) for k in range(c, 3)]
        line("plan_strain", plan_strain)
        line("laplacian", lambda: g.laplacian(u, outs["laplacian"]))

        def plan_laplacian():
            acc = None
            for k in range(3):
                plans[k].mult(u, t[0]); plans[k].mult(t[0], t[1])
                acc = t[1].clone() if acc is None else acc + t[1]
            return acc
        line("plan_laplacian", plan_laplacian)
        G = g.tensor(u)
        line("invariants_from", lambda: g.invariants_from(G, names, outs["inv"]))
        line("invariants", lambda: g.invariants(u, names, outs["inv"]))

        def torch_invariants():
            T = G.view(3, 3, N)
            S = 0.5 * (T + T.transpose(0, 1))
            W = T - T.transpose(0, 1)
            ss = (S * S).sum(dim=(0, 1))
            vv = 0.5 * (W * W).sum(dim=(0, 1))
            return T[0, 0] + T[1, 1] + T[2, 2], vv, ss, 0.5 * ss, 0.25 * vv - 0.5 * ss, (T * T).sum(dim=(0, 1))
        line("torch_invariants", torch_invariants)

        # the layout: a Stokes state to d + 1 full-grid fields
        op = sp.StokesOp(dims)
        x = torch.randn(op.global_size, dtype=torch.float64, device="cuda", generator=gen)
        dv = torch.randn(op.dirichlet_size, dtype=torch.float64, device="cuda", generator=gen)
        line("stokes_fields", lambda: solve.stokes_fields(sp, op, x, dv))
        inner, bnd = solve._node_split(dims, x.device)

        def index_fields():
            xc = x.view(-1, d + 1)
            full = torch.zeros((d + 1, N), dtype=torch.float64, device=x.device)
            for c in range(d):
                full[c][inner] = xc[:, c]
                full[c][bnd] = dv.view(-1, d)[:, c]
            full[d][inner] = xc[:, d]
            return full
        line("index_fields", index_fields)
        op.destroy()
        for p in plans + one:
            p.destroy()
        g.destroy()


if __name__ == "__main__":
    main()
