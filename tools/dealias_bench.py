#!/usr/bin/env python3
"""Times ChebDealias (cheb_dealias_*) on the device at 128^3 -> 192^3 and 256^3 -> 384^3: device events, 5 warm-up and `reps` timed
calls per case.  multiply and advect beside the composition of existing calls that multiply replaces -- two Resample up, a torch
multiply, a sharp ChebModal.filter keeping n modes per direction, a Resample down -- and beside ChebModal.forward on the coarse
grid (three plain line products: the yardstick for the line kernels' TFLOP/s in the same session).  FLOP are counted from the
launch schedule (2 K per output value of a line product of K points; the pair kernel runs two of them per output value).
usage: dealias_bench.py [reps] [only]     (one JSON line per case to stdout; only: run the calls whose name contains it)"""
import json, os, sys
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


def chain_flop(sizes_in, sizes_out, order):
    """FLOP of line products taking a grid sizes_in to sizes_out direction by direction in `order`."""
    cur, fl = list(sizes_in), 0.0
    for k in order:
        K = cur[k]
        cur[k] = sizes_out[k]
        v = 1.0
        for c in cur:
            v *= c
        fl += 2.0 * K * v
    return fl


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    only = sys.argv[2] if len(sys.argv) > 2 else ""
    sp = ge.load()
    assert torch.cuda.is_available(), "dealias_bench needs a GPU"
    for dims in ((128,) * 3, (256,) * 3):
        d = len(dims)
        h = sp.ChebDealias(dims, 1)
        fine = h.fine
        n, nfine = h.size(), 1
        for m in fine:
            nfine *= m
        u, v, c = (torch.randn(n, dtype=torch.float64, device="cuda") for _ in range(3))
        vel = torch.randn(d * n, dtype=torch.float64, device="cuda")
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        # the composition (what a user of Resample and ChebModal writes today)
        up, down, modal_f, modal_c = sp.Resample(dims, fine), sp.Resample(fine, dims), sp.ChebModal(fine), sp.ChebModal(dims)
        for k, (nk, mk) in enumerate(zip(dims, fine)):
            modal_f.set_filter(k, sp.sharp_filter(mk, nk))
        U, V, W = (torch.empty(nfine, dtype=torch.float64, device="cuda") for _ in range(3))

        def composition():
            up.apply(u, U); up.apply(v, V)
            torch.mul(U, V, out=U)
            modal_f.filter(U, W)
            down.apply(W, out)

        # FLOP from the schedules (equal ratios: direction d-1 runs last on the way up and first on the way down)
        lift = chain_flop(dims, fine, range(d - 1))
        pair = 2.0 * 2.0 * dims[-1] * nfine
        lower = chain_flop(fine, dims, [d - 1] + list(range(d - 1)))
        f_mul = 2 * lift + pair + lower
        f_adv = 2 * d * lift + d * pair + lower            # vel (d fields) and c once per direction (G in it), d pairs
        f_comp = 2 * chain_flop(dims, fine, range(d)) + chain_flop(fine, fine, range(d)) + chain_flop(fine, dims, range(d))
        f_fwd = chain_flop(dims, dims, range(d))
        calls = [("multiply", lambda: h.multiply(u, v, out), f_mul), ("square", lambda: h.multiply(u, u, out), f_mul - lift),
                 ("advect", lambda: h.advect(vel, c, out), f_adv), ("composition", composition, f_comp),
                 ("forward", lambda: modal_c.forward(u, out), f_fwd)]
        for name, fn, fl in calls:
            if only not in name:
                continue
            us = timed(fn, reps)
            print(json.dumps({"case": "x".join(map(str, dims)) + "->" + "x".join(map(str, fine)), "call": name, "us": round(us, 1),
                              "reps": reps, "gflop": round(fl / 1e9, 2), "achieved_tflops": round(fl / us / 1e6, 2),
                              "pair_launch_gflop": round(pair / 1e9, 2), "work_mbytes": round(h.work_bytes() / 1e6, 1)}), flush=True)
        for o in (h, up, down, modal_f, modal_c):
            o.destroy()


if __name__ == "__main__":
    main()
