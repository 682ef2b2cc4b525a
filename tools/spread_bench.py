#!/usr/bin/env python3
"""Times ChebPoints.spread (cheb_points_spread) on the device: device events, 5 warm-up and 100 timed calls per case.  One field at
128^3 and 256^3 for npts in {1, 128, 4096}, against two figures taken in the same session: ChebPoints.eval of the same points on
the same handle, and the composition a user had before -- rows() per direction and one torch.einsum (a vendor GEMM over an
npts x n_1 n_2 array).  The matrix-core product of spread is 2 npts prod(dims) FLOP, eval's direction 0.
usage: spread_bench.py [reps] [only]     (one JSON line per case to stdout; only: run the cases whose name contains it)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge

PEAK_F64 = 78.6e12        # FP64 MFMA, MI355X


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
    assert torch.cuda.is_available(), "spread_bench needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(20240229)
    uniform = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0
    for dims in ((128,) * 3, (256,) * 3):
        case = "x".join(map(str, dims))
        h = sp.ChebPoints(dims, 1)
        n = h.size()
        u = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        g = torch.zeros(n, dtype=torch.float64, device="cuda")
        for npts in (1, 128, 4096):
            name = "spread_%d" % npts
            if only not in name:
                continue
            pts = uniform(npts, 3)
            s = torch.randn((1, npts), dtype=torch.float64, device="cuda", generator=gen)
            vals = torch.empty((1, npts), dtype=torch.float64, device="cuda")
            us = timed(lambda: h.spread(s, pts, out=g), reps)
            us_acc = timed(lambda: h.spread(s, pts, out=g, accumulate=True), reps)
            us_delta = timed(lambda: h.spread(s, pts, out=g, delta=True), reps)
            us_eval = timed(lambda: h.eval(u, pts, vals), reps)

            def composition():
                R = [h.rows(k, pts[:, k].contiguous()) for k in range(3)]
                return torch.einsum("fp,pi,pj,pk->fijk", s, *R)
            us_comp = timed(composition, reps)
            err = float(torch.linalg.norm(h.spread(s, pts, out=g).reshape(dims) - composition()[0]) / torch.linalg.norm(g))
            flop = 2.0 * npts * n
            print(json.dumps({"case": case, "call": name, "pass": h.spread_pass(), "passes": -(-npts // h.spread_pass()), "us": round(us, 2),
                              "us_accumulate": round(us_acc, 2), "us_delta": round(us_delta, 2), "us_eval": round(us_eval, 2),
                              "us_rows_einsum": round(us_comp, 2), "spread_over_eval": round(us / us_eval, 3),
                              "spread_over_rows_einsum": round(us / us_comp, 3), "product_gflop": round(flop / 1e9, 3),
                              "flop_bound_us": round(flop / PEAK_F64 * 1e6, 1), "out_mib": n * 8 >> 20,
                              "rel_diff_to_rows_einsum": float("%.3g" % err), "reps": reps}), flush=True)
        h.destroy()


if __name__ == "__main__":
    main()
