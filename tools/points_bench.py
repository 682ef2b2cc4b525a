#!/usr/bin/env python3
"""Times ChebPoints (cheb_points_*) on the device: device events, 5 warm-up and 100 timed calls per case.  Scattered points at
128^3 and 256^3 for npts in {1, chunk, 4096} (per call, per chunk and per point; direction 0's line product is
2 chunk prod(dims) FLOP per chunk), a 256^2 plane cut and a 256^3 -> 300^3 uniform grid (sum over the directions of
2 n_k x values of the product's output FLOP).
usage: points_bench.py [reps] [only]     (one JSON line per case to stdout; only: run the cases whose name contains it)"""
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
    assert torch.cuda.is_available(), "points_bench needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(20240229)
    uniform = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0
    for dims in ((128,) * 3, (256,) * 3):
        case = "x".join(map(str, dims))
        h = sp.ChebPoints(dims, 1)
        n = h.size()
        u = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        C = h.chunk
        for npts in (1, C, 4096):
            name = "eval_%d" % npts
            if only not in name:
                continue
            pts = uniform(npts, 3)
            out = torch.empty((1, npts), dtype=torch.float64, device="cuda")
            us = timed(lambda: h.eval(u, pts, out), reps)
            chunks = -(-npts // C)
            flop = 2.0 * npts * n
            print(json.dumps({"case": case, "call": name, "chunk": C, "chunks": chunks, "us": round(us, 2), "us_per_chunk": round(us / chunks, 2),
                              "us_per_point": round(us / npts, 3), "line_product_gflop": round(flop / 1e9, 3),
                              "flop_bound_us": round(flop / PEAK_F64 * 1e6, 1), "reps": reps}), flush=True)
        if dims[0] == 256:
            if only in "plane_256x256":
                coords = [torch.tensor([0.3], dtype=torch.float64, device="cuda"), uniform(256), uniform(256)]
                h.reserve_grid((1, 256, 256))
                out = torch.empty((1, 1, 256, 256), dtype=torch.float64, device="cuda")
                us = timed(lambda: h.eval_grid(u, coords, out), reps)
                flop = 2.0 * 256 * (256 * 256 + 256 * 256 + 256 * 256)          # 1 x 256 x 256, then the two directions of the plane
                print(json.dumps({"case": case, "call": "plane_256x256", "us": round(us, 2), "gflop": round(flop / 1e9, 3), "reps": reps}), flush=True)
            if only in "grid_300x300x300":
                coords = [torch.linspace(-1.0, 1.0, 300, dtype=torch.float64, device="cuda") for _ in range(3)]
                h.reserve_grid((300, 300, 300))
                out = torch.empty((1, 300, 300, 300), dtype=torch.float64, device="cuda")
                us = timed(lambda: h.eval_grid(u, coords, out), reps)
                flop = 2.0 * 256 * (300 * 256 * 256 + 300 * 300 * 256 + 300 * 300 * 300)
                print(json.dumps({"case": case, "call": "grid_300x300x300", "us": round(us, 2), "gflop": round(flop / 1e9, 3),
                                  "achieved_tflops": round(flop / us / 1e6, 2), "reps": reps}), flush=True)
        h.destroy()


if __name__ == "__main__":
    main()
