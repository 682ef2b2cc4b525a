#!/usr/bin/env python3
"""Times cheb_resample_apply (Resample) on the device: device events, warm-up, >= 50 timed applications per case.  For every case the
least work from the shapes -- the FLOP of the per-direction products in the order the library runs them (shrinking directions
first) and the bytes every launch must read and write -- and the share of the FP64 MFMA peak (78.6 TF) and of a 5 TB/s HBM stream
that the measured time is.  usage: resample_bench.py [reps] (writes one JSON line per case to stdout)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge

PEAK_F64 = 78.6e12        # FP64 MFMA, MI355X
HBM = 5.0e12              # the rate the project's streaming launches reach


def bounds(dims_in, dims_out, nodes_in, nodes_out, ncomp):
    """(FLOP, bytes) of the direction-by-direction product, directions in ascending n_out / n_in as cheb_resample_create orders them."""
    k_in = [n - 2 if nodes_in == "interior" else n for n in dims_in]
    k_out = [n - 2 if nodes_out == "interior" else n for n in dims_out]
    order = [k for k in range(len(k_in)) if not (k_in[k] == k_out[k] and nodes_in == nodes_out)]
    order.sort(key=lambda k: k_out[k] / k_in[k])
    cur, flop, byt = list(k_in), 0.0, 0.0
    for k in order:
        size_in = ncomp
        for n in cur:
            size_in *= n
        size_out = size_in // cur[k] * k_out[k]
        flop += 2.0 * k_in[k] * size_out
        byt += 8.0 * (size_in + size_out)
        cur[k] = k_out[k]
    return flop, byt


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    sp = ge.load()
    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    cases = [("64^3->128^3 scalar", [((64,) * 3, (128,) * 3, "all", "all", 1)]),
             ("128^3->256^3 scalar", [((128,) * 3, (256,) * 3, "all", "all", 1)]),
             ("64^3->128^3 Stokes state (velocity ALL->INTERIOR x3 + pressure INTERIOR->INTERIOR)",
              [((64,) * 3, (128,) * 3, "all", "interior", 3), ((64,) * 3, (128,) * 3, "interior", "interior", 1)]),
             ("256^3->128^3 scalar", [((256,) * 3, (128,) * 3, "all", "all", 1)])]
    for name, parts in cases:
        hs, xs, ys = [], [], []
        flop = byt = 0.0
        for p in parts:
            r = sp.Resample(*p)
            hs.append(r)
            xs.append(torch.randn(r.size(0), dtype=torch.float64, device="cuda"))
            ys.append(torch.empty(r.size(1), dtype=torch.float64, device="cuda"))
            f, b = bounds(*p)
            flop += f; byt += b
        for _ in range(5):
            for r, x, y in zip(hs, xs, ys):
                r.apply(x, y)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for r, x, y in zip(hs, xs, ys):
                r.apply(x, y)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        tf, tb = flop / PEAK_F64 * 1e6, byt / HBM * 1e6
        print(json.dumps({"case": name, "us": round(us, 2), "reps": reps, "gflop": round(flop / 1e9, 3), "mbytes": round(byt / 1e6, 1),
                          "flop_bound_us": round(tf, 1), "byte_bound_us": round(tb, 1), "bound": "flop" if tf >= tb else "bytes",
                          "share_of_flop_bound": round(tf / us, 3), "share_of_byte_bound": round(tb / us, 3),
                          "achieved_tflops": round(flop / us / 1e6, 2)}), flush=True)
        for r in hs:
            r.destroy()


if __name__ == "__main__":
    main()
