#!/usr/bin/env python3
"""Times the ChebModal calls (cheb_modal_*) on the device: device events, warm-up, 100 timed calls per case.  forward / backward /
filter (all directions filtered) against their flop bound -- d products of 2 n FLOP per value at the FP64 MFMA peak (78.6 TF) --
and integrate / spectrum against their byte bound -- one read of the field (two with v).
usage: modal_bench.py [reps] [only]     (one JSON line per case to stdout; only: run the calls whose name contains it)"""
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
    assert torch.cuda.is_available(), "modal_bench needs a GPU"
    for dims in ((128,) * 3, (256,) * 3):
        m = sp.ChebModal(dims, 1)
        n = m.size()
        u, v = (torch.randn(n, dtype=torch.float64, device="cuda") for _ in range(2))
        a = torch.empty(n, dtype=torch.float64, device="cuda")
        E = torch.empty(m.spectrum_size(), dtype=torch.float64, device="cuda")
        out = torch.empty(1, dtype=torch.float64, device="cuda")
        for k, nk in enumerate(dims):
            m.set_filter(k, sp.exp_filter(nk))
        flop = sum(2.0 * nk * n for nk in dims)
        calls = [("forward", lambda: m.forward(u, a), flop, 0.0), ("backward", lambda: m.backward(u, a), flop, 0.0),
                 ("filter", lambda: m.filter(u, a), flop, 0.0), ("integrate", lambda: m.integrate(u, None, out), 0.0, 8.0 * n),
                 ("integrate_uv", lambda: m.integrate(u, v, out), 0.0, 16.0 * n), ("spectrum", lambda: m.spectrum(u, E), 0.0, 8.0 * n)]
        for name, fn, fl, by in calls:
            if only not in name:
                continue
            us = timed(fn, reps)
            rec = {"case": "x".join(map(str, dims)), "call": name, "us": round(us, 2), "reps": reps}
            if fl:
                rec.update(gflop=round(fl / 1e9, 3), flop_bound_us=round(fl / PEAK_F64 * 1e6, 1), achieved_tflops=round(fl / us / 1e6, 2))
            else:
                rec.update(mbytes=round(by / 1e6, 1), achieved_tbytes_per_s=round(by / us / 1e6, 3))
            print(json.dumps(rec), flush=True)
        m.destroy()


if __name__ == "__main__":
    main()
