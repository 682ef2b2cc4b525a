#!/usr/bin/env python3
"""Gradients at scattered points on the cube at 128^3 and 256^3 with 1 and 3 fields at 1, 128 and 4096
uniform points, device events, 5 warm-up calls, then 3 windows of timed calls each: `_us` is the median window's time per call,
`_spread` the (max - min) / median of the three:
  eval_grad     ChebPoints.eval_grad: every first derivative of every field in one call
  eval_deriv    d calls of ChebPoints.eval(deriv=e_k) on the same handle
  composition   what the call replaces: ChebGrad.grad into d nfields full-grid fields, then ChebPoints.eval on a handle of that
                many fields; `composition_extra_MB` is the memory of those fields
  eval          the plain evaluation of the fields, for scale
Every line carries the library's launches per call (chebhip_launch_count).  Prints one JSON line per case.  The per-kernel split
comes from a kernel-trace run of the same script with fewer calls and the library's own call only:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/points_deriv_bench.py 5 lib 256
usage: points_deriv_bench.py [timed calls] [all|lib] [128|256]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
WHAT = sys.argv[2] if len(sys.argv) > 2 else "all"
CASE = int(sys.argv[3]) if len(sys.argv) > 3 else None
WARM = 5
WINDOWS = 3


def dev_us(fn, reps):
    """(median device time per call in microseconds over WINDOWS windows of reps back-to-back calls between two events,
    (max - min) / median of the windows, library launches per call)."""
    L = sp.lib()
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    c0 = L.chebhip_launch_count()
    fn()
    launches = L.chebhip_launch_count() - c0
    torch.cuda.synchronize()
    t = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / reps)
    t.sort()
    med = t[len(t) // 2]
    return round(med, 1), round((t[-1] - t[0]) / med, 3), launches


def put(row, key, res):
    row[key + "_us"], row[key + "_spread"], row[key + "_launches"] = res


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "timed_calls": REPS, "windows": WINDOWS, "warm_up": WARM}), flush=True)
    d = 3
    for n in (128, 256):
        if CASE is not None and CASE != n:
            continue
        dims = (n,) * d
        T = n ** d
        for nf in (1, 3):
            rng = np.random.default_rng(n + nf)
            u = torch.from_numpy(rng.standard_normal(nf * T)).cuda()
            h = sp.ChebPoints(dims, nf)
            units = [tuple(1 if k == c else 0 for k in range(d)) for c in range(d)]
            if WHAT == "all":
                gr = sp.ChebGrad(dims)
                hg = sp.ChebPoints(dims, d * nf)
                G = torch.empty(d * nf * T, dtype=torch.float64, device="cuda")
            for npts in (1, 128, 4096):
                reps = max(3, REPS // 8) if npts == 4096 else REPS
                pts = torch.from_numpy(rng.uniform(-1.0, 1.0, (npts, d))).cuda()
                row = {"dims": "%d^3" % n, "nfields": nf, "npts": npts, "chunk": h.chunk, "grad_chunk": max(1, h.chunk // 2)}
                og = torch.empty((nf, d, npts), dtype=torch.float64, device="cuda")
                oe = torch.empty((nf, npts), dtype=torch.float64, device="cuda")
                put(row, "eval_grad", dev_us(lambda: h.eval_grad(u, pts, out=og), reps))
                if WHAT == "all":
                    def d_calls():
                        for a in units:
                            h.eval(u, pts, out=oe, deriv=a)
                    put(row, "eval_deriv", dev_us(d_calls, reps))
                    put(row, "eval", dev_us(lambda: h.eval(u, pts, out=oe), reps))
                    oc = torch.empty((d * nf, npts), dtype=torch.float64, device="cuda")

                    def composition():
                        gr.grad(u, out=G)
                        hg.eval(G, pts, out=oc)
                    put(row, "composition", dev_us(composition, reps))
                    row["composition_chunk"] = hg.chunk
                    row["composition_extra_MB"] = round(d * nf * T * 8e-6, 1)
                print(json.dumps(row), flush=True)
            h.destroy()
            if WHAT == "all":
                gr.destroy(); hg.destroy()


if __name__ == "__main__":
    main()
