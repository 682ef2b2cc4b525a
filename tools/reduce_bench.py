#!/usr/bin/env python3
"""Times ChebReduce (cheb_reduce_*) on the device: device events, 5 warm-up and 100 timed calls per case.  128^3 and 256^3, one
field, with and without v: the full contraction, each direction kept alone and each direction contracted alone, next to
ChebModal.integrate (the same bytes as the full contraction: the yardstick is its time per byte) and to the torch.einsum
composition of each output (a vendor GEMM route; u v is formed first where v is given).  Bytes = the input arrays read once.
usage: reduce_bench.py [reps] [only]     (one JSON line per case to stdout; only: run the cases whose name contains it)"""
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


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    only = sys.argv[2] if len(sys.argv) > 2 else ""
    sp = ge.load()
    assert torch.cuda.is_available(), "reduce_bench needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(20241018)
    configs = [("full", (0, 1, 2)), ("keep0", (1, 2)), ("keep1", (0, 2)), ("keep2", (0, 1)), ("over0", (0,)), ("over1", (1,)), ("over2", (2,))]
    for dims in ((128,) * 3, (256,) * 3):
        case = "x".join(map(str, dims))
        n = dims[0] * dims[1] * dims[2]
        u = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        v = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        u3, v3 = u.view(dims), v.view(dims)
        w = [torch.from_numpy(sp.cc_weights(m)).cuda() for m in dims]
        m = sp.ChebModal(dims, 1)
        mo = torch.empty(1, dtype=torch.float64, device="cuda")

        def line(call, us, nin, **more):
            byt = 8.0 * n * nin
            print(json.dumps(dict(case=case, call=call, us=round(us, 2), bytes=int(byt), tbps=round(byt / us / 1e6, 3), reps=reps, **more)), flush=True)

        for nin, vv in ((1, None), (2, v)):
            tag = "uv" if vv is not None else "u"
            if only in "integrate_" + tag:
                line("integrate_" + tag, timed(lambda: m.integrate(u, vv, mo), reps), nin)
            for name, over in configs:
                if only not in name + "_" + tag:
                    continue
                h = sp.ChebReduce(dims, 1, over=over)
                out = torch.empty((1,) + h.out_dims, dtype=torch.float64, device="cuda")
                line(name + "_" + tag, timed(lambda: h.apply(u, vv, out), reps), nin, slices=h.slices, outputs=h.size(1))
                h.destroy()
                spec = "abc," + ",".join("abc"[k] for k in over) + "->" + "".join("abc"[k] for k in range(3) if k not in over)
                ops = [w[k] for k in over]
                ein = (lambda: torch.einsum(spec, u3 * v3, *ops)) if vv is not None else (lambda: torch.einsum(spec, u3, *ops))
                line("einsum_" + name + "_" + tag, timed(ein, reps), nin)
        m.destroy()


if __name__ == "__main__":
    main()
