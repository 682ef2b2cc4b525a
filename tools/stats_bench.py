#!/usr/bin/env python3
"""ChebStats against the torch compositions a user writes without it, on the cube at 128^3 and 256^3 with
1 and 3 fields, device events, 5 warm-up calls, then 3 windows of 200 timed calls each: `_us` is the median window's time per
call, `_spread` the (max - min) / median of the three:
  summary    against min, argmin, max, argmax, isnan().sum() and four weighted power sums, field by field (W precomputed once,
             outside the timed window)
  hist       CHEB_STATS_UNIFORM and CHEB_STATS_EDGES with 64 and 1024 bins, on N(0, 1) over (-4, 4), against torch.bincount with
             weights of precomputed slots plus the slot computation itself (bucketize for the edges) -- the composition adds with
             floating atomics: its low bits change from run to run; and on the same data sorted (a whole wave in one bin: the
             groups that are added in registers)
  cfl        against (|v_0| r_0 + |v_1| r_1 + |v_2| r_2).max() with the rates broadcast
Every line carries the library's launches per call (chebhip_launch_count) and the bytes of input per second.  Prints one JSON
line per case.  The per-kernel split comes from a kernel-trace run of the same script with fewer calls and the library only:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/stats_bench.py 5 lib 256
usage: stats_bench.py [timed calls] [all|lib] [128|256]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
WHAT = sys.argv[2] if len(sys.argv) > 2 else "all"
CASE = int(sys.argv[3]) if len(sys.argv) > 3 else None
WARM = 5
WINDOWS = 3


def dev_us(fn):
    """(median device time per call in microseconds over WINDOWS windows of REPS back-to-back calls between two events,
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
        for _ in range(REPS):
            fn()
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / REPS)
    t.sort()
    med = t[len(t) // 2]
    return round(med, 1), round((t[-1] - t[0]) / med, 3), launches


def put(row, key, res, nbytes, lib=True):
    us, spread, launches = res
    row[key + "_us"] = us
    row[key + "_spread"] = spread
    row[key + "_GBps"] = round(nbytes / us * 1e-3, 1)
    if lib:
        row[key + "_launches"] = launches


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "timed_calls": REPS, "windows": WINDOWS, "warm_up": WARM}), flush=True)
    for n in (128, 256):
        if CASE is not None and CASE != n:
            continue
        dims = (n,) * 3
        T = n ** 3
        for nf in (1, 3):
            rng = np.random.default_rng(n + nf)
            u = torch.from_numpy(rng.standard_normal(nf * T)).cuda()
            us = torch.sort(u.reshape(nf, T), dim=1).values.reshape(-1).contiguous()
            st = sp.ChebStats(dims, nf, max_bins=1024)
            nbytes = nf * T * 8
            row = {"dims": "%d^3" % n, "nfields": nf, "MB_in": round(nbytes * 1e-6, 1),
                   "wgs_summary": st.size(3), "wgs_hist": st.size(4)}
            out = torch.empty((nf, 9), dtype=torch.float64, device="cuda")
            put(row, "summary", dev_us(lambda: st.summary(u, out=out)), nbytes)
            lohi = torch.tensor([[-4.0, 4.0]] * nf, dtype=torch.float64, device="cuda")
            for nb in (64, 1024):
                ho = torch.empty((nf, 2, nb + 3), dtype=torch.float64, device="cuda")
                e = torch.linspace(-4.0, 4.0, nb + 1, dtype=torch.float64, device="cuda").repeat(nf, 1).contiguous()
                put(row, "hist%d_uniform" % nb, dev_us(lambda: st.histogram(u, nb, range=lohi, out=ho)), nbytes)
                put(row, "hist%d_edges" % nb, dev_us(lambda: st.histogram(u, nb, edges=e, out=ho)), nbytes)
                put(row, "hist%d_uniform_sorted" % nb, dev_us(lambda: st.histogram(us, nb, range=lohi, out=ho)), nbytes)
                put(row, "hist%d_uniform_cond" % nb, dev_us(lambda: st.histogram(u, nb, range=lohi, cond=us, out=ho)), 2 * nbytes)
            if nf == 3:
                co = torch.empty(2, dtype=torch.float64, device="cuda")
                put(row, "cfl", dev_us(lambda: st.cfl(u, out=co)), nbytes)
            if WHAT == "all":
                w = torch.from_numpy(sp.cc_weights(n)).cuda()
                W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).reshape(1, T).contiguous()
                uf = u.reshape(nf, T)

                def t_summary():                         # field by field: one (nf, T) call with dim=1 reductions takes 48 x the
                    r = []                               # time of one field for 3 fields, which is torch's reduction, not the work
                    for f in range(nf):
                        x = uf[f]
                        r += [x.min(), x.argmin(), x.max(), x.argmax(), torch.isnan(x).sum(), (W[0] * x).sum()]
                        x2 = x * x
                        r.append((W[0] * x2).sum())
                        x3 = x2 * x
                        r.append((W[0] * x3).sum())
                        r.append((W[0] * (x3 * x)).sum())
                    return r
                put(row, "torch_summary", dev_us(t_summary), nbytes, lib=False)
                Wf = W.expand(nf, T).reshape(-1).contiguous()
                offs = (torch.arange(nf, device="cuda") * (1024 + 3)).repeat_interleave(T)
                for nb in (64, 1024):
                    def t_hist():
                        t = (u + 4.0) * (nb / 8.0)
                        s = torch.where(u < -4.0, 0, torch.where(t >= nb, nb + 1, 1 + t.floor().clamp(0, nb - 1).long()))
                        return torch.bincount(s + offs, weights=Wf, minlength=nf * (1024 + 3))
                    put(row, "torch_bincount%d" % nb, dev_us(t_hist), nbytes, lib=False)
                    e1 = torch.linspace(-4.0, 4.0, nb + 1, dtype=torch.float64, device="cuda")

                    def t_edges():
                        s = torch.bucketize(u, e1, right=True)
                        return torch.bincount(s + offs, weights=Wf, minlength=nf * (1024 + 3))
                    put(row, "torch_bucketize_bincount%d" % nb, dev_us(t_edges), nbytes, lib=False)
                if nf == 3:
                    r = torch.from_numpy(sp.stats_rate(n)).cuda()
                    v = u.reshape(3, n, n, n)

                    def t_cfl():
                        return (v[0].abs() * r[:, None, None] + v[1].abs() * r[None, :, None] + v[2].abs() * r[None, None, :]).max()
                    put(row, "torch_cfl", dev_us(t_cfl), nbytes, lib=False)
            st.destroy()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
