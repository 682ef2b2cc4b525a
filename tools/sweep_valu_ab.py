#!/usr/bin/env python3
"""The constant-coefficient MatMult_Elliptic of the three-launch route with and without the multiply by alpha = -1 in its first
launch (option sweep_alpha_multiply; default: the sign rides in the recombination), alternating timed loops on ONE handle (the option
is read per call); results compared with the default's.  Under `rocprofv3 --kernel-trace --stats` the two first launches show up as
two kernels (template argument SG = 1 / 0).
usage: sweep_valu_ab.py [P [rounds [reps]]]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as ge
sp = ge.load()
P = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 200
NAMES = ("sweep_alpha_multiply",)
CASES = [("default", (0,)), ("multiply", (1,))]
def t(fn, reps):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps
op = sp.EllipticOp((P, P, P))
U = torch.randn(op.global_size, dtype=torch.float64, device="cuda")
V0, V = torch.empty_like(U), torch.empty_like(U)
op.mult(U, V0)
for _ in range(100): op.mult(U, V)
res = {c[0]: [] for c in CASES}
same = {}
try:
    for rnd in range(ROUNDS):
        for name, vals in CASES:
            for k, v in zip(NAMES, vals): sp.set_option(k, v)
            V.fill_(float("nan"))
            res[name].append(t(lambda: op.mult(U, V), REPS))
            same[name] = bool(torch.equal(V, V0))
finally:
    for k in NAMES: sp.set_option(k, 0)
for name, _ in CASES:
    r = sorted(res[name])
    print("P=%d %-16s median %8.2f us  min %8.2f  max %8.2f  (%d rounds of %d)  same values as default: %s" % (
        P, name, r[len(r) // 2], r[0], r[-1], ROUNDS, REPS, same[name]), flush=True)
op.destroy()
