#!/usr/bin/env python3
"""Timings tools/stokes_ab.py does not take: stokes_op_mult_vv_cm (k_st_local_cm3p / k_st_out_cm3p) at 128^3 and 64^3 on the power-law
state, and the 2-D callbacks (k_st_node_vv<2, true>, k_st_node_fn<2>) at 1024^2.  The timing loop of stokes_ab.py, three rounds, one
line per round; compares nothing: run it in a fresh process per build (CHEBHIP_LIB_PATH selects another build of the library), the
builds in turn (profiles/stokes_node/ab.txt).
usage: stokes_ab_extra.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
sp = ge.load()


def t(fn, reps=60):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


for dims in ((128, 128, 128), (64, 64, 64), (1024, 1024)):
    op = sp.StokesOp(dims); op.set_rheology(1, 1.0, 3.0, 1e-4, 1.0)
    op.set_dirichlet(np.zeros(op.dirichlet_size)); op.set_force(np.zeros(op.global_size))
    x = torch.randn(op.global_size, dtype=torch.float64, device="cuda"); y = torch.empty_like(x)
    xv = x[:op.velocity_size]; yv = y[:op.velocity_size]
    op.function(x, y)
    tag = "x".join(map(str, dims))
    for rnd in range(3):
        if len(dims) == 3:
            print("%s: MatMultVVcm %.1f us" % (tag, t(lambda: op.mult_vv_cm(xv, yv))), flush=True)
        else:
            print("%s: MatMult %.1f us  Function %.1f us" % (tag, t(lambda: op.mult(x, y)), t(lambda: op.function(x, y))), flush=True)
    op.destroy()
