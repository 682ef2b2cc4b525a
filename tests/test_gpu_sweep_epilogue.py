"""The epilogue of the long-line sweep kernel (csrc/sweep_vec.hip vec4_body; run with -m gpu on the MI355X box): the lane exchange
as one DPP-carrying select per dword and the sign-only store of alpha = -1.  (The descending tile walk and the `nt` result stores
of the same proposal did not pay and were taken out again -- DESIGN_history.md -- so there is no switch left to force them with.)

Shapes are STORED extents (lines of K + 2 points with implicit zero ends), the smallest that reach every path of the epilogue:
  (130, 66, 70)    KS = 32 / 16 / 16, strided and contiguous lines, 70 = 64 + 6: a partial last column block; 70 / 2 = 35 is odd, so the
                   contiguous direction folds its middle pair (y_ie, y_{n-ie}) into one 16-byte piece
  (67, 130, 131)   odd extents: the self-paired middle point of a strided line of 67; an odd stride and an odd contiguous extent, which
                   the library sends to the general kernel (the results must not depend on who runs them)
  (66, 66, 66)     fewer tiles than compute units
  (136, 200)       2-D, KS = 32 twice
Every result array starts NaN-filled.  Elementwise bar against the long-double truth: tests/linewise.py, |y - truth| <= (K + 8)
2^-53 B (+ |acc|), on the whole lines of linewise.line_subset (Lap1dPlan) / on six planes (EllipticOp).  Between the settings of the
option that must not change a value (sweep_alpha_multiply) whole results are compared with torch.equal.
Measured on an MI355X: 74 figures, worst 7.18 (caps 72 .. 355); the file takes 3.5 s."""
import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import linewise as lw

pytestmark = pytest.mark.gpu
sp = ge.load()
SEED = 20241019
LD = np.longdouble

SHAPES = [(130, 66, 70), (67, 130, 131), (66, 66, 66), (136, 200)]
ALPHAS = (1.0, -1.0, 0.37)


def sid(shape):
    return "x".join(map(str, shape))


class option:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: sp.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            sp.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            sp.set_option(k, v)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def launches(fn):
    L = sp.lib()
    torch.cuda.synchronize()
    before = L.chebhip_launch_count()
    out = fn()
    torch.cuda.synchronize()
    return out, L.chebhip_launch_count() - before


@pytest.mark.parametrize("shape,axis", [(s, a) for s in SHAPES for a in range(len(s))], ids=lambda v: sid(v) if isinstance(v, tuple) else "ax%d" % v)
def test_lap1d_alpha(shape, axis):
    """y = alpha L x (STORE) and y = acc + alpha L x (ACC) for alpha = 1, -1, 0.37: alpha = -1 without acc is the launch that carries the
    sign in its recombination; with option sweep_alpha_multiply = 1 it multiplies as the others do, and the two agree exactly."""
    K = shape[axis]
    M = lw.dense_L(K + 2)
    x = lw.noise(shape, axis, SEED)
    acc = lw.noise(shape, axis, SEED + 5)
    lines = lw.line_subset(shape, axis, SEED)
    t, B = lw.truth(M, x, axis, lines), lw.bound(M, x, axis, lines)
    al = lw.take_lines(acc, axis, lines)
    xd, ad = dev(x).reshape(-1), dev(acc).reshape(-1)
    plan = sp.Lap1dPlan(shape, axis)
    try:
        def run(alpha, with_acc):
            yd = torch.full_like(xd, float("nan"))
            _, n = launches(lambda: plan.apply(xd, yd, ad if with_acc else None, alpha))
            assert n == 1
            return yd

        for alpha in ALPHAS:
            for with_acc in (False, True):
                yd = run(alpha, with_acc)
                what = "Lap1dPlan %s axis=%d alpha=%g %s" % (sid(shape), axis, alpha, "acc" if with_acc else "store")
                tt = LD(alpha) * t + (al.astype(LD) if with_acc else 0)
                BB = abs(alpha) * B + (np.abs(al) if with_acc else 0)
                y = lw.take_lines(yd.cpu().numpy().reshape(shape), axis, lines)
                r, idx = lw.check(y, tt, BB, K + 8, what)
                print("epilogue-ratio %s %.2f at %s cap %d" % (what, r, idx, K + 8))
                if alpha == -1.0:
                    with option(sweep_alpha_multiply=1):
                        assert torch.equal(run(alpha, with_acc), yd), what + ": sweep_alpha_multiply changes the result"
        assert torch.equal(xd.cpu(), torch.from_numpy(x.reshape(-1))) and torch.equal(ad.cpu(), torch.from_numpy(acc.reshape(-1)))
    finally:
        plan.destroy()
    assert sp.get_option("sweep_alpha_multiply") == 0


# poisson_launches = 2: a launch per direction (STORE, ACC, ACC).  3 asks for two launches (two STORE jobs, then ACC2), which ell_op_mult
# grants from 6 M unknowns on; below, directions with one KS and even strides share ONE launch of d STORE jobs (+ the sum pass) and the
# others keep the per-direction chain.  (ACC2 itself: test_gpu_linewise.py::test_elliptic_mult_groupings at 128^3, 208^3, 256^3.)
LAUNCHES_PL3 = {(130, 66, 70): 3, (67, 130, 131): 3, (66, 66, 66): 1, (136, 200): 1}


@pytest.mark.parametrize("pl", [2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_elliptic_mult_epilogue_switches(shape, pl):
    """EllipticOp.mult, V = -sum_k L_k U, against the long-double truth; then the same apply with the multiply kept in the STORE
    launches (sweep_alpha_multiply = 1): the same values."""
    d = len(shape)
    dims = tuple(k + 2 for k in shape)
    nlaunch = d if pl == 2 else LAUNCHES_PL3[shape]
    U = lw.noise(shape, d - 1, SEED + 1)
    planes = lw.plane_subset(shape[0], SEED)
    t, B, fac = lw.elliptic_truth_bound(dims, U, planes)
    Ud = dev(U).reshape(-1)
    with option(poisson_launches=pl):
        op = sp.EllipticOp(dims)
        try:
            def run():
                Vd = torch.full_like(Ud, float("nan"))
                _, n = launches(lambda: op.mult(Ud, Vd))
                assert n == nlaunch, "%s pl=%d: %d sweep launches, %d expected" % (sid(shape), pl, n, nlaunch)
                return Vd

            V0 = run()
            what = "EllipticOp %s pl=%d" % (sid(shape), pl)
            r, idx = lw.check(V0.cpu().numpy().reshape(shape)[planes], t, B, fac, what)
            print("epilogue-ratio %s %.2f at %s cap %d" % (what, r, idx, fac))
            with option(sweep_alpha_multiply=1):
                assert torch.equal(run(), V0), what + ": sweep_alpha_multiply changes the result"
            assert torch.equal(Ud.cpu(), torch.from_numpy(U.reshape(-1)))
        finally:
            op.destroy()
    assert [sp.get_option(k) for k in ("poisson_launches", "sweep_alpha_multiply")] == [0, 0]
