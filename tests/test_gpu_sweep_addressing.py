"""The addressing of the long-line sweep kernel (csrc/sweep_vec.hip vec4_body, csrc/tile.h rsrc_at; run with -m gpu on the MI355X
box): every stream goes through a buffer descriptor that is re-based per tile -- base = array + tile origin, num_records = what is
left of the array from there -- and the per-lane offsets are constants of the launch.  What can go wrong is a window: a wrong
origin, a num_records that is too long (a neighbour's data read, a store past the end) or too short (zeros read, stores lost), the
lane mask of a row's last tile.  The shapes are the smallest at which those differ:
  line lengths 66 / 67 (the shortest the kernel takes), 128 / 129 / 130 (KS = 16 up to 128 points, KS = 32 from 129 on: DiffMat's
  choice, which launch_v4 follows) and 255 / 256; line counts that are no multiple of the 32 (KS = 32) / 64 (KS = 16) lines of a
  tile; rows of 66 .. 408 columns that end inside a tile and inside a 16-column sub-tile; odd extents and strides, which the
  library sends to the general kernel (the results must not depend on who runs them).
References: the CPU oracle at the suite's bar for white noise, ||y - ref|| / ||ref|| < 1e-10 (tests/test_gpu_parity.py), and for
the guard-band tests the same call on arrays of their own, bit for bit.  Every result array starts NaN- or sentinel-filled."""
import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import oracle_lib as orc
from conftest import relerr

pytestmark = pytest.mark.gpu
sp = ge.load()
TOL = 1e-10
SEED = 20261019
SENTINEL = -7.25e77          # what the output guards hold
GUARD = 64 * 256             # doubles of guard on each side: more than a tile of the longest lines (32 x 256)

# C-ordered extents; ChebPlan differentiates every direction of each
CHEB_SHAPES = [(66, 5, 67), (67, 66, 3), (130, 7, 33), (256, 3, 66), (5, 256, 31),
               (66, 6, 68), (128, 2, 130), (129, 34, 2), (4, 255, 70), (3, 130, 98)]
# stored (interior) extents of Lap1dPlan / EllipticOp: lines of K + 2 points with zero ends, K points stored
LAP_SHAPES = [(66, 6, 70), (130, 34), (3, 254, 66), (128, 129, 2)]


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


def noise(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


def takes_vec(shape, tr):
    """Whether lines along `tr` (more than 64 points) run the 16-byte kernels: sweep_vec_eligible's rule for aligned dense arrays --
    strided lines (16 or more values apart) need an even stride, contiguous ones an even length, strides of 2 .. 15 never do."""
    inner = int(np.prod(shape[tr + 1:], dtype=np.int64))
    return (inner % 2 == 0) if inner >= 16 else (inner == 1 and shape[tr] % 2 == 0)


def counts():
    L = sp.lib()
    torch.cuda.synchronize()
    return np.array([L.chebhip_launch_count(), L.chebhip_vec_launch_count()])


def carve(n, fill, where):
    """A view of n doubles inside a larger allocation filled with `fill`, at least GUARD doubles of it on each side.
    where = 0: the view starts right behind the front guard; 1: in the middle; 2: it ends right in front of the end guard -- always
    16 or 48 bytes past a 128-byte boundary.  Returns (view, whole allocation, offset)."""
    room = 3 * GUARD
    whole = torch.full((n + 2 * GUARD + room + 32,), fill, dtype=torch.float64, device="cuda")
    base = (-(whole.data_ptr() // 8)) % 16                 # doubles up to the next 128-byte boundary
    off = (base + GUARD + 2, base + GUARD + room // 2 + 6, base + GUARD + room - 14)[where]
    assert (whole.data_ptr() + 8 * off) % 128 in (16, 48) and off >= GUARD and off + n + GUARD <= whole.numel()
    return whole[off:off + n], whole, off


def guards_intact(whole, off, n, fill):
    g = torch.cat([whole[:off], whole[off + n:]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


@pytest.mark.parametrize("shape", CHEB_SHAPES, ids=sid)
def test_cheb_mult_every_direction(shape):
    """STORE: ChebPlan.mult along every direction against the oracle; lines of more than 64 points run the kernel that
    sweep_vec_eligible's rule says (chebhip_vec_launch_count), so a shape that silently moves to the general kernel fails here."""
    x = noise(shape, SEED)
    xd = dev(x).reshape(-1)
    for tr in range(len(shape)):
        plan = sp.ChebPlan(shape, tr)
        try:
            yd = torch.full_like(xd, float("nan"))
            c0 = counts()
            plan.mult(xd, yd)
            dc = counts() - c0
        finally:
            plan.destroy()
        if shape[tr] > 64:
            assert list(dc) == [1, int(takes_vec(shape, tr))], (shape, tr, list(dc))
        y = yd.cpu().numpy().reshape(shape)
        assert np.isfinite(y).all(), (shape, tr)
        e = relerr(y, orc.cheb_mult(x, tr, mode=orc.FAST))
        print("addressing cheb %s tr=%d relerr %.2e" % (sid(shape), tr, e))
        assert e < TOL, (shape, tr, e)
    assert torch.equal(xd.cpu(), torch.from_numpy(x.reshape(-1)))


@pytest.mark.parametrize("where", [0, 1, 2], ids=["front", "middle", "end"])
@pytest.mark.parametrize("shape", CHEB_SHAPES[:6], ids=sid)
def test_cheb_mult_between_guard_bands(shape, where):
    """STORE with the input between NaN guards and the result between sentinel guards, both carved out of larger allocations at
    starts that are 16-byte but not 128-byte aligned: finite, the bits of the run on arrays of their own, guards untouched."""
    x = noise(shape, SEED + 1)
    n = x.size
    xd = dev(x).reshape(-1)
    xg, xwhole, xoff = carve(n, float("nan"), where)
    xg.copy_(xd)
    for tr in range(len(shape)):
        plan = sp.ChebPlan(shape, tr)
        try:
            y0 = torch.full_like(xd, float("nan"))
            plan.mult(xd, y0)
            yg, ywhole, yoff = carve(n, SENTINEL, where)
            c0 = counts()
            plan.mult(xg, yg)
            dc = counts() - c0
        finally:
            plan.destroy()
        if shape[tr] > 64:
            assert list(dc) == [1, int(takes_vec(shape, tr))], (shape, tr, list(dc))
        assert bool(torch.isfinite(yg).all()), (shape, tr)
        assert torch.equal(yg, y0), (shape, tr, "guarded and unguarded runs differ")
        assert guards_intact(ywhole, yoff, n, SENTINEL), (shape, tr, "stored into the guard")
    assert guards_intact(xwhole, xoff, n, float("nan")) and torch.equal(xg, xd)


@pytest.mark.parametrize("where", [0, 1, 2], ids=["front", "middle", "end"])
@pytest.mark.parametrize("shape", LAP_SHAPES, ids=sid)
def test_lap1d_store_and_acc_between_guard_bands(shape, where):
    """Lap1dPlan.apply, y = alpha L x (STORE; alpha = -1 is the sign-only store) and y = acc + alpha L x (ACC), every direction:
    input and operand between NaN guards, result between sentinel guards, against the run on arrays of their own bit for bit;
    that run against the oracle's second derivative of the zero-ended lines."""
    d = len(shape)
    x = noise(shape, SEED + 2)
    a = noise(shape, SEED + 3)
    n = x.size
    xd, ad = dev(x).reshape(-1), dev(a).reshape(-1)
    xg, xwhole, xoff = carve(n, float("nan"), where)
    ag, awhole, aoff = carve(n, float("nan"), where)
    xg.copy_(xd); ag.copy_(ad)
    for axis in range(d):
        # the oracle: D D of the lines with their zero ends, interior rows
        pad = [(0, 0)] * d
        pad[axis] = (1, 1)
        xp = np.pad(x, pad)
        ref = orc.cheb_mult(orc.cheb_mult(xp, axis, mode=orc.FAST), axis, mode=orc.FAST)
        ref = np.take(ref, np.arange(1, shape[axis] + 1), axis=axis)
        plan = sp.Lap1dPlan(shape, axis)
        try:
            for alpha, with_acc in ((-1.0, False), (0.37, False), (-1.0, True)):
                y0 = torch.full_like(xd, float("nan"))
                plan.apply(xd, y0, ad if with_acc else None, alpha)
                yg, ywhole, yoff = carve(n, SENTINEL, where)
                plan.apply(xg, yg, ag if with_acc else None, alpha)
                torch.cuda.synchronize()
                what = (sid(shape), axis, alpha, with_acc)
                assert bool(torch.isfinite(yg).all()), what
                assert torch.equal(yg, y0), what + ("guarded and unguarded runs differ",)
                assert guards_intact(ywhole, yoff, n, SENTINEL), what + ("stored into the guard",)
                if where == 0:
                    want = alpha * ref + (a if with_acc else 0.0)
                    e = relerr(y0.cpu().numpy().reshape(shape), want)
                    print("addressing lap1d %s axis=%d alpha=%g acc=%d relerr %.2e" % (what + (e,)))
                    assert e < TOL, what + (e,)
        finally:
            plan.destroy()
    assert guards_intact(xwhole, xoff, n, float("nan")) and guards_intact(awhole, aoff, n, float("nan"))
    assert torch.equal(xg, xd) and torch.equal(ag, ad)


# poisson_launches: 2 = a launch per direction (STORE, ACC, ACC into the padded accumulator W, the last one into V); 3 = two STORE
# jobs into the padded W, W2 and an ACC2 launch, where the first two directions have one KS (else the chain of 2); 0 = the library's
# own choice.  Sweep launches expected (None: not pinned down here).  (68, 70, 134): ACC2 on contiguous lines of 132 points, KS = 32
# (one operand set, ONEBUF); (134, 132, 70): ACC2 at KS = 16; (70, 132, 68): KS = 16 / 32 / 16, the chain at every setting;
# (68, 67, 66): an odd line length and a last direction of 64 points, which is not the long-line kernel's.
ELL_LAUNCHES = {((68, 70, 134), 2): 3, ((68, 70, 134), 3): 2, ((134, 132, 70), 2): 3, ((134, 132, 70), 3): 2,
                ((70, 132, 68), 0): 3, ((70, 132, 68), 2): 3, ((70, 132, 68), 3): 3, ((132, 68), 2): 2}


@pytest.mark.parametrize("pl", [0, 2, 3])
@pytest.mark.parametrize("dims", [(68, 67, 66), (70, 132, 68), (132, 68), (68, 70, 134), (134, 132, 70)], ids=sid)
def test_elliptic_mult_modes_between_guard_bands(dims, pl):
    """EllipticOp.mult at gamma = 0 (V = -sum_k L_k U: STORE, ACC and ACC2 launches, the accumulator W with rows padded to 128
    bytes) on non-cubic grids, U between NaN guards and V between sentinel guards, against the oracle and against the run on
    arrays of their own."""
    shape = tuple(k - 2 for k in dims)
    U = noise(shape, SEED + 4).reshape(-1)
    n = U.size
    Ud = dev(U)
    ref = orc.elliptic_mult(dims, U, mode=orc.FAST)
    with option(poisson_launches=pl):
        op = sp.EllipticOp(dims)
        try:
            assert op.global_size == n
            V0 = torch.full_like(Ud, float("nan"))
            c0 = counts()
            op.mult(Ud, V0)
            nl, nv = counts() - c0
            e = relerr(V0.cpu().numpy(), ref)
            print("addressing elliptic %s pl=%d: %d sweep launches, %d of the 16-byte kernels, relerr %.2e" % (sid(dims), pl, nl, nv, e))
            assert bool(torch.isfinite(V0).all()) and e < TOL, (dims, pl, e)
            if (dims, pl) in ELL_LAUNCHES:
                assert nl == ELL_LAUNCHES[(dims, pl)], (dims, pl, nl)
            if min(shape) > 64:                      # every direction is the long-line kernel's: none may fall to the general kernel
                assert nv == nl, (dims, pl, nl, nv)
            for where in (0, 2):
                Ug, Uwhole, Uoff = carve(n, float("nan"), where)
                Ug.copy_(Ud)
                Vg, Vwhole, Voff = carve(n, SENTINEL, where)
                c0 = counts()
                op.mult(Ug, Vg)
                assert list(counts() - c0) == [nl, nv], (dims, pl, where)
                assert torch.equal(Vg, V0), (dims, pl, where, "guarded and unguarded runs differ")
                assert guards_intact(Vwhole, Voff, n, SENTINEL) and guards_intact(Uwhole, Uoff, n, float("nan")), (dims, pl, where)
        finally:
            op.destroy()
    assert sp.get_option("poisson_launches") == 0


def test_cheb_batch_above_the_old_size_limit():
    """A batch of 256-point lines of just above 0x38000000 bytes, where the 32-bit offsets of a whole-array descriptor ended and
    the general kernel used to take over: the re-based descriptors have no such limit.  Compared with the oracle on sub-blocks of
    whole lines at the start, in the middle and at the very end (tests/test_gpu_parity.py
    test_cheb_arrays_around_the_buffer_offset_limit).  That the 16-byte kernel ran is read from chebhip_vec_launch_count (the two
    kernels give the same bits, so the result cannot tell); with option general_kernels = 1 the count stands still."""
    nl = 0x38000000 // (8 * 256) + 96            # 458848 lines: 939.7 MB
    assert 8 * nl * 256 > 0x38000000
    g = torch.Generator(device="cuda").manual_seed(SEED)
    xd = torch.randn((nl, 256), dtype=torch.float64, device="cuda", generator=g)
    yd = torch.full_like(xd, float("nan"))
    L = sp.lib()
    plan = sp.ChebPlan((nl, 256), 1)
    try:
        torch.cuda.synchronize(); c0, v0 = L.chebhip_launch_count(), L.chebhip_vec_launch_count()
        plan.mult(xd.view(-1), yd.view(-1))
        torch.cuda.synchronize()
        assert L.chebhip_launch_count() - c0 == 1
        assert L.chebhip_vec_launch_count() - v0 == 1, "an array above 0x38000000 bytes still runs the general kernel"
        assert bool(torch.isfinite(yd).all())
        for lo, hi in ((0, 96), (nl // 2 - 31, nl // 2 + 33), (nl - 96, nl)):
            ref = orc.cheb_mult(xd[lo:hi].cpu().numpy(), 1, mode=orc.FAST)
            e = relerr(yd[lo:hi].cpu().numpy(), ref)
            print("addressing big batch lines %d..%d relerr %.2e" % (lo, hi, e))
            assert e < TOL, (lo, e)
        with option(general_kernels=1):
            yg = torch.full_like(xd, float("nan"))
            plan.mult(xd.view(-1), yg.view(-1))
            torch.cuda.synchronize()
        assert L.chebhip_vec_launch_count() - v0 == 1 and L.chebhip_launch_count() - c0 == 2
        assert float((yg - yd).norm() / yd.norm()) < 1e-13
    finally:
        plan.destroy()
    assert sp.get_option("general_kernels") == 0
    del xd, yd, yg
    torch.cuda.empty_cache()
