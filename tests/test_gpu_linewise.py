"""Every route of the sweep kernels, element by element and line by line (run with -m gpu on the MI355X box), against the dense
long-double product of tests/linewise.py.  The bar, for EVERY checked element:

    |y_i - truth_i| <= (K + 8) 2^-53 B_i,   B_i = 1/2 sum_j (|M_ij| + |M_i,m-j|) (|x_j| + |x_m-j|)  (+ |acc_i|)

(derivation: linewise.py; K = points of the line).  B_i = 0 demands an exact zero.  Inputs: noise, per-line scaled noise
(10^-100 .. 10^100), impulses (every matrix entry, twice), alternating / constant lines, mostly-zero arrays; and the isolation
runs: lines replaced by NaN / +Inf must leave every other line bit-identical and come out non-finite in every row.

Which kernel a shape runs is decided by the library (csrc/sweep.hip sweep_launch, sweep_vec.hip sweep_vec_eligible,
sweep_xl.hip sweep_xl_eligible, chebhip.hip ell_op_mult); the ABI reports only launch counts.  Each test restates the rule that
sends its shapes to the intended kernel (`vec_rule`), asserts it on its shapes, sets the documented option where a route is
forced, and asserts the launch count.

Worst ratios measured on an MI355X (profiles/linewise/ratios.txt holds one line per test id and input kind):
  test_cheb_vec_strided                        96 figures, worst   9.3 (cap  264) at [256] alternating (1, 255, 10)
  test_cheb_contiguous                         96 figures, worst   9.3 (cap  264) at [256] alternating (44, 255)
  test_cheb_general_kernel_by_option           42 figures, worst   7.7 (cap  264) at [jfast-256] noise (120, 255)
  test_cheb_general_kernel_by_shape            21 figures, worst   6.6 (cap  264) at [9x256x35-tr1] scaled (4, 0, 34)
  test_cheb_general_kernel_by_alignment        12 figures, worst   7.1 (cap  264) at [5x256x34-tr1] noise (1, 0, 20)
  test_cheb_line_counts_and_ranks              32 figures, worst   5.5 (cap  264) at [2x256x30-tr1] noise (0, 255, 1)
  test_cheb_xl_kernel                          36 figures, worst  15.6 (cap 1032) at [colfast-1024] noise (0, 1023, 10)
  test_cheb_xl_kernel_large_tiles               4 figures, worst  11.9 (cap  520) at [512x16400-tr0] scaled (row 0, line 16308)
  test_cheb_valu_kernel                         9 figures, worst  21.1 (cap 1033) at [1025x18-tr0] scaled (0, 9)
  test_cheb_rocblas_long_lines                 12 figures, worst  21.1 (cap 1033) at [1025x18-tr0] scaled (0, 9)
  test_cheb_rocblas_force_gemm                 12 figures, worst   9.6 (cap  264) at [37x256-tr1] scaled (20, 0)
  test_cheb_full_size                          12 figures, worst  10.9 (cap  264) at [256-0] scaled (row 0, line 11371)
  test_lap1d_shapes_of_the_parity_test         72 figures, worst  10.1 (cap  262) at [5x254x20-ax1] noise/alias (4, 218, 5)
  test_lap1d_extents                          216 figures, worst  10.3 (cap  260) at [jfast-252] scaled/alias (281, 247)
  test_lap1d_general_kernel_by_option          54 figures, worst   8.6 (cap  262) at [colfast-254] scaled/store (10, 28, 27)
  test_elliptic_mult_groupings                 45 figures, worst  11.2 (cap  469) at [66x128x254-pl2] noise (35, 83, 0)
Before the fix of csrc/diffmat.cpp that these tests led to (sine arguments folded into [0, pi/2]) the impulse input gave 453 (cap
262) through Lap1dPlan at 252 / 254 stored points and 463 (cap 469) through EllipticOp.mult at 66 x 128 x 254: entries of L off by
5e-14 of their size.  Now the impulse figures of L are at most 4.7.
The file takes 57 s on the GPU box; the whole -m gpu suite with it 333 s (269 s were recorded for the suite of round 6).
"""

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import linewise as lw

pytestmark = pytest.mark.gpu
sp = ge.load()
SEED = 20240229
KINDS3 = ("noise", "scaled", "impulse")
KINDS6 = ("noise", "scaled", "impulse", "alternating", "constant", "sparse")
_NODE = [""]
_CACHE = {}


@pytest.fixture(autouse=True)
def _nodeid(request):
    _NODE[0] = request.node.nodeid.split("::", 1)[-1]
    yield


def record(kind, r, idx, cap):
    print("linewise-ratio %s %s %.2f at %s cap %d" % (_NODE[0], kind, r, idx, cap))


def launches(fn):
    L = sp.lib()
    torch.cuda.synchronize()
    before = L.chebhip_launch_count()
    out = fn()
    torch.cuda.synchronize()
    return out, L.chebhip_launch_count() - before


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


def ks_of(K):
    """k-steps of the register-resident kernels for lines of K points (csrc/diffmat.cpp): 4, 8, 16, 32 for K <= 32, 64, 128, 256."""
    ks = 4
    while 4 * ks < (K + 1) // 2:
        ks *= 2
    return ks


def tile_lines(K):
    """Lines per tile of sweep.hip / sweep_vec.hip: 128, 64, 64, 32 for KS = 4, 8, 16, 32."""
    return {4: 128, 8: 64, 16: 64, 32: 32}[ks_of(K)]


def vec_rule(K, inner, aligned16=True):
    """sweep_vec_eligible for a plain dense sweep: strided lines (inner >= 16) need an even stride, contiguous lines an even
    number of points, any other small stride stays with the general kernel; every array 16-byte aligned."""
    if not aligned16 or K > 256:
        return False
    return (inner == 1 and K % 2 == 0) if inner < 16 else inner % 2 == 0


def inner_of(shape, tr):
    return int(np.prod(shape[tr + 1:], dtype=np.int64))


def dev(a, off8=False):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not off8:
        t = torch.from_numpy(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    v = buf[1:].view(a.shape)
    assert v.data_ptr() % 16 == 8
    v.copy_(torch.from_numpy(a))
    return v


def out_like(xd, off8=False):
    if not off8:
        return torch.full_like(xd, float("nan"))
    buf = torch.full((xd.numel() + 1,), float("nan"), dtype=torch.float64, device="cuda")
    return buf[1:].view(xd.shape)


def reference(mat, P, shape, axis, kind, seed=SEED, lines=None):
    """(x, truth, B) for matrix `mat` ('D': dense_D(P) on lines of P points, 'L': dense_L(P) on lines of P - 2), computed once per
    shape and input kind.  lines: subset of whole lines -> truth, B are (K, len(lines))."""
    key = (mat, P, tuple(shape), axis, kind, seed, None if lines is None else (len(lines), int(lines.sum())))
    if key not in _CACHE:
        M = lw.dense_D(P) if mat == "D" else lw.dense_L(P)
        x = lw.GENERATORS[kind](tuple(shape), axis, seed)
        if kind == "impulse" and lines is None:
            t, B = lw.impulse_truth_bound(M, tuple(shape), axis, seed)
        else:
            t, B = lw.truth(M, x, axis, lines), lw.bound(M, x, axis, lines)
        cache_put(key, (x, t, B))
    return _CACHE[key]


def cache_put(key, value):
    """Truth arrays are computed once per shape and input kind; the oldest entries leave when the cache holds 16."""
    while len(_CACHE) >= 16:
        _CACHE.pop(next(iter(_CACHE)))
    _CACHE[key] = value


def poison_positions(shape, axis, K):
    """Flat line indices (C order of the other indices) for the isolation runs: first line, last line of the array, last line
    of a full tile, first line of the ragged tail, the line next to a padded lane (the last real line of a ragged tile)."""
    L = lw.nlines(shape, axis)
    inner = inner_of(shape, axis)
    nt = tile_lines(K) if K <= 256 else 16
    pos = {0, L - 1}
    if inner >= 16:                                   # tiles are (outer block, nt neighbouring columns)
        if inner > nt:
            pos.update({nt - 1, nt, inner - 1, L - inner + nt})
        else:
            pos.update({inner - 1, min(inner, L - 1)})
    elif L > nt:
        pos.update({nt - 1, nt, (L - 1) // nt * nt})
    return sorted(pos)


def isolation(run, x, axis, what):
    """run(x) -> y (numpy).  Lines at poison_positions replaced by NaN, then by +Inf: bystanders bit-identical, poisoned lines
    non-finite in every row."""
    K = x.shape[axis]
    pos = poison_positions(x.shape, axis, K)
    clean = run(x)
    assert np.isfinite(clean).all(), what
    cm = np.moveaxis(clean, axis, 0).reshape(K, -1)
    by = np.ones(cm.shape[1], dtype=bool)
    by[pos] = False
    for val in (float("nan"), float("inf")):
        xp = np.moveaxis(x.copy(), axis, 0).reshape(K, -1)
        xp[:, pos] = val
        xp = np.ascontiguousarray(np.moveaxis(xp.reshape(np.moveaxis(x, axis, 0).shape), 0, axis))
        ym = np.moveaxis(run(xp), axis, 0).reshape(K, -1)
        same = (ym[:, by].view(np.int64) == cm[:, by].view(np.int64)).all(axis=0)
        assert same.all(), "%s: bystander line %d differs after poisoning lines %s with %r" % (what, int(np.flatnonzero(by)[np.argmin(same)]), pos, val)
        fin = np.isfinite(ym[:, pos])
        assert not fin.any(), "%s: poisoned line %d is finite in row %d (%r)" % (what, pos[int(np.nonzero(fin)[1][0])], int(np.nonzero(fin)[0][0]), val)


# ----------------------------------------------------------------------------------------------
# ChebPlan.mult
# ----------------------------------------------------------------------------------------------
def cheb_run(shape, tr, off8=False, expect_launches=1):
    def run(x):
        plan = sp.ChebPlan(shape, tr)
        try:
            xd = dev(x, off8)
            yd = out_like(xd, off8)
            _, n = launches(lambda: plan.mult(xd.view(-1), yd.view(-1)))
            assert n == expect_launches
            assert torch.equal(xd.cpu(), torch.from_numpy(np.ascontiguousarray(x))) or not np.isfinite(x).all()
            return yd.cpu().numpy()
        finally:
            plan.destroy()
    return run


def cheb_check(shape, tr, kinds, off8=False, iso=True):
    P = shape[tr]
    run = cheb_run(shape, tr, off8)
    for kind in kinds:
        x, t, B = reference("D", P, shape, tr, kind)
        r, idx = lw.check(run(x), t, B, P + 8, "ChebPlan %s tr=%d %s" % ("x".join(map(str, shape)), tr, kind))
        record(kind, r, idx, P + 8)
    if iso:
        isolation(run, reference("D", P, shape, tr, "noise")[0], tr, "ChebPlan %s tr=%d" % ("x".join(map(str, shape)), tr))


def strided_shape(P):
    """(A, P, W): strided lines, W = tile + 2 neighbouring lines per outer block (a full tile and a ragged one of two lines), at
    least 2 P lines in all."""
    W = tile_lines(P) + 2
    return (-(-2 * P // W) + 1, P, W)


def contiguous_shape(P):
    """(L, P): contiguous lines, L = at least 2 P and one more than a multiple of the tile."""
    nt = tile_lines(P)
    return (-(-2 * P // nt) * nt + 1, P)


PS = [2, 3, 4, 5, 16, 17, 32, 33, 64, 65, 66, 128, 129, 130, 255, 256]


@pytest.mark.parametrize("P", PS)
def test_cheb_vec_strided(P):
    """16-byte kernels (sweep_vec.hip), COLFAST tiling: lines of stride W >= 16, W even (sweep_vec_eligible: `!jfast && (inner & 1)`
    rejects odd strides), arrays from the caching allocator (16-byte aligned).  W = tile + 2: every outer block has a full tile and a
    ragged one.  Extents on both sides of every KS step (32 | 33, 64 | 65, 128 | 129) and of the MFMA k-step of 4."""
    shape = strided_shape(P)
    assert vec_rule(P, inner_of(shape, 1)) and shape[0] * shape[2] >= 2 * P
    cheb_check(shape, 1, KINDS6)


@pytest.mark.parametrize("P", PS)
def test_cheb_contiguous(P):
    """Contiguous lines (JFAST tiling), one more line than a multiple of the tile.  Even P: 16-byte kernels (sweep_vec_eligible:
    `jfast && (inner != 1 || (P & 1))`); odd P fails that rule by itself and runs the general 8-byte kernel of sweep.hip."""
    shape = contiguous_shape(P)
    assert vec_rule(P, 1) == (P % 2 == 0) and shape[0] >= 2 * P and shape[0] % tile_lines(P) == 1
    cheb_check(shape, 1, KINDS6)


@pytest.mark.parametrize("P", [4, 5, 33, 64, 65, 130, 256])
@pytest.mark.parametrize("tiling", ["colfast", "jfast"])
def test_cheb_general_kernel_by_option(P, tiling):
    """Option general_kernels = 1 (sweep_launch: `!opt(OPT_GENERAL_KERNELS) && sweep_vec_eligible`): the general 8-byte kernel,
    KS = 4 (P = 4, 5), 8 (33, 64), 16 (65), 32 (130, and the 256-point instantiation), both tilings (inner >= 16 / inner < 16)."""
    shape = strided_shape(P) if tiling == "colfast" else contiguous_shape(P)
    assert (inner_of(shape, 1) >= 16) == (tiling == "colfast")
    with option(general_kernels=1):
        assert sp.get_option("general_kernels") == 1
        cheb_check(shape, 1, KINDS3)
    assert sp.get_option("general_kernels") == 0


@pytest.mark.parametrize("shape,tr", [((3, 16, 17), 1), ((3, 66, 131), 1), ((9, 256, 35), 1), ((40, 17, 3), 1), ((70, 128, 3), 1), ((11, 64, 2, 7), 1),
                                      ((9, 130, 15), 1)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "tr%d" % v)
def test_cheb_general_kernel_by_shape(shape, tr):
    """Shapes that fail the 16-byte rules by themselves: odd strides >= 16 (COLFAST), strides of 2 .. 15 (JFAST tiling of the
    general kernel with strided points; the 16-byte JFAST kernel takes contiguous lines only)."""
    assert not vec_rule(shape[tr], inner_of(shape, tr))
    cheb_check(shape, tr, KINDS3)


@pytest.mark.parametrize("shape,tr", [((70, 32), 1), ((3, 32, 130), 1), ((40, 256), 1), ((5, 256, 34), 1)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "tr%d" % v)
def test_cheb_general_kernel_by_alignment(shape, tr):
    """An 8-byte-aligned view x[1:] of a bigger allocation (input and output): sweep_vec_eligible's `al(p.in0) && al(p.out)` fails,
    the general kernel runs shapes the 16-byte kernels would otherwise take."""
    assert vec_rule(shape[tr], inner_of(shape, tr)) and not vec_rule(shape[tr], inner_of(shape, tr), aligned16=False)
    cheb_check(shape, tr, KINDS3, off8=True)


@pytest.mark.parametrize("shape,tr", [((64,), 0), ((256,), 0), ((33,), 0), ((127, 4), 1), ((63, 66), 1), ((31, 256), 1), ((2, 64, 62), 1), ((2, 256, 30), 1),
                                      ((3, 4, 5, 6, 16), 4), ((66, 2, 3, 2, 4), 0), ((2, 3, 130, 2, 8), 2), ((2, 3, 32, 16), 2), ((128, 6, 6), 0),
                                      ((5, 6, 7), 0), ((5, 6, 7), 1), ((5, 6, 7), 2)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "tr%d" % v)
def test_cheb_line_counts_and_ranks(shape, tr):
    """Line counts off the tile (one line, tile - 1, tile - 2 neighbouring strided lines) and rank 1 to 5 with the transform
    dimension first, in the middle and last; whichever kernel sweep_launch picks by the rules above."""
    cheb_check(shape, tr, ("noise", "scaled"))


@pytest.mark.parametrize("P", [257, 258, 512, 513, 1000, 1024])
@pytest.mark.parametrize("tiling", ["colfast", "jfast"])
def test_cheb_xl_kernel(P, tiling):
    """cheb_sweep_xl_kernel (sweep_xl_eligible: 256 < P <= 1024, plain input, contiguous lines or strides >= 16): tiles of 16 lines
    at these sizes (fewer than 512 workgroups), ragged last tile in both tilings."""
    shape = (-(-2 * P // 18) + 1, P, 18) if tiling == "colfast" else (2 * P + 3, P)
    small = (3, P, 18) if tiling == "colfast" else (35, P)
    assert sp.get_option("long_lines_gemm") == 0 and inner_of(shape, 1) in (1, 18) and lw.nlines(shape, 1) >= 2 * P
    cheb_check(shape, 1, ("impulse",), iso=False)             # every entry twice: needs 2 P lines
    cheb_check(small, 1, ("noise", "scaled"))


@pytest.mark.parametrize("shape,tr", [((512, 16400), 0), ((16400, 512), 1)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "tr%d" % v)
def test_cheb_xl_kernel_large_tiles(shape, tr):
    """Arrays large enough for the long-line kernel's tiles of 32 lines with two m-tiles per wave (sweep_xl_launch: at least 512
    workgroups), ragged last tile (16400 = 512 * 32 + 16); checked on a subset of whole lines (8.4 M elements)."""
    subset_check(shape, tr, ("noise", "scaled"))


@pytest.mark.parametrize("shape,tr", [((1025, 18), 0), ((7, 1100), 1), ((5, 1100, 3), 1)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "tr%d" % v)
def test_cheb_valu_kernel(shape, tr):
    """Lines beyond 1024 points: cheb_sweep_long_kernel (FP64 VALU, dense D^T streamed; sweep_launch -> launch_long, no option
    set so no vendor GEMM).  A dense product without the even / odd split: P terms, cap P + 8."""
    assert sp.get_option("vendor_gemm") == 0 and sp.get_option("long_lines_gemm") == 0 and sp.get_option("force_gemm") == 0
    cheb_check(shape, tr, KINDS3)


@pytest.mark.parametrize("shape,tr", [((300, 40), 0), ((12, 513), 1), ((1025, 18), 0), ((7, 1100), 1)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "tr%d" % v)
def test_cheb_rocblas_long_lines(shape, tr):
    """Option long_lines_gemm = 1: launch_long_gemm hands plain sweeps of long lines to rocBLAS DGEMM (strided batched), both
    layouts (contiguous lines: one GEMM; strided lines: one per outer block).  A GEMM without the split has P terms: cap P + 8.
    The ABI cannot tell rocBLAS from the VALU kernel launch_long falls back to when the library cannot be loaded (both count one
    launch); a kernel trace of this test and the next (profiles/linewise/gemm_routes_kernel_trace.txt) shows 48 Tensile DGEMM
    dispatches for their 48 applies and no sweep kernel.  Beyond 1024 points the figures coincide with the VALU kernel's."""
    with option(long_lines_gemm=1):
        cheb_check(shape, tr, KINDS3)
    assert sp.get_option("long_lines_gemm") == 0


@pytest.mark.parametrize("shape,tr", [((37, 4), 1), ((3, 64, 18), 1), ((37, 256), 1), ((3, 255, 18), 1)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "tr%d" % v)
def test_cheb_rocblas_force_gemm(shape, tr):
    """Option force_gemm = 1, read when the plan is created (diffmat_create): extents of 4 .. 256 points get the dense matrix of the
    long lines (KS = 0) and go to rocBLAS."""
    with option(force_gemm=1):
        cheb_check(shape, tr, KINDS3)
    assert sp.get_option("force_gemm") == 0


def subset_check(shape, tr, kinds, seed=SEED):
    """A full-size array on a subset of whole lines (linewise.line_subset); the two coverage conditions are asserted first."""
    P = shape[tr]
    L = lw.nlines(shape, tr)
    lines = lw.line_subset(shape, tr, seed)
    frac, res = lw.subset_coverage(lines, L)
    assert frac >= 0.02 and res == 128, (frac, res)
    run = cheb_run(shape, tr)
    for kind in kinds:
        x, t, B = reference("D", P, shape, tr, kind, seed, lines)
        y = lw.take_lines(run(x), tr, lines)
        r, (row, k) = lw.check(y, t, B, P + 8, "ChebPlan %s tr=%d %s (rows x subset lines)" % ("x".join(map(str, shape)), tr, kind))
        record(kind, r, "(row %d, line %d)" % (row, int(lines[k])), P + 8)


@pytest.mark.parametrize("tr", [0, 1, 2])
@pytest.mark.parametrize("n", [128, 256])
def test_cheb_full_size(n, tr):
    """The BASELINE sizes, every transform dimension, noise and per-line scaled noise, on at least 2 % of the lines covering every
    residue of the line index modulo 128 (16-byte kernels: even strides / even P, aligned arrays)."""
    shape = (n, n, n)
    assert vec_rule(n, inner_of(shape, tr))
    subset_check(shape, tr, ("noise", "scaled"))


# ----------------------------------------------------------------------------------------------
# Lap1dPlan.apply: y = acc + alpha L x, sym = 1
# ----------------------------------------------------------------------------------------------
def lap_run(shape, axis, mode, acc):
    def run(x):
        plan = sp.Lap1dPlan(shape, axis)
        try:
            xd = dev(x).reshape(-1)
            if mode == "store":
                yd = torch.full_like(xd, float("nan"))
                _, n = launches(lambda: plan.apply(xd, yd, None, 1.0))
            elif mode == "acc":
                yd = torch.full_like(xd, float("nan"))
                ad = dev(acc).reshape(-1)
                _, n = launches(lambda: plan.apply(xd, yd, ad, -1.0))
                assert torch.equal(ad.cpu(), torch.from_numpy(acc.reshape(-1)))
            else:
                yd = dev(acc).reshape(-1)
                _, n = launches(lambda: plan.apply(xd, yd, yd, -1.0))
            assert n == 1
            return yd.cpu().numpy().reshape(shape)
        finally:
            plan.destroy()
    return run


def lap_check(shape, axis, kinds=KINDS3, iso=True):
    K = shape[axis]
    P = K + 2
    what = "Lap1dPlan %s axis=%d" % ("x".join(map(str, shape)), axis)
    for kind in kinds:
        x, t, B = reference("L", P, shape, axis, kind)
        acc = lw.noise(shape, axis, SEED + 5)
        if kind == "scaled":
            acc = acc * 10.0 ** lw.scale_exponents(shape, axis, SEED)
        for mode in ("store", "acc", "alias"):
            y = lap_run(shape, axis, mode, acc)(x)
            tt, BB = (t, B) if mode == "store" else (acc.astype(np.longdouble) - t, B + np.abs(acc))
            r, idx = lw.check(y, tt, BB, K + 8, "%s %s %s" % (what, kind, mode))
            record(kind + "/" + mode, r, idx, K + 8)
    if iso:
        x = reference("L", P, shape, axis, "noise")[0]
        acc = lw.noise(shape, axis, SEED + 5)
        isolation(lap_run(shape, axis, "store", None), x, axis, what + " store")
        isolation(lap_run(shape, axis, "acc", acc), x, axis, what + " acc")


@pytest.mark.parametrize("shape,axis", [((30, 18, 14), 0), ((30, 18, 14), 1), ((30, 18, 14), 2), ((7, 62), 1), ((126, 40, 33), 0), ((5, 254, 20), 1),
                                        ((6, 10, 254), 2), ((4, 5, 6, 3), 2)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "ax%d" % v)
def test_lap1d_shapes_of_the_parity_test(shape, axis):
    """The shapes of test_gpu_parity.py::test_lap1d_vs_oracle: acc = None, acc given with alpha = -1, acc aliasing the output."""
    lap_check(shape, axis)


@pytest.mark.parametrize("K", [2, 3, 4, 5, 64, 65, 66, 67, 128, 130, 252, 254])
@pytest.mark.parametrize("tiling", ["colfast", "jfast"])
def test_lap1d_extents(K, tiling):
    """Stored extents K (lines of P = K + 2 points with implicit zero ends) on both sides of the KS steps: full extents 4, 5, 66,
    67, 130, 254, 256 and stored extents 4, 5, 66, 67, 130, 254; strided lines (16-byte kernel, even stride) and contiguous lines
    (16-byte kernel for even K, general kernel for odd K).  258 points are beyond the interior-layout plans
    (test_lap1d_rejects_more_than_256_points)."""
    shape = strided_shape(K) if tiling == "colfast" else contiguous_shape(K)
    assert vec_rule(K, inner_of(shape, 1)) == (tiling == "colfast" or K % 2 == 0)
    lap_check(shape, 1)


@pytest.mark.parametrize("K", [5, 66, 254])
@pytest.mark.parametrize("tiling", ["colfast", "jfast"])
def test_lap1d_general_kernel_by_option(K, tiling):
    """The centro-symmetric matrix (sym = 1: mirror rows a - b) and the OUT_ACC store of the general kernel (general_kernels = 1)."""
    shape = strided_shape(K) if tiling == "colfast" else contiguous_shape(K)
    with option(general_kernels=1):
        lap_check(shape, 1)
    assert sp.get_option("general_kernels") == 0


@pytest.mark.parametrize("K", [255, 256, 258])
def test_lap1d_rejects_more_than_256_points(K):
    """cheb_plan_create_trimmed: lines of K + 2 > 256 points are an error, not another route."""
    with pytest.raises(sp.ChebhipError):
        sp.Lap1dPlan((4, K), 1)


# ----------------------------------------------------------------------------------------------
# EllipticOp.mult at eta = 1: V = -sum_k L_k U
# ----------------------------------------------------------------------------------------------
ELL = [
    # dims, poisson_launches, sweep launches, grouping
    ((20, 18, 18), 0, 1, "d-job launch + sum"),            # interior 18 x 16 x 16: one KS, strides 256 / 16 / 1, even last extent
    ((36, 40, 66), 0, 1, "d-job launch + sum"),            # interior 34 x 38 x 64: KS = 8 in every direction
    ((136, 200), 0, 1, "d-job launch + sum"),              # 2-D, KS = 32 twice
    ((128, 128, 128), 1, 1, "d-job launch + sum"),         # forced: the three-job route at a size that takes two launches by default
    ((128, 128, 128), 0, 2, "two jobs + OUT_ACC2"),        # 1.5 M <= G < 6 M, lines of at most 128 points
    ((128, 128, 128), 2, 3, "launch per direction"),       # forced; padded rows (126 interior points: > 64, even)
    ((130, 98, 128), 0, 2, "two jobs + OUT_ACC2"),         # G = 128 * 96 * 126 = 1.55 M, KS = 16 in every direction
    ((132, 134, 76), 0, 2, "two launches, padded rows"),   # KS = 32, 32, 16: no three-job launch; interior > 64, even: padded accumulator
    ((208, 208, 208), 0, 2, "two launches, padded rows"),  # G = 8.7 M >= 6 M, padded field 8.8 M <= 9 M values
    ((256, 256, 256), 0, 3, "launch per direction"),       # padded field 16.5 M > 9 M values
    ((256, 256, 256), 3, 2, "two launches, padded rows"),  # forced at a size beyond the limit
    ((66, 128, 254), 2, 3, "launch per direction"),        # forced, dense rows (64 interior points: no padded accumulator)
    ((20, 18, 16), 0, 3, "launch per direction"),          # stride 14 of direction 1 is neither >= 16 nor 1: no shared launch
    ((33, 70, 9), 0, 3, "launch per direction"),           # KS = 4, 16, 4 and odd extents
    ((8, 7, 6, 5), 0, 4, "launch per direction"),          # d = 4: the d-job forms exist for d = 2, 3
]


@pytest.mark.parametrize("dims,pl,nlaunch,grouping", ELL, ids=["%s-pl%d" % ("x".join(map(str, e[0])), e[1]) for e in ELL])
def test_elliptic_mult_groupings(dims, pl, nlaunch, grouping):
    """MatMult_Elliptic with constant coefficients, one shape per launch grouping of ell_op_mult (option text of poisson_launches
    in include/chebhip.h; the table above says which rule sends each shape where) with the sweep-launch count as evidence.
    truth = -sum_k L_k U in long double; bound: sum_k B_k with the factor sum_k (K_k + 8) + d.  Arrays of more than 4 M unknowns
    are checked on six whole planes of the outermost index (first two, last two, two seeded ones)."""
    d = len(dims)
    kd = [p - 2 for p in dims]
    G = int(np.prod(kd))
    planes = lw.plane_subset(kd[0], SEED) if G > 4_000_000 else None
    key = ("ell", dims)
    with option(poisson_launches=pl):
        op = sp.EllipticOp(dims)
        try:
            assert op.global_size == G
            for kind in KINDS3:
                ck = key + (kind,)
                if ck not in _CACHE:
                    U = lw.GENERATORS[kind](tuple(kd), d - 1, SEED)
                    cache_put(ck, (U,) + lw.elliptic_truth_bound(dims, U, planes))
                U, t, B, fac = _CACHE[ck]
                Ud = dev(U).reshape(-1)
                Vd = torch.full_like(Ud, float("nan"))
                op.mult(Ud, Vd)
                _, n = launches(lambda: op.mult(Ud, Vd))
                assert n == nlaunch, "%s: %d sweep launches, %d expected for '%s'" % (dims, n, nlaunch, grouping)
                V = Vd.cpu().numpy().reshape(kd)
                if planes is not None:
                    V = V[planes]
                r, idx = lw.check(V, t, B, fac, "EllipticOp %s pl=%d %s" % ("x".join(map(str, dims)), pl, kind))
                if planes is not None:
                    idx = (int(planes[idx[0]]),) + idx[1:]
                record(kind, r, idx, fac)
        finally:
            op.destroy()
    assert sp.get_option("poisson_launches") == 0
