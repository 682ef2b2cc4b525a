"""The line-by-line, element-by-element bar of tests/linewise.py, checked on the CPU: its matrices against independent ones,
plain double products through it, and planted faults that it must catch and the normwise bar (relerr < 1e-10) must miss.

Measured on the CPU (worst |y - truth| / (2^-53 B) over all input kinds): plain double product 0.3 .. 17 (D) and 0.5 .. 20 (L),
even / odd product 0.2 .. 12 (D) and 0.2 .. 16 (L), for P = 5 .. 513 against caps P + 8 = 13 .. 521 and P + 6;
orc.cheb_mult_truth on impulses 0.9 .. 4.5; orc.cheb_mult(FAST) at P = 256: about 2 700 (cap 264)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import linewise as lw
import oracle_lib as orc
from conftest import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SEED = 20240229
KINDS = sorted(lw.GENERATORS)


def test_dense_D_is_antisymmetric_and_differentiates_polynomials():
    """Written from the mathematics: D is centro-antisymmetric to the bit, annihilates constants and maps x to 1, x^2 to 2x
    (degree < P is exact) at long-double rounding level of the componentwise weight."""
    for P in (2, 3, 4, 5, 17, 64, 129, 256, 513):
        D = lw.dense_D(P)
        assert D.dtype == np.longdouble and D.shape == (P, P)
        assert np.array_equal(D, -D[::-1, ::-1])
        x = np.cos(lw.PI_L * np.arange(P) / (P - 1))
        A = np.abs(D)
        for f, df in ((np.ones_like(x), 0 * x), (x, np.ones_like(x)), (x * x, 2 * x)):
            if P == 2 and f is not x and df[0] != 0:
                continue
            err = np.abs(np.dot(D, f) - df)
            assert np.all(err <= (P + 8) * 2.0 ** -63 * np.dot(A, np.abs(f))), P


@pytest.mark.parametrize("P", [2, 3, 4, 5, 16, 17, 33, 64, 65, 129, 130, 255, 256])
def test_dense_D_vs_oracle_truth_on_impulses(P):
    """Every column of D as the long-double transform chain of the oracle gives it (orc.cheb_mult_truth on the identity), to the
    cap of linewise.py.  The centre entry of an odd extent is exactly zero by antisymmetry (B = 0 there); the transform chain
    leaves long-double rounding noise in it, bounded separately by (P + 8) 2^-64 of the largest entry of D."""
    D = lw.dense_D(P)
    x = np.eye(P)
    y = orc.cheb_mult_truth(x, 1)                    # line l = e_l: y[l, :] = column l of D
    t, B = lw.truth(D, x, 1), lw.bound(D, x, 1)
    assert np.array_equal(t, D.T)
    if P & 1:
        c = P // 2
        assert B[c, c] == 0.0 and D[c, c] == 0
        assert abs(y[c, c]) <= (P + 8) * 2.0 ** -64 * float(np.abs(D).max())
        y[c, c] = 0.0
    r, idx = lw.check(y, t, B, P + 8, "cheb_mult_truth P=%d" % P)
    print("linewise-host truth-vs-oracle P=%d ratio %.2f at %s" % (P, r, idx))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_dense_D_vs_library_host_matrix(tmp_path):
    """diffmat_dense_host (csrc/diffmat.cpp, the matrix every kernel's fragments are cut from) is not exported by the ABI: a small
    host build prints it.  Both matrices are roundings to double of long-double values with relative errors of a few 2^-64, so
    they agree to 1 ulp of the entry (2 allowed); exact zeros agree exactly."""
    csrc = os.path.join(ROOT, "spectral-petsc_amd", "csrc")
    objs = []
    for src, extra in ((os.path.join(csrc, "diffmat.cpp"), ["-x", "hip"]), (os.path.join(csrc, "options.cpp"), ["-x", "hip"]),
                       (os.path.join(ROOT, "tests", "host", "dense_check.cpp"), [])):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", csrc] + extra + ["-c", src, "-o", o], check=True, timeout=600)
        objs.append(o)
    exe = str(tmp_path / "dense_check")
    subprocess.run([HIPCC] + objs + ["-o", exe], check=True, timeout=600)
    sizes = [2, 3, 4, 5, 17, 64, 65, 129, 256, 257, 513]
    out = subprocess.run([exe] + [str(p) for p in sizes], check=True, capture_output=True, text=True, timeout=600).stdout.split()
    k = 0
    for P in sizes:
        assert int(out[k]) == P
        lib = np.array([float.fromhex(v) for v in out[k + 1:k + 1 + P * P]]).reshape(P, P)
        k += 1 + P * P
        mine = lw.dense_D(P).astype(np.float64)
        assert np.array_equal(lib == 0, mine == 0), P
        ulps = np.abs(lib - mine) / np.spacing(np.abs(mine))
        assert ulps.max() <= 2, (P, ulps.max(), np.unravel_index(np.argmax(ulps), ulps.shape))
    assert k == len(out)


@pytest.mark.parametrize("P", [3, 4, 5, 10, 33, 34, 130, 256, 258])
def test_dense_L_vs_helmholtz_line(P):
    """dense_L against the matrix cheb_helmholtz_line_host decomposes, -S diag(lam) S^-1.  test_helmholtz_host.py states that
    decomposition's accuracy as ||A S - S lam|| <= 1e-12 ||A|| ||S|| and ||S S^-1 - I|| <= 1e-12, hence
    ||S lam S^-1 - A|| <= 1e-12 ||A|| (||S|| ||S^-1|| + 1)."""
    ge.build()
    sp = ge.load()
    S, Si, lam = sp.helmholtz_line(P)
    L = lw.dense_L(P)
    assert L.dtype == np.longdouble and L.shape == (P - 2, P - 2)
    assert np.abs(L - L[::-1, ::-1]).max() <= P * 2.0 ** -63 * np.abs(L).max()     # centro-symmetric to long-double rounding
    A = -(L.astype(np.float64))
    err = np.linalg.norm((S * lam) @ Si - A, 2)
    assert err <= 1e-12 * np.linalg.norm(A, 2) * (np.linalg.norm(S, 2) * np.linalg.norm(Si, 2) + 1), err


def test_dense_L_vs_50_digit_product():
    """The long-double product D D cancels (sum_k |D_ik||D_kj| is up to 500 times |L_ij| + |L_i,m-j| at P = 66, 7 700 times at
    P = 256), so the truth's own error is not negligible by itself: against 50-digit arithmetic dense_L is within 2 x 2^-53 of
    |L_ij| + |L_i,m-j| at P = 66 (measured 0.4; 8.2 at P = 256, 3 % of the cap there) -- which needs every entry of D right to
    long-double rounding, i.e. the folded sine arguments."""
    mp = pytest.importorskip("mpmath")
    P, n = 66, 65
    with mp.workdps(50):
        x = [mp.cos(mp.pi * i / n) for i in range(P)]
        D = mp.matrix(P, P)
        for i in range(P):
            for j in range(P):
                if i != j:
                    D[i, j] = mp.mpf((2 if i in (0, n) else 1) * (-1) ** (i + j)) / (2 if j in (0, n) else 1) / (x[i] - x[j])
                else:
                    D[i, j] = -x[i] / (2 * (1 - x[i] ** 2)) if 0 < i < n else mp.mpf((2 * n * n + 1) * (1 if i == 0 else -1)) / 6
        Lm = (D * D)[1:n, 1:n]
        Lt = np.array([[np.longdouble(mp.nstr(Lm[i, j], 25)) for j in range(P - 2)] for i in range(P - 2)])
        Dt = np.array([[np.longdouble(mp.nstr(D[i, j], 25)) for j in range(P)] for i in range(P)])
    Dl = lw.dense_D(P)
    # per entry: pi a / 2n (two roundings, passed on by sin with a factor t cot t <= 1), sin to 1 ulp, twice; product, quotient
    assert np.all(np.abs(Dl - Dt) <= 16 * 2.0 ** -64 * np.abs(Dt))
    A = np.abs(Lt)
    r = np.abs(lw.dense_L(P) - Lt) / (lw.U53 * (A + A[:, ::-1]))
    print("linewise-host dense_L P=66 vs 50 digits: %.2f x 2^-53 (|L_ij| + |L_i,m-j|)" % float(r.max()))
    assert r.max() <= 2


@pytest.mark.parametrize("P", [5, 33, 64, 130, 256, 513])
def test_double_products_pass_the_cap(P):
    """What any IEEE double implementation gives: a plain dense product and the even / odd split product of the kernels, D and
    L, every input kind -- all under the derived cap, so the cap rejects no correct route."""
    D, L = lw.dense_D(P), lw.dense_L(P)
    shape = (2 * P + 3, P)
    for kind in KINDS:
        x = lw.GENERATORS[kind](shape, 1, SEED + P)
        for name, M, xs, sym in (("D", D, x, 0), ("L", L, np.ascontiguousarray(x[:, :P - 2]), 1)):
            K = M.shape[0]
            t, B = lw.truth(M, xs, 1), lw.bound(M, xs, 1)
            r1, _ = lw.check(lw.product_double(M, xs, 1), t, B, K + 8, "dense %s P=%d %s" % (name, P, kind))
            r2, _ = lw.check(lw.product_evenodd(M, xs, 1, sym), t, B, K + 8, "even/odd %s P=%d %s" % (name, P, kind))
            print("linewise-host %s P=%d %-11s dense %.2f even/odd %.2f (cap %d)" % (name, P, kind, r1, r2, K + 8))


def test_generators():
    shape, axis = (5, 12, 7), 1
    x = lw.impulse(shape, axis)
    assert x.sum() == 35 and np.all(x.sum(axis=axis) == 1)
    l = np.arange(35).reshape(5, 7)
    assert np.array_equal(np.argmax(x, axis=axis), l % 12)
    s = lw.scaled(shape, axis, 3)
    e = lw.scale_exponents(shape, axis, 3)
    assert e.min() >= -100 and e.max() <= 100 and e.shape == (5, 1, 7)
    assert np.array_equal(s, lw.noise(shape, axis, 3) * 10.0 ** e)
    z = lw.sparse_lines(shape, axis, 3)
    nz = np.flatnonzero(np.abs(z).sum(axis=axis).reshape(-1))
    assert list(nz) == lw.sparse_positions(35, 3) and 0 in nz and 34 in nz and 31 in nz and 32 in nz
    a = lw.alternating(shape, axis, 3)
    assert np.array_equal(a[:, 1:], -a[:, :-1])
    c = lw.constant(shape, axis, 3)
    assert np.array_equal(c, np.broadcast_to(c[:, :1], shape))


# ----------------------------------------------------------------------------------------------
# planted faults: caught by the new bar, missed by the normwise one
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube():
    shape, axis = (64, 64, 64), 1
    D = lw.dense_D(64)
    x = lw.noise(shape, axis, SEED)
    t, B = lw.truth(D, x, axis), lw.bound(D, x, axis)
    y = lw.product_evenodd(D, x, axis, 0)
    assert lw.worst(y, t, B)[0] <= 72
    return D, x, y, t, B


CAP64 = 64 + 8


def test_fault_one_middle_row_element(cube):
    """(a) one middle-row element of one line changed by 1e-9 relative.  The element is chosen with |y_i| at least its row's
    r.m.s.: one that is small by cancellation hides behind its own B_i, rightly."""
    D, x, y, t, B = cube
    row = 31
    rms = np.sqrt(np.mean(y[:, row, :] ** 2))
    a, c = [int(v[0]) for v in np.nonzero(np.abs(y[:, row, :]) >= rms)]
    bad = y.copy()
    bad[a, row, c] *= 1 + 1e-9
    assert relerr(bad, t.astype(np.float64)) < 1e-10
    r, k = lw.worst(bad, t, B)
    assert r > CAP64 and np.unravel_index(k, y.shape) == (a, row, c)
    with pytest.raises(AssertionError, match=r"\(%d, %d, %d\)" % (a, row, c)):
        lw.check(bad, t, B, CAP64, "planted")


def test_fault_one_line_scaled(cube):
    """(b) one whole line multiplied by 1 + 1e-9: a line that has lost a third of its digits moves relerr by about 2e-11."""
    D, x, y, t, B = cube
    bad = y.copy()
    bad[40, :, 17] *= 1 + 1e-9
    assert relerr(bad, t.astype(np.float64)) < 1e-10
    r, k = lw.worst(bad, t, B)
    idx = np.unravel_index(k, y.shape)
    assert r > CAP64 and (idx[0], idx[2]) == (40, 17)


def test_fault_one_matrix_entry(cube):
    """(c) entry D[i, i+1] of one middle row perturbed by 1e-10 relative before the product.  The two next-to-diagonal entries are the
    largest of a middle row (about n / pi = 20 each; the rest fall off like 1 / |i - j|), so that the change,
    1e-10 |D_i,i+1| |x_i+1|, exceeds the cap of 72 x 2^-53 B_i = 8e-15 B_i on the lines where |x_i+1| is not small; the same
    perturbation of a far entry (|D_ij| about 1) would stay near the cap."""
    D, x, y, t, B = cube
    Dp = D.copy()
    i = 30
    assert abs(Dp[i, i + 1]) >= 0.99 * np.abs(Dp[i]).max()
    Dp[i, i + 1] *= np.longdouble(1 + 1e-10)
    bad = lw.product_evenodd(Dp, x, 1, 0)
    assert relerr(bad, t.astype(np.float64)) < 1e-10
    r, k = lw.worst(bad, t, B)
    assert r > CAP64 and np.unravel_index(k, y.shape)[1] in (i, 63 - i)


def test_fault_tiny_line_zeroed():
    """(d) the output of one line of the `scaled` input with s = -100 replaced by zeros: invisible in any norm over the array."""
    shape, axis = (64, 64, 64), 1
    D = lw.dense_D(64)
    x = lw.scaled(shape, axis, SEED)
    e = lw.scale_exponents(shape, axis, SEED)
    a, c = [int(v[0]) for v in np.nonzero(e[:, 0, :] == -100)]
    t, B = lw.truth(D, x, axis), lw.bound(D, x, axis)
    y = lw.product_evenodd(D, x, axis, 0)
    assert lw.worst(y, t, B)[0] <= CAP64
    bad = y.copy()
    bad[a, :, c] = 0.0
    assert relerr(bad, t.astype(np.float64)) < 1e-10
    r, k = lw.worst(bad, t, B)
    idx = np.unravel_index(k, y.shape)
    assert r > CAP64 and (idx[0], idx[2]) == (a, c)


def test_fault_fft_recipe_is_not_the_reference():
    """(e) the oracle's FAST mode (the reference's FFT recipe in double) at P = 256 exceeds the cap by itself -- its componentwise
    error is far larger than a matrix product's, which is why the long-double dense product is the reference here -- while
    passing the normwise bar."""
    D = lw.dense_D(256)
    x = lw.noise((40, 256), 1, SEED)
    t, B = lw.truth(D, x, 1), lw.bound(D, x, 1)
    y = orc.cheb_mult(x, 1, orc.FAST)
    assert relerr(y, t.astype(np.float64)) < 1e-10
    r, _ = lw.worst(y, t, B)
    print("linewise-host ORC_FAST P=256 ratio %.0f (cap 264)" % r)
    assert r > 256 + 8


def test_zero_bound_demands_exact_zero():
    y, t, B = np.zeros(4), np.zeros(4, dtype=np.longdouble), np.zeros(4)
    assert lw.worst(y, t, B)[0] == 0.0
    y[2] = 5e-324
    assert lw.worst(y, t, B) == (np.inf, 2)
    y[2] = np.nan
    assert lw.worst(y, t, B + 1.0) == (np.inf, 2)


# ----------------------------------------------------------------------------------------------
# subsets and the two truths at full size
# ----------------------------------------------------------------------------------------------
FULL = [((256, 256, 256), 0), ((256, 256, 256), 1), ((256, 256, 256), 2), ((128, 128, 128), 0), ((128, 128, 128), 1), ((128, 128, 128), 2)]


@pytest.mark.parametrize("shape,axis", FULL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "tr%d" % v)
def test_line_subset_coverage(shape, axis):
    L = lw.nlines(shape, axis)
    lines = lw.line_subset(shape, axis, SEED)
    assert np.array_equal(lines, np.unique(lines)) and lines[0] == 0 and lines[-1] == L - 1
    frac, res = lw.subset_coverage(lines, L)
    assert frac >= 0.02 and res == 128
    assert set(range(128)) <= set(lines.tolist()) and set(range(L - 128, L)) <= set(lines.tolist())
    rest = [s for k, s in enumerate(shape) if k != axis]
    idx = np.unravel_index(lines, rest)
    for a, s in enumerate(rest):
        for v in (0, 1, s - 2, s - 1):                         # first two and last two values of every non-transform index
            assert np.count_nonzero(idx[a] == v) >= 4
        counts = np.bincount(idx[a], minlength=s)               # one full interior plane per non-transform axis
        assert counts[1:-1].max() == L // s
    assert frac <= 0.12                                         # a subset, not the array


def test_plane_subset():
    for n0 in (126, 254, 64, 16):
        p = lw.plane_subset(n0, SEED)
        assert {0, 1, n0 - 2, n0 - 1} <= set(p.tolist()) and len(p) == 6 and p.min() == 0 and p.max() == n0 - 1


def test_subset_truth_equals_whole_truth_and_the_oracle_truth():
    """truth(lines=...) is the whole-array truth on those lines, and orc.cheb_mult_truth (C, long double transform chain) agrees
    with the dense long-double product under the cap on a noise input of every axis: either may serve at full size."""
    shape = (9, 64, 11)
    D = lw.dense_D(64)
    x = lw.scaled(shape, 1, SEED)
    whole, Bw = lw.truth(D, x, 1), lw.bound(D, x, 1)
    lines = np.array([0, 5, 11, 98])
    assert np.array_equal(lw.truth(D, x, 1, lines), lw.take_lines(whole, 1, lines))
    assert np.allclose(lw.bound(D, x, 1, lines), lw.take_lines(Bw, 1, lines), rtol=1e-14, atol=0)
    for axis, P in ((0, 130), (1, 64), (2, 256)):
        shape = [6, 5, 7]
        shape[axis] = P
        x = lw.noise(shape, axis, SEED)
        r, idx = lw.check(orc.cheb_mult_truth(x, axis), lw.truth(lw.dense_D(P), x, axis), lw.bound(lw.dense_D(P), x, axis), P + 8, "truth")
        print("linewise-host cheb_mult_truth noise P=%d ratio %.2f" % (P, r))


def test_elliptic_truth_sign_and_planes():
    """truth = -sum_k L_k U: the sign and the layout against orc.elliptic_mult (transforms in long double), and the plane subset
    against the whole array."""
    dims = (12, 9, 10)
    G = int(np.prod([p - 2 for p in dims]))
    U = lw.noise((G,), 0, SEED)
    t, B, fac = lw.elliptic_truth_bound(dims, U)
    assert fac == 10 + 7 + 8 + 24 + 3
    ref = orc.elliptic_mult(dims, U, mode=orc.DIRECT)
    assert relerr(t.astype(np.float64).ravel(), ref) < 1e-13
    planes = np.array([0, 1, 4, 8, 9])
    tp, Bp, _ = lw.elliptic_truth_bound(dims, U, planes)
    assert np.abs(tp - t[planes]).max() <= 2.0 ** -60 * np.abs(t).max()
    assert np.allclose(Bp, B[planes], rtol=1e-13, atol=0)
