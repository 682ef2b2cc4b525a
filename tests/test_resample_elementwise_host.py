"""The per-element bar of resample_ref.py on the host (no device): what a plain IEEE float64 chain gives passes it, in the
library's run order and in the reverse one, for every shape and input kind of test_gpu_resample.py; planted faults of the kinds a
line-product kernel or its driver can have fail it, the failing element named; the long-double restatements of the prolongations
reproduce a cubic state and notice two exchanged boundary values; the entries of cheb_resample_matrix_host are correct relative
to their own size."""
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import linewise as lw
import resample_ref as rr
import test_resample_host as trh

sp = ge.load()
SEED = 20261021
LD = np.longdouble
U = 2.0 ** -53


def setup(s, kind="noise", which=0):
    di, do, a, b, c = s
    Ms = rr.mats(tuple(di), tuple(do), a, b)
    order = rr.run_order(Ms)
    x = rr.inputs(kind, rr.stored(di, a) + (c,), SEED, order)[which]
    return Ms, order, x


# ---- float64 chains pass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", rr.ALL_SHAPES, ids=rr.shape_id)
def test_float64_chains_pass_in_either_order(s):
    """Worst ratios over all kinds and both orders measured here: 11.9 of cap 1030 ((1024)i -> (700)a, noise) and 5.4 of cap 28
    ((5, 20) -> (5, 70), 4 components, noise); every other shape stays below 5."""
    di, do, a, b, c = s
    Ms = rr.mats(tuple(di), tuple(do), a, b)
    order = rr.run_order(Ms)
    assert len(order) == sum(rr.runs(M) for M in Ms) >= 1
    for kind in rr.KINDS:
        for n, x in enumerate(rr.inputs(kind, rr.stored(di, a) + (c,), SEED, order)):
            t, B, cap = rr.truth_bound(x, di, do, a, b)
            assert cap == sum(Ms[k].shape[1] + 8 for k in order) and t.shape == rr.stored(do, b) + (c,)
            assert np.isfinite(B).all() and np.isfinite(t.astype(np.float64)).all()
            for o in (order, order[::-1]):
                r, _ = lw.check(rr.chain(Ms, x, o), t, B, cap, "%s %s%d order %s" % (rr.shape_id(s), kind, n, o))
            if kind == "constant":                              # the constant itself, not only the truth of the rounded rows
                lw.check(rr.chain(Ms, x, order), np.broadcast_to(x.reshape(-1, c)[0].astype(LD), t.shape), B, cap, "constant")
            print("%-34s %-12s %.3f of cap %d" % (rr.shape_id(s), kind + str(n), r, cap))


def test_run_order_is_the_ratio_order():
    """The five-direction chain runs its two shrinking directions first (most shrinking first), not in index order."""
    di, do, a, b, c = rr.SHAPES["chains"][-1]
    assert rr.run_order(rr.mats(di, do, a, b)) == [2, 0, 1, 3, 4]           # 4/8, 5/9, 7/4, 9/5, 11/6
    assert [g[0] for g in rr.geometry(rr.SHAPES["chains"][1])] == [0, 3, 1]     # (6,5,4,3) -> (7,9,4,5): direction 2 is skipped


def test_shapes_reach_every_template():
    """resample_launch's rule on the launches of the shapes: both tilings at both output tiles, LINES_A at every component count
    in a last direction and alone, the first COLFAST stride."""
    seen = {rr.route(*q[2:]) for s in rr.ALL_SHAPES for q in rr.geometry(s)}
    assert seen == {(True, 64), (True, 128), (False, 64), (False, 128)}
    assert {q[4] for s in rr.SHAPES["lines_a"] for q in rr.geometry(s)} == {1, 2, 3, 4}
    assert {(q[1], q[4]) for s in rr.SHAPES["components"] for q in rr.geometry(s)} == {(1, 2), (1, 3), (1, 4)}
    assert {q[4] for s in rr.SHAPES["colfast"] for q in rr.geometry(s)} == {5, 6, 15, 16, 17}
    assert len(rr.ALL_SHAPES) == 49 and len(set(rr.ALL_SHAPES)) == 49


def test_scaled_input_is_one_scale_per_line_of_the_direction_under_test():
    """One running direction: the exponent is constant along it and differs between neighbouring lines; the chains vary it along
    the direction that runs last and along every direction that does not run."""
    for s in rr.ALL_SHAPES:
        di, do, a, b, c = s
        order = rr.run_order(rr.mats(di, do, a, b))
        shape = rr.stored(di, a) + (c,)
        (x,) = rr.inputs("scaled", shape, SEED, order)
        e = np.round(np.log10(np.abs(x) / np.abs(rr.inputs("noise", shape, SEED)[0])))
        same = order[:-1] if len(order) > 1 else order                # the directions along which the scale must not change
        for k in same:
            assert (e == np.take(e, [0], axis=k)).all(), (s, k)
        scales = int(np.prod(shape)) // int(np.prod([shape[k] for k in same]))
        assert np.unique(e).size == min(scales, 201) and (scales == 1 or (e.min(), e.max()) == (-100, 100)), s


def test_impulse_combs_hit_every_column():
    for s in rr.ALL_SHAPES:
        di, _, a, _, c = s
        xs = rr.inputs("impulse", rr.stored(di, a) + (c,), 0)
        for k in range(len(di)):
            other = tuple(j for j in range(len(di) + 1) if j != k)
            assert (sum(x.sum(axis=other) for x in xs) > 0).all(), (s, k)


# ---- planted faults fail -------------------------------------------------------------------------------------------------------
def fails(y, t, B, cap, where=None):
    """The bar fails and names an element (one of `where` when given)."""
    with pytest.raises(AssertionError) as e:
        lw.check(y, t, B, cap, "planted")
    m = re.search(r"at \(([0-9, ]+)\)", str(e.value))
    assert m, str(e.value)
    idx = tuple(int(v) for v in m.group(1).replace(" ", "").rstrip(",").split(","))
    if where is not None:
        assert where(idx), (idx, str(e.value))
    return idx


def test_fault_matrix_entry_off():
    """One entry 1e-13 of its size off, a unit impulse under it: ~900 units of 2^-53 B against a cap of 25."""
    s = ((17,), (33,), "all", "all", 1)
    Ms, order, _ = setup(s)
    R = Ms[0].copy()
    i, j = 5, 7
    assert R[i, j] != 0.0 and R[i, j] != 1.0
    R[i, j] *= 1.0 + 1e-13
    x = np.zeros((17, 1)); x[j, 0] = 1.0
    t, B, cap = rr.truth_bound(x, *s[:4])
    lw.check(rr.chain(Ms, x), t, B, cap)
    assert fails(rr.chain([R], x), t, B, cap) == (i, 0)


def test_fault_transposed_matrix():
    """ALL(n) -> INTERIOR(n + 2): a square matrix that is not symmetric."""
    s = ((9, 6), (11, 8), "all", "interior", 2)
    Ms, order, x = setup(s)
    assert Ms[0].shape == (9, 9) and not np.array_equal(Ms[0], Ms[0].T) and rr.runs(Ms[0])
    t, B, cap = rr.truth_bound(x, *s[:4])
    lw.check(rr.chain(Ms, x, order), t, B, cap)
    fails(rr.chain([Ms[0].T.copy(), Ms[1]], x, order), t, B, cap)


def test_fault_components_swapped():
    s = ((7, 6), (9, 8), "all", "interior", 3)
    Ms, order, x = setup(s, "scaled")
    t, B, cap = rr.truth_bound(x, *s[:4])
    y = rr.chain(Ms, x, order)
    lw.check(y, t, B, cap)
    fails(y[..., [1, 0, 2]], t, B, cap, lambda idx: idx[-1] in (0, 1))


def test_fault_line_from_its_neighbour():
    s = ((7, 12, 9), (7, 17, 9), "all", "all", 1)
    Ms, order, x = setup(s)
    t, B, cap = rr.truth_bound(x, *s[:4])
    y = rr.chain(Ms, x, order)
    lw.check(y, t, B, cap)
    y[3, :, 4, 0] = y[3, :, 5, 0]
    fails(y, t, B, cap, lambda idx: idx[0] == 3 and idx[2] == 4)


LEAKS = [((7, 12, 9), (7, 17, 9), "all", "all", 1), ((8, 12, 8), (8, 17, 8), "all", "all", 1), ((5, 20), (5, 33), "all", "all", 2),
         ((5, 20), (5, 70), "all", "all", 2), ((12, 15), (17, 15), "all", "all", 1), ((12, 17), (17, 17), "all", "all", 1),
         ((1024,), (3,), "all", "all", 2), ((20,), (70,), "interior", "all", 4)]


@pytest.mark.parametrize("s", LEAKS, ids=rr.shape_id)
def test_fault_tiny_leak_between_lines(s):
    """1e-60 of the next output line (cyclically) added to every line: invisible in any norm, and on N(0, 1) data below the last
    bit.  The scaled input carries one scale per line, so some line has a neighbour 10^60 times its size or more (asserted) and
    fails the bar there by many orders of magnitude."""
    Ms, order, x = setup(s, "scaled")
    ((k, O, K, M, Q),) = rr.geometry(s)
    t, B, cap = rr.truth_bound(x, *s[:4])
    y = rr.chain(Ms, x, order)
    lw.check(y, t, B, cap)
    lines = np.moveaxis(y, k, 0).reshape(M, O * Q)
    size = np.abs(lines).max(axis=0)
    assert (np.roll(size, -1) >= 1e75 * size).any()
    leaky = np.moveaxis((lines + 1e-60 * np.roll(lines, -1, axis=1)).reshape(np.moveaxis(y, k, 0).shape), 0, k)
    fails(leaky, t, B, cap)
    (xn,) = rr.inputs("noise", x.shape, SEED)                     # the same leak under N(0, 1) data: not seen
    yn = np.moveaxis(rr.chain(Ms, xn, order), k, 0)
    lw.check(np.moveaxis(yn + 1e-60 * np.roll(yn.reshape(M, O * Q), -1, axis=1).reshape(yn.shape), 0, k), *rr.truth_bound(xn, *s[:4]))


def test_fault_tail_chunk_dropped():
    """Points 16 .. of a 17-point line of the last direction left out of the sum."""
    s = ((5, 17), (5, 33), "all", "all", 2)
    Ms, order, x = setup(s)
    t, B, cap = rr.truth_bound(x, *s[:4])
    lw.check(rr.chain(Ms, x, order), t, B, cap)
    R = Ms[1].copy(); R[:, 16:] = 0.0
    fails(rr.chain([Ms[0], R], x, order), t, B, cap)


def test_fault_identity_direction_run_inexactly():
    """A skipped direction run through a matrix with a 1 - 2^-52 diagonal stays inside the bar of the running directions (two
    units of 2^-53 against a cap of 37) -- it is the copy-bits checks that catch it: an equal-grid handle returns the input's
    bits, and a one-direction handle returns bits that do not depend on the other directions."""
    s = ((6, 5, 4, 3), (7, 9, 4, 5), "all", "all", 1)
    Ms, order, x = setup(s)
    assert not rr.runs(Ms[2]) and order == [0, 3, 1]
    t, B, cap = rr.truth_bound(x, *s[:4])
    bad = list(Ms); bad[2] = np.eye(4) * (1.0 - 2.0 ** -52)
    y = rr.chain(bad, x, [0, 3, 2, 1])
    lw.check(y, t, B, cap)                                        # the bar does not see it
    assert not np.array_equal(y, rr.chain(Ms, x, order))
    # equal grids: truth_bound says "no direction runs", and the check is on the bits
    t0, B0, cap0 = rr.truth_bound(x, s[0], s[0])
    assert cap0 == 0 and np.array_equal(t0.astype(np.float64), x)
    y0 = rr.chain([np.eye(n) * (1.0 - 2.0 ** -52) for n in s[0]], x)
    assert not np.array_equal(y0, x)
    fails(y0, t0, B0, cap0)                                       # (cap 0: the bar asks for the bits too)


# ---- prolongations -------------------------------------------------------------------------------------------------------------
ELLIPTIC = [((5, 4), (9, 7)), ((4, 5, 6), (7, 9, 8))]
STOKES = [((5, 4), (9, 7)), ((4, 5, 4), (7, 6, 9))]


def swap_two_boundary_values(dv, ncomp):
    """Two boundary nodes with different values exchanged."""
    v = np.array(dv, dtype=np.float64).reshape(-1, ncomp)
    a, b = 1, v.shape[0] - 2
    assert (v[a] != v[b]).all()
    v[[a, b]] = v[[b, a]]
    return v.ravel()


@pytest.mark.parametrize("dims_c,dims_f", ELLIPTIC)
def test_prolong_elliptic_restatement(dims_c, dims_f):
    x, dv, fine = rr.elliptic_polynomial(dims_c, dims_f)
    assert x.size == np.prod([n - 2 for n in dims_c]) and dv.size == np.prod(dims_c) - x.size
    t, B, cap = rr.prolong_elliptic(dims_c, x, dv, dims_f)
    assert cap == sum(n + 8 for n in dims_c)
    lw.check(fine, t, B, cap, "cubic")
    t2, _, _ = rr.prolong_elliptic(dims_c, x, swap_two_boundary_values(dv, 1), dims_f)
    fails(fine, t2, B, cap)


@pytest.mark.parametrize("dims_c,dims_f", STOKES)
def test_prolong_stokes_restatement(dims_c, dims_f):
    d = len(dims_c)
    x, dv, vfine, pfine = rr.stokes_polynomial(dims_c, dims_f)
    (tv, Bv, capv), (tp, Bp, capp) = rr.prolong_stokes(dims_c, x, dv, dims_f)
    assert capv == sum(n + 8 for n in dims_c) and capp == sum(n - 2 + 8 for n in dims_c) and tv.shape[-1] == d and tp.shape[-1] == 1
    lw.check(vfine, tv, Bv, capv, "velocity")
    lw.check(pfine, tp, Bp, capp, "pressure")
    (t2, _, _), (tp2, _, _) = rr.prolong_stokes(dims_c, x, swap_two_boundary_values(dv, d), dims_f)
    fails(vfine, t2, Bv, capv)
    assert np.array_equal(tp2, tp)                                # the pressure takes no boundary value
    # a state whose components are exchanged node by node is noticed too
    xs = x.reshape(-1, d + 1)[:, [1, 0] + list(range(2, d + 1))].ravel()
    fails(vfine, rr.prolong_stokes(dims_c, xs, dv, dims_f)[0][0], Bv, capv)


# ---- entries -------------------------------------------------------------------------------------------------------------------
ENTRY_C = 2.0 * 1.1184


def test_entries_relative_to_their_size():
    """|R - ref| <= c 2^-53 |ref| per entry over the CASES of test_resample_host.py, ref the independent long-double barycentric
    restatement there; exact zeros and ones stay exact.  The library forms the rows in long double and rounds once, so c = 1 up to
    the error of the two long-double computations (2^-11 of a double's each, times the row's own cancellation).  Measured here:
    worst c = 1.1184, in the row that extrapolates from 1022 interior nodes to x = -1 ((1024) INTERIOR -> (1024) ALL, entry
    (1023, 82)); asserted: twice that."""
    worst, at = 0.0, None
    for n_in, n_out, a, b in trh.CASES:
        R = sp.resample_matrix(n_in, n_out, a, b)
        ref = trh.reference(n_in, n_out, a, b)
        exact = (ref == 0) | (ref == 1)
        assert np.array_equal(R[exact], ref[exact].astype(np.float64)), (n_in, n_out, a, b)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(exact, 0.0, (np.abs(R.astype(LD) - ref) / (U * np.abs(ref))).astype(np.float64))
        if c.size and c.max() > worst:
            worst, at = float(c.max()), (n_in, n_out, a, b) + tuple(int(v) for v in np.unravel_index(int(c.argmax()), c.shape))
    print("worst c = %.4f at %s" % (worst, at))
    assert worst <= ENTRY_C, at
