"""cheb_resample_apply on the device (Resample): the tensor product of the host interpolation matrices, exact copies of equal
grids, polynomial reproduction, round trips, unaligned tensors and stream ordering -- normwise on N(0, 1) data (the first half of
this file) and element by element against the long-double application of the library's double host matrices (the second half;
resample_ref.py states the bar, cap = sum of K_k + 8 over the directions that run, and lists the shapes by the route of
cheb_resample_kernel / line_chain they reach), with the two prolongations of solve.py held to the same bar.

Which template of cheb_resample_kernel a launch runs is decided by resample_launch (LINES_A for Q <= 4, BM = 128 for M > 64); the
ABI reports only launch counts.  The per-element tests restate that rule (resample_ref.route), assert it on their shapes and
assert the launch count.  Every route is reached from the ABI at a small shape; none needed a switch.

Worst ratios |y - truth| / (2^-53 B) measured on an MI355X (printed with pytest -s; profiles/resample/ratios.txt holds one line per
test id and input kind, written where RESAMPLE_RATIOS_OUT names a file):
  test_per_element                       343 figures, worst 37.2 (cap 1030) at [1024i-700a-c1] alternating (69, 0);
                                         nearest to its cap: 6.0 of 28 at [5x20a-5x70a-c3] scaled (1, 10, 1)
  test_odd_element_offsets_per_element     4 figures, worst  4.7 (cap   28) at [5x20a-5x70a-c3] noise (1, 1, 1)
  test_prolong_elliptic_per_element        6 figures, worst  3.5 (cap   25) at [5x4-9x7] cubic against the polynomial itself (0, 4, 0)
  test_prolong_stokes_per_element         12 figures, worst  4.1 (cap   25) at [5x4-9x7] cubic velocity against the polynomial itself (1, 4, 1)
The unit-impulse and isolation tests compare bits and have no figure."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import linewise as lw
import resample_ref as rr

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = 20240229
LD = np.longdouble
RATIOS = []                       # (test, case, kind, worst ratio, cap, element)


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("RESAMPLE_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |y - truth| / (2^-53 B) per test id and input kind (tests/test_gpu_resample.py); cap = sum of K_k + 8 over the running directions\n")
            for test, case, kind, r, cap, idx in RATIOS:
                f.write("%-28s %-34s %-12s %8.3f of cap %4d at %s\n" % (test, case, kind, r, cap, idx))


def stored(dims, nodes):
    return tuple(n - 2 if nodes == "interior" else n for n in dims)


def reference(x, dims_in, dims_out, nodes_in, nodes_out, ncomp):
    """numpy float64: the host matrices applied direction by direction."""
    t = x.reshape(stored(dims_in, nodes_in) + (ncomp,))
    for k, (a, b) in enumerate(zip(dims_in, dims_out)):
        R = sp.resample_matrix(a, b, nodes_in, nodes_out)
        t = np.moveaxis(np.tensordot(R, t, axes=([1], [k])), 0, k)
    return t.ravel()


def run(dims_in, dims_out, nodes_in="all", nodes_out="all", ncomp=1, seed=0):
    r = sp.Resample(dims_in, dims_out, nodes_in, nodes_out, ncomp)
    x = np.random.default_rng(SEED + seed).standard_normal(r.size(0))
    y = torch.full((r.size(1),), float("nan"), dtype=torch.float64, device="cuda")
    r.apply(torch.from_numpy(x).cuda(), y)
    torch.cuda.synchronize()
    out = y.cpu().numpy()
    r.destroy()
    return x, out


CASES = [
    ((17,), (33,), "all", "all", 1), ((33,), (17,), "all", "all", 1), ((2,), (1024,), "all", "all", 1), ((1024,), (3,), "all", "all", 1),
    ((257,), (100,), "interior", "all", 1), ((9, 7), (16, 5), "all", "interior", 3), ((3, 2), (257, 4), "all", "all", 4),
    ((12, 9, 20), (15, 24, 8), "all", "all", 3), ((10, 11, 12), (20, 22, 6), "interior", "interior", 4),
    ((6, 5, 4, 3), (7, 9, 4, 5), "all", "interior", 1), ((12, 12, 12, 12, 12), (16, 16, 16, 16, 16), "all", "all", 1),
    ((5, 4, 3, 6, 5), (4, 7, 5, 3, 6), "interior", "all", 3), ((64, 64, 64), (128, 128, 128), "all", "interior", 3),
    ((1024, 2), (5, 1024), "all", "all", 1), ((40, 31), (40, 62), "all", "all", 4),
]


@pytest.mark.parametrize("dims_in,dims_out,nodes_in,nodes_out,ncomp", CASES, ids=lambda v: str(v))
def test_parity_with_host_matrices(dims_in, dims_out, nodes_in, nodes_out, ncomp):
    x, y = run(dims_in, dims_out, nodes_in, nodes_out, ncomp)
    ref = reference(x, dims_in, dims_out, nodes_in, nodes_out, ncomp)
    assert np.isfinite(y).all()
    assert np.linalg.norm(y - ref) <= 1e-13 * np.linalg.norm(ref)


def test_parity_128_to_256():
    x, y = run((128, 128, 128), (256, 256, 256))
    ref = reference(x, (128,) * 3, (256,) * 3, "all", "all", 1)
    assert np.linalg.norm(y - ref) <= 1e-13 * np.linalg.norm(ref)


def test_asymmetric_matrix_layout():
    """An interpolation matrix that is not centro-symmetric (INTERIOR -> ALL of different sizes along the last, contiguous
    direction and along an outer one) catches a transposed or mis-rowed C/D layout."""
    for dims_in, dims_out in (((7, 40), (7, 23)), ((40, 7), (23, 7))):
        r = sp.Resample(dims_in, dims_out, "all", "all")
        x = np.zeros(r.size(0)); x[3] = 1.0
        y = r.apply(torch.from_numpy(x).cuda(), torch.empty(r.size(1), dtype=torch.float64, device="cuda")).cpu().numpy()
        assert np.linalg.norm(y - reference(x, dims_in, dims_out, "all", "all", 1)) <= 1e-14
        r.destroy()


@pytest.mark.parametrize("dims,nodes,ncomp", [((17, 33, 8), "all", 1), ((9, 10, 11), "interior", 3), ((1024, 4), "all", 2)])
def test_equal_grids_copy_bits(dims, nodes, ncomp):
    x, y = run(dims, dims, nodes, nodes, ncomp)
    assert np.array_equal(x, y)


def test_one_changing_direction_keeps_the_others_bits():
    """(9, 17) -> (17, 17): the second direction is the identity and the coincident nodes of the first are unit rows."""
    x, y = run((9, 17), (17, 17))
    assert np.array_equal(y.reshape(17, 17)[::2], x.reshape(9, 17))


@pytest.mark.parametrize("dims_in,dims_out,nodes_in,nodes_out", [((8, 9, 10), (31, 20, 13), "all", "all"),
                                                                 ((12, 12, 12), (24, 24, 24), "interior", "all"),
                                                                 ((40, 30), (9, 11), "all", "interior")])
def test_low_degree_polynomial_reproduced(dims_in, dims_out, nodes_in, nodes_out):
    def field(dims, nodes):
        axes = [np.cos(np.pi * np.arange(n) / (n - 1))[1:n - 1] if nodes == "interior" else np.cos(np.pi * np.arange(n) / (n - 1)) for n in dims]
        g = np.meshgrid(*axes, indexing="ij")
        return (1.0 + g[0] ** 3 - 2.0 * g[0] * g[1] ** 2 + 0.5 * g[-1] ** 4).ravel()
    r = sp.Resample(dims_in, dims_out, nodes_in, nodes_out)
    y = r.apply(torch.from_numpy(field(dims_in, nodes_in)).cuda(), torch.empty(r.size(1), dtype=torch.float64, device="cuda"))
    assert np.abs(y.cpu().numpy() - field(dims_out, nodes_out)).max() <= 1e-12
    r.destroy()


@pytest.mark.parametrize("coarse,fine,nodes,ncomp", [((12, 13, 14), (24, 25, 30), "all", 1), ((10, 10, 10), (21, 19, 18), "interior", 3)])
def test_round_trip(coarse, fine, nodes, ncomp):
    up = sp.Resample(coarse, fine, nodes, nodes, ncomp)
    down = sp.Resample(fine, coarse, nodes, nodes, ncomp)
    x = torch.from_numpy(np.random.default_rng(SEED + 3).standard_normal(up.size(0))).cuda()
    y = up.apply(x, torch.empty(up.size(1), dtype=torch.float64, device="cuda"))
    z = down.apply(y, torch.empty(down.size(1), dtype=torch.float64, device="cuda"))
    assert float((z - x).norm()) <= 1e-13 * float(x.norm())
    up.destroy(); down.destroy()


def test_odd_element_offsets():
    """Input and output tensors that are torch slices starting at an odd element (8-byte, not 16-byte, aligned)."""
    dims_in, dims_out = (20, 15, 9), (31, 8, 16)
    r = sp.Resample(dims_in, dims_out, "all", "all", 3)
    x = np.random.default_rng(SEED + 5).standard_normal(r.size(0))
    bx = torch.zeros(r.size(0) + 3, dtype=torch.float64, device="cuda")
    by = torch.full((r.size(1) + 4,), -7.0, dtype=torch.float64, device="cuda")
    bx[1:1 + r.size(0)] = torch.from_numpy(x).cuda()
    r.apply(bx[1:1 + r.size(0)], by[3:3 + r.size(1)])
    out = by.cpu().numpy()
    ref = reference(x, dims_in, dims_out, "all", "all", 3)
    assert np.linalg.norm(out[3:3 + r.size(1)] - ref) <= 1e-13 * np.linalg.norm(ref)
    assert (out[:3] == -7.0).all() and out[-1] == -7.0                    # nothing written outside the slice
    r.destroy()


def test_non_default_stream_ordering():
    """Everything on a side stream: the input is produced, resampled and consumed there, the result read after a synchronise."""
    dims_in, dims_out = (96, 96, 96), (128, 128, 128)
    r = sp.Resample(dims_in, dims_out)
    x = torch.from_numpy(np.random.default_rng(SEED + 7).standard_normal(r.size(0))).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xin = torch.empty_like(x)
        y = torch.empty(r.size(1), dtype=torch.float64, device="cuda")
        for rep in range(3):
            xin.copy_(x).mul_(rep + 1.0)
            r.apply(xin, y)
            z = y.clone()
    s.synchronize()
    ref = reference(x.cpu().numpy() * 3.0, dims_in, dims_out, "all", "all", 1)
    assert np.linalg.norm(z.cpu().numpy() - ref) <= 1e-13 * np.linalg.norm(ref)
    r.destroy()


def test_overlapping_arguments_refused():
    r = sp.Resample((8, 8), (8, 9))
    buf = torch.zeros(200, dtype=torch.float64, device="cuda")
    with pytest.raises(sp.ChebhipError):
        r.apply(buf[:64], buf[10:82])
    r.destroy()


# =================================================================================================================================
# element by element (resample_ref.py)
# =================================================================================================================================
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).ravel()).cuda()


def apply(r, x, shape):
    """One call on a NaN-filled output, as a host array of `shape`."""
    y = torch.full((r.size(1),), float("nan"), dtype=torch.float64, device="cuda")
    r.apply(dev(x), y)
    torch.cuda.synchronize()
    return y.cpu().numpy().reshape(shape)


def held(test, case, kind, y, t, B, cap):
    """The bar, printed and recorded."""
    ratio, idx = lw.check(y, t, B, cap, "%s %s %s" % (test, case, kind))
    print("%-28s %-34s %-12s %8.3f of cap %4d at %s" % (test, case, kind, ratio, cap, idx))
    RATIOS.append((test, case, kind, ratio, cap, idx))
    return ratio


# what each group of resample_ref.SHAPES must reach: a predicate on the launches [(direction, O, K, M, Q)] of a shape
ROUTES = {
    "chunks": lambda g, s: len(g) == 1 and g[0][1] == 1 and g[0][4] == 1 and rr.route(*g[0][2:]) == (True, 64),
    "tile": lambda g, s: len(g) == 1 and g[0][1] * g[0][4] == 1 and rr.route(*g[0][2:])[1] == (128 if g[0][3] > 64 else 64),
    "lines": lambda g, s: len(g) == 1 and g[0][0] == 1 and g[0][1] > 1 and g[0][4] > 4 and g[0][1] * g[0][4] in (63, 64, 65, 130)
                          and rr.route(*g[0][2:]) == (False, 64),
    "lines_a": lambda g, s: len(g) == 1 and g[0][4] == (4 if s[0] == (12, 2) else s[4]) and rr.route(*g[0][2:]) == (True, 128 if g[0][3] > 64 else 64),
    "components": lambda g, s: len(g) == 1 and g[0][1] == 1 and g[0][4] == s[4] > 1 and rr.route(*g[0][2:]) == (True, 128 if g[0][3] > 64 else 64),
    "colfast": lambda g, s: len(g) == 1 and g[0][0] == 0 and g[0][4] == s[0][1] and rr.route(*g[0][2:]) == (False, 128 if g[0][3] > 64 else 64),
    "nodes": lambda g, s: len(g) == len(s[0]) and (s[0] != (3, 5) or [(q[2], q[3]) for q in g] == [(3, 1), (1, 5)]),
    "chains": lambda g, s: len(g) == {2: 2, 4: 3 if s[0] == (6, 5, 4, 3) else 4, 5: 5}[len(s[0])],
}
GROUPED = [(group, s) for group, shapes in rr.SHAPES.items() for s in shapes]


@pytest.mark.parametrize("group,s", GROUPED, ids=lambda v: v if isinstance(v, str) else rr.shape_id(v))
def test_per_element(group, s):
    """Every input kind of resample_ref.inputs on every shape: the bar, the launch count, the asserted route, the same bits from a
    second call on the handle; constants are reproduced to the bar."""
    di, do, a, b, c = s
    geo = rr.geometry(s)
    assert ROUTES[group](geo, s), geo
    r = sp.Resample(di, do, a, b, c)
    shape_in, shape_out = rr.stored(di, a) + (c,), rr.stored(do, b) + (c,)
    assert r.size(0) == np.prod(shape_in) and r.size(1) == np.prod(shape_out)
    count = sp.lib().chebhip_launch_count
    for kind in rr.KINDS:
        for n, x in enumerate(rr.inputs(kind, shape_in, SEED, [q[0] for q in geo])):
            t, B, cap = rr.truth_bound(x, di, do, a, b)
            c0 = count()
            y = apply(r, x, shape_out)
            assert count() - c0 == len(geo)
            held("per_element", rr.shape_id(s), kind + (str(n) if kind == "impulse" else ""), y, t, B, cap)
            assert np.array_equal(y, apply(r, x, shape_out)), "second call on the handle"
            if kind == "constant":
                lw.check(y, np.broadcast_to(x.reshape(-1, c)[0].astype(LD), shape_out), B, cap, "constant reproduced")
    r.destroy()


ONE_DIRECTION = rr.SHAPES["chunks"] + rr.SHAPES["tile"] + rr.SHAPES["components"]


@pytest.mark.parametrize("s", ONE_DIRECTION, ids=rr.shape_id)
def test_unit_impulses_return_the_column_bits_1d(s):
    """One direction, a single 1.0 per line: 1.0 times an entry plus exact zeros is exact on the MFMA chain, so every line of the
    output is a column of the double matrix bit for bit.  ceil(K / ncomp) calls show every column; inputs and outputs are rows of
    two device arrays, so most calls see tensors that are 8-byte but not 16-byte aligned."""
    di, do, a, b, c = s
    (R,) = rr.mats(di, do, a, b)
    M, K = R.shape
    nrun = (K + c - 1) // c
    xs, cols = zip(*[rr.unit_impulses(K, c, run) for run in range(nrun)])
    assert set(np.concatenate(cols)) == set(range(K))
    r = sp.Resample(di, do, a, b, c)
    X = dev(np.stack(xs)).reshape(nrun, K * c)
    Y = torch.full((nrun, M * c), float("nan"), dtype=torch.float64, device="cuda")
    for run in range(nrun):
        r.apply(X[run], Y[run])
    torch.cuda.synchronize()
    Y = Y.cpu().numpy().reshape(nrun, M, c)
    for run in range(nrun):
        assert np.array_equal(Y[run], R[:, cols[run]]), (run, cols[run])
    r.destroy()


@pytest.mark.parametrize("s", rr.SHAPES["lines"] + rr.SHAPES["lines_a"] + rr.SHAPES["colfast"], ids=rr.shape_id)
def test_unit_impulses_return_the_column_bits(s):
    """The same with other directions around the running one: line l holds its 1.0 at point (l + seed) mod K (linewise.impulse)."""
    di, do, a, b, c = s
    Ms = rr.mats(di, do, a, b)
    ((k, O, K, M, Q),) = rr.geometry(s)
    shape_in, shape_out = rr.stored(di, a) + (c,), rr.stored(do, b) + (c,)
    r = sp.Resample(di, do, a, b, c)
    seen = set()
    for seed in range(-(-K // (O * Q))):
        j = (np.arange(O * Q) + seed * O * Q) % K
        seen.update(j)
        rest = [n for m, n in enumerate(shape_in) if m != k]
        want = np.moveaxis(Ms[k][:, j].reshape([M] + rest), 0, k)
        assert np.array_equal(apply(r, lw.impulse(shape_in, k, seed * O * Q), shape_out), want), seed
    assert seen == set(range(K))
    r.destroy()


@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_isolation(ncomp, bad):
    """A NaN, and separately +Inf, at one node of one component: every other component keeps the bits of the clean run (the lines
    of different components share MFMA tiles, never a column), and the component itself is non-finite wherever the
    tensor-product row has a non-zero weight at that node.  The component's other outputs -- the unit rows of the shared end
    nodes, whose weight at the node is an exact zero -- are left unasserted: 0 times Inf or NaN is NaN in the product, and
    either outcome is acceptable there."""
    di, do = (9, 7), (12, 12)                                            # only the end nodes are shared: every other row is full
    Ms = rr.mats(di, do, "all", "all")
    geo = rr.geometry((di, do, "all", "all", ncomp))
    assert [rr.route(*q[2:])[0] for q in geo] == [False, True]            # COLFAST (Q = 7 ncomp), then LINES_A (Q = ncomp)
    node, comp = (4, 3), 1
    x = lw.noise(di + (ncomp,), 0, SEED + ncomp)
    r = sp.Resample(di, do, "all", "all", ncomp)
    clean = apply(r, x, do + (ncomp,))
    x[node + (comp,)] = bad
    y = apply(r, x, do + (ncomp,))
    others = [q for q in range(ncomp) if q != comp]
    assert np.isfinite(clean).all() and np.array_equal(y[..., others], clean[..., others])
    touched = np.multiply.outer(Ms[0][:, node[0]] != 0.0, Ms[1][:, node[1]] != 0.0)
    assert touched.sum() >= (do[0] - 2) * (do[1] - 2) and not np.isfinite(y[..., comp][touched]).any()
    r.destroy()


@pytest.mark.parametrize("s", [((5, 20), (5, 70), "all", "all", 3), ((12, 17), (17, 17), "all", "all", 1)], ids=rr.shape_id)
def test_odd_element_offsets_per_element(s):
    """x and y start at odd elements (8-byte, not 16-byte aligned): one LINES_A case (Q = 3) and one COLFAST case (Q = 17) under
    the bar, the cells around y untouched."""
    di, do, a, b, c = s
    ((k, O, K, M, Q),) = rr.geometry(s)
    assert rr.route(K, M, Q)[0] == (c == 3)
    r = sp.Resample(di, do, a, b, c)
    for kind in ("noise", "scaled"):
        (x,) = rr.inputs(kind, rr.stored(di, a) + (c,), SEED + 5, [k])
        bx = torch.zeros(r.size(0) + 3, dtype=torch.float64, device="cuda")
        by = torch.full((r.size(1) + 4,), -7.0, dtype=torch.float64, device="cuda")
        bx[1:1 + r.size(0)] = dev(x)
        assert bx[1:].data_ptr() % 16 == 8 and by[3:].data_ptr() % 16 == 8
        r.apply(bx[1:1 + r.size(0)], by[3:3 + r.size(1)])
        torch.cuda.synchronize()
        out = by.cpu().numpy()
        t, B, cap = rr.truth_bound(x, di, do, a, b)
        held("odd_offsets", rr.shape_id(s), kind, out[3:3 + r.size(1)].reshape(t.shape), t, B, cap)
        assert (out[:3] == -7.0).all() and out[-1] == -7.0
    r.destroy()


# ---- the prolongations of solve.py ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims_c,dims_f", [((5, 4), (9, 7)), ((4, 5, 6), (7, 9, 8))], ids=str)
def test_prolong_elliptic_per_element(dims_c, dims_f):
    """solve.prolong_elliptic against resample_ref.prolong_elliptic (interior row-major, compact boundary values row-major over
    the boundary nodes): noise, and a cubic state with its own boundary values, which is also reproduced on the fine interior; the
    second call of a level pair comes from the cache with the same bits."""
    case = "%s-%s" % ("x".join(map(str, dims_c)), "x".join(map(str, dims_f)))
    nin = int(np.prod([n - 2 for n in dims_c]))
    rng = np.random.default_rng(SEED + 21)
    xp, dvp, fine = rr.elliptic_polynomial(dims_c, dims_f)
    for kind, x, dv in (("noise", rng.standard_normal(nin), rng.standard_normal(int(np.prod(dims_c)) - nin)), ("cubic", xp, dvp)):
        t, B, cap = rr.prolong_elliptic(dims_c, x, dv, dims_f)
        y = solve.prolong_elliptic(sp, dims_c, dev(x), dv, dims_f)
        cached = len(solve._prolong_cache)
        y2 = solve.prolong_elliptic(sp, dims_c, dev(x), dev(dv), dims_f)
        torch.cuda.synchronize()
        assert len(solve._prolong_cache) == cached and torch.equal(y, y2)
        y = y.cpu().numpy().reshape(t.shape)
        held("prolong_elliptic", case, kind, y, t, B, cap)
        if kind == "cubic":
            held("prolong_elliptic", case, "cubic-exact", y, fine.astype(LD), B, cap)


@pytest.mark.parametrize("dims_c,dims_f", [((5, 4), (9, 7)), ((4, 5, 4), (7, 6, 9))], ids=str)
def test_prolong_stokes_per_element(dims_c, dims_f):
    """solve.prolong_stokes against resample_ref.prolong_stokes: the velocity (node-major, d components, ALL -> INTERIOR with the
    compact Dirichlet values) and the pressure (INTERIOR -> INTERIOR) each under their own bar, interleaved [v, p] per fine node."""
    d = len(dims_c)
    case = "%s-%s" % ("x".join(map(str, dims_c)), "x".join(map(str, dims_f)))
    nin = int(np.prod([n - 2 for n in dims_c]))
    rng = np.random.default_rng(SEED + 22)
    xp, dvp, vfine, pfine = rr.stokes_polynomial(dims_c, dims_f)
    for kind, x, dv in (("noise", rng.standard_normal(nin * (d + 1)), rng.standard_normal((int(np.prod(dims_c)) - nin) * d)),
                        ("cubic", xp, dvp)):
        (tv, Bv, capv), (tp, Bp, capp) = rr.prolong_stokes(dims_c, x, dv, dims_f)
        y = solve.prolong_stokes(sp, dims_c, dev(x), dv, dims_f)
        cached = len(solve._prolong_cache)
        y2 = solve.prolong_stokes(sp, dims_c, dev(x), dev(dv), dims_f)
        torch.cuda.synchronize()
        assert len(solve._prolong_cache) == cached and torch.equal(y, y2)
        y = y.cpu().numpy().reshape(tv.shape[:-1] + (d + 1,))
        held("prolong_stokes", case, kind + "-velocity", y[..., :d], tv, Bv, capv)
        held("prolong_stokes", case, kind + "-pressure", y[..., d:], tp, Bp, capp)
        if kind == "cubic":
            held("prolong_stokes", case, "cubic-exact-velocity", y[..., :d], vfine.astype(LD), Bv, capv)
            held("prolong_stokes", case, "cubic-exact-pressure", y[..., d:], pfine.astype(LD), Bp, capp)
