"""cheb_reduce_* on the device (ChebReduce): partial contractions against the long-double truth of reduce_ref.py, output by output
within the derived bar (T + S + 4) 2^-53 B, on every mask of every shape; against ChebModal.integrate, the field's own planes,
ChebPoints.eval_grid and ChebPlan.mult; exact partial integrals of a polynomial; isolation of NaN / Inf, run-to-run bits; the
interface and the two solve.py wrappers."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import linewise as lw
import points_ref as pref
import reduce_ref as ref

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = 20241018
LD = np.longdouble
U = 2.0 ** -53

# the shapes of test_gpu_modal.py (odd rows and odd field sizes: 8-byte aligned rows; rows of 2 .. 1024 points; one to five
# directions) and one whose last direction needs two pairs per lane
CASES = [((2,), 16), ((3, 2), 3), ((5, 7, 9), 16), ((17,), 3), ((1024,), 16), ((257, 4), 1), ((4, 257), 3), ((63, 64, 65), 1),
         ((66, 65, 64), 3), ((129, 3, 16), 16), ((6, 5, 4, 3), 3), ((12,) * 5, 1), ((40, 48, 130), 1)]
case_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).ravel()).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def data(dims, nf):
    """The inputs of a case, made once and left unchanged: N(0, 1) fields u, v; the same scaled per node by 10^+-100 (us) and by
    10^+-50 (u50, v50: the product stays finite)."""
    rng = np.random.default_rng(SEED + sum(dims) + nf)
    n = nf * int(np.prod(dims))
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    us = u * 10.0 ** rng.integers(-100, 101, size=n)
    u50, v50 = u * 10.0 ** rng.integers(-50, 51, size=n), v * 10.0 ** rng.integers(-50, 51, size=n)
    return dict(u=u, v=v, us=us, u50=u50, v50=v50)


def handle(dims, nf, mask, weights=None):
    return sp.ChebReduce(dims, nf, over=ref.over(mask), weights=weights)


# ---- 1. every output within the derived bar -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_per_element_bar(dims, nf):
    """Every mask; u, u v and u u on N(0, 1) and on per-node scaled data with the default weights, u and u v with dnode, point and
    mean mixed over the contracted directions.  Prints the worst ratio of the case (profiles/reduce/ratios.txt)."""
    d = data(dims, nf)
    t = {k: dev(x) for k, x in d.items()}
    worst, where = 0.0, None
    for mask in ref.masks(dims):
        cap = ref.cap(dims, mask)
        h = handle(dims, nf, mask)
        assert h.out_dims == ref.out_dims(dims, mask) and h.size(1) == nf * int(np.prod(h.out_dims, dtype=np.int64))
        ws = ref.default_weights(dims, mask)
        runs = [("u", "u", None), ("uv", "u", "v"), ("uu", "u", "u"), ("scaled u", "us", None), ("scaled uv", "u50", "v50"),
                ("scaled uu", "u50", "u50")]
        for what, a, b in runs:
            out = host(h.apply(t[a], None if b is None else t[b]))
            assert out.shape == (nf,) + h.out_dims
            tr, B = ref.truth_bound(dims, nf, mask, ws, d[a], None if b is None else d[b])
            r = ref.ratio(out, tr, B)
            print("%s nf %d mask %s slices %d %s: %.3g of %d" % (case_ids(dims), nf, "".join(map(str, mask)), h.slices, what, r, cap))
            assert r <= cap, (mask, what, r, cap)
            if r / cap > worst:
                worst, where = r / cap, (mask, what, r, cap)
        kinds = ref.mixed_kinds(dims, mask)
        ws = [None if k is None else sp.reduce_weights(n, k) for n, k in zip(dims, kinds)]
        for k, kind in enumerate(kinds):
            if kind is not None:
                h.set_weights(k, kind)
        for what, a, b in (("mixed u", "u", None), ("mixed uv", "u", "v")):
            out = host(h.apply(t[a], None if b is None else t[b]))
            tr, B = ref.truth_bound(dims, nf, mask, ws, d[a], None if b is None else d[b])
            r = ref.ratio(out, tr, B)
            assert r <= cap, (mask, what, r, cap)
            if r / cap > worst:
                worst, where = r / cap, (mask, what, r, cap)
        h.destroy()
    print("reduce-ratio %s nf %d: worst error / bar = %.3g (mask %s, %s: %.3g of cap %d)" % (
        case_ids(dims), nf, worst, "".join(map(str, where[0])), where[1], where[2], where[3]))
    for k, x in d.items():                                          # the inputs are unmodified
        assert (bits(host(t[k])) == bits(x)).all()


def test_both_paths_of_both_kernels():
    """The shapes above reach the direct store (slices == 1) and the sliced path of the row kernel (last direction contracted) and
    of the column kernel (last direction kept)."""
    seen = set()
    for dims, nf in CASES:
        for mask in ref.masks(dims):
            h = handle(dims, nf, mask)
            assert h.slices >= 1
            seen.add((mask[-1], h.slices > 1))
            h.destroy()
    assert seen == {(1, False), (1, True), (0, False), (0, True)}


# ---- 2. values against existing calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_full_contraction_is_integrate(dims, nf):
    """Within the sum of the two bars, (T + S + 4) U B of this call and (L + 8) U B of ChebModal.integrate."""
    d = data(dims, nf)
    u, v = dev(d["u"]), dev(d["v"])
    mask = (1,) * len(dims)
    h, m = handle(dims, nf, mask), sp.ChebModal(dims, nf)
    L = int(np.prod(dims))
    for b, vb in ((None, None), (v, d["v"])):
        got, want = host(h.apply(u, b)), host(m.integrate(u, b))
        _, B = ref.truth_bound(dims, nf, mask, ref.default_weights(dims, mask), d["u"], vb)
        assert got.shape == (nf,)
        assert (np.abs(got - want) <= (ref.cap(dims, mask) + L + 8) * U * B).all()
    h.destroy(); m.destroy()


@pytest.mark.parametrize("dims,nf", [((5, 7, 9), 16), ((66, 65, 64), 3), ((6, 5, 4, 3), 3)], ids=case_ids)
def test_node_returns_the_plane(dims, nf):
    """Unit vectors as weights: one 1.0 x value and exact zeros, so every element is the field's own (finite data)."""
    d = data(dims, nf)
    u = d["u"].reshape((nf,) + dims)
    ud = dev(u)
    nd = len(dims)
    for k in range(nd):                                              # a face or an interior plane
        for j in sorted({0, dims[k] // 2, dims[k] - 1}):
            h = sp.ChebReduce(dims, nf, over=(k,), weights={k: ("node", j)})
            assert (host(h.apply(ud)) == np.take(u, j, axis=k + 1)).all()
            h.destroy()
    for k0, k1 in ((0, 1), (0, nd - 1), (nd - 2, nd - 1)):            # an edge
        j0, j1 = dims[k0] - 1, 1
        h = sp.ChebReduce(dims, nf, over=(k0, k1), weights={k0: ("node", j0), k1: ("node", j1)})
        assert (host(h.apply(ud)) == np.take(np.take(u, j1, axis=k1 + 1), j0, axis=k0 + 1)).all()
        h.destroy()


@pytest.mark.parametrize("dims,nf", [((5, 7, 9), 16), ((63, 64, 65), 1)], ids=case_ids)
def test_point_is_eval_grid(dims, nf):
    """The plane x_k = x against ChebPoints.eval_grid with one coordinate along k and the nodes elsewhere: within the sum of the
    two bars, (T + S + 4) U B here and cap(dims) U B there (points_ref), B = sum |l_j| |u|."""
    d = data(dims, nf)
    ud = dev(d["u"])
    pts = sp.ChebPoints(dims, nf)
    pts.reserve_grid(dims)
    for k, n in enumerate(dims):
        for x in (0.3, -0.987654321):
            mask = tuple(int(m == k) for m in range(len(dims)))
            h = sp.ChebReduce(dims, nf, over=(k,), weights={k: ("point", x)})
            got = host(h.apply(ud))
            coords = [dev(np.array([x])) if m == k else dev(sp.cgl_nodes(p)) for m, p in enumerate(dims)]
            want = host(pts.eval_grid(ud, coords)).squeeze(k + 1)
            ws = [sp.reduce_weights(n, ("point", x)) if m == k else None for m in range(len(dims))]
            _, B = ref.truth_bound(dims, nf, mask, ws, d["u"])
            assert (np.abs(got - want) <= (ref.cap(dims, mask) + pref.cap(dims)) * U * B).all()
            h.destroy()
    pts.destroy()


@pytest.mark.parametrize("dims,nf", [((5, 7, 9), 16), ((66, 65, 64), 3)], ids=case_ids)
def test_dnode_is_a_slice_of_the_derivative(dims, nf):
    """d/dx_k on a grid plane against the slice of ChebPlan.mult on the stacked tensor: within the sum of the two bars,
    (T + S + 4) U B here and (K + 8) U B_i there (README, second bar; linewise.bound)."""
    d = data(dims, nf)
    u = d["u"].reshape((nf,) + dims)
    ud = dev(u)
    for k, n in enumerate(dims):
        plan = sp.ChebPlan((nf,) + dims, k + 1)
        full = host(plan.mult(ud, torch.empty_like(ud))).reshape((nf,) + dims)
        Bplan = lw.bound(lw.dense_D(n), u, k + 1)
        plan.destroy()
        for j in sorted({0, n // 2, n - 1}):
            mask = tuple(int(m == k) for m in range(len(dims)))
            h = sp.ChebReduce(dims, nf, over=(k,), weights={k: ("dnode", j)})
            got = host(h.apply(ud))
            ws = [sp.reduce_weights(n, ("dnode", j)) if m == k else None for m in range(len(dims))]
            _, B = ref.truth_bound(dims, nf, mask, ws, d["u"])
            bar = ref.cap(dims, mask) * U * B + (n + 8) * U * np.take(Bplan, j, axis=k + 1)
            assert (np.abs(got - np.take(full, j, axis=k + 1)) <= bar).all()
            h.destroy()


def test_exact_partial_integrals():
    """u = x^2 y + z on (9, 10, 11): Clenshaw-Curtis is exact for it, so every partial integral is known: over x 2 y / 3 + 2 z,
    over y 2 z, over z 2 x^2 y, and so on.  Bar: (T + 2 S + 12) U B' with B' = sum |W| (|x^2 y| + |z|): T + S + 4 for the device,
    S for the rounding of the weights, one for the rounding of u, at most 4 for the nodes of the table (x du/dx = 2 x^2 y is
    within 2 (|x^2 y| + |z|), the other two directions likewise), the rest for evaluating the closed form."""
    dims = (9, 10, 11)
    x, y, z = (sp.cgl_nodes(n).astype(LD).reshape([-1 if m == k else 1 for m in range(3)]) for k, n in enumerate(dims))
    u = (x * x * y + z).astype(np.float64)
    mag = (np.abs(x * x * y) + np.abs(z) + 0 * u).astype(np.float64)
    exact = {(1, 0, 0): LD(2) / 3 * y + 2 * z + 0 * x, (0, 1, 0): 2 * z + 0 * x * y, (0, 0, 1): 2 * x * x * y + 0 * z,
             (1, 1, 0): 4 * z + 0 * x * y, (1, 0, 1): LD(4) / 3 * y + 0 * x * z, (0, 1, 1): 0 * x * y * z, (1, 1, 1): 0 * x * y * z}
    ud = dev(u)
    for mask, full in exact.items():
        want = full
        for k in (2, 1, 0):
            if mask[k]:
                want = np.take(want, 0, axis=k)
        h = handle(dims, 1, mask)
        got = host(h.apply(ud))[0]
        Bp = ref.contract(mag[None], mask, [None if w is None else np.abs(w) for w in ref.default_weights(dims, mask)])[0]
        T = int(np.prod([n for n, c in zip(dims, mask) if c]))
        assert got.shape == want.shape
        assert (np.abs(got.astype(LD) - want).astype(np.float64) <= (T + 2 * sum(mask) + 12) * U * Bp).all(), mask
        h.destroy()


# ---- 3. isolation and bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_isolation_and_bits(dims, nf):
    """One NaN, then one +Inf, at one node of u: exactly the outputs that own the node (its field, its kept indices) turn
    non-finite, every other output keeps the bits of the clean run; a second clean run repeats the first bit for bit."""
    d = data(dims, nf)
    rng = np.random.default_rng(SEED + 7 + sum(dims))
    ud, vd = dev(d["u"]), dev(d["v"])
    node = (int(rng.integers(nf)),) + tuple(int(rng.integers(n)) for n in dims)
    flat = int(np.ravel_multi_index(node, (nf,) + dims))
    for mask in ref.masks(dims):
        h = handle(dims, nf, mask)
        clean = [host(h.apply(ud)), host(h.apply(ud, vd))]
        again = [host(h.apply(ud)), host(h.apply(ud, vd))]
        owner = np.zeros((nf,) + h.out_dims, dtype=bool)
        owner[(node[0],) + tuple(i for i, c in zip(node[1:], mask) if not c)] = True
        for bad in (float("nan"), float("inf")):
            ub = ud.clone()
            ub[flat] = bad
            for c, a, out in zip(clean, again, (host(h.apply(ub)), host(h.apply(ub, vd)))):
                assert (bits(c) == bits(a)).all()
                assert (~np.isfinite(out[owner])).all() and owner.sum() == 1
                assert (bits(out)[~owner] == bits(c)[~owner]).all(), (mask, bad)
        h.destroy()
    assert (bits(host(ud)) == bits(d["u"])).all() and (bits(host(vd)) == bits(d["v"])).all()


# ---- 4. interface ---------------------------------------------------------------------------------------------------------------
def test_interface():
    dims, nf = (6, 5, 4, 3), 3
    d = data(dims, nf)
    ud = dev(d["u"])
    h = sp.ChebReduce(dims, nf, over=(1, 3))
    assert h.out_dims == (6, 4) and h.size(0) == nf * 360 and h.size(1) == nf * 24 and h.size() == nf * 360 and h.slices >= 1
    assert sp.lib().cheb_reduce_size(h._h, 2) == -1
    out = torch.full((nf, 6, 4), float("nan"), dtype=torch.float64, device="cuda")
    assert h.apply(ud, out=out) is out
    first = host(out).copy()
    # new weights are used by the next apply, None restores the default
    mask = (0, 1, 0, 1)
    h.set_weights(1, ("dnode", 0))
    h.set_weights(3, np.array([1.0, -2.0, 0.5]))
    ws = [None, sp.reduce_weights(5, ("dnode", 0)), None, np.array([1.0, -2.0, 0.5])]
    tr, B = ref.truth_bound(dims, nf, mask, ws, d["u"])
    assert ref.ratio(host(h.apply(ud)), tr, B) <= ref.cap(dims, mask)
    h.set_weights(1, None); h.set_weights(3, "integral")
    assert (bits(host(h.apply(ud))) == bits(first)).all()
    # refused: weights on a kept direction, wrong lengths, directions out of range, overlapping output
    with pytest.raises(sp.ChebhipError) as e:
        h.set_weights(0, "mean")
    assert e.value.code == 4
    with pytest.raises(sp.ChebhipError) as e:
        h.set_weights(4, "mean")
    assert e.value.code == 2
    with pytest.raises(ValueError):
        h.set_weights(1, np.ones(6))
    with pytest.raises(AssertionError):
        h.apply(ud[:-1])
    with pytest.raises(AssertionError):
        h.apply(ud, ud[:-1])
    with pytest.raises(AssertionError):
        h.apply(ud, out=out[:, :, :3].contiguous())
    big = torch.zeros(nf * 360 + 100, dtype=torch.float64, device="cuda")
    for o in (0, nf * 360 - 1):
        with pytest.raises(sp.ChebhipError) as e:
            h.apply(big[:nf * 360], out=big[o:o + nf * 24])
        assert e.value.code == 4 and "overlap" in str(e.value)
        with pytest.raises(sp.ChebhipError):
            h.apply(ud, big[:nf * 360], out=big[o:o + nf * 24])
    assert h.apply(big[:nf * 360], out=big[nf * 360:nf * 360 + nf * 24]).shape == (nf * 24,)
    h.destroy(); h.destroy()
    with pytest.raises(sp.ChebhipError) as e:
        sp.ChebReduce(dims, nf, over=())
    assert e.value.code == 4
    with pytest.raises(sp.ChebhipError) as e:
        sp.ChebReduce(dims, nf, over=(4,))
    assert e.value.code == 2
    assert sp.ChebReduce(dims, nf, over=1).out_dims == (6, 4, 3)
    torch.cuda.synchronize()


def test_profile_and_face_flux():
    dims, nf = (17, 12, 9), 2
    rng = np.random.default_rng(SEED)
    u = rng.standard_normal((nf,) + dims)
    ud = dev(u)
    for axis in range(3):
        mask = tuple(int(k != axis) for k in range(3))
        ws = [None if k == axis else sp.reduce_weights(n, "mean") for k, n in enumerate(dims)]
        tr, B = ref.truth_bound(dims, nf, mask, ws, u)
        got = host(solve.profile(sp, dims, ud, axis))
        assert got.shape == (nf, dims[axis]) and ref.ratio(got, tr, B) <= ref.cap(dims, mask)
        for side in (0, 1):
            j, sign = (0, 1.0) if side == 0 else (dims[axis] - 1, -1.0)
            ws = [sign * sp.reduce_weights(n, ("dnode", j)) if k == axis else sp.cc_weights(n) for k, n in enumerate(dims)]
            tr, B = ref.truth_bound(dims, nf, (1, 1, 1), ws, u)
            got = host(solve.face_flux(sp, dims, ud, axis, side))
            assert got.shape == (nf,) and ref.ratio(got, tr, B) <= ref.cap(dims, (1, 1, 1))
            mask = tuple(int(k == axis) for k in range(3))
            tr, B = ref.truth_bound(dims, nf, mask, [w if k == axis else None for k, w in enumerate(ws)], u)
            got = host(solve.face_flux(sp, dims, ud, axis, side, integrate=False))
            assert got.shape == (nf,) + ref.out_dims(dims, mask) and ref.ratio(got, tr, B) <= ref.cap(dims, mask)
    # u = x on a line of 17 points: du/dnu = +1 at x = +1 and -1 at x = -1, to a few roundings of the row of D
    x = sp.cgl_nodes(17)
    assert abs(float(host(solve.face_flux(sp, (17,), dev(x), 0, 0))[0]) - 1.0) <= 25 * U * np.abs(sp.reduce_weights(17, ("dnode", 0)) * x).sum()
    assert abs(float(host(solve.face_flux(sp, (17,), dev(x), 0, 1))[0]) + 1.0) <= 25 * U * np.abs(sp.reduce_weights(17, ("dnode", 16)) * x).sum()
    assert (host(solve.profile(sp, (17,), dev(x), 0)) == x[None]).all()
    with pytest.raises(ValueError):
        solve.profile(sp, dims, ud, 3)
    with pytest.raises(ValueError):
        solve.face_flux(sp, dims, ud, 0, 2)
