"""cheb_points_* on the device (ChebPoints): interpolation rows, scattered points and tensor grids of arbitrary coordinates against
the numpy long-double restatement of the same formula on the double node table (tests/points_ref.py), element by element:
|out - value_p| <= cap(dims) U B_p, cap(dims) = sum_k ((1 + Lambda(n_k)) n_k + 8), B_p = sum prod |l| |u|.  cap counts the
roundings of one direction -- three per entry (two differences and a quotient), (n - 1) Lambda for the normalising sum, one for
the division, n plus a few for the contraction -- and the directions add.  Also: nodes return the field's bits, NaN / Inf
coordinates stay at their point, run-to-run and position-to-position bits, a check that does not use the formula (Chebyshev sums),
grids against Resample and solve.sample_plane, the interface."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import points_ref as ref

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = 20240229
LD = np.longdouble
U = ref.U

# Q <= 4 and Q > 4 in the line product, its 64-line and 16-point chunk edges, odd (8-byte aligned) blocks, one to five directions
CASES = [((2,), 16), ((17,), 3), ((1024,), 1), ((3, 2), 3), ((4, 257), 3), ((257, 4), 1), ((5, 7, 9), 16), ((33, 20, 17), 1),
         ((63, 64, 65), 1), ((66, 65, 64), 3), ((6, 5, 4, 3), 3), ((12,) * 5, 1)]
case_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def field(dims, nf, scaled=False):
    rng = np.random.default_rng(SEED)
    u = rng.standard_normal(nf * int(np.prod(dims)))
    if scaled:                                           # every node by 10^+100 or 10^-100
        u = u * np.where(rng.integers(0, 2, u.size) == 1, 1e100, 1e-100)
    return u


@functools.lru_cache(maxsize=None)
def point_set(dims):
    """(points (npts, d), number of leading all-node points, their flat node indices)."""
    d = len(dims)
    rng = np.random.default_rng(SEED + 1)
    xn = [sp.cgl_nodes(n) for n in dims]
    pick = lambda cnt: np.stack([rng.integers(0, n, cnt) for n in dims], axis=1)       # node indices (cnt, d)
    at = lambda idx: np.stack([xn[k][idx[:, k]] for k in range(d)], axis=1)
    parts = []
    idx_nodes = pick(12)
    parts.append(at(idx_nodes))                                                        # every coordinate on a node
    corners = np.array(np.meshgrid(*[[1.0, -1.0]] * d, indexing="ij")).reshape(d, -1).T
    parts.append(corners)
    parts.append(rng.uniform(-1.0, 1.0, (300, d)))
    some = at(pick(12))
    mask = rng.integers(0, 2, some.shape) == 1
    parts.append(np.where(mask, some, rng.uniform(-1.0, 1.0, some.shape)))             # some coordinates on nodes
    parts.append(np.nextafter(at(pick(8)), 2.0))
    parts.append(np.nextafter(at(pick(8)), -2.0))
    for e in (1e-16, 1e-13, 1e-10, 1e-7, 1e-5, 1e-3):
        parts.append(at(pick(2)) * np.array([[1.0 + e], [1.0 - e]]))
    parts.append(np.zeros((1, d)))
    parts.append(np.full((1, d), 5e-324))
    z = rng.uniform(-1.0, 1.0, (2, d)); z[0, 0] = 0.0; z[1, -1] = 5e-324
    parts.append(z)
    flat = np.ravel_multi_index(tuple(idx_nodes.T), dims)
    return np.ascontiguousarray(np.concatenate(parts)), len(idx_nodes), flat


@functools.lru_cache(maxsize=None)
def truth(dims, nf, scaled=False):
    pts, _, _ = point_set(dims)
    rows = [ref.rows_ld(n, pts[:, k]) for k, n in enumerate(dims)]
    return ref.values_ld(dims, nf, field(dims, nf, scaled), rows)


def within(out, value, B, dims, what=""):
    err = np.abs(out.astype(LD) - value)
    bar = ref.cap(dims) * U * B
    worst = float((err / np.maximum(bar, np.finfo(float).tiny)).max())
    print("%s %s: worst error / bar = %.3g (bar = %.0f U B)" % (case_ids(tuple(dims)), what, worst, ref.cap(dims)))
    return bool((err <= bar).all())


@pytest.mark.parametrize("n", [2, 17, 64, 257, 1024])
def test_rows(n):
    h = sp.ChebPoints((n,))
    xn = sp.cgl_nodes(n)
    rng = np.random.default_rng(SEED + n)
    x = np.concatenate([rng.uniform(-1, 1, 300), xn, np.nextafter(xn, 2.0), np.nextafter(xn, -2.0), xn * (1 + 1e-13), xn * (1 - 1e-7),
                        [0.0, 5e-324, 1.0, -1.0]])
    xd = dev(x)
    R = host(h.rows(0, xd))
    want = sp.interp_matrix(n, x)
    assert R.shape == (x.size, n) and np.isfinite(R).all()
    assert (np.abs(R - want) <= ref.cap1(n) * U * np.abs(want) + ref.TINY).all()
    E = R[300:300 + n]
    assert (E == np.eye(n)).all() and not np.signbit(E).any()
    assert (host(h.rows(0, xd)).view(np.int64) == R.view(np.int64)).all()
    bad = x.copy(); bad[5] = np.nan; bad[7] = -np.inf
    Rb = host(h.rows(0, dev(bad)))
    assert np.isnan(Rb[[5, 7]]).all()
    keep = np.ones(x.size, bool); keep[[5, 7]] = False
    assert (Rb[keep].view(np.int64) == R[keep].view(np.int64)).all()
    h.destroy()


@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_scattered_values(dims, nf):
    pts, nn, flat = point_set(dims)
    value, B = truth(dims, nf)
    u = field(dims, nf)
    h = sp.ChebPoints(dims, nf)
    C = h.chunk
    assert 1 <= C <= 1024 and (C % 64 == 0 or C < 64)
    ud = dev(u)
    out = host(h.eval(ud, dev(pts)))
    assert out.shape == (nf, len(pts))
    assert within(out, value, B, dims, "base set")
    # nodes return their values
    assert (out[:, :nn].view(np.int64) == u.reshape(nf, -1)[:, flat].view(np.int64)).all()
    # the same call twice
    assert (host(h.eval(ud, dev(pts))).view(np.int64) == out.view(np.int64)).all()
    # chunk edges: the base set repeated cyclically to each length; a point's bits do not depend on its position
    nb = len(pts)
    for npts in (1, 63, 65, C, C + 1, 2 * C + 3):
        idx = np.arange(npts) % nb
        o = host(h.eval(ud, dev(pts[idx])))
        assert o.shape == (nf, npts)
        assert within(o, value[:, idx], B[:, idx], dims, "npts = %d" % npts)
        assert (o.view(np.int64) == out[:, idx].view(np.int64)).all()
    h.destroy()


@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_scattered_values_scaled_nodes(dims, nf):
    pts, nn, flat = point_set(dims)
    value, B = truth(dims, nf, True)
    u = field(dims, nf, True)
    h = sp.ChebPoints(dims, nf)
    out = host(h.eval(dev(u), dev(pts)))
    assert within(out, value, B, dims, "scaled nodes")
    assert (out[:, :nn].view(np.int64) == u.reshape(nf, -1)[:, flat].view(np.int64)).all()
    h.destroy()


@pytest.mark.parametrize("dims,nf", [((17,), 3), ((4, 257), 3), ((5, 7, 9), 16), ((66, 65, 64), 3), ((6, 5, 4, 3), 3)], ids=case_ids)
def test_nan_and_inf_stay_at_their_point(dims, nf):
    pts, _, _ = point_set(dims)
    h = sp.ChebPoints(dims, nf)
    C = h.chunk
    idx = np.arange(C + 40) % len(pts)
    p = pts[idx].copy()
    ud = dev(field(dims, nf))
    clean = host(h.eval(ud, dev(p)))
    a, b = 20, C + 3                                      # one in each chunk
    p[a, 0] = np.nan
    p[b, -1] = np.inf
    out = host(h.eval(ud, dev(p)))
    assert np.isnan(out[:, [a, b]]).all()
    keep = np.ones(len(p), bool); keep[[a, b]] = False
    assert (out[:, keep].view(np.int64) == clean[:, keep].view(np.int64)).all()
    h.destroy()


def cheb_vandermonde(x, n):
    """T_k(x_j), k < n, in long double as cos(k arccos x)."""
    return np.cos(np.arange(n, dtype=LD)[None, :] * np.arccos(np.asarray(x, dtype=np.float64).astype(LD))[:, None])


@pytest.mark.parametrize("dims", [(17,), (1024,), (4, 257), (5, 7, 9), (33, 20, 17), (6, 5, 4, 3)], ids=case_ids)
def test_chebyshev_sums(dims):
    """Independent of the barycentric formula: u = sum a prod T_k sampled at the double nodes; the values at the points are the
    long-double Chebyshev sums.  Bar: (cap + sum (n_k - 1)^2) U sum |a| -- the second term is |T_k'| <= k^2 times a node's rounding
    U / 2, in every direction.  Loose by construction: a wrong node order, sign or end weight gives O(1)."""
    d = len(dims)
    rng = np.random.default_rng(SEED + 2)
    a = rng.standard_normal(dims)
    pts, _, _ = point_set(dims)
    pts = pts[(np.abs(pts) <= 1).all(axis=1)]

    def expand(mats):                                    # sum over k of a[k_0 ..] prod mats[k][., k_k], direction by direction
        t = a.astype(LD)
        for k, M in enumerate(mats):
            t = np.moveaxis(np.tensordot(M, t, axes=([1], [k])), 0, k)
        return t
    u = expand([cheb_vandermonde(sp.cgl_nodes(n), n) for n in dims]).astype(np.float64)
    V = [cheb_vandermonde(pts[:, k], n) for k, n in enumerate(dims)]
    t = np.moveaxis(np.tensordot(V[0], a.astype(LD), axes=([1], [0])), 0, 0)            # [p][k_1 ..]
    for k in range(d - 1, 0, -1):
        t = np.einsum("p...i,pi->p...", t, V[k])
    h = sp.ChebPoints(dims)
    out = host(h.eval(dev(u.ravel()), dev(pts)))[0]
    bar = (ref.cap(dims) + sum((n - 1) ** 2 for n in dims)) * U * np.abs(a).sum()
    err = float(np.abs(out.astype(LD) - t).max())
    print("%s: worst error %.3g U sum|a|, bar %.3g U sum|a|" % (case_ids(dims), err / (U * np.abs(a).sum()), bar / (U * np.abs(a).sum())))
    assert err <= bar
    h.destroy()


def grid_coords(dims, m, seed):
    rng = np.random.default_rng(SEED + seed)
    out = []
    for n, mk in zip(dims, m):
        x = rng.uniform(-1.0, 1.0, mk)
        if mk >= 3:
            xn = sp.cgl_nodes(n)
            x[0] = xn[n // 2]; x[1] = np.nextafter(xn[1], 2.0); x[2] = 1.0
        out.append(x)
    return out


def grid_truth(dims, nf, u, coords):
    """(value, B) of the tensor grid, shrinking directions first (the cheapest order for the long-double products)."""
    t = u.reshape((nf,) + tuple(dims)).astype(LD)
    b = np.abs(u).reshape((nf,) + tuple(dims))
    for k in sorted(range(len(dims)), key=lambda k: len(coords[k]) / dims[k]):
        R = ref.rows_ld(dims[k], coords[k])
        t = np.moveaxis(np.tensordot(R, t, axes=([1], [k + 1])), 0, k + 1)
        b = np.moveaxis(np.tensordot(np.abs(R).astype(np.float64), b, axes=([1], [k + 1])), 0, k + 1)
    return t, b


GRIDS = [((5, 7, 9), 16, (64, 3, 130)), ((5, 7, 9), 16, (1, 65, 1)), ((5, 7, 9), 16, (3, 1, 3)),
         ((33, 20, 17), 1, (65, 1, 64)), ((33, 20, 17), 1, (130, 3, 1)),
         ((66, 65, 64), 3, (1, 64, 65)), ((66, 65, 64), 3, (3, 130, 1)),
         ((4, 257), 3, (130, 65)), ((4, 257), 3, (1, 64)), ((4, 257), 3, (3, 1))]


@pytest.mark.parametrize("dims,nf,m", GRIDS, ids=case_ids)
def test_grids(dims, nf, m):
    u = field(dims, nf)
    coords = grid_coords(dims, m, 3)
    value, B = grid_truth(dims, nf, u, coords)
    h = sp.ChebPoints(dims, nf)
    h.reserve_grid(m)
    ud = dev(u)
    out = host(h.eval_grid(ud, [dev(c) for c in coords]))
    assert out.shape == (nf,) + tuple(m)
    assert within(out, value, B, dims, "grid " + case_ids(tuple(m)))
    assert (host(h.eval_grid(ud, [dev(c) for c in coords])).view(np.int64) == out.view(np.int64)).all()
    h.destroy()


@pytest.mark.parametrize("dims,nf", [((5, 7, 9), 16), ((33, 20, 17), 1), ((4, 257), 3)], ids=case_ids)
def test_grid_of_the_nodes_returns_the_field(dims, nf):
    u = field(dims, nf, True)
    h = sp.ChebPoints(dims, nf)
    out = host(h.eval_grid(dev(u), [dev(sp.cgl_nodes(n)) for n in dims]))
    assert (out.ravel().view(np.int64) == u.view(np.int64)).all()
    h.destroy()


@pytest.mark.parametrize("dims,dims_out", [((5, 7, 9), (7, 5, 12)), ((33, 20, 17), (20, 24, 9))], ids=case_ids)
def test_grid_against_resample(dims, dims_out):
    u = field(dims, 1)
    ud = dev(u)
    h = sp.ChebPoints(dims)
    out = host(h.eval_grid(ud, [dev(sp.cgl_nodes(n)) for n in dims_out]))
    rs = sp.Resample(dims, dims_out)
    y = host(rs.apply(ud, torch.empty(rs.size(1), dtype=torch.float64, device="cuda"))).reshape(dims_out)
    b = np.abs(u).reshape(dims)
    for k in range(len(dims)):
        b = np.moveaxis(np.tensordot(np.abs(sp.resample_matrix(dims[k], dims_out[k])), b, axes=([1], [k])), 0, k)
    assert (np.abs(out[0] - y) <= ref.cap(dims) * U * b).all()
    h.destroy(); rs.destroy()


def test_grid_larger_than_reserved_is_refused():
    dims = (5, 7, 9)
    h = sp.ChebPoints(dims)
    ud = dev(field(dims, 1))
    c = lambda m: [dev(np.linspace(-1, 1, k)) for k in m]
    # nothing reserved: the C call refuses
    assert sp.lib().cheb_points_eval_grid(h._h, ud.data_ptr(), ud.data_ptr(), sp._ints((1, 1, 1)), ud.data_ptr(), None) == 4
    h.reserve_grid((3, 4, 5))
    assert h.eval_grid(ud, c((3, 4, 5))).shape == (1, 3, 4, 5)
    assert h.eval_grid(ud, c((1, 4, 2))).shape == (1, 1, 4, 2)
    with pytest.raises(sp.ChebhipError) as e:
        h.eval_grid(ud, c((3, 5, 5)))
    assert e.value.code == 4 and "reserved" in str(e.value)
    with pytest.raises(sp.ChebhipError):
        h.reserve_grid((3, 0, 5))
    h.reserve_grid((3, 5, 5))
    assert h.eval_grid(ud, c((3, 5, 5))).shape == (1, 3, 5, 5)
    h.destroy()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sample_plane(axis):
    dims, nf = (9, 6, 7), 2
    ud = dev(field(dims, nf))
    for m in (None, 11):
        coords = [dev([0.3]) if k == axis else (dev(sp.cgl_nodes(n)) if m is None else torch.linspace(-1.0, 1.0, m, dtype=torch.float64, device="cuda"))
                  for k, n in enumerate(dims)]
        h = sp.ChebPoints(dims, nf)
        want = host(h.eval_grid(ud, coords))
        h.destroy()
        got = host(solve.sample_plane(sp, dims, ud, axis, 0.3, m=m))
        shape = tuple(c.numel() for k, c in enumerate(coords) if k != axis)
        assert got.shape == (nf,) + shape
        assert (got.view(np.int64) == want.squeeze(axis + 1).view(np.int64)).all()


def test_interface():
    dims, nf = (5, 4, 3), 2
    h = sp.ChebPoints(dims, nf)
    assert h.size() == 120 and h.chunk == 1024
    ud = dev(field(dims, nf))
    pts = dev(np.random.default_rng(SEED).uniform(-1, 1, (10, 3)))
    out = torch.full((nf, 10), float("nan"), dtype=torch.float64, device="cuda")
    assert h.eval(ud, pts, out=out) is out and np.isfinite(host(out)).all()
    assert h.eval(ud, pts[:0]).shape == (nf, 0)
    assert sp.lib().cheb_points_eval(h._h, ud.data_ptr(), pts.data_ptr(), 0, out.data_ptr(), None) == 0
    assert h.rows(1, pts[:0, 0].contiguous()).shape == (0, 4)
    with pytest.raises(ValueError):
        h.eval(ud, pts[:, :2].contiguous())
    with pytest.raises(sp.ChebhipError) as e:
        h.rows(3, pts[:, 0].contiguous())
    assert e.value.code == 2
    big = torch.zeros(200, dtype=torch.float64, device="cuda")                     # fields and output in one allocation
    with pytest.raises(sp.ChebhipError) as e:
        h.eval(big[:120], pts, out=big[110:130].view(nf, 10))
    assert e.value.code == 4 and "overlap" in str(e.value)
    assert h.eval(big[:120], pts, out=big[120:140].view(nf, 10)).shape == (nf, 10)
    with pytest.raises(sp.ChebhipError) as e:
        h.eval_grid(big[:120], [pts[:2, 0].contiguous()] * 3, out=big[116:132].view(nf, 2, 2, 2))
    assert e.value.code == 4
    g = torch.empty((nf, 2, 2, 2), dtype=torch.float64, device="cuda")
    assert h.eval_grid(ud, [pts[:2, k].contiguous() for k in range(3)], out=g) is g
    torch.cuda.synchronize()
    h.destroy()
    h.destroy()
