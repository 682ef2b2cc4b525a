"""First derivatives at points on the device (ChebPoints.drows, eval / spread / eval_grid with deriv, eval_grad,
solve.velocity_gradient) against the numpy long-double restatement of the derivative rows on the double node table
(tests/points_deriv_ref.py), element by element:  |out - truth_p| <= cap U B'_p,  B'_p = sum prod m_k |u| with m_k = the majorant
a in derivative directions and |l| elsewhere,  cap = sum_k (cap1(n_k) or cap1d(n_k) + n_k + 5)  (+ 1 where a scale multiplies);
spread takes spread_ref's bar with the derivative directions' terms.  cap1d is derived in points_deriv_ref.py by counting roundings.
The shapes and the adversarial point set are those of tests/test_gpu_points.py.  The long-double truth of spread holds one row of
prod(dims) values per point, so grids of more than 20 000 nodes take every eighth point of the set there (all its kinds remain).
Also: a point on a node against the differentiation matrix, NaN / Inf coordinates, run-to-run, position-to-position and
stream-to-stream bits, a clean call after a NaN call, gradient chunk edges, a handle whose chunk is one point, refusals."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import points_deriv_ref as dref
import points_ref as pref
import spread_ref as sref
import test_gpu_points as tp

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = tp.SEED
LD = np.longdouble
U = pref.U
CASES = tp.CASES
case_ids = tp.case_ids
dev, host, field, point_set = tp.dev, tp.host, tp.field, tp.point_set


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def unit(d, c):
    return tuple(1 if k == c else 0 for k in range(d))


def mixed(d):
    return (1, 1) + (0,) * (d - 2)


@functools.lru_cache(maxsize=None)
def truths(dims, nf, scaled):
    """{alpha: (value[f][p] long double, B'[f][p])} at the point set for zero, every unit multi-index and the mixed one.  Both row
    kinds of every direction are built once, and direction 0's two long-double products with the field, the expensive part, are
    shared by all of them; only the small results are kept."""
    d = len(dims)
    pts, _, _ = point_set(dims)
    u = field(dims, nf, scaled)
    rv, mv = dref.rows_kinds(dims, pts, (0,) * d)
    rd, md = dref.rows_kinds(dims, pts, (1,) * d)
    f0, f1 = dref.first_products(dims, nf, u, rv[0], mv[0]), dref.first_products(dims, nf, u, rd[0], md[0])
    out = {}
    for alpha in [(0,) * d] + [unit(d, c) for c in range(d)] + ([mixed(d)] if d > 1 else []):
        rows = [rd[k] if a else rv[k] for k, a in enumerate(alpha)]
        mags = [md[k] if a else mv[k] for k, a in enumerate(alpha)]
        t, b = f1 if alpha[0] else f0
        out[alpha] = dref.later_products(t, b, rows, mags)
    return out


def truth(dims, nf, scaled, alpha):
    return truths(dims, nf, scaled)[alpha]


def grad_truth(dims, nf, scaled, scale=None):
    """The truth of eval_grad with the value: (nf, d + 1, npts), and the caps of the d + 1 components."""
    d = len(dims)
    alphas = [unit(d, c) for c in range(d)] + [(0,) * d]
    tb = [truth(dims, nf, scaled, a) for a in alphas]
    t = np.stack([v for v, _ in tb], axis=1)
    b = np.stack([v for _, v in tb], axis=1)
    caps = np.array([dref.cap(dims, a, scale is not None and c < d) for c, a in enumerate(alphas)])
    if scale is not None:
        s = np.concatenate([np.asarray(scale, dtype=np.float64), [1.0]])
        t = t * s.astype(LD)[None, :, None]
        b = b * np.abs(s)[None, :, None]
    return t, b, caps


def within(out, t, b, c, what):
    r = dref.worst(out, t, b, c)
    print("%s: worst error / bar = %.3g (bar = %.0f U B')" % (what, r, c))
    return r <= 1.0


def grad_within(out, t, b, caps, what):
    return all(within(out[:, c], t[:, c], b[:, c], caps[c], "%s component %d" % (what, c)) for c in range(out.shape[1]))


@pytest.mark.parametrize("n", [2, 17, 64, 257, 1024])
def test_drows(n):
    h = sp.ChebPoints((n,))
    xn = sp.cgl_nodes(n)
    rng = np.random.default_rng(SEED + n)
    x = np.concatenate([rng.uniform(-1, 1, 300), xn, np.nextafter(xn, 2.0), np.nextafter(xn, -2.0), xn * (1 + 1e-13), xn * (1 - 1e-9),
                        xn * (1 - 1e-7), [0.0, 5e-324, 1.0, -1.0]])
    xd = dev(x)
    R = host(h.drows(0, xd))
    want, a = dref.drows_ld(n, x)
    assert R.shape == (x.size, n) and np.isfinite(R).all()
    ratio = float((np.abs(R.astype(LD) - want) / (U * a)).max())
    print("n = %d: worst entry error %.3g U a (cap1d = %.0f)" % (n, ratio, dref.cap1d(n)))
    assert (np.abs(R.astype(LD) - want) <= dref.cap1d(n) * U * a).all()
    twin = sp.deriv_matrix(n, x)
    assert (np.abs(R - twin) <= (dref.cap1d(n) + 1) * U * a.astype(np.float64)).all()
    assert (bits(host(h.drows(0, xd))) == bits(R)).all()
    bad = x.copy(); bad[5] = np.nan; bad[7] = -np.inf
    Rb = host(h.drows(0, dev(bad)))
    assert np.isnan(Rb[[5, 7]]).all()
    keep = np.ones(x.size, bool); keep[[5, 7]] = False
    assert (bits(Rb[keep]) == bits(R[keep])).all()
    assert h.drows(0, xd[:0]).shape == (0, n)
    h.destroy()


@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_eval_deriv(dims, nf):
    """Every unit multi-index, one mixed one and zero (bit for bit the plain call), N(0,1) fields."""
    d = len(dims)
    pts, _, _ = point_set(dims)
    h = sp.ChebPoints(dims, nf)
    ud, pd = dev(field(dims, nf)), dev(pts)
    plain = host(h.eval(ud, pd))
    assert (bits(host(h.eval(ud, pd, deriv=(0,) * d))) == bits(plain)).all()
    for alpha in [unit(d, c) for c in range(d)] + ([mixed(d)] if d > 1 else []):
        t, b = truth(dims, nf, False, alpha)
        out = host(h.eval(ud, pd, deriv=alpha))
        assert out.shape == (nf, len(pts))
        assert within(out, t, b, dref.cap(dims, alpha), "%s eval deriv %r" % (case_ids(dims), alpha))
        assert (bits(host(h.eval(ud, pd, deriv=alpha))) == bits(out)).all()
    assert (bits(host(h.eval(ud, pd))) == bits(plain)).all()
    h.destroy()


@pytest.mark.parametrize("scaled", [False, True], ids=["normal", "scaled_nodes"])
@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_eval_grad(dims, nf, scaled):
    """Every component within its bar, with and without the value and a scale; the value within the value bar of eval; the
    derivatives' bits do not depend on the flag, on a repeat, on the point's position or on the chunk it falls into."""
    d = len(dims)
    pts, _, _ = point_set(dims)
    h = sp.ChebPoints(dims, nf)
    ud, pd = dev(field(dims, nf, scaled)), dev(pts)
    t, b, caps = grad_truth(dims, nf, scaled)
    full = host(h.eval_grad(ud, pd, value=True))
    assert full.shape == (nf, d + 1, len(pts))
    assert grad_within(full, t, b, caps, "%s grad" % case_ids(dims))
    plain = host(h.eval(ud, pd))
    assert (np.abs(full[:, d].astype(LD) - plain.astype(LD)) <= 2 * pref.cap(dims) * U * b[:, d]).all()
    g = host(h.eval_grad(ud, pd))
    assert g.shape == (nf, d, len(pts)) and (bits(g) == bits(full[:, :d])).all()
    assert (bits(host(h.eval_grad(ud, pd, value=True))) == bits(full)).all()
    # the derived bars also hold for the d calls of eval(deriv = e_c) (scaled nodes: here; N(0,1): test_eval_deriv)
    if scaled:
        for c in range(d):
            assert within(host(h.eval(ud, pd, deriv=unit(d, c))), t[:, c], b[:, c], caps[c], "%s scaled eval deriv %d" % (case_ids(dims), c))
    scale = [2.0 / (0.7 + 0.6 * k) for k in range(d)]
    ts, bs, cs = grad_truth(dims, nf, scaled, scale)
    for value in (False, True):
        o = host(h.eval_grad(ud, pd, value=value, scale=scale))
        nc = d + (1 if value else 0)
        assert grad_within(o, ts[:, :nc], bs[:, :nc], cs[:nc], "%s grad scale value=%d" % (case_ids(dims), value))
        if value:
            assert (bits(o[:, d]) == bits(full[:, d])).all()
    # gradient chunk edges: the base set repeated cyclically; a point's bits do not depend on its position
    H = max(1, h.chunk // 2)
    for npts in (1, 63, 65, H, H + 1, 2 * H + 3):
        idx = np.arange(npts) % len(pts)
        o = host(h.eval_grad(ud, dev(pts[idx]), value=True))
        assert o.shape == (nf, d + 1, npts)
        assert (bits(o) == bits(full[:, :, idx])).all()
    h.destroy()


def spread_points(dims):
    pts, _, _ = point_set(dims)
    return pts if int(np.prod(dims)) <= 20000 else np.ascontiguousarray(pts[::8])


@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_spread_deriv(dims, nf):
    """The long-double sum, with and without delta and accumulate, and the adjoint identity with the library's eval(deriv)."""
    d = len(dims)
    pts = spread_points(dims)
    npts, N = len(pts), int(np.prod(dims))
    rng = np.random.default_rng(SEED + 11)
    s = rng.standard_normal((nf, npts))
    u = field(dims, nf)
    h = sp.ChebPoints(dims, nf)
    sd, pd, ud = dev(s), dev(pts), dev(u)
    alphas = [unit(d, 0)] + ([unit(d, d - 1)] if N <= 20000 else []) + ([mixed(d)] if d > 1 else [])
    for alpha in dict.fromkeys(alphas):
        rows, mags = dref.rows_kinds(dims, pts, alpha)
        Lm, Am = sref.outer(rows), sref.outer(mags)
        t = s.astype(LD) @ Lm
        b = np.abs(s) @ Am
        g = host(h.spread(sd, pd, deriv=alpha)).reshape(nf, N)
        c = dref.spread_cap(dims, npts, alpha)
        assert within(g, t, b, c, "%s spread deriv %r" % (case_ids(dims), alpha))
        assert (bits(host(h.spread(sd, pd, deriv=alpha)).reshape(nf, N)) == bits(g)).all()
        # accumulate: twice the points in two calls against one sum of 2 npts terms
        base = rng.standard_normal(nf * N)
        acc = host(h.spread(sd, pd, out=dev(base), accumulate=True, deriv=alpha)).reshape(nf, N)
        assert within(acc, t + base.reshape(nf, N).astype(LD), b + np.abs(base).reshape(nf, N), c + 1, "%s accumulate" % case_ids(dims))
        # delta: divided by the Clenshaw-Curtis weights
        W = sref.weights_ld(dims)
        gd = host(h.spread(sd, pd, delta=True, deriv=alpha)).reshape(nf, N)
        assert within(gd, t / W, (b / W).astype(np.float64), dref.spread_cap(dims, npts, alpha, True), "%s delta" % case_ids(dims))
        # <spread_deriv s, u> = <s, eval_deriv u>, each side within its own bar
        e = host(h.eval(ud, pd, deriv=alpha))
        lhs = (e.astype(LD) * s.astype(LD)).sum(axis=1)
        rhs = (g.astype(LD) * u.reshape(nf, N).astype(LD)).sum(axis=1)
        Be = np.abs(u.reshape(nf, N)) @ Am.T
        bar = U * (dref.cap(dims, alpha) * (np.abs(s) * Be).sum(axis=1) + c * (np.abs(u.reshape(nf, N)) * b).sum(axis=1))
        print("%s %r: |lhs - rhs| / bar = %.3g" % (case_ids(dims), alpha, float((np.abs(lhs - rhs) / bar).max())))
        assert (np.abs(lhs - rhs) <= bar).all()
    plain = host(h.spread(sd, pd))
    assert (bits(host(h.spread(sd, pd, deriv=(0,) * d))) == bits(plain)).all()
    h.destroy()


GRIDS = [((5, 7, 9), 16, (64, 3, 130), (0, 1, 0)), ((5, 7, 9), 16, (1, 65, 1), (1, 0, 1)), ((33, 20, 17), 1, (65, 1, 64), (1, 0, 0)),
         ((66, 65, 64), 3, (3, 130, 1), (0, 0, 1)), ((4, 257), 3, (130, 65), (0, 1)), ((4, 257), 3, (3, 1), (1, 1)),
         ((257, 4), 1, (65, 3), (1, 0)), ((6, 5, 4, 3), 3, (3, 4, 5, 2), (0, 1, 1, 0))]


@pytest.mark.parametrize("dims,nf,m,alpha", GRIDS, ids=case_ids)
def test_grids(dims, nf, m, alpha):
    """eval_grid(deriv) against the dense long-double rows, direction by direction."""
    u = field(dims, nf)
    coords = tp.grid_coords(dims, m, 3)
    t = u.reshape((nf,) + tuple(dims)).astype(LD)
    b = np.abs(u).reshape((nf,) + tuple(dims))
    for k in sorted(range(len(dims)), key=lambda k: len(coords[k]) / dims[k]):
        if alpha[k]:
            R, A = dref.drows_ld(dims[k], coords[k])
            A = A.astype(np.float64)
        else:
            R = pref.rows_ld(dims[k], coords[k])
            A = np.abs(R).astype(np.float64)
        t = np.moveaxis(np.tensordot(R, t, axes=([1], [k + 1])), 0, k + 1)
        b = np.moveaxis(np.tensordot(A, b, axes=([1], [k + 1])), 0, k + 1)
    h = sp.ChebPoints(dims, nf)
    ud, cd = dev(u), [dev(c) for c in coords]
    out = host(h.eval_grid(ud, cd, deriv=alpha))
    assert out.shape == (nf,) + tuple(m)
    assert within(out, t, b, dref.cap(dims, alpha), "%s grid %s deriv %r" % (case_ids(dims), case_ids(tuple(m)), alpha))
    assert (bits(host(h.eval_grid(ud, cd, deriv=alpha))) == bits(out)).all()
    assert (bits(host(h.eval_grid(ud, cd, deriv=(0,) * len(dims)))) == bits(host(h.eval_grid(ud, cd)))).all()
    h.destroy()


@pytest.mark.parametrize("axis", [0, 2])
def test_sample_plane_deriv(axis):
    dims, nf = (9, 6, 7), 2
    ud = dev(field(dims, nf))
    alpha = (0, 1, 0)
    coords = [dev([0.3]) if k == axis else dev(sp.cgl_nodes(n)) for k, n in enumerate(dims)]
    h = sp.ChebPoints(dims, nf)
    want = host(h.eval_grid(ud, coords, deriv=alpha))
    h.destroy()
    got = host(solve.sample_plane(sp, dims, ud, axis, 0.3, deriv=alpha))
    assert (bits(got) == bits(want.squeeze(axis + 1))).all()


@pytest.mark.parametrize("n", [17, 64, 257])
def test_a_point_on_a_node_takes_the_differentiation_matrix(n):
    xn = sp.cgl_nodes(n).astype(LD)
    j = np.arange(n)
    c = np.where((j == 0) | (j == n - 1), LD(2), LD(1))
    with np.errstate(divide="ignore"):
        D = (c[:, None] / c[None, :]) * np.where((j[:, None] + j[None, :]) & 1, LD(-1), LD(1)) / (xn[:, None] - xn[None, :])
    D[j, j] = 0
    A = np.abs(D)
    A[j, j] = A.sum(axis=1)
    D[j, j] = -D.sum(axis=1)
    u = field((n,), 1)
    h = sp.ChebPoints((n,))
    pd = dev(sp.cgl_nodes(n)[:, None])
    bar = dref.cap((n,), (1,)) * U * (A.astype(np.float64) @ np.abs(u))
    for out in (host(h.eval(dev(u), pd, deriv=(1,)))[0], host(h.eval_grad(dev(u), pd))[0, 0]):
        assert (np.abs(out.astype(LD) - D @ u.astype(LD)) <= bar).all()
    h.destroy()


@pytest.mark.parametrize("dims,nf", [((17,), 3), ((4, 257), 3), ((5, 7, 9), 16), ((66, 65, 64), 3), ((6, 5, 4, 3), 3)], ids=case_ids)
def test_nan_and_inf_stay_at_their_point(dims, nf):
    """One bad coordinate in each of two gradient chunks; afterwards a clean call gives the bits of a fresh handle."""
    d = len(dims)
    pts, _, _ = point_set(dims)
    h = sp.ChebPoints(dims, nf)
    H = max(1, h.chunk // 2)
    idx = np.arange(H + 40) % len(pts)
    p = pts[idx].copy()
    ud = dev(field(dims, nf))
    alpha = unit(d, d - 1)
    clean = host(h.eval_grad(ud, dev(p), value=True))
    clean_e = host(h.eval(ud, dev(p), deriv=alpha))
    a, b = 20, H + 3
    q = p.copy()
    q[a, 0] = np.nan
    q[b, -1] = np.inf
    out = host(h.eval_grad(ud, dev(q), value=True))
    out_e = host(h.eval(ud, dev(q), deriv=alpha))
    assert np.isnan(out[:, :, [a, b]]).all() and np.isnan(out_e[:, [a, b]]).all()
    keep = np.ones(len(p), bool); keep[[a, b]] = False
    assert (bits(out[:, :, keep]) == bits(clean[:, :, keep])).all()
    assert (bits(out_e[:, keep]) == bits(clean_e[:, keep])).all()
    again = host(h.eval_grad(ud, dev(p), value=True))
    fresh = sp.ChebPoints(dims, nf)
    assert (bits(again) == bits(clean)).all() and (bits(host(fresh.eval_grad(ud, dev(p), value=True))) == bits(clean)).all()
    fresh.destroy()
    h.destroy()


@pytest.mark.parametrize("dims,nf", [((17,), 3), ((5, 7, 9), 16), ((33, 20, 17), 1), ((6, 5, 4, 3), 3)], ids=case_ids)
def test_a_second_stream_gives_the_same_bits(dims, nf):
    d = len(dims)
    pts, _, _ = point_set(dims)
    h = sp.ChebPoints(dims, nf)
    ud, pd = dev(field(dims, nf)), dev(pts)
    sd = dev(np.random.default_rng(SEED + 12).standard_normal((nf, len(pts))))
    alpha = unit(d, 0)
    first = [host(h.eval_grad(ud, pd, value=True)), host(h.eval(ud, pd, deriv=alpha)), host(h.spread(sd, pd, deriv=alpha))]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = [h.eval_grad(ud, pd, value=True), h.eval(ud, pd, deriv=alpha), h.spread(sd, pd, deriv=alpha)]
    side.synchronize()
    for x, y in zip(first, second):
        assert (bits(x) == bits(host(y))).all()
    h.destroy()


def test_a_chunk_of_one_point():
    """A first direction of two nodes under 32 MiB of field: the work memory holds one point, and a gradient takes one pass of the
    eval pipeline per component."""
    dims, nf = (2, 1024, 1024, 2), 1
    d = len(dims)
    h = sp.ChebPoints(dims, nf)
    assert h.chunk == 1
    rng = np.random.default_rng(SEED + 13)
    u = rng.standard_normal(int(np.prod(dims)))
    xn = [sp.cgl_nodes(n) for n in dims]
    pts = np.array([[0.3, -0.7, 0.2, 0.9], [xn[0][1], xn[1][5], xn[2][1000], xn[3][0]], [0.5, np.nextafter(xn[1][7], 2.0), -0.1, 0.0]])
    scale = [2.0, 0.5, 3.0, 1.25]
    alphas = [unit(d, c) for c in range(d)] + [(0,) * d]
    ud, pd = dev(u), dev(pts)
    out = host(h.eval_grad(ud, pd, value=True, scale=scale))
    assert out.shape == (1, d + 1, 3)
    for c, alpha in enumerate(alphas):
        rows, mags = dref.rows_kinds(dims, pts, alpha)
        t, b = dref.values_ld(dims, nf, u, rows, mags)
        s = scale[c] if c < d else 1.0
        assert within(out[:, c], t * LD(s), b * s, dref.cap(dims, alpha, c < d), "chunk of one point, component %d" % c)
    assert (bits(host(h.eval_grad(ud, pd, scale=scale))) == bits(out[:, :d])).all()
    h.destroy()


def test_velocity_gradient_of_a_linear_field():
    """u_i = sum_j A_ij x_j on the nodes: the tensor is A_ij s_j within the bar (the interpolant of a linear function on the rounded
    nodes is linear up to the node-rounding term, well inside it)."""
    dims = (9, 8, 7)
    d = len(dims)
    rng = np.random.default_rng(SEED + 14)
    A = rng.standard_normal((d, d))
    X = np.stack(np.meshgrid(*[sp.cgl_nodes(n) for n in dims], indexing="ij"))                 # (d, dims)
    vel = np.einsum("ij,j...->i...", A, X).ravel()
    pts, _, _ = point_set(dims)
    for scale in (None, [2.0 / 3.0, 2.0, 0.25]):
        G = host(solve.velocity_gradient(sp, dims, dev(vel), dev(pts), scale=scale))
        assert G.shape == (len(pts), d, d)
        for j in range(d):
            rows, mags = dref.rows_kinds(dims, pts, unit(d, j))
            _, b = dref.values_ld(dims, d, vel, rows, mags)
            s = 1.0 if scale is None else scale[j]
            bar = dref.cap(dims, unit(d, j), scale is not None) * U * b * abs(s)           # (d, npts)
            assert (np.abs(G[:, :, j].T - (A[:, j] * s)[:, None]) <= bar).all()


def test_refusals():
    dims, nf = (5, 4, 3), 2
    h = sp.ChebPoints(dims, nf)
    ud = dev(field(dims, nf))
    pts = dev(np.random.default_rng(SEED).uniform(-1, 1, (10, 3)))
    sd = dev(np.ones((nf, 10)))
    for bad in ((0, 2, 0), (0, -1, 0)):
        for call in (lambda: h.eval(ud, pts, deriv=bad), lambda: h.spread(sd, pts, deriv=bad),
                     lambda: h.eval_grid(ud, [pts[:2, k].contiguous() for k in range(3)], deriv=bad)):
            with pytest.raises(sp.ChebhipError) as e:
                call()
            assert e.value.code == 4 and "must be 0 or 1" in str(e.value)
    with pytest.raises(ValueError):
        h.eval(ud, pts, deriv=(1, 0))
    with pytest.raises(ValueError):
        h.eval_grad(ud, pts, scale=[1.0, 2.0])
    with pytest.raises(ValueError):
        h.eval_grad(ud, pts[:, :2].contiguous())
    for bad in ([1.0, float("inf"), 1.0], [float("nan"), 1.0, 1.0]):
        with pytest.raises(sp.ChebhipError) as e:
            h.eval_grad(ud, pts, scale=bad)
        assert e.value.code == 4 and "finite" in str(e.value)
    L = sp.lib()
    out = torch.empty((nf, 4, 10), dtype=torch.float64, device="cuda")
    assert L.cheb_points_eval_grad(h._h, ud.data_ptr(), pts.data_ptr(), 10, None, 2, out.data_ptr(), None) == 4      # unknown flag
    assert L.cheb_points_eval_grad(h._h, ud.data_ptr(), pts.data_ptr(), -1, None, 0, out.data_ptr(), None) == 4
    assert L.cheb_points_eval_grad(h._h, ud.data_ptr(), pts.data_ptr(), 0, None, 0, None, None) == 0
    assert L.cheb_points_eval_grad(h._h, None, pts.data_ptr(), 10, None, 0, out.data_ptr(), None) == 4
    big = torch.zeros(400, dtype=torch.float64, device="cuda")                     # fields and output in one allocation
    with pytest.raises(sp.ChebhipError) as e:
        h.eval_grad(big[:120], pts, out=big[100:160].view(nf, 3, 10))
    assert e.value.code == 4 and "overlap" in str(e.value)
    assert h.eval_grad(big[:120], pts, out=big[120:180].view(nf, 3, 10)).shape == (nf, 3, 10)
    with pytest.raises(sp.ChebhipError) as e:
        h.drows(3, pts[:, 0].contiguous())
    assert e.value.code == 2
    assert h.eval_grad(ud, pts[:0]).shape == (nf, 3, 0)
    assert h.eval(ud, pts[:0], deriv=(1, 0, 0)).shape == (nf, 0)
    torch.cuda.synchronize()
    h.destroy()
