"""cheb_points_spread on the device (ChebPoints.spread), the transpose of the scattered evaluation, against the long-double truth and
the derived bar of tests/spread_ref.py, element by element: |g_i - truth_i| <= cap(dims, npts) U B_i.  Counts of points either side
of a k-step (4), an LDS chunk (16) and a tile (64, 128); the adversarial points of tests/test_gpu_points.py (uniform, corners,
nodes, neighbours of nodes, 0, 5e-324, |x| > 1) ordered so that every prefix mixes the kinds.  As there, the points beyond the cube
lie within 1e-7 of a face: the bar's Lambda(n) bounds the Lebesgue function on [-1, 1] only, beyond it the function grows like
T_N(|x|) and stays below Lambda(n) while |x| - 1 is small against 1 / N^2; further out the rows themselves, on the device and in
any double-precision model, lose the digits the bar counts on (test_extrapolation_far_outside checks |x| up to 1.5 without this
bar, against the composition of the same rows and against eval).  Also: the adjoint
identity with the library's own eval, exact scatter on nodes, NaN isolation and stale rows, passes, accumulate, the empty call, the
delta form through ChebModal.integrate, the rows + einsum composition, run-to-run bits, refusals."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import points_ref as pref
import spread_ref as ref

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = 20240229
LD = np.longdouble
U = ref.U

SHAPES = [(2,), (7,), (130,), (12, 9), (6, 130), (258, 6), (10, 9, 8), (6, 5, 34), (70, 6, 5), (33, 17, 16), (5, 4, 6, 5), (3, 2, 4, 3, 2)]
NFIELDS = (1, 3, 16)
NPTS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 129, 130)
NMAX = 130
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def point_set(dims):
    """NMAX points (NMAX, d): the kinds in turn, a uniform point first, so that every prefix holds generic points."""
    d = len(dims)
    rng = np.random.default_rng(SEED + 1 + sum(dims))
    xn = [sp.cgl_nodes(n) for n in dims]
    node = lambda: np.array([xn[k][rng.integers(0, dims[k])] for k in range(d)])
    uni = lambda: rng.uniform(-1.0, 1.0, d)
    pts = []
    for p in range(NMAX):
        kind = p % 10
        if kind in (0, 5):
            x = uni()
        elif kind == 1:
            x = node()
        elif kind == 2:
            x = np.where(rng.integers(0, 2, d) == 1, 1.0, -1.0)                   # a corner
        elif kind == 3:
            x = np.nextafter(node(), 2.0)
        elif kind == 4:
            x = np.nextafter(node(), -2.0)
        elif kind == 6:
            x = np.where(rng.integers(0, 2, d) == 1, node(), uni())               # some coordinates on nodes
        elif kind == 7:
            x = np.zeros(d) if (p // 10) % 2 == 0 else uni() * (rng.integers(0, 2, d) == 1)
        elif kind == 8:
            x = np.full(d, 5e-324) if (p // 10) % 2 == 0 else np.where(rng.integers(0, 2, d) == 1, 5e-324, uni())
        else:
            e = (0.0, 1e-13, 1e-10, 1e-7)[(p // 10) % 4]                          # |x| > 1: one ulp (e = 0) .. 1e-7 beyond a face
            x = uni(); x[rng.integers(0, d)] = np.nextafter(1.0 + e, 2.0) * (1.0 if rng.integers(0, 2) else -1.0)
        pts.append(x)
    return np.ascontiguousarray(np.stack(pts))


@functools.lru_cache(maxsize=None)
def outer_ld(dims):
    """(L, |L| in double): L[p][i] = prod_k l_k,p[i_k] of the point set, long double."""
    L = ref.outer(ref.rows_all_ld(dims, point_set(dims)))
    return L, np.abs(L).astype(np.float64)


def strengths(nf, scaled=False):
    rng = np.random.default_rng(SEED + 2 + nf)
    s = rng.standard_normal((nf, NMAX))
    if scaled:                                                                     # every point by 10^+100 or 10^-100
        s = s * np.where(rng.integers(0, 2, NMAX) == 1, 1e100, 1e-100)[None, :]
    return s


def truth(dims, s, npts, delta=False, first=0):
    """(truth, B) of the points first .. npts - 1 of the set."""
    L, A = outer_ld(dims)
    t = s[:, first:npts].astype(LD) @ L[first:npts]
    b = np.abs(s[:, first:npts]) @ A[first:npts]
    if delta:
        W = ref.weights_ld(dims)
        t, b = t / W, (b / W).astype(np.float64)
    return t, b


def spread(h, s, pts, **kw):
    return host(h.spread(dev(s), dev(pts), **kw)).reshape(h.nfields, -1)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("nf", NFIELDS)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_every_element_within_the_bar(dims, nf):
    pts = point_set(dims)
    L, A = outer_ld(dims)
    N = int(np.prod(dims))
    h = sp.ChebPoints(dims, nf)
    assert h.spread_pass() >= NMAX
    for scaled in (False, True):
        s = strengths(nf, scaled)
        t, b, done, worst = np.zeros((nf, N), dtype=LD), np.zeros((nf, N)), 0, 0.0
        for npts in NPTS:                                                          # the sets are prefixes: the truth grows with them
            t = t + s[:, done:npts].astype(LD) @ L[done:npts]
            b = b + np.abs(s[:, done:npts]) @ A[done:npts]
            done = npts
            g = spread(h, s[:, :npts], pts[:npts])
            assert g.shape == (nf, N)
            r = ref.worst_ratio(g, t, b, ref.cap(dims, npts))
            worst = max(worst, r)
            assert r <= 1.0, "npts = %d: worst error / bar = %.3g" % (npts, r)
        c = ref.cap(dims, NMAX)
        print("%s nf=%d %s: worst error / bar = %.3g (bar at %d points = %.0f U B)" % (ids(dims), nf, "scaled" if scaled else "N(0,1)", worst, NMAX, c))
    h.destroy()


@pytest.mark.parametrize("nf", NFIELDS)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_adjoint_of_the_library_eval(dims, nf):
    """sum_p eval(u)[f][p] s[f][p] = sum_i u[f][i] spread(s)[f][i] within the sum of eval's and spread's bars: same rows, layouts and
    field order (distinct fields and distinct strengths per field: a swapped order fails by O(1))."""
    pts = point_set(dims)
    N = int(np.prod(dims))
    u = np.random.default_rng(SEED + 3).standard_normal((nf, N))
    s = strengths(nf)
    h = sp.ChebPoints(dims, nf)
    ud = dev(u.ravel())
    rows = ref.rows_all_ld(dims, pts)
    for npts in (1, 17, NMAX):
        e = host(h.eval(ud, dev(pts[:npts])))
        g = spread(h, s[:, :npts], pts[:npts])
        lhs = (e.astype(LD) * s[:, :npts].astype(LD)).sum(axis=1)
        rhs = (u.astype(LD) * g.astype(LD)).sum(axis=1)
        _, Be = pref.values_ld(dims, nf, u.ravel(), [r[:npts] for r in rows])
        _, Bs = truth(dims, s, npts)
        bar = U * (pref.cap(dims) * (np.abs(s[:, :npts]) * Be).sum(axis=1) + ref.cap(dims, npts) * (np.abs(u) * Bs).sum(axis=1))
        print("%s nf=%d npts=%d: |lhs - rhs| / bar = %.3g" % (ids(dims), nf, npts, float((np.abs(lhs - rhs) / bar).max())))
        assert (np.abs(lhs - rhs) <= bar).all()
    h.destroy()


@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_points_on_nodes_scatter_exactly(dims):
    nf, d = 3, len(dims)
    rng = np.random.default_rng(SEED + 4)
    flat = rng.permutation(int(np.prod(dims)))[:20]                                # distinct nodes ...
    flat = np.concatenate([flat, flat[:6]])                                        # ... of which some hold two points (three would add in an order)
    idx = np.stack(np.unravel_index(flat, dims), axis=1)
    pts = np.stack([sp.cgl_nodes(n)[idx[:, k]] for k, n in enumerate(dims)], axis=1)
    s = rng.standard_normal((nf, len(pts))) * 10.0 ** rng.uniform(-100, 100, len(pts))[None, :]
    want = np.zeros((nf, int(np.prod(dims))))
    for f in range(nf):
        np.add.at(want[f], flat, s[f])
    h = sp.ChebPoints(dims, nf)
    g = spread(h, s, pts)
    assert (g == want).all()
    one = spread(h, s[:, :1], pts[:1])                                             # one point: s at its node bit for bit, zeros elsewhere
    assert (bits(one[:, flat[0]]) == bits(s[:, 0])).all()
    one[:, flat[0]] = 0.0
    assert (bits(one) == 0).all()
    h.destroy()


@pytest.mark.parametrize("dims", [(7,), (130,), (6, 130), (10, 9, 8), (70, 6, 5), (5, 4, 6, 5)], ids=ids)
def test_nan_isolation_and_stale_rows(dims):
    nf = 3
    pts = point_set(dims)
    s = strengths(nf)
    h = sp.ChebPoints(dims, nf)
    clean = spread(h, s, pts)
    bad = s.copy(); bad[1, 40] = np.nan
    g = spread(h, bad, pts)
    assert np.isnan(g[1]).all()
    assert (bits(g[[0, 2]]) == bits(clean[[0, 2]])).all()
    for k, v in ((0, np.nan), (len(dims) - 1, np.nan), (0, np.inf), (len(dims) - 1, -np.inf)):
        p = pts.copy(); p[77, k] = v
        assert np.isnan(spread(h, s, p)).all()
    # the same handle, fewer points.  First every point from 5 on gets NaN or infinite coordinates in every direction, so the slots
    # 5 .. 129 of the work memory hold NaN rows of every direction: the padded part of the short call's only chunk (slots 5 .. 15)
    # among them.  An operand that read a slot past the last point would give NaN (NaN times the other operand's 0)
    p = pts.copy(); p[5:] = np.where(np.arange(NMAX - 5)[:, None] % 2 == 0, np.nan, np.inf)
    assert np.isnan(spread(h, s, p)).all()
    g = spread(h, s[:, :5], pts[:5])
    t, b = truth(dims, s, 5)
    assert np.isfinite(g).all() and ref.worst_ratio(g, t, b, ref.cap(dims, 5)) <= 1.0
    h.destroy()


@pytest.mark.parametrize("dims,nf", [((130,), 3), ((6, 130), 1), ((10, 9, 8), 16), ((33, 17, 16), 3), ((3, 2, 4, 3, 2), 3)], ids=ids)
def test_passes(dims, nf):
    pts, s = point_set(dims), strengths(nf)
    t, b = truth(dims, s, NMAX)
    h = sp.ChebPoints(dims, nf)
    count = sp.lib().chebhip_launch_count
    try:
        for size, passes in ((130, 1), (65, 2), (26, 5)):
            sp.set_option("points_spread_pass", size)
            assert h.spread_pass() == size
            c0 = count()
            g = spread(h, s, pts)
            assert count() - c0 == 2 * passes                                      # rows and product, once a pass
            r = ref.worst_ratio(g, t, b, ref.cap(dims, NMAX))
            print("%s nf=%d, %d passes: worst error / bar = %.3g" % (ids(dims), nf, passes, r))
            assert r <= 1.0
            assert (bits(spread(h, s, pts)) == bits(g)).all()
    finally:
        sp.set_option("points_spread_pass", 0)
    assert h.spread_pass() >= NMAX
    h.destroy()


@pytest.mark.parametrize("dims,nf", [((7,), 3), ((258, 6), 1), ((10, 9, 8), 16), ((5, 4, 6, 5), 3)], ids=ids)
def test_accumulate(dims, nf):
    pts, s = point_set(dims), strengths(nf)
    t, b = truth(dims, s, NMAX)
    h = sp.ChebPoints(dims, nf)
    out0 = np.random.default_rng(SEED + 5).standard_normal(t.shape)
    try:
        for size in (0, 65):
            sp.set_option("points_spread_pass", size)
            out = dev(out0.ravel())
            assert h.spread(dev(s), dev(pts), out=out, accumulate=True) is out
            err = np.abs(host(out).reshape(t.shape).astype(LD) - (out0.astype(LD) + t))
            assert (err <= ref.cap(dims, NMAX) * U * b + U * np.abs(out0)).all()
    finally:
        sp.set_option("points_spread_pass", 0)
    with pytest.raises(ValueError):
        h.spread(dev(s), dev(pts), accumulate=True)
    h.destroy()


def test_empty_call():
    dims, nf = (5, 4, 3), 2
    h = sp.ChebPoints(dims, nf)
    pts = dev(np.zeros((0, 3)))
    s = dev(np.zeros((nf, 0)))
    out = torch.full((h.size(),), 7.0, dtype=torch.float64, device="cuda")
    assert h.spread(s, pts, out=out, accumulate=True) is out and (host(out) == 7.0).all()
    h.spread(s, pts, out=out)
    assert (bits(host(out)) == 0).all()
    assert (host(h.spread(s, pts)) == 0.0).all()
    assert sp.lib().cheb_points_spread(h._h, None, None, 0, None, 1, None) == 0
    h.destroy()


@pytest.mark.parametrize("dims,nf", [((7,), 3), ((130,), 1), ((12, 9), 3), ((258, 6), 1), ((10, 9, 8), 16), ((33, 17, 16), 3), ((5, 4, 6, 5), 3)], ids=ids)
def test_delta_is_a_point_source(dims, nf):
    """integrate(spread(s, delta=True) phi) = sum_p s_p phi(x_p) for phi the interpolant of random nodal values.  The element bar
    cap_delta U B_i / W_i carried through the integral is cap_delta U sum_i B_i |phi_i|; the integral's own rounding is
    (prod(dims) + 8) U sum_i W_i |g_i phi_i|, the bar of tests/test_gpu_modal.py."""
    pts, s = point_set(dims), strengths(nf)
    L, _ = outer_ld(dims)
    N = int(np.prod(dims))
    h = sp.ChebPoints(dims, nf)
    m = sp.ChebModal(dims, nf)
    phi = np.random.default_rng(SEED + 6).standard_normal((nf, N))
    W = ref.weights_ld(dims)
    for npts in (1, 17, NMAX):
        gd = h.spread(dev(s[:, :npts]), dev(pts[:npts]), delta=True)
        g = host(gd).reshape(nf, N)
        t, b = truth(dims, s, npts, delta=True)
        r = ref.worst_ratio(g, t, b, ref.cap(dims, npts, True))
        assert r <= 1.0
        integ = host(m.integrate(gd, dev(phi.ravel())))
        want = (s[:, :npts].astype(LD) * (L[:npts] @ phi.astype(LD).T).T).sum(axis=1)          # sum_p s_p phi(x_p)
        _, bp = truth(dims, s, npts)
        bar = U * (ref.cap(dims, npts, True) * (bp * np.abs(phi)).sum(axis=1) + (N + 8) * (W[None] * np.abs(g * phi)).sum(axis=1))
        print("%s nf=%d npts=%d delta: element ratio %.3g, integral error / bar = %.3g" % (ids(dims), nf, npts, r, float((np.abs(integ - want) / bar).max())))
        assert (np.abs(integ - want) <= bar).all()
    # the one-off wrapper gives the same bits
    ps = solve.point_sources(sp, dims, dev(pts), dev(s))
    assert ps.shape == (nf,) + tuple(dims)
    assert (bits(host(ps).reshape(nf, N)) == bits(g)).all()
    buf = torch.full((nf,) + tuple(dims), float("nan"), dtype=torch.float64, device="cuda")
    r = solve.point_sources(sp, dims, dev(pts), dev(s), out=buf)
    assert r.data_ptr() == buf.data_ptr() and (bits(host(buf).reshape(nf, N)) == bits(g)).all()
    with pytest.raises(ValueError):                                                # a non-contiguous out would be written through a copy
        solve.point_sources(sp, dims, dev(pts), dev(s), out=torch.empty((nf, 2 * N), dtype=torch.float64, device="cuda")[:, ::2])
    with pytest.raises(ValueError):
        solve.point_sources(sp, dims, dev(pts), dev(s[:, :5]))
    h.destroy(); m.destroy()


@pytest.mark.parametrize("dims,nf", [((7,), 3), ((6, 130), 3), ((10, 9, 8), 16), ((33, 17, 16), 1), ((5, 4, 6, 5), 3)], ids=ids)
def test_against_rows_and_einsum(dims, nf):
    pts, s = point_set(dims), strengths(nf)
    h = sp.ChebPoints(dims, nf)
    pd, sd = dev(pts), dev(s)
    R = [h.rows(k, pd[:, k].contiguous()) for k in range(len(dims))]
    letters = "ijklm"[:len(dims)]
    want = torch.einsum("fp," + ",".join("p" + c for c in letters) + "->f" + letters, sd, *R)
    g = h.spread(sd, pd).reshape(want.shape)
    torch.cuda.synchronize()
    assert float(torch.linalg.norm(g - want) / torch.linalg.norm(want)) <= 1e-10
    h.destroy()


@pytest.mark.parametrize("dims,nf", [((7,), 3), ((130,), 1), ((6, 130), 3), ((10, 9, 8), 16), ((5, 4, 6, 5), 3)], ids=ids)
def test_extrapolation_far_outside(dims, nf):
    """|x| = 1.001 .. 1.5 in one or all directions, where the bar of the other tests does not apply (see the module's text): spread
    extrapolates by the rows eval uses -- against the rows + einsum composition at the project's 1e-10 normwise, and the adjoint
    identity with the library's eval to the same 1e-10 of sum |s| |eval| + sum |u| |spread|."""
    d = len(dims)
    rng = np.random.default_rng(SEED + 8)
    pts = rng.uniform(-1.0, 1.0, (24, d))
    for p, x in enumerate((1.001, -1.001, 1.01, -1.1, 1.5, -1.5)):
        pts[p, p % d] = x                                                          # one direction outside
        pts[6 + p, :] = x                                                          # every direction outside
    s = rng.standard_normal((nf, len(pts)))
    h = sp.ChebPoints(dims, nf)
    pd, sd = dev(pts), dev(s)
    R = [h.rows(k, pd[:, k].contiguous()) for k in range(d)]
    letters = "ijklm"[:d]
    want = torch.einsum("fp," + ",".join("p" + c for c in letters) + "->f" + letters, sd, *R)
    g = h.spread(sd, pd)
    torch.cuda.synchronize()
    assert torch.isfinite(g).all()
    assert float(torch.linalg.norm(g.reshape(want.shape) - want) / torch.linalg.norm(want)) <= 1e-10
    u = rng.standard_normal((nf, int(np.prod(dims))))
    e = host(h.eval(dev(u.ravel()), pd))
    gh = host(g).reshape(nf, -1)
    lhs, rhs = (e.astype(LD) * s).sum(axis=1), (u.astype(LD) * gh).sum(axis=1)
    mag = (np.abs(e) * np.abs(s)).sum(axis=1) + (np.abs(u) * np.abs(gh)).sum(axis=1)
    assert (np.abs(lhs - rhs) <= 1e-10 * mag).all()
    h.destroy()


@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_bits_repeat(dims):
    nf = 3
    pts, s = dev(point_set(dims)), dev(strengths(nf, True))
    h = sp.ChebPoints(dims, nf)
    for npts in (17, NMAX):
        a = host(h.spread(s[:, :npts].contiguous(), pts[:npts]))
        b = host(h.spread(s[:, :npts].contiguous(), pts[:npts], out=torch.full((h.size(),), float("nan"), dtype=torch.float64, device="cuda")))
        assert (bits(a) == bits(b)).all()
    h2 = sp.ChebPoints(dims, nf)                                                   # another handle, the same bits
    assert (bits(host(h2.spread(s, pts))) == bits(b)).all()
    h.destroy(); h2.destroy()


def test_refusals():
    dims, nf = (5, 4, 3), 2
    h = sp.ChebPoints(dims, nf)
    L = sp.lib()
    pts = dev(np.random.default_rng(SEED).uniform(-1, 1, (10, 3)))
    s = dev(np.ones((nf, 10)))
    out = torch.zeros(h.size(), dtype=torch.float64, device="cuda")
    assert h.spread(s, pts, out=out) is out
    big = torch.zeros(200, dtype=torch.float64, device="cuda")                      # everything in one allocation
    with pytest.raises(sp.ChebhipError) as e:
        h.spread(big[110:130].view(nf, 10), pts, out=big[:120])
    assert e.value.code == 4 and "overlap" in str(e.value)
    with pytest.raises(sp.ChebhipError) as e:
        h.spread(s, big[100:130].view(10, 3), out=big[:120])
    assert e.value.code == 4 and "overlap" in str(e.value)
    big[120:140] = 1.0
    assert h.spread(big[120:140].view(nf, 10), pts, out=big[:120]) is not None     # adjacent is fine
    with pytest.raises(ValueError):
        h.spread(s, pts[:, :2].contiguous(), out=out)
    with pytest.raises(ValueError):
        h.spread(s[:1].contiguous(), pts, out=out)
    with pytest.raises((ValueError, AssertionError)):
        h.spread(s, pts, out=out[:100])
    assert L.cheb_points_spread(h._h, s.data_ptr(), pts.data_ptr(), -1, out.data_ptr(), 0, None) == 4
    assert b"negative" in L.chebhip_last_error()
    assert L.cheb_points_spread(h._h, s.data_ptr(), pts.data_ptr(), 10, out.data_ptr(), 8, None) == 4
    assert L.cheb_points_spread(h._h, None, pts.data_ptr(), 10, out.data_ptr(), 0, None) == 4
    assert L.cheb_points_spread(h._h, s.data_ptr(), pts.data_ptr(), 10, None, 0, None) == 4
    torch.cuda.synchronize()
    h.destroy()
