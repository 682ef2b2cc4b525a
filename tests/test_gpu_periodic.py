"""Periodic (Fourier) directions on the device: ChebGrad, ChebModal and HelmholtzSolver handles with periodic
directions against long-double restatements (periodic_ref.py, fdm_ref.py, grad_ref.py, linewise.py).

  ChebGrad         grad, div, laplacian per element with the bar (K + 8 + T) 2^-53 sum B of grad_ref.py; a NaN stays in its lines;
                   periodic=None / all-False is ChebGrad(dims, scale) bit for bit.
  ChebModal        forward then backward, single modes, filters: per element against the long-double chain of the host matrices,
                   bar sum_steps (n_k + 8) 2^-53 (|M| .. |M| |x|); integrals of trigonometric products: exact in long double, the
                   device within (N + 8 + d) 2^-53 sum w |u v|; the same bits from run to run.
  HelmholtzSolver  the steps by hand give the solve bit for bit; every step within fdm_ref.step_cap; the solve within 16 x the two
                   double restatements; NaN containment per line and per stacked field.
  solve_full       boundary rows to rounding, unknown nodes = solve(lifted f) bit for bit, sizes, aliasing.
  the two modules  the residual of the solve under ChebGrad.laplacian at most 16 x that of the all-wall Dirichlet handle.
  singular, known answer, argument errors.

Where PERIODIC_RATIOS_OUT names a file the measured figures are written there (profiles/periodic/ratios.txt)."""
import functools
import itertools
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import linewise as lw
import fdm_ref as fr
import grad_ref as gr
import periodic_ref as pr

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
LD = np.longdouble
U = 2.0 ** -53
SEED = 20261020
MARGIN = 16.0
RATIOS = []


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("PERIODIC_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            for line in RATIOS:
                f.write(line + "\n")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().reshape(-1)


def new(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and v and isinstance(v[0], (int, np.integer)) else str(v)

# the smallest shapes that reach every route: odd and even lines, strided and contiguous periodic lines, the one-launch z solve
# (last direction periodic, 96 unknowns), a 66-point strided periodic line, the longest periodic line (256)
SHAPES_12 = [(8,), (9,), (16, 9), (12, 16)]
SHAPES_3 = [(16, 9, 12), (7, 6, 16), (6, 5, 96), (6, 66, 5), (256, 4, 3)]
MASKS_3 = [(1, 0, 1), (0, 1, 0), (1, 1, 1), (0, 0, 1)]


def masks(d, all_false=False):
    if d == 3:
        return MASKS_3
    return [m for m in itertools.product((0, 1), repeat=d) if all_false or any(m)]


GRID = [(dims, m) for dims in SHAPES_12 + SHAPES_3 for m in masks(len(dims)) if all(n <= 256 for n, p in zip(dims, m) if p)]
SCALE = {1: (0.75,), 2: (0.5, 2.0), 3: (0.5, 1.0, 2.0), 4: (0.5, 1.0, 2.0, 1.5)}


# =================================================================================================================================
# ChebGrad
# =================================================================================================================================
def grad_inputs(shape, seed):
    ax = len(shape) - 1
    return {"noise": lw.noise(shape, ax, seed), "scaled": lw.scaled(shape, ax, seed), "impulse": lw.impulse(shape, ax, seed % 7)}


@pytest.mark.parametrize("dims,mask", GRID, ids=ids)
def test_grad_div_laplacian_per_element(dims, mask):
    d = len(dims)
    scale = SCALE[d]
    h = sp.ChebGrad(dims, scale, periodic=mask)
    assert h.periodic == tuple(bool(p) for p in mask)
    for name, x in grad_inputs((2 * d,) + dims, SEED + sum(dims)).items():
        dv = pr.derivs(sp, dims, mask, x)
        xd = dev(x)
        for op, nunits, nin in (("grad", 2, 2), ("div", 2, 2 * d)):
            t, W = gr.first_order(op, dims, scale, (dv[0][:nin], dv[1][:nin]), nunits)
            y = host(getattr(h, op)(xd[:nin * h.N])).reshape(t.shape)
            r = gr.ratio(y, t, W)
            print("%s %s %s %s: %.3f of the bar" % (ids(dims), mask, op, name, r))
            assert r <= 1.0, (op, name, r)
        t, W = pr.laplacian(sp, dims, mask, scale, x[:2])
        y = host(h.laplacian(xd[:2 * h.N])).reshape(t.shape)
        r = gr.ratio(y, t, W)
        print("%s %s laplacian %s: %.3f of the bar" % (ids(dims), mask, name, r))
        assert r <= 1.0, ("laplacian", name, r)
    h.destroy()


@pytest.mark.parametrize("dims,mask", [((9,), (1,)), ((12, 16), (1, 1)), ((16, 9, 12), (1, 0, 1)), ((6, 5, 96), (0, 0, 1))], ids=ids)
def test_grad_nan_stays_in_its_lines(dims, mask):
    """One NaN node: output k of grad changes only on the line along k through that node; the Laplacian only on the d lines."""
    d = len(dims)
    h = sp.ChebGrad(dims, periodic=mask)
    x = np.random.default_rng(SEED).standard_normal(dims)
    node = tuple(n // 3 for n in dims)
    xb = x.copy()
    xb[node] = np.nan
    y, yb = host(h.grad(dev(x))).reshape((d,) + dims), host(h.grad(dev(xb))).reshape((d,) + dims)
    l, lb = host(h.laplacian(dev(x))).reshape(dims), host(h.laplacian(dev(xb))).reshape(dims)
    touched = np.zeros(dims, dtype=bool)
    for k in range(d):
        line = np.zeros(dims, dtype=bool)
        line[tuple(slice(None) if m == k else node[m] for m in range(d))] = True
        assert np.array_equal(yb[k][~line], y[k][~line]), k
        assert np.isnan(yb[k][line]).any()
        touched |= line
    assert np.array_equal(lb[~touched], l[~touched])
    h.destroy()


@pytest.mark.parametrize("dims", [(9,), (16, 9), (16, 9, 12)], ids=ids)
def test_grad_without_periodic_direction_keeps_its_bits(dims):
    d = len(dims)
    x = dev(np.random.default_rng(SEED + 1).standard_normal((d,) + dims))
    h0 = sp.ChebGrad(dims, SCALE[d])
    want = [host(h0.grad(x)), host(h0.div(x)), host(h0.laplacian(x))]
    for per in (None, (False,) * d):
        h = sp.ChebGrad(dims, SCALE[d], periodic=per)
        got = [host(h.grad(x)), host(h.div(x)), host(h.laplacian(x))]
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        h.destroy()
    h0.destroy()


# =================================================================================================================================
# ChebModal
# =================================================================================================================================
def modal_mats(dims, mask, which):
    return [sp.fourier_modal_matrix(n, which) if p else sp.modal_matrix(n, which) for n, p in zip(dims, mask)]


def chain_ld(mats, x):
    """(truth, A, cap): the matrices (double, as uploaded) applied in order along their directions in long double; A the same chain
    of absolute values on |x|; cap = sum of (n_k + 8) over the steps.  First order: step s errs by at most (n_k + 8) 2^-53 |M_s| |its
    input|, and what follows it is bounded by the absolute chain."""
    t, A, cap = np.asarray(x).astype(LD), np.abs(np.asarray(x, dtype=np.float64)), 0
    for k, M in mats:
        t = np.moveaxis(np.tensordot(M.astype(LD), t, axes=([1], [k + 1])), 0, k + 1)
        A = np.moveaxis(np.tensordot(np.abs(M), A, axes=([1], [k + 1])), 0, k + 1)
        cap += M.shape[1] + 8
    return t, A, cap


@pytest.mark.parametrize("dims,mask", GRID, ids=ids)
def test_modal_round_trip_and_repeatability(dims, mask):
    nf = 3
    m = sp.ChebModal(dims, nf, periodic=mask)
    x = np.random.default_rng(SEED + 2 + sum(dims)).standard_normal((nf,) + dims)
    T, B = modal_mats(dims, mask, "forward"), modal_mats(dims, mask, "backward")
    xd = dev(x)
    a = m.forward(xd, new(m.size()))
    y = host(m.backward(a, new(m.size()))).reshape(x.shape)
    a = host(a).reshape(x.shape)
    t, A, cap = chain_ld(list(enumerate(T)), x)
    r = lw.worst(a, t, cap * A)[0]
    assert r <= 1.0, ("forward", r)
    t, A, cap = chain_ld(list(enumerate(T)) + list(enumerate(B)), x)
    r2 = lw.worst(y, t, cap * A)[0]
    print("%s %s: forward %.3f, round trip %.3f of the bar" % (ids(dims), mask, r, r2))
    assert r2 <= 1.0, ("round trip", r2)
    # ... and the chain's truth is the field itself: T B = I to the rounding of the entries
    assert np.abs(t - x.astype(LD)).max() <= cap * U * A.max()
    a2 = host(m.forward(xd, new(m.size()))).reshape(x.shape)
    assert np.array_equal(a, a2)
    I1, I2 = host(m.integrate(xd)), host(m.integrate(xd))
    assert np.array_equal(I1, I2)
    m.destroy()


@pytest.mark.parametrize("dims,mask", [((8,), (1,)), ((9,), (1,)), ((12, 16), (1, 1)), ((16, 9, 12), (1, 0, 1)), ((7, 6, 16), (1, 1, 1))], ids=ids)
def test_modal_single_modes(dims, mask):
    """A product of single modes (amplitude 1) has the coefficient 1 at its position and nothing elsewhere; on a wall direction the
    mode is a Chebyshev polynomial."""
    d = len(dims)
    rng = np.random.default_rng(SEED + 3)
    m = sp.ChebModal(dims, 1, periodic=mask)
    T = modal_mats(dims, mask, "forward")
    for trial in range(4):
        pos = tuple(int(rng.integers(0, n)) for n in dims)
        vec = []
        for n, p, q in zip(dims, mask, pos):
            if p:
                k, kind = sp.fourier_modes(n)[q]
                vec.append(pr.mode_vector(n, k, kind).astype(np.float64))
            else:
                vec.append(sp.modal_matrix(n, "backward")[:, q])
        u = vec[0]
        for v in vec[1:]:
            u = np.multiply.outer(u, v)
        a = host(m.forward(dev(u), new(m.size()))).reshape(dims)
        _, A, cap = chain_ld(list(enumerate(T)), u[None])
        want = np.zeros(dims)
        want[pos] = 1.0
        # (the sampled mode: one rounding per factor and d - 1 for their product)
        assert np.all(np.abs(a - want) <= (cap + 2 * d) * U * A[0]), (pos, np.abs(a - want).max())
    m.destroy()


def trig(n, k, phase):
    """cos(pi k (x + 1) + phase) at the n periodic nodes, long double: pi k (x_j + 1) = 2 pi k j / n, reduced in integers."""
    j = np.arange(n)
    return pr.cos_pi(2 * k * j, n) * np.cos(LD(phase)) - pr.sin_pi(2 * k * j, n) * np.sin(LD(phase))


def cheb_T(n, a):
    return pr.cos_pi(a * np.arange(n), n - 1)                      # T_a(cos(pi j / (n - 1)))


@pytest.mark.parametrize("dims,mask", [((8,), (1,)), ((9,), (1,)), ((16, 9), (1, 0)), ((12, 16), (1, 1)), ((16, 9, 12), (1, 0, 1)), ((256, 4, 3), (1, 0, 1))], ids=ids)
def test_modal_integrates_trigonometric_products_exactly(dims, mask):
    """u v with u, v single trigonometric modes of total degree < n on the periodic directions (Chebyshev polynomials of total
    degree <= n - 1 on the wall ones): the quadrature is exact -- in long double on long-double samples it gives the analytic
    integral; the device is within (N + 8 + d) 2^-53 sum w |u v| of the long-double quadrature of ITS (double) samples."""
    d = len(dims)
    N = int(np.prod(dims))
    m = sp.ChebModal(dims, 1, periodic=mask)
    for ku in (0, 1, 2):
        fu, fv, exact, w = [], [], LD(1), []
        for n, p in zip(dims, mask):
            if p:
                k1 = min(ku + 1, (n - 1) // 2)
                k2 = k1 if ku != 1 else max(k1 - 1, 0)
                p1, p2 = LD(0.3), LD(1.1)
                fu.append(trig(n, k1, p1)); fv.append(trig(n, k2, p2))
                # int_-1^1 cos(pi k1 (x+1) + p1) cos(pi k2 (x+1) + p2) dx = cos(p1 - p2) (k1 = k2 > 0), 2 cos p1 cos p2 (both 0), else 0
                exact *= (LD(2) * np.cos(p1) * np.cos(p2) if k1 == 0 and k2 == 0 else (np.cos(p1 - p2) if k1 == k2 else LD(0)))
                w.append(np.full(n, LD(2) / LD(n)))
            else:
                a, b = min(ku, n - 1), max(min(ku, n - 1 - min(ku, n - 1)), 0)
                fu.append(cheb_T(n, a)); fv.append(cheb_T(n, b))
                exact *= (LD(1) / (LD(1) - LD(a + b) ** 2) + LD(1) / (LD(1) - LD(a - b) ** 2)) if (a + b) % 2 == 0 else LD(0)
                w.append(sp.cc_weights(n).astype(LD))
        outer = lambda fs: functools.reduce(np.multiply.outer, fs)
        uL, vL, wL = outer(fu), outer(fv), outer(w)
        # (long double sums, and the Clenshaw-Curtis weights of the wall directions as the doubles they are)
        assert abs((wL * uL * vL).sum() - exact) <= (N * 2.0 ** -60 + d * U) * (np.abs(wL * uL * vL)).sum()
        u, v = uL.astype(np.float64), vL.astype(np.float64)
        got = host(m.integrate(dev(u), dev(v)))[0]
        ref = (wL * u.astype(LD) * v.astype(LD)).sum()
        bound = (N + 8 + d) * U * float((wL * np.abs(u) * np.abs(v)).sum())         # (+ d: the device's weights are rounded once)
        assert abs(got - ref) <= bound, (ku, got, float(ref), bound)
    m.destroy()


def test_modal_filter_by_wavenumber():
    dims, mask = (16, 9), (1, 0)
    m = sp.ChebModal(dims, 1, periodic=mask)
    sig = sp.fourier_filter(16, lambda k: 1.0 if k <= 3 else (0.25 if k <= 5 else 0.0))
    m.set_filter(0, sig)
    x = np.random.default_rng(SEED + 4).standard_normal((1,) + dims)
    y = host(m.filter(dev(x), new(m.size()))).reshape(x.shape)
    T, B = sp.fourier_modal_matrix(16, "forward").astype(LD), sp.fourier_modal_matrix(16, "backward").astype(LD)
    F = np.dot(B * sig.astype(LD)[None, :], T)
    absF = np.dot(np.abs(B) * sig[None, :], np.abs(T)).astype(np.float64)
    t = np.moveaxis(np.tensordot(F, x.astype(LD), axes=([1], [1])), 0, 1)
    A = np.moveaxis(np.tensordot(absF, np.abs(x), axes=([1], [1])), 0, 1)
    # the library forms F from the long-double B and T, the truth from their doubles: two more roundings per term
    assert lw.worst(y, t, (16 + 8 + 2) * A)[0] <= 1.0
    # the filtered field has no coefficient above k = 5: forward of it (the device's y) against the long-double chain, which is
    # itself 0 there up to the roundings of y (26 per element, above) and of T B = I (16 + 8 per entry of the chain)
    a = host(m.forward(dev(y), new(m.size()))).reshape(x.shape)
    Tm = modal_mats(dims, mask, "forward")
    t2, A2, cap2 = chain_ld(list(enumerate(Tm)), y)
    assert lw.worst(a, t2, cap2 * A2)[0] <= 1.0
    dead = np.array([k > 5 for k, _ in sp.fourier_modes(16)])
    _, Ad, _ = chain_ld(list(enumerate(Tm)), A)
    assert np.all(np.abs(t2[0][dead]).astype(np.float64) <= (cap2 + 26 + 2 * 24) * U * Ad[0][dead])
    m.destroy()


# =================================================================================================================================
# HelmholtzSolver
# =================================================================================================================================
WALLS = ["dirichlet", "neumann", (1.0, 1.0), ("dirichlet", "neumann")]
COMBOS = [(0.0, 1), (1.5, 3), (1e3, 1), (0.0, 3), (1.5, 1), (1e3, 3)]


class Case:
    def __init__(self, dims, mask, q):
        self.dims, self.mask, self.d = tuple(dims), tuple(mask), len(dims)
        self.sigma, self.nf = COMBOS[q % len(COMBOS)]
        self.scale = SCALE[self.d] if q % 2 else None
        self.wall = [WALLS[(q + k) % len(WALLS)] for k in range(self.d)]
        self.bc = pr.bc_entries(self.wall, mask)
        self.h = sp.HelmholtzSolver(dims, self.sigma, self.nf, bc=self.bc, scale=self.scale)
        self.inner = pr.unknown_shape(dims, mask)
        self.G = int(np.prod(self.inner))
        self.n = self.nf * self.G
        self.shape = (self.nf,) + self.inner
        self.L = pr.lines(sp, dims, mask, self.wall, self.scale)
        self.parity = [True if p else fr.parity_ok(b) for p, b in zip(mask, self.wall)]
        self.eta = None

    def plan(self):
        d, h = self.d, self.h
        steps = []
        z = h.step_route(d - 1, "zsolve") is not None
        for k in range(d):
            if k == d - 1 and d >= 2:
                if z:
                    steps.append(("zsolve", k))
                    continue
                if h.step_route(k, "forward_scaled") is not None:
                    steps.append(("forward_scaled", k))
                    continue
            steps.append(("forward", k))
            assert h.step_route(k, "forward") is not None
        if steps[-1][0] == "forward":
            steps.append(("scale", d - 1))
        for k in range(d - 2 if z else d - 1, -1, -1):
            steps.append(("backward", k))
        return steps

    def run_step(self, mode, k, x):
        return host(self.h.step(k, mode, dev(x), new(self.n))).reshape(self.shape)

    def by_hand(self, x):
        cur = dev(x)
        out = []
        for mode, k in self.plan():
            nxt = self.h.step(k, mode, cur, new(self.n))
            out.append((mode, k, host(cur).reshape(self.shape).copy(), host(nxt).reshape(self.shape).copy()))
            cur = nxt
        return out

    def solve(self, x):
        return host(self.h.solve(dev(x), new(self.n))).reshape(self.shape)

    def tag(self):
        return "%s %s sigma=%g nf=%d %s" % (ids(self.dims), self.mask, self.sigma, self.nf, self.wall)


def check_step(c, mode, k, x, y):
    t, B = fr.step_truth_bound(mode, k, x, c.L, c.sigma, None)
    cap = fr.step_cap(mode, c.inner[k], c.d)
    B = np.where(B > 0, B + 2.0 ** -1021, 0.0)
    r, _ = lw.check(y, t, B, cap, what="%s %s[%d] %s" % (c.tag(), mode, k, sorted(c.h.step_route(k, mode) or ())))
    return r / cap


def check_composite(c, x, z):
    t = fr.truth(x, c.L, c.sigma, None)
    e_dev = fr.errors(z, t)
    e_ref = [fr.errors(fr.chain(x, c.L, c.sigma, None, how, parity=c.parity)[0], t) for how in ("plain", "evenodd")]
    worst = 0.0
    for f in range(c.nf):
        for q in range(2):
            ref = max(e[f][q] for e in e_ref)
            ratio = e_dev[f][q] / ref if ref > 0 else (0.0 if e_dev[f][q] == 0 else np.inf)
            worst = max(worst, ratio)
            assert ratio <= MARGIN, "%s field %d: error %.3g = %.1f x the restatements' %.3g" % (c.tag(), f, e_dev[f][q], ratio, ref)
    return worst


HGRID = [(dims, m, q) for q, (dims, m) in enumerate(GRID)]
# d = 4: the kernels' forms for any d (index arithmetic at run time), three stacked fields, a box, a Dirichlet and a Robin wall
HGRID.append(((4, 5, 4, 6), (1, 0, 1, 0), 3))


@pytest.mark.parametrize("dims,mask,q", HGRID, ids=ids)
def test_helmholtz_steps_composition_and_solve(dims, mask, q):
    c = Case(dims, mask, q)
    h = c.h
    assert h.size == c.n and h.periodic == tuple(bool(p) for p in mask)
    walls_neumann = all(p or w == "neumann" for p, w in zip(mask, c.wall))
    assert h.singular == (c.sigma == 0.0 and walls_neumann)
    if dims == (6, 5, 96) and mask[2]:
        assert h.step_route(2, "zsolve") is not None, "the one-launch z solve must take a periodic last direction of 96 points"
    x = np.random.default_rng(SEED + 5 + q).standard_normal(c.shape)
    z = c.solve(x)
    steps = c.by_hand(x)
    assert np.array_equal(steps[-1][3], z), "the steps run by hand are not the solve"
    worst = max(check_step(c, mode, k, xi, yi) for mode, k, xi, yi in steps)
    w = check_composite(c, x, z)
    print("%s: steps %s, worst step %.3f of its cap, solve %.2f x the restatements" % (c.tag(), [s[:2] for s in steps], worst, w))
    RATIOS.append("solve   %-60s worst step %.3f of cap, device / restatement %.2f" % (c.tag(), worst, w))
    # containment per line: a NaN in one line of a step leaves every other line's bits alone
    mode, k, xi, yi = steps[0]
    K = c.inner[k]
    xm = np.moveaxis(xi.copy(), k + 1, -1).reshape(-1, K)
    for line in sorted({0, xm.shape[0] - 1, xm.shape[0] // 3}):
        xb = xm.copy()
        xb[line, K // 2] = np.nan
        xb = np.moveaxis(xb.reshape([c.shape[j] for j in range(c.d + 1) if j != k + 1] + [K]), -1, k + 1)
        yb = np.moveaxis(c.run_step(mode, k, np.ascontiguousarray(xb)), k + 1, -1).reshape(-1, K)
        keep = np.arange(xm.shape[0]) != line
        assert np.array_equal(yb[keep], np.moveaxis(yi, k + 1, -1).reshape(-1, K)[keep]), (mode, k, line)
    # ... and per stacked field of the whole solve
    if c.nf > 1:
        xb = x.copy()
        xb[1].flat[c.G // 2] = np.nan
        zb = c.solve(xb)
        assert np.array_equal(zb[0], z[0]) and np.array_equal(zb[2], z[2]) and np.isnan(zb[1]).any()
    h.destroy()


# =================================================================================================================================
# solve_full
# =================================================================================================================================
def scatter_g(dims, mask, g, nf):
    Gf = np.zeros((nf,) + tuple(dims))
    bm = pr.boundary_mask(dims, mask)
    for f in range(nf):
        Gf[f][bm] = g.reshape(nf, -1)[f]
    return Gf


def lifted(c, f, Gf):
    """t = f + sum over the wall directions (ascending) of L0 g0 + L1 g1, the faces' nodes taken at unknown indices of the other
    directions: the device's association.  Exact in double when g holds signed powers of two (each product is then exact)."""
    t = f.copy()
    unk = pr.unknown_slices(c.mask)
    for k, n in enumerate(c.dims):
        if c.mask[k]:
            continue
        Lk = sp.helmholtz_line_box(n, c.wall[k], 1.0 if c.scale is None else c.scale[k])[4]
        face = []
        for e in (0, n - 1):
            sl = [slice(None)] + list(unk)
            sl[k + 1] = e
            face.append(Gf[tuple(sl)])
        t = t + (np.moveaxis(np.multiply.outer(Lk[:, 0], face[0]), 0, k + 1) + np.moveaxis(np.multiply.outer(Lk[:, 1], face[1]), 0, k + 1))
    return t


FULL = [(dims, m, q) for dims, m, q in HGRID if not all(m)]
# ... and the handles without a periodic direction, which run the same lift and extension kernels
FULL += [(dims, (0,) * len(dims), len(GRID) + q) for q, dims in enumerate(SHAPES_12 + SHAPES_3 + [(4, 5, 4, 6)])]


@pytest.mark.parametrize("dims,mask,q", FULL, ids=ids)
def test_solve_full(dims, mask, q):
    c = Case(dims, mask, q)
    h, nf, d = c.h, c.nf, c.d
    N = int(np.prod(dims))
    bm = pr.boundary_mask(dims, mask)
    assert h.full_size == nf * N and h.boundary_size == nf * int(bm.sum()) == nf * (N - c.G)      # no face entries on a periodic direction
    rng = np.random.default_rng(SEED + 6 + q)
    f = rng.standard_normal(c.shape)
    unk = (slice(None),) + pr.unknown_slices(mask)

    # 1. signed powers of two as boundary data: the lift is exact in double, so every unknown node is solve(lifted f) bit for bit
    g2 = rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], size=h.boundary_size)
    u = host(h.solve_full(dev(f), dev(g2), new(h.full_size))).reshape((nf,) + tuple(dims))
    z = c.solve(lifted(c, f, scatter_g(dims, mask, g2, nf)))
    assert np.array_equal(u[unk], z), "unknown nodes differ from solve(lifted f)"
    u0 = host(h.solve_full(dev(f), None, new(h.full_size))).reshape(u.shape)
    assert np.array_equal(u0[unk], c.solve(f))

    # 2. noise as boundary data: every boundary node carries the condition of the highest wall direction it is an end node of
    g = rng.standard_normal(h.boundary_size)
    u = host(h.solve_full(dev(f), dev(g), new(h.full_size))).reshape((nf,) + tuple(dims))
    assert np.isfinite(u).all()
    Gf = scatter_g(dims, mask, g, nf)
    rows = pr.wall_rows(sp, dims, mask, c.wall, c.scale)
    worst = 0.0
    for k, n in enumerate(dims):
        if mask[k]:
            continue
        # the lines direction k's pass owns: any index before k, unknown indices after it
        sl = (slice(None),) + tuple(slice(None) if (m < k or mask[m]) else slice(1, -1) for m in range(d) if m != k)
        V = np.moveaxis(u, k + 1, -1)[sl]
        Gd = np.moveaxis(Gf, k + 1, -1)[sl][..., [0, n - 1]]
        _, _, _, Q, _, Bi = sp.helmholtz_line_box(n, c.wall[k], 1.0 if c.scale is None else c.scale[k])
        r0, r1 = rows[k]
        R = np.stack([r0, r1])                                             # 2 x n, long double
        res = np.tensordot(V.astype(LD), R, axes=([-1], [1])) - Gd.astype(LD)
        # u_B = Q u_I + Binv g with at most (M + 8) roundings; the rows see it through |B_BB|
        dB = (n - 2 + 8) * (np.tensordot(np.abs(V[..., 1:-1]), np.abs(Q), axes=([-1], [1])) + np.tensordot(np.abs(Gd), np.abs(Bi), axes=([-1], [1])))
        Bbb = np.abs(R[:, [0, n - 1]]).astype(np.float64)
        W = np.tensordot(dB, Bbb, axes=([-1], [1]))
        worst = max(worst, lw.worst(np.zeros(res.shape), -res, W)[0])
    print("%s: boundary rows %.3f of the bar" % (c.tag(), worst))
    assert worst <= 1.0, worst

    # 3. u may alias neither f nor g
    buf = new(h.full_size)
    with pytest.raises(sp.ChebhipError):
        h.solve_full(buf[:h.size], dev(g), buf)
    with pytest.raises(sp.ChebhipError):
        h.solve_full(dev(f), buf[:h.boundary_size], buf)
    h.destroy()


def test_all_periodic_full_grid_is_the_solve():
    for dims in ((8, 9), (8, 6, 4)):
        h = sp.HelmholtzSolver(dims, 1.5, 3, bc=["periodic"] * len(dims))
        assert h.boundary_size == 0 and h.full_size == h.size
        f = dev(np.random.default_rng(SEED + 7).standard_normal(h.size))
        a, b = host(h.solve(f, new(h.size))), host(h.solve_full(f, None, new(h.size)))
        assert np.array_equal(a, b)
        with pytest.raises(sp.ChebhipError) as e:                      # g given with nothing to lift
            h.solve_full(f, new(1), new(h.size))
        assert e.value.code == 4
        u = new(h.size)
        rc = sp.lib().cheb_helmholtz_solve_bc(h._h, f.data_ptr(), f.data_ptr(), u.data_ptr(), None)
        assert rc == 4 and b"no boundary data" in sp.lib().chebhip_last_error()
        h.destroy()


# =================================================================================================================================
# the two modules agree: the solve's residual under ChebGrad.laplacian
# =================================================================================================================================
def residual(dims, mask, sigma, scale, seed):
    d = len(dims)
    bc = pr.bc_entries(None, mask)
    h = sp.HelmholtzSolver(dims, sigma, 1, bc=bc, scale=scale)
    g = sp.ChebGrad(dims, scale, periodic=mask)
    unk = pr.unknown_slices(mask)
    f = np.random.default_rng(seed).standard_normal(pr.unknown_shape(dims, mask))
    u = h.solve_full(dev(f), None, new(h.full_size))
    lap = host(g.laplacian(u)).reshape(dims)
    uh = host(u).reshape(dims)
    r = f - (sigma * uh - lap)[unk]
    Bu = sigma * np.abs(uh)
    for k, n in enumerate(dims):
        s2 = 1.0 if scale is None else scale[k] ** 2
        Bu = Bu + s2 * np.moveaxis(np.tensordot(np.abs(pr.dmat(sp, n, mask[k], 2)).astype(np.float64), np.abs(uh), axes=([1], [k])), 0, k)
    h.destroy(); g.destroy()
    return float(np.linalg.norm(r) / (np.linalg.norm(f) + np.linalg.norm(Bu[unk])))


@pytest.mark.parametrize("dims,mask", [(dims, m) for dims, m in GRID if not all(m)], ids=ids)
def test_solve_and_laplacian_agree(dims, mask):
    d = len(dims)
    for sigma, scale in ((0.0, None), (1.5, SCALE[d])):
        rp = residual(dims, mask, sigma, scale, SEED + 8)
        rw = residual(dims, (0,) * d, sigma, scale, SEED + 8)
        print("%s %s sigma=%g: periodic %.3g, all-wall %.3g" % (ids(dims), mask, sigma, rp, rw))
        RATIOS.append("residual %-14s %-10s sigma=%-4g scale=%-16s periodic %.3e  all-wall %.3e  ratio %.2f" % (ids(dims), mask, sigma, scale, rp, rw, rp / rw))
        assert rp <= MARGIN * rw, (rp, rw)


# =================================================================================================================================
# singular cases, the known answer
# =================================================================================================================================
def drop_modes(L, a):
    """a (nf, *unknowns) without its components along the dropped modes (every product of zero-eigenvalue modes), long double."""
    t = np.asarray(a).astype(LD)
    for k, (S, Si, lam) in enumerate(L):
        t = np.moveaxis(np.tensordot(Si.astype(LD), t, axes=([1], [k + 1])), 0, k + 1)
    zero = fr.weight_sum(L, 0.0, LD) == 0
    coef = np.where(zero, t, LD(0))
    t = np.where(zero, LD(0), t)
    for k, (S, Si, lam) in enumerate(L):
        t = np.moveaxis(np.tensordot(S.astype(LD), t, axes=([1], [k + 1])), 0, k + 1)
    return t, coef


@pytest.mark.parametrize("dims", [(8, 9), (8, 6, 4)], ids=ids)
def test_singular_all_periodic(dims):
    d = len(dims)
    mask = (1,) * d
    h = sp.HelmholtzSolver(dims, 0.0, 1, bc=["periodic"] * d)
    assert h.singular
    L = pr.lines(sp, dims, mask)
    nzero = int((fr.weight_sum(L, 0.0, LD) == 0).sum())
    assert nzero == int(np.prod([1 + (n % 2 == 0) for n in dims]))            # the constants and the Nyquist vectors, all products
    rng = np.random.default_rng(SEED + 9)
    # compatible data: f = A u0 with u0 free of the dropped modes
    u0, _ = drop_modes(L, rng.standard_normal((1,) + dims))
    f = np.zeros(u0.shape, dtype=LD)
    for k, n in enumerate(dims):
        f = f - np.moveaxis(np.tensordot(sp.fourier_diff_matrix(n, 2).astype(LD), u0, axes=([1], [k + 1])), 0, k + 1)
    f = f.astype(np.float64)
    u = host(h.solve(dev(f), new(h.size))).reshape(f.shape)
    # no component along any dropped mode: those coefficients of u are roundings of the backward transforms
    # (u = S c: the backward transforms err by (n_k + 8) 2^-53 |S| |c| per step, which the coefficients see through |S^-1|)
    _, coef = drop_modes(L, u)
    A = u.astype(LD)
    for k, (S, Si, lam) in enumerate(L):
        A = np.moveaxis(np.tensordot(Si.astype(LD), A, axes=([1], [k + 1])), 0, k + 1)
    A = np.abs(A).astype(np.float64)
    for M in (0, 1):
        for k, mats in enumerate(L):
            A = np.moveaxis(np.tensordot(np.abs(mats[M]), A, axes=([1], [k + 1])), 0, k + 1)
    cap = 2 * sum(n + 8 for n in dims)
    assert np.all(np.abs(coef).astype(np.float64) <= cap * U * A), float(np.abs(coef).max())
    # reproduced up to those modes, as well as the double restatements reproduce it
    err = lambda v: float(np.abs(drop_modes(L, v)[0] - u0).max())
    e_dev = err(u)
    e_ref = max(err(fr.chain(f, L, 0.0, None, how)[0]) for how in ("plain", "evenodd"))
    print("%s: device %.3g, restatements %.3g" % (ids(dims), e_dev, e_ref))
    assert e_dev <= MARGIN * e_ref
    # noise with components along the dropped modes: they are ignored
    x = rng.standard_normal((1,) + dims)
    z = host(h.solve(dev(x), new(h.size))).reshape(x.shape)
    assert check_composite_plain(L, x, z) <= MARGIN
    h.destroy()


def check_composite_plain(L, x, z):
    t = fr.truth(x, L, 0.0, None)
    e_dev = fr.errors(z, t)[0]
    e_ref = [fr.errors(fr.chain(x, L, 0.0, None, how)[0], t)[0] for how in ("plain", "evenodd")]
    return max(e_dev[q] / max(e[q] for e in e_ref) for q in range(2))


def test_channel_known_answer():
    """Periodic x and z, Dirichlet y at (16, 17, 12): u = sin(pi (x+1)) (1 - y^2) cos(2 pi (z+1)), f = -Laplace u from the formula,
    through solve.channel_poisson; the bar is 16 x the error the all-wall handle reaches on (1 - x^2)(1 - y^2)(1 - z^2)."""
    dims, mask = (16, 17, 12), (True, False, True)
    for scale in (None, (0.5, 1.0, 2.0)):
        s = (1.0, 1.0, 1.0) if scale is None else scale
        x, z = pr.nodes(16), pr.nodes(12)
        y = lw._sin_half(16 - 2 * np.arange(17), 16)                        # cos(pi j / 16)
        sx, cz = pr.sin_pi(2 * np.arange(16), 16), pr.cos_pi(4 * np.arange(12), 12)    # sin(pi (x_j + 1)), cos(2 pi (z_j + 1))
        wy = LD(1) - y * y
        uex = np.einsum("i,j,k->ijk", sx, wy, cz)
        f = (LD(s[0]) ** 2 * lw.PI_L ** 2 + LD(s[2]) ** 2 * 4 * lw.PI_L ** 2) * uex + LD(s[1]) ** 2 * 2 * np.einsum("i,j,k->ijk", sx, np.ones(17, dtype=LD), cz)
        u = host(solve.channel_poisson(sp, dims, dev(f.astype(np.float64)), mask, scale)).reshape(dims)
        e_per = float(np.abs(u - uex).max() / np.abs(uex).max())
        # the all-wall handle on its own polynomial answer
        xs = [lw._sin_half(n - 1 - 2 * np.arange(n), n - 1) for n in dims]
        p = [LD(1) - v * v for v in xs]
        wex = np.einsum("i,j,k->ijk", *p)
        one = [np.ones(n, dtype=LD) for n in dims]
        fw = sum(LD(s[k]) ** 2 * 2 * np.einsum("i,j,k->ijk", *[one[m] if m == k else p[m] for m in range(3)]) for k in range(3))
        w = host(solve.helmholtz_bvp(sp, dims, dev(fw.astype(np.float64)), None, ["dirichlet"] * 3, 0.0, scale=scale)).reshape(dims)
        e_wall = float(np.abs(w - wex).max() / np.abs(wex).max())
        print("scale %s: channel %.3g, all-wall %.3g" % (scale, e_per, e_wall))
        RATIOS.append("known answer 16x17x12 scale=%-16s channel %.3e  all-wall %.3e  ratio %.2f" % (scale, e_per, e_wall, e_per / e_wall))
        assert e_per <= MARGIN * e_wall, (e_per, e_wall)


def test_argument_errors_on_the_device():
    with pytest.raises(sp.ChebhipError) as e:
        sp.HelmholtzSolver((257, 8), bc=["periodic", "dirichlet"])
    assert e.value.code == 4 and "256" in str(e.value)
    with pytest.raises(sp.ChebhipError) as e:
        sp.ChebGrad((8, 257), periodic=(False, True))
    assert e.value.code == 4 and "256" in str(e.value)
    with pytest.raises(sp.ChebhipError) as e:
        sp.ChebModal((257,), periodic=(True,))
    assert e.value.code == 4 and "256" in str(e.value)
    with pytest.raises(sp.ChebhipError):
        sp.HelmholtzSolver((8, 8), bc=["dirichlet", ("neumann", "periodic")])
    h = sp.HelmholtzSolver((2, 5), 1.0, bc=["periodic", "neumann"])            # two points are enough for a periodic direction
    assert h.size == 6 and h.boundary_size == 4
    h.destroy()
