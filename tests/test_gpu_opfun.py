"""ChebOpFun on the device (cheb_opfun_*) against the model and the bars of opfun_ref.py: the device functions over
thirty-nine decades of s, every kind on every shape at which a transform route changes, `inv` against the solver bit for bit,
`pow` with p = 1 against the operator, term tables that mix fields, analytic heat solutions, and the plumbing."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import linewise as lw
import opfun_ref as R

pytestmark = pytest.mark.gpu
sp = R.sp
solve = import_module(sp.__name__ + ".solve")

NEU, DIR = "neumann", "dirichlet"
MIXED = (NEU, (DIR, NEU), (1.0, 0.5))
# (dims, bc, scale, sigma): the smallest shapes at which a route changes (one launch / two launches per transform, the 66-point
# kernel switch, M = 128 where the solver's one-launch z solve exists, the longest line, the index chain of d > 3), the three
# kinds of faces, a box, and the singular handle
SHAPES = [((7,), None, None, 0.0), ((12, 9), None, None, 0.5), ((10, 9, 8), None, None, 0.0), ((6, 5, 34), None, None, 2.0),
          ((70, 6, 5), None, None, 0.0), ((130, 6), None, None, 0.0), ((6, 130), None, None, 1.0), ((258, 6), None, None, 0.0),
          ((5, 4, 6, 5), None, None, 0.25), ((20, 12, 9), MIXED, None, 0.0), ((20, 12, 9), MIXED, (2.0, 0.5, 1.25), 0.5),
          ((10, 9, 8), (NEU, NEU, NEU), None, 0.0)]
KIND_ARGS = {"one": (0.0, 0.0), "inv": (0.0, 0.0), "res": (0.02, 1.5), "exp": (0.01, 0.0), "phi1": (0.01, 0.0), "phi2": (0.01, 0.0),
             "phi3": (0.01, 0.0), "pow": (0.0, 0.5)}


def sid(c):
    dims, bc, scale, sigma = c
    return "x".join(map(str, dims)) + ("" if bc is None else "-bc") + ("" if scale is None else "-box") + ("-s%g" % sigma if sigma else "")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def gsize(dims):
    return int(np.prod([n - 2 for n in dims]))


# ---- 1: the device functions ----------------------------------------------------------------------------------------------
def test_device_functions():
    rng = np.random.default_rng(11)
    base = np.concatenate([10.0 ** rng.uniform(-30.0, 9.0, 100000), [0.0]])
    worst = {k: 0.0 for k in R.KINDS}
    bad = []
    for kind in R.KINDS:
        for tau in (0.0, 1e-9, 1e-3, 1.0, 10.0):
            for par in ((1.0, 0.5, -0.5, 2.0) if kind == "pow" else (1.0,)):
                s = base
                if kind in ("phi2", "phi3") and tau > 0:      # the series / recurrence threshold |tau s| = 2 and its neighbours
                    t = R.PHI_SERIES / tau
                    s = np.concatenate([base, [np.nextafter(t, 0.0), t, np.nextafter(t, np.inf)]])
                w = host(sp.opfun_eval(kind, tau, par, dev(s)))
                twin = sp.opfun_weight(kind, tau, par, s)
                err = np.abs(w - twin)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(err == 0, 0.0, err / R.weight_bar(kind, tau, s, twin))
                i = int(np.argmax(ratio))
                worst[kind] = max(worst[kind], float(ratio[i]))
                print("%-5s tau %-6g par %-4g worst %.3f of the bar at s = %.17g" % (kind, tau, par, ratio[i], s[i]))
                if not ratio[i] <= 1.0:
                    bad.append((kind, tau, par, float(s[i]), float(ratio[i])))
    try:
        path = os.path.join(ge.ROOT, "profiles", "opfun")
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "ratios.txt"), "w") as f:
            f.write("worst |w - twin| / weight bar per kind: cheb_opfun_eval on 10^5 log-uniform s in [1e-30, 1e9], s = 0 and the\n"
                    "phi thresholds +- 1 ulp, tau in {0, 1e-9, 1e-3, 1, 10} (tests/test_gpu_opfun.py::test_device_functions)\n")
            for k in R.KINDS:
                f.write("%-5s K = %-2d  %.3f\n" % (k, R.K[k], worst[k]))
    except OSError:
        pass
    assert not bad, bad
    assert max(R.K.values()) <= 16


# ---- 2: every kind on every shape -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=sid)
def test_every_kind(case):
    dims, bc, scale, sigma = case
    ln = R.lines(dims, bc, scale)
    x = np.random.default_rng(21).standard_normal((1, gsize(dims)))
    h = sp.ChebOpFun(dims, 1, 1, sigma, bc=bc, scale=scale)
    assert h.size == h.out_size == gsize(dims) and h.full_size == int(np.prod(dims))
    assert h.singular == (bc is not None and sigma == 0.0 and all(b == NEU for b in bc))
    xd = dev(x)
    for kind in R.KINDS:
        tau, par = KIND_ARGS[kind]
        h.set_terms(kind, tau=tau, par=par)
        y = host(h.apply(xd))
        ref, bar = R.model(dims, [(0, 0, kind, 1.0, tau, par)], x, 1, sigma=sigma, ln=ln)
        ratio, nerr = R.check(y, ref, bar, "%s %s" % (sid(case), kind))
        print("%s %-5s worst %.2e of the field bar, normwise %.1e" % (sid(case), kind, ratio, nerr))
    h.destroy()


def test_many_lines_take_the_index_chain():
    """258 x 258 x 3 has 65536 lines of the last dimension, one more than a launch's second grid dimension holds: the smallest d <= 3
    shape that takes the index-chain kernel of d > 3."""
    dims, sigma = (258, 258, 3), 0.5
    ln = R.lines(dims)
    x = np.random.default_rng(22).standard_normal((1, gsize(dims)))
    h = sp.ChebOpFun(dims, sigma=sigma)
    xd = dev(x)
    for kind, tau in (("exp", 1e-6), ("inv", 0.0)):
        h.set_terms(kind, tau=tau)
        y = host(h.apply(xd))
        ref, bar = R.model(dims, [(0, 0, kind, 1.0, tau, 0.0)], x, 1, sigma=sigma, ln=ln)
        R.check(y, ref, bar, "258x258x3 %s" % kind)
    h.destroy()


# ---- 3: inv against the solver, bit for bit ---------------------------------------------------------------------------------
def same_route(dims, bc):
    """The solver multiplies by its W array only where the LAST forward transform is one launch of the 16-byte kernels, which on
    contiguous lines needs an even number of interior points and a parity line (equal ends); elsewhere its separate pass divides,
    which differs from a product with the reciprocal in the last bit."""
    ends = (1.0, 0.0, 1.0, 0.0) if bc is None else sp.bc_array(bc, len(dims))[-4:]
    return (dims[-1] - 2) % 2 == 0 and tuple(ends[:2]) == tuple(ends[2:])


INV_CASES = [c for c in SHAPES if 2 <= len(c[0]) <= 3 and same_route(c[0], c[1])]
assert len(INV_CASES) >= 6          # (the rule leaves the bitwise test most of the d = 2, 3 shapes)


@pytest.mark.parametrize("case", INV_CASES, ids=sid)
def test_inv_is_the_solver(case):
    dims, bc, scale, sigma = case
    nf = 2
    x = dev(np.random.default_rng(31).standard_normal(nf * gsize(dims)))
    old = sp.get_option("fdm_z_separate")
    sp.set_option("fdm_z_separate", 1)
    try:
        hs = sp.HelmholtzSolver(dims, sigma, nf, bc=bc, scale=scale)
        h = sp.ChebOpFun(dims, nf, nf, sigma, bc=bc, scale=scale)
        h.set_terms("inv")
        u = torch.empty_like(x)
        hs.solve(x, u)
        y = h.apply(x)
        torch.cuda.synchronize()
        assert torch.equal(y, u), "%d of %d values differ, largest relative difference %.3g" % (
            int((y != u).sum()), y.numel(), float(((y - u).abs() / u.abs()).max()))
        hs.destroy(); h.destroy()
    finally:
        sp.set_option("fdm_z_separate", old)


# ---- 4: pow with p = 1 against the operator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in SHAPES if c[1] is None], ids=sid)
def test_pow_one_is_the_operator(case):
    dims, bc, scale, sigma = case
    x = np.random.default_rng(41).standard_normal((1, gsize(dims)))
    h = sp.ChebOpFun(dims, sigma=sigma)
    h.set_terms("pow", par=1.0)
    op = sp.EllipticOp(dims)
    xd = dev(x[0])
    y = h.apply(xd)
    v = torch.empty_like(xd)
    op.mult(xd, v)
    v = host(v) + sigma * x[0]
    y = host(y)
    _, bar = R.model(dims, [(0, 0, "pow", 1.0, 0.0, 1.0)], x, 1, sigma=sigma)
    t, B, factor = lw.elliptic_truth_bound(dims, x[0])
    bar_op = R.U * (factor * np.asarray(B, dtype=np.float64).ravel() + 2 * (np.abs(v) + np.abs(sigma * x[0])))
    err = np.abs(y - v)
    ratio = float(np.max(err / (bar[0] + bar_op)))
    assert ratio <= 1.0, ratio
    assert np.linalg.norm(err) <= R.NORM_BAR * np.linalg.norm(v)
    h.destroy(); op.destroy()


# ---- 5: tables that mix fields ----------------------------------------------------------------------------------------------
HSTEP = 0.01
TABLES = {
    "etd1": ((10, 9, 8), 2, 1, [(0, 0, "exp", 1.0, HSTEP, 0.0), (0, 1, "phi1", HSTEP, HSTEP, 0.0)]),
    "3to2": ((10, 9, 8), 3, 2, [(0, 0, "exp", 1.0, HSTEP, 0.0), (0, 1, "phi1", HSTEP, HSTEP, 0.0), (1, 2, "inv", -2.0, 0.0, 0.0),
                                (1, 0, "exp", 0.5, HSTEP, 0.0), (0, 2, "res", 3.0, 0.1, 1.0), (1, 1, "phi2", HSTEP * HSTEP, HSTEP, 0.0),
                                (1, 1, "phi1", -1.0, HSTEP, 0.0), (0, 0, "pow", 0.125, 0.0, 0.5)]),
    "res16": ((12, 9), 16, 16, [(f, f, "res", 1.0 + f, 0.001 * (f + 1), 1.0 + 0.25 * f) for f in range(16)]),
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_mixing(name):
    dims, nin, nout, terms = TABLES[name]
    G = gsize(dims)
    x = np.random.default_rng(51).standard_normal((nin, G))
    ln = R.lines(dims)
    h = sp.ChebOpFun(dims, nin, nout, 0.0)
    h.set_terms(terms)
    xd = dev(x)
    y1 = h.apply(xd)
    y2 = h.apply(xd)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)
    y = host(y1).reshape(nout, G)
    ref, bar = R.model(dims, terms, x, nout, ln=ln)
    R.check(y, ref, bar, name)
    # the same from one-term calls and torch additions, in table order
    one = sp.ChebOpFun(dims, 1, 1, 0.0)
    comp = torch.zeros(nout, G, dtype=torch.float64, device="cuda")
    cbar = np.zeros((nout, G))
    for (o, i, kind, c, tau, par) in terms:
        one.set_terms([(0, 0, kind, c, tau, par)])
        part = one.apply(xd[i].contiguous())
        comp[o] += part
        cbar[o] += R.model(dims, [(0, 0, kind, c, tau, par)], x[i:i + 1], 1, ln=ln)[1][0] + R.U * (np.abs(host(part)) + np.abs(host(comp[o])))
    assert np.all(np.abs(y - host(comp)) <= bar + cbar)
    h.destroy(); one.destroy()


# ---- 6: analytic heat solutions ---------------------------------------------------------------------------------------------
HEAT_DIMS, HEAT_T = (24, 20, 18), 0.1


def nodes(dims):
    return np.meshgrid(*[np.cos(np.pi * np.arange(n) / (n - 1)) for n in dims], indexing="ij")


def heat_cases():
    X = nodes(HEAT_DIMS)
    p = np.pi
    c = lambda k, w: np.cos(w * X[k])
    return {
        "dirichlet": ((DIR, DIR, DIR), 0.0, c(0, p / 2) * c(1, p / 2) * c(2, p / 2), 0.75 * p * p),
        "neumann": ((NEU, NEU, NEU), 1.0, c(0, p) * c(1, p) * c(2, p), 3.0 * p * p),
        "mixed": ((DIR, NEU, DIR), 0.0, c(0, p / 2) * c(1, p) * c(2, p / 2), 1.5 * p * p),
    }


@pytest.mark.parametrize("name", ["dirichlet", "neumann", "mixed"])
def test_heat(name):
    bc, const, mode, rate = heat_cases()[name]
    inner = tuple(slice(1, -1) for _ in HEAT_DIMS)
    u0 = const + mode
    exact = const + np.exp(-rate * HEAT_T) * mode
    tol = 1e-9 * np.max(np.abs(exact))
    h = sp.ChebOpFun(HEAT_DIMS, bc=bc)
    h.set_terms("exp", tau=HEAT_T)
    xi = dev(u0[inner].ravel())
    y = host(h.apply(xi)).reshape(exact[inner].shape)
    assert np.max(np.abs(y - exact[inner])) <= tol, np.max(np.abs(y - exact[inner])) / tol
    yf = host(h.apply_full(xi)).reshape(HEAT_DIMS)
    assert np.max(np.abs(yf - exact)) <= tol, np.max(np.abs(yf - exact)) / tol
    assert np.array_equal(yf[inner], y)
    h.destroy()
    ud = solve.diffuse(sp, HEAT_DIMS, dev(u0), HEAT_T, bc)
    assert np.max(np.abs(host(ud) - exact)) <= tol
    # kappa and the box: u_t = kappa sum_k s_k^2 d_k^2 u on [-1/s_k, 1/s_k] has the same solution at t / (kappa s^2) for s_k = s
    ud = solve.diffuse(sp, HEAT_DIMS, dev(u0), HEAT_T / (0.5 * 4.0), bc, kappa=0.5, scale=(2.0, 2.0, 2.0))
    assert np.max(np.abs(host(ud) - exact)) <= tol


def test_diffuse_with_steady_boundary_data():
    bc, _, mode, rate = heat_cases()["dirichlet"]
    X = nodes(HEAT_DIMS)
    us = 1.0 + 0.5 * X[0] + 0.25 * X[1] * X[2]                # harmonic: the steady state of its own boundary values
    mask = np.ones(HEAT_DIMS, dtype=bool)
    mask[tuple(slice(1, -1) for _ in HEAT_DIMS)] = False
    g = dev(us[mask])
    exact = us + np.exp(-rate * HEAT_T) * mode
    ud = solve.diffuse(sp, HEAT_DIMS, dev(us + mode), HEAT_T, bc, g=g)
    assert np.max(np.abs(host(ud) - exact)) <= 1e-9 * np.max(np.abs(exact))
    # a source: -Laplace u_s = f = 2 for u_s = us + (1 - x_0^2), with that field's own boundary values
    us2 = us + (1.0 - X[0] ** 2)
    f = dev(np.full(HEAT_DIMS, 2.0))
    exact = us2 + np.exp(-rate * HEAT_T) * mode
    ud = solve.diffuse(sp, HEAT_DIMS, dev(us2 + mode), HEAT_T, bc, g=dev(us2[mask]), f=f)
    assert np.max(np.abs(host(ud) - exact)) <= 1e-9 * np.max(np.abs(exact))
    with pytest.raises(ValueError):
        solve.diffuse(sp, HEAT_DIMS, dev(us), HEAT_T, (NEU, NEU, NEU), g=g)
    with pytest.raises(ValueError):
        solve.diffuse(sp, HEAT_DIMS, dev(us), -1.0, bc)


# ---- 7: plumbing --------------------------------------------------------------------------------------------------------------
def test_in_place_overlap_and_empty_outputs():
    dims = (10, 9, 8)
    G = gsize(dims)
    x = dev(np.random.default_rng(71).standard_normal(2 * G))
    h = sp.ChebOpFun(dims, 2, 2, 0.5)
    h.set_terms("exp", tau=0.01)
    y = h.apply(x)
    z = x.clone()
    assert h.apply(z, out=z) is z
    torch.cuda.synchronize()
    assert torch.equal(z, y)
    buf = torch.zeros(4 * G, dtype=torch.float64, device="cuda")
    with pytest.raises(sp.ChebhipError) as e:
        h.apply(buf[:2 * G], out=buf[G:3 * G])
    assert e.value.code == 4
    h.destroy()
    h = sp.ChebOpFun(dims, 2, 1, 0.5)
    h.set_terms([(0, 1, "one", 1.0, 0, 0)])
    with pytest.raises(sp.ChebhipError):
        h.apply(x, out=x[:G])                                  # y inside x with nin != nout
    with pytest.raises(sp.ChebhipError):
        h.apply(x, out=x[G:])
    assert torch.allclose(h.apply(x), x[G:], rtol=0, atol=1e-10)
    h.destroy()
    # an output without a term is zero, a new handle has no term at all
    h = sp.ChebOpFun(dims, 1, 3, 0.0)
    out = torch.full((3 * G,), float("nan"), dtype=torch.float64, device="cuda")
    h.apply(x[:G], out=out)
    torch.cuda.synchronize()
    assert torch.count_nonzero(out) == 0
    h.set_terms([(1, 0, "exp", 1.0, 0.01, 0.0)])
    out.fill_(float("nan"))
    h.apply(x[:G], out=out)
    torch.cuda.synchronize()
    assert torch.count_nonzero(out[:G]) == 0 and torch.count_nonzero(out[2 * G:]) == 0
    assert torch.isfinite(out).all() and float(out[G:2 * G].abs().max()) > 0
    with pytest.raises(ValueError):
        h.apply_full(x[:G])                                    # no bc
    h.destroy()


def test_set_terms_between_queued_applies():
    dims = (34, 18, 10)
    G = gsize(dims)
    x = dev(np.random.default_rng(72).standard_normal(G))
    h = sp.ChebOpFun(dims)
    a, b = [(0, 0, "exp", 1.0, 0.01, 0.0)], [(0, 0, "res", 2.0, 0.5, 1.0)]
    h.set_terms(a)
    ra = h.apply(x).clone()
    torch.cuda.synchronize()
    h.set_terms(b)
    rb = h.apply(x).clone()
    torch.cuda.synchronize()
    assert not torch.equal(ra, rb)
    ya, yb = torch.empty_like(x), torch.empty_like(x)
    h.set_terms(a)
    h.apply(x, out=ya)
    h.set_terms(b)                                             # the first apply is still queued or running
    h.apply(x, out=yb)
    torch.cuda.synchronize()
    assert torch.equal(ya, ra) and torch.equal(yb, rb)
    with pytest.raises(sp.ChebhipError):
        h.set_terms([(0, 0, "exp", 1.0, -1.0, 0.0)])
    assert torch.equal(h.apply(x), rb)                         # a refused table leaves the old one in place
    h.destroy()


def test_wrong_sizes_and_dtypes():
    dims = (12, 9)
    G = gsize(dims)
    h = sp.ChebOpFun(dims, 2, 1, bc=(NEU, DIR))
    x = torch.zeros(2 * G, dtype=torch.float64, device="cuda")
    for bad in (x[:G], x.float(), x.cpu(), x.reshape(2, G).t(), None):
        with pytest.raises(ValueError):
            h.apply(bad)
    for bad in (torch.zeros(2 * G, dtype=torch.float64, device="cuda"), torch.zeros(G, dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            h.apply(x, out=bad)
    with pytest.raises(ValueError):
        h.apply_full(x, out=torch.zeros(G, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        h.set_terms("exp", tau=0.1)                            # the shorthand needs nin == nout
    with pytest.raises(ValueError):
        h.set_terms([(0, 0, "exp", 1.0)])
    with pytest.raises(ValueError):
        sp.ChebOpFun(dims, scale=(1.0, 2.0))
    assert h.apply_full(x).numel() == h.full_size == 12 * 9
    h.destroy()
