"""cheb_grad_* on the device (ChebGrad): every element of grad, tensor, div, curl, strain and laplacian within the derived bar of
grad_ref.py (N(0, 1) data and data scaled per line by 10^+-100, unit and non-unit scales), the invariants kernel against the
long-double formulas on the tensor it was given, ChebPlan.mult, div against DIV, run-to-run bits, exact fields, and the argument
errors that need a handle."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import grad_ref as gr
import linewise as lw

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = 20261018
LD = np.longdouble
U = 2.0 ** -53

# (dims, vectors): lines of at most 64, 65 .. 256 and more than 256 points, odd and even N, every direction strided and contiguous;
# 1 .. 3 vectors, 1 .. 16 scalars (grad takes the nv * d fields as scalars)
CASES = [((2,), 16), ((17,), 16), ((1024,), 2), ((5, 7), 3), ((66, 65), 2), ((257, 4), 1), ((4, 257), 2), ((9, 8, 7), 3),
         ((20, 18, 16), 2), ((63, 64, 65), 1), ((6, 5, 4, 3), 3), ((12,) * 5, 1)]
case_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
KINDS = ["noise", "scaled"]
SCALE = (0.5, 2.0, 3.0, 4.0, 5.0)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).ravel()).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def data(dims, nv, kind):
    """The nv * d input fields of a case, made once and left unchanged; "scaled": field j scaled per line along direction j mod d."""
    d = len(dims)
    gen = lw.noise if kind == "noise" else lw.scaled
    return np.stack([gen(dims, j % d, SEED + 17 * j + sum(dims)) for j in range(nv * d)])


@functools.lru_cache(maxsize=None)
def table(dims, nv, kind):
    """D_k x[j] in long double with its weights: shared by every first-order operator, scale and test of the case."""
    return gr.derivs(dims, data(dims, nv, kind))


def scales(d):
    return [None, SCALE[:d]]


def ops_of(d):
    return ["grad", "tensor", "div", "strain"] + (["curl"] if d in (2, 3) else [])


def units(op, dims, nv):
    return nv * len(dims) if op == "grad" else nv


# ---- 1. every element within its bar --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,nv", CASES, ids=case_ids)
def test_per_element_bar(dims, nv, kind):
    """Prints the worst |out - truth| / bar of every operator of the case (profiles/grad/ratios.txt)."""
    d = len(dims)
    x = data(dims, nv, kind)
    xd = dev(x)
    tab = table(dims, nv, kind)
    for sc in scales(d):
        g = sp.ChebGrad(dims, sc)
        assert g.N == int(np.prod(dims))
        for op in ops_of(d):
            out = host(getattr(g, op)(xd))
            tr, W = gr.first_order(op, dims, sc, tab, units(op, dims, nv))
            assert out.shape == tr.shape
            r = gr.ratio(out, tr, W)
            print("%s nv %d %s scale %s %s: %.3g of the bar" % (case_ids(dims), nv, kind, "1" if sc is None else "s", op, r))
            assert r <= 1.0, (op, sc, r)
        nf = min(nv * d, 16)
        out = host(g.laplacian(xd[:nf * g.N]))
        tr, W = gr.laplacian(dims, sc, x[:nf])
        r = gr.ratio(out, tr, W)
        print("%s nf %d %s scale %s laplacian: %.3g of the bar" % (case_ids(dims), nf, kind, "1" if sc is None else "s", r))
        assert r <= 1.0, ("laplacian", sc, r)
        assert g.work_size(nf) == (nf * g.N if max(dims) > 256 else 0)
        g.destroy()
    assert (bits(host(xd)) == bits(x.ravel())).all()                       # the inputs keep their bits


# ---- 2. the invariants kernel ---------------------------------------------------------------------------------------------------
INV_CASES = [((17,), 3), ((16,), 1), ((5, 7), 2), ((6, 7), 3), ((5, 7, 9), 1), ((9, 8, 7), 3), ((3, 5, 3, 3), 2), ((6, 5, 4, 3), 1)]


def check_invariants(G, dims, nv, which, out, tag):
    d = len(dims)
    out = out.reshape((nv, len(which)) + dims)
    worst = 0.0
    for v in range(nv):
        ref = gr.invariants(G[v])
        for i, name in enumerate(which):
            val, A, T = ref[name]
            r = gr.ratio(out[v, i], val, (T + 4) * A)
            worst = max(worst, r)
            assert r <= 1.0, (tag, name, v, r)
    return worst


@pytest.mark.parametrize("dims,nv", INV_CASES, ids=case_ids)
def test_invariants_bar(dims, nv):
    d = len(dims)
    N = int(np.prod(dims))
    rng = np.random.default_rng(SEED + N)
    G0 = rng.standard_normal((nv, d, d) + dims)
    Gs = G0 * 10.0 ** rng.integers(-50, 51, size=dims)
    g = sp.ChebGrad(dims)
    for tag, G in (("noise", G0), ("scaled", Gs)):
        Gd = dev(G)
        full = host(g.invariants_from(Gd, gr.NAMES))
        worst = check_invariants(G, dims, nv, gr.NAMES, full, tag)
        full = full.reshape((nv, 6) + dims)
        for i, name in enumerate(gr.NAMES):
            one = host(g.invariants_from(Gd, (name,)))
            assert one.shape == (nv,) + dims
            check_invariants(G, dims, nv, (name,), one, tag)
            assert (bits(one) == bits(full[:, i])).all(), name                # one kernel: a field does not depend on the mask
        print("%s nv %d %s invariants: %.3g of the bar" % (case_ids(dims), nv, tag, worst))
        assert (bits(host(Gd)) == bits(G.ravel())).all()
        # a tensor that starts on an odd multiple of 8 bytes takes the 8-byte accesses: same bits
        buf = torch.empty(G.size + 1, dtype=torch.float64, device="cuda")
        buf[1:].copy_(Gd)
        assert (bits(host(g.invariants_from(buf[1:], gr.NAMES))) == bits(full.ravel().reshape(-1, *dims))).all()
    g.destroy()


@pytest.mark.parametrize("dims,nv", [((6, 7), 2), ((5, 7, 9), 2), ((6, 5, 4, 3), 2)], ids=case_ids)
def test_invariants_isolate_nan_and_inf(dims, nv):
    d = len(dims)
    N = int(np.prod(dims))
    rng = np.random.default_rng(SEED + N + 1)
    G = rng.standard_normal((nv, d, d, N))
    g = sp.ChebGrad(dims)
    clean = host(g.invariants_from(dev(G), gr.NAMES)).reshape(nv, 6, N)
    for bad, node, (c, k) in ((np.nan, N // 3, (0, 0)), (np.inf, N - 1, (0, d - 1))):
        Gb = G.copy()
        Gb[1, c, k, node] = bad
        out = host(g.invariants_from(dev(Gb), gr.NAMES)).reshape(nv, 6, N)
        keep = np.ones((nv, 6, N), dtype=bool)
        keep[1, :, node] = False
        assert (bits(out)[keep] == bits(clean)[keep]).all()
        touched = [n for n in gr.NAMES if (n not in ("vort2",) if c == k else n not in ("div",))]
        for i, name in enumerate(gr.NAMES):
            if name in touched:
                assert not np.isfinite(out[1, i, node]), (bad, name)
            else:
                assert bits(out[1, i, node]) == bits(clean[1, i, node]), (bad, name)
    g.destroy()


@pytest.mark.parametrize("dims,nv", [((5, 7), 3), ((20, 18, 16), 2), ((6, 5, 4, 3), 1)], ids=case_ids)
def test_invariants_of_a_field_equal_invariants_from_its_tensor(dims, nv):
    xd = dev(data(dims, nv, "noise"))
    g = sp.ChebGrad(dims, SCALE[:len(dims)])
    a = host(g.invariants(xd, gr.NAMES))
    b = host(g.invariants_from(g.tensor(xd), gr.NAMES))
    assert a.shape == (nv * 6,) + dims and (bits(a) == bits(b)).all()
    gam = host(solve.strain_invariant(sp, dims, xd[:len(dims) * g.N], SCALE[:len(dims)]))
    assert gam.shape == dims and (bits(gam) == bits(a[3])).all()
    g.destroy()


# ---- 3. grad against ChebPlan.mult ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nv", CASES, ids=case_ids)
def test_grad_agrees_with_chebplan(dims, nv):
    """Both are one sweep of the same line: each within (n + 8) 2^-53 B of the truth, so within twice that of each other."""
    d = len(dims)
    x = data(dims, nv, "noise")
    nf = nv * d
    xd = dev(x)
    g = sp.ChebGrad(dims)
    out = host(g.grad(xd)).reshape((nf, d) + dims)
    _, B = table(dims, nv, "noise")
    for k in range(d):
        plan = sp.ChebPlan((nf,) + dims, k + 1)
        y = host(plan.mult(xd, torch.empty_like(xd))).reshape((nf,) + dims)
        plan.destroy()
        Bk = np.stack([B[j][k] for j in range(nf)])
        r = gr.ratio(out[:, k], y.astype(LD), 2 * (dims[k] + 8) * Bk)
        assert r <= 1.0, (k, r)
    g.destroy()


# ---- 4. div against DIV of the tensor -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nv", CASES, ids=case_ids)
def test_div_agrees_with_div_of_the_tensor(dims, nv):
    d = len(dims)
    xd = dev(data(dims, nv, "noise"))
    for sc in scales(d):
        g = sp.ChebGrad(dims, sc)
        dv = host(g.div(xd))
        G = g.tensor(xd)
        Dv = host(g.invariants_from(G, ("div",)))
        Gh = host(G).reshape((nv, d, d) + dims)
        _, W = gr.first_order("div", dims, sc, table(dims, nv, "noise"), nv)
        A = np.stack([gr.invariants(Gh[v])["div"][1] for v in range(nv)])
        r = gr.ratio(dv, Dv.astype(LD), W + (d + 4) * A)
        assert r <= 1.0, (sc, r)
        g.destroy()


# ---- 5. run-to-run bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nv", CASES, ids=case_ids)
def test_same_bits_every_run(dims, nv):
    d = len(dims)
    xd = dev(data(dims, nv, "scaled"))
    g = sp.ChebGrad(dims, SCALE[:d])
    for op in ops_of(d) + ["laplacian"]:
        a = host(getattr(g, op)(xd))
        b = host(getattr(g, op)(xd))
        assert (bits(a) == bits(b)).all(), op
    G = g.tensor(dev(data(dims, nv, "noise")))
    assert (bits(host(g.invariants_from(G, gr.NAMES))) == bits(host(g.invariants_from(G, gr.NAMES)))).all()
    assert (bits(host(g.tensor(xd))) == bits(host(g.grad(xd)))).all()      # the same call under another name
    g.destroy()


# ---- 6. exact fields ------------------------------------------------------------------------------------------------------------
def test_exact_fields():
    """grad(x_0^2 x_1 + x_2) = (2 x_0 x_1, x_0^2, 1) and curl(Omega x r) = 2 Omega on (9, 8, 7): within the bars, with one more
    unit per term for the rounding of the sampled field (an input perturbation of 2^-53 |u| moves a term by at most 2^-53 B)."""
    dims = (9, 8, 7)
    X = np.meshgrid(*[np.cos(lw.PI_L * np.arange(n).astype(LD) / LD(n - 1)) for n in dims], indexing="ij")
    g = sp.ChebGrad(dims)
    phi = (X[0] * X[0] * X[1] + X[2]).astype(np.float64)[None]
    out = host(g.grad(dev(phi)))
    _, W = gr.first_order("grad", dims, None, gr.derivs(dims, phi), 1)
    want = [2 * X[0] * X[1], X[0] * X[0], np.ones(dims, dtype=LD)]
    for k in range(3):
        c = dims[k] + 8 + 1
        assert gr.ratio(out[k], want[k], W[k] * (c + 1) / c) <= 1.0, k
    om = (0.75, -1.25, 2.0)
    u = np.stack([om[1] * X[2] - om[2] * X[1], om[2] * X[0] - om[0] * X[2], om[0] * X[1] - om[1] * X[0]]).astype(np.float64)
    w = host(g.curl(dev(u)))
    _, W = gr.first_order("curl", dims, None, gr.derivs(dims, u), 1)
    for i in range(3):
        c = max(dims) + 8 + 2
        assert gr.ratio(w[i], np.full(dims, 2 * om[i], dtype=LD), W[i] * (c + 1) / c) <= 1.0, i
    g.destroy()


# ---- the argument errors that need a handle -------------------------------------------------------------------------------------
def test_argument_errors_with_a_handle():
    L = sp.lib()
    for dims in ((8,), (4, 4, 4, 4)):
        g = sp.ChebGrad(dims)
        x = torch.zeros(len(dims) * g.N, dtype=torch.float64, device="cuda")
        with pytest.raises(sp.ChebhipError) as e:
            g.curl(x)
        assert e.value.code == 4 and "curl" in str(e.value)
        g.destroy()
    g = sp.ChebGrad((6, 5))
    buf = torch.zeros(8 * g.N, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = buf.data_ptr()
    assert L.cheb_grad_grad(g._h, 1, p, p + 8 * (g.N - 1), st) == 4 and b"overlap" in L.chebhip_last_error()
    assert L.cheb_grad_div(g._h, 1, p, p + 8 * g.N, st) == 4                       # the second component is the output
    assert L.cheb_grad_strain(g._h, 1, p + 8 * 3 * g.N, p + 8 * g.N, st) == 4      # the last output field is the input
    assert L.cheb_grad_laplacian(g._h, 1, p, None, p, st) == 4
    assert L.cheb_grad_invariants(g._h, 1, p, 63, p + 8 * 3 * g.N, st) == 4
    assert L.cheb_grad_invariants(g._h, 1, p, 0, p + 8 * 4 * g.N, st) == 4 and b"mask" in L.chebhip_last_error()
    assert L.cheb_grad_invariants(g._h, 1, p, 64, p + 8 * 4 * g.N, st) == 4
    assert L.cheb_grad_grad(g._h, 1, None, p, st) == 4
    with pytest.raises(ValueError):
        g.grad(buf[:g.N + 1])
    g.destroy()
    g = sp.ChebGrad((300,))
    b2 = torch.zeros(3 * 300, dtype=torch.float64, device="cuda")
    q = b2.data_ptr()
    assert g.work_size(1) == 300
    assert L.cheb_grad_laplacian(g._h, 1, q, None, q + 8 * 300, st) == 4 and b"work" in L.chebhip_last_error()
    assert L.cheb_grad_laplacian(g._h, 1, q, q + 8 * 100, q + 8 * 600, st) == 4    # the work array overlaps the input
    g.destroy()
    g.destroy()
