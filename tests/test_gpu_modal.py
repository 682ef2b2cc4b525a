"""cheb_modal_* on the device (ChebModal): coefficient transforms, filters, spectra and Clenshaw-Curtis integrals against the host
matrices (element by element in one direction and as tensor products, there also normwise), against numpy's own Chebyshev
recurrence, on single modes and single nodes; round trips, projections, run-to-run bits; the interface.

The tensor products are held to the bar of resample_ref.py: |y - truth| <= cap 2^-53 B per element, truth the long-double
application of the double host matrices, B = (x |M_k|) |x|, cap = sum of n_k + 8 over the directions that are not dropped.
Worst ratios measured on an MI355X (printed with pytest -s; profiles/modal/ratios.txt holds one line per test id and input kind,
written where MODAL_RATIOS_OUT names a file):
  test_tensor_product_parity      72 figures, worst 23.9 (cap 1032) at [1024-f16] noise filter (12, 20);
                                  nearest to its cap: 4.6 of 40 at [12x12x12x12x12-f1] noise filter
  test_dropped_directions          1 figure,  2.5 (cap  15) at [5x7x9-f16] (11, 1, 0, 3)
  test_odd_element_offsets         1 figure,  0.3 (cap  68) at [20x15x9-f3] (2, 9, 2, 1)
  test_non_default_stream_ordering 1 figure,  0.1 (cap 312) at [96x96x96-f1] (0, 75, 68, 4)"""
import functools
import os
from importlib import import_module

import numpy as np
import pytest
import torch
from numpy.polynomial import chebyshev as npcheb

import __graft_entry__ as ge
import linewise as lw
import resample_ref as rr

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = 20240229
LD = np.longdouble
U = 2.0 ** -53
RATIOS = []                       # (test, case, kind, worst ratio, cap, element)


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("MODAL_RATIOS_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |y - truth| / (2^-53 B) per test id and input kind (tests/test_gpu_modal.py); cap = sum of n_k + 8 over the directions not dropped\n")
            for test, case, kind, r, cap, idx in RATIOS:
                f.write("%-28s %-20s %-18s %8.3f of cap %4d at %s\n" % (test, case, kind, r, cap, idx))


def held(test, case, kind, mats, x, y, dims, nf):
    """The per-element bar of resample_ref.py on nf stacked fields: printed, recorded, asserted."""
    t, B, cap = rr.chain_truth_bound(mats, np.asarray(x).reshape((nf,) + tuple(dims)), first_axis=1, skip_identities=False)
    ratio, idx = lw.check(np.asarray(y).reshape(t.shape), t, B, cap, "%s %s %s" % (test, case, kind))
    print("%-28s %-20s %-18s %8.3f of cap %4d at %s" % (test, case, kind, ratio, cap, idx))
    RATIOS.append((test, case, kind, ratio, cap, idx))

# every boundary of the GEMM tiles and of the reductions' vector paths: 64 lines, 64 / 128 output points, 16-point chunks, Q <= 4
# against Q > 4, odd rows and odd field sizes (8-byte aligned rows and fields), one to five directions
CASES = [((2,), 16), ((3, 2), 3), ((5, 7, 9), 16), ((17,), 3), ((1024,), 16), ((257, 4), 1), ((4, 257), 3), ((63, 64, 65), 1),
         ((66, 65, 64), 3), ((129, 3, 16), 16), ((6, 5, 4, 3), 3), ((12,) * 5, 1)]
ORACLE = [((33, 20, 17), 1), ((2, 3, 66), 3), ((65, 64, 5), 1), ((16, 16, 16, 3), 3)]
case_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).ravel()).cuda()


def new(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def along(mats, x, dims, nf):
    """numpy: the matrices (None: identity) applied direction by direction to nf stacked fields, in x's precision."""
    t = x.reshape((nf,) + tuple(dims))
    for k, M in enumerate(mats):
        if M is not None:
            t = np.moveaxis(np.tensordot(M, t, axes=([1], [k + 1])), 0, k + 1)
    return t.ravel()


def sigmas(dims):
    """The filter of a case: direction 0 exponential (sharp at n > 257, where the host product of a full sigma is the cost),
    the last direction sharp, the others unset."""
    n0 = dims[0]
    s = [None] * len(dims)
    s[0] = sp.exp_filter(n0, order=8, cutoff=n0 // 3) if n0 <= 257 else sp.sharp_filter(n0, n0 // 3)
    if len(dims) > 1:
        s[-1] = sp.sharp_filter(dims[-1], (2 * dims[-1] + 2) // 3)
    return s


def proj_sigmas(dims):
    s = sigmas(dims)
    if dims[0] <= 257:
        s[0] = None
    s[-1] = sp.sharp_filter(dims[-1], (2 * dims[-1] + 2) // 3) if len(dims) > 1 or dims[0] <= 257 else s[0]
    return s


def spectrum_ok(E, a, dims, nf):
    """Every bin within (L_k + 8) 2^-53 E of the long-double sum of squares (L_k terms per bin, all non-negative)."""
    sq = a.astype(LD).reshape((nf,) + tuple(dims)) ** 2
    E = E.reshape(nf, sum(dims))
    o, ok = 0, True
    for k, n in enumerate(dims):
        ref = sq.sum(axis=tuple(j + 1 for j in range(len(dims)) if j != k))
        ok = ok and bool((np.abs(E[:, o:o + n] - ref) <= (np.prod(dims) // n + 8) * U * ref).all())
        o += n
    return ok


def weights(dims):
    """prod_k w_k[i_k] on the grid, long double products of the double weights."""
    W = np.ones((1,) * len(dims), dtype=LD)
    for k, n in enumerate(dims):
        W = W * sp.cc_weights(n).astype(LD).reshape([-1 if m == k else 1 for m in range(len(dims))])
    return W


@functools.lru_cache(maxsize=None)
def case(dims, nf):
    """One run of everything on N(0, 1) data, shared by the tests below: inputs and device results as host arrays."""
    m = sp.ChebModal(dims, nf)
    rng = np.random.default_rng(SEED + sum(dims) + nf)
    u, v = rng.standard_normal(m.size()), rng.standard_normal(m.size())
    ud, vd = dev(u), dev(v)
    a = m.forward(ud, new(m.size()))
    r = dict(u=u, v=v, a=host(a), back=host(m.backward(ud, new(m.size()))), trip=host(m.backward(a, new(m.size()))),
             E=host(m.spectrum(a, new(m.spectrum_size()))), E2=host(m.spectrum(a)),
             I=host(m.integrate(ud, out=new(nf))), I2=host(m.integrate(ud)), Iuv=host(m.integrate(ud, vd)), Iuu=host(m.integrate(ud, ud)),
             copy=host(m.filter(ud, new(m.size()))))
    sig = sigmas(dims)
    for k, s in enumerate(sig):
        m.set_filter(k, s)
    f1 = m.filter(ud, new(m.size()))
    r.update(sig=sig, f1=host(f1), f1b=host(m.filter(ud, new(m.size()))))
    for k, s in enumerate(proj_sigmas(dims)):                      # sharp filters only, applied twice: a projection
        m.set_filter(k, s)
    p1 = m.filter(ud, new(m.size()))
    r.update(p1=host(p1), p2=host(m.filter(p1, new(m.size()))))
    m.destroy()
    return r


@functools.lru_cache(maxsize=None)
def case_scaled(dims, nf):
    """The transforms and the filter of case() on fields scaled by 10^+100 and 10^-100 in turn."""
    m = sp.ChebModal(dims, nf)
    u = np.random.default_rng(SEED + sum(dims) + nf + 1).standard_normal((nf,) + tuple(dims))
    u *= (10.0 ** (100 * (-1) ** np.arange(nf))).reshape((nf,) + (1,) * len(dims))
    ud = dev(u)
    r = dict(u=u.ravel(), a=host(m.forward(ud, new(m.size()))), back=host(m.backward(ud, new(m.size()))))
    for k, s in enumerate(sigmas(dims)):
        m.set_filter(k, s)
    r.update(f1=host(m.filter(ud, new(m.size()))))
    m.destroy()
    return r


# ---- 1. one direction, element by element ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 17, 64, 65, 257, 1024])
def test_one_direction_elementwise(n):
    """|y_i - truth_i| <= (n + 8) 2^-53 sum_j |M_ij| |x_j|: one rounding per entry, n for the sum in any order and a few more (the
    project's per-element bar without the even/odd term); truth: the long-double product with the host matrix."""
    m = sp.ChebModal((n,), 16)
    x = np.random.default_rng(SEED + n).standard_normal((16, n))
    xd = dev(x)
    for which, fn in (("forward", m.forward), ("backward", m.backward)):
        M = sp.modal_matrix(n, which)
        y = host(fn(xd, new(16 * n))).reshape(16, n)
        truth = np.dot(x.astype(LD), np.asfortranarray(M.astype(LD).T))
        bound = (n + 8) * U * (np.abs(x) @ np.abs(M).T)
        ratio = (np.abs(y - truth) / bound).max()
        print("n = %d %s: max error / bound = %.3f" % (n, which, ratio))
        assert np.isfinite(y).all() and ratio <= 1.0
    m.destroy()


# ---- 2. tensor products against the host matrices -------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_tensor_product_parity(dims, nf):
    r = case(dims, nf)
    T = [sp.modal_matrix(n, "forward") for n in dims]
    B = [sp.modal_matrix(n, "backward") for n in dims]
    F = [None if s is None else sp.filter_matrix(n, s) for n, s in zip(dims, r["sig"])]
    for name, got, ref in (("forward", r["a"], along(T, r["u"], dims, nf)), ("backward", r["back"], along(B, r["u"], dims, nf)),
                           ("filter", r["f1"], along(F, r["u"], dims, nf))):
        err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print("%s %s: %.2e" % (case_ids(dims), name, err))
        assert np.isfinite(got).all() and err <= 1e-13, name
    cid = "%s-f%d" % (case_ids(dims), nf)
    for kind, rc in (("noise", r), ("scaled", case_scaled(dims, nf))):
        for name, key, mats in (("forward", "a", T), ("backward", "back", B), ("filter", "f1", F)):
            held("tensor_product_parity", cid, kind + "-" + name, mats, rc["u"], rc[key], dims, nf)


# ---- 3. numpy's Chebyshev recurrence as an independent oracle -------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", ORACLE, ids=case_ids)
def test_independent_oracle(dims, nf):
    """Random coefficients, values by numpy.polynomial.chebyshev.chebvander (its recurrence, none of our matrices): forward returns
    the coefficients, integrate the exact integral sum a prod 2 / (1 - k^2) over the even multi-indices, and a sharp filter removes
    exactly the modes at and above `keep`."""
    rng = np.random.default_rng(SEED + sum(dims))
    a = rng.standard_normal((nf,) + dims)
    V = [npcheb.chebvander(np.cos(np.pi * np.arange(n) / (n - 1)), n - 1) for n in dims]
    u = along(V, a, dims, nf)
    m = sp.ChebModal(dims, nf)
    ud = dev(u)
    got = host(m.forward(ud, new(m.size())))
    err = np.linalg.norm(got - a.ravel()) / np.linalg.norm(a)
    print("%s coefficients: %.2e" % (case_ids(dims), err))
    assert err <= 1e-12

    I = [np.where(np.arange(n) % 2 == 0, LD(2) / np.where(np.arange(n) % 2 == 0, 1 - np.arange(n, dtype=LD) ** 2, LD(1)), LD(0)) for n in dims]
    exact = a.astype(LD)
    for Ik in I:
        exact = np.tensordot(exact, Ik, axes=([1], [0]))
    integ = host(m.integrate(ud))
    bound = (np.prod(dims) + 8) * U * (weights(dims)[None] * np.abs(u.reshape((nf,) + dims))).reshape(nf, -1).sum(axis=1)
    print("%s integral: max error / bound = %.3f" % (case_ids(dims), (np.abs(integ - exact) / bound).max()))
    assert (np.abs(integ - exact) <= bound).all()

    keep = [max(1, (2 * n) // 3) for n in dims]
    mask = np.ones(dims)
    for k, n in enumerate(dims):
        m.set_filter(k, sp.sharp_filter(n, keep[k]))
        mask = mask * (np.arange(n) < keep[k]).reshape([-1 if j == k else 1 for j in range(len(dims))])
    fa = host(m.forward(m.filter(ud, new(m.size())), new(m.size())))
    assert np.linalg.norm(fa - (a * mask[None]).ravel()) <= 1e-12 * np.linalg.norm(a)
    m.destroy()


# ---- 4. single modes and single nodes -------------------------------------------------------------------------------------------
def test_single_mode():
    dims, mode = (9, 4, 8), (3, 0, 5)
    x = [np.cos(np.pi * np.arange(n) / (n - 1)) for n in dims]
    u = np.einsum("i,j,k->ijk", *[npcheb.chebval(xk, np.eye(n)[q]) for xk, n, q in zip(x, dims, mode)])
    m = sp.ChebModal(dims)
    a = m.forward(dev(u), new(m.size()))
    E = host(m.spectrum(a))
    a = host(a).reshape(dims)
    assert abs(a[mode] - 1.0) <= 1e-14
    a[mode] = 0.0
    assert np.abs(a).max() <= 1e-14
    o = 0
    for n, q in zip(dims, mode):
        Ek = E[o:o + n].copy(); o += n
        assert abs(Ek[q] - 1.0) <= 1e-13
        Ek[q] = 0.0
        assert Ek.max() <= 1e-26 and Ek.min() >= 0.0
    m.destroy()


def test_single_nodes():
    """u = e_i at a corner, on an edge, on a face and inside, one node per field of 16 fields of odd size: any wrong weight or index
    map shows."""
    dims = (5, 7, 9)
    nodes = [(0, 0, 0), (4, 6, 8), (0, 0, 4), (0, 3, 8), (2, 6, 0), (0, 3, 4), (2, 0, 5), (1, 2, 8), (2, 3, 4), (1, 1, 1), (3, 5, 7),
             (4, 0, 0), (0, 6, 0), (3, 6, 8), (4, 3, 3), (1, 5, 2)]
    u = np.zeros((16,) + dims)
    for f, i in enumerate(nodes):
        u[(f,) + i] = 1.0
    m = sp.ChebModal(dims, 16)
    got = host(m.integrate(dev(u)))
    W = weights(dims)
    for f, i in enumerate(nodes):
        assert abs(got[f] - W[i]) <= 8 * U * W[i], (f, i)
    m.destroy()


# ---- 5. spectrum, integrals of N(0, 1) data -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_spectrum_and_integrals(dims, nf):
    """Every bin within (L_k + 8) 2^-53 E of numpy's sum of squares of the device's own coefficients (L_k terms per bin, all
    non-negative); the integrals within (L + 8) 2^-53 sum W |u| (|u v|) of the long-double sums."""
    r = case(dims, nf)
    assert spectrum_ok(r["E"], r["a"], dims, nf)
    W, L = weights(dims)[None], np.prod(dims)
    u, v = (r[q].astype(LD).reshape((nf,) + dims) for q in "uv")
    for got, f in ((r["I"], u), (r["Iuv"], u * v), (r["Iuu"], u * u)):
        ref, mag = (W * f).reshape(nf, -1).sum(axis=1), (W * np.abs(f)).reshape(nf, -1).sum(axis=1)
        assert (np.abs(got - ref) <= (L + 8) * U * mag).all()


# ---- 6. round trip, projection, identity, run-to-run bits -----------------------------------------------------------------------
@pytest.mark.parametrize("dims,nf", CASES, ids=case_ids)
def test_round_trip_projection_bits(dims, nf):
    r = case(dims, nf)
    nu = np.linalg.norm(r["u"])
    assert np.linalg.norm(r["trip"] - r["u"]) <= 1e-13 * nu
    assert np.linalg.norm(r["p2"] - r["p1"]) <= 1e-13 * nu
    assert np.array_equal(r["copy"], r["u"])                      # no sigma set: a copy
    assert np.array_equal(r["f1"], r["f1b"]) and np.array_equal(r["E"], r["E2"]) and np.array_equal(r["I"], r["I2"])


def test_dropped_directions():
    """All ones and cleared directions are dropped: one launch for the one real filter, whose lines along the other directions keep
    the bits of a one-direction handle."""
    dims = (5, 7, 9)
    m = sp.ChebModal(dims, 16)
    u = dev(np.random.default_rng(SEED + 11).standard_normal(m.size()))
    m.set_filter(0, np.ones(5)); m.set_filter(1, sp.exp_filter(7, order=4)); m.set_filter(2, sp.sharp_filter(9, 4)); m.set_filter(2, None)
    c0 = sp.lib().chebhip_launch_count()
    v = m.filter(u, new(m.size()))
    assert sp.lib().chebhip_launch_count() - c0 == 1
    F = [None, sp.filter_matrix(7, sp.exp_filter(7, order=4)), None]
    ref = along(F, host(u), dims, 16)
    assert np.linalg.norm(host(v) - ref) <= 1e-13 * np.linalg.norm(ref)
    held("dropped_directions", "5x7x9-f16", "noise-filter", F, host(u), host(v), dims, 16)            # cap 7 + 8: one direction
    m.destroy()


# ---- 7. interface ---------------------------------------------------------------------------------------------------------------
def test_odd_element_offsets():
    """Tensors that are torch slices starting at an odd element (8-byte, not 16-byte, aligned), rows of odd length."""
    dims, nf = (20, 15, 9), 3
    m = sp.ChebModal(dims, nf)
    n = m.size()
    x = np.random.default_rng(SEED + 5).standard_normal(n)
    bx = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
    by = torch.full((n + 4,), -7.0, dtype=torch.float64, device="cuda")
    bx[1:1 + n] = dev(x)
    m.forward(bx[1:1 + n], by[3:3 + n])
    out = host(by)
    T = [sp.modal_matrix(k, "forward") for k in dims]
    ref = along(T, x, dims, nf)
    assert np.linalg.norm(out[3:3 + n] - ref) <= 1e-13 * np.linalg.norm(ref)
    held("odd_element_offsets", "20x15x9-f3", "noise-forward", T, x, out[3:3 + n], dims, nf)
    assert (out[:3] == -7.0).all() and out[-1] == -7.0                    # nothing written outside the slice
    aligned = dev(x)
    be = torch.full((m.spectrum_size() + 2,), -7.0, dtype=torch.float64, device="cuda")
    bi = torch.full((nf + 2,), -7.0, dtype=torch.float64, device="cuda")
    m.spectrum(bx[1:1 + n], be[1:-1]); m.integrate(bx[1:1 + n], by[3:3 + n], bi[1:-1])
    E, I = host(m.spectrum(aligned)), host(m.integrate(aligned, by[3:3 + n]))
    assert spectrum_ok(E, x, dims, nf)
    f = (x.astype(LD) * out[3:3 + n].astype(LD)).reshape((nf,) + dims)
    Iref, mag = ((weights(dims)[None] * q).reshape(nf, -1).sum(axis=1) for q in (f, np.abs(f)))
    assert (np.abs(I - Iref) <= (n // nf + 8) * U * mag).all()
    # the same sums whatever the alignment (the order of the additions does not depend on it), nothing written outside
    assert np.array_equal(host(be)[1:-1], E) and np.array_equal(host(bi)[1:-1], I)
    assert host(be)[0] == -7.0 and host(be)[-1] == -7.0 and host(bi)[0] == -7.0 and host(bi)[-1] == -7.0
    m.destroy()


def test_non_default_stream_ordering():
    """Everything on a side stream: the input is produced, transformed, integrated and consumed there, read after a synchronise."""
    dims = (96, 96, 96)
    m = sp.ChebModal(dims)
    x = dev(np.random.default_rng(SEED + 7).standard_normal(m.size()))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xin = torch.empty_like(x)
        y = torch.empty(m.size(), dtype=torch.float64, device="cuda")
        for rep in range(3):
            xin.copy_(x).mul_(rep + 1.0)
            m.forward(xin, y)
            z, q, e = y.clone(), m.integrate(xin).clone(), m.spectrum(y).clone()
    s.synchronize()
    x3 = x.cpu().numpy() * 3.0
    T = [sp.modal_matrix(n, "forward") for n in dims]
    ref = along(T, x3, dims, 1)
    assert np.linalg.norm(z.cpu().numpy() - ref) <= 1e-13 * np.linalg.norm(ref)
    held("non_default_stream", "96x96x96-f1", "noise-forward", T, x3, z.cpu().numpy(), dims, 1)
    W = weights(dims).astype(np.float64).ravel()
    assert abs(float(q[0]) - W @ x3) <= 2 * (x3.size + 8) * U * (W @ np.abs(x3))          # (device sum and numpy's dot)
    assert abs(float(e[:96].sum()) - ref @ ref) <= 1e-10 * (ref @ ref)
    m.destroy()


def test_arguments_refused():
    m = sp.ChebModal((8, 8))
    buf = torch.zeros(200, dtype=torch.float64, device="cuda")
    for fn in (m.forward, m.backward, m.filter):
        with pytest.raises(sp.ChebhipError):
            fn(buf[:64], buf[10:74])
        with pytest.raises(sp.ChebhipError):
            fn(buf[:64], buf[:64])
    for k in (-1, 2):
        with pytest.raises(sp.ChebhipError):
            m.set_filter(k, np.ones(8))
        with pytest.raises(sp.ChebhipError):
            m.set_filter(k, None)
    m.destroy()
    for dims, nf in (((), 1), ((4,) * 11, 1), ((4, 1), 1), ((4, 1025), 1), ((4, 4), 0), ((4, 4), 17), ((1024, 1024, 1024, 2), 1),
                     ((1024, 1024, 128), 16)):
        with pytest.raises(sp.ChebhipError):
            sp.ChebModal(dims, nf)


def test_launch_counts():
    count = sp.lib().chebhip_launch_count
    for dims in ((33,), (9, 10), (6, 5, 4, 3)):
        m = sp.ChebModal(dims, 3)
        u, a = dev(np.ones(m.size())), new(m.size())
        c0 = count(); m.forward(u, a); c1 = count(); m.integrate(u, a); c2 = count(); m.spectrum(a); c3 = count(); m.backward(a, u); c4 = count()
        assert c1 - c0 == len(dims) and c4 - c3 == len(dims) and 1 <= c2 - c1 <= 2 and 1 <= c3 - c2 <= 2
        m.destroy()


def test_resolution():
    dims = (12, 13, 14)
    g = np.meshgrid(*[np.cos(np.pi * np.arange(n) / (n - 1)) for n in dims], indexing="ij")
    poly = 1.0 + g[0] ** 3 - 2.0 * g[0] * g[1] ** 2 + 0.5 * g[2] ** 4
    noise = np.random.default_rng(SEED + 13).standard_normal(dims)
    r = solve.resolution(dims, dev(poly))
    assert r.shape == (3,) and (r < 1e-10).all()
    r = solve.resolution(dims, dev(noise))
    assert (r > 0.1).all() and (r < 1.0).all()
    r = solve.resolution(dims, dev(np.stack([poly, noise])))
    assert r.shape == (2, 3) and (r[0] < 1e-10).all() and (r[1] > 0.1).all()
