"""cheb_dealias_* on the device (ChebDealias): dealiased products and advection terms, element by element against the long-double
application of the library's double host matrices (dealias_ref.py states the bars), against the chebmul / chebder truncations of
separable series, against the composition Resample -> multiply -> sharp ChebModal.filter -> Resample; the handle's behaviour.

Shapes: every boundary of the tiles -- 64 lines, 64 / 128 output points of the plain line products and 64 of the pair kernel, 16-point
chunks, the pair kernel with Q <= 4 (last direction, and Q = 3 in (3, 2)) and Q > 4 ((5, 7, 9) and the explicit fine grids), one to
five directions, the 1024-point limit.  The measured worst ratios are printed (pytest -s) and kept in profiles/dealias/ratios.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from numpy.polynomial import chebyshev as npc

import __graft_entry__ as ge
import dealias_ref as dr
import linewise as lw

pytestmark = pytest.mark.gpu
sp = ge.load()
SEED = 20261018
LD = np.longdouble
U = 2.0 ** -53

# (dims, nfields, fine or None: the 3/2 rule)
CASES = [((2,), 16, None), ((3, 2), 3, None), ((5, 7, 9), 16, None), ((17,), 3, None), ((43,), 1, None), ((85,), 1, None),
         ((86,), 1, None), ((171, 3), 1, None), ((4, 171), 1, None), ((33, 20, 17), 1, None), ((6, 5, 4, 3), 3, None),
         ((8,) * 5, 1, None), ((682,), 1, None),
         ((5, 7, 9), 2, (10, 11, 14)), ((33, 20, 17), 1, (66, 30, 26)), ((9, 70), 2, (140, 70))]


def case_id(c):
    dims, nf, fine = c
    return "x".join(map(str, dims)) + "-f%d" % nf + ("" if fine is None else "-fine" + "x".join(map(str, fine)))


def dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float64).ravel()).cuda()


def host(t, shape):
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(shape)


@functools.lru_cache(maxsize=None)
def data(dims, nf, kind):
    """(u, v, vel, c): N(0, 1), or the same with whole fields scaled by 10^+-100."""
    rng = np.random.default_rng(SEED + sum(dims) + nf)
    d = len(dims)
    u, v, c = (rng.standard_normal((nf,) + dims) for _ in range(3))
    vel = rng.standard_normal((d,) + dims)
    if kind == "scaled":
        e = lambda f, step: 10.0 ** (100 * (-1) ** ((np.arange(f) // step) % 2)).reshape((f,) + (1,) * d)
        u, v, c, vel = u * e(nf, 1), v * e(nf, 2), c * e(nf, 1), vel * 1e100
    for a in (u, v, c, vel):
        a.setflags(write=False)
    return u, v, vel, c


@functools.lru_cache(maxsize=None)
def reference(dims, nf, fine, kind):
    """Truths and weights of a case, computed once."""
    u, v, vel, c = data(dims, nf, kind)
    f = fine or dr.fine_dims(dims)
    return dr.multiply_truth_bound(dims, f, u, v), dr.advect_truth_bound(dims, f, vel, c)


@pytest.mark.parametrize("kind", ["normal", "scaled"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_per_element(case, kind):
    dims, nf, fine = case
    u, v, vel, c = data(dims, nf, kind)
    (tm, Bm), (ta, Ba) = reference(dims, nf, fine, kind)
    h = sp.ChebDealias(dims, nf, fine)
    assert h.fine == (fine or dr.fine_dims(dims)) and h.size() == u.size
    cap = dr.cap_multiply(dims, h.fine)
    shape = (nf,) + dims
    rm, _ = lw.check(host(h.multiply(dev(u), dev(v)), shape), tm, Bm, cap, "multiply %s" % case_id(case))
    ra, _ = lw.check(host(h.advect(dev(vel), dev(c)), shape), ta, Ba, cap + len(dims), "advect %s" % case_id(case))
    print("\n%-28s %-6s multiply %.3f of cap %d, advect %.3f of cap %d" % (case_id(case), kind, rm, cap, ra, cap + len(dims)))
    h.destroy()


@pytest.mark.parametrize("dims", [(2,), (9,), (6, 5), (5, 7, 9), (4, 3, 6, 5)], ids=lambda d: "x".join(map(str, d)))
def test_top_mode_squares_to_one_half(dims):
    """u = T_N along one direction: the nodal square is 1 everywhere, the truncation of T_N^2 = (T_0 + T_2N) / 2 is 1/2."""
    h = sp.ChebDealias(dims)
    cap = dr.cap_multiply(dims, h.fine)
    for k, n in enumerate(dims):
        line = (-1.0) ** np.arange(n)
        u = np.broadcast_to(line.reshape((1,) * (k + 1) + (n,) + (1,) * (len(dims) - k - 1)), (1,) + dims).copy()
        assert (u * u == 1.0).all()
        ud = dev(u)
        _, B = dr.multiply_truth_bound(dims, h.fine, u, u)
        lw.check(host(h.multiply(ud, ud), (1,) + dims), np.full((1,) + dims, LD(0.5)), B, cap, "T_N^2 direction %d" % k)
    h.destroy()


@pytest.mark.parametrize("dims", [(9,), (6, 7), (5, 6, 9), (4, 5, 3, 6)], ids=lambda d: "x".join(map(str, d)))
def test_separable_series(dims):
    """Products of 1-d series: the truncation of the product is the product of the chebmul truncations, that of vel . grad c the
    sum over k of the same with chebder in direction k.  Normwise 1e-10, the project's parity bar."""
    rng = np.random.default_rng(SEED + len(dims))
    d = len(dims)
    a, b = ([rng.standard_normal(n) for n in dims] for _ in range(2))
    w = [[rng.standard_normal(n) for n in dims] for _ in range(d)]
    u, v = dr.separable(dims, a), dr.separable(dims, b)
    vel = np.stack([dr.separable(dims, w[k]) for k in range(d)])
    ref_mul = dr.separable(dims, [dr.trunc_mul(a[j], b[j], dims[j]) for j in range(d)])
    ref_adv = sum(dr.separable(dims, [dr.trunc_mul(w[k][j], npc.chebder(b[j]) if j == k else b[j], dims[j]) for j in range(d)])
                  for k in range(d))
    h = sp.ChebDealias(dims)
    rel = lambda g, r: np.linalg.norm(g.ravel() - r.ravel()) / np.linalg.norm(r)
    assert rel(host(h.multiply(dev(u), dev(v)), dims), ref_mul) <= 1e-10
    assert rel(host(h.advect(dev(vel), dev(v)), dims), ref_adv) <= 1e-10
    # the nodal product is NOT the truncation
    assert rel(u * v, ref_mul) > 1e-3
    h.destroy()


@pytest.mark.parametrize("dims", [(17,), (12, 9), (33, 20, 17)], ids=lambda d: "x".join(map(str, d)))
def test_against_the_composition(dims):
    """Resample up, torch multiply, sharp ChebModal.filter keeping n modes per direction, Resample down."""
    u, v, _, _ = data(dims, 1, "normal")
    h = sp.ChebDealias(dims)
    fine = h.fine
    up, down, modal = sp.Resample(dims, fine), sp.Resample(fine, dims), sp.ChebModal(fine)
    for k, (n, m) in enumerate(zip(dims, fine)):
        modal.set_filter(k, sp.sharp_filter(m, n))
    nfine = int(np.prod(fine))
    U_, V_, W_ = (torch.empty(nfine, dtype=torch.float64, device="cuda") for _ in range(3))
    up.apply(dev(u), U_); up.apply(dev(v), V_)
    modal.filter(U_ * V_, W_)
    ref = host(down.apply(W_, torch.empty(u.size, dtype=torch.float64, device="cuda")), dims)
    got = host(h.multiply(dev(u), dev(v)), dims)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) <= 1e-10
    for o in (h, up, down, modal):
        o.destroy()


def test_squares_nan_isolation_and_bits():
    dims, nf = (5, 7, 9), 16
    u, v, vel, c = data(dims, nf, "normal")
    (tm, Bm), _ = reference(dims, nf, None, "normal")
    h = sp.ChebDealias(dims, nf)
    cap = dr.cap_multiply(dims, h.fine)
    ud, vd, veld, cd = dev(u), dev(v), dev(vel), dev(c)
    # u is v: squares
    tsq, Bsq = dr.multiply_truth_bound(dims, h.fine, u, u)
    sq = h.multiply(ud, ud)
    lw.check(host(sq, (nf,) + dims), tsq, Bsq, cap, "squares")
    assert torch.equal(sq, h.multiply(ud, ud.clone()))
    # two runs: identical bits
    m1, a1 = h.multiply(ud, vd), h.advect(veld, cd)
    assert torch.equal(m1, h.multiply(ud, vd)) and torch.equal(a1, h.advect(veld, cd))
    # a NaN in field 5 stays in field 5
    un, cn = u.copy(), c.copy()
    un[5, 2, 3, 4] = np.nan; cn[5, 0, 0, 0] = np.nan
    mn, an = host(h.multiply(dev(un), vd), (nf,) + dims), host(h.advect(veld, dev(cn)), (nf,) + dims)
    keep = np.arange(nf) != 5
    assert np.isnan(mn[5]).any() and np.isnan(an[5]).any()
    assert mn[keep].tobytes() == host(m1, (nf,) + dims)[keep].tobytes()
    assert an[keep].tobytes() == host(a1, (nf,) + dims)[keep].tobytes()
    h.destroy()


@pytest.mark.parametrize("dims", [(17,), (5, 7, 9)], ids=lambda d: "x".join(map(str, d)))
def test_unpadded_and_two_n_rule(dims):
    u, v, _, _ = data(dims, 1, "normal")
    ud, vd = dev(u), dev(v)
    shape = (1,) + dims
    # fine == dims: R = P = I, the nodal product
    h0 = sp.ChebDealias(dims, 1, fine=dims)
    t0, B0 = dr.multiply_truth_bound(dims, dims, u, v)
    assert np.array_equal(t0.astype(np.float64), u * v)
    lw.check(host(h0.multiply(ud, vd), shape), t0, B0, dr.cap_multiply(dims, dims), "fine = dims")
    # the 2n rule and the 3/2 rule truncate the same polynomial: each is within its own bar of it (a K + 8 already holds the
    # rounding of the matrix entries), so the two differ by at most the sum of the two bars
    h32, h2 = sp.ChebDealias(dims), sp.ChebDealias(dims, 1, fine=tuple(2 * n for n in dims))
    o32, o2 = host(h32.multiply(ud, vd), shape), host(h2.multiply(ud, vd), shape)
    _, B32 = dr.multiply_truth_bound(dims, h32.fine, u, v)
    _, B2 = dr.multiply_truth_bound(dims, h2.fine, u, v)
    bar = U * (dr.cap_multiply(dims, h32.fine) * B32 + dr.cap_multiply(dims, h2.fine) * B2)
    assert (np.abs(o32 - o2) <= bar).all(), float((np.abs(o32 - o2) / bar).max())
    for h in (h0, h32, h2):
        h.destroy()


@pytest.mark.parametrize("case", [((8,), 1), ((6, 9), 3), ((5, 7, 9), 16), ((6, 5, 4, 3), 1), ((4,) * 5, 2)], ids=lambda c: case_id(c + (None,)))
def test_work_bytes(case):
    """At most 8 (nfields prod(m) + 2 F prod(m) n_l / m_l) bytes plus the matrices, F = 2 nfields operand fields for multiply and
    d (1 + nfields) once advect has reserved; l with the smallest n_l / m_l is the strictest reading of the bound."""
    dims, nf = case
    h = sp.ChebDealias(dims, nf)
    d, fine = len(dims), h.fine
    pm = int(np.prod(fine))
    img = min(pm // m * n for n, m in zip(dims, fine))
    matrices = 8 * sum(3 * n * m for n, m in set(zip(dims, fine)))
    assert matrices < h.work_bytes() <= 8 * (nf * pm + 2 * (2 * nf) * img) + matrices
    h.reserve_advect()
    assert h.work_bytes() <= 8 * (nf * pm + 2 * d * (1 + nf) * img) + matrices
    h.destroy()


def test_interface():
    L = sp.lib()
    dims = (6, 5)
    h = sp.ChebDealias(dims, 2)
    u, v = dev(np.ones((2,) + dims)), dev(np.ones((2,) + dims))
    vel = dev(np.ones((2,) + dims))
    out = torch.empty_like(u)
    # the C call before the reservation
    assert L.cheb_dealias_advect(h._h, vel.data_ptr(), u.data_ptr(), out.data_ptr(), None) == 4
    assert b"reserve_advect" in L.chebhip_last_error()
    # the Python method reserves on first use
    before = h.work_bytes()
    assert h.advect(vel, u, out) is out and h.work_bytes() > before
    assert L.cheb_dealias_advect(h._h, vel.data_ptr(), u.data_ptr(), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    # overlap
    for call in (lambda: h.multiply(u, v, out=u), lambda: h.multiply(u, v, out=v), lambda: h.advect(vel, u, out=u),
                 lambda: h.advect(vel, u, out=vel)):
        with pytest.raises(sp.ChebhipError) as e:
            call()
        assert e.value.code == 4
    both = torch.empty(3 * u.numel(), dtype=torch.float64, device="cuda")
    with pytest.raises(sp.ChebhipError):
        h.multiply(both[:u.numel()], v, out=both[u.numel() - 1:2 * u.numel() - 1])
    with pytest.raises(AssertionError):
        h.multiply(u[:-1], v)
    h.destroy()
    # the limit of the default rule
    with pytest.raises(sp.ChebhipError) as e:
        sp.ChebDealias((683,))
    assert e.value.code == 4
    with pytest.raises(sp.ChebhipError):
        sp.ChebDealias((8, 8), fine=(12, 7))
    with pytest.raises(ValueError):
        sp.ChebDealias((8, 8), fine=(12,))
    h = sp.ChebDealias((683,), fine=(1024,))
    assert h.fine == (1024,)
    h.destroy()
