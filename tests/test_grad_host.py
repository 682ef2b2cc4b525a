"""CPU-side checks of ChebGrad / ChebLayout: the long-double reference of grad_ref.py against itself (exact polynomials, the
vector identities, the invariants against the symmetric / antisymmetric split), the boundary ordering of the layout table against
a BlockIt walk, and the argument errors of cheb_grad_* / cheb_layout_* that are decided before any device use.  The checks that
need a handle (curl at d = 1 or 4, overlapping arrays) are in test_gpu_grad.py / test_gpu_layout.py: without a device no handle
exists.  No device needed."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import grad_ref as gr
import linewise as lw

sp = ge.load()
LD = np.longdouble
UL = 2.0 ** -63          # a few units of the long-double roundoff (2^-64): the bar of identities evaluated in long double


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def nodes(dims):
    """Long-double CGL coordinates of every node, one array per direction."""
    ax = [np.cos(lw.PI_L * np.arange(n).astype(LD) / LD(n - 1)) for n in dims]
    return np.meshgrid(*ax, indexing="ij")


def test_low_degree_polynomials_differentiate_exactly():
    dims = (9, 8, 7)
    X = nodes(dims)
    phi = X[0] * X[0] * X[1] + X[2]
    want = [2 * X[0] * X[1], X[0] * X[0], np.ones(dims, dtype=LD)]
    t, B = gr.derivs(dims, phi[None])
    for k in range(3):
        err = np.abs(t[0][k] - want[k]).astype(np.float64)
        assert (err <= (dims[k] + 8) * UL * B[0][k]).all(), k
    # the Laplacian: 2 x_1
    tl, Wl = gr.laplacian(dims, None, phi[None])
    assert (np.abs(tl[0] - 2 * X[1]).astype(np.float64) <= UL * Wl[0]).all()
    # scale multiplies the derivative, its square the second derivative
    tg, _ = gr.first_order("grad", dims, (0.5, 2.0, 3.0), (t, B), 1)
    for k, s in enumerate((0.5, 2.0, 3.0)):
        assert (np.abs(tg[k] - LD(s) * want[k]).astype(np.float64) <= (dims[k] + 8) * UL * s * B[0][k]).all()


@pytest.mark.parametrize("dims", [(5, 7), (9, 8, 7)])
def test_curl_grad_and_div_curl_vanish(dims):
    d = len(dims)
    rng = np.random.default_rng(7)
    phi = rng.standard_normal((1,) + dims)
    g, _ = gr.first_order("grad", dims, None, gr.derivs(dims, phi), 1)                 # d fields, long double
    dv = gr.derivs(dims, g)
    c, _ = gr.first_order("curl", dims, None, dv, 1)
    # the size of a mixed second derivative: |D_a| (|D_b| |phi|), the largest over the pairs
    mag = np.zeros(dims)
    for a in range(d):
        for b in range(d):
            if a != b:
                mag = np.maximum(mag, lw.bound(lw.dense_D(dims[a]), lw.bound(lw.dense_D(dims[b]), phi[0], b), a))
    assert (np.abs(c).astype(np.float64) <= 4 * (max(dims) + 8) * UL * mag).all()
    if d == 3:
        u = rng.standard_normal((3,) + dims)
        w, _ = gr.first_order("curl", dims, None, gr.derivs(dims, u), 1)
        dw, _ = gr.first_order("div", dims, None, gr.derivs(dims, w), 1)
        mag = np.zeros(dims)
        for a in range(3):
            for b in range(3):
                for j in range(3):
                    if a != b:
                        mag = np.maximum(mag, lw.bound(lw.dense_D(dims[a]), lw.bound(lw.dense_D(dims[b]), u[j], b), a))
        assert (np.abs(dw[0]).astype(np.float64) <= 12 * (max(dims) + 8) * UL * mag).all()


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_invariants_against_the_symmetric_split(d):
    rng = np.random.default_rng(d)
    G = rng.standard_normal((d, d, 11))
    inv = gr.invariants(G)
    g = G.astype(LD)
    S = (g + np.swapaxes(g, 0, 1)) / 2
    Wm = (g - np.swapaxes(g, 0, 1)) / 2
    SS, WW = (S * S).sum(axis=(0, 1)), (Wm * Wm).sum(axis=(0, 1))
    tol = lambda a: 64 * UL * np.asarray(a, dtype=np.float64) + 1e-300
    assert (np.abs(inv["strain2"][0] - SS) <= tol(SS)).all()
    assert (np.abs(inv["vort2"][0] - 2 * WW) <= tol(WW)).all()
    assert (inv["gamma"][0] == inv["strain2"][0] / 2).all()                       # GAMMA = 1/2 STRAIN2, exactly
    assert (inv["q"][0] == inv["vort2"][0] / 4 - inv["strain2"][0] / 2).all()     # Q = 1/4 V - 1/2 S
    assert (np.abs(inv["q"][0] - (WW - SS) / 2) <= tol(WW + SS)).all()
    assert (np.abs(inv["norm2"][0] - (SS + WW)) <= tol(SS + WW)).all()
    assert (np.abs(inv["div"][0] - np.trace(g)) <= tol(np.abs(g).sum(axis=(0, 1)))).all()
    for name, (val, A, T) in inv.items():
        assert (A >= np.abs(val).astype(np.float64) * (1 - 1e-15)).all(), name
    assert [inv[n][2] for n in gr.NAMES] == [d, d * (d - 1) // 2, d * (d + 1) // 2, d * (d + 1) // 2, d * d, d * d]
    if d == 3:                                                                    # VORT2 is |curl u|^2
        w = np.stack([g[2, 1] - g[1, 2], g[0, 2] - g[2, 0], g[1, 0] - g[0, 1]])
        assert (np.abs(inv["vort2"][0] - (w * w).sum(axis=0)) <= tol(inv["vort2"][1])).all()


@pytest.mark.parametrize("dims", [(3,), (3, 4), (4, 3, 5)])
def test_layout_table_is_blockit_order(dims):
    """A plain walk over the nodes in row-major (BlockIt) order, counting interior and boundary nodes separately."""
    want = np.empty(dims, dtype=np.int64)
    g = b = 0
    for ind in np.ndindex(*dims):
        if any(i == 0 or i == n - 1 for i, n in zip(ind, dims)):
            want[ind] = -1 - b
            b += 1
        else:
            want[ind] = g
            g += 1
    assert (gr.layout_map(dims) == want).all()
    got = sp.layout_map(dims)
    assert got.dtype == np.int32 and got.shape == tuple(dims) and (got == want).all()
    assert g == int(np.prod([n - 2 for n in dims])) and g + b == int(np.prod(dims))


def test_argument_errors():
    L = sp.lib()
    h = C.c_void_p()
    ints = lambda v: (C.c_int * len(v))(*v)
    dbl = lambda v: (C.c_double * len(v))(*v)
    one = C.c_void_p(16)                                                          # never dereferenced: the checks come first
    # create: all before any device is touched
    assert L.cheb_grad_create(2, ints([4, 4]), None, None) == 4
    assert L.cheb_grad_create(2, None, None, C.byref(h)) == 3
    assert L.cheb_grad_create(0, ints([4]), None, C.byref(h)) == 3
    assert L.cheb_grad_create(11, ints([2] * 11), None, C.byref(h)) == 3
    assert L.cheb_grad_create(2, ints([4, 1]), None, C.byref(h)) == 1 and b"must be >= 2" in L.chebhip_last_error()
    assert L.cheb_grad_create(2, ints([1025, 4]), None, C.byref(h)) == 4
    assert L.cheb_grad_create(4, ints([1024, 1024, 1024, 2]), None, C.byref(h)) == 3
    assert L.cheb_grad_create(2, ints([4, 4]), dbl([1.0, float("nan")]), C.byref(h)) == 4 and b"scale[1]" in L.chebhip_last_error()
    assert L.cheb_layout_create(2, ints([4, 4]), None) == 4
    assert L.cheb_layout_create(2, None, C.byref(h)) == 3
    assert L.cheb_layout_create(0, ints([4]), C.byref(h)) == 3
    assert L.cheb_layout_create(11, ints([3] * 11), C.byref(h)) == 3
    assert L.cheb_layout_create(2, ints([4, 2]), C.byref(h)) == 1 and b">= 3" in L.chebhip_last_error()
    assert L.cheb_layout_create(2, ints([4, 1]), C.byref(h)) == 1
    assert L.cheb_layout_create(2, ints([1025, 4]), C.byref(h)) == 4
    assert L.cheb_layout_create(4, ints([1024, 1024, 1024, 3]), C.byref(h)) == 3
    assert h.value is None
    assert L.cheb_layout_map_host(2, ints([4, 4]), None) == 4 and L.cheb_layout_map_host(1, ints([2]), ints([0, 0])) == 1
    # entry points: field counts and NULL handles
    for fn in (L.cheb_grad_grad, L.cheb_grad_tensor, L.cheb_grad_div, L.cheb_grad_curl, L.cheb_grad_strain):
        for nf in (0, 17, -1):
            assert fn(None, nf, one, one, None) == 4
            assert b"NULL handle" not in L.chebhip_last_error()
        assert fn(None, 1, one, one, None) == 4 and b"NULL handle" in L.chebhip_last_error()
    for nf in (0, 17):
        assert L.cheb_grad_laplacian(None, nf, one, None, one, None) == 4 and b"input fields" in L.chebhip_last_error()
        assert L.cheb_grad_invariants(None, nf, one, 1, one, None) == 4 and b"input fields" in L.chebhip_last_error()
    assert L.cheb_grad_laplacian(None, 1, one, None, one, None) == 4 and b"NULL handle" in L.chebhip_last_error()
    assert L.cheb_grad_invariants(None, 1, one, 1, one, None) == 4 and b"NULL handle" in L.chebhip_last_error()
    assert L.cheb_grad_size(None) == -1 and L.cheb_grad_work_size(None, 1) == -1
    assert L.cheb_grad_destroy(None) == 4 and L.cheb_layout_destroy(None) == 4
    assert L.cheb_layout_size(None, 0) == -1
    # layout: strides and offsets are checked before the handle is looked at
    for fn, args in ((L.cheb_layout_unpack, lambda nc, si, oi, sb, ob: (None, nc, one, si, oi, one, sb, ob, one, None)),
                     (L.cheb_layout_pack, lambda nc, si, oi, sb, ob: (None, nc, one, one, si, oi, one, sb, ob, None))):
        assert fn(*args(0, 1, 0, 1, 0)) == 4 and b"ncomp" in L.chebhip_last_error()
        assert fn(*args(2, 3, 2, 2, 0)) == 4 and b"interior offset" in L.chebhip_last_error()      # oi + ncomp > si
        assert fn(*args(2, 3, -1, 2, 0)) == 4 and b"interior offset" in L.chebhip_last_error()
        assert fn(*args(2, 3, 1, 2, 1)) == 4 and b"boundary offset" in L.chebhip_last_error()      # ob + ncomp > sb
        assert fn(*args(2, 3, 1, 2, 0)) == 4 and b"NULL handle" in L.chebhip_last_error()
    with pytest.raises(ValueError):
        sp._inv_mask(("gamma", "helicity"))
    with pytest.raises(ValueError):
        sp._inv_mask(())
    assert sp._inv_mask("gamma") == (8, 1) and sp._inv_mask(gr.NAMES) == (63, 6)
    assert [sp.INVARIANTS[n] for n in gr.NAMES] == [1, 2, 4, 8, 16, 32]


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = sp.lib()
    h = C.c_void_p()
    assert L.cheb_grad_create(2, (C.c_int * 2)(8, 8), None, C.byref(h)) == 5 and h.value is None
    assert b"no CPU fallback" in L.chebhip_last_error()
    assert L.cheb_layout_create(2, (C.c_int * 2)(8, 8), C.byref(h)) == 5 and h.value is None
    assert b"no CPU fallback" in L.chebhip_last_error()
    with pytest.raises(sp.ChebhipError):
        sp.ChebGrad((8, 8))
    with pytest.raises(sp.ChebhipError):
        sp.ChebLayout((8, 8))
