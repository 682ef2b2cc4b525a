"""cheb_layout_* on the device (ChebLayout): unpack against a numpy scatter built from the boolean interior mask, pack as its
inverse on bits, untouched entries of the targets, and the tie-in with StokesOp: the strain the power-law node loop keeps against
ChebGrad.strain of stokes_fields, the pressure field against the state."""
from importlib import import_module

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import grad_ref as gr

pytestmark = pytest.mark.gpu
sp = ge.load()
solve = import_module(sp.__name__ + ".solve")
SEED = 20261019
SHAPES = [(3,), (3, 3), (4, 5, 6), (5, 4, 3, 3), (20, 18, 16)]
ids = lambda v: "x".join(map(str, v))
# (ncomp, si, oi, sb, ob): interior strides 1 .. 4 with offsets
GEOM = [(1, 1, 0, 1, 0), (1, 2, 1, 3, 2), (2, 3, 1, 2, 0), (3, 4, 0, 3, 0), (3, 4, 1, 4, 1), (1, 4, 3, 1, 0)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).ravel()).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def vectors(dims, si, sb, seed):
    """Random interior and boundary arrays whose bit patterns are all different from 0.0 (and include a NaN and a -0.0)."""
    rng = np.random.default_rng(seed)
    I = int(np.prod([n - 2 for n in dims]))
    B = int(np.prod(dims)) - I
    xi, xb = rng.standard_normal(I * si), rng.standard_normal(B * sb)
    xi[0], xb[0], xb[-1] = np.nan, -0.0, np.inf
    return xi, xb


@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_unpack_is_the_numpy_scatter(dims):
    lay = sp.ChebLayout(dims)
    N = int(np.prod(dims))
    assert (lay.N, lay.I, lay.B) == (N, int(np.prod([n - 2 for n in dims])), N - int(np.prod([n - 2 for n in dims])))
    for i, (nc, si, oi, sb, ob) in enumerate(GEOM):
        xi, xb = vectors(dims, si, sb, SEED + i)
        xid, xbd = dev(xi), dev(xb)
        out = host(lay.unpack(nc, xid, si, oi, xbd, sb, ob))
        assert out.shape == (nc,) + dims
        assert (bits(out) == bits(gr.unpack(dims, nc, xi, si, oi, xb, sb, ob))).all()
        out = host(lay.unpack(nc, xid, si, oi, None))                          # no boundary source: zeros there
        assert (bits(out) == bits(gr.unpack(dims, nc, xi, si, oi, None, 1, 0))).all()
        out = host(lay.unpack(nc, None, 1, 0, xbd, sb, ob))                    # no interior source
        assert (bits(out) == bits(gr.unpack(dims, nc, None, 1, 0, xb, sb, ob))).all()
        assert (bits(host(xid)) == bits(xi)).all() and (bits(host(xbd)) == bits(xb)).all()
    lay.destroy()


@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_pack_inverts_unpack_and_leaves_the_rest_alone(dims):
    lay = sp.ChebLayout(dims)
    sentinel = np.float64(-1.2345678901234567e300)
    for i, (nc, si, oi, sb, ob) in enumerate(GEOM):
        xi, xb = vectors(dims, si, sb, SEED + 100 + i)
        fields = lay.unpack(nc, dev(xi), si, oi, dev(xb), sb, ob)
        ti = torch.full((lay.I * si,), float(sentinel), dtype=torch.float64, device="cuda")
        tb = torch.full((lay.B * sb,), float(sentinel), dtype=torch.float64, device="cuda")
        lay.pack(nc, fields, ti, si, oi, tb, sb, ob)
        for got, src, s, o in ((host(ti), xi, si, oi), (host(tb), xb, sb, ob)):
            got, src = got.reshape(-1, s), src.reshape(-1, s)
            assert (bits(got[:, o:o + nc]) == bits(src[:, o:o + nc])).all()    # pack o unpack: the identity on bits
            rest = np.ones(s, dtype=bool)
            rest[o:o + nc] = False
            assert (bits(got[:, rest]) == bits(sentinel)).all()                # the other interleaved components
        # one target only
        ti.fill_(float(sentinel)); tb.fill_(float(sentinel))
        lay.pack(nc, fields, ti, si, oi, None)
        assert (bits(host(tb)) == bits(sentinel)).all()
        assert (bits(host(ti).reshape(-1, si)[:, oi:oi + nc]) == bits(xi.reshape(-1, si)[:, oi:oi + nc])).all()
        ti.fill_(float(sentinel))
        lay.pack(nc, fields, None, 1, 0, tb, sb, ob)
        assert (bits(host(ti)) == bits(sentinel)).all()
        assert (bits(host(tb).reshape(-1, sb)[:, ob:ob + nc]) == bits(xb.reshape(-1, sb)[:, ob:ob + nc])).all()
    lay.destroy()


def test_argument_errors_with_a_handle():
    L = sp.lib()
    lay = sp.ChebLayout((4, 5))
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(4 * lay.N, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    assert L.cheb_layout_unpack(lay._h, 1, p, 1, 0, None, 1, 0, p + 8, st) == 4 and b"overlap" in L.chebhip_last_error()
    assert L.cheb_layout_pack(lay._h, 1, p, None, 1, 0, p + 8 * (lay.N - 1), 1, 0, st) == 4 and b"overlap" in L.chebhip_last_error()
    assert L.cheb_layout_unpack(lay._h, 1, p, 1, 0, None, 1, 0, None, st) == 4
    assert L.cheb_layout_unpack(lay._h, 2, p, 2, 1, None, 1, 0, p + 8 * 2 * lay.N, st) == 4       # oi + ncomp > si
    assert L.cheb_layout_size(lay._h, 3) == -1
    lay.destroy()
    lay.destroy()


def test_stokes_state_to_fields_and_strain():
    """Power-law rheology, so that the node loop that keeps the strain runs.  Both sides are D sweeps of the same full-grid
    velocity followed by one 1/2 (a + b): each within the strain bar of the truth, so within twice the bar of each other."""
    dims = (10, 9, 8)
    d = len(dims)
    rng = np.random.default_rng(SEED + 7)
    op = sp.StokesOp(dims)
    x = rng.standard_normal(op.global_size)
    dv = rng.standard_normal(op.dirichlet_size)
    op.set_rheology(1, 1.0, 3.0, 1e-2, 1.0)
    op.set_dirichlet(dv)
    op.set_force(np.zeros(op.global_size))
    xd = dev(x)
    op.function(xd, torch.empty_like(xd))
    f = solve.stokes_fields(sp, op, xd, dv)
    assert tuple(f.shape) == (d + 1,) + dims
    fh = host(f)
    inside = gr.interior_mask(dims)
    # the fields are the numpy scatter of the state, the pressure's boundary is zero
    assert (bits(fh[:d]) == bits(gr.unpack(dims, d, x, d + 1, 0, dv, d, 0))).all()
    assert (bits(fh[d][inside]) == bits(x[d::d + 1])).all()
    assert (bits(fh[d][~inside]) == 0).all()
    g = sp.ChebGrad(dims)
    S = host(g.strain(f[:d].reshape(-1)))
    _, W = gr.first_order("strain", dims, None, gr.derivs(dims, fh[:d]), 1)
    kept = [op.get_state(2 + j).reshape(dims + (d,)) for j in range(d)]
    for o, (j, k) in enumerate(gr.npairs(d)):
        r = gr.ratio(kept[j][..., k], S[o].astype(np.longdouble), 2 * W[o])
        assert r <= 1.0, (j, k, r)
    # gamma of the same velocity, through the wrapper
    gam = host(solve.strain_invariant(sp, dims, f[:d]))
    assert (bits(gam) == bits(host(g.invariants(f[:d].reshape(-1), ("gamma",)))[0])).all()
    # the scalar operator's state
    eop = sp.EllipticOp(dims)
    xe, de = rng.standard_normal(eop.global_size), rng.standard_normal(eop.dirichlet_size)
    fe = host(solve.elliptic_field(sp, eop, dev(xe), de))
    assert fe.shape == dims and (bits(fe) == bits(gr.unpack(dims, 1, xe, 1, 0, de, 1, 0)[0])).all()
    g.destroy(); op.destroy(); eop.destroy()
