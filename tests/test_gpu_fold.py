"""The addressing of the folds: k_modal_fold (csrc/modal.hip), which adds the per-workgroup partial sums of ChebModal.integrate /
spectrum, and k_reduce_fold (csrc/reduce.hip), the same scheme for the per-slice partial sums of ChebReduce.apply: the base of an output's terms, the stride
between them and the partly empty last workgroup (FOLD_OUT = 4 outputs each).  The inputs are small integers (|x| <= 8), so every
partial sum is an integer far below 2^53: any order of additions gives the same double, and the results are compared bit for bit
with an integer NumPy sum.  What this test pins is which partials an output reads, not the order it adds them in (the bits of
random doubles against the previous kernels: tools/fieldpass_bits.py)."""
import numpy as np
import pytest
import torch

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu
sp = ge.load()
SEED = 20261021
NF = 3

# ChebModal.spectrum, dims -> workgroups per field (not exposed; from modal_create): the last extent n = 3 gives lg = 1 (two lanes
# a row), so a wave takes 64 >> 1 = 32 rows a step and a workgroup 4 * 32 = 128; nsteps = ceil(rows / 128) with rows = n_0 n_1 =
# 63, 8190, 9215, and the workgroups are min(nsteps, 1024 / 3 fields) = 1, 64, 72: one term for part 0 alone, one term for each of
# the 64 parts, two terms for the parts 0..7.  The last grid has 3 * (97 + 95 + 3) = 585 outputs: its last fold workgroup holds one.
MODAL = [(9, 7, 3), (91, 90, 3), (97, 95, 3)]
# ChebReduce over direction 0, dims -> slices (from cheb_reduce_create): the last direction is kept (the cols route), the 3 * 3
# lanes of a launch are far below the target, so slices = cap = n_0 / 8 terms each.  NT = 3 * 5 = 15 outputs: a partial last workgroup.
REDUCE = [((264, 5), 33), ((512, 5), 64), ((1024, 5), 128)]
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def ints(rng, shape):
    return rng.integers(-8, 9, size=shape)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(got, want):
    want = np.asarray(want, dtype=np.int64)
    assert np.abs(want).max() < 2 ** 53
    return (np.ascontiguousarray(got).view(np.int64) == want.astype(np.float64).view(np.int64)).all()


@pytest.mark.parametrize("dims", MODAL, ids=ids)
def test_modal_spectrum_of_integers(dims):
    rng = np.random.default_rng([SEED, sum(dims)])
    a = ints(rng, (NF,) + dims)
    h = sp.ChebModal(dims, NF)
    assert h.spectrum_size() == NF * sum(dims)
    E = host(h.spectrum(dev(a)))
    h.destroy()
    sq = a * a
    want = np.concatenate([np.concatenate([sq[f].sum(axis=tuple(j for j in range(len(dims)) if j != k)) for k in range(len(dims))])
                           for f in range(NF)])
    assert E.shape == want.shape and same_bits(E, want)


@pytest.mark.parametrize("dims", MODAL, ids=ids)
def test_modal_integrate_of_integers(dims):
    """The same kernel with one output per field and terms one value apart (1, 64 and 72 workgroups per field again: 128 rows each).
    The Clenshaw-Curtis weights are no integers, so field f is the constant c_f, the three a power of two apart: scaling by a power
    of two commutes with every rounding, so out[f] = c_f out[0] bit for bit if and only if the fields' partials stay apart.
    out[0] itself is the volume 2^d: all terms are positive and a term passes fewer than 256 roundings (three weights, the
    additions of a lane, a wave, a workgroup and the fold), so it is off by less than 256 2^-53 of it."""
    h = sp.ChebModal(dims, NF)
    c = np.array([1.0, 4.0, -16.0])
    u = np.repeat(c, int(np.prod(dims)))
    out = host(h.integrate(dev(u)))
    h.destroy()
    base = out[0]
    assert abs(base - 2.0 ** len(dims)) <= 256 * 2.0 ** -53 * 2.0 ** len(dims)
    assert (np.ascontiguousarray(out).view(np.int64) == (base * c).view(np.int64)).all()      # scaling by a power of two is exact


@pytest.mark.parametrize("dims,slices", REDUCE, ids=ids)
def test_reduce_slices_of_integers(dims, slices):
    rng = np.random.default_rng([SEED, dims[0]])
    u, w = ints(rng, (NF,) + dims), ints(rng, dims[0])
    h = sp.ChebReduce(dims, NF, over=(0,))
    assert h.slices == slices
    h.set_weights(0, w.astype(np.float64))
    out = host(h.apply(dev(u)))
    h.destroy()
    want = np.einsum("i,fij->fj", w, u)
    assert out.shape == want.shape and same_bits(out, want)
