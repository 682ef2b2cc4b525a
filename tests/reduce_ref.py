"""The truth the cheb_reduce_* tests compare against (helper module of test_reduce_host.py / test_gpu_reduce.py): the contraction
of include/chebhip.h restated in numpy long double, direction by direction with tensordot, with the DOUBLE weights the device is
given.  The bar is componentwise: for every output

    |out - truth| <= (T + S + 4) 2^-53 B,      B = sum |W_i| |u_i| |v_i|,   W_i = prod_{k contracted} w_k[i_k],

S = contracted directions, T = prod of their extents = terms per output.  Roundings counted (first order): S - 1 for the product
of the weights, one for u v, two for weight x value (the row's own weight and the product of the others), T - 1 additions in any
order, the fold of the slices included."""
import itertools

import numpy as np

import __graft_entry__ as ge

sp = ge.load()
LD = np.longdouble
U = 2.0 ** -53


def masks(dims):
    """Every non-empty mask up to four directions; beyond: all contracted, the two interleaved ones, single directions 0, 2, 4."""
    d = len(dims)
    if d <= 4:
        return [m for m in itertools.product((0, 1), repeat=d) if any(m)]
    assert d == 5
    return [(1,) * 5, (1, 0, 1, 0, 1), (0, 1, 0, 1, 0), (1, 0, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 0, 1)]


def over(mask):
    return tuple(k for k, c in enumerate(mask) if c)


def out_dims(dims, mask):
    return tuple(n for n, c in zip(dims, mask) if not c)


def cap(dims, mask):
    T = int(np.prod([n for n, c in zip(dims, mask) if c]))
    return T + sum(mask) + 4


def default_weights(dims, mask):
    return [sp.cc_weights(n) if c else None for n, c in zip(dims, mask)]


def mixed_kinds(dims, mask):
    """dnode (last node), point and mean in turn over the contracted directions."""
    kinds, i = [], 0
    for n, c in zip(dims, mask):
        kinds.append([("dnode", n - 1), ("point", 0.3), "mean"][i % 3] if c else None)
        i += bool(c)
    return kinds


def contract(f, mask, ws):
    """f: (nfields,) + dims, any dtype; the contracted directions summed against ws[k] in f's precision, last direction first."""
    for k in range(len(mask) - 1, -1, -1):
        if mask[k]:
            f = np.tensordot(f, np.asarray(ws[k]).astype(f.dtype), axes=([k + 1], [0]))
    return f


def truth_bound(dims, nf, mask, ws, u, v=None):
    """(truth in long double, B in double), each of shape (nfields,) + out_dims."""
    shape = (nf,) + tuple(dims)
    f = u.astype(LD).reshape(shape)
    if v is not None:
        f = f * v.astype(LD).reshape(shape)
    t = contract(f, mask, ws)
    B = contract(np.abs(f), mask, [None if w is None else np.abs(w) for w in ws])
    return t, B.astype(np.float64)


def ratio(out, t, B):
    """The worst |out - truth| / (2^-53 B); an output with B == 0 counts as 0 if it is exactly 0 and as inf otherwise."""
    err = np.abs(np.asarray(out).reshape(t.shape).astype(LD) - t).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(B > 0, err / (U * B), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())
