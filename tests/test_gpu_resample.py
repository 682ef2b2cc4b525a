"""cheb_resample_apply on the device (Resample): the tensor product of the host interpolation matrices, exact copies of equal
grids, polynomial reproduction, round trips, unaligned tensors and stream ordering."""
import numpy as np
import pytest
import torch

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu
sp = ge.load()
SEED = 20240229


def stored(dims, nodes):
    return tuple(n - 2 if nodes == "interior" else n for n in dims)


def reference(x, dims_in, dims_out, nodes_in, nodes_out, ncomp):
    """numpy float64: the host matrices applied direction by direction."""
    t = x.reshape(stored(dims_in, nodes_in) + (ncomp,))
    for k, (a, b) in enumerate(zip(dims_in, dims_out)):
        R = sp.resample_matrix(a, b, nodes_in, nodes_out)
        t = np.moveaxis(np.tensordot(R, t, axes=([1], [k])), 0, k)
    return t.ravel()


def run(dims_in, dims_out, nodes_in="all", nodes_out="all", ncomp=1, seed=0):
    r = sp.Resample(dims_in, dims_out, nodes_in, nodes_out, ncomp)
    x = np.random.default_rng(SEED + seed).standard_normal(r.size(0))
    y = torch.full((r.size(1),), float("nan"), dtype=torch.float64, device="cuda")
    r.apply(torch.from_numpy(x).cuda(), y)
    torch.cuda.synchronize()
    out = y.cpu().numpy()
    r.destroy()
    return x, out


CASES = [
    ((17,), (33,), "all", "all", 1), ((33,), (17,), "all", "all", 1), ((2,), (1024,), "all", "all", 1), ((1024,), (3,), "all", "all", 1),
    ((257,), (100,), "interior", "all", 1), ((9, 7), (16, 5), "all", "interior", 3), ((3, 2), (257, 4), "all", "all", 4),
    ((12, 9, 20), (15, 24, 8), "all", "all", 3), ((10, 11, 12), (20, 22, 6), "interior", "interior", 4),
    ((6, 5, 4, 3), (7, 9, 4, 5), "all", "interior", 1), ((12, 12, 12, 12, 12), (16, 16, 16, 16, 16), "all", "all", 1),
    ((5, 4, 3, 6, 5), (4, 7, 5, 3, 6), "interior", "all", 3), ((64, 64, 64), (128, 128, 128), "all", "interior", 3),
    ((1024, 2), (5, 1024), "all", "all", 1), ((40, 31), (40, 62), "all", "all", 4),
]


@pytest.mark.parametrize("dims_in,dims_out,nodes_in,nodes_out,ncomp", CASES, ids=lambda v: str(v))
def test_parity_with_host_matrices(dims_in, dims_out, nodes_in, nodes_out, ncomp):
    x, y = run(dims_in, dims_out, nodes_in, nodes_out, ncomp)
    ref = reference(x, dims_in, dims_out, nodes_in, nodes_out, ncomp)
    assert np.isfinite(y).all()
    assert np.linalg.norm(y - ref) <= 1e-13 * np.linalg.norm(ref)


def test_parity_128_to_256():
    x, y = run((128, 128, 128), (256, 256, 256))
    ref = reference(x, (128,) * 3, (256,) * 3, "all", "all", 1)
    assert np.linalg.norm(y - ref) <= 1e-13 * np.linalg.norm(ref)


def test_asymmetric_matrix_layout():
    """An interpolation matrix that is not centro-symmetric (INTERIOR -> ALL of different sizes along the last, contiguous
    direction and along an outer one) catches a transposed or mis-rowed C/D layout."""
    for dims_in, dims_out in (((7, 40), (7, 23)), ((40, 7), (23, 7))):
        r = sp.Resample(dims_in, dims_out, "all", "all")
        x = np.zeros(r.size(0)); x[3] = 1.0
        y = r.apply(torch.from_numpy(x).cuda(), torch.empty(r.size(1), dtype=torch.float64, device="cuda")).cpu().numpy()
        assert np.linalg.norm(y - reference(x, dims_in, dims_out, "all", "all", 1)) <= 1e-14
        r.destroy()


@pytest.mark.parametrize("dims,nodes,ncomp", [((17, 33, 8), "all", 1), ((9, 10, 11), "interior", 3), ((1024, 4), "all", 2)])
def test_equal_grids_copy_bits(dims, nodes, ncomp):
    x, y = run(dims, dims, nodes, nodes, ncomp)
    assert np.array_equal(x, y)


def test_one_changing_direction_keeps_the_others_bits():
    """(9, 17) -> (17, 17): the second direction is the identity and the coincident nodes of the first are unit rows."""
    x, y = run((9, 17), (17, 17))
    assert np.array_equal(y.reshape(17, 17)[::2], x.reshape(9, 17))


@pytest.mark.parametrize("dims_in,dims_out,nodes_in,nodes_out", [((8, 9, 10), (31, 20, 13), "all", "all"),
                                                                 ((12, 12, 12), (24, 24, 24), "interior", "all"),
                                                                 ((40, 30), (9, 11), "all", "interior")])
def test_low_degree_polynomial_reproduced(dims_in, dims_out, nodes_in, nodes_out):
    def field(dims, nodes):
        axes = [np.cos(np.pi * np.arange(n) / (n - 1))[1:n - 1] if nodes == "interior" else np.cos(np.pi * np.arange(n) / (n - 1)) for n in dims]
        g = np.meshgrid(*axes, indexing="ij")
        return (1.0 + g[0] ** 3 - 2.0 * g[0] * g[1] ** 2 + 0.5 * g[-1] ** 4).ravel()
    r = sp.Resample(dims_in, dims_out, nodes_in, nodes_out)
    y = r.apply(torch.from_numpy(field(dims_in, nodes_in)).cuda(), torch.empty(r.size(1), dtype=torch.float64, device="cuda"))
    assert np.abs(y.cpu().numpy() - field(dims_out, nodes_out)).max() <= 1e-12
    r.destroy()


@pytest.mark.parametrize("coarse,fine,nodes,ncomp", [((12, 13, 14), (24, 25, 30), "all", 1), ((10, 10, 10), (21, 19, 18), "interior", 3)])
def test_round_trip(coarse, fine, nodes, ncomp):
    up = sp.Resample(coarse, fine, nodes, nodes, ncomp)
    down = sp.Resample(fine, coarse, nodes, nodes, ncomp)
    x = torch.from_numpy(np.random.default_rng(SEED + 3).standard_normal(up.size(0))).cuda()
    y = up.apply(x, torch.empty(up.size(1), dtype=torch.float64, device="cuda"))
    z = down.apply(y, torch.empty(down.size(1), dtype=torch.float64, device="cuda"))
    assert float((z - x).norm()) <= 1e-13 * float(x.norm())
    up.destroy(); down.destroy()


def test_odd_element_offsets():
    """Input and output tensors that are torch slices starting at an odd element (8-byte, not 16-byte, aligned)."""
    dims_in, dims_out = (20, 15, 9), (31, 8, 16)
    r = sp.Resample(dims_in, dims_out, "all", "all", 3)
    x = np.random.default_rng(SEED + 5).standard_normal(r.size(0))
    bx = torch.zeros(r.size(0) + 3, dtype=torch.float64, device="cuda")
    by = torch.full((r.size(1) + 4,), -7.0, dtype=torch.float64, device="cuda")
    bx[1:1 + r.size(0)] = torch.from_numpy(x).cuda()
    r.apply(bx[1:1 + r.size(0)], by[3:3 + r.size(1)])
    out = by.cpu().numpy()
    ref = reference(x, dims_in, dims_out, "all", "all", 3)
    assert np.linalg.norm(out[3:3 + r.size(1)] - ref) <= 1e-13 * np.linalg.norm(ref)
    assert (out[:3] == -7.0).all() and out[-1] == -7.0                    # nothing written outside the slice
    r.destroy()


def test_non_default_stream_ordering():
    """Everything on a side stream: the input is produced, resampled and consumed there, the result read after a synchronise."""
    dims_in, dims_out = (96, 96, 96), (128, 128, 128)
    r = sp.Resample(dims_in, dims_out)
    x = torch.from_numpy(np.random.default_rng(SEED + 7).standard_normal(r.size(0))).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xin = torch.empty_like(x)
        y = torch.empty(r.size(1), dtype=torch.float64, device="cuda")
        for rep in range(3):
            xin.copy_(x).mul_(rep + 1.0)
            r.apply(xin, y)
            z = y.clone()
    s.synchronize()
    ref = reference(x.cpu().numpy() * 3.0, dims_in, dims_out, "all", "all", 1)
    assert np.linalg.norm(z.cpu().numpy() - ref) <= 1e-13 * np.linalg.norm(ref)
    r.destroy()


def test_overlapping_arguments_refused():
    r = sp.Resample((8, 8), (8, 9))
    buf = torch.zeros(200, dtype=torch.float64, device="cuda")
    with pytest.raises(sp.ChebhipError):
        r.apply(buf[:64], buf[10:82])
    r.destroy()
