"""The host side of the box Helmholtz solve and of ChebProject (no device): cheb_helmholtz_line_box_host against
cheb_helmholtz_line_bc_host (s = 1: bit for bit) and against numpy, cheb_project_faces_host against the edge rule, and the numpy
model of tests/project_ref.py against every bar tests/test_gpu_project.py holds the library to."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import project_ref as pr

sp = ge.load()
SIZES = (3, 4, 5, 8, 17, 64, 65, 129, 258)
CONDS = {
    "neumann": "neumann",
    "robin11": (1.0, 1.0),
    "robin3_01": (3.0, 0.1),
    "dir_neu": ("dirichlet", "neumann"),
    "neu_dir": ("neumann", "dirichlet"),
    "robin21_neu": ((2.0, 1.0), "neumann"),
}
SCALES = (0.25, 1.0, 3.5)


@pytest.fixture(scope="module")
def L():
    ge.build()
    return sp.lib()


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


@pytest.mark.parametrize("name", list(CONDS))
@pytest.mark.parametrize("P", SIZES)
def test_line_box(L, P, name):
    bc = CONDS[name]
    M = P - 2
    for s in SCALES:
        S, Si, lam, Q, Lf, Bi = sp.helmholtz_line_box(P, bc, s)
        if s == 1.0:
            for a, b in zip((S, Si, lam, Q, Lf, Bi), sp.helmholtz_line_bc(P, bc)):
                assert np.array_equal(a, b), (P, name)
            continue
        A, Qn, Ln, Bn = pr.scaled_line(P, sp._bc_ends(bc), s)
        res = np.linalg.norm(A @ S - S * lam[None, :]) / max(np.linalg.norm(A) * np.linalg.norm(S), 1e-300)
        assert res <= 1e-13, (s, res)
        assert np.abs(S @ Si - np.eye(M)).max() <= 1e-13
        ev = np.sort(np.linalg.eigvals(A).real)
        assert np.abs(np.sort(lam) - ev).max() <= 1e-12 * np.abs(lam).max()
        assert np.all(lam >= 0.0)
        assert rel(Q, Qn) <= 1e-13 and rel(Lf, Ln) <= 1e-13 and rel(Bi, Bn) <= 1e-13
        if name == "neumann":
            assert np.sum(lam == 0.0) == 1


def test_line_box_is_the_scaled_line(L):
    """lam and L are the unit line's of the ends (alpha, beta s) times s^2, rounded once; S, S^-1, Q, B_BB^-1 are that line's own."""
    for P, bc, s in ((17, (3.0, 0.1), 0.25), (64, ("dirichlet", "neumann"), 3.5), (9, "dirichlet", 2.0)):
        a0, b0, a1, b1 = sp._bc_ends(bc)
        S, Si, lam, Q, Lf, Bi = sp.helmholtz_line_box(P, bc, s)
        S1, Si1, lam1, Q1, L1, Bi1 = sp.helmholtz_line_bc(P, ((a0, b0 * s), (a1, b1 * s)))
        assert np.array_equal(S, S1) and np.array_equal(Si, Si1) and np.array_equal(Q, Q1) and np.array_equal(Bi, Bi1)
        assert rel(lam, s * s * lam1) <= 1e-15 and rel(Lf, s * s * L1) <= 1e-15


def test_line_box_errors(L):
    M = 6
    buf = [np.empty(M * M), np.empty(M * M), np.empty(M), np.empty(2 * M), np.empty(2 * M), np.empty(4)]
    ptrs = [b.ctypes.data_as(C.POINTER(C.c_double)) for b in buf]
    bc = (C.c_double * 4)(0, 1, 0, 1)
    assert L.cheb_helmholtz_line_box_host(8, bc, 2.0, *ptrs) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.cheb_helmholtz_line_box_host(8, bc, bad, *ptrs) == 4, bad
    assert L.cheb_helmholtz_line_box_host(2, bc, 1.0, *ptrs) == 1
    assert L.cheb_helmholtz_line_box_host(259, bc, 1.0, *ptrs) == 4
    assert L.cheb_helmholtz_line_box_host(8, None, 1.0, *ptrs) == 4
    # create_box refuses a bad scale before it touches a device
    h = C.c_void_p()
    dims = (C.c_int * 2)(8, 8)
    good = (C.c_double * 8)(*[0.0, 1.0] * 4)
    for bad in ((1.0, 0.0), (-2.0, 1.0), (1.0, float("nan")), (float("inf"), 1.0)):
        assert L.cheb_helmholtz_create_box(2, dims, good, (C.c_double * 2)(*bad), 0.0, 1, C.byref(h)) == 4, bad
    assert L.cheb_helmholtz_create_box(2, dims, None, (C.c_double * 2)(1.0, 1.0), 0.0, 1, C.byref(h)) == 4
    assert h.value is None
    with pytest.raises(ValueError):
        sp.HelmholtzSolver((8, 8), scale=(1.0, 2.0))                      # scale needs bc
    with pytest.raises(ValueError):
        sp.HelmholtzSolver((8, 8), bc=["neumann", "neumann"], scale=(1.0,))


@pytest.mark.parametrize("dims", [(3,), (9,), (3, 3), (5, 4), (12, 10), (3, 4, 3), (8, 7, 6), (3, 3, 3, 3), (7, 6, 5, 6)],
                         ids=lambda d: "x".join(map(str, d)))
def test_faces_table(L, dims):
    f = sp.project_faces(dims)
    N, G = int(np.prod(dims)), int(np.prod([n - 2 for n in dims]))
    assert f.dtype == np.int32 and f.shape == (N - G,)
    assert np.array_equal(f, pr.face_table(dims))
    # the rule, node by node: k is the highest direction in which the node is an end node
    bnd = np.argwhere(pr.boundary_mask(dims))
    for b, ind in enumerate(bnd):
        ks = [k for k in range(len(dims)) if ind[k] in (0, dims[k] - 1)]
        assert f[b] == 2 * ks[-1] + (ind[ks[-1]] != 0)


def test_faces_errors(L):
    out = (C.c_int * 64)()
    assert L.cheb_project_faces_host(2, (C.c_int * 2)(4, 2), out) == 1
    assert L.cheb_project_faces_host(2, (C.c_int * 2)(4, 259), out) == 4
    assert L.cheb_project_faces_host(0, (C.c_int * 2)(4, 4), out) == 3
    assert L.cheb_project_faces_host(2, (C.c_int * 2)(4, 4), None) == 4
    for bad in (["wall"], "wall", ["wall", "closed"], [("wall", "open", "wall"), "wall"], [1, "wall"]):
        with pytest.raises(ValueError):
            sp._face_codes(bad, 2)
    assert sp._face_codes(["open", ("wall", "open")], 2) == [1, 1, 0, 1] and sp._face_codes(None, 3) is None
    # create refuses these before it touches a device
    h = C.c_void_p()
    d3 = (C.c_int * 3)(8, 7, 6)
    assert L.cheb_project_create(3, d3, None, None, 6, C.byref(h)) == 4                                    # nvec * d > 16
    assert L.cheb_project_create(3, d3, None, None, 0, C.byref(h)) == 4
    assert L.cheb_project_create(3, (C.c_int * 3)(8, 2, 6), None, None, 1, C.byref(h)) == 1
    assert L.cheb_project_create(3, (C.c_int * 3)(8, 259, 6), None, None, 1, C.byref(h)) == 4
    assert L.cheb_project_create(3, d3, (C.c_int * 6)(0, 0, 2, 0, 0, 0), None, 1, C.byref(h)) == 4         # a bad face code
    assert L.cheb_project_create(3, d3, None, (C.c_double * 3)(1.0, 0.0, 1.0), 1, C.byref(h)) == 4         # a bad scale
    assert L.cheb_project_create(3, d3, None, (C.c_double * 3)(1.0, float("nan"), 1.0), 1, C.byref(h)) == 4
    assert L.cheb_project_create(3, d3, None, None, 1, None) == 4
    assert h.value is None
    assert L.cheb_project_size(None, 0) == -1 and L.cheb_project_singular(None) == -1 and L.cheb_project_destroy(None) == 4
    assert L.cheb_project_apply(None, None, None, None, None, None) == 4


MODEL = [((12, 10), (1.0, 3.0)), ((8, 7, 6), (0.5, 2.0, 1.25)), ((7, 6, 5, 6), (0.5, 2.0, 1.25, 0.8))]


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "box"])
@pytest.mark.parametrize("faces", ["walls", "open_first", "open_last"])
@pytest.mark.parametrize("dims,sc", MODEL, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else None)
def test_model_properties(dims, sc, faces, scaled):
    """The numpy model stays inside every bar of test_gpu_project.py (project_ref.py's docstring defines them)."""
    d = len(dims)
    scale = sc if scaled else None
    bc = {"walls": None, "open_first": [("open", "wall")] + ["wall"] * (d - 1), "open_last": ["wall"] * (d - 1) + [("wall", "open")]}[faces]
    kinds = pr.kinds_of(bc, d)
    rng = np.random.default_rng(d * 11 + len(faces) + scaled)
    u = rng.standard_normal((d,) + dims)
    flux = 0.3 * rng.standard_normal(pr.face_table(dims).size) if scaled else None
    out, phi = pr.project(dims, bc, scale, u, flux)
    eps = 1e-9 * np.abs(phi).max()
    assert pr.out_ratio(dims, scale, u, phi, out) <= 1.0
    assert pr.div_ratio(dims, scale, u, phi, out, eps, spread=faces == "walls") <= 1.0
    assert pr.normal_ratio(dims, kinds, scale, out, flux, eps) <= 1.0
    out2, _ = pr.project(dims, bc, scale, out, flux)
    assert pr.node_ratio(dims, scale, out2 - out, eps) <= 1.0
    s = pr.scales(scale, d)
    psi = pr.psi_field(dims, kinds, 5)
    gu = np.stack([s[k] * pr.apply(pr.cheb_d(dims[k]), psi, k) for k in range(d)])
    o3, p3 = pr.project(dims, bc, scale, gu)
    assert pr.node_ratio(dims, scale, o3, 1e-9 * np.abs(p3).max()) <= 1.0
    if faces == "walls":                             # the divergence that is left is ONE constant, and for noise it is not small
        dv = sum(s[k] * pr.apply(pr.cheb_d(dims[k]), out[k], k) for k in range(d))[tuple(slice(1, -1) for _ in dims)]
        assert np.ptp(dv) <= 1e-9 * max(abs(dv.mean()), 1.0)
