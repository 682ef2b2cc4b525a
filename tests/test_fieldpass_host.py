"""What the constructors of the toolbox modules over stacked full-grid fields refuse, word for word: cheb_modal_create(_basis),
cheb_reduce_create, cheb_stats_create and cheb_stats_check, cheb_points_create(_basis), cheb_grad_create(_basis) and
cheb_dealias_create(_basis), each called through ctypes with ONE bad argument at a time.  The return code and the full text of
chebhip_last_error() are asserted.  The modules share their checks (check_field_grid, csrc/ops.h); where a module answers a
mistake in its own words or with its own code, the table below says so.  The argument checks come before any device is touched:
no device needed.  The expected strings are those of the library before the checks were shared; the test passes against either
build (CHEBHIP_LIB_PATH selects another one)."""
import ctypes as C

import pytest

import __graft_entry__ as ge

sp = ge.load()
SIZE, TDIM, DIMS, ARG = 1, 2, 3, 4              # CHEBHIP_ERR_*

# entry: (takes nfields, takes basis)
ENTRIES = {
    "cheb_modal_create": (True, False), "cheb_modal_create_basis": (True, True),
    "cheb_reduce_create": (True, False),
    "cheb_stats_create": (True, False), "cheb_stats_check": (True, False),
    "cheb_points_create": (True, False), "cheb_points_create_basis": (True, True),
    "cheb_grad_create": (False, False), "cheb_grad_create_basis": (False, True),
    "cheb_dealias_create": (True, False), "cheb_dealias_create_basis": (True, True),
}
GOOD = dict(d=2, dims=(4, 5), nfields=2, basis=(0, 0), out=True, fine=None)

# fault: (what changes in GOOD, code, text)
FAULTS = {
    "out NULL": (dict(out=False), ARG, "out is NULL"),
    "dims NULL": (dict(dims=None), DIMS, "d = 2 must be in 1..10"),
    "d = 0": (dict(d=0), DIMS, "d = 0 must be in 1..10"),
    "d = 11": (dict(d=11, dims=(2,) * 11, basis=(0,) * 11), DIMS, "d = 11 must be in 1..10"),
    "nfields = 0": (dict(nfields=0), ARG, "nfields = 0 must be in 1..16"),
    "nfields = 17": (dict(nfields=17), ARG, "nfields = 17 must be in 1..16"),
    "extent 1": (dict(dims=(4, 1)), SIZE, "n = 1 but must be >= 2"),
    "extent 1025": (dict(dims=(4, 1025)), ARG, "n = 1025: at most 1024 points per direction"),
    "basis code 2": (dict(basis=(0, 2)), ARG, "basis[1] = 2 is neither 0 (CGL) nor 1 (Fourier)"),
    "periodic extent 257": (dict(dims=(4, 257), basis=(0, 1)), ARG, "dims[1] = 257: a periodic direction supports at most 256 points"),
    # (dealias is given its coarse extents as the fine ones too: its one bound is the fine grid's)
    "2^31 values": (dict(d=4, dims=(1024, 1024, 1024, 2), nfields=1, basis=(0,) * 4, fine=(1024, 1024, 1024, 2)), DIMS, "2^31 values or more"),
}
# a module's own answer to the same mistake
OWN = {
    ("cheb_stats_create", "dims NULL"): (ARG, None), ("cheb_stats_check", "dims NULL"): (ARG, None),
    ("cheb_stats_create", "d = 0"): (ARG, None), ("cheb_stats_check", "d = 0"): (ARG, None),
    ("cheb_stats_create", "d = 11"): (ARG, None), ("cheb_stats_check", "d = 11"): (ARG, None),
    ("cheb_dealias_create_basis", "basis code 2"): (ARG, "basis = 2 is neither 0 (CGL) nor 1 (Fourier)"),
    ("cheb_dealias_create_basis", "periodic extent 257"): (ARG, "n = 257: a periodic direction supports at most 256 points"),
    ("cheb_dealias_create", "2^31 values"): (DIMS, "2^31 values or more on the fine grid"),
    ("cheb_dealias_create_basis", "2^31 values"): (DIMS, "2^31 values or more on the fine grid"),
}


def applies(entry, fault):
    nfields, basis = ENTRIES[entry]
    if fault == "out NULL":
        return entry != "cheb_stats_check"
    if fault.startswith("nfields"):
        return nfields
    if fault in ("basis code 2", "periodic extent 257"):
        return basis
    return True


def call(L, entry, a):
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)
    h = C.c_void_p()
    out = C.byref(h) if a["out"] else None
    d, dims, nf, basis = a["d"], ints(a["dims"]), a["nfields"], ints(a["basis"])
    fn = getattr(L, entry)
    if entry == "cheb_stats_check":
        rc = fn(d, dims, nf, 64, 64)
    elif entry == "cheb_stats_create":
        rc = fn(d, dims, nf, 64, out)
    elif entry == "cheb_reduce_create":
        rc = fn(d, dims, nf, ints((1,) * max(d, 1)), out)
    elif entry == "cheb_grad_create":
        rc = fn(d, dims, None, out)
    elif entry == "cheb_grad_create_basis":
        rc = fn(d, dims, None, basis, out)
    elif entry == "cheb_dealias_create":
        rc = fn(d, dims, ints(a["fine"]), nf, out)
    elif entry == "cheb_dealias_create_basis":
        rc = fn(d, dims, ints(a["fine"]), basis, nf, out)
    elif entry.endswith("_basis"):
        rc = fn(d, dims, nf, basis, out)
    else:
        rc = fn(d, dims, nf, out)
    assert h.value is None, "%s left a handle behind" % entry
    return rc


CASES = [(e, f) for e in ENTRIES for f in FAULTS if applies(e, f)]


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def test_the_table_covers_every_entry():
    """Six faults for all eleven entries, `out` for the ten constructors, nfields for the nine that take it, basis for the four."""
    assert len(ENTRIES) == 11 and len(CASES) == 11 * 6 + 10 + 2 * 9 + 2 * 4


@pytest.mark.parametrize("entry,fault", CASES, ids=["%s-%s" % (e[5:], f.replace(" ", "_")) for e, f in CASES])
def test_one_bad_argument(entry, fault):
    L = sp.lib()
    change, code, text = FAULTS[fault]
    own = OWN.get((entry, fault))
    if own:
        code, text = own[0], own[1] or text
    rc = call(L, entry, dict(GOOD, **change))
    got = L.chebhip_last_error().decode()
    print("%s, %s: %d %r" % (entry, fault, rc, got))
    assert rc == code and got == text
