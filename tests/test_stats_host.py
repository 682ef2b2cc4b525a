"""The host side of cheb_stats_* and the twin the device tests compare against (stats_ref.py): the node spacings and rates
against the long-double formula, the twin's slots against a value-by-value loop, its sums against a brute-force loop, plain
double restatements inside the derived bars, planted faults outside them, and the argument errors.  No device needed."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import stats_ref as ref

sp = ge.load()
LD = np.longdouble
U = 2.0 ** -53
SEED = 20241101
SHAPES = [(2,), (7, 3), (33, 34, 35), (96, 97, 95)]
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module", autouse=True)
def built():
    ge.build()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- spacings -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 17, 256, 1024])
def test_spacing_against_long_double(n):
    """|h - ref| <= U ref + 8 2^-64 ref with ref the product formula in numpy long double: one rounding to double and a few
    long-double roundings on either side.  Against the difference of the cosines themselves, which cancels next to the walls:
    an absolute 4 2^-64 more.  h is symmetric, positive, smallest at the walls, and its ends are 1 - cos(pi / N)
    (which cancels too)."""
    h = sp.stats_spacing(n)
    r = ref.spacing_ld(n)
    assert h.shape == (n,) and (h > 0).all()
    err = np.abs(h.astype(LD) - r).astype(np.float64)
    assert (err <= U * r.astype(np.float64) * (1 + 2.0 ** -8)).all()
    N = n - 1
    pi = LD(4) * np.arctan(LD(1))
    x = np.cos(pi * np.arange(n).astype(LD) / LD(N))
    gap = x[:-1] - x[1:]
    hd = np.empty(n, dtype=LD)
    hd[0], hd[N] = gap[0], gap[N - 1]
    hd[1:N] = np.minimum(gap[:-1], gap[1:])
    assert (np.abs(h.astype(LD) - hd).astype(np.float64) <= U * h + 4 * 2.0 ** -64).all()
    assert (bits(h) == bits(h[::-1])).all()
    assert h[0] == h.min() and abs(float(LD(h[0]) - (1 - np.cos(pi / LD(N))))) <= U * h[0] + 4 * 2.0 ** -64
    # the rates: the quotient in long double, rounded once
    for s in (1.0, 2.0 / 3.0, 0.0):
        rr = sp.stats_rate(n, s)
        q = LD(s) / r
        assert (np.abs(rr.astype(LD) - q).astype(np.float64) <= U * np.abs(q).astype(np.float64) * (1 + 2.0 ** -8)).all()


# ---- the twin against loops -----------------------------------------------------------------------------------------------------
def test_slots_against_a_loop():
    rng = np.random.default_rng(SEED)
    u = np.concatenate([rng.standard_normal(500), [-1.0, 1.0, 0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324],
                        -1.0 + np.arange(65) / 32.0])
    for nbins in (1, 2, 63, 64, 65, 256, 1024):
        for lo, hi in ((-1.0, 1.0), (-2.5, 3.0), (0.0, 0.0), (1.0, -1.0), (-np.inf, 1.0), (-1e308, 1e308)):
            assert (ref.slots_uniform(u, lo, hi, nbins) == ref.slots_brute(u, nbins, lo=lo, hi=hi)).all(), (nbins, lo, hi)
        e = np.sort(rng.standard_normal(nbins + 1))
        if nbins >= 2:
            e[nbins // 2] = e[nbins // 2 - 1]                       # an empty bin
        uu = np.concatenate([u, e])
        assert (ref.slots_edges(uu, e, nbins) == ref.slots_brute(uu, nbins, e=e.tolist())).all(), nbins
        assert (bits(sp.stats_edges(e, 2, nbins)) == bits(np.stack([e, e]))).all()      # what the wrapper uploads for these edges
    # dyadic edges: every value k / 32 - 1 sits in bin k exactly, 1.0 in overflow
    s = ref.slots_uniform(-1.0 + np.arange(65) / 32.0, -1.0, 1.0, 64)
    assert (s == 1 + np.arange(65)).all() and s[64] == 64 + 1


def test_twin_against_brute_force():
    """summary_truth, histogram_truth and cfl_sums on (7, 3) x 3 fields against loops over the nodes in long double."""
    dims, nf = (7, 3), 3
    rng = np.random.default_rng(SEED + 1)
    T = 21
    u = rng.standard_normal(nf * T)
    u[T + 4] = np.nan
    u[5] = u[2] = np.nanmin(u) - 1.0                                     # a tie: the first index counts
    ws = ref.default_weights(dims)
    c = np.array([0.25, 0.0, -1.0])
    tr = ref.summary_truth(dims, nf, ws, u, c)
    nb = 5
    spec = np.tile([-1.0, 1.5], (nf, 1))
    slots = ref.field_slots(nf, u, nb, spec, False)
    ht = ref.histogram_truth(dims, nf, ws, slots, nb)
    for f in range(nf):
        M, mass, cnt = [LD(0)] * 4, [LD(0)] * (nb + 3), [0] * (nb + 3)
        mn = mx = None
        for i0 in range(7):
            for i1 in range(3):
                i = i0 * 3 + i1
                W = LD(ws[0][i0]) * LD(ws[1][i1])
                x = u[f * T + i]
                for p in range(4):
                    M[p] = M[p] + W * (LD(x) - LD(c[f])) ** (p + 1)
                mass[slots[f, i]] += W
                cnt[slots[f, i]] += 1
                if x == x:
                    if mn is None or x < mn[0]:
                        mn = (x, i)
                    if mx is None or x > mx[0]:
                        mx = (x, i)
        assert (tr["mn"][f], tr["imn"][f], tr["mx"][f], tr["imx"][f]) == (mn[0], mn[1], mx[0], mx[1])
        assert tr["nan"][f] == (1 if f == 1 else 0)
        for p in range(4):
            if f == 1:
                assert np.isnan(tr["M"][f, p])
            else:
                assert abs(tr["M"][f, p] - M[p]) <= 64 * 2.0 ** -64 * tr["B"][f, p]
        assert (ht["count"][f] == cnt).all()
        assert (np.abs(ht["mass"][f] - np.array(mass, dtype=LD)).astype(np.float64) <= 64 * 2.0 ** -64 * ht["B"][f]).all()
    assert tr["imn"][0] == 2
    vel = rng.standard_normal(2 * T)
    rs = ref.rates(dims, (2.0, 0.5))
    S = ref.cfl_sums(dims, rs, vel)
    for i0 in range(7):
        for i1 in range(3):
            want = abs(LD(vel[i0 * 3 + i1])) * LD(rs[0][i0]) + abs(LD(vel[T + i0 * 3 + i1])) * LD(rs[1][i1])
            assert abs(S[i0, i1] - want) <= 4 * 2.0 ** -64 * want
    assert (bits(rs[0]) == bits(sp.stats_rate(7, 2.0))).all()


# ---- restatements inside the bars, planted faults outside -----------------------------------------------------------------------
def case(dims, nf=2):
    rng = np.random.default_rng(SEED + sum(dims))
    T = int(np.prod(dims))
    u = rng.standard_normal(nf * T)
    u[T - 1] = 1.0                      # the last element of field 0 sits on hi: overflow, and what "drop_last" loses
    u[nf * T - 1] = -0.5
    return u, rng.standard_normal(nf * T)


@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_restatements_inside_the_bars(dims):
    nf = 2
    u, c = case(dims, nf)
    ws = ref.default_weights(dims)
    st = ref.summary_truth(dims, nf, ws, u)
    r = ref.summary_ratio(dims, nf, ref.restate_summary(dims, nf, ws, u), st)
    print("stats-host %s summary: %.3g of the bar" % (ids(dims), r))
    assert r <= 1.0
    spec = np.tile([-1.0, 1.0], (nf, 1))
    slots = ref.field_slots(nf, u, 64, spec, False)
    for cond in (None, c):
        ht = ref.histogram_truth(dims, nf, ws, slots, 64, cond)
        r = ref.histogram_ratio(dims, nf, 64, ref.restate_histogram(dims, nf, ws, u, 64, spec, cond=cond), ht)
        print("stats-host %s histogram%s: %.3g of the bar" % (ids(dims), "" if cond is None else " cond", r))
        assert r <= 1.0
    d = len(dims)
    vel = np.random.default_rng(SEED).standard_normal(d * int(np.prod(dims)))
    rs = ref.rates(dims)
    assert ref.cfl_ratio(dims, rs, vel, ref.cfl_restate(dims, rs, vel)) <= 1.0


@pytest.mark.parametrize("dims", [(7, 3), (33, 34, 35)], ids=ids)
def test_planted_faults_fail(dims):
    """`t > nbins` with a closed last bin, the last element dropped, the weights of two directions swapped: each leaves the bars
    (or the exact entries), in the summary and in the histogram; a dropped last node that carries the maximum, in cfl."""
    nf = 2
    u, c = case(dims, nf)
    T = int(np.prod(dims))
    ws = ref.default_weights(dims)
    st = ref.summary_truth(dims, nf, ws, u)
    spec = np.tile([-1.0, 1.0], (nf, 1))
    ht = ref.histogram_truth(dims, nf, ws, ref.field_slots(nf, u, 64, spec, False), 64)
    for fault in ("drop_last", "swap_weights"):
        assert ref.summary_ratio(dims, nf, ref.restate_summary(dims, nf, ws, u, fault=fault), st) > 1.0, fault
    for fault in ("gt", "drop_last", "swap_weights"):
        assert ref.histogram_ratio(dims, nf, 64, ref.restate_histogram(dims, nf, ws, u, 64, spec, fault=fault), ht) > 1.0, fault
    d = len(dims)
    vel = np.random.default_rng(SEED).standard_normal(d * T)
    vel[T - 1] = 1e3
    rs = ref.rates(dims)
    assert ref.cfl_ratio(dims, rs, vel, ref.cfl_restate(dims, rs, vel, fault="drop_last")) > 1.0


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    """Each CHEBHIP_ERR_ARG (4), checked before any device is touched."""
    L = sp.lib()
    ints = lambda v: (C.c_int * len(v))(*v)
    h = C.c_void_p()
    one = C.c_void_p(8)                                                          # never dereferenced: the checks come first
    # a NULL handle
    assert L.cheb_stats_summary(None, one, None, one, None) == 4
    assert L.cheb_stats_histogram(None, one, None, 0, 4, one, one, None) == 4
    assert L.cheb_stats_cfl(None, one, None, one, None) == 4
    assert L.cheb_stats_set_weights(None, 0, None) == 4 and L.cheb_stats_destroy(None) == 4
    assert L.cheb_stats_size(None, 0) == -1
    # nbins of 0, nbins above max_bins, max_bins above 1024, d of 0: the checks of create and histogram, without a handle
    assert L.cheb_stats_check(2, ints([4, 4]), 1, 64, 64) == 0
    assert L.cheb_stats_check(2, ints([4, 4]), 1, 64, 0) == 4 and b"nbins" in L.chebhip_last_error()
    assert L.cheb_stats_check(2, ints([4, 4]), 1, 64, 65) == 4 and b"nbins" in L.chebhip_last_error()
    assert L.cheb_stats_check(2, ints([4, 4]), 1, 1025, 4) == 4 and b"max_bins" in L.chebhip_last_error()
    assert L.cheb_stats_check(2, ints([4, 4]), 1, 0, 1) == 4
    assert L.cheb_stats_check(0, ints([4]), 1, 64, 4) == 4 and b"d = 0" in L.chebhip_last_error()
    assert L.cheb_stats_check(11, ints([2] * 11), 1, 64, 4) == 4
    assert L.cheb_stats_check(2, None, 1, 64, 4) == 4
    assert L.cheb_stats_check(2, ints([4, 4]), 17, 64, 4) == 4 and L.cheb_stats_check(2, ints([4, 4]), 0, 64, 4) == 4
    assert L.cheb_stats_check(2, ints([4, 1]), 1, 64, 4) == 1                    # CHEBHIP_ERR_SIZE, as everywhere
    assert L.cheb_stats_check(4, ints([1024, 1024, 1024, 2]), 1, 64, 4) == 3    # 2^31 values: CHEBHIP_ERR_DIMS
    assert L.cheb_stats_create(2, ints([4, 4]), 1, 1025, C.byref(h)) == 4 and h.value is None
    assert L.cheb_stats_create(0, ints([4]), 1, 64, C.byref(h)) == 4 and h.value is None
    assert L.cheb_stats_create(2, ints([4, 4]), 1, 64, None) == 4
    w = (C.c_double * 8)()
    assert L.cheb_stats_spacing_host(1, w) == 1 and L.cheb_stats_spacing_host(1025, w) == 4
    assert L.cheb_stats_spacing_host(8, None) == 4 and L.cheb_stats_rate_host(8, float("nan"), w) == 4
    assert L.cheb_stats_spacing_host(8, w) == 0 and L.cheb_stats_rate_host(8, 2.0, w) == 0
    # a non-monotone host edge array passed to the Python wrapper
    for bad in ([0.0, 1.0, 0.5, 2.0], [0.0, np.nan, 1.0, 2.0]):
        with pytest.raises(sp.ChebhipError) as e:
            sp.stats_edges(bad, 2, 3)
        assert e.value.code == 4
    with pytest.raises(sp.ChebhipError) as e:
        sp.stats_edges([0.0, 1.0, 2.0], 2, 3)                                    # bins + 1 values
    assert e.value.code == 4
    assert sp.stats_edges([0.0, 1.0, 1.0, 2.0], 2, 3).shape == (2, 4)


def test_create_needs_a_device():
    import torch
    if torch.cuda.is_available():
        sp.ChebStats((4, 4)).destroy()
        return
    with pytest.raises(sp.ChebhipError) as e:
        sp.ChebStats((4, 4))
    assert e.value.code == 5
