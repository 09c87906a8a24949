"""The families of tests/sppm_cases.py without a device: the oracle's brute-force gather (oracle.sppm_gather: sppm_update twice per point and
adjust_flux's division) against an independent reference written here -- numpy for d^2 in the oracle's operation order, a partition for
the k-th distance, Python integers for the fixed-point sums, plain Python numbers for the update -- bit for bit on every row; the
construction of the families (each reaches what it is named for, so tests/test_sppm_gather_gpu.py cannot pass vacuously); the grid's
shape through the host-only rt_debug_grid_shape; and the argument checks of rt_debug_sppm_gather_device, which are decided on the host."""
import ctypes as C
import math

import numpy as np
import pytest

import sppm_cases as sp

PI = 3.14159265358979323846264338327950288


# ---- the independent reference -------------------------------------------------------------------------------------------------------------
def _d2(ph, p):
    d = ph[:, 0:3] - p                                            # position - p, then x x + y y + z z from the left
    return d, d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def _fixed_flux(ph, d, d2, sel, bsdf, S):
    """sum over the selected photons of round_half_even(bsdf * power * (1 - |norm . unit(position - p)|) * 2^S), in Python integers"""
    tot = [0, 0, 0]
    for i in np.flatnonzero(sel):
        l = math.sqrt(float(d2[i]))
        u = [float(d[i, a]) / l for a in range(3)]
        nx, ny, nz = (float(v) for v in ph[i, 6:9])
        df = abs(nx * u[0] + ny * u[1] + nz * u[2])
        for a in range(3):
            t = (float(bsdf[a]) * float(ph[i, 3 + a])) * (1.0 - df)
            tot[a] += round(math.ldexp(t, S))                     # round(): an exact integer, ties to even
    return [math.ldexp(float(v), -S) for v in tot]


def _update(st, ph, p, bsdf, k, alpha, S):
    """SPPM::update on st = [flux[3], radius2, photons] (a list of Python numbers)"""
    d, d2 = _d2(ph, p)
    if st[4] == 0:
        st[4] = k
        st[3] = 0.0
        sel = np.zeros(len(ph), dtype=bool)
        if len(ph):
            r2k = np.partition(d2, min(k, len(ph)) - 1)[min(k, len(ph)) - 1]
            sel = d2 <= r2k
            st[3] = float(d2[sel].max())
        st[0:3] = _fixed_flux(ph, d, d2, sel, bsdf, S)
    else:
        radius = math.sqrt(st[3])
        sel = d2 < radius * radius
        found = int(sel.sum())
        flux = _fixed_flux(ph, d, d2, sel, bsdf, S)
        prev = st[4]
        st[4] = prev + int(alpha * float(found))
        frac = float(st[4]) / float(prev + found)
        st[3] = st[3] * frac
        st[0:3] = [(st[a] + flux[a]) * frac for a in range(3)]


def reference_run(c):
    m = len(c["points"])
    state = [[[0.0, 0.0, 0.0, 0.0, 0] for _ in range(2)] for _ in range(m)]      # per point: global, caustic
    out = []
    for glo, cau in c["iterations"]:
        stats, est = np.zeros((m, 10)), np.zeros((m, 6))
        for i, row in enumerate(c["points"]):
            if row[0] != 0.0:
                _update(state[i][1], cau, row[1:4], row[4:7], c["k_caustic"], c["alpha"], c["S"])
                _update(state[i][0], glo, row[1:4], row[4:7], c["k_global"], c["alpha"], c["S"])
            for j in range(2):
                stats[i, 5 * j:5 * j + 5] = state[i][j]
            with np.errstate(invalid="ignore", divide="ignore"):
                for j, col in ((1, 0), (0, 3)):
                    est[i, col:col + 3] = np.float64(state[i][j][0:3]) / np.float64(PI * state[i][j][3] * c["n_emitted"])
        out.append((stats, est))
    return out


@pytest.mark.parametrize("fam", [f for f in sp.FAMILIES if f != "j_unit_zero"])
def test_oracle_gather_equals_the_independent_reference(fam):
    rows = 0
    for c in sp.family(fam):
        ref = reference_run(c)
        for it, ((st, est, uz), (rst, rest)) in enumerate(zip(sp.oracle_run(c), ref)):
            assert not uz, (c["name"], it)
            bad = ~(sp.same(st, rst).all(axis=1) & sp.same(est, rest).all(axis=1))
            assert not bad.any(), "%s iteration %d: %d of %d rows differ, first row %d: oracle %r %r, reference %r %r" % (
                c["name"], it, bad.sum(), len(bad), np.flatnonzero(bad)[0], st[bad][0], est[bad][0], rst[bad][0], rest[bad][0])
            rows += len(st)
        valid = c["points"][:, 0] != 0.0
        assert (sp.oracle_run(c)[-1][0][valid, 4] >= c["k_global"]).all() and (sp.oracle_run(c)[-1][0][~valid] == 0.0).all()
    assert rows > 0


def test_unit_zero_family_reports_it():
    (c,) = sp.family("j_unit_zero")
    (st, est, uz), = sp.oracle_run(c)
    assert uz
    g = c["iterations"][0][0]
    assert (g[:, 0:3] == c["points"][1, 1:4]).all(axis=1).sum() == 1


# ---- the families reach what they are named for --------------------------------------------------------------------------------------------
def test_generic_family_covers_the_block_boundary_and_every_k():
    cases = sp.family("a_generic")
    assert sorted(len(c["points"]) for c in cases) == [1, 4, 5, 67]
    n_g, n_c = 400, 60
    ks = {c["k_global"] for c in cases} | {c["k_caustic"] for c in cases}
    assert {1, 5, 50, n_g, n_g + 1, n_c + 1} <= ks
    assert all(len(c["iterations"]) == 3 and len(c["iterations"][0][0]) == n_g and len(c["iterations"][0][1]) == n_c for c in cases)
    assert any((c["points"][:, 0] == 0.0).any() for c in cases)


def test_tie_family_has_shells_that_k_splits_and_ends():
    split = at_end = 0
    for c in sp.family("b_ties"):
        tied = 0
        for which, k in ((0, c["k_global"]), (1, c["k_caustic"])):
            for row in c["points"]:
                below, shell = sp.shell_of_kth(c["iterations"][0][which][:, 0:3], row[1:4], k)
                assert below < k <= below + shell
                if shell > 1:
                    tied += 1
                    split += k < below + shell          # the k-th nearest lies inside the shell: the device's bisection never sees cnt == k
                    at_end += k == below + shell
        assert tied > 0, c["name"]
    assert split > 20 and at_end > 20
    for c in sp.family("b_ties"):                       # no point on a photon
        for g, cau in c["iterations"]:
            for ph in (g, cau):
                assert all(((ph[:, 0:3] - row[1:4]) ** 2).sum(axis=1).min() > 0 for row in c["points"])


def test_few_family_sizes():
    names = {c["name"]: c for c in sp.family("c_few")}
    for which, col in (("global", 0), ("caustic", 1)):
        for n in (0, 1, 2, sp.FEW_K - 1, sp.FEW_K):
            c = names["few_%s_n%d" % (which, n)]
            assert [len(it[col]) for it in c["iterations"]] == [n, n] and all(len(it[1 - col]) == 200 for it in c["iterations"])
    assert [tuple(len(a) for a in it) for it in names["few_both_empty_then_full"]["iterations"]] == [(0, 0), (200, 50)]
    assert [tuple(len(a) for a in it) for it in names["few_full_then_empty"]["iterations"]] == [(200, 50), (0, 0), (0, 1)]
    # both maps empty: radius2 stays 0 and the estimate is 0 / 0
    st, est, _ = sp.oracle_run(names["few_both_empty_then_full"])[0]
    valid = names["few_both_empty_then_full"]["points"][:, 0] != 0
    assert (st[valid][:, [3, 8]] == 0).all() and (st[valid][:, [4, 9]] == sp.FEW_K).all() and np.isnan(est).all()
    st, _, _ = sp.oracle_run(names["few_full_then_empty"])[2]
    assert (st[valid][:, 3] > 0).all()


def _candidates(ph, p, k, cell, dim, lo):
    """the photons within the radius at which the device's search stops growing (r = cell, doubled up to r_all, until k are inside)"""
    import numpy as np
    _, d2 = _d2(ph, p)
    kk = min(k, len(ph))
    span = float(max(dim)) * cell
    dist_out = 0.0
    for a in range(3):
        dist_out = max(dist_out, lo[a] - p[a], p[a] - (lo[a] + dim[a] * cell))
    r_all = 2.0 * (span + dist_out) + cell
    r = cell
    while True:
        n_in = int((d2 <= r * r).sum())
        if n_in >= kk or r >= r_all:
            return n_in
        r = min(2.0 * r, r_all)


def test_degenerate_family_shapes_and_more_than_1024_candidates():
    import rtamd
    big = 0
    for c in sp.family("d_degenerate"):
        for g, cau in c["iterations"]:
            for ph, k in ((g, c["k_global"]), (cau, c["k_caustic"])):
                lo, hi = sp.bbox(ph)
                ext = hi - lo
                cell, dim = rtamd.debug_grid_shape(lo, hi, len(ph))
                if c["shape"] == "point":
                    assert (ext == 0).all() and cell == 1.0 and dim == (1, 1, 1)
                elif c["shape"] == "line":
                    assert (ext == 0).sum() == 2 and cell == ext.max() and sorted(dim) == [1, 1, 2]      # no area: cell = the longest extent
                elif c["shape"] == "plane":
                    assert (ext == 0).sum() == 1 and cell == max(2.0 * math.sqrt(2.0 * ext[0] * ext[1] / len(ph)), ext.max() / 160.0) and dim[2] == 1
                if c.get("big_search") and k > 1024:
                    for row in c["points"]:
                        n_in = _candidates(ph, row[1:4], k, cell, dim, lo)
                        assert n_in > 1024, (c["name"], n_in)          # more than KNN_CAND: the selection re-reads the grid
                        big += 1
    assert big >= 10
    two = [c for c in sp.family("d_degenerate") if c["name"] == "degenerate_two_clusters"][0]
    g = two["iterations"][0][0]
    lo, hi = sp.bbox(g)
    cell, dim = rtamd.debug_grid_shape(lo, hi, len(g))
    assert cell == (hi - lo).max() / 160.0 and dim == (161, 1, 1)                                            # the 160-cells-per-axis floor
    for half in (g[:len(g) // 2], g[len(g) // 2:]):
        assert len(half) >= 3000 and (half[:, 0:3].max(axis=0) - half[:, 0:3].min(axis=0)).max() < cell      # a cluster is narrower than a cell
    assert abs(g[-1, 0] - g[0, 0]) > 0.99e6 and two["k_global"] == 2000


def test_outside_family_points():
    for c in sp.family("e_outside"):
        g = c["iterations"][0][0]
        lo, hi = sp.bbox(g)
        assert (lo == 0).all() and (hi == 1).all()
        p = c["points"][:, 1:4]
        far = np.maximum(lo - p, p - hi).max(axis=1)
        for s in (1.0, 10.0, 1e4):
            assert (far == s).sum() >= 6
        on = ((p == 0) | (p == 1)).any(axis=1) & (far <= 0)
        assert on.sum() >= 6
        cell, _ = __import__("rtamd").debug_grid_shape(lo, hi, len(g))
        inside = (far < 0) & (np.minimum(p - lo, hi - p).min(axis=1) < cell)
        assert inside.sum() >= 3                                        # the first search cube [p - cell, p + cell] leaves the grid


def test_scale_family_rounds_d2_coarsely():
    tr = [c for c in sp.family("f_scale") if c["name"] == "scale_translated_1e6"][0]
    g = tr["iterations"][0][0]
    assert (np.abs(g[:, 0:3]) >= 1e6).all()
    _, d2 = _d2(g, tr["points"][0, 1:4])
    assert len(np.unique(d2)) <= len(d2) and (d2 * 2.0 ** 66 % 1.0 == 0).all()     # coordinates are multiples of 2^-33 there


def test_radius_family_squares():
    sq, non = sp.family("g_radius")
    assert sq["r2"] == 0.25 and math.sqrt(0.25) * math.sqrt(0.25) == 0.25
    assert non["r2"] == 0.5 and math.sqrt(0.5) * math.sqrt(0.5) > 0.5
    for c in (sq, non):
        runs = sp.oracle_run(c)
        assert runs[0][0][0, 3] == c["r2"] and runs[0][0][0, 8] == c["r2"]             # iteration 0 leaves radius2 = r2 in both maps
        _, d2 = _d2(c["iterations"][1][0], c["points"][0, 1:4])
        assert (d2 == c["r2"]).sum() == c["n_at"] == 4
        inside = int((d2 < c["r2"]).sum())
        found = inside + (c["n_at"] if c is non else 0)                               # at exactly the radius: out for 0.25, in for 0.5
        assert runs[1][0][0, 4] == 2 + int(0.7 * found)


def test_update_family_products():
    assert any(sp.crosses_an_integer(a, f) for a in sp.ALPHAS for f in sp.FOUND)
    assert sp.crosses_an_integer(2.0 / 3.0, 3) and int(2.0 / 3.0 * 3.0) == 2          # the double below 2/3, times 3, rounds up to 2.0
    assert sp.crosses_an_integer(0.7, 10) and int(0.7 * 10.0) == 7                       # the double below 0.7, times 10, rounds up to 7.0
    assert int(0.7 * 3.0) == 2 and int(0.7 * 30.0) == 21 and int(0.7 * 43.0) == 30 and int(0.1 * 30.0) == 3
    for c in sp.family("h_update"):
        runs = sp.oracle_run(c)
        assert (runs[0][0][:, [3, 8]] == 0.25).all()
        for which, counts in ((0, sp.FOUND), (1, sp.FOUND[::-1])):
            for i, n in enumerate(counts):
                _, d2 = _d2(c["iterations"][1][which], c["points"][i, 1:4])
                assert (d2 < 0.25).sum() == n
                assert runs[1][0][i, 5 * which + 4] == 2 + int(c["alpha"] * float(n))
                _, d2 = _d2(c["iterations"][2][which], c["points"][i, 1:4])
                assert (d2 < runs[1][0][i, 5 * which + 3]).sum() == 0                   # found == 0 in iteration 2
        assert np.array_equal(runs[2][0][:, [3, 4, 8, 9]], runs[1][0][:, [3, 4, 8, 9]])


def test_fixed_family_terms_lie_half_way():
    assert sorted(c["S"] for c in sp.family("i_fixed")) == [0, 17, 40, 60]
    for c in sp.family("i_fixed"):
        for g, cau in c["iterations"]:
            for ph in (g, cau):
                t = ph[:, 3:6] * 2.0 ** c["S"]
                assert (np.abs(t) % 1.0 == 0.5).all() and (np.abs(t) < 2.0 ** 52).all() and (t < 0).any() and (t > 0).any()
                assert (np.floor(np.abs(t)) % 2 == 0).any() and (np.floor(np.abs(t)) % 2 == 1).any()
                assert (ph[:, 2] == 0).all() and (ph[:, 6:9] == sp.UP).all()
        assert (c["points"][:, 3] == 0).all() and (c["points"][:, 4:7] == 1).all()


def test_large_family_has_more_than_2_to_the_21_cells():
    import rtamd
    (c,) = sp.family("k_large")
    assert len(c["points"]) == 64 and c["k_global"] == 100 and len(c["iterations"]) == 2
    for g, _ in c["iterations"]:
        lo, hi = sp.bbox(g)
        cell, dim = rtamd.debug_grid_shape(lo, hi, len(g))
        assert 2.0 * math.sqrt(6.0 / len(g)) < cell == 1.0 / 160.0 and dim == (161, 161, 161)      # the headline workload's shape: the floor
        assert dim[0] * dim[1] * dim[2] > 2 ** 21                 # more than 2048 scan blocks: scan_sums_kernel's carry loop runs


# ---- the grid's shape ------------------------------------------------------------------------------------------------------------------------
def test_grid_shape_of_every_family():
    import rtamd
    n_maps = 0
    for fam in sp.FAMILIES:
        for c in sp.family(fam):
            for it in c["iterations"]:
                for ph in it:
                    if len(ph) == 0:
                        continue
                    lo, hi = sp.bbox(ph)
                    ext = hi - lo
                    cell, dim = rtamd.debug_grid_shape(lo, hi, len(ph))
                    assert cell > 0 and math.isfinite(cell), c["name"]
                    assert all(1 <= d <= 161 for d in dim), (c["name"], dim)
                    assert all(math.floor(ext[a] / cell) < dim[a] for a in range(3)), (c["name"], ext, cell, dim)
                    n_maps += 1
    assert n_maps > 100


def test_grid_shape_fallbacks_and_refusals():
    import rtamd
    assert rtamd.debug_grid_shape((1, 2, 3), (1, 2, 3), 50) == (1.0, (1, 1, 1))                  # a point: cell = 1
    assert rtamd.debug_grid_shape((0, 0, 0), (0, 0, 0), 0) == (1.0, (1, 1, 1))                  # no photons: no grid
    assert rtamd.debug_grid_shape((9, 9, 9), (0, 0, 0), 0) == (1.0, (1, 1, 1))                  # (the box is not read then)
    assert rtamd.debug_grid_shape((0, 5, 5), (4, 5, 5), 1000) == (4.0, (2, 1, 1))               # a line: cell = its length
    assert rtamd.debug_grid_shape((0, 0, 0), (1, 1, 1), 6) == (2.0, (1, 1, 1))                  # 2 sqrt(6 / 6)
    cell, dim = rtamd.debug_grid_shape((0, 0, 0), (1, 1, 1), 10 ** 9)                            # the floor: longest / 160
    assert cell == 1.0 / 160.0 and dim == (161, 161, 161)
    cell, dim = rtamd.debug_grid_shape((0, 0, 0), (1e6, 0.5, 0.5), 6000)
    assert cell == 1e6 / 160.0 and dim == (161, 1, 1)
    for lo, hi in (((0, 0, 0), (1, -1, 1)), ((0, 0, 0), (math.inf, 1, 1)), ((math.nan, 0, 0), (1, 1, 1)), ((-1e308, 0, 0), (1e308, 1, 1))):
        with pytest.raises(rtamd.RtError) as e:
            rtamd.debug_grid_shape(lo, hi, 10)
        assert e.value.code == -10                                # RT_ERR_UNSUPPORTED
    L = rtamd.lib()
    assert L.rt_debug_grid_shape(None, None, 1, None, None) == -1


# ---- refusals of the device entry: decided on the host, before a device is asked for ---------------------------------------------------------
def test_gather_entry_checks_its_arguments_before_it_asks_for_a_device():
    import rtamd
    L = rtamd.lib()
    dp = C.POINTER(C.c_double)
    g, pts, st, est = np.zeros((4, 9)), np.zeros((2, 7)), np.zeros((2, 10)), np.zeros((2, 6))

    def io(**kw):
        a = rtamd.rt_debug_sppm_gather()
        a.n_global, a.n_caustic, a.m = 4, 0, 2
        a.global_, a.caustic = g.ctypes.data_as(dp), None
        a.points, a.stats, a.estimates = pts.ctypes.data_as(dp), st.ctypes.data_as(dp), est.ctypes.data_as(dp)
        a.k_global, a.k_caustic, a.alpha, a.shift, a.n_emitted = 3, 3, 0.7, 40, 100.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(a, device=0):
        return L.rt_debug_sppm_gather_device(device, C.byref(a) if a is not None else None)
    assert call(None) == -1
    for bad in (dict(points=None), dict(stats=None), dict(estimates=None), dict(global_=None), dict(n_caustic=1), dict(m=0), dict(m=2 ** 31),
                dict(k_global=0), dict(k_caustic=-1), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=math.nan), dict(shift=-1), dict(shift=61),
                dict(n_global=2 ** 30 + 1)):
        assert call(io(**bad)) == -1, bad                          # RT_ERR_ARG, with and without a device
    if rtamd.device_count() > 0:
        return                                                     # a HIP device is visible: tests/test_sppm_gather_gpu.py runs the entry
    assert call(io()) == -9                                        # RT_ERR_NO_DEVICE
    with pytest.raises(rtamd.RtError) as e:
        rtamd.debug_sppm_gather(g, np.zeros((0, 9)), pts, st, 3, 3, 0.7, 40, 100.0)
    assert e.value.code == -9
