"""The SPPM photon gather on the device, point by point: rt_debug_sppm_gather_device -- the render's own build_grid, sort_into_grid,
gather_kernel and estimate_kernel -- on the families of tests/sppm_cases.py.  After every iteration the statistics and the estimates of
EVERY row equal the oracle's brute-force gather bit for bit (a NaN equal to any NaN: the both-empty case gives 0 / 0), and the grid of
both maps is a valid counting sort of the photons into the cells numpy puts them in.  tests/test_sppm_cases.py shows without a device that
the families reach the paths they aim at and that the oracle is right there."""
import numpy as np
import pytest

import sppm_cases as sp
from conftest import scene_path

pytestmark = pytest.mark.gpu


def check_grid(name, grid, ph):
    """cell_start is an exclusive scan that ends at n, index a permutation, and every photon sits in the cell floor((x - lo) / cell) gives"""
    n = len(ph)
    if n == 0:
        assert grid["dim"] == (1, 1, 1) and grid["cell"] == 1.0 and grid["cell_start"] is None
        return
    import rtamd
    lo, hi = sp.bbox(ph)
    cell, dim = rtamd.debug_grid_shape(lo, hi, n)
    assert np.array_equal(grid["lo"], lo) and grid["cell"] == cell and grid["dim"] == dim, name
    cs, ix = grid["cell_start"].astype(np.int64), grid["index"].astype(np.int64)
    cells = dim[0] * dim[1] * dim[2]
    assert len(cs) == cells + 1 and cs[0] == 0 and cs[-1] == n and (np.diff(cs) >= 0).all(), name
    assert np.array_equal(np.sort(ix), np.arange(n)), name
    inv_cell = 1.0 / cell
    c3 = np.clip(np.floor((ph[:, 0:3] - lo) * inv_cell), 0, np.array(dim) - 1).astype(np.int64)
    want = (c3[:, 2] * dim[1] + c3[:, 1]) * dim[0] + c3[:, 0]
    got = np.repeat(np.arange(cells), np.diff(cs))            # the cell of every slot of index
    assert np.array_equal(got, want[ix]), name
    assert np.array_equal(np.diff(cs), np.bincount(want, minlength=cells)), name       # every one of the cells, the empty ones included


def run_case(c, grids=True):
    import rtamd
    st = np.zeros((len(c["points"]), 10))
    rows = 0
    for it, ((glo, cau), (rst, rest, ruz)) in enumerate(zip(c["iterations"], sp.oracle_run(c))):
        dev = rtamd.debug_sppm_gather(glo, cau, c["points"], st, c["k_global"], c["k_caustic"], c["alpha"], c["S"], c["n_emitted"], grids=grids)
        name = "%s iteration %d" % (c["name"], it)
        assert dev["unit_zero"] == ruz, name
        if grids:
            check_grid(name + " global", dev["grid_global"], glo)
            check_grid(name + " caustic", dev["grid_caustic"], cau)
        if ruz:                                                   # family j: the oracle stops at the throw, only the status compares
            return rows
        st = dev["stats"]
        bad = ~(sp.same(st, rst).all(axis=1) & sp.same(dev["estimates"], rest).all(axis=1))
        print("%s: %d rows, %d differ" % (name, len(bad), bad.sum()))
        assert not bad.any(), "%s: %d of %d rows differ, first row %d: device %r %r, oracle %r %r" % (
            name, bad.sum(), len(bad), np.flatnonzero(bad)[0], st[bad][0], dev["estimates"][bad][0], rst[bad][0], rest[bad][0])
        rows += len(bad)
    return rows


@pytest.mark.parametrize("fam", list(sp.FAMILIES))
def test_gather_equals_the_oracle(fam):
    rows = sum(run_case(c) for c in sp.family(fam))
    assert rows == (0 if fam == "j_unit_zero" else sum(len(c["points"]) * len(c["iterations"]) for c in sp.family(fam)))     # no row left out


@pytest.mark.parametrize("fam", ["a_generic", "b_ties", "d_degenerate"])
def test_gather_with_the_selection_outside_lds_equals_the_oracle(fam, tuning):
    tuning(sppm_knn_candidates=0)
    rows = sum(run_case(c, grids=False) for c in sp.family(fam))
    assert rows == sum(len(c["points"]) * len(c["iterations"]) for c in sp.family(fam))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_photon_position_that_is_not_finite_is_refused(bad):
    """build_grid's refusal, decided on the host from the bounding box the device found, before any grid is built"""
    import rtamd
    (c,) = sp.family("j_unit_zero")
    glo, cau = (a.copy() for a in c["iterations"][0])
    glo[5, 1] = bad
    with pytest.raises(rtamd.RtError) as e:
        rtamd.debug_sppm_gather(glo, cau, c["points"], np.zeros((3, 10)), 10, 10, 0.7, 40, 100.0)
    assert e.value.code == -10                                    # RT_ERR_UNSUPPORTED
    cau[0, 2] = bad
    with pytest.raises(rtamd.RtError) as e:
        rtamd.debug_sppm_gather(c["iterations"][0][0], cau, c["points"], np.zeros((3, 10)), 10, 10, 0.7, 40, 100.0)
    assert e.value.code == -10


def test_render_statistics_equal_the_gather_on_the_oracles_photons():
    """what ties the diagnostic to the render: one iteration of rt_render_sppm's pre-pass on the small Cornell configuration of
    tests/test_sppm.py leaves the statistics the diagnostic computes from the oracle's photon maps and gather points of that iteration"""
    import oracle
    import rtamd
    from test_sppm import CFG
    cube = scene_path("cube.obj")
    w, cam = rtamd.select_scene(cube, 1.0, 1)
    o = oracle.cornell_box_scene(cube, 1.0, seed=1)
    cfg = dict(CFG, iterations=1)
    _, st, tot, _ = w.render_sppm(cam, width=24, height=24, spp=0, seed=1, **cfg)
    glo, cau, gp, S = o.sppm_iteration(24, 24, 0, cfg["photons_per_iter"], cfg["k_global"], cfg["k_caustic"], seed=1)
    assert tot == (len(glo), len(cau)) and len(cau) > 0 and 100 < (gp[:, 0] != 0).sum() < len(gp)
    dev = rtamd.debug_sppm_gather(glo, cau, gp, np.zeros((len(gp), 10)), cfg["k_global"], cfg["k_caustic"], 0.7, S,
                                  float(cfg["photons_per_iter"]))
    assert not dev["unit_zero"]
    assert sp.same(dev["stats"], st.reshape(-1, 10)).all()
    assert (dev["stats"][:, 4] > 0).sum() == (gp[:, 0] != 0).sum()
    check_grid("cornell global", dev["grid_global"], glo)
    check_grid("cornell caustic", dev["grid_caustic"], cau)
