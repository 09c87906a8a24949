"""The SPPM photon pass and eye pass on the device, photon by photon and pixel by pixel: rt_debug_sppm_trace_device -- render_sppm's own
light table, variant choice, launches and grow-and-retry -- on the families of tests/sppm_trace_cases.py.  Both photon maps equal the
oracle's sppm_iteration as multisets of bit patterns (the device stores photons in the order its waves finish), the counts and S are
equal, the gather points are equal in all seven columns for EVERY pixel, and the launch count and the variant word are the case's.
tests/test_sppm_trace_cases.py shows without a device that the families reach what they aim at."""
import numpy as np
import pytest

import sppm_cases as sp
import sppm_trace_cases as tc
from conftest import scene_path

pytestmark = pytest.mark.gpu


def run_case(c, set_tuning):
    """-> (photon rows compared, gather-point rows compared)"""
    w, cam, _ = tc.scene(c["scene"])
    g, cau, gp, S = tc.oracle_run(c)
    set_tuning(**c["tuning"])
    cap = c["capacity"](len(g), len(cau)) if c["capacity"] else (0, 0)
    dev = w.debug_sppm_trace(cam, c["width"], c["height"], iteration=c["iteration"], photons_per_iter=c["P"], max_bounces=c["max_bounces"],
                             seed=c["seed"], capacity=cap, photons=c["photons"])
    set_tuning()
    name = c["name"]
    print("%s: %d + %d photons, %d pixels (%d valid), S %d, launches %d, variant %d" % (
        name, dev["n_global"], dev["n_caustic"], len(gp), int((dev["points"][:, 0] != 0).sum()), dev["S"], dev["photon_launches"], dev["variant"]))
    assert not dev["unit_zero"], name
    assert dev["S"] == S and dev["variant"] == c["variant"] and dev["photon_launches"] == c["launches"], (name, dev["S"], dev["variant"], dev["photon_launches"])
    rows = 0
    if c["photons"]:
        assert (dev["n_global"], dev["n_caustic"]) == (len(g), len(cau)), name
        for what, got, exp in (("global", dev["global"], g), ("caustic", dev["caustic"], cau)):
            a, b = tc.sorted_rows(got), tc.sorted_rows(exp)
            assert a.shape == b.shape, (name, what)
            bad = (a != b).any(axis=1)
            assert np.array_equal(a, b), "%s %s map: %d of %d sorted rows differ, first %d: device %r, oracle %r" % (
                name, what, bad.sum(), len(bad), np.flatnonzero(bad)[0], a[bad][0].view(np.float64), b[bad][0].view(np.float64))
            rows += len(a)
    else:
        assert dev["global"] is None and dev["n_global"] == 0 and dev["photon_launches"] == 0, name
    pts = dev["points"] + 0.0
    bad = (pts.view(np.uint64) != (gp + 0.0).view(np.uint64)).any(axis=1)
    assert not bad.any(), "%s: %d of %d gather points differ, first pixel %d: device %r, oracle %r" % (
        name, bad.sum(), len(bad), np.flatnonzero(bad)[0], pts[bad][0], gp[bad][0])
    return rows, len(pts)


def expected_rows(cases):
    return sum(len(tc.oracle_run(c)[0]) + len(tc.oracle_run(c)[1]) for c in cases if c["photons"]), sum(c["width"] * c["height"] for c in cases)


@pytest.mark.parametrize("fam", [f for f in tc.FAMILIES if f != "g_stride"])
def test_photon_and_eye_pass_equal_the_oracle(fam, tuning):
    cases = tc.family(fam)
    done = [run_case(c, tuning) for c in cases]
    assert (sum(d[0] for d in done), sum(d[1] for d in done)) == expected_rows(cases)      # no row left out
    if fam == "e_variants":
        assert {c["variant"] for c in cases} == {w for _, _, _, w in tc.VARIANTS}             # (each asserted above) all 8 photon kernels, all 6 eye kernels
    if fam == "f_capacity":                                                                 # and the same maps each time
        assert len({(len(tc.oracle_run(c)[0]), len(tc.oracle_run(c)[1])) for c in cases}) == 1


def test_eye_pass_takes_a_second_trip_through_its_grid_stride_loop(tuning):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = tc.family("g_stride", cus)
    (c,) = cases
    assert c["width"] * c["height"] > cus * 8 * 256
    gp = tc.oracle_run(c)[2]
    assert (gp[cus * 8 * 256:, 0] != 0).all()                       # what a kernel without the second trip would leave at zero
    assert run_case(c, tuning) == expected_rows(cases)


def test_render_statistics_equal_the_gather_on_the_traced_maps():
    """what ties the diagnostic to the render: two iterations of rt_render_sppm's pre-pass on the small Cornell configuration of
    tests/test_sppm.py leave the statistics the gather diagnostic computes from the maps and points this diagnostic traces on the device"""
    import rtamd
    from test_sppm import CFG
    w, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    cfg = dict(CFG, iterations=2)
    _, st, tot, _ = w.render_sppm(cam, width=24, height=24, spp=0, seed=1, **cfg)
    stats = np.zeros((24 * 24, 10))
    n = [0, 0]
    for it in range(2):
        tr = w.debug_sppm_trace(cam, 24, 24, iteration=it, photons_per_iter=cfg["photons_per_iter"], seed=1)
        assert not tr["unit_zero"] and tr["photon_launches"] == 1 and tr["variant"] == tc.ACCEL | tc.LDS
        n = [n[0] + tr["n_global"], n[1] + tr["n_caustic"]]
        dev = rtamd.debug_sppm_gather(tr["global"], tr["caustic"], tr["points"], stats, cfg["k_global"], cfg["k_caustic"], 0.7, tr["S"],
                                      2.0 * cfg["photons_per_iter"], grids=False)
        assert not dev["unit_zero"]
        stats = dev["stats"]
    assert tuple(n) == tot and tot[1] > 0
    assert sp.same(stats, st.reshape(-1, 10)).all()
    assert 100 < (stats[:, 4] > 0).sum() < len(stats)


# ---- what a render refuses, the entry refuses -----------------------------------------------------------------------------------------------
def _refused(fn, code, *words):
    import rtamd
    with pytest.raises(rtamd.RtError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for wd in words:
        assert wd in str(e.value), str(e.value)


def _small(kind):
    import rtamd
    w = rtamd.World()
    white = w.Lambertian(w.ConstantTexture((0.8, 0.8, 0.8)))
    floor = w.XZRectangle((-5.0, -5.0), (5.0, 5.0), 0.0, white)
    cam = rtamd.Camera(((0.0, 2.0, -6.0), (0.0, 1.0, 0.0)), (0, 1, 0), 40.0, 1.0, 0.0, 6.0)
    if kind == "light_in_medium":
        lt = w.SphereDiffuseLight((0.0, 3.0, 0.0), 0.5, (1.0, 1.0, 1.0), 100.0)
        items = [floor, w.ConstantMedium(0.5, lt, w.Isotropic(w.ConstantTexture((0.9, 0.9, 0.9))))]
    else:
        lt = w.XZRectLight((-1.0, -1.0), (1.0, 1.0), 5.0, (1.0, 1.0, 1.0), 100.0)
        items = [floor, lt]
        if kind == "moving":
            items.append(w.MovingSphere((0.0, 1.0, 0.0), (0.5, 1.0, 0.0), 0.0, 1.0, 1.0, white))
    if kind == "background":
        w.set_background(color=(0.5, 0.6, 0.7))
    w.new(items, lights=[lt], bvh_seed=1)
    return w, cam


@pytest.mark.parametrize("kind, words", [("background", ("background",)), ("moving", ("no notion of time",)), ("light_in_medium", ("light", "ConstantMedium"))])
def test_what_a_render_refuses_the_entry_refuses(kind, words):
    w, cam = _small(kind)
    _refused(lambda: w.render_sppm(cam, width=8, height=8, spp=1, iterations=1, photons_per_iter=500), -10, *words)
    _refused(lambda: w.debug_sppm_trace(cam, 8, 8, photons_per_iter=500), -10, *words)


def test_a_host_buffer_one_row_short_is_refused_with_the_counts():
    import ctypes as C
    import rtamd
    c = tc.family("f_capacity")[0]
    w, cam, _ = tc.scene(c["scene"])
    g, cau, _, _ = tc.oracle_run(c)
    kw = dict(iteration=c["iteration"], photons_per_iter=c["P"], seed=c["seed"], points=False)
    for rows in ((len(g) - 1, len(cau)), (len(g), len(cau) - 1)):
        io = rtamd.rt_debug_sppm_trace()
        io.width, io.height, io.iteration, io.photons_per_iter, io.max_bounces, io.seed = c["width"], c["height"], c["iteration"], c["P"], 4096, c["seed"]
        bg, bc = np.zeros((rows[0], 9)), np.zeros((rows[1], 9))
        io.global_, io.global_rows = bg.ctypes.data_as(C.POINTER(C.c_double)), rows[0]
        io.caustic, io.caustic_rows = bc.ctypes.data_as(C.POINTER(C.c_double)), rows[1]
        assert rtamd.lib().rt_debug_sppm_trace_device(w.h, C.byref(cam.c), 0, C.byref(io)) == -1          # RT_ERR_ARG
        assert (io.n_global, io.n_caustic) == (len(g), len(cau)) and not bg.any() and not bc.any()       # the counts, and no partial copy
        _refused(lambda: w.debug_sppm_trace(cam, c["width"], c["height"], rows=rows, **kw), -1, "fewer rows")
    exact = w.debug_sppm_trace(cam, c["width"], c["height"], rows=(len(g), len(cau)), **kw)
    assert exact["points"] is None and np.array_equal(tc.sorted_rows(exact["global"]), tc.sorted_rows(g))
    sized = w.debug_sppm_trace(cam, c["width"], c["height"], **dict(kw, photons_per_iter=1, iteration=0))   # the wrapper's defaults always fit
    assert sized["n_global"] <= 8 + 1024
