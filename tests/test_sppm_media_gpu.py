"""SPPM (rt_render_sppm) on scenes with a ConstantMedium: the photon pass, the eye pass and the final pass walk through
media with their own streams (photon: (seed^PHOTON, photon index); eye: (seed^EYE, pixel, iteration); final pass: the path's), and a
volume event is a pass-through (Specular) interaction (D8).  Every render is compared with oracle.Scene.render_sppm on the same scene,
built through both builders: photon totals, all 10 per-pixel statistics and the image, bit for bit."""

import numpy as np
import pytest

import nested_scenes as ns
from sppm_trace_cases import OB, _cornell_smoke, _cornell_smoke_book, _nested_fog, _pair  # noqa: F401  (both builders; shared with the trace cases)

pytestmark = pytest.mark.gpu

CFG = dict(iterations=3, photons_per_iter=20000, k_global=40, k_caustic=10)


def _assert_same(got, exp, floor):
    """photon totals, the 10 per-pixel statistics and the image equal the oracle's; `floor`: least fraction of non-zero pixels (the
    Cornell frames at this size: about 0.34)"""
    img, st, tot = got[0], got[1], got[2]
    eimg, est, etot = exp
    assert tot == etot, (tot, etot)
    assert np.array_equal(st, est), "per-pixel SPPM statistics differ in %d pixels" % int((st != est).any(axis=2).sum())
    assert np.array_equal(img, eimg, equal_nan=True), "%d pixels differ" % int(((img != eimg) & ~(np.isnan(img) & np.isnan(eimg))).any(axis=2).sum())
    assert (eimg > 0).any(axis=2).mean() > floor      # not a black (or all-NaN) frame


CORNELL_CAM = ns.CORNELL_CAM


_ORACLE = {}


def _oracle(key, o, *args, **kw):
    """oracle frames are shared between the tests of this module (each costs seconds of CPU)"""
    if key not in _ORACLE:
        _ORACLE[key] = o.render_sppm(*args, n_workers=16, **kw)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def smoke():
    w, cam, o = _pair(_cornell_smoke, CORNELL_CAM, bvh_seed=2)
    return w, cam, _oracle("smoke", o, 48, 32, 3, seed=1, **CFG)


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_cornell_smoke_on_the_accel_walk(smoke, kernel):
    w, cam, exp = smoke
    assert w.info()["accel_ok"] == 1
    got = w.render_sppm(cam, width=48, height=32, spp=3, seed=1, kernel=kernel, **CFG)
    assert got[3]["kernel_used"] == (2 if kernel == 0 else kernel)
    _assert_same(got, exp, 0.25)


def test_cornell_smoke_as_the_book_builds_it():
    w, cam, o = _pair(_cornell_smoke_book, CORNELL_CAM, bvh_seed=3)
    assert w.info()["accel_ok"] == 0
    exp = o.render_sppm(40, 28, 2, seed=5, n_workers=16, **CFG)
    got = w.render_sppm(cam, width=40, height=28, spp=2, seed=5, **CFG)
    assert got[3]["kernel_used"] == 1
    _assert_same(got, exp, 0.25)


def _fogged_caustics(with_fog):
    def build(B):
        white = B.Lambertian(B.ConstantTexture((0.8, 0.8, 0.8)))
        glass = B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0)))
        light = B.SphereDiffuseLight((0.0, 5.0, 0.0), 0.3, (1.0, 0.9, 0.8), 500.0)
        items = [B.XZRectangle((-6.0, -6.0), (6.0, 6.0), 0.0, white), B.Sphere((0.0, 1.0, 0.0), 1.0, glass), light]
        if with_fog:   # holds the light and the glass ball
            items.append(B.ConstantMedium(0.04, B.Sphere((0.0, 2.5, 0.0), 4.0, white), B.Isotropic(B.ConstantTexture((0.9, 0.85, 0.8)))))
        return items, [light]
    return build


def test_sphere_light_and_glass_inside_a_sphere_bounded_fog():
    cam_args = ((0.0, 4.0, -8.0), (0.0, 0.5, 0.0), (0, 1, 0), 40.0, 1.0, 0.0, 8.0)
    cfg = dict(iterations=3, photons_per_iter=5000, k_global=30, k_caustic=20)
    w, cam, o = _pair(_fogged_caustics(True), cam_args)
    exp = o.render_sppm(32, 32, 2, seed=4, n_workers=16, **cfg)
    got = w.render_sppm(cam, width=32, height=32, spp=2, seed=4, **cfg)
    _assert_same(got, exp, 0.5)
    assert got[2][1] > 0 and (got[1][..., 9] > 0).any()          # the caustic map receives photons, and pixels gather them
    w2, cam2, _ = _pair(_fogged_caustics(False), cam_args)
    clear = w2.render_sppm(cam2, width=32, height=32, spp=2, seed=4, **cfg)
    assert clear[2] != got[2]                                     # the fog changes what the photon pass stores


def _c5r_lit(B):
    """rtamd.shapes.final_scene_reduced with its ceiling rectangle made an XZRectLight (flux 7): photons start inside the global fog"""
    from rtamd import shapes
    items = shapes.final_scene_reduced(B)
    items[1] = B.XZRectLight((123.0, 147.0), (423.0, 412.0), 554.0, (7.0, 7.0, 7.0), 1.0)
    return items, [items[1]]


def test_final_scene_reduced_with_a_rect_light():
    from rtamd import shapes
    cfg = dict(iterations=3, photons_per_iter=20000, k_global=40, k_caustic=10)
    w, cam, o = _pair(_c5r_lit, shapes.FINAL_SCENE_CAMERA, bvh_seed=3)
    assert w.info()["accel_ok"] == 1
    exp = o.render_sppm(48, 48, 4, seed=2, n_workers=16, **cfg)
    got = w.render_sppm(cam, width=48, height=48, spp=4, seed=2, **cfg)
    assert got[3]["kernel_used"] == 2
    _assert_same(got, exp, 0.4)


@pytest.fixture(scope="module")
def nested():
    w, cam, o = _pair(_nested_fog, CORNELL_CAM, bvh_seed=4)
    return w, cam, _oracle("nested", o, 36, 24, 2, seed=3, **CFG)


@pytest.mark.parametrize("kernel", [1, 2])
def test_nested_transforms_with_media(nested, kernel):
    w, cam, exp = nested
    assert w.info()["accel_ok"] == 1
    got = w.render_sppm(cam, width=36, height=24, spp=2, seed=3, kernel=kernel, **CFG)
    assert got[3]["kernel_used"] == kernel
    _assert_same(got, exp, 0.25)


def test_nested_media_under_transforms():
    """tests/nested_scenes.n6: a medium under two Transforms (reference-order walks only) and one whose boundary is a 2-level chain"""
    import oracle
    import rtamd
    w, cam = ns.n6(rtamd.World())
    o = ns.n6(oracle.Scene())
    assert w.info()["accel_ok"] == 0
    exp = o.render_sppm(32, 24, 2, seed=1, n_workers=16, **CFG)
    got = w.render_sppm(cam, width=32, height=24, spp=2, seed=1, **CFG)
    _assert_same(got, exp, 0.25)


@pytest.mark.parametrize("setting", [dict(no_lds=1), dict(sppm_photon_capacity=64), dict(sppm_knn_candidates=0)])
def test_tuning_switches_give_the_same_bits(smoke, tuning, setting):
    """photon pass without the staged tables, grow-and-retry of the photon buffers (the streams are replayed), k-nearest selection
    outside LDS: the same frame as the default (and therefore as the oracle's)"""
    w, cam, exp = smoke
    tuning(**setting)
    got = w.render_sppm(cam, width=48, height=32, spp=3, seed=1, **CFG)
    _assert_same(got, exp, 0.25)


def test_multi_device_fanout_equals_the_single_device_frame(smoke, tuning):
    w, cam, exp = smoke
    tuning(multi_force_rccl=1)
    img, st = w.render_sppm_multi(cam, devices=[0, 0, 0], width=48, height=32, spp=3, seed=1, **CFG)
    assert len(st) == 3 and np.array_equal(img, exp[0], equal_nan=True)


@pytest.mark.parametrize("world_size", [2, 3])
def test_tiles_over_ranks_stitch_to_the_single_device_frame(smoke, world_size):
    import torch
    import rtamd
    from rtamd.distributed import TileLayout, stitch_host
    w, cam, exp = smoke
    W, H = 48, 32
    lay = TileLayout(W, H, world_size)
    parts = []
    for r in range(world_size):
        p = rtamd.default_params(width=W, height=H, spp=3, seed=1, rank=r, world=world_size)
        buf = torch.zeros(lay.stride * 64 * 3, dtype=torch.float64, device="cuda:0")
        info = w.render_sppm_tiles_device(cam, p, buf.data_ptr(), **CFG)
        assert info["prepass_seconds"] > 0
        parts.append(buf.cpu())
    frame = stitch_host(torch.cat(parts).numpy(), lay)
    assert np.array_equal(frame, exp[0], equal_nan=True)


# ---- what stays refused ------------------------------------------------------------------------------------------------------------
def _refused(fn, *words):
    import rtamd
    with pytest.raises(rtamd.RtError) as e:
        fn()
    assert e.value.code == -10, str(e.value)
    for wd in words:
        assert wd in str(e.value), str(e.value)


def test_media_refusals(smoke):
    w, cam, _ = smoke
    tiny = dict(width=8, height=8, spp=1, seed=1)
    _refused(lambda: w.render(cam, integrator=1, **tiny), "ConstantMedium", "integrator 0")
    _refused(lambda: w.render(cam, kernel=5, **tiny), "kernel 5")
    _refused(lambda: w.render(cam, kernel=6, **tiny), "kernel 6")
    _refused(lambda: w.render_sppm(cam, kernel=5, iterations=1, photons_per_iter=500, **tiny), "kernel 5")
    _refused(lambda: w.debug_hit(np.array([[278.0, 278.0, -800.0, 0.0, 0.0, 1.0]]), kernel=1), "ConstantMedium")


def test_book2_media_under_sppm_are_refused():
    import rtamd
    for kind in ("moving", "noise"):
        w = rtamd.World()
        white = w.Lambertian(w.ConstantTexture((0.8, 0.8, 0.8)))
        fog = w.Isotropic(w.ConstantTexture((0.9, 0.9, 0.9)))
        lt = w.XZRectLight((-1.0, -1.0), (1.0, 1.0), 5.0, (1.0, 1.0, 1.0), 100.0)
        if kind == "moving":   # a fog with a moving boundary
            med = w.ConstantMedium(0.5, w.MovingSphere((0.0, 1.0, 0.0), (0.5, 1.0, 0.0), 0.0, 1.0, 1.0, white), fog)
        else:
            med = w.ConstantMedium(0.5, w.Sphere((0.0, 1.0, 0.0), 1.0, white), fog)
        items = [w.XZRectangle((-5.0, -5.0), (5.0, 5.0), 0.0, w.Lambertian(w.NoiseTexture(0.5)) if kind == "noise" else white), lt, med]
        w.new(items, lights=[lt], bvh_seed=1)
        cam = rtamd.Camera(((0.0, 2.0, -6.0), (0.0, 1.0, 0.0)), (0, 1, 0), 40.0, 1.0, 0.0, 6.0)
        _refused(lambda: w.render_sppm(cam, width=8, height=8, spp=1, iterations=1, photons_per_iter=500), "no notion of time")


def test_medium_inside_a_medium_is_refused():
    import rtamd
    w = rtamd.World()
    m = w.Isotropic(w.ConstantTexture((1.0, 1.0, 1.0)))
    inner = w.ConstantMedium(1.0, w.Sphere((0.0, 0.0, 0.0), 1.0, m), m)
    _refused(lambda: w.ConstantMedium(1.0, inner, m), "ConstantMedium as the boundary of a ConstantMedium")
    w2 = rtamd.World()
    m = w2.Isotropic(w2.ConstantTexture((1.0, 1.0, 1.0)))
    inner = w2.ConstantMedium(1.0, w2.Sphere((0.0, 0.0, 0.0), 1.0, m), m)
    outer = w2.ConstantMedium(1.0, w2.HitableList([w2.Sphere((0.0, 0.0, 0.0), 2.0, m), inner]), m)
    _refused(lambda: w2.new([outer, w2.Sphere((0.0, -10.0, 0.0), 5.0, m)], bvh_seed=1), "inside the boundary of a ConstantMedium")


def test_a_light_that_bounds_a_medium_is_refused_by_sppm():
    """a SphereDiffuseLight that is also the boundary of a ConstantMedium: the photon pass refuses it; integrator 0 renders it"""
    import rtamd
    w = rtamd.World()
    white = w.Lambertian(w.ConstantTexture((0.8, 0.8, 0.8)))
    lt = w.SphereDiffuseLight((0.0, 3.0, 0.0), 0.5, (1.0, 1.0, 1.0), 100.0)
    med = w.ConstantMedium(0.5, lt, w.Isotropic(w.ConstantTexture((0.9, 0.9, 0.9))))
    w.new([w.XZRectangle((-5.0, -5.0), (5.0, 5.0), 0.0, white), med], lights=[lt], bvh_seed=1)
    cam = rtamd.Camera(((0.0, 2.0, -6.0), (0.0, 1.0, 0.0)), (0, 1, 0), 40.0, 1.0, 0.0, 6.0)
    _refused(lambda: w.render_sppm(cam, width=8, height=8, spp=1, iterations=1, photons_per_iter=500), "light", "ConstantMedium")
    img, _ = w.render(cam, width=8, height=8, spp=1, seed=1)
    assert np.isfinite(img).all()
