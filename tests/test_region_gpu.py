"""Pixel regions of a frame on the GPU (rt_region_render): every region is the slice of rt_render's frame for the same
scene, camera and params, bit for bit -- whatever kernel, LDS residency, unit size or launch split renders it -- and equals the oracle's
render(..., window=...), the independent check; rt_stats.samples is what the touched tiles cost."""
import numpy as np
import pytest

import light_scenes as ls
import nested_scenes as ns
from conftest import scene_path
from region_cases import case_regions, in_image_pixels, python_tiles, small_regions
from seeded_windows import seeded_windows

pytestmark = pytest.mark.gpu


def assert_slices(views, regions, frame, what=""):
    assert len(views) == len(regions)
    for v, (x0, y0, x1, y1) in zip(views, regions):
        assert v.shape == (y1 - y0, x1 - x0, 3)
        assert np.array_equal(v, frame[y0:y1, x0:x1]), "%s region (%d, %d, %d, %d)" % (what, x0, y0, x1, y1)


# ---- 1. scene_10, 61 x 37: partial tiles on both edges, every kind of region in ONE call ----------------------------------------------
W1, H1, SPP1 = 61, 37, 8


@pytest.fixture(scope="module")
def scene_10():
    """the product scene, rt_render's frame and the oracle's window of every distinct region of the call, each computed once"""
    import oracle
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    frame, st = world.render(cam, width=W1, height=H1, spp=SPP1, seed=1)
    assert st["samples"] == W1 * H1 * SPP1 and frame.max() > 0
    frame.setflags(write=False)
    sc = oracle.load_scene_file(scene_path("scene_10.json"))
    windows = {r: sc.render(W1, H1, SPP1, seed=1, window=r)[0] for r in set(case_regions(W1, H1))}
    return world, cam, frame, windows


def test_one_call_with_every_kind_of_region_equals_the_frame_and_the_oracle(scene_10):
    world, cam, frame, windows = scene_10
    regions = case_regions(W1, H1)
    views, st = world.render_regions(cam, regions, width=W1, height=H1, spp=SPP1, seed=1)
    assert_slices(views, regions, frame)
    for v, r in zip(views, regions):
        assert np.array_equal(v, windows[r]), "oracle window %r" % (r,)
    assert st["samples"] == W1 * H1 * SPP1 and st["launches"] == 1              # the whole frame is among them: every tile, once
    # the same call without the whole frame leaves tiles untouched, and costs exactly the touched ones
    small = small_regions(W1, H1)
    views, st = world.render_regions(cam, small, width=W1, height=H1, spp=SPP1, seed=1)
    assert_slices(views, small, frame)
    tiles = python_tiles(W1, H1, small)
    assert st["samples"] == in_image_pixels(W1, H1, tiles) * SPP1 < W1 * H1 * SPP1
    # one region through render_region
    one, st = world.render_region(cam, (W1 - 1, H1 - 1, W1, H1), width=W1, height=H1, spp=SPP1, seed=1)
    assert np.array_equal(one, frame[H1 - 1:, W1 - 1:]) and st["samples"] == 5 * 5 * SPP1    # the partial corner tile: 5 x 5 pixels inside


@pytest.mark.parametrize("variant", ["kernel1", "kernel2", "no_lds", "sub_spp1", "sub_spp8", "spp_chunk3"])
def test_the_bits_do_not_depend_on_kernel_residency_or_schedule(scene_10, tuning, variant):
    world, cam, frame, _ = scene_10
    kw = dict(width=W1, height=H1, spp=SPP1, seed=1)
    if variant == "kernel1":
        kw["kernel"] = 1
    elif variant == "kernel2":
        kw["kernel"] = 2
    elif variant == "no_lds":
        tuning(no_lds=1)
    elif variant == "sub_spp1":
        tuning(sub_spp=1)
    elif variant == "sub_spp8":
        tuning(sub_spp=8)
    else:
        kw["spp_chunk"] = 3
    for regions in (case_regions(W1, H1), small_regions(W1, H1)):
        views, st = world.render_regions(cam, regions, **kw)
        assert_slices(views, regions, frame, variant)
        assert st["samples"] == in_image_pixels(W1, H1, python_tiles(W1, H1, regions)) * SPP1
    if variant in ("kernel1", "kernel2"):
        assert st["kernel_used"] == kw["kernel"]
    if variant == "no_lds":
        assert st["scene_in_lds"] == 0
    if variant == "spp_chunk3":
        assert st["launches"] == 3 and st["spp_chunk"] == 3


# ---- 2. Cornell box, light importance sampling ---------------------------------------------------------------------------------------
def test_cornell_box_integrator_1_equals_the_frame_and_the_oracle():
    import oracle
    import rtamd
    world, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    sc = oracle.cornell_box_scene(scene_path("cube.obj"), 1.0, seed=1)
    kw = dict(width=48, height=48, spp=4, seed=1, integrator=1)
    frame, _ = world.render(cam, **kw)
    regions = [(13, 9, 30, 26), (40, 40, 48, 48)]
    views, st = world.render_regions(cam, regions, **kw)
    assert_slices(views, regions, frame)
    for v, r in zip(views, regions):
        assert np.array_equal(v, sc.render(48, 48, 4, seed=1, integrator=1, window=r)[0]), r
    assert st["samples"] == len(python_tiles(48, 48, regions)) * 64 * 4


# ---- 3. backgrounds, env sampling, area lights ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["sky_env", "area"])
def test_env_sampled_sky_and_area_lights_equal_the_frame(scene):
    if scene == "sky_env":
        world, cam, _, extra = ls.pair_cornell(ls.GRADIENT, (16, 8))
    else:
        world, cam, _, extra = ls.pair_area()
    kw = dict(width=40, height=28, spp=4, seed=3, integrator=1, **extra)
    frame, st_f = world.render(cam, **kw)
    region = (9, 6, 31, 21)
    view, st = world.render_region(cam, region, **kw)
    assert frame.max() > 0 and np.array_equal(view, frame[6:21, 9:31])
    assert st["kernel_used"] == st_f["kernel_used"] and st["samples"] == len(python_tiles(40, 28, [region])) * 64 * 4


# ---- 4. a ConstantMedium --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
def test_constant_medium_equals_the_frame(kernel):
    world, cam, _, extra = ls.pair_smoke(None)
    kw = dict(width=40, height=40, spp=4, seed=2, integrator=0, kernel=kernel, **extra)
    frame, _ = world.render(cam, **kw)
    regions = [(3, 5, 22, 18), (20, 12, 40, 40)]
    views, st = world.render_regions(cam, regions, **kw)
    assert frame.max() > 0 and st["kernel_used"] == kernel
    assert_slices(views, regions, frame)


# ---- 5. the instance service: kernel 5 ------------------------------------------------------------------------------------------------
def test_torus_mesh_cornell_takes_kernel_5_and_equals_the_frame():
    import rtamd
    from rtamd import shapes
    world = rtamd.World()
    P, N, I = shapes.torus(nu=40, nv=80)
    world.new(shapes.cornell_with_mesh(world, P, N, I), bvh_seed=1)
    f, t, up, vfov, asp, ap, fd = ns.CORNELL_CAM
    cam = rtamd.Camera((f, t), up, vfov, asp, ap, fd)
    kw = dict(width=32, height=24, spp=2, seed=1)
    frame, _ = world.render(cam, **kw)
    regions = [(6, 4, 27, 19), (0, 0, 32, 24), (31, 23, 32, 24)]
    for kernel in (0, 5):
        views, st = world.render_regions(cam, regions, kernel=kernel, **kw)
        assert st["kernel_used"] == 5
        assert_slices(views, regions, frame, "kernel %d" % kernel)
    views, st = world.render_regions(cam, regions[:1], **kw)                 # few tiles: fewer than the launch has workgroups
    assert st["kernel_used"] == 5
    assert_slices(views, regions[:1], frame)


# ---- 6. the headline size ---------------------------------------------------------------------------------------------------------------
def test_headline_windows_at_1000_spp_equal_the_oracle_for_44_tiles():
    """scene_500, 1200 x 1200, 1000 spp, seed 1: the three fixed windows of tests/test_golden.py and the eight of seeded_windows in ONE
    region call -- at most 44 tiles x 64 x 1000 samples in place of the frame's 1.44 G"""
    import oracle
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_500.json"))
    sc = oracle.load_scene_file(scene_path("scene_500.json"))
    corners = [(600, 900), (296, 640), (1000, 40)] + seeded_windows(1200, 1200, 1000)
    regions = [(x0, y0, x0 + 8, y0 + 8) for (x0, y0) in corners]
    assert len(regions) == 11
    views, st = world.render_regions(cam, regions, width=1200, height=1200, spp=1000, seed=1)
    assert st["samples"] == len(python_tiles(1200, 1200, regions)) * 64 * 1000 <= 44 * 64 * 1000
    assert st["launches"] == 1 and st["kernel_used"] == 2
    for v, r in zip(views, regions):
        exp, _ = sc.render(1200, 1200, 1000, seed=1, window=r, n_jobs=8)
        assert np.array_equal(v, exp), "window at (%d, %d)" % r[:2]
    assert max(v.max() for v in views) > 0


# ---- 7. rt_region_render_device ---------------------------------------------------------------------------------------------------------
def test_device_entry_point_on_a_torch_stream_equals_the_host_entry_point(scene_10):
    import torch
    import rtamd
    world, cam, frame, _ = scene_10
    regions = case_regions(W1, H1)
    p = rtamd.default_params(width=W1, height=H1, spp=SPP1, seed=1)
    n = rtamd.region_doubles(p, regions)
    host, st_h = world.render_regions(cam, regions, width=W1, height=H1, spp=SPP1, seed=1)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream):
        out = torch.full((n + 8,), -1.0, dtype=torch.float64, device="cuda")
    stream.synchronize()
    st = world.render_regions_device(cam, p, regions, out.data_ptr(), stream.cuda_stream)     # returns after the work has completed
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], np.concatenate([v.ravel() for v in host]))
    assert (got[n:] == -1.0).all()                                                           # nothing behind the packed output
    assert st["samples"] == st_h["samples"] and st["kernel_used"] == st_h["kernel_used"]
    at = 0
    for (x0, y0, x1, y1) in regions:
        size = (y1 - y0) * (x1 - x0) * 3
        assert np.array_equal(got[at:at + size].reshape(y1 - y0, x1 - x0, 3), frame[y0:y1, x0:x1])
        at += size
