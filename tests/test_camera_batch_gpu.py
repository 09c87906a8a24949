"""Camera rays generated 64 at a time: whole frames against the oracle, bit for bit.

The sphere-only LDS variants of pt_kernel no longer build a camera ray in the lane whose path ended.  The whole wave generates the 64
rays of one (tile, sample index) -- a batch -- into a buffer of its own in global memory, and free lanes pick their entry up: origin,
direction and the stream's state after the camera draws.  What can go wrong is which entry a lane takes, when a batch is generated (a
new unit, a batch boundary inside one regeneration, the end of a unit), what travels through the buffer (the origin differs per ray
only under a lens) and pixels of edge tiles outside the image, which get no entry.  So the cases are the smallest shapes at which each
of those happens:

  * scene_10 at 61 x 37 (partial tiles on both edges) with 1, 8, 9 and 17 samples: one batch, exactly one unit (8 sample indices), one
    unit plus one batch, two units plus one batch.  Frames this small run the POOL twin of the kernel;
  * scene_10 at 520 x 516 x 11: more tiles than the launch has waves, so the FIFO twin runs (asserted from the call's stats);
  * five spheres built here under a lens of aperture 0.3, 48 x 32 x 8: the origins differ per ray;
  * the same kernel launched on a pixel region, on the sample ranges of an adaptive render and on the tile list of rank 1 of 3.

Every frame goes through kernel 2 with the scene in LDS (the batched variants), kernel 2 with the scene forced out of LDS and kernel 1
(both generate per lane, as before); the oracle renders each frame once."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 5
# name: (World.render's kernel, the no_lds tuning, kernel_used and scene_in_lds of the call's stats)
FORMS = {
    "kernel2-lds": (2, 0, 2, 1),
    "kernel2-plain": (2, 1, 2, 0),
    "kernel1": (1, 0, 1, None),
}


def _same(got, exp, what):
    if np.array_equal(got, exp):
        return
    bad = (got != exp).any(axis=-1)
    idx = np.argwhere(bad)[:4]
    lines = ["  %s: hip=%s oracle=%s" % (tuple(int(v) for v in i), got[tuple(i)].tolist(), exp[tuple(i)].tolist()) for i in idx]
    raise AssertionError("%s: %d / %d pixels differ, first (index):\n%s" % (what, int(bad.sum()), bad.size, "\n".join(lines)))


def _check_stats(st, form):
    _, _, used, lds = FORMS[form]
    assert st["kernel_used"] == used, st
    if lds is not None:
        assert st["scene_in_lds"] == lds, st


def _render(world, cam, form, tuning, **kw):
    kernel, no_lds, _, _ = FORMS[form]
    tuning(no_lds=no_lds)
    img, st = world.render(cam, kernel=kernel, **kw)
    _check_stats(st, form)
    return img, st


@functools.lru_cache(maxsize=None)
def _scene_10():
    return configs.product("scene_10")


@functools.lru_cache(maxsize=None)
def _oracle_scene_10(width, height, spp):
    exp, cnt = configs.oracle_scene("scene_10").render(width, height, spp, seed=SEED, n_workers=16)
    assert cnt["n_samples"] == width * height * spp
    assert (exp != 0).any(), "the oracle frame is black: nothing is compared"
    exp.setflags(write=False)
    return exp


# ---- batch and unit boundaries -------------------------------------------------------------------------------------------------------
BW, BH = 61, 37


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("spp", [1, 8, 9, 17])
def test_batch_and_unit_boundaries(spp, form, tuning):
    world, cam = _scene_10()
    exp = _oracle_scene_10(BW, BH, spp)
    img, st = _render(world, cam, form, tuning, width=BW, height=BH, spp=spp, seed=SEED)
    tiles = ((BW + 7) // 8) * ((BH + 7) // 8)
    print("scene_10 %dx%dx%d %s: kernel_ms %.3f, %d tiles for %d waves" % (BW, BH, spp, form, st["kernel_ms"], tiles, st["grid_blocks"] * st["block_threads"] // 64))
    assert st["samples"] == BW * BH * spp
    assert tiles < st["grid_blocks"] * st["block_threads"] // 64  # (fewer tiles than waves: single-unit jobs, the POOL twin where one exists)
    _same(img, exp, "scene_10 %dx%dx%d, %s" % (BW, BH, spp, form))


# ---- the FIFO variant ----------------------------------------------------------------------------------------------------------------
FW_, FH_, FSPP_ = 520, 516, 11


@pytest.mark.parametrize("form", list(FORMS))
def test_fifo_variant(form, tuning):
    world, cam = _scene_10()
    kernel, no_lds, _, _ = FORMS[form]
    tuning(no_lds=no_lds)
    img, st = world.render(cam, kernel=kernel, width=FW_, height=FH_, spp=FSPP_, seed=SEED)
    _check_stats(st, form)
    tiles = ((FW_ + 7) // 8) * ((FH_ + 7) // 8)
    waves = st["grid_blocks"] * 16
    print("scene_10 %dx%dx%d %s: kernel_ms %.3f, %d tiles for grid_blocks x 16 = %d waves" % (FW_, FH_, FSPP_, form, st["kernel_ms"], tiles, waves))
    if tiles < waves:
        pytest.skip("this device has %d waves for %d tiles: the frame would run the POOL twin, not next_unit()" % (waves, tiles))
    assert tiles >= waves
    exp = _oracle_scene_10(FW_, FH_, FSPP_)
    assert st["samples"] == FW_ * FH_ * FSPP_
    _same(img, exp, "scene_10 %dx%dx%d, %s" % (FW_, FH_, FSPP_, form))


# ---- a lens: five spheres, aperture 0.3 -----------------------------------------------------------------------------------------------
LW, LH, LSPP, LDEPTH = 48, 32, 8, 50
LENS_CAM = ((0.0, 1.2, 5.0), (0.0, 0.6, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.3, 5.0)
BACKGROUND = (0.7, 0.8, 1.0)


def _five_spheres(B):
    ground = B.Sphere((0.0, -1000.0, 0.0), 1000.0, B.Lambertian(B.CheckerTexture(B.ConstantTexture((0.2, 0.3, 0.1)), B.ConstantTexture((0.9, 0.9, 0.9)))))
    matte = B.Sphere((-0.55, 0.5, 0.0), 0.5, B.Lambertian(B.ConstantTexture((0.7, 0.3, 0.3))))
    rough = B.Sphere((0.55, 0.5, 0.0), 0.5, B.Metal(B.ConstantTexture((0.8, 0.8, 0.6)), 1.0))
    glass = B.Sphere((0.0, 0.4, 1.4), 0.4, B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0))))
    lamp = B.Sphere((0.0, 3.5, 0.0), 0.6, B.DiffuseLight(B.ConstantTexture((4.0, 4.0, 4.0))))
    return [ground, matte, rough, glass, lamp]


@functools.lru_cache(maxsize=None)
def _lens_pair():
    import oracle
    import rtamd

    class Deferred(rtamd.World):  # new() leaves the scene uncommitted, so that the background can still be set
        def commit(self):
            return self
    w = Deferred()
    w.new(_five_spheres(w), bvh_seed=1)
    w.set_background(color=BACKGROUND)
    rtamd.World.commit(w)
    o = oracle.Scene()
    o.World(_five_spheres(o), 1)
    o.set_background(1, color0=BACKGROUND)
    o.Camera(*LENS_CAM)
    f, t, up, vfov, asp, ap, fd = LENS_CAM
    return w, rtamd.Camera((f, t), up, vfov, asp, ap, fd), o


@functools.lru_cache(maxsize=None)
def _lens_oracle():
    """the oracle's frame under the lens, after showing that the lens matters: the same frame through a pinhole differs"""
    import oracle
    _, _, o = _lens_pair()
    exp, cnt = o.render(LW, LH, LSPP, max_depth=LDEPTH, seed=SEED, n_workers=16)
    assert cnt["n_samples"] == LW * LH * LSPP
    assert (exp != 0).any(), "the oracle frame is black: nothing is compared"
    p = oracle.Scene()
    p.World(_five_spheres(p), 1)
    p.set_background(1, color0=BACKGROUND)
    p.Camera(*(LENS_CAM[:5] + (0.0,) + LENS_CAM[6:]))
    pin, _ = p.render(LW, LH, LSPP, max_depth=LDEPTH, seed=SEED, n_workers=16)
    differ = int((pin != exp).any(axis=2).sum())
    print("five spheres: %d / %d pixels differ between aperture 0.3 and a pinhole" % (differ, LW * LH))
    assert differ > LW * LH // 2, "the lens changes too little of the frame: the case proves nothing about the ray origins"
    exp.setflags(write=False)
    return exp


@pytest.mark.parametrize("form", list(FORMS))
def test_lens(form, tuning):
    world, cam, _ = _lens_pair()
    exp = _lens_oracle()
    img, st = _render(world, cam, form, tuning, width=LW, height=LH, spp=LSPP, max_depth=LDEPTH, seed=SEED)
    print("five spheres, aperture 0.3, %s: kernel_ms %.3f" % (form, st["kernel_ms"]))
    assert st["samples"] == LW * LH * LSPP
    _same(img, exp, "five spheres %dx%dx%d aperture 0.3, %s" % (LW, LH, LSPP, form))


# ---- sample ranges and tile lists: the other callers of the kernel -------------------------------------------------------------------
RSPP = 9


@pytest.mark.parametrize("form", list(FORMS))
def test_region_is_the_crop_of_the_frame(form, tuning):
    world, cam = _scene_10()
    exp = _oracle_scene_10(BW, BH, RSPP)
    kernel, no_lds, _, _ = FORMS[form]
    tuning(no_lds=no_lds)
    x0, y0, x1, y1 = 13, 5, 61, 37  # (starts inside a tile, ends at the image's partial edge tiles)
    view, st = world.render_region(cam, (x0, y0, x1, y1), width=BW, height=BH, spp=RSPP, seed=SEED, kernel=kernel)
    _check_stats(st, form)
    print("region %s of %dx%dx%d %s: kernel_ms %.3f" % ((x0, y0, x1, y1), BW, BH, RSPP, form, st["kernel_ms"]))
    _same(view, exp[y0:y1, x0:x1], "region (%d, %d, %d, %d) of scene_10 %dx%dx%d, %s" % (x0, y0, x1, y1, BW, BH, RSPP, form))


@pytest.mark.parametrize("form", list(FORMS))
def test_adaptive_at_threshold_0_is_the_frame(form, tuning):
    """rt_render_adaptive with threshold 0 stops no tile early: its frame is rt_render's (tests/test_adaptive_gpu.py), here the oracle's.
    It launches the sample ranges [0, 1) [1, 2) [2, 4) [4, 8) [8, 9): units that begin at a sample index other than 0."""
    world, cam = _scene_10()
    exp = _oracle_scene_10(BW, BH, RSPP)
    kernel, no_lds, _, _ = FORMS[form]
    tuning(no_lds=no_lds)
    img, tile_spp, st = world.render_adaptive(cam, BW, BH, RSPP, min_spp=2, threshold=0.0, seed=SEED, kernel=kernel)
    _check_stats(st, form)
    print("adaptive %dx%dx%d %s: kernel_ms %.3f, launches %d" % (BW, BH, RSPP, form, st["kernel_ms"], st["launches"]))
    assert (tile_spp == RSPP).all() and st["launches"] >= 4, (np.unique(tile_spp), st["launches"])
    assert st["samples"] == BW * BH * RSPP
    _same(img, exp, "adaptive scene_10 %dx%dx%d, %s" % (BW, BH, RSPP, form))


@pytest.mark.parametrize("form", list(FORMS))
def test_rank_1_of_3_renders_its_tiles(form, tuning):
    """rt_render_tiles_device for rank 1 of a world of 3: the tiles t = 1, 4, 7, ... (t % 3 == 1), each [64, 3] in pixel order, against
    the oracle's pixels of those tiles.  Pixels of an edge tile outside the image are zero."""
    import torch
    import rtamd
    world, cam = _scene_10()
    exp = _oracle_scene_10(BW, BH, RSPP)
    kernel, no_lds, _, _ = FORMS[form]
    tuning(no_lds=no_lds)
    p = rtamd.default_params(width=BW, height=BH, spp=RSPP, seed=SEED, kernel=kernel, rank=1, world=3)
    tiles_x, tiles_y = (BW + 7) // 8, (BH + 7) // 8
    mine = [t for t in range(tiles_x * tiles_y) if t % 3 == 1]
    assert rtamd.tiles_owned(p) == len(mine)
    want = np.zeros((len(mine), 64, 3))
    inside = np.zeros((len(mine), 64), dtype=bool)
    for i, t in enumerate(mine):
        tx, ty = t % tiles_x, t // tiles_x
        for pix in range(64):
            x, y = tx * 8 + (pix & 7), ty * 8 + (pix >> 3)
            if x < BW and y < BH:
                want[i, pix] = exp[y, x]
                inside[i, pix] = True
    buf = torch.full((len(mine), 64, 3), float("nan"), dtype=torch.float64, device="cuda")
    st = world.render_tiles_device(cam, p, buf.data_ptr())
    torch.cuda.synchronize()
    _check_stats(st, form)
    got = buf.cpu().numpy()
    outside = got[~inside]
    print("rank 1 of 3, %dx%dx%d %s: %d tiles, %d pixels outside the image, all zero: %s" % (BW, BH, RSPP, form, len(mine), len(outside), bool((outside == 0).all())))
    assert len(outside) > 0 and (outside == 0).all(), "pixels of edge tiles outside the image must be zero"
    assert st["samples"] == int(inside.sum()) * RSPP
    _same(got, want, "rank 1 of 3 of scene_10 %dx%dx%d, %s" % (BW, BH, RSPP, form))
