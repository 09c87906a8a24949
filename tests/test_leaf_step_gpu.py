"""The item step of the sphere-only LDS walk: whole frames against the oracle, bit for bit.

The sphere-only LDS variants of pt_kernel -- the whole-frame kernel, its POOL twin and the background twin -- stage their item table
with every item's first word rewritten to the LDS address of its sphere's row.  The walk reads the sphere through that word, has no
kind test, runs a leaf's items from an address to an end address, and its hit carries the address to materialize, which reads the
row through it and takes the sphere's index (for the material) from its distance to the table.  What can go wrong is an address (a
wrong row, a wrong material), the count of a leaf's items, the rule by which a candidate replaces the hit, and a hit that reaches
materialize in the wrong form.  A wrong value is a wrong pixel, so every case compares every pixel of a frame:

  * scene_500 at 64 x 48, 4 spp, depth 50: leaves of every item count the build produces, the ground sphere, segments inside glass.
    A frame this small has fewer tiles than the GPU has waves and runs the POOL twin; the same scene at 520 x 516, 1 spp has more
    tiles than a launch has waves and runs the whole-frame (FIFO) kernel, the one bench.py measures;
  * scene_10 at 40 x 24, 8 spp: the POOL twin; the same frame under book 1's sky: the background twin;
  * depths 1 and 2 of both: the hit reaches materialize in the iteration in which the path ends, with and without a walk behind it;
  * an exact tie: two coincident spheres of different materials beside others.  They share a leaf (equal centroids are never split),
    every ray that hits one hits the other at the same t, and the later one in reference order must win.  On the oracle's side it is
    shown that the order decides: the frame with the two swapped differs;
  * a leaf of the maximum item count, four: four concentric spheres (three glass shells around a matte core) beside a ground and a
    lamp.  Equal centroids are never split, so they form one leaf; the scene's info says so (6 items under 2 inner nodes are 3 leaves);
  * a pixel region and an adaptive render of the scene_500 frame: the other entry points that launch these variants.

The item step's square root is sqrt_hot (part C): the compiler's core sequence when no active lane of the wave holds an operand outside
[2^-767, +inf), sqrt() for the whole wave otherwise.  rtamd.debug_math(4, x) runs it on waves of 64 consecutive elements, against
numpy.sqrt, with op 0 (the plain sqrt) on the same values as the control.

The oracle renders each frame once, and each of its frames is checked to be finite (a NaN never equals itself: the comparison would
fail for the wrong reason) -- its render() raises if the reference's error flag is set.  Frames go through kernel 2 with the scene in
LDS, the changed code; the built scenes also through kernel 2 out of LDS and kernel 1, which keep the blob's item words."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 11
# name: (World.render's kernel, the no_lds tuning, kernel_used and scene_in_lds of the call's stats)
FORMS = {
    "kernel2-lds": (2, 0, 2, 1),
    "kernel2-plain": (2, 1, 2, 0),
    "kernel1": (1, 0, 1, None),
}
SKY = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))


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


def _waves(st):
    return st["grid_blocks"] * st["block_threads"] // 64


def _checked(exp, cnt, samples, lit=True):
    """an oracle frame the comparison can rest on: complete, finite, and (where the scene allows it) not black"""
    assert cnt["n_samples"] == samples, cnt
    assert np.isfinite(exp).all(), "the oracle frame holds a NaN or an infinity"
    if lit:
        assert (exp != 0).any(), "the oracle frame is black: nothing is compared"
    exp.setflags(write=False)
    return exp


# ---- the scene files: scene_500, scene_10, scene_10 under a sky ------------------------------------------------------------------------
SHAPES = {"scene_500": (64, 48, 4), "scene_10": (40, 24, 8), "scene_10_sky": (40, 24, 8)}
FILES = {"scene_500": "scene_500.json", "scene_10": "scene_10.json", "scene_10_sky": "scene_10.json"}
ASPECT = {"scene_500": None, "scene_10": 16 / 9, "scene_10_sky": 16 / 9}


@functools.lru_cache(maxsize=None)
def _product(key):
    import rtamd
    w, cam = rtamd.load_scene_file(os.path.join(configs.SCENES, FILES[key]), commit=False)
    if key.endswith("_sky"):
        w.set_background(gradient=SKY)
    w.commit()
    return w, (cam if ASPECT[key] is None else cam.with_aspect(ASPECT[key]))


@functools.lru_cache(maxsize=None)
def _oracle(key):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    o = oracle.load_scene_file(os.path.join(configs.SCENES, FILES[key]), aspect=ASPECT[key])
    if key.endswith("_sky"):
        o.set_background(2, color0=SKY[0], color1=SKY[1])
    return o


@functools.lru_cache(maxsize=None)
def _oracle_frame(key, width, height, spp, depth):
    exp, cnt = _oracle(key).render(width, height, spp, max_depth=depth, seed=SEED, n_workers=16)
    # (without a background a path that sees no light within `depth` surfaces is black: scene_10's lights sit inside glass shells)
    return _checked(exp, cnt, width * height * spp, lit=key.endswith("_sky") or depth >= 50)


@pytest.mark.parametrize("depth", [1, 2, 50])
@pytest.mark.parametrize("key", list(SHAPES))
def test_small_frame(key, depth, tuning):
    """fewer tiles than waves: scene_500 and scene_10 run the POOL twin, scene_10 under the sky the background twin"""
    width, height, spp = SHAPES[key]
    world, cam = _product(key)
    exp = _oracle_frame(key, width, height, spp, depth)
    img, st = _render(world, cam, "kernel2-lds", tuning, width=width, height=height, spp=spp, max_depth=depth, seed=SEED)
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    print("%s %dx%dx%d depth %d: kernel_ms %.3f, %d tiles for %d waves, non-zero pixels %.3f" %
          (key, width, height, spp, depth, st["kernel_ms"], tiles, _waves(st), float((exp != 0).any(axis=2).mean())))
    assert st["samples"] == width * height * spp
    assert tiles < _waves(st)
    _same(img, exp, "%s %dx%dx%d depth %d" % (key, width, height, spp, depth))


def test_depths_differ():
    """the three depths are three different frames (else depth 1 and 2 would add nothing to depth 50)"""
    for key, (width, height, spp) in SHAPES.items():
        a, b, c = (_oracle_frame(key, width, height, spp, d) for d in (1, 2, 50))
        assert not np.array_equal(b, c), key
        if key.endswith("_sky"):
            assert not np.array_equal(a, b), key


HW, HH, HSPP = 520, 516, 1


def test_whole_frame_kernel():
    """scene_500 with more tiles than the launch has waves: next_unit()'s kernel, the instantiation bench.py measures"""
    world, cam = _product("scene_500")
    img, st = world.render(cam, kernel=2, width=HW, height=HH, spp=HSPP, seed=SEED)
    _check_stats(st, "kernel2-lds")
    tiles = ((HW + 7) // 8) * ((HH + 7) // 8)
    print("scene_500 %dx%dx%d: kernel_ms %.3f, %d tiles for %d waves" % (HW, HH, HSPP, st["kernel_ms"], tiles, _waves(st)))
    if tiles < _waves(st):
        pytest.skip("this device has %d waves for %d tiles: the frame would run the POOL twin, not next_unit()" % (_waves(st), tiles))
    exp = _oracle_frame("scene_500", HW, HH, HSPP, 50)
    assert st["samples"] == HW * HH * HSPP
    _same(img, exp, "scene_500 %dx%dx%d" % (HW, HH, HSPP))


# ---- the other entry points that launch these variants ---------------------------------------------------------------------------------
def test_region_is_the_crop_of_the_frame(tuning):
    width, height, spp = SHAPES["scene_500"]
    world, cam = _product("scene_500")
    exp = _oracle_frame("scene_500", width, height, spp, 50)
    tuning(no_lds=0)
    x0, y0, x1, y1 = 11, 6, 64, 45  # (starts inside a tile, ends inside one)
    view, st = world.render_region(cam, (x0, y0, x1, y1), width=width, height=height, spp=spp, seed=SEED, kernel=2)
    _check_stats(st, "kernel2-lds")
    _same(view, exp[y0:y1, x0:x1], "region (%d, %d, %d, %d) of scene_500 %dx%dx%d" % (x0, y0, x1, y1, width, height, spp))


def test_adaptive_at_threshold_0_is_the_frame(tuning):
    """rt_render_adaptive with threshold 0 stops no tile early: its frame is rt_render's, here the oracle's"""
    width, height, spp = SHAPES["scene_500"]
    world, cam = _product("scene_500")
    exp = _oracle_frame("scene_500", width, height, spp, 50)
    tuning(no_lds=0)
    img, tile_spp, st = world.render_adaptive(cam, width, height, spp, min_spp=2, threshold=0.0, seed=SEED, kernel=2)
    _check_stats(st, "kernel2-lds")
    assert (tile_spp == spp).all() and st["launches"] >= 2, (np.unique(tile_spp), st["launches"])
    assert st["samples"] == width * height * spp
    _same(img, exp, "adaptive scene_500 %dx%dx%d" % (width, height, spp))


# ---- scenes built here: an exact tie, a leaf of four -------------------------------------------------------------------------------------
BW, BH, BSPP = 48, 32, 8
BUILT_CAM = ((0.0, 1.4, 6.0), (0.0, 0.8, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 10.0)
BACKGROUND = (0.7, 0.8, 1.0)


def _tie_spheres(B, swap=False):
    ground = B.Sphere((0.0, -1000.0, 0.0), 1000.0, B.Lambertian(B.ConstantTexture((0.5, 0.5, 0.5))))
    red = B.Sphere((0.0, 1.0, 0.0), 1.0, B.Lambertian(B.ConstantTexture((0.9, 0.1, 0.1))))
    mirror = B.Sphere((0.0, 1.0, 0.0), 1.0, B.Metal(B.ConstantTexture((0.2, 0.9, 0.2)), 0.0))  # the same sphere, another material
    left = B.Sphere((-2.2, 0.7, 0.3), 0.7, B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0))))
    right = B.Sphere((2.2, 0.7, -0.3), 0.7, B.Lambertian(B.ConstantTexture((0.2, 0.3, 0.8))))
    pair = [mirror, red] if swap else [red, mirror]
    return [ground] + pair + [left, right]


def _leaf4_spheres(B):
    ground = B.Sphere((0.0, -1000.0, 0.0), 1000.0, B.Lambertian(B.ConstantTexture((0.5, 0.5, 0.5))))
    lamp = B.Sphere((2.5, 3.0, 1.0), 0.7, B.DiffuseLight(B.ConstantTexture((5.0, 5.0, 5.0))))
    glass = lambda: B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0)))  # noqa: E731
    c = (0.0, 1.2, 0.0)
    shells = [B.Sphere(c, 1.2, glass()), B.Sphere(c, 0.9, glass()), B.Sphere(c, 0.6, glass()),
              B.Sphere(c, 0.3, B.Lambertian(B.ConstantTexture((0.8, 0.6, 0.2))))]
    return [ground, lamp] + shells


BUILT = {"tie": _tie_spheres, "leaf4": _leaf4_spheres}


@functools.lru_cache(maxsize=None)
def _built_product(name):
    import rtamd

    class Deferred(rtamd.World):  # new() leaves the scene uncommitted, so that the background can still be set
        def commit(self):
            return self
    w = Deferred()
    w.new(BUILT[name](w), bvh_seed=1)
    w.set_background(color=BACKGROUND)
    rtamd.World.commit(w)
    f, t, up, vfov, asp, ap, fd = BUILT_CAM
    return w, rtamd.Camera((f, t), up, vfov, asp, ap, fd)


def _built_oracle_frame(spheres):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    o = oracle.Scene()
    o.World(spheres(o), 1)
    o.set_background(1, color0=BACKGROUND)
    o.Camera(*BUILT_CAM)
    exp, cnt = o.render(BW, BH, BSPP, seed=SEED, n_workers=16)
    return _checked(exp, cnt, BW * BH * BSPP)


@functools.lru_cache(maxsize=None)
def _built_oracle(name):
    exp = _built_oracle_frame(BUILT[name])
    if name == "tie":
        # the order of the two coincident spheres decides what the frame shows: with the two swapped the other material wins the ties
        other = _built_oracle_frame(lambda B: _tie_spheres(B, swap=True))
        differ = int((other != exp).any(axis=2).sum())
        print("tie: %d / %d pixels differ between the two orders of the coincident spheres" % (differ, BW * BH))
        assert differ > BW * BH // 20, "the order of the coincident spheres changes too little: the case proves nothing about ties"
    return exp


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(BUILT))
def test_built_scene(name, form, tuning):
    world, cam = _built_product(name)
    info = world.info()
    if name == "leaf4":
        # four spheres with one centroid are never split and four items fit a leaf: 6 items under 2 inner nodes are the leaves
        # {four shells}, {ground}, {lamp}
        assert (info["accel_items"], info["accel_nodes"]) == (6, 2), info
    exp = _built_oracle(name)
    img, st = _render(world, cam, form, tuning, width=BW, height=BH, spp=BSPP, seed=SEED)
    print("%s %s: kernel_ms %.3f, accel items %d, inner nodes %d" % (name, form, st["kernel_ms"], info["accel_items"], info["accel_nodes"]))
    assert st["samples"] == BW * BH * BSPP
    _same(img, exp, "%s %dx%dx%d, %s" % (name, BW, BH, BSPP, form))


# ---- sqrt_hot: both paths of the ballot ---------------------------------------------------------------------------------------------------
EDGE = 2.0 ** -767  # the smallest operand of the core sequence
ODD = {
    "zero": 0.0, "minus_zero": -0.0, "denormal": 5e-324, "large_denormal": 2.0 ** -1030,
    "below_edge": np.nextafter(EDGE, 0.0), "edge": EDGE, "above_edge": np.nextafter(EDGE, 1.0),
    "inf": np.inf, "nan": np.nan, "minus_one": -1.0,
}


def _ordinary(n, seed):
    """operands of the kind the item step sees, and beyond: 2^-200 .. 2^200, plus exact squares"""
    rng = np.random.default_rng(seed)
    x = np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-200, 200, n))
    x[::7] = np.arange(len(x[::7]), dtype=np.float64) ** 2 + 1.0
    return x


def _bits_equal(got, exp, what):
    """bit for bit; where numpy's result is a NaN the device's must be one (the payload and sign of an invalid operation's NaN are the
    processor's own: x86 gives the negative default NaN, the GPU the positive one)"""
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), what
    a, b = got[~nan].view(np.uint64), exp[~nan].view(np.uint64)
    bad = np.argwhere(a != b)[:4].ravel()
    assert len(bad) == 0, "%s: %s" % (what, [(float(got[~nan][i]).hex(), float(exp[~nan][i]).hex()) for i in bad])


@pytest.mark.parametrize("op", [4, 0])
def test_sqrt_hot_all_lanes_in_range(op):
    """no lane outside the range: the core sequence runs (op 4); the range's ends included"""
    import rtamd
    x = _ordinary(64 * 8, 3)
    x[64:128:9] = EDGE
    x[128:192:5] = np.nextafter(EDGE, 1.0)
    x[192:256:3] = np.finfo(np.float64).max
    x[256:320] = np.ldexp(np.random.default_rng(4).uniform(0.5, 1.0, 64), -766)
    assert ((x >= EDGE) & (x < np.inf)).all()
    _bits_equal(rtamd.debug_math(op, x), np.sqrt(x), "op %d, all lanes in range" % op)


@pytest.mark.parametrize("op", [4, 0])
@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("name", list(ODD))
def test_sqrt_hot_one_odd_lane(name, lane, op):
    """one lane of a wave holds `name`, the others ordinary values; the waves before and behind it are all in range.  Only 2^-767 and
    its upper neighbour leave the wave on the core sequence: every other odd value sends it through sqrt()"""
    import rtamd
    x = _ordinary(64 * 3, 5)
    x[64 + lane] = ODD[name]
    outside = ~((x >= EDGE) & (x < np.inf))
    assert int(outside.sum()) == (0 if name in ("edge", "above_edge") else 1)
    with np.errstate(invalid="ignore"):
        exp = np.sqrt(x)
    _bits_equal(rtamd.debug_math(op, x), exp, "op %d, %s in lane %d" % (op, name, lane))
