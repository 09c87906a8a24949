"""The end of a path segment in pt_kernel and the hit of the LDS walk: whole frames against the oracle, bit for bit.

DESIGN.md s5-r14 changed where a lane keeps its state at the end of a segment -- the hit point is written into the ray's origin where
it is computed, shade() writes the scattered direction into the ray's direction, the throughput is updated under the branch that
scatters -- and how the LDS (WIDE) walk leaves its loop, so that the hit stays in one set of registers.  A value that is lost, or taken
from the wrong side of one of those joins, gives a wrong pixel, so every case compares every pixel of a frame:

  * scene_10 (spheres only: the headline instantiation's family) and the Cornell box (the general primitive set; a DiffuseLight, whose
    emitted term is not zero; walls on which paths end; a mesh under a Transform, so the walk enters and leaves an instance), 64 x 40,
    4 spp, at depths 1, 2 and 50 -- at depth 1 and 2 a path ends in the very iteration that also writes its next origin and direction;
  * five spheres built here: a Metal with fuzz 1.0 (it absorbs the reflections that point into it) next to a Lambertian one, a glass
    sphere, a small sphere light and a checker ground, under a constant background, 48 x 32, 8 spp.  On the oracle's side it is first
    shown that paths are absorbed and that paths leave the scene after a bounce -- otherwise the case would prove nothing.

Every frame goes through kernel 2 with the scene in LDS (the WIDE walk), kernel 2 with the scene forced out of LDS (the plain form of
the same walk) and kernel 1 (the reference-order walk), by the switches tests/test_walk_state_gpu.py and its neighbours use
(World.render's `kernel`, the `no_lds` tuning).  The oracle renders each frame once."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 7
W, H, SPP = 64, 40, 4
DEPTHS = (1, 2, 50)
# name: (World.render's kernel, the no_lds tuning, kernel_used and scene_in_lds of the call's stats)
FORMS = {
    "kernel2-lds": (2, 0, 2, 1),
    "kernel2-plain": (2, 1, 2, 0),
    "kernel1": (1, 0, 1, None),
}


def _same(got, exp, what):
    if np.array_equal(got, exp):
        return
    bad = (got != exp).any(axis=2)
    idx = np.argwhere(bad)[:4]
    lines = ["  (x=%d, y=%d): hip=%s oracle=%s" % (x, y, got[y, x].tolist(), exp[y, x].tolist()) for y, x in idx]
    raise AssertionError("%s: %d / %d pixels differ, first:\n%s" % (what, int(bad.sum()), bad.size, "\n".join(lines)))


def _render(world, cam, form, tuning, **kw):
    kernel, no_lds, used, lds = FORMS[form]
    tuning(no_lds=no_lds)
    img, st = world.render(cam, kernel=kernel, **kw)
    assert st["kernel_used"] == used, st
    if lds is not None:
        assert st["scene_in_lds"] == lds, st
    return img, st


# ---- scene_10 and the Cornell box ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_frame(key, depth):
    exp, _ = configs.oracle_scene(key).render(W, H, SPP, max_depth=depth, seed=SEED, n_workers=16)
    exp.setflags(write=False)
    return exp


@functools.lru_cache(maxsize=None)
def _product(key):
    return configs.product(key)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("key", ["scene_10", "cornell"])
def test_frame_at_depth(key, depth, form, tuning):
    world, cam = _product(key)
    exp = _oracle_frame(key, depth)
    img, st = _render(world, cam, form, tuning, width=W, height=H, spp=SPP, max_depth=depth, seed=SEED)
    print("%s depth %d %s: kernel_ms %.3f, non-zero pixels %.3f" % (key, depth, form, st["kernel_ms"], float((exp != 0).any(axis=2).mean())))
    assert st["samples"] == W * H * SPP
    if (key, depth) != ("scene_10", 1):
        # (scene_10's lights sit inside glass shells: no camera ray sees one directly, so at depth 1 -- one surface, then the path ends on
        # the next -- its frame is black, and has to be.  The Cornell box at depth 1 has the pixels that see the lamp.)
        assert (exp != 0).any(), "the oracle frame is black: nothing is compared"
    _same(img, exp, "%s %dx%dx%d depth %d, %s" % (key, W, H, SPP, depth, form))


def test_depth_cases_differ():
    """the three depths are three different frames (else depth 1 and 2 would add nothing to depth 50)"""
    for key in ("scene_10", "cornell"):
        a, b, c = (_oracle_frame(key, d) for d in DEPTHS)
        assert not np.array_equal(a, b) and not np.array_equal(b, c), key


# ---- five spheres: absorbed reflections, refraction, a checker, a light --------------------------------------------------------------
FW, FH, FSPP, FDEPTH = 48, 32, 8, 50
FIVE_CAM = ((0.0, 1.2, 5.0), (0.0, 0.6, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 10.0)
BACKGROUND = (0.7, 0.8, 1.0)


def _five_spheres(B):
    ground = B.Sphere((0.0, -1000.0, 0.0), 1000.0, B.Lambertian(B.CheckerTexture(B.ConstantTexture((0.2, 0.3, 0.1)), B.ConstantTexture((0.9, 0.9, 0.9)))))
    matte = B.Sphere((-0.55, 0.5, 0.0), 0.5, B.Lambertian(B.ConstantTexture((0.7, 0.3, 0.3))))
    rough = B.Sphere((0.55, 0.5, 0.0), 0.5, B.Metal(B.ConstantTexture((0.8, 0.8, 0.6)), 1.0))
    glass = B.Sphere((0.0, 0.4, 1.4), 0.4, B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0))))
    lamp = B.Sphere((0.0, 3.5, 0.0), 0.6, B.DiffuseLight(B.ConstantTexture((4.0, 4.0, 4.0))))
    return [ground, matte, rough, glass, lamp]


@functools.lru_cache(maxsize=None)
def _five_pair():
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
    o.Camera(*FIVE_CAM)
    f, t, up, vfov, asp, ap, fd = FIVE_CAM
    return w, rtamd.Camera((f, t), up, vfov, asp, ap, fd), o


@functools.lru_cache(maxsize=None)
def _five_oracle():
    """the oracle's frame, after showing on its side that paths of this frame are absorbed and that paths leave the scene"""
    _, _, o = _five_pair()
    # Sample 0 of every pixel on its own (the stream of a path is keyed by seed, pixel and sample index: these are paths of the frame
    # below).  The background and the lamp are positive and no albedo is zero, so a path that reaches either leaves its pixel non-zero;
    # a black pixel's path ended on a surface -- absorbed, or out of depth.  Out of depth takes max_depth + 1 segments; the counters of
    # that one path, rendered alone, say how many it had.
    first, _ = o.render(FW, FH, 1, max_depth=FDEPTH, seed=SEED, n_workers=16)
    black = np.argwhere(~(first != 0).any(axis=2))
    absorbed = 0
    for y, x in black[:8]:
        one, cnt = o.render(FW, FH, 1, max_depth=FDEPTH, seed=SEED, window=(int(x), int(y), int(x) + 1, int(y) + 1), n_workers=1)
        assert not (one != 0).any() and cnt["n_samples"] == 1, (x, y, cnt)
        assert 1 <= cnt["n_segments"] <= FDEPTH, (x, y, cnt)  # (it did not run out of depth; a miss would have lit the pixel)
        absorbed += 1
    assert absorbed >= 1, "no path of the oracle's frame is absorbed: the case proves nothing"
    exp, cnt = o.render(FW, FH, FSPP, max_depth=FDEPTH, seed=SEED, n_workers=16)
    left = o.light_counters()["n_miss_after_bounce"]
    assert left >= 1, "no path of the oracle's frame leaves the scene after a bounce: the case proves nothing"
    assert cnt["n_samples"] == FW * FH * FSPP
    print("five spheres: %d black first-sample pixels (%d checked: absorbed), %d paths left the scene after a bounce" % (len(black), absorbed, left))
    exp.setflags(write=False)
    return exp


@pytest.mark.parametrize("form", list(FORMS))
def test_five_spheres(form, tuning):
    world, cam, _ = _five_pair()
    exp = _five_oracle()
    img, st = _render(world, cam, form, tuning, width=FW, height=FH, spp=FSPP, max_depth=FDEPTH, seed=SEED)
    print("five spheres %s: kernel_ms %.3f" % (form, st["kernel_ms"]))
    assert st["samples"] == FW * FH * FSPP
    _same(img, exp, "five spheres %dx%dx%d, %s" % (FW, FH, FSPP, form))
