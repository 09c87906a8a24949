"""START walks: the sphere-only LDS variants of pt_kernel begin every closest-hit walk where csrc/common/walk_start.h
says -- at the root's dominant leaf child with the other child pushed, or at the root.  Only the order of visits changes, so every frame
and every hit record must be the oracle's bit for bit.  What can go wrong: the staged words (a wrong ref, a ref of the wrong table), the
first trip through the loop with no inner node and one entry on the stack, the rows a column needs, a pushed ref that is itself a leaf,
and an exact tie with the start leaf as one party.

  * frames of scene_10 and of the built scenes of tests/walk_start_scenes.py (tests/test_walk_start.py shows what the rule does with each:
    a ground leaf picked, a leaf child not picked, two leaves, the one-item BVH) at depths 1, 2 and 50 -- from depth 2 on, rays start on
    the ground sphere, at the t_min edge.  64 x 36 at 16 spp has fewer tiles than the launch has waves and runs the POOL twin; the
    whole-frame kernel (next_unit(), the instantiation bench.py measures) is chosen only for a frame with at least as many tiles as
    waves, so the same scenes run through it at 520 x 516 (4 225 tiles), 1 spp;
  * the ground sphere with a coincident twin of another material, listed before it and after it: every hit of the start leaf is an exact
    tie, the later one in reference order wins, and the two orders give different frames;
  * the picked scene under a sky (the background twin), as a pixel region, as an adaptive render, and as rank 1 of 3's tiles;
  * 4 096 explicit rays through rt_debug_hit_device's mode 8 -- mode 3, the LDS form of the walk, as a START walk -- against the oracle's
    hit_batch: origins inside the ground sphere, on it, below it and far outside the root's box, directions that miss everything among them.

The oracle renders each frame once; its frames are checked to be finite and, where the scene is lit, not black."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path
import walk_start_scenes as wss

pytestmark = pytest.mark.gpu

SEED = 7
PW, PH, PSPP = 64, 36, 16     # fewer tiles than waves: the POOL twin
FW, FH, FSPP = 520, 516, 1    # more tiles than waves: the whole-frame kernel
SKY = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))
FRAME_SCENES = ["scene_10", "five", "five_small", "two", "one"]


def _same(got, exp, what):
    if np.array_equal(got, exp):
        return
    bad = (got != exp).any(axis=-1)
    idx = np.argwhere(bad)[:4]
    lines = ["  %s: hip=%s oracle=%s" % (tuple(int(v) for v in i), got[tuple(i)].tolist(), exp[tuple(i)].tolist()) for i in idx]
    raise AssertionError("%s: %d / %d pixels differ, first (index):\n%s" % (what, int(bad.sum()), bad.size, "\n".join(lines)))


def _waves(st):
    return st["grid_blocks"] * st["block_threads"] // 64


def _tiles(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


@functools.lru_cache(maxsize=None)
def _product(name, sky=False):
    import rtamd
    if name == "scene_10":
        w, cam = rtamd.load_scene_file(scene_path("scene_10.json"), commit=False)
        cam = cam.with_aspect(16.0 / 9.0)
    else:
        class Deferred(rtamd.World):  # new() leaves the scene uncommitted, so that the background can still be set
            def commit(self):
                return self
        w = Deferred()
        w.new(wss.build(w, name), bvh_seed=1)
        f, t, up, vfov, asp, ap, fd = wss.CAM
        cam = rtamd.Camera((f, t), up, vfov, asp, ap, fd)
    if sky:
        w.set_background(gradient=SKY)
    rtamd.World.commit(w)
    return w, cam


@functools.lru_cache(maxsize=None)
def _oracle(name, sky=False):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    if name == "scene_10":
        o = oracle.load_scene_file(scene_path("scene_10.json"), aspect=16.0 / 9.0)
    else:
        o = oracle.Scene()
        o.World(wss.build(o, name), 1)
        o.Camera(*wss.CAM)
    if sky:
        o.set_background(2, color0=SKY[0], color1=SKY[1])
    return o


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, width, height, spp, depth, sky=False):
    exp, cnt = _oracle(name, sky).render(width, height, spp, max_depth=depth, seed=SEED, n_workers=16)
    assert cnt["n_samples"] == width * height * spp, cnt
    assert np.isfinite(exp).all(), "the oracle frame holds a NaN or an infinity"
    # (scene_10's lights sit inside glass shells: without a background its paths see no light within one or two surfaces; the lamp of the
    # five-sphere scenes is out of the camera's view: at depth 1 their frames are black)
    if sky or depth >= 50 or name in ("two", "one") or (name != "scene_10" and depth >= 2):
        assert (exp != 0).any(), "the oracle frame is black: nothing is compared"
    exp.setflags(write=False)
    return exp


def _frame(name, width, height, spp, depth, pool):
    world, cam = _product(name)
    exp = _oracle_frame(name, width, height, spp, depth)
    img, st = world.render(cam, kernel=2, width=width, height=height, spp=spp, max_depth=depth, seed=SEED)
    print("%s %dx%dx%d depth %d: kernel_ms %.3f, %d tiles for %d waves, non-zero pixels %.3f" %
          (name, width, height, spp, depth, st["kernel_ms"], _tiles(width, height), _waves(st), float((exp != 0).any(axis=2).mean())))
    assert st["kernel_used"] == 2 and st["scene_in_lds"] == 1 and st["samples"] == width * height * spp, st
    assert (_tiles(width, height) < _waves(st)) == pool, "the frame ran the other twin: %d tiles, %d waves" % (_tiles(width, height), _waves(st))
    _same(img, exp, "%s %dx%dx%d depth %d" % (name, width, height, spp, depth))


@pytest.mark.parametrize("depth", [1, 2, 50])
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_pool_twin(name, depth):
    _frame(name, PW, PH, PSPP, depth, pool=True)


@pytest.mark.parametrize("depth", [1, 2, 50])
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_whole_frame_kernel(name, depth):
    _frame(name, FW, FH, FSPP, depth, pool=False)


def test_depths_differ():
    """the three depths are three different frames (else depths 1 and 2 would add nothing to depth 50)"""
    for name in FRAME_SCENES:
        a, b, c = (_oracle_frame(name, PW, PH, PSPP, d) for d in (1, 2, 50))
        if name != "one":  # (a lone light: every path ends on it or misses)
            assert not np.array_equal(b, c), name
        if name not in ("scene_10", "one"):
            assert not np.array_equal(a, b), name


@pytest.mark.parametrize("size", ["pool", "whole_frame"])
def test_exact_tie_with_the_start_leaf(size):
    """the ground sphere and its coincident twin share the start leaf; whichever comes later in reference order wins every hit of it"""
    width, height, spp = (PW, PH, PSPP) if size == "pool" else (FW, FH, FSPP)
    before, after = (_oracle_frame(n, width, height, spp, 50) for n in ("tie_before", "tie_after"))
    differ = int((before != after).any(axis=2).sum())
    print("tie: %d / %d pixels differ between the two orders of the coincident spheres" % (differ, width * height))
    assert differ > width * height // 50, "the order of the coincident spheres changes too little: the case proves nothing about ties"
    for name in ("tie_before", "tie_after"):
        _frame(name, width, height, spp, 50, pool=size == "pool")


def test_background_twin():
    world, cam = _product("five", True)
    exp = _oracle_frame("five", PW, PH, PSPP, 50, True)
    img, st = world.render(cam, kernel=2, width=PW, height=PH, spp=PSPP, seed=SEED)
    assert st["kernel_used"] == 2 and st["scene_in_lds"] == 1, st
    _same(img, exp, "five under a sky")


def test_region_is_the_crop_of_the_frame():
    world, cam = _product("five")
    exp = _oracle_frame("five", PW, PH, PSPP, 50)
    x0, y0, x1, y1 = 11, 6, 61, 33  # (starts inside a tile, ends inside one)
    view, st = world.render_region(cam, (x0, y0, x1, y1), width=PW, height=PH, spp=PSPP, seed=SEED, kernel=2)
    assert st["kernel_used"] == 2 and st["scene_in_lds"] == 1, st
    _same(view, exp[y0:y1, x0:x1], "region (%d, %d, %d, %d) of five" % (x0, y0, x1, y1))


def test_adaptive_at_threshold_0_is_the_frame():
    """rt_render_adaptive with threshold 0 stops no tile early: its frame is rt_render's, here the oracle's"""
    world, cam = _product("five")
    exp = _oracle_frame("five", PW, PH, PSPP, 50)
    img, tile_spp, st = world.render_adaptive(cam, PW, PH, PSPP, min_spp=2, threshold=0.0, seed=SEED, kernel=2)
    assert st["kernel_used"] == 2 and st["scene_in_lds"] == 1, st
    assert (tile_spp == PSPP).all() and st["launches"] >= 2, (np.unique(tile_spp), st["launches"])
    _same(img, exp, "adaptive five")


def test_rank_1_of_3():
    """a rank's frame holds its own tiles and zeros: under the sky no pixel of the frame is black, so an 8 x 8 tile is either the oracle's or zero"""
    world, cam = _product("five", True)
    exp = _oracle_frame("five", PW, PH, PSPP, 50, True)
    assert (exp != 0).any(axis=2).all()
    part, st = world.render(cam, kernel=2, width=PW, height=PH, spp=PSPP, seed=SEED, rank=1, world=3)
    assert st["kernel_used"] == 2 and st["scene_in_lds"] == 1, st
    owned = 0
    for ty in range(0, PH, 8):
        for tx in range(0, PW, 8):
            tile, ref = part[ty:ty + 8, tx:tx + 8], exp[ty:ty + 8, tx:tx + 8]
            if (tile != 0).any():
                owned += 1
                _same(tile, ref, "rank 1 of 3, tile (%d, %d)" % (tx // 8, ty // 8))
    n = _tiles(PW, PH)
    assert n // 3 <= owned <= n // 3 + 1, (owned, n)


def _rays():
    """4 096 rays in eight groups of 512: origins inside the ground sphere (near its centre; just under its top), on it (centre + 1000 u,
    rounded), below it, far outside the root's box, and above the ground among the small spheres; each group aims a third of its rays at
    the small spheres, a third anywhere, and a third away from the scene (from outside: they miss everything)"""
    rng = np.random.default_rng(29)
    n, g = 4096, 512
    c, r = np.array(wss.GROUND[0]), wss.GROUND[1]
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = np.zeros((n, 3))
    o[0 * g:1 * g] = c + 300.0 * u[0 * g:1 * g] * rng.uniform(0.0, 1.0, (g, 1))               # inside, near the centre
    o[1 * g:2 * g] = np.column_stack([rng.uniform(-3, 3, g), -rng.uniform(1e-6, 0.5, g), rng.uniform(-3, 3, g)])  # inside, just under the top
    o[2 * g:3 * g] = c + r * u[2 * g:3 * g]                                                    # on the sphere, anywhere
    top = np.column_stack([rng.uniform(-4, 4, g), np.zeros(g), rng.uniform(-4, 4, g)])
    top[:, 1] = np.sqrt(r * r - top[:, 0] ** 2 - top[:, 2] ** 2) - r                           # on the sphere, under the small ones
    o[3 * g:4 * g] = top
    o[4 * g:5 * g] = c + (1.5 * r + rng.uniform(0, r, (g, 1))) * u[4 * g:5 * g] * (1, 0.2, 1) - (0, 2.5 * r, 0)  # below it
    o[5 * g:6 * g] = 1e5 * u[5 * g:6 * g]                                                      # far outside the root's box
    o[6 * g:7 * g] = np.column_stack([rng.uniform(-4, 4, g), rng.uniform(0.01, 4, g), rng.uniform(-4, 4, g)])    # among the small spheres
    o[7 * g:8 * g] = np.array(wss.CAM[0]) + rng.normal(0, 0.2, (g, 3))                         # the camera's place
    small = np.array([s[0] for s in wss.SCENES["five"][1:]])
    d = np.zeros((n, 3))
    for i in range(n):
        k = i % 3
        if k == 0:
            d[i] = small[rng.integers(0, len(small))] + rng.normal(0, 0.4, 3) - o[i]
        elif k == 1:
            d[i] = rng.normal(size=3)
        else:  # away from everything: from the origin's side of the scene outwards
            out = o[i] - (0.0, -500.0, 0.0)
            d[i] = out / max(np.linalg.norm(out), 1e-9) + rng.normal(0, 0.05, 3)
    return np.column_stack([o, d])


def test_explicit_rays_through_the_start_walk():
    import rtamd
    world, _ = _product("five")
    rays = _rays()
    exp = _oracle("five").hit_batch(rays, t_min=1e-3, n_workers=16)
    hit = exp[:, 0] == 1.0
    print("hits per group of 512:", [int(hit[k * 512:(k + 1) * 512].sum()) for k in range(8)])
    # the cases are there: rays that miss everything (from outside, aimed away), rays from inside that can only hit the ground sphere from within
    away = np.arange(len(rays)) % 3 == 2  # (_rays: every third ray is aimed away from the scene)
    far = slice(5 * 512, 6 * 512)
    assert away[far].sum() > 150 and hit[far][away[far]].sum() == 0 and (~hit).sum() > 400
    assert hit[0:512].all() and hit.sum() > 2000
    ref = world.debug_hit(rays, t_min=1e-3, kernel=1)
    assert np.array_equal(ref[:, :11], exp[:, :11], equal_nan=True), "kernel 1 differs from the oracle in %d rows" % int((ref[:, :11] != exp[:, :11]).any(axis=1).sum())
    for mode in (8, 3):
        got = world.debug_hit(rays, t_min=1e-3, kernel=mode)
        bad = (got != ref).any(axis=1)
        assert not bad.any(), "mode %d differs from kernel 1 in %d rows, first %s" % (mode, int(bad.sum()), np.argwhere(bad)[:4].ravel().tolist())
    # the scenes the rule leaves alone, the two-leaf root and the tie walk through mode 8 as well (kernel 1 is the reference order)
    for name in ("five_small", "two", "one", "tie_before", "tie_after"):
        w, _ = _product(name)
        a, b = w.debug_hit(rays, t_min=1e-3, kernel=1), w.debug_hit(rays, t_min=1e-3, kernel=8)
        assert np.array_equal(a, b, equal_nan=True), "%s: mode 8 differs from kernel 1 in %d rows" % (name, int((a != b).any(axis=1).sum()))
    with pytest.raises(rtamd.RtError):
        world.debug_hit(rays[:4], t_min=1e-3, kernel=4)
