"""Path state across the BVH walk of the LDS kernel (kernel 2, scene in LDS): whole frames against the oracle, bit for bit.

A lane of pt_kernel carries its path -- origin, direction, throughput, radiance, depth, random stream, pixel and ring slot -- through
the walk, through the shading behind it and through the regeneration of its neighbours; which registers hold that state, and how the
main loop's control flow hands it from one iteration to the next, is what DESIGN.md s5-r13 changed.  State that is lost or swapped on
any of those ways gives a wrong pixel somewhere in a frame, so every case compares every pixel:

  * scene_500, 520 x 516, 3 spp, depth 50: 65 x 65 = 4 225 tiles, no fewer than the waves of the launch, so the first-in-first-out
    fold of pt_kernel<true, 0, 2, 0, false, false> (the headline instantiation); 516 is no multiple of 8: a partial last row of tiles;
  * scene_500, 20 x 12, 17 spp: six tiles for all the waves, so the out-of-order twin <true, 0, 2, 0, false, true>; 17 samples run the
    tapered schedule's units of 8, 4, 2 and 1 samples, and lanes are regenerated while their neighbours are deep in a path;
  * the Cornell box at 520 x 516 x 3: <true, 1, 2, 0>, the general primitive set with the tie rule.

Which kernel ran is asserted from the call's stats (kernel_used, scene_in_lds) and from the tile count against the waves of the launch,
the rule render_tiles picks the twin by.  The oracle renders each frame once, on 16 threads."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 7
DEPTH = 50
# name: (configuration of tools/configs.py, width, height, spp, the out-of-order (POOL) twin?)
CASES = {
    "scene_500-fifo": ("scene_500", 520, 516, 3, False),
    "scene_500-pool": ("scene_500", 20, 12, 17, True),
    "cornell-fifo": ("cornell", 520, 516, 3, False),
}
# at least this fraction of the ORACLE frame's pixels is not black, so that the comparison is not of two empty frames (the oracle has
# 0.473 and 0.658 for the two scene_500 frames; 0.062 for the Cornell box, where a path lights its pixel only by reaching the lamp and
# 3 spp leave most pixels dark)
NONZERO_FLOOR = {"scene_500": 0.35, "cornell": 0.03}


def _same(got, exp, what):
    if np.array_equal(got, exp, equal_nan=True):
        return
    bad = ((got != exp) & ~(np.isnan(got) & np.isnan(exp))).any(axis=2)
    idx = np.argwhere(bad)[:4]
    lines = ["  (x=%d, y=%d) tile (%d, %d): hip=%s oracle=%s" % (x, y, x // 8, y // 8, got[y, x].tolist(), exp[y, x].tolist()) for y, x in idx]
    raise AssertionError("%s: %d / %d pixels differ, first:\n%s" % (what, int(bad.sum()), bad.size, "\n".join(lines)))


@pytest.mark.parametrize("name", list(CASES))
def test_whole_frame_keeps_its_path_state(name):
    import rtamd
    key, W, H, spp, pool = CASES[name]
    world, cam = configs.product(key)
    img, st = world.render(cam, width=W, height=H, spp=spp, max_depth=DEPTH, seed=SEED)
    tiles = rtamd.tiles_owned(rtamd.default_params(width=W, height=H, spp=spp))
    waves = st["grid_blocks"] * st["block_threads"] // 64
    print("%s: %d x %d x %d spp, tiles %d, waves %d, kernel_ms %.3f" % (name, W, H, spp, tiles, waves, st["kernel_ms"]))
    assert st["kernel_used"] == 2 and st["scene_in_lds"] == 1, st
    assert st["samples"] == W * H * spp
    assert tiles == ((W + 7) // 8) * ((H + 7) // 8)
    assert (tiles < waves) if pool else (tiles >= waves), (tiles, waves)
    assert H % 8 != 0  # a partial last row of tiles (520 = 65 x 8: the 520-wide frames have no partial column; 20 x 12 has both)
    exp, _ = configs.oracle_scene(key).render(W, H, spp, max_depth=DEPTH, seed=SEED, n_workers=16)
    nonzero = float((exp != 0).any(axis=2).mean())
    assert nonzero >= NONZERO_FLOOR[key], "%s: the oracle frame is only %.4f non-zero" % (name, nonzero)
    _same(img, exp, "%s %dx%dx%d" % (name, W, H, spp))
