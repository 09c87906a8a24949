"""Whole frames and full-resolution closest-hit maps of every BASELINE configuration (tools/configs.py) against the oracle, bit for
bit, through every kernel that applies.  The windows of test_golden.py / test_book2.py compare a few hundred pixels at full spp; these
compare every pixel at a low spp, and every pixel's camera ray and one secondary ray from its hit point as closest-hit records, so
that a wrong pixel, tile, RNG key or missed primitive anywhere in the frame fails.  Each oracle frame / hit map is computed once per
module (fixture `oracle_cache`), compared with every kernel, and dropped after the configuration's last kernel."""
import os
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu

# key: (spp, floor on the oracle frame's non-zero-pixel fraction, kernel the automatic choice picks, explicit kernels)
# floors: measured fraction minus a margin (C1 0.205, C2 0.403, headline 0.433, C3 0.371 / 0.532, C4 0.024, C5 reduced and as named 0.106), so that a change
# which turns most of a frame black -- and the comparison vacuous -- fails here
FRAMES = {
    "scene_10": (100, 0.15, 2, (1, 2)),
    "scene_500_c2": (2, 0.35, 2, (1, 2)),
    "scene_500": (2, 0.38, 2, (1, 2)),
    "cornell": (32, 0.32, 2, (1, 2)),
    "cornell_mix": (8, 0.47, 2, (1, 2)),
    "c4": (1, 0.018, 5, (1, 2, 5, 6)),
    "c5r": (2, 0.08, 2, (1, 2)),
    "c5": (2, 0.08, 2, (1, 2)),
}
# the configurations without media (closest-hit queries need no random stream) and the traversals they are compared through:
# 3 = kernel 2's LDS node table, used where the scene is LDS-resident; 5 / 6 = the instance walks of the cooperative kernels.
# (cornell_mix is the cornell scene: the same hit map.)
# Second number: floor on the fraction of primary hits whose secondary ray hits too (measured: C1 0.050 -- most of them leave the
# ground for the sky --, C2 0.409, headline 0.437, C3 0.788 -- the box is open towards the camera --, C4 0.814).
HIT_KERNELS = {
    "scene_10": ((1, 2, 3), 0.03),
    "scene_500_c2": ((1, 2, 3), 0.3),
    "scene_500": ((1, 2, 3), 0.3),
    "cornell": ((1, 2, 3), 0.6),
    "c4": ((1, 2, 5, 6), 0.6),
}
T_MIN = 1e-3


class _Cache:
    def __init__(self):
        self.oracle, self.product, self.frames, self.hit_maps = {}, {}, {}, {}

    def scene(self, key):
        if key not in self.oracle:
            self.oracle[key] = configs.oracle_scene(key)
        return self.oracle[key]

    def world(self, key):
        if key not in self.product:
            self.product[key] = configs.product(key)
        return self.product[key]

    def frame(self, key):
        """the oracle's whole frame at the configuration's own W x H and FRAMES' spp"""
        if key not in self.frames:
            _, W, H, _, _ = configs.CONFIGS[key]
            img, _ = self.scene(key).render(W, H, FRAMES[key][0], seed=1, n_jobs=max(64, H // 4), integrator=configs.INTEGRATOR.get(key, 0))
            self.frames[key] = img
        return self.frames[key]

    def hits(self, key):
        """-> (primary rays [H, W, 6], their oracle records [H, W, 12], secondary rays [H, W, 6] (NaN where the primary missed),
        their oracle records [H, W, 12] (zero there))"""
        if key not in self.hit_maps:
            _, W, H, _, _ = configs.CONFIGS[key]
            sc = self.scene(key)
            rays = sc.camera_rays(W, H, seed=1, sample=0)
            rec = sc.hit_batch(rays.reshape(-1, 6), t_min=T_MIN).reshape(H, W, 12)
            sec = _secondary_rays(rays, rec, seed=zlib.crc32(key.encode()))
            hit = ~np.isnan(sec[..., 0])
            rec2 = np.zeros((H, W, 12))
            rec2[hit] = sc.hit_batch(sec[hit], t_min=T_MIN)
            self.hit_maps[key] = (rays, rec, sec, rec2)
        return self.hit_maps[key]


@pytest.fixture(scope="module")
def oracle_cache():
    return _Cache()


def _secondary_rays(rays, rec, seed):
    """one ray from every primary hit point p: a uniform direction in the hemisphere of the record's normal for even pixels (x + y
    even), the mirror reflection of the primary direction for odd pixels.  NaN rows where the primary ray missed."""
    H, W, _ = rays.shape
    rng = np.random.default_rng(seed)
    n = rec[..., 5:8]
    u = rng.normal(size=(H, W, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    u = np.where((np.sum(u * n, axis=2) < 0.0)[..., None], -u, u)
    d = rays[..., 3:]
    m = d - 2.0 * np.sum(d * n, axis=2, keepdims=True) * n
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.concatenate([rec[..., 2:5], np.where(((xx + yy) % 2 == 0)[..., None], u, m)], axis=2)
    out[rec[..., 0] != 1.0] = np.nan
    return out


def _assert_same(got, exp, what):
    """got / exp: [H, W, k]; bit for bit, NaN == NaN.  The message gives the count of differing pixels and the first few with
    their (x, y), 8 x 8 tile and both values."""
    if np.array_equal(got, exp, equal_nan=True):
        return
    bad = ((got != exp) & ~(np.isnan(got) & np.isnan(exp))).any(axis=2)
    idx = np.argwhere(bad)[:4]
    lines = ["  (x=%d, y=%d) tile (%d, %d): hip=%s oracle=%s" % (x, y, x // 8, y // 8, got[y, x].tolist(), exp[y, x].tolist()) for y, x in idx]
    raise AssertionError("%s: %d / %d pixels differ, first:\n%s" % (what, int(bad.sum()), bad.size, "\n".join(lines)))


@pytest.mark.parametrize("key,kernel", [(k, kn) for k, v in FRAMES.items() for kn in (0,) + v[3]])
def test_whole_frame_matches_the_oracle(oracle_cache, key, kernel):
    """every pixel of the configuration's frame at its own W x H (integrator and shutter as BASELINE names them), the automatic kernel
    pinned to what it picks, and every explicit kernel, against the oracle's whole frame"""
    spp, floor, auto, _ = FRAMES[key]
    _, W, H, _, _ = configs.CONFIGS[key]
    exp = oracle_cache.frame(key)
    nonzero = float((exp != 0).any(axis=2).mean())
    assert nonzero >= floor, "%s: the oracle frame is only %.4f non-zero" % (key, nonzero)
    if kernel == FRAMES[key][3][-1]:  # the key's last test (the parametrisation groups them): free the frame
        del oracle_cache.frames[key]
    world, cam = oracle_cache.world(key)
    img, st = world.render(cam, width=W, height=H, spp=spp, seed=1, kernel=kernel, integrator=configs.INTEGRATOR.get(key, 0),
                           shutter=configs.SHUTTER.get(key, (0.0, 0.0)))
    assert st["kernel_used"] == (auto if kernel == 0 else kernel) and st["samples"] == W * H * spp
    _assert_same(img, exp, "%s %dx%dx%d kernel %d" % (key, W, H, spp, kernel))


def _debug_hit(world, rays, kernel):
    H, W, _ = rays.shape
    flat = rays.reshape(-1, 6)
    ok = ~np.isnan(flat[:, 0])
    out = np.zeros((H * W, 12))
    out[ok] = world.debug_hit(flat[ok], t_min=T_MIN, kernel=kernel)
    return out.reshape(H, W, 12)


@pytest.mark.parametrize("key,kernel", [(k, kn) for k, v in HIT_KERNELS.items() for kn in v[0]])
def test_full_resolution_hit_map_matches_the_oracle(oracle_cache, key, kernel):
    """the closest-hit record of every pixel's sample-0 camera ray (the oracle's camera_rays, t_min 1e-3), then of one secondary ray
    from each hit point (uniform in the normal's hemisphere for even pixels, the mirror reflection for odd ones: rays that start on a
    surface, where the t_min edge and near ties between abutting or coplanar faces -- Cornell walls, cube sides, mesh triangles --
    occur), through World.debug_hit: fields 0-10 {hit, t, p, normal, front_face, u, v} bit for bit (sphere uv goes through
    rtamd-acos-1 / rtamd-atan2-1 on both sides).  Field 11 is left out: the oracle's prim_id is the primitive's index
    among all of its hitables in builder order (lists, BVH nodes, meshes and transforms counted too), the product's is the leaf index
    in its flattened reference-order program; no exact mapping between the two is exposed to compare through."""
    rays, rec, sec, rec2 = oracle_cache.hits(key)
    if kernel == HIT_KERNELS[key][0][-1]:  # the key's last test (the parametrisation groups them): free the map (288 bytes a pixel)
        del oracle_cache.hit_maps[key]
    H, W, _ = rays.shape
    world, _ = oracle_cache.world(key)
    assert rec[..., 0].mean() > 0.5, "%s: primary hit fraction %.3f" % (key, rec[..., 0].mean())
    _assert_same(_debug_hit(world, rays, kernel)[..., :11], rec[..., :11], "%s %dx%d primary hits, kernel %d" % (key, W, H, kernel))
    frac = rec2[..., 0].sum() / rec[..., 0].sum()
    assert frac >= HIT_KERNELS[key][1], "%s: secondary hit fraction %.3f" % (key, frac)
    _assert_same(_debug_hit(world, sec, kernel)[..., :11], rec2[..., :11], "%s %dx%d secondary hits (pixel of origin), kernel %d" % (key, W, H, kernel))
