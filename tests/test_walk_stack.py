"""The BVH2 walk's stack (traverse2, csrc/device/kernels.hip "The stack"): in the LDS (WIDE) form row 0 of a lane's column holds REF_DONE and
every pop is unconditional; the plain form keeps its emptiness test.  Exact comparisons on the trees where that can go wrong: the smallest ones (the first pop meets the sentinel), the
deepest one (a row too many lands in the ring bookkeeping behind the stacks), the plain and the LDS (WIDE) form of the walk, restore
markers of instances, and one small frame each through the other users of the walk (the media walks, kernels 5 / 6).  rt_debug_hit_device: kernel 1 is the
reference-order program, 2 the plain form of the walk, 3 the LDS form; the oracle's records are compared in fields 0-10 (its prim_id
counts other things than the product's, test_full_frames_gpu)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu

T_MIN = 1e-3


def _sphere_scene(spheres, cam_args, bvh_seed=1):
    """spheres: [(centre, radius)] -> (rtamd.World, rtamd.Camera, oracle.Scene)"""
    import oracle
    import rtamd
    out = []
    for B in (rtamd.World(), oracle.Scene()):
        mats = [B.DiffuseLight(B.ConstantTexture((4.0, 4.0, 4.0))), B.Lambertian(B.ConstantTexture((0.8, 0.3, 0.2))),
                B.Metal(B.ConstantTexture((0.7, 0.7, 0.9)), 0.1)]
        ids = [B.Sphere(tuple(float(v) for v in c), float(r), mats[i % 3]) for i, (c, r) in enumerate(spheres)]
        if isinstance(B, rtamd.World):
            B.new(ids, bvh_seed=bvh_seed)
        else:
            B.World(ids, bvh_seed)
            B.Camera(*cam_args)
        out.append(B)
    f, t, up, vfov, asp, ap, fd = cam_args
    return out[0], rtamd.Camera((f, t), up, vfov, asp, ap, fd), out[1]


def _check_hits(world, ref, rays, what):
    """the records of the walk's two forms equal the reference-order program's in every field, and the oracle's in fields 0-10"""
    exp = ref.hit_batch(rays, t_min=T_MIN, n_workers=4)
    a = world.debug_hit(rays, t_min=T_MIN, kernel=1)
    assert np.array_equal(a[:, :11], exp[:, :11], equal_nan=True), "%s: kernel 1 differs from the oracle in %d rows" % (
        what, int((a[:, :11] != exp[:, :11]).any(axis=1).sum()))
    for k in (2, 3):
        b = world.debug_hit(rays, t_min=T_MIN, kernel=k)
        assert np.array_equal(a, b, equal_nan=True), "%s: kernel %d differs from kernel 1 in %d rows" % (what, k, int((a != b).any(axis=1).sum()))
    return exp


def _same_frames(world, cam, what, kernels=(0,), **kw):
    """64 x 64 x 4 spp: each of `kernels` equals kernel 1 bit for bit, and a second identical render equals the first"""
    exp, _ = world.render(cam, width=64, height=64, spp=4, seed=1, kernel=1, **kw)
    assert (exp != 0).any(), what
    used = []
    for k in kernels:
        img, st = world.render(cam, width=64, height=64, spp=4, seed=1, kernel=k, **kw)
        assert np.array_equal(img, exp, equal_nan=True), "%s: kernel %d differs from kernel 1 in %d pixels" % (
            what, k, int(((img != exp) & ~(np.isnan(img) & np.isnan(exp))).any(axis=2).sum()))
        again, _ = world.render(cam, width=64, height=64, spp=4, seed=1, kernel=k, **kw)
        assert np.array_equal(again, img, equal_nan=True), "%s: kernel %d is not repeatable" % (what, k)
        used.append((st["kernel_used"], st["scene_in_lds"]))
    return used


SMALL = {
    1: [((0.0, 0.0, 0.0), 1.0)],
    2: [((-1.5, 0.0, 0.0), 1.0), ((1.5, 0.0, 0.5), 1.2)],
    3: [((-1.5, 0.0, 0.0), 1.0), ((1.5, 0.0, 0.5), 1.2), ((0.0, 0.3, 4.0), 2.0)],
}
SMALL_CAM = ((0.0, 0.5, -9.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 9.0)


def _small_rays(spheres):
    """256 rays from in front of the scene: a third aimed far off (they miss everything), a third at one sphere's centre or rim (one
    child), a third along the line through two spheres (both children) or, the two being the same, through the low corner of that
    sphere's box and on to the sphere (the one-item BVH's second child is a zero-size box there)"""
    rng = np.random.default_rng(17)
    rays = np.zeros((256, 6))
    rays[:, :3] = (0.0, 0.5, -9.0) + rng.normal(0.0, 0.3, (256, 3))
    c = np.array([s[0] for s in spheres])
    r = np.array([s[1] for s in spheres])
    for i in range(256):
        j = int(rng.integers(0, len(spheres)))
        if i % 3 == 0:
            tgt = np.array([40.0, 30.0, 0.0]) * rng.choice([-1.0, 1.0], 3) + rng.normal(0.0, 3.0, 3)
        elif i % 3 == 1:
            tgt = c[j] + rng.normal(0.0, 0.6, 3) * r[j]
        else:
            k = int(rng.integers(0, len(spheres)))
            if k != j:
                rays[i, :3] = c[j] + (c[j] - c[k]) * 3.0 + rng.normal(0.0, 0.05, 3)
                tgt = c[k]
            else:  # through the low corner of the sphere's box (the one-item BVH's zero-size second box) towards the centre
                rays[i, :3] = c[j] - 3.0 * r[j] + rng.normal(0.0, 0.02, 3)
                tgt = c[j] - r[j]
        rays[i, 3:] = tgt - rays[i, :3]
    return rays


@pytest.mark.parametrize("n", [1, 2, 3])
def test_smallest_trees(n, tuning):
    """1, 2 and 3 spheres: the one-item BVH is the node whose two children are the same leaf, the root of the others a forced split"""
    world, cam, ref = _sphere_scene(SMALL[n], SMALL_CAM)
    info = world.info()
    assert info["accel_ok"] == 1 and info["accel_items"] == n and info["accel_nodes"] == max(1, n - 1)
    rays = _small_rays(SMALL[n])
    exp = _check_hits(world, ref, rays, "%d spheres" % n)
    hit = exp[:, 0] == 1.0
    assert hit[0::3].sum() == 0 and hit[1::3].mean() > 0.5 and hit[2::3].mean() > 0.5, (hit[0::3].sum(), hit[1::3].mean(), hit[2::3].mean())
    # the frame: the automatic kernel is the sphere-only LDS variant, then the same scene outside LDS
    assert _same_frames(world, cam, "%d spheres" % n) == [(2, 1)]
    tuning(no_lds=1)
    assert _same_frames(world, cam, "%d spheres outside LDS" % n) == [(2, 0)]


CHAIN_N, CHAIN_R0 = 30, 1e-10
CHAIN_CAM = ((-3.0, 0.02, 0.01), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 30.0, 1.0, 0.0, 3.0)


def _chain():
    """30 spheres on the x axis, each touching its predecessor and max(2, sqrt(n)) times its size, n being its number in the row.
    accel.cpp's binned SAH takes the largest sphere alone off a range of n only when no other cut is cheaper, and peeling j of them
    costs about (n - j) * growth^(-2 j) + j: with a uniform growth of 1.5, 48 spheres give a depth of 16 only, and a uniform growth
    that would do (7) overruns the accel's coordinate limit of 2^36 / 64.  The result here is a maximally unbalanced tree, depth 29,
    whose boxes all contain the axis; radii from 1e-10 to 1e7, all far above the rounding of a hit point one unit away."""
    out, x, r = [], 0.0, CHAIN_R0
    for i in range(CHAIN_N):
        out.append(((x, 0.0, 0.0), r))
        g = max(2.0, float(np.sqrt(i + 2)))
        x += r + g * r
        r *= g
    return out


def test_deepest_stack(tuning):
    world, cam, ref = _sphere_scene(_chain(), CHAIN_CAM)
    info = world.info()
    depth = info["accel_stack"] - 2  # (FlatView::stack2 = the BVH's depth + 2)
    assert info["accel_ok"] == 1 and depth >= 24, info
    # along the axis from just in front of the small end (both children of every level are hit, every level pushes; origin and
    # direction at the scale of the smallest spheres, which a ray from one unit away could not resolve), a little off it, and
    # from beyond the large end
    rng = np.random.default_rng(23)
    s = 100.0 * CHAIN_R0
    rays = np.zeros((256, 6))
    rays[:, :3] = (-s, 0.0, 0.0)
    rays[:, 3:] = (s, 0.0, 0.0)
    rays[64:, 4:] = s * rng.normal(0.0, 0.01, (192, 2))
    rays[128:192, :3] += s * rng.normal(0.0, 0.3, (64, 3))
    rays[192:, 0] = 1e9
    rays[192:, 3] = -1.0
    exp = _check_hits(world, ref, rays, "chain")
    assert (exp[:, 0] == 1.0).mean() > 0.9
    assert _same_frames(world, cam, "chain") == [(2, 1)]
    tuning(no_lds=1)  # the plain form of the walk, scene in L2
    assert _same_frames(world, cam, "chain outside LDS") == [(2, 0)]


def test_plain_form_on_a_fixture_scene(tuning):
    """scene_10 with the scene forced out of LDS (DESIGN.md s9 rt_tuning no_lds): the plain (non-WIDE) form in the render kernel"""
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    tuning(no_lds=1)
    assert _same_frames(world, cam, "scene_10 outside LDS") == [(2, 0)]


def test_restore_marker_of_an_instance(tuning):
    """the Cornell box: its cube mesh sits under a Transform, entered in the lane (REF_RESTORE on the stack) -- LDS form, then plain form"""
    import rtamd
    world, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    assert world.info()["accel_instances"] >= 1
    assert _same_frames(world, cam, "cornell") == [(2, 1)]
    tuning(no_lds=1)
    assert _same_frames(world, cam, "cornell outside LDS") == [(2, 0)]


def test_media_walks():
    """traverse2_media's TRACK / LIMIT walks share the lane's stack column one after another: the Cornell smoke scene of test_sppm_media_gpu"""
    from test_sppm_media_gpu import CORNELL_CAM, _cornell_smoke, _pair
    world, cam, _ = _pair(_cornell_smoke, CORNELL_CAM, bvh_seed=2)
    assert [u[0] for u in _same_frames(world, cam, "cornell smoke")] == [2]


def test_kernels_5_and_6():
    """the DEFER walk of kernels 5 / 6 and their instance walks on one column: Cornell box with a 2 048-triangle torus instance"""
    import rtamd
    from rtamd import shapes
    P, N, I = shapes.torus(32, 32)
    world = rtamd.World()
    world.new(shapes.cornell_with_mesh(world, P, N, I), bvh_seed=1)
    f, t, up, vfov, asp, ap, fd = configs.CORNELL_CAM
    cam = rtamd.Camera((f, t), up, vfov, asp, ap, fd)
    assert [u[0] for u in _same_frames(world, cam, "cornell + torus", kernels=(2, 5, 6))] == [2, 5, 6]
