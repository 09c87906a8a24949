"""The LDS node table of kernel 2 with the pads of the render at hand (csrc/common/tighten.h).  Boxes only cull, so
everything is compared exactly: small frames of the automatic kernel against kernel 1 (the reference-order program) from cameras at the
places where the pads differ most, and explicit rays through rt_debug_hit_device 7 -- mode 3's table tightened for the batch's own
origins -- against kernel 1, aimed where a box one ulp too small would change the answer."""
import json

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

T_MIN = 1e-3
_cache = {}


def _walk_spheres(node, out):
    if isinstance(node, dict):
        if node.get("type") == "Sphere":
            c = node["center"]
            out.append((float(c["x"]), float(c["y"]), float(c["z"]), float(node["radius"])))
        for v in node.values():
            _walk_spheres(v, out)
    elif isinstance(node, list):
        for v in node:
            _walk_spheres(v, out)


def _scene(name):
    """(World, Camera, oracle scene, spheres [n, 4], extent ew) of a sphere-only fixture scene; loaded once"""
    if name not in _cache:
        import oracle
        import rtamd
        world, cam = rtamd.load_scene_file(scene_path(name))
        ref = oracle.load_scene_file(scene_path(name))
        sph = []
        _walk_spheres(json.load(open(scene_path(name)))["objects"], sph)
        sph = np.unique(np.array(sph), axis=0)
        ew = float((np.abs(sph[:, :3]) + np.abs(sph[:, 3:4])).max())  # largest |coordinate| of the item boxes c -+ r
        assert world.info()["accel_instances"] == 0
        _cache[name] = (world, cam, ref, sph, ew)
    return _cache[name]


def _pad_r(ew, o_abs):
    return 3.0 * 2.0 ** -22 * 2.0 * max(ew, o_abs)


def _cameras(name):
    import rtamd
    world, cam, _, sph, ew = _scene(name)
    limit = 64.0 * ew
    up = (0.0, 1.0, 0.0)
    return {
        "own": cam,
        "aperture 2": rtamd.Camera(((-6.0, 2.0, -6.0), (0.0, 0.0, -1.0)), up, 45.0, 1.0, 2.0, 8.0),
        "0.9 x limit": rtamd.Camera(((0.0, 0.02 * limit, -0.9 * limit), (0.0, 0.0, 0.0)), up, 0.05, 1.0, 0.0, 0.9 * limit),
        "8 x extent": rtamd.Camera(((8.0 * ew, 2.0 * ew, -3.0 * ew), (0.0, 0.0, 0.0)), up, 1.0, 1.0, 0.0, 8.0 * ew),
        "ground level": rtamd.Camera(((-5.5, 0.21, -4.5), (6.0, 0.2, 5.0)), up, 60.0, 1.0, 0.0, 5.0),
    }


def _frame_equals_kernel1(world, cam, what, width=64, height=64, spp=4, lit=True, **kw):
    exp, _ = world.render(cam, width=width, height=height, spp=spp, seed=1, kernel=1, **kw)
    img, st = world.render(cam, width=width, height=height, spp=spp, seed=1, kernel=0, **kw)
    assert (exp != 0).any() or not lit, what
    assert np.array_equal(img, exp, equal_nan=True), "%s: the automatic kernel differs from kernel 1 in %d pixels" % (
        what, int(((img != exp) & ~(np.isnan(img) & np.isnan(exp))).any(axis=2).sum()))
    assert (st["kernel_used"], st["scene_in_lds"]) == (2, 1), (what, st)
    return img, st


@pytest.mark.parametrize("name", ["scene_10.json", "scene_500.json"])
@pytest.mark.parametrize("view", ["own", "aperture 2", "0.9 x limit", "8 x extent", "ground level"])
def test_frames_equal_kernel_1_from_every_camera(name, view):
    world, _, ref, _, ew = _scene(name)
    cam = _cameras(name)[view]
    img, st = _frame_equals_kernel1(world, cam, "%s, %s" % (name, view))
    # the shrink the launch code reports is pad_w - pad_r for the camera's bound: the whole of pad_w but 1/32 from inside the scene, a
    # proportionally smaller part of it from far away, nearly nothing close to the limit -- and never more than the difference
    limit = 64.0 * ew
    pad_w = 3.0 * 2.0 ** -22 * limit
    cam_abs = {"own": 6.0 + 0.05, "aperture 2": 6.0 + 1.0, "0.9 x limit": 0.9 * limit, "8 x extent": 8.0 * ew, "ground level": 5.5}[view]
    want = pad_w - _pad_r(ew, cam_abs) if 2.0 * cam_abs < limit else 0.0
    assert st["box_shrink"] <= want and st["box_shrink"] >= want * (1.0 - 1e-6), (st["box_shrink"], want)
    if view == "0.9 x limit":
        assert st["box_shrink"] == 0.0  # O_r = 1.8 x the limit: the stored boxes
    if view == "own":
        exp, _ = ref.render(64, 64, 4, seed=1)
        assert np.array_equal(img, exp, equal_nan=True), "%s: differs from the oracle" % name


def test_camera_between_extent_and_limit_gets_a_proportionally_smaller_shrink():
    """O_r = 2 cam_abs runs from 2 ew to the limit while the camera moves out to limit / 2: the shrink falls linearly to exactly 0"""
    import rtamd
    world, _, _, _, ew = _scene("scene_10.json")
    limit = 64.0 * ew
    pad_w = 3.0 * 2.0 ** -22 * limit
    got = []
    for f in (0.125, 0.25, 0.4375, 0.5, 0.75):
        cam = rtamd.Camera(((0.0, 0.5 * f * limit, -f * limit), (0.0, 0.0, 0.0)), (0.0, 1.0, 0.0), 0.2, 1.0, 0.0, f * limit)
        _, st = _frame_equals_kernel1(world, cam, "camera at %g x limit" % f, width=16, height=16, spp=2, lit=False)  # (a few pixels of the ground from afar)
        got.append(st["box_shrink"])
        want = max(0.0, pad_w * (1.0 - 2.0 * f))
        assert want * (1.0 - 1e-6) <= st["box_shrink"] <= want, (f, st["box_shrink"], want)
    assert got[3] == 0.0 and got[4] == 0.0 and got[0] > got[1] > got[2] > 0.0


@pytest.mark.parametrize("integrator", [0, 1])
def test_cornell_box_keeps_the_stored_boxes_and_equals_kernel_1(integrator):
    """rectangles, a cube and a mesh under a Transform (the GENERAL = 1 variant): a scene with an instance renders with shrink 0 -- its
    table holds the object-space BVH too"""
    import rtamd
    world, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    assert world.info()["accel_instances"] == 1
    _, st = _frame_equals_kernel1(world, cam, "cornell, integrator %d" % integrator, integrator=integrator)
    assert st["box_shrink"] == 0.0


@pytest.mark.parametrize("integrator", [0, 1])
def test_room_of_rectangles_without_an_instance_is_tightened_and_equals_kernel_1(integrator):
    """the same kinds without the Transform: rectangles (boxes of zero thickness), a cube, spheres, a rectangle light; GENERAL = 1, tightened"""
    import rtamd
    w = rtamd.World()
    white, red, green = (w.Lambertian(w.ConstantTexture(c)) for c in ((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15)))
    light = w.XZRectangle((213.0, 227.0), (343.0, 332.0), 554.0, w.DiffuseLight(w.ConstantTexture((15.0, 15.0, 15.0))))
    items = [w.YZRectangle((0.0, 0.0), (555.0, 555.0), 555.0, green), w.YZRectangle((0.0, 0.0), (555.0, 555.0), 0.0, red), light,
             w.XZRectangle((0.0, 0.0), (555.0, 555.0), 0.0, white), w.XZRectangle((0.0, 0.0), (555.0, 555.0), 555.0, white),
             w.XYRectangle((0.0, 0.0), (555.0, 555.0), 555.0, white), w.Cube((130.0, 0.0, 65.0), (295.0, 165.0, 230.0), white),
             w.Sphere((400.0, 90.0, 300.0), 90.0, w.Dielectric(1.5, w.ConstantTexture((1.0, 1.0, 1.0)))),
             w.Sphere((190.0, 240.0, 150.0), 75.0, w.Metal(w.ConstantTexture((0.8, 0.85, 0.88)), 0.0))]
    w.new(items, lights=[light], bvh_seed=1)
    cam = rtamd.Camera(((278.0, 278.0, -800.0), (278.0, 278.0, 0.0)), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0)
    _, st = _frame_equals_kernel1(w, cam, "room, integrator %d" % integrator, integrator=integrator)
    want = 3.0 * 2.0 ** -22 * (64.0 * 555.0 - 2.0 * 800.0)
    assert want * (1.0 - 1e-5) <= st["box_shrink"] <= want * (1.0 + 1e-5)  # (the rectangles' boxes are 1e-4 thick: the extent is 555 to 2e-7)


def test_many_samples_on_few_pixels_so_that_waves_regenerate_mid_unit():
    """16 x 16 x 64 spp of scene_500: lanes of every depth side by side in a wave, every mix of descending, waiting and finished lanes"""
    world, cam, _, _, _ = _scene("scene_500.json")
    exp, _ = world.render(cam, width=16, height=16, spp=64, seed=1, kernel=1)
    img, st = world.render(cam, width=16, height=16, spp=64, seed=1, kernel=2)
    assert (st["kernel_used"], st["scene_in_lds"]) == (2, 1) and st["box_shrink"] > 0.0
    assert np.array_equal(img, exp, equal_nan=True)


def _ulps(x, k):
    x = np.asarray(x, dtype=np.float32)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x.astype(np.float64)


def _rays(name, n, seed):
    """n rays with origins on sphere surfaces (c + r n) and at the camera; a third tangent to a sphere (n x random, tilted by +-1e-9), a
    third through corners and face points of the tightened item boxes (c -+ r) -+ pad_r, stepped by -1, 0, +1 f32 ulp, a third random"""
    _, _, _, sph, ew = _scene(name)
    rng = np.random.default_rng(seed)
    cam_o = np.array([-6.0, 2.0, -6.0])
    pad = _pad_r(ew, ew)  # every origin lies within the extent
    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    for i in range(n):
        j = int(rng.integers(len(sph)))
        c, r = sph[j, :3], sph[j, 3]
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        if i % 16 == 0:  # (axis normals: the origin lies in a face of the sphere's own box)
            nrm = np.eye(3)[int(rng.integers(3))] * rng.choice([-1.0, 1.0])
        at_camera = i % 4 == 3
        o[i] = cam_o if at_camera else c + r * nrm
        kind = i % 3
        if kind == 0:  # tangent: from the surface point along the tangent plane; from the camera at the silhouette
            t = np.cross(nrm, rng.normal(size=3))
            t /= np.linalg.norm(t)
            if at_camera:
                u = c - cam_o
                p = np.cross(u, rng.normal(size=3))
                p /= np.linalg.norm(p)
                d[i] = c + p * r * (1.0 + rng.choice([-1e-9, 1e-9])) - cam_o
            else:
                d[i] = t + nrm * rng.choice([-1e-9, 0.0, 1e-9])
        elif kind == 1:  # a corner or a face point of another sphere's tightened box
            k = int(rng.integers(len(sph)))
            ck, rk = sph[k, :3], sph[k, 3]
            sgn = rng.choice([-1.0, 1.0], 3)
            p = ck + sgn * (rk + pad)
            if i % 2:  # a point inside one face instead of the corner
                ax = int(rng.integers(3))
                keep = p[ax]
                p = ck + rng.uniform(-1.0, 1.0, 3) * (rk + pad)
                p[ax] = keep
            p = _ulps(p, int(rng.integers(-1, 2)))
            d[i] = p - o[i]
        else:
            d[i] = rng.normal(size=3)
    return np.concatenate([o, d], axis=1)


@pytest.mark.parametrize("name", ["scene_10.json", "scene_500.json"])
def test_explicit_rays_through_the_tightened_table(name):
    world, _, ref, _, ew = _scene(name)
    n = 20000
    rays = _rays(name, n, 7)
    assert np.abs(rays[:, :3]).max() <= ew * (1.0 + 1e-12)
    k1 = world.debug_hit(rays, t_min=T_MIN, kernel=1)
    exp = ref.hit_batch(rays, t_min=T_MIN, n_workers=4)
    assert np.array_equal(k1[:, :11], exp[:, :11], equal_nan=True), "kernel 1 differs from the oracle in %d rows" % int((k1[:, :11] != exp[:, :11]).any(axis=1).sum())
    k3 = world.debug_hit(rays, t_min=T_MIN, kernel=3)
    k7 = world.debug_hit(rays, t_min=T_MIN, kernel=7)
    # the tightened table finds what the stored one finds, in every field of every ray
    assert np.array_equal(k7, k3, equal_nan=True), "%d rows differ between the tightened and the stored table" % int((k7 != k3).any(axis=1).sum())
    # ... and what the reference-order program finds.  The one caveat of the strict comparisons: kernel 1 tests the reference's own f64 boxes
    # (no pad), which cull a ray within rounding of a box edge that the padded boxes keep, so the accel may FIND a nearer hit kernel 1 misses --
    # never the other way round.  Such rays are counted, and capped at 0.1 %
    diff = (k7 != k1).any(axis=1) & ~(np.isnan(k7) & np.isnan(k1)).all(axis=1)
    nearer = diff & (k7[:, 0] == 1.0) & ((k1[:, 0] == 0.0) | (k7[:, 1] < k1[:, 1]))
    print("%s: %d of %d rays differ from kernel 1, %d of them nearer hits at a reference box edge; hits %d" % (name, diff.sum(), n, nearer.sum(), int(k1[:, 0].sum())))
    assert not (diff & ~nearer).any(), "%d rays lost or changed by the accel, first %s" % ((diff & ~nearer).sum(), rays[np.argmax(diff & ~nearer)])
    assert nearer.sum() <= n // 1000
    assert 0.3 < k1[:, 0].mean() < 0.999


def test_a_batch_from_far_origins_keeps_the_stored_boxes():
    """origins at 40 x the extent: O_r = 80 ew is beyond origin_limit2 = 64 ew, the shrink is 0 and mode 7 is mode 3"""
    world, _, _, sph, ew = _scene("scene_10.json")
    rng = np.random.default_rng(3)
    n = 2048
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = u * 40.0 * ew
    tgt = sph[rng.integers(len(sph), size=n), :3] + rng.normal(0.0, 0.3, (n, 3))
    rays = np.concatenate([o, tgt - o], axis=1)
    k1 = world.debug_hit(rays, t_min=T_MIN, kernel=1)
    assert np.array_equal(world.debug_hit(rays, t_min=T_MIN, kernel=7), k1)
    assert np.array_equal(world.debug_hit(rays, t_min=T_MIN, kernel=3), k1)
    assert k1[:, 0].mean() > 0.3
