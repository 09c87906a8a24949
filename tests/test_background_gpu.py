"""Backgrounds for rays that miss the scene (rt_scene_set_background) on the GPU.  Miss pixels and the furnace frame are
restated in numpy from the oracle's camera rays and hit classification, bit for bit; a black background reproduces every frame rendered
without one; kernels 1 and 2 and every entry point agree under a sky; a medium and integrator 1 stay unbiased; the refusals hold."""
import math

import numpy as np
import pytest

import nested_scenes as ns
from conftest import scene_path
from env_ref import _background, _checker, _sphere_uv, _texel, _unit  # noqa: F401

pytestmark = pytest.mark.gpu

PI = 3.14159265358979323846264338327950288
FRAC_1_PI = 0.318309886183790671537767526745028724
SKY = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))
BLACK = dict(color=(0.0, 0.0, 0.0))


def _deferred_world():
    """a World whose new() / set_root() leave the scene uncommitted, so that a background can still be set"""
    import rtamd

    class Deferred(rtamd.World):
        def commit(self):
            return self
    return Deferred()


def _commit(w, bg):
    import rtamd
    if bg is not None:
        w.set_background(**bg)
    rtamd.World.commit(w)
    return w


# ---- 1. miss pixels bit for bit -----------------------------------------------------------------------------------------------------
OPEN_CAM = ((0.0, 1.0, 6.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 50.0, 1.5, 0.0, 10.0)


def _open_scene(B, bg_spec=None, oracle_side=False):
    """one Lambertian sphere left of centre and a sphere light behind the camera; returns (items, lights, background kwargs)"""
    ball = B.Sphere((-1.2, 0.5, 0.0), 0.8, B.Lambertian(B.ConstantTexture((0.6, 0.5, 0.4))))
    if oracle_side:
        lt = B.Sphere((0.0, 3.0, 12.0), 1.0, B.DiffuseLight(B.ConstantTexture((4.0, 4.0, 4.0))))
    else:
        lt = B.SphereDiffuseLight((0.0, 3.0, 12.0), 1.0, (4.0, 4.0, 4.0))
    kw = None
    if bg_spec is not None and not oracle_side:
        if bg_spec["kind"] == 1:
            kw = dict(color=bg_spec["color"], scale=bg_spec.get("scale", 1.0))
        elif bg_spec["kind"] == 2:
            kw = dict(gradient=bg_spec["gradient"], scale=bg_spec.get("scale", 1.0))
        elif bg_spec["tex"] == "image":
            kw = dict(texture=B.ImageTexture(bg_spec["image"]), scale=bg_spec.get("scale", 1.0))
        else:
            kw = dict(texture=B.CheckerTexture(B.ConstantTexture(bg_spec["c0"]), B.ConstantTexture(bg_spec["c1"])), scale=bg_spec.get("scale", 1.0))
    return [ball, lt], [lt], kw


def _pair_open(bg_spec):
    import oracle
    import rtamd
    w = _deferred_world()
    items, lights, kw = _open_scene(w, bg_spec)
    w.new(items, lights=lights, bvh_seed=1)
    _commit(w, kw)
    o = oracle.Scene()
    oitems, _, _ = _open_scene(o, bg_spec, oracle_side=True)
    o.World(oitems, 1)
    o.Camera(*OPEN_CAM)
    f, t, up, vfov, asp, ap, fd = OPEN_CAM
    return w, rtamd.Camera((f, t), up, vfov, asp, ap, fd), o


def _image_tex():
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, size=(9, 17, 3), dtype=np.uint8)


BG_SPECS = {
    "constant": dict(kind=1, color=(0.3, 0.55, 0.9), scale=1.5),
    "gradient": dict(kind=2, gradient=SKY, scale=1.0),
    "gradient_scaled": dict(kind=2, gradient=((0.2, 0.1, 0.0), (0.9, 0.8, 1.3)), scale=0.75),
    "image": dict(kind=3, tex="image", image=_image_tex(), scale=2.0),
    "checker": dict(kind=3, tex="checker", c0=(0.1, 0.2, 0.3), c1=(0.9, 0.8, 0.7), scale=1.0),
}


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("name", sorted(BG_SPECS))
def test_miss_pixels_bit_for_bit(name, kernel, integrator):
    spec = BG_SPECS[name]
    W, H, SPP, SEED = 36, 24, 4, 3
    w, cam, o = _pair_open(spec)
    img, st = w.render(cam, width=W, height=H, spp=SPP, seed=SEED, kernel=kernel, integrator=integrator)
    assert st["kernel_used"] == kernel
    acc = np.zeros((H, W, 3))
    all_miss = np.ones((H, W), dtype=bool)
    for s in range(SPP):
        rays = o.camera_rays(W, H, SEED, s)
        hit = o.hit_batch(rays.reshape(-1, 6), t_min=1e-3)[:, 0].reshape(H, W) != 0.0
        all_miss &= ~hit
        acc = acc + _background(spec, rays[..., 3:])
    exp = acc / SPP
    assert all_miss.mean() > 0.5
    assert (~all_miss).sum() > 20
    assert np.array_equal(img[all_miss], exp[all_miss]), "%d miss pixels differ" % int((img[all_miss] != exp[all_miss]).any(axis=-1).sum())
    assert (img[all_miss] > 0).all()


# ---- 2. furnace frame ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
def test_furnace_frame_bit_for_bit(kernel):
    import oracle
    import rtamd
    a, c = (0.5, 0.625, 0.75), (0.8, 0.4, 1.2)
    cam_args = ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 1.0, 0.0, 10.0)
    w = _deferred_world()
    w.new([w.Sphere((0.0, 0.0, 0.0), 1.0, w.Lambertian(w.ConstantTexture(a)))])
    _commit(w, dict(color=c))
    o = oracle.Scene()
    o.World([o.Sphere((0.0, 0.0, 0.0), 1.0, o.Lambertian(o.ConstantTexture(a)))], 1)
    o.Camera(*cam_args)
    f, t, up, vfov, asp, ap, fd = cam_args
    cam = rtamd.Camera((f, t), up, vfov, asp, ap, fd)
    W = H = 32
    SPP, SEED = 6, 11
    img, _ = w.render(cam, width=W, height=H, spp=SPP, seed=SEED, kernel=kernel)
    ac = np.array(a) * np.array(c)
    acc = np.zeros((H, W, 3))
    n_hit = 0
    for s in range(SPP):
        rays = o.camera_rays(W, H, SEED, s)
        hit = o.hit_batch(rays.reshape(-1, 6), t_min=1e-3)[:, 0].reshape(H, W) != 0.0
        n_hit += int(hit.sum())
        acc = acc + np.where(hit[..., None], ac, np.array(c))
    assert 0 < n_hit < W * H * SPP
    assert np.array_equal(img, acc / SPP)


# ---- scenes for 3. and 4. -----------------------------------------------------------------------------------------------------------
def _cornell(bg):
    import rtamd
    w, cam = rtamd.select_scene(scene_path("cube.obj"), 1.5, commit=False)
    return _commit(w, bg), cam, {}


def _scene10(bg):
    import rtamd
    w, cam = rtamd.load_scene_file(scene_path("scene_10.json"), commit=False)
    return _commit(w, bg), cam.with_aspect(1.5), {}


def _smoke(bg):
    import rtamd
    from test_sppm_media_gpu import _cornell_smoke
    w = _deferred_world()
    items, lights = _cornell_smoke(w)
    w.new(items, lights=lights, bvh_seed=2)
    f, t, up, vfov, asp, ap, fd = ns.CORNELL_CAM
    return _commit(w, bg), rtamd.Camera((f, t), up, vfov, asp, ap, fd), {}


def _book2(bg):
    import rtamd
    from rtamd import shapes
    w = _deferred_world()
    w.new(shapes.final_scene(w, n_boxes=5, n_cluster=60), bvh_seed=3)
    f, t, up, vfov, asp, ap, fd = shapes.FINAL_SCENE_CAMERA
    return _commit(w, bg), rtamd.Camera((f, t), up, vfov, asp, ap, fd), dict(shutter=shapes.FINAL_SCENE_SHUTTER)


def _nested(bg):
    w = _deferred_world()
    w, cam = ns.n1(w)
    return _commit(w, bg), cam, {}


SCENES = {"cornell": _cornell, "scene_10": _scene10, "smoke": _smoke, "book2": _book2, "nested": _nested}
CASES = [("cornell", 0), ("cornell", 1), ("scene_10", 0), ("smoke", 0), ("book2", 0), ("nested", 0), ("nested", 1)]


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("scene,integrator", CASES)
def test_black_background_is_a_no_op(scene, integrator, kernel):
    w0, cam, kw = SCENES[scene](None)
    w1, _, _ = SCENES[scene](BLACK)
    assert w1.background()["kind"] == 1 and w0.background()["kind"] == 0
    assert w1.fingerprint() != w0.fingerprint()
    ref, st0 = w0.render(cam, width=40, height=28, spp=4, seed=5, kernel=kernel, integrator=integrator, **kw)
    got, st1 = w1.render(cam, width=40, height=28, spp=4, seed=5, kernel=kernel, integrator=integrator, **kw)
    assert st0["kernel_used"] == st1["kernel_used"] == kernel
    assert (ref > 0).any()
    assert np.array_equal(got, ref, equal_nan=True), "%d pixels differ" % int((got != ref).any(axis=-1).sum())


@pytest.mark.parametrize("scene,integrator", CASES)
def test_kernel_1_equals_kernel_2_under_a_sky(scene, integrator):
    w, cam, kw = SCENES[scene](dict(gradient=SKY))
    w0, _, _ = SCENES[scene](None)
    i1, _ = w.render(cam, width=40, height=28, spp=4, seed=7, kernel=1, integrator=integrator, **kw)
    i2, st = w.render(cam, width=40, height=28, spp=4, seed=7, kernel=2, integrator=integrator, **kw)
    assert st["kernel_used"] == 2
    assert np.array_equal(i1, i2, equal_nan=True), "%d pixels differ" % int((i1 != i2).any(axis=-1).sum())
    plain, _ = w0.render(cam, width=40, height=28, spp=4, seed=7, kernel=2, integrator=integrator, **kw)
    assert ((i2 >= plain) | np.isnan(plain)).all() and (i2 > plain).any()  # the sky only adds light (same paths, same draws)


# ---- 5. entry points ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sky_cornell():
    return _cornell(dict(gradient=SKY, scale=2.0))


@pytest.mark.parametrize("integrator", [0, 1])
def test_entry_points_agree_under_a_background(sky_cornell, integrator, tuning):
    import rtamd
    w, cam, _ = sky_cornell
    W, H, SPP = 44, 30, 8
    ref, _ = w.render(cam, width=W, height=H, spp=SPP, seed=9, integrator=integrator)
    plain, _, _ = _cornell(None)
    no_bg, _ = plain.render(cam, width=W, height=H, spp=SPP, seed=9, integrator=integrator)
    assert (ref > no_bg).any()
    p = rtamd.default_params(width=W, height=H, spp=SPP, seed=9, integrator=integrator)
    state = None
    for a, b in ((0, 3), (3, 5), (5, 8)):
        state, _ = w.render_accumulate(cam, p, a, b, state)
    assert np.array_equal(rtamd.accum_finalize(p, state), ref)
    img, tile_spp, _ = w.render_adaptive(cam, W, H, SPP, min_spp=2, threshold=0.0, seed=9, integrator=integrator)
    assert (tile_spp == SPP).all() and np.array_equal(img, ref)
    for force in (0, 1):
        tuning(multi_force_rccl=force)
        img, _ = w.render_multi(cam, devices=[0, 0], width=W, height=H, spp=SPP, seed=9, integrator=integrator)
        assert np.array_equal(img, ref), force
    tuning()
    img, _ = w.render_camera_frame(cam.frame(), width=W, height=H, spp=SPP, seed=9, integrator=integrator)
    assert np.array_equal(img, ref)


# ---- 6. Beer-Lambert ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
def test_medium_under_a_constant_background_follows_beer_lambert(kernel):
    import oracle
    import rtamd
    sigma, R, c = 0.6, 1.0, np.array([0.9, 0.6, 0.3])
    cam_args = ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0)
    w = _deferred_world()
    # a second object (behind the camera, out of every camera ray's way): a lone object would sit in both children of the root BVHNode
    # (bvh.rs:66), and a medium visited twice draws twice
    w.new([w.ConstantMedium(sigma, w.Sphere((0.0, 0.0, 0.0), R, w.Lambertian(w.ConstantTexture((0.5, 0.5, 0.5)))),
                            w.Isotropic(w.ConstantTexture((0.0, 0.0, 0.0)))),
           w.Sphere((0.0, 0.0, 20.0), 0.5, w.Lambertian(w.ConstantTexture((0.5, 0.5, 0.5))))])
    _commit(w, dict(color=tuple(c)))
    f, t, up, vfov, asp, ap, fd = cam_args
    cam = rtamd.Camera((f, t), up, vfov, asp, ap, fd)
    W = H = 12
    SPP, SEED = 512, 4
    img, st = w.render(cam, width=W, height=H, spp=SPP, seed=SEED, kernel=kernel)
    assert st["kernel_used"] == kernel
    o = oracle.Scene()
    o.World([o.Sphere((0.0, 0.0, 0.0), R, o.Lambertian(o.ConstantTexture((0.5, 0.5, 0.5))))], 1)
    o.Camera(*cam_args)
    p_sum = np.zeros((H, W))
    pq_sum = np.zeros((H, W))
    for s in range(SPP):  # the expected transmittance of every sample's camera ray: exp(-sigma * chord)
        r = o.camera_rays(W, H, SEED, s)
        orig, d = r[..., :3], r[..., 3:]
        a = (d * d).sum(-1)
        hb = (orig * d).sum(-1)
        disc = hb * hb - a * ((orig * orig).sum(-1) - R * R)
        chord = np.where(disc > 0, 2.0 * np.sqrt(np.maximum(disc, 0.0)) / np.sqrt(a), 0.0)
        p = np.exp(-sigma * chord)
        p_sum += p
        pq_sum += p * (1.0 - p)
    exp_t = p_sum / SPP
    se = np.sqrt(np.maximum(pq_sum / SPP, 1e-4 / SPP) / SPP)
    inside = exp_t < 0.999
    assert inside.sum() > 20
    for ch in range(3):
        z = np.abs(img[..., ch] / c[ch] - exp_t) / se
        assert z.max() < 5.0, (ch, float(z.max()))


# ---- 7. the mixture stays unbiased ------------------------------------------------------------------------------------------------
def test_mixture_integrator_is_unbiased_under_a_gradient():
    import rtamd
    w = _deferred_world()
    ground = w.Sphere((0.0, -1000.0, 0.0), 1000.0, w.Lambertian(w.ConstantTexture((0.5, 0.5, 0.5))))
    ball = w.Sphere((0.0, 1.0, 0.0), 1.0, w.Lambertian(w.ConstantTexture((0.7, 0.3, 0.2))))
    lt = w.SphereDiffuseLight((3.0, 5.0, 1.0), 1.5, (3.0, 3.0, 3.0))
    w.new([ground, ball, lt], lights=[lt])
    _commit(w, dict(gradient=SKY))
    cam = rtamd.Camera(((0.0, 2.0, 8.0), (0.0, 1.0, 0.0)), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0)
    W = H = 32
    K, SPP = 12, 16

    def blocks(integrator):
        out = []
        for k in range(K):
            img, _ = w.render(cam, width=W, height=H, spp=SPP, seed=100 + k, integrator=integrator)
            out.append(img.reshape(4, 8, 4, 8, 3).mean(axis=(1, 3)))
        out = np.array(out)
        return out.mean(0), out.std(0, ddof=1) / math.sqrt(K)
    m0, s0 = blocks(0)
    m1, s1 = blocks(1)
    z = np.abs(m0 - m1) / np.sqrt(s0 * s0 + s1 * s1 + 1e-12)
    assert np.isfinite(m1).all() and (m1 > 0).all()
    assert z.max() < 5.0, float(z.max())


# ---- 8. refusals and selection ----------------------------------------------------------------------------------------------------
def test_sppm_refuses_a_scene_with_a_background(sky_cornell):
    import rtamd
    w, cam, _ = sky_cornell
    with pytest.raises(rtamd.RtError) as e:
        w.render_sppm(cam, width=16, height=16, spp=2, iterations=1, photons_per_iter=1000)
    assert e.value.code == -10 and "background" in str(e.value)


def _large_mesh(bg):
    import rtamd
    from rtamd import shapes
    w = _deferred_world()
    P, N, I = shapes.torus(nu=40, nv=80)
    w.new(shapes.cornell_with_mesh(w, P, N, I), bvh_seed=1)
    f, t, up, vfov, asp, ap, fd = ns.CORNELL_CAM
    return _commit(w, bg), rtamd.Camera((f, t), up, vfov, asp, ap, fd)


def test_kernels_5_6_refused_and_auto_selection_picks_kernel_2():
    import rtamd
    w0, cam = _large_mesh(None)
    _, st = w0.render(cam, width=32, height=24, spp=2, seed=1)
    assert st["kernel_used"] in (5, 6)  # the scene takes the instance service without a background
    w, _ = _large_mesh(dict(gradient=SKY))
    for k in (5, 6):
        with pytest.raises(rtamd.RtError) as e:
            w.render(cam, width=32, height=24, spp=2, seed=1, kernel=k)
        assert e.value.code == -10 and "background" in str(e.value)
    auto, st = w.render(cam, width=32, height=24, spp=2, seed=1)
    assert st["kernel_used"] == 2
    k2, _ = w.render(cam, width=32, height=24, spp=2, seed=1, kernel=2)
    assert np.array_equal(auto, k2)
