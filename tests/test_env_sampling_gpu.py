"""Env sampling -- the background as a light of integrator 1 (rt_scene_set_env_sampling) -- on the GPU.  The table the
device builds, the draws from it and its pdf are restated in numpy from rtamd.h, bit for bit; the pdf integrates to one; integrator 1
with env sampling agrees with a closed form and with integrator 0 within 5 standard errors; it cuts the variance of a scene lit by a
small sun; every entry point inherits it; with the switch off nothing moved (frames pinned from the parent commit)."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import nested_scenes as ns
from conftest import GOLDEN, scene_path
from env_ref import _background, _checker, _checker_sines, _sphere_uv, _texel, _unit, det_sin, env_dir, pdf_ref, sample_ref, table_ref  # noqa: F401

pytestmark = pytest.mark.gpu

PI = 3.14159265358979323846264338327950288
FRAC_1_PI = 0.318309886183790671537767526745028724
SKY = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))


def _deferred_world():
    """a World whose new() / set_root() leave the scene uncommitted, so that a background and env sampling can still be set"""
    import rtamd

    class Deferred(rtamd.World):
        def commit(self):
            return self
    return Deferred()


def _commit(w, bg=None, env=None):
    import rtamd
    if bg is not None:
        w.set_background(**bg)
    if env is not None:
        w.set_env_sampling(True, *env)
    rtamd.World.commit(w)
    return w


def _bg_kwargs(B, spec):
    if spec["kind"] == 1:
        return dict(color=spec["color"], scale=spec.get("scale", 1.0))
    if spec["kind"] == 2:
        return dict(gradient=spec["gradient"], scale=spec.get("scale", 1.0))
    if spec["tex"] == "image":
        return dict(texture=B.ImageTexture(spec["image"]), scale=spec.get("scale", 1.0))
    return dict(texture=B.CheckerTexture(B.ConstantTexture(spec["c0"]), B.ConstantTexture(spec["c1"])), scale=spec.get("scale", 1.0))


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def sun_image():
    """64 x 32, every texel (1, 1, 1) except a 4 x 4 block of (255, 255, 255) in rows 6-9 from the top, columns 30-33"""
    img = np.ones((32, 64, 3), dtype=np.uint8)
    img[6:10, 30:34] = 255
    return img


SUN = dict(kind=3, tex="image", image=sun_image(), scale=20.0)
SPECS = {
    "constant": (dict(kind=1, color=(0.3, 0.55, 0.9), scale=1.5), None),
    "gradient": (dict(kind=2, gradient=SKY, scale=1.0), None),
    "sun": (SUN, None),
    "sun_16x8": (SUN, (16, 8)),
    "checker": (dict(kind=3, tex="checker", c0=(0.1, 0.2, 0.3), c1=(0.9, 0.8, 0.7), scale=1.0), None),
}
AUTO = {"constant": (256, 128), "gradient": (256, 128), "sun": (64, 32), "sun_16x8": (16, 8), "checker": (256, 128)}
FLOOR_ALBEDO = (0.6, 0.5, 0.4)


def _floor_world(spec, env, ball=False, lights=False):
    """a large Lambertian XZRectangle floor at y = 0 under the background `spec`; ball: one Lambertian sphere resting on it"""
    w = _deferred_world()
    items = [w.XZRectangle((-1000.0, -1000.0), (1000.0, 1000.0), 0.0, w.Lambertian(w.ConstantTexture(FLOOR_ALBEDO)))]
    if ball:
        items.append(w.Sphere((0.0, 1.0, 0.0), 1.0, w.Lambertian(w.ConstantTexture((0.7, 0.3, 0.2)))))
    w.new(items, bvh_seed=1)
    return _commit(w, _bg_kwargs(w, spec), env)


def _table_world(name):
    spec, size = SPECS[name]
    return _floor_world(spec, size if size is not None else (0, 0)), spec


def _sun_share(q):
    """the share of the 4 x 4 block in the 64 x 32 table's total, and the share of the sphere it covers"""
    block = np.zeros((32, 64), dtype=bool)
    block[32 - 10:32 - 6, 30:34] = True  # image row r from the top is table row H - 1 - r
    theta = PI * (np.arange(32) + 0.5) / 32
    solid = np.broadcast_to((np.sin(theta) * (PI / 32) * (2 * PI / 64))[:, None], (32, 64))
    return float(q[block].astype(np.float64).sum() / q.astype(np.float64).sum()), float(solid[block].sum() / (4 * PI))


# ---- 1. the table, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SPECS))
def test_table_bit_for_bit(name):
    w, spec = _table_world(name)
    q = w.debug_env_table()
    W, H = AUTO[name]
    assert q.shape == (H, W) and q.dtype == np.uint32
    ref, sure = table_ref(spec, W, H)
    left_out = 1.0 - sure.mean()
    print("%s: %d x %d, cells left out %.4f, q max %d, zeros %d" % (name, W, H, left_out, int(q.max()), int((q == 0).sum())))
    assert left_out <= 0.01
    assert int(q.max()) == 4294967295 and (q > 0).all()
    bad = (q.astype(np.uint64) != ref) & sure
    assert not bad.any(), "%d cells differ" % int(bad.sum())
    assert np.array_equal(w.debug_env_table(), q)  # read twice: the same table
    if name == "sun":  # the fixture is the hard case: more than half of the total in under 1 % of the sphere
        share, sphere = _sun_share(q)
        print("the block holds %.4f of the total on %.5f of the sphere" % (share, sphere))
        assert share > 0.5 and sphere < 0.01 and _sun_share(ref)[0] == share


# ---- 2. draws and pdf, bit for bit ------------------------------------------------------------------------------------------------------
def _xi(n, stream=0):
    import rtamd
    g, _ = rtamd.debug_rng_floats(77, stream, 0, 4 * n, 0.0, 1.0)
    return np.array(g).reshape(n, 4)


@pytest.mark.parametrize("name", ["sun", "sun_16x8", "gradient"])
def test_draws_and_pdf_bit_for_bit(name):
    w, _ = _table_world(name)
    q = w.debug_env_table()
    xi = _xi(4096)
    got = w.debug_env_sample(xi)
    d_ref, _ = sample_ref(q, xi)
    assert np.array_equal(got[:, :3], d_ref), "%d directions differ" % int((got[:, :3] != d_ref).any(axis=1).sum())
    p_ref = pdf_ref(q, d_ref)
    assert np.array_equal(got[:, 3], p_ref), "%d pdfs differ" % int((got[:, 3] != p_ref).sum())
    assert (got[:, 3] > 0).all()
    assert np.array_equal(w.debug_env_pdf(got[:, :3]), got[:, 3])
    assert np.array_equal(w.debug_env_pdf(3.5 * got[:, :3]), pdf_ref(q, 3.5 * got[:, :3]))  # any length: unit(d) first


def _chi2_sf(x, k):
    """upper tail of chi-square with k degrees of freedom, Wilson-Hilferty (k = 127 here: good to a few percent of p)"""
    z = ((x / k) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * k))) / math.sqrt(2.0 / (9.0 * k))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def test_histogram_of_draws_follows_the_table():
    w, _ = _table_world("sun_16x8")
    q = w.debug_env_table().astype(np.float64)
    n = 65536
    xi = _xi(n, stream=1)
    got = w.debug_env_sample(xi)
    _, cells = sample_ref(q.astype(np.uint64), xi)
    assert np.array_equal(got[:, :3], env_dir((cells[:, 0] + xi[:, 2]) / 16, (cells[:, 1] + xi[:, 3]) / 8)[0])
    obs = np.zeros((8, 16))
    np.add.at(obs, (cells[:, 1], cells[:, 0]), 1.0)
    exp = n * q / q.sum()
    assert exp.min() >= 5.0
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    p = _chi2_sf(chi2, 16 * 8 - 1)
    print("chi2 = %.2f on 127 dof, p = %.4g" % (chi2, p))
    assert p > 1e-4


# ---- 3. the pdf integrates to one -------------------------------------------------------------------------------------------------------
def test_pdf_integrates_to_one():
    w, _ = _table_world("sun")
    GW, GH = 2048, 1024
    u = np.broadcast_to(((np.arange(GW) + 0.5) / GW)[None, :], (GH, GW))
    v = np.broadcast_to(((np.arange(GH) + 0.5) / GH)[:, None], (GH, GW))
    theta, phi = np.pi * v, 2.0 * np.pi * u
    d = np.stack([-np.cos(phi) * np.sin(theta), -np.cos(theta), np.sin(phi) * np.sin(theta)], axis=-1)
    p = w.debug_env_pdf(d.reshape(-1, 3)).reshape(GH, GW)
    total = float((p * (2.0 * np.pi / GW) * (np.pi / GH) * np.sin(theta)).sum())
    print("integral of the pdf: %.6f" % total)
    assert abs(total - 1.0) < 1e-3


# ---- 4. unbiased ------------------------------------------------------------------------------------------------------------------------
def _floor_expectation(spec):
    """a / pi * sum over the image's texels of B * integral over the texel of max(0, cos theta_n) dOmega, n = +y: with theta the polar
    angle from straight down (v = theta / pi), cos theta_n = -cos theta, so a texel row between theta_a < theta_b in the upper hemisphere
    contributes dphi * (sin^2 theta_a - sin^2 theta_b) / 2"""
    img = spec["image"].astype(np.float64) / 255.0 * spec["scale"]
    h, wd, _ = img.shape
    r = np.arange(h)
    th_b = np.pi * (1.0 - r / h)          # image row r from the top spans v in [1 - (r + 1) / h, 1 - r / h]
    th_a = np.maximum(np.pi * (1.0 - (r + 1) / h), np.pi / 2)
    band = np.where(th_b > np.pi / 2, (np.sin(th_a) ** 2 - np.sin(th_b) ** 2) / 2.0, 0.0) * (2.0 * np.pi / wd)
    irradiance = (img * band[:, None, None]).sum(axis=(0, 1))
    return np.asarray(FLOOR_ALBEDO) / np.pi * irradiance


def _down_camera():
    import rtamd
    return rtamd.Camera(((0.0, 5.0, 0.0), (0.0, 0.0, 0.0)), (0.0, 0.0, -1.0), 40.0, 1.0, 0.0, 10.0)


@pytest.mark.parametrize("kernel", [1, 2])
def test_floor_under_the_sun_matches_the_closed_form(kernel):
    w = _floor_world(SUN, (0, 0))
    cam = _down_camera()
    want = _floor_expectation(SUN)
    means = []
    for k in range(16):
        img, st = w.render(cam, width=64, height=64, spp=256, seed=300 + k, kernel=kernel, integrator=1)
        assert st["kernel_used"] == kernel
        means.append(img.mean(axis=(0, 1)))
    means = np.array(means)
    m, se = means.mean(0), means.std(0, ddof=1) / math.sqrt(len(means))
    z = np.abs(m - want) / se
    print("kernel %d: mean %s, closed form %s, se %s, z %s" % (kernel, m, want, se, z))
    assert (se > 0).all()
    assert z.max() < 5.0, z


def _block_compare(w, cam, W=32, H=32, K=12, SPP=16, **kw):
    def blocks(integrator):
        out = []
        for k in range(K):
            img, _ = w.render(cam, width=W, height=H, spp=SPP, seed=100 + k, integrator=integrator, **kw)
            out.append(img.reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3)))
        out = np.array(out)
        return out.mean(0), out.std(0, ddof=1) / math.sqrt(K)
    m0, s0 = blocks(0)
    m1, s1 = blocks(1)
    z = np.abs(m0 - m1) / np.sqrt(s0 * s0 + s1 * s1 + 1e-12)
    print("z max %.3f, mean %.3f" % (float(z.max()), float(z.mean())))
    assert np.isfinite(m1).all() and (m1 > 0).all()
    return z


def test_cornell_with_its_light_and_the_sky_is_unbiased():
    import rtamd
    w, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, commit=False)
    _commit(w, dict(gradient=SKY), (0, 0))
    z = _block_compare(w, cam)
    assert z.max() < 5.0, float(z.max())


def test_nested_scene_under_the_sky_is_unbiased():
    w = _deferred_world()
    w, cam = ns.n1(w)
    _commit(w, dict(gradient=SKY), (0, 0))
    z = _block_compare(w, cam, W=48, H=32)
    assert z.max() < 5.0, float(z.max())


# ---- 5. it reduces noise where it should ---------------------------------------------------------------------------------------------
def _shadow_camera():
    import rtamd
    return rtamd.Camera(((0.0, 6.0, 8.0), (0.0, 0.5, 0.0)), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0)


def variance_ratio(w, cam, W=64, H=64, SPP=16, K=16):
    """per-pixel variance across K seeds, averaged over the floor pixels (luminance-free: all three channels): integrator 1 / integrator 0"""
    aov, _ = w.render_aov(cam, W, H, aov_spp=16, seed=1)
    floor = (aov[..., 7] == 1.0) & (aov[..., 1] == 1.0)  # every guide ray hit a surface whose normal is +y
    assert 0.5 < floor.mean() < 1.0
    var = []
    for integ in (1, 0):
        frames = np.array([w.render(cam, width=W, height=H, spp=SPP, seed=500 + k, integrator=integ)[0] for k in range(K)])
        var.append(float(frames.var(axis=0, ddof=1)[floor].mean()))
    return var[0] / var[1], var


def test_env_sampling_cuts_the_variance_of_the_sun_scene():
    """Measured on an MI355X: variance 0.00549 with env sampling against 0.1425 under integrator 0, ratio 0.0385; the
    figure is printed below.  The bound 0.5 was set before the measurement: cosine sampling finds the block with about one percent of
    its draws, so anything short of a large gain means the strategy is not working."""
    w = _floor_world(SUN, (0, 0), ball=True)
    ratio, var = variance_ratio(w, _shadow_camera())
    print("variance integrator 1 with env sampling %.6g, integrator 0 %.6g, ratio %.5f" % (var[0], var[1], ratio))
    assert ratio < 0.5


# ---- 6. inherited entry points --------------------------------------------------------------------------------------------------------
def test_entry_points_kernels_and_repeats_agree(tuning):
    import rtamd
    w = _floor_world(SUN, (0, 0), ball=True)
    cam = _shadow_camera()
    W, H, SPP = 44, 30, 8
    ref, st = w.render(cam, width=W, height=H, spp=SPP, seed=9, integrator=1)
    assert st["kernel_used"] == 2
    again, _ = w.render(cam, width=W, height=H, spp=SPP, seed=9, integrator=1)
    assert np.array_equal(again, ref)
    k1, st1 = w.render(cam, width=W, height=H, spp=SPP, seed=9, integrator=1, kernel=1)
    assert st1["kernel_used"] == 1 and np.array_equal(k1, ref)
    tuning(no_lds=1)  # the L2 variants
    for kernel in (1, 2):
        img, _ = w.render(cam, width=W, height=H, spp=SPP, seed=9, integrator=1, kernel=kernel)
        assert np.array_equal(img, ref), kernel
    tuning()
    off = _floor_world(SUN, None, ball=True)
    i0, _ = off.render(cam, width=W, height=H, spp=SPP, seed=9, integrator=0)
    assert not np.array_equal(i0, ref)
    e0, _ = w.render(cam, width=W, height=H, spp=SPP, seed=9, integrator=0)
    assert np.array_equal(e0, i0)  # integrator 0 does not know the switch
    p = rtamd.default_params(width=W, height=H, spp=SPP, seed=9, integrator=1)
    state = None
    for a, b in ((0, 3), (3, 5), (5, 8)):
        state, _ = w.render_accumulate(cam, p, a, b, state)
    assert np.array_equal(rtamd.accum_finalize(p, state), ref)
    img, tile_spp, _ = w.render_adaptive(cam, W, H, SPP, min_spp=2, threshold=0.0, seed=9, integrator=1)
    assert (tile_spp == SPP).all() and np.array_equal(img, ref)
    img, _ = w.render_multi(cam, devices=[0, 0], width=W, height=H, spp=SPP, seed=9, integrator=1)
    assert np.array_equal(img, ref)
    img, _ = w.render_camera_frame(cam.frame(), width=W, height=H, spp=SPP, seed=9, integrator=1)
    assert np.array_equal(img, ref)


# ---- 7. nothing else moved ------------------------------------------------------------------------------------------------------------
def _sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, dtype=np.float64).tobytes()).hexdigest()


def off_frames():
    """the frames tests/golden/env_sampling_off_frames.json pins (tests/golden/make_env_sampling_off_frames.py recorded them on the parent
    commit): Cornell + sky under integrator 1, and test_background_gpu.py's open scene under the sky, kernels 1 and 2"""
    import rtamd
    out = {}
    w, cam = rtamd.select_scene(scene_path("cube.obj"), 1.5, commit=False)
    w.set_background(gradient=SKY)
    w.commit()
    for kernel in (1, 2):
        out["cornell_sky_integrator1_kernel%d" % kernel] = _sha(w.render(cam, width=48, height=32, spp=8, seed=5, kernel=kernel, integrator=1)[0])
    w = _deferred_world()
    ball = w.Sphere((-1.2, 0.5, 0.0), 0.8, w.Lambertian(w.ConstantTexture((0.6, 0.5, 0.4))))
    lt = w.SphereDiffuseLight((0.0, 3.0, 12.0), 1.0, (4.0, 4.0, 4.0))
    w.new([ball, lt], lights=[lt], bvh_seed=1)
    w.set_background(gradient=SKY)
    rtamd.World.commit(w)
    cam = rtamd.Camera(((0.0, 1.0, 6.0), (0.0, 0.5, 0.0)), (0.0, 1.0, 0.0), 50.0, 1.5, 0.0, 10.0)
    for kernel in (1, 2):
        for integ in (0, 1):
            out["open_sky_integrator%d_kernel%d" % (integ, kernel)] = _sha(w.render(cam, width=36, height=24, spp=4, seed=3, kernel=kernel,
                                                                                   integrator=integ)[0])
    return out


def test_with_the_switch_off_the_frames_of_the_parent_commit_hold():
    pins = json.load(open(os.path.join(GOLDEN, "env_sampling_off_frames.json")))
    got = off_frames()
    assert sorted(got) == sorted(pins["frames"])
    for name, sha in got.items():
        assert sha == pins["frames"][name], name


@pytest.mark.parametrize("kernel", [1, 2])
def test_black_background_with_env_sampling_equals_the_frame_without(kernel):
    import rtamd
    frames = []
    for env in (None, (0, 0)):
        w, cam = rtamd.select_scene(scene_path("cube.obj"), 1.5, commit=False)
        _commit(w, dict(color=(0.0, 0.0, 0.0)), env)
        frames.append(w.render(cam, width=40, height=28, spp=4, seed=5, kernel=kernel, integrator=1)[0])
        if env is not None:
            assert not w.debug_env_table().any()
            assert not w.debug_env_sample(np.full((3, 4), 0.5)).any() and not w.debug_env_pdf(np.eye(3)).any()
    assert (frames[0] > 0).any() and np.array_equal(frames[0], frames[1])


def test_refusals():
    import rtamd
    cam = _shadow_camera()
    # without the switch integrator 1 still needs object lights, with a black table too
    for spec, env in ((SUN, None), (dict(kind=1, color=(0.0, 0.0, 0.0)), (0, 0))):
        w = _floor_world(spec, env, ball=True)
        with pytest.raises(rtamd.RtError) as e:
            w.render(cam, width=16, height=16, spp=2, integrator=1)
        assert e.value.code == -1 and "rt_scene_set_lights" in str(e.value)
    w = _floor_world(SUN, (0, 0), ball=True)
    for k in (5, 6):  # no env (and no background) variants of kernels 5 / 6
        with pytest.raises(rtamd.RtError) as e:
            w.render(cam, width=16, height=16, spp=2, integrator=1, kernel=k)
        assert e.value.code == -10 and "background" in str(e.value)
    with pytest.raises(rtamd.RtError) as e:
        w.render_sppm(cam, width=16, height=16, spp=2, iterations=1, photons_per_iter=1000)
    assert e.value.code == -10 and "background" in str(e.value)
    # a medium, and the book-2 kinds, stay with integrator 0
    m = _deferred_world()
    m.new([m.XZRectangle((-1000.0, -1000.0), (1000.0, 1000.0), 0.0, m.Lambertian(m.ConstantTexture(FLOOR_ALBEDO))),
           m.ConstantMedium(0.5, m.Sphere((0.0, 1.0, 0.0), 1.0, m.Lambertian(m.ConstantTexture((0.5, 0.5, 0.5)))),
                            m.Isotropic(m.ConstantTexture((0.9, 0.9, 0.9))))])
    _commit(m, _bg_kwargs(m, SUN), (0, 0))
    with pytest.raises(rtamd.RtError) as e:
        m.render(cam, width=16, height=16, spp=2, integrator=1)
    assert e.value.code == -10 and "ConstantMedium" in str(e.value)
    b = _deferred_world()
    b.new([b.XZRectangle((-1000.0, -1000.0), (1000.0, 1000.0), 0.0, b.Lambertian(b.NoiseTexture(0.5))),
           b.Sphere((0.0, 1.0, 0.0), 1.0, b.Lambertian(b.ConstantTexture((0.5, 0.5, 0.5))))])
    _commit(b, _bg_kwargs(b, SUN), (0, 0))
    with pytest.raises(rtamd.RtError) as e:
        b.render(cam, width=16, height=16, spp=2, integrator=1)
    assert e.value.code == -10 and "book-2" in str(e.value)
    # the diagnostics want a scene that enabled it
    off = _floor_world(SUN, None)
    with pytest.raises(rtamd.RtError) as e:
        off.debug_env_table()
    assert e.value.code == -1
