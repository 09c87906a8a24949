"""The denoiser on the GPU.  Guide buffers (rt_render_aov) against the oracle bit for bit: the camera rays of samples 0 .. aov_spp-1
(oracle.camera_rays), their closest hits (hit_batch), the albedo of the hit object's material (its constant texture, or oracle.scatter's
attenuation / emission for textured ones), summed in sample order and divided as the kernel does.  The a-trous filter (rt_denoise,
rt_denoise_device) against tests/denoise_ref.py bit for bit.  render_denoised: its noisy frame is render()'s, and it brings a 32-spp Cornell
frame closer to a 4096-spp one.  Refusals of scenes with media and moving spheres."""
import os
import sys

import numpy as np
import pytest

import denoise_ref
import nested_scenes as ns
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu

T_MIN = 1e-3


# ---- which object a ray hit, and its material: the oracle's builder calls are recorded while a scene is built ----------------------
class _Record:
    def __init__(self):
        self.tex, self.mat, self.prims = {}, {}, []


def _recorded(build):
    """build() with oracle.Scene's texture / material / primitive constructors recorded -> (its result, _Record)"""
    import oracle
    rec = _Record()
    hooks = {
        "ConstantTexture": lambda r, c: rec.tex.__setitem__(r, tuple(float(x) for x in c)),
        "Lambertian": lambda r, t: rec.mat.__setitem__(r, ("lambertian", t)),
        "Metal": lambda r, t, fuzz: rec.mat.__setitem__(r, ("metal", t)),
        "Dielectric": lambda r, ir, t: rec.mat.__setitem__(r, ("dielectric", t)),
        "DiffuseLight": lambda r, t: rec.mat.__setitem__(r, ("light", t)),
        "Sphere": lambda r, c, rad, m: rec.prims.append(("sphere", np.array(c, dtype=float), float(rad), m)),
        "XYRectangle": lambda r, a, b, k, m: rec.prims.append(("rect", 2, (0, 1), a, b, float(k), m)),
        "XZRectangle": lambda r, a, b, k, m: rec.prims.append(("rect", 1, (0, 2), a, b, float(k), m)),
        "YZRectangle": lambda r, a, b, k, m: rec.prims.append(("rect", 0, (1, 2), a, b, float(k), m)),
        "Cube": lambda r, mn, mx, m: rec.prims.append(("cube", np.array(mn, dtype=float), np.array(mx, dtype=float), m)),
    }
    saved = {}
    for name, hook in hooks.items():
        saved[name] = getattr(oracle.Scene, name)

        def spy(self, *a, _f=saved[name], _h=hook, **k):
            r = _f(self, *a, **k)
            _h(r, *a, **k)
            return r
        setattr(oracle.Scene, name, spy)
    try:
        return build(), rec
    finally:
        for name, f in saved.items():
            setattr(oracle.Scene, name, f)


def _which(rec, p):
    """index into rec.prims of the world-space primitive whose surface each point p [n, 3] lies on (-1: none of them -- an object under
    a Transform or inside a mesh); the first of equally close ones"""
    best = np.full(len(p), -1)
    bd = np.full(len(p), 1e-7)
    for i, pr in enumerate(rec.prims):
        if pr[0] == "sphere":
            d = np.abs(np.linalg.norm(p - pr[1], axis=1) - pr[2]) / max(pr[2], 1.0)
        elif pr[0] == "rect":
            _, k_ax, (a_ax, b_ax), a, b, k, _ = pr
            inside = (p[:, a_ax] >= a[0] - 1e-9) & (p[:, a_ax] <= b[0] + 1e-9) & (p[:, b_ax] >= a[1] - 1e-9) & (p[:, b_ax] <= b[1] + 1e-9)
            d = np.where(inside, np.abs(p[:, k_ax] - k) / max(abs(k), 1.0), np.inf)
        else:
            mn, mx = pr[1], pr[2]
            inside = np.all((p >= mn - 1e-7) & (p <= mx + 1e-7), axis=1)
            d = np.where(inside, np.min(np.minimum(np.abs(p - mn), np.abs(p - mx)), axis=1) / max(np.abs(mx).max(), 1.0), np.inf)
        take = d < bd
        best[take], bd[take] = i, d[take]
    return best


def _albedo(sc, rec, rays, hits, default_mat):
    """[n, 3]: the texture value of the hit object's material at the hit (rays [n, 6], hits [n, 12] oracle records)"""
    which = _which(rec, hits[:, 2:5])
    out = np.zeros((len(hits), 3))
    for i in np.unique(which):
        m = default_mat if i < 0 else rec.prims[i][-1]
        kind, tex = rec.mat[m]
        sel = np.nonzero(which == i)[0]
        if tex in rec.tex:
            out[sel] = rec.tex[tex]
            continue
        assert kind in ("lambertian", "light"), "textured %s: the test reads the albedo of Lambertian and DiffuseLight only" % kind
        for j in sel:
            h = hits[j]
            s = sc.scatter(m, rays[j, :3], rays[j, 3:], h[2:5], h[5:8], h[8] != 0.0, uv=(h[9], h[10]))
            out[j] = s["attenuation"] if kind == "lambertian" else s["emitted"]
    return out


def _expected_aov(sc, rec, width, height, aov_spp, seed, default_mat):
    sums = np.zeros((height, width, 7))
    hits = np.zeros((height, width))
    for s in range(aov_spp):
        rays = sc.camera_rays(width, height, seed=seed, sample=s).reshape(-1, 6)
        r = sc.hit_batch(rays, t_min=T_MIN)
        hit = r[:, 0] != 0.0
        vals = np.zeros((len(r), 7))
        vals[:, 0:3] = r[:, 5:8]
        vals[:, 3] = r[:, 1]
        vals[hit, 4:7] = _albedo(sc, rec, rays[hit], r[hit], default_mat)
        sums.reshape(-1, 7)[hit] += vals[hit]
        hits.reshape(-1)[hit] += 1.0
    out = np.zeros((height, width, 8))
    m = hits > 0
    out[m, :7] = sums[m] / hits[m][:, None]
    out[m, 7] = hits[m] / float(aov_spp)
    return out


def _textured(B):
    """checker, image and noise textures on Lambertian spheres, an image-textured light, a glass and a metal ball"""
    yy, xx = np.mgrid[0:16, 0:24]
    img = np.stack([(xx * 10) % 256, (yy * 15) % 256, ((xx + yy) * 7) % 256], axis=2).astype(np.uint8)
    checker = B.Lambertian(B.CheckerTexture(B.ConstantTexture((0.2, 0.3, 0.1)), B.ConstantTexture((0.9, 0.9, 0.9))))
    image = B.Lambertian(B.ImageTexture(img))
    marble = B.Lambertian(B.NoiseTexture(4.0, 7) if ns.is_oracle(B) else B.NoiseTexture(4.0, seed=7))
    glow = B.DiffuseLight(B.ImageTexture(img[::-1].copy()))
    glass = B.Dielectric(1.5, B.ConstantTexture((0.9, 0.95, 1.0)))
    metal = B.Metal(B.ConstantTexture((0.8, 0.6, 0.3)), 0.2)
    items = [B.Sphere((0.0, -1000.0, 0.0), 1000.0, checker), B.Sphere((0.0, 1.0, 0.0), 1.0, image), B.Sphere((-2.2, 1.0, 0.3), 1.0, marble),
             B.Sphere((2.2, 1.0, -0.3), 1.0, glow), B.Sphere((1.0, 0.4, 1.6), 0.4, glass), B.Sphere((-1.0, 0.35, 1.8), 0.35, metal)]
    return ns.finish(B, items, seed=3, cam=((0.0, 2.5, 7.0), (0.0, 0.8, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.05, 7.0))


def _scene(name):
    """-> (world, camera, oracle scene, record, width, height, material of hits on no world-space primitive)"""
    import rtamd
    if name in ("cornell", "scene_10"):
        w, cam = configs.product(name)
        sc, rec = _recorded(lambda: configs.oracle_scene(name))
        W, H = (40, 40) if name == "cornell" else (64, 36)
    elif name == "textured":
        w, cam = _textured(rtamd.World())
        sc, rec = _recorded(lambda: _textured(__import__("oracle").Scene()))
        W, H = 60, 40
    else:  # a nested-Transform scene: Cornell walls and light around white cubes under two levels of Transforms
        w, cam = ns.SCENES[name](rtamd.World())
        sc, rec = _recorded(lambda: ns.SCENES[name](__import__("oracle").Scene()))
        W, H = 48, 32
    # hits on no world-space primitive: the mesh cube of Cornell, the Transformed cubes of n1 -- white in both
    white = [m for m, (kind, t) in rec.mat.items() if kind == "lambertian" and rec.tex.get(t) == (0.75, 0.75, 0.75)]
    return w, cam, sc, rec, W, H, (white[0] if white else None)


_SCENES = {}


def _cached(name):
    if name not in _SCENES:
        _SCENES[name] = _scene(name)
    return _SCENES[name]


@pytest.mark.parametrize("aov_spp", [1, 3])
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("name", ["cornell", "scene_10", "textured", "n1"])
def test_guides_match_the_oracle(name, kernel, aov_spp):
    w, cam, sc, rec, W, H, default_mat = _cached(name)
    got, st = w.render_aov(cam, W, H, aov_spp=aov_spp, seed=5, kernel=kernel)
    assert st["kernel_used"] == kernel and st["samples"] == W * H * aov_spp
    exp = _expected_aov(sc, rec, W, H, aov_spp, 5, default_mat)
    assert (exp[..., 7] > 0).mean() > 0.25, "a good part of the frame should hit something"
    bad = np.argwhere(np.any(got != exp, axis=2))
    assert bad.size == 0, "%d / %d pixels differ, first (y, x) %s: got %s expected %s" % (
        len(bad), W * H, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def test_guides_automatic_walk_is_kernel_2_and_agrees():
    w, cam, _, _, W, H, _ = _cached("cornell")
    a, st = w.render_aov(cam, W, H, aov_spp=2, seed=9)
    b, _ = w.render_aov(cam, W, H, aov_spp=2, seed=9, kernel=1)
    assert st["kernel_used"] == 2 and np.array_equal(a, b)


# ---- the filter --------------------------------------------------------------------------------------------------------------------
def _random_inputs(h=23, w=37, seed=1):
    rng = np.random.default_rng(seed)
    c = rng.gamma(2.0, 0.3, size=(h, w, 3))
    v = rng.gamma(1.0, 0.02, size=(h, w))
    g = np.zeros((h, w, 8))
    n = rng.standard_normal((h, w, 3))
    g[..., 0:3] = n / np.linalg.norm(n, axis=2, keepdims=True)
    g[..., 3] = rng.uniform(1.0, 3.0, size=(h, w))
    g[..., 4:7] = rng.random((h, w, 3))
    g[..., 7] = 1.0
    g[rng.random((h, w)) < 0.1] = 0.0  # pixels without a hit
    return c, v, g


def _check(got, exp, what):
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d values differ, first at %s: %r vs %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("with_variance", [False, True])
@pytest.mark.parametrize("guides", [None, 0, 1, 2, 3, 4, 5, 6, 7])
def test_filter_matches_the_numpy_restatement(guides, with_variance, iterations):
    import rtamd
    c, v, g = _random_inputs()
    aov = None if guides is None else g
    cfg = dict(iterations=iterations) if guides is None else dict(iterations=iterations, guides=guides)
    exp_c, exp_v = denoise_ref.denoise(c, v if with_variance else None, aov, **cfg)
    if with_variance:
        got_c, got_v = rtamd.denoise(c, v, aov, return_variance=True, **cfg)
        _check(got_v, exp_v, "variance")
    else:
        got_c = rtamd.denoise(c, None, aov, **cfg)
    _check(got_c, exp_c, "colour")


def test_filter_settings_and_tiny_images_match():
    import rtamd
    c, v, g = _random_inputs(h=5, w=3, seed=4)  # steps beyond the image at every pass after the first two
    cfg = dict(iterations=8, normal_power_log2=0, sigma_depth=0.25, sigma_albedo=2.0, sigma_luma=0.5, eps=1e-3)
    exp_c, exp_v = denoise_ref.denoise(c, v, g, **cfg)
    got_c, got_v = rtamd.denoise(c, v, g, return_variance=True, **cfg)
    _check(got_c, exp_c, "colour")
    _check(got_v, exp_v, "variance")
    one = rtamd.denoise(c[:1, :1], v[:1, :1], g[:1, :1])
    assert np.array_equal(one, c[:1, :1])


@pytest.mark.parametrize("with_variance", [False, True])
def test_device_entry_point_agrees_with_the_host_one(with_variance):
    import torch
    import rtamd
    c, v, g = _random_inputs(h=41, w=29, seed=8)
    host_c, host_v = rtamd.denoise(c, v, g, return_variance=True) if with_variance else (rtamd.denoise(c, None, g), None)
    dev = torch.device("cuda", 0)
    tc, tv, tg = (torch.from_numpy(x).to(dev) for x in (c, v, g))
    oc, ov = torch.zeros_like(tc), torch.zeros_like(tv)
    stream = torch.cuda.current_stream(dev)
    rtamd.denoise_device(29, 41, tc.data_ptr(), oc.data_ptr(), d_variance_ptr=tv.data_ptr() if with_variance else None, d_aov_ptr=tg.data_ptr(),
                         d_out_variance_ptr=ov.data_ptr() if with_variance else None, stream_ptr=stream.cuda_stream)
    torch.cuda.synchronize(dev)
    _check(oc.cpu().numpy(), host_c, "device colour")
    if with_variance:
        _check(ov.cpu().numpy(), host_v, "device variance")


def test_filter_of_a_rendered_cornell_frame_matches():
    import rtamd
    w, cam = configs.product("cornell")
    den, noisy, var, aov = w.render_denoised(cam, width=48, height=48, spp=8, aov_spp=2, integrator=0)
    exp_c, _ = denoise_ref.denoise(noisy, var, aov)
    _check(den, exp_c, "Cornell frame")
    got_c, got_v = rtamd.denoise(noisy, var, aov, return_variance=True)
    _check(got_c, den, "rt_denoise vs render_denoised")
    _check(got_v, denoise_ref.denoise(noisy, var, aov)[1], "Cornell variance")


# ---- render_denoised ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", [0, 1])
def test_noisy_frame_is_the_render_frame(integrator):
    w, cam = configs.product("cornell")
    _, noisy, var, aov = w.render_denoised(cam, width=40, height=40, spp=6, seed=3, integrator=integrator)
    img, _ = w.render(cam, width=40, height=40, spp=6, seed=3, integrator=integrator)
    assert np.array_equal(noisy, img)
    assert var.shape == (40, 40) and np.all(var >= 0.0) and aov.shape == (40, 40, 8)


def test_denoised_cornell_is_closer_to_a_converged_frame():
    """Cornell 128 x 128, light sampling, 32 spp, the default filter: the filtered frame's MSE against a 4096-spp frame of another seed,
    over the noisy frame's MSE.  Measured on an MI355X: 0.619, and the frame's mean moves down by 8.0 % (the luminance
    stop, fed by a two-half variance estimate, keeps dark pixels whose halves agree and averages away the bright samples of the others).
    The bounds hold those measurements with a margin; the filter is deterministic, so a change of either number is a change of the code."""
    w, cam = configs.product("cornell")
    den, noisy, _, _ = w.render_denoised(cam, width=128, height=128, spp=32, seed=1, integrator=1)
    ref, _ = w.render(cam, width=128, height=128, spp=4096, seed=2, integrator=1)
    mse_noisy = float(np.mean((noisy - ref) ** 2))
    mse_den = float(np.mean((den - ref) ** 2))
    ratio = mse_den / mse_noisy
    shift = abs(float(den.mean()) / float(noisy.mean()) - 1.0)
    print("\ndenoise quality: MSE noisy %.6g, denoised %.6g, ratio %.4f; mean shift %.4f %%" % (mse_noisy, mse_den, ratio, 100 * shift))
    assert ratio <= 0.65
    assert shift <= 0.09


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n5", "n6"])  # n5: a moving sphere; n6: ConstantMedium objects
def test_guides_refuse_moving_spheres_and_media(name):
    import rtamd
    w, cam = ns.SCENES[name](rtamd.World())
    for kernel in (0, 1):
        with pytest.raises(rtamd.RtError) as e:
            w.render_aov(cam, 16, 16, aov_spp=1, kernel=kernel)
        assert e.value.code == -10
        assert ("moving spheres" if name == "n5" else "ConstantMedium") in str(e.value)


def test_media_scene_denoises_on_colour_and_variance_alone():
    import rtamd
    w, cam = configs.product("c5r")
    with pytest.raises(rtamd.RtError) as e:
        w.render_aov(cam, 32, 32, aov_spp=1)
    assert e.value.code == -10
    den, noisy, var, aov = w.render_denoised(cam, width=64, height=64, spp=4, guides=False)
    assert aov is None and np.all(np.isfinite(den))
    img, _ = w.render(cam, width=64, height=64, spp=4)
    assert np.array_equal(noisy, img)
    _check(den, denoise_ref.denoise(noisy, var, None)[0], "C5r colour-only filter")
