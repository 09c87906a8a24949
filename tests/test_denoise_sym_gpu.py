"""The energy-preserving denoise mode and the one-call denoised render on the GPU.  rt_denoise_sym / rt_denoise_sym_device against
tests/denoise_sym_ref.py bit for bit; rt_denoised_render with luma_mode 0 against the Python composition World.render_denoised(native=False)
bit for bit in all four outputs, with luma_mode 1 against the restatement applied to the call's own outputs; the device form against the
host form; the quality the denoiser was first specified with (MSE ratio <= 0.5 at a mean shift within 2 %); the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import denoise_ref
import denoise_sym_ref
import nested_scenes as ns
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu


def _random_inputs(h=23, w=37, seed=1):
    """as test_denoise_gpu._random_inputs, with some variances exactly 0"""
    rng = np.random.default_rng(seed)
    c = rng.gamma(2.0, 0.3, size=(h, w, 3))
    v = rng.gamma(1.0, 0.02, size=(h, w))
    v[rng.random((h, w)) < 0.15] = 0.0
    g = np.zeros((h, w, 8))
    n = rng.standard_normal((h, w, 3))
    g[..., 0:3] = n / np.linalg.norm(n, axis=2, keepdims=True)
    g[..., 3] = rng.uniform(1.0, 3.0, size=(h, w))
    g[..., 4:7] = rng.random((h, w, 3))
    g[..., 7] = 1.0
    g[rng.random((h, w)) < 0.1] = 0.0  # pixels without a hit
    return c, v, g


def _check(got, exp, what):
    assert got.shape == exp.shape, what
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d values differ, first at %s: %r vs %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


_WORLDS = {}


def _world(name):
    if name not in _WORLDS:
        _WORLDS[name] = configs.product(name)
    return _WORLDS[name]


# ---- 1-4: the filter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("guides", [None, 0, 7])
def test_symmetric_filter_matches_the_numpy_restatement(guides, iterations):
    import rtamd
    c, v, g = _random_inputs()
    assert (v == 0.0).sum() > 50
    aov = None if guides is None else g
    cfg = dict(iterations=iterations) if guides is None else dict(iterations=iterations, guides=guides)
    exp_c, exp_v = denoise_sym_ref.denoise(c, v, aov, **cfg)
    got_c, got_v = rtamd.denoise(c, v, aov, return_variance=True, symmetric=True, **cfg)
    _check(got_c, exp_c, "colour")
    _check(got_v, exp_v, "variance")
    assert not np.array_equal(got_c, rtamd.denoise(c, v, aov, **cfg))  # (it is another filter than rt_denoise)


def test_symmetric_filter_on_a_tiny_image_with_taps_outside():
    import rtamd
    c, v, g = _random_inputs(h=5, w=3, seed=4)  # 8 iterations: steps beyond the image at every pass after the first two
    cfg = dict(iterations=8, normal_power_log2=0, sigma_depth=0.25, sigma_albedo=2.0, sigma_luma=0.5, eps=1e-3)
    exp_c, exp_v = denoise_sym_ref.denoise(c, v, g, **cfg)
    got_c, got_v = rtamd.denoise(c, v, g, return_variance=True, symmetric=True, **cfg)
    _check(got_c, exp_c, "colour")
    _check(got_v, exp_v, "variance")


def test_one_pixel_comes_back():
    import rtamd
    c, v, g = _random_inputs(h=5, w=3, seed=4)
    one, one_v = rtamd.denoise(c[:1, :1], v[:1, :1], g[:1, :1], return_variance=True, symmetric=True)
    assert np.array_equal(one, c[:1, :1])
    _check(one_v, denoise_sym_ref.denoise(c[:1, :1], v[:1, :1], g[:1, :1])[1], "variance of one pixel")


def test_symmetric_device_entry_point_agrees_with_the_host_one():
    import torch
    import rtamd
    c, v, g = _random_inputs(h=41, w=29, seed=8)
    host_c, host_v = rtamd.denoise(c, v, g, return_variance=True, symmetric=True)
    dev = torch.device("cuda", 0)
    tc, tv, tg = (torch.from_numpy(x).to(dev) for x in (c, v, g))
    oc, ov = torch.zeros_like(tc), torch.zeros_like(tv)
    stream = torch.cuda.current_stream(dev)
    rtamd.denoise_device(29, 41, tc.data_ptr(), oc.data_ptr(), d_variance_ptr=tv.data_ptr(), d_aov_ptr=tg.data_ptr(), d_out_variance_ptr=ov.data_ptr(),
                         stream_ptr=stream.cuda_stream, symmetric=True)
    torch.cuda.synchronize(dev)
    _check(oc.cpu().numpy(), host_c, "device colour")
    _check(ov.cpu().numpy(), host_v, "device variance")
    with pytest.raises(rtamd.RtError) as e:
        rtamd.denoise_device(29, 41, tc.data_ptr(), oc.data_ptr(), symmetric=True)
    assert e.value.code == -1


# ---- 5-7: the one call ----------------------------------------------------------------------------------------------------------------
CASES = {
    "cornell-i0": ("cornell", dict(width=40, height=40, spp=6, aov_spp=2, integrator=0, seed=3)),
    "cornell-i1": ("cornell", dict(width=40, height=40, spp=6, aov_spp=2, integrator=1, seed=3)),
    "cornell-ragged": ("cornell", dict(width=37, height=21, spp=2, aov_spp=1)),          # ragged edge tiles, half = 1
    "c5r-media": ("c5r", dict(width=64, height=64, spp=4, guides=False)),                # a ConstantMedium: colour and variance alone
}
_NATIVE = {}


def _native(case, luma_mode):
    if (case, luma_mode) not in _NATIVE:
        scene, kw = CASES[case]
        w, cam = _world(scene)
        _NATIVE[(case, luma_mode)] = w.render_denoised(cam, native=True, luma_mode=luma_mode, **kw)
    return _NATIVE[(case, luma_mode)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_luma_mode_0_is_the_python_composition_bit_for_bit(case):
    scene, kw = CASES[case]
    w, cam = _world(scene)
    exp = w.render_denoised(cam, native=False, **kw)
    got = _native(case, 0)
    for name, g, e in zip(("denoised", "noisy", "variance", "aov"), got, exp):
        if e is None:
            assert g is None and name == "aov" and not kw.get("guides", True)
        else:
            _check(g, e, "%s: %s" % (case, name))
    img, _ = w.render(cam, **{k: v for k, v in kw.items() if k not in ("aov_spp", "guides")})
    _check(got[1], img, "%s: noisy vs render()" % case)
    assert np.any(got[2] > 0.0) and np.all(got[2] >= 0.0)


@pytest.mark.parametrize("case", sorted(CASES))
def test_luma_mode_1_is_the_restatement_of_its_own_outputs(case):
    den, noisy, var, aov = _native(case, 1)
    _check(noisy, _native(case, 0)[1], "%s: the noisy frame does not depend on the mode" % case)
    _check(var, _native(case, 0)[2], "%s: nor does the variance" % case)
    exp, _ = denoise_sym_ref.denoise(noisy, var, aov)
    _check(den, exp, "%s: denoised" % case)
    assert not np.array_equal(den, _native(case, 0)[0])


def test_settings_reach_the_filter_and_null_config_is_the_default():
    import rtamd
    w, cam = _world("cornell")
    kw = dict(CASES["cornell-i1"][1])
    den, noisy, var, aov = w.render_denoised(cam, native=True, luma_mode=1, sigma_luma=2.0, iterations=3, normal_power_log2=2, **kw)
    _check(den, denoise_sym_ref.denoise(noisy, var, aov, sigma_luma=2.0, iterations=3, normal_power_log2=2)[0], "sigma_luma 2, 3 passes, n.n'^4")
    p = rtamd.default_params(width=40, height=40, spp=6, seed=3, integrator=1)
    out = np.zeros((40, 40, 3))
    st = rtamd.rt_stats()
    rc = w.L.rt_denoised_render(w.h, C.byref(cam.c), C.byref(p), None, 1, 2, out.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, C.byref(st))
    assert rc == 0
    _check(out, _native("cornell-i1", 1)[0], "NULL config, optional outputs NULL")
    assert st.samples == 40 * 40 * 6 and st.launches >= 2 and st.kernel_ms > 0.0 and st.seconds > 0.0 and st.kernel_used in (1, 2, 5)


@pytest.mark.parametrize("case", ["cornell-i1", "cornell-ragged", "c5r-media"])
def test_device_form_equals_the_host_form(case):
    import torch
    import rtamd
    scene, kw = CASES[case]
    w, cam = _world(scene)
    W, H = kw["width"], kw["height"]
    guides = kw.get("guides", True)
    p = rtamd.default_params(width=W, height=H, spp=kw["spp"], seed=kw.get("seed", 1), integrator=kw.get("integrator", 0))
    dev = torch.device("cuda", 0)
    nan = float("nan")
    den, noisy = torch.full((H, W, 3), nan, dtype=torch.float64, device=dev), torch.full((H, W, 3), nan, dtype=torch.float64, device=dev)
    var, aov = torch.full((H, W), nan, dtype=torch.float64, device=dev), torch.full((H, W, 8), nan, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    st = w.render_denoised_device(cam, p, den.data_ptr(), noisy.data_ptr(), var.data_ptr(), aov.data_ptr() if guides else None,
                                  aov_spp=kw.get("aov_spp", 4) if guides else 0, luma_mode=1, stream_ptr=stream.cuda_stream)
    torch.cuda.synchronize(dev)
    exp = _native(case, 1)
    _check(den.cpu().numpy(), exp[0], "denoised")
    _check(noisy.cpu().numpy(), exp[1], "noisy")
    _check(var.cpu().numpy(), exp[2], "variance")
    if guides:
        _check(aov.cpu().numpy(), exp[3], "aov")
    assert st["samples"] == W * H * kw["spp"]
    only = torch.full((H, W, 3), nan, dtype=torch.float64, device=dev)  # the optional outputs left out
    w.render_denoised_device(cam, p, only.data_ptr(), aov_spp=kw.get("aov_spp", 4) if guides else 0, luma_mode=1, stream_ptr=stream.cuda_stream)
    torch.cuda.synchronize(dev)
    _check(only.cpu().numpy(), exp[0], "denoised alone")


@pytest.mark.parametrize("flags, aov_spp, luma_mode", [((), 4, 1), (("--aov-spp", "2", "--luma-mode", "0"), 2, 0)])
def test_cpp_host_writes_the_denoised_frame(tmp_path, flags, aov_spp, luma_mode):
    """rtamd_render --denoise (World::render_denoised of rtamd.hpp over rt_denoised_render): the PNG is the tone-mapped frame of the
    Python call with the same arguments (the C++ Cornell box is select_scene's)"""
    import subprocess
    import rtamd
    from PIL import Image
    out = str(tmp_path / "denoised.png")
    exe = os.path.join(ROOT, "rust-raytracer_amd", "rtamd_render")
    cube = os.path.join(ROOT, "tests", "golden", "scenes", "cube.obj")
    r = subprocess.run([exe, "--cube", cube, "-w", "40", "-h", "40", "--spp", "6", "--seed", "3", "--integrator", "1", "--denoise", *flags, "-o", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "denoised (luma mode %d, %d guide rays per pixel): 9600 samples" % (luma_mode, aov_spp) in r.stdout, r.stdout + r.stderr
    w, cam = _world("cornell")
    exp = w.render_denoised(cam, width=40, height=40, spp=6, seed=3, integrator=1, aov_spp=aov_spp, native=True, luma_mode=luma_mode)[0]
    assert np.array_equal(np.asarray(Image.open(out)), rtamd.tonemap_u8(exp))
    r = subprocess.run([exe, "--cube", cube, "-w", "16", "-h", "16", "--spp", "5", "--denoise", "-o", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "error -1" in r.stderr                      # odd spp


# ---- 8: quality -----------------------------------------------------------------------------------------------------------------------
# the CPU restatement over oracle frames and guides (bit-exact with the GPU's), Cornell 128 x 128, 32 spp seed 1 against 4096 spp seed 2,
# sigma_luma 2: (MSE ratio, mean shift) to the digits it printed
EXPECTED = {1: (0.448, 0.0012), 0: (0.353, -0.0069)}


@pytest.mark.parametrize("integrator", [1, 0])
def test_symmetric_stop_reaches_the_quality_the_denoiser_was_specified_with(integrator):
    """MSE ratio <= 0.5 and |mean shift| <= 2 %: the two numbers DESIGN.md s4e says the denoiser was first specified with and, with
    rt_denoise's one-sided stop, never reached together (0.619 at -8.0 % under integrator 1; 0.617 at -31.2 % under integrator 0 at
    sigma_luma 2).  The filter is deterministic: the values equal the CPU restatement's to the digits it printed."""
    w, cam = _world("cornell")
    kw = dict(width=128, height=128, spp=32, seed=1, integrator=integrator)
    den, noisy, _, _ = w.render_denoised(cam, native=True, luma_mode=1, sigma_luma=2.0, **kw)
    old, old_noisy, _, _ = w.render_denoised(cam, native=False, sigma_luma=2.0, **kw)
    _check(noisy, old_noisy, "noisy")
    ref, _ = w.render(cam, width=128, height=128, spp=4096, seed=2, integrator=integrator)
    mse_noisy = float(np.mean((noisy - ref) ** 2))

    def figures(img):
        return float(np.mean((img - ref) ** 2)) / mse_noisy, float(img.mean()) / float(noisy.mean()) - 1.0
    ratio, shift = figures(den)
    old_ratio, old_shift = figures(old)
    print("\ndenoise quality, integrator %d, sigma_luma 2: symmetric stop MSE ratio %.4f, mean shift %+.3f %%; rt_denoise's stop %.4f, %+.3f %%"
          % (integrator, ratio, 100 * shift, old_ratio, 100 * old_shift))
    assert ratio <= 0.5
    assert abs(shift) <= 0.02
    exp_ratio, exp_shift = EXPECTED[integrator]
    assert abs(ratio - exp_ratio) < 5e-4 and abs(shift - exp_shift) < 5e-5


# ---- 9: refusals ----------------------------------------------------------------------------------------------------------------------
def test_kernel_6_integrator_2_and_odd_spp_are_refused():
    import rtamd
    w, cam = _world("cornell")
    for bad in (dict(kernel=6), dict(integrator=2)):
        with pytest.raises(rtamd.RtError) as e:
            w.render_denoised(cam, width=16, height=16, spp=2, native=True, **bad)
        assert e.value.code == -10, bad
    p = rtamd.default_params(width=16, height=16, spp=3)
    out = np.zeros((16, 16, 3))
    assert w.L.rt_denoised_render(w.h, C.byref(cam.c), C.byref(p), None, 1, 0, out.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None) == -1


@pytest.mark.parametrize("name", ["n5", "n6"])  # n5: a moving sphere; n6: ConstantMedium objects
def test_guides_of_scenes_with_moving_spheres_or_media_are_refused(name):
    import rtamd
    w, cam = ns.SCENES[name](rtamd.World())
    with pytest.raises(rtamd.RtError) as e:
        w.render_denoised(cam, width=16, height=16, spp=2, aov_spp=1, native=True)
    assert e.value.code == -10
    assert ("moving spheres" if name == "n5" else "ConstantMedium") in str(e.value)
    den, noisy, var, aov = w.render_denoised(cam, width=16, height=16, spp=2, guides=False, native=True)  # such scenes pass aov_spp = 0
    assert aov is None and np.all(np.isfinite(den))
    _check(noisy, w.render(cam, width=16, height=16, spp=2)[0], "noisy")
