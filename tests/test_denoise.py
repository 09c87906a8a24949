"""The a-trous denoiser and its guide buffers without a GPU: the numpy restatement's own properties (tests/denoise_ref.py), the
validation of rt_denoise_config and of the arguments of rt_denoise / rt_denoise_device / rt_render_aov through the C ABI, and the new
symbols in the header, the Python binding, the Rust FFI file and the C++ wrapper."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rtamd.h")
NEW_SYMBOLS = ("rt_render_aov", "rt_default_denoise_config", "rt_denoise", "rt_denoise_device")


def _guides(h, w, normal, depth=5.0, albedo=(0.5, 0.5, 0.5)):
    g = np.zeros((h, w, 8))
    g[..., 0:3] = normal
    g[..., 3] = depth
    g[..., 4:7] = albedo
    g[..., 7] = 1.0
    return g


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 5, 8])
def test_constant_image_with_constant_guides_comes_back(iterations):
    h, w = 23, 37
    c = np.empty((h, w, 3))
    c[...] = (0.3, 0.55, 0.9)
    v = np.full((h, w), 0.01)
    out, vo = denoise_ref.denoise(c, v, _guides(h, w, (0.0, 0.0, 1.0)), iterations=iterations)
    assert np.max(np.abs(out - c)) <= 1e-15
    assert np.all(vo > 0.0) and np.all(vo <= 0.01)  # averaging shrinks the variance of the mean


def test_flat_regions_with_perpendicular_normals_do_not_mix():
    h, w = 24, 32
    g = _guides(h, w, (0.0, 0.0, 1.0))
    g[:, w // 2:, 0:3] = (1.0, 0.0, 0.0)  # right half faces another way
    rng = np.random.default_rng(3)
    c = np.empty((h, w, 3))
    c[:, : w // 2] = 0.2 + 0.05 * rng.standard_normal((h, w // 2, 3))
    c[:, w // 2:] = 0.8 + 0.05 * rng.standard_normal((h, w - w // 2, 3))
    out, _ = denoise_ref.denoise(c, None, g, iterations=5)
    left, right = out[:, : w // 2], out[:, w // 2:]
    assert left.max() < c[:, : w // 2].max() + 1e-12 and right.min() > c[:, w // 2:].min() - 1e-12  # no tap crossed the edge
    assert left.std() < c[:, : w // 2].std() and right.std() < c[:, w // 2:].std()                  # and each side was smoothed


def test_without_guides_the_filter_is_a_plain_b3_blur():
    """no variance and no aov: every factor is 1, one pass at step 1 is the separable B3 kernel renormalised at the border"""
    rng = np.random.default_rng(5)
    c = rng.random((9, 11, 3))
    out, v = denoise_ref.denoise(c, iterations=1)
    assert v is None
    k = np.array(denoise_ref.H[::-1][:2] + denoise_ref.H)  # 1/16, 1/4, 3/8, 1/4, 1/16
    y, x = 4, 5
    patch = c[y - 2:y + 3, x - 2:x + 3]
    exp = np.einsum("i,j,ijc->c", k, k, patch)
    assert np.allclose(out[y, x], exp, rtol=0, atol=1e-15)


def test_guide_selection_masks_factors():
    """guides = 0 with an aov is the same filter as no aov at all"""
    rng = np.random.default_rng(11)
    c, v, g = rng.random((13, 17, 3)), rng.random((13, 17)) * 0.1, rng.random((13, 17, 8))
    a = denoise_ref.denoise(c, v, g, guides=0)
    b = denoise_ref.denoise(c, v, None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_default_config_matches_the_documented_defaults():
    import rtamd
    c = rtamd.denoise_config()
    for k, v in denoise_ref.DEFAULTS.items():
        assert getattr(c, k) == v, k
    assert list(c.reserved) == [0] * 5
    assert C.sizeof(rtamd.rt_denoise_config) == 64


BAD_CONFIGS = [dict(iterations=0), dict(iterations=9), dict(normal_power_log2=-1), dict(normal_power_log2=17), dict(sigma_depth=0.0),
               dict(sigma_albedo=-1.0), dict(sigma_luma=float("nan")), dict(eps=0.0), dict(eps=float("inf")), dict(guides=8), dict(guides=-1)]


def _call(fn_name, cfg, h=4, w=5, variance=True, aov=True, out_variance=True, same_out=False):
    import rtamd
    L = rtamd.lib()
    hb, wb = max(h, 1), max(w, 1)  # (real buffers also when the call is given a bad size)
    rgb, v, g = np.zeros((hb, wb, 3)), np.zeros((hb, wb)), np.zeros((hb, wb, 8))
    out, ov = np.zeros((hb, wb, 3)), np.zeros((hb, wb))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    args = [C.byref(cfg), w, h, p(rgb), p(v) if variance else None, p(g) if aov else None, p(rgb) if same_out else p(out),
            p(ov) if out_variance else None]
    if fn_name == "rt_denoise_device":
        args = [C.byref(cfg), w, h] + [C.c_void_p(C.cast(a, C.c_void_p).value) if a is not None else None for a in args[3:]] + [None]
    return getattr(L, fn_name)(*args)


@pytest.mark.parametrize("fn_name", ["rt_denoise", "rt_denoise_device"])
@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_bad_config_is_an_argument_error(fn_name, bad):
    import rtamd
    assert _call(fn_name, rtamd.denoise_config(**bad)) == -1


@pytest.mark.parametrize("fn_name", ["rt_denoise", "rt_denoise_device"])
def test_bad_arguments_are_argument_errors(fn_name):
    import rtamd
    cfg = rtamd.denoise_config()
    assert _call(fn_name, cfg, h=0) == -1
    assert _call(fn_name, cfg, w=-3) == -1
    assert _call(fn_name, cfg, variance=False) == -1        # out_variance without a variance input
    assert _call(fn_name, cfg, same_out=True) == -1         # output aliasing the input
    cfg.reserved[2] = 1
    assert _call(fn_name, cfg) == -1
    assert "reserved" in rtamd.lib().rt_last_error().decode()


@pytest.mark.parametrize("fn_name", ["rt_denoise", "rt_denoise_device"])
def test_good_arguments_without_a_device_report_no_device(fn_name):
    import rtamd
    if rtamd.device_count() > 0:
        pytest.skip("a HIP device is visible: the GPU tests cover this path")
    cfg = rtamd.denoise_config()
    for kw in (dict(), dict(variance=False, out_variance=False), dict(aov=False), dict(out_variance=False)):
        assert _call(fn_name, cfg, **kw) == -9, kw


def test_denoise_wrapper_raises_no_device_without_a_gpu():
    import rtamd
    if rtamd.device_count() > 0:
        pytest.skip("a HIP device is visible")
    with pytest.raises(rtamd.RtError) as e:
        rtamd.denoise(np.zeros((3, 4, 3)), np.zeros((3, 4)), np.zeros((3, 4, 8)))
    assert e.value.code == -9
    with pytest.raises(TypeError):
        rtamd.denoise(np.zeros((3, 4, 3)), sigma=1.0)
    with pytest.raises(ValueError):
        rtamd.denoise(np.zeros((3, 4, 3)), np.zeros((4, 3)))


def test_render_aov_argument_checks_come_before_the_device():
    import rtamd
    w, cam = rtamd.select_scene(os.path.join(ROOT, "tests", "golden", "scenes", "cube.obj"), 1.0, 1)
    L = rtamd.lib()
    out = np.zeros((8, 8, 8))
    dp = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(aov_spp=1, **kw):
        p = rtamd.default_params(width=8, height=8, **kw)
        return L.rt_render_aov(w.h, C.byref(cam.c), C.byref(p), aov_spp, dp, None)
    assert call(world=2) == -1
    assert call(world=2, rank=1) == -1
    assert call(kernel=5) == -1
    assert call(aov_spp=0) == -1
    assert L.rt_render_aov(w.h, C.byref(cam.c), C.byref(rtamd.default_params(width=8, height=8)), 1, None, None) == -1
    if rtamd.device_count() == 0:
        assert call() == -9
        assert call(kernel=2) == -9


def test_render_denoised_needs_an_even_spp():
    import rtamd
    w, cam = rtamd.select_scene(os.path.join(ROOT, "tests", "golden", "scenes", "cube.obj"), 1.0, 1)
    for spp in (0, 1, 7):
        with pytest.raises(ValueError):
            w.render_denoised(cam, width=8, height=8, spp=spp)


# ---- the symbols in every binding ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_everywhere():
    import rtamd
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust-raytracer_amd", "rust", "rtamd_ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "rust-raytracer_amd", "host_cpp", "rtamd.hpp")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in rtamd.ABI_SYMBOLS, name
        assert re.search(r"pub fn %s\(" % name, rs), name
        assert hasattr(rtamd.lib(), name), name
    assert "rt_render_aov(" in hpp and "rt_denoise(" in hpp


def _c_fields(struct):
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
    return [re.sub(r"\[.*\]", "", d.split()[-1]) for d in body.split(";") if d.strip()]


def test_config_struct_has_the_same_fields_in_every_binding():
    import rtamd
    fields = _c_fields("rt_denoise_config")
    assert fields == ["iterations", "normal_power_log2", "sigma_depth", "sigma_albedo", "sigma_luma", "eps", "guides", "reserved"]
    assert [f for f, _ in rtamd.rt_denoise_config._fields_] == fields
    rs = open(os.path.join(ROOT, "rust-raytracer_amd", "rust", "rtamd_ffi.rs")).read()
    body = re.search(r"pub struct rt_denoise_config \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == fields
    assert "reserved: [i32; 5]" in body
