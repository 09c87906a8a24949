"""The energy-preserving denoise mode and the one-call denoised render without a GPU: the numpy restatement's own properties
(tests/denoise_sym_ref.py), the four new symbols and their argument order in the header, the Python binding and the Rust FFI file, and
every argument error of rt_denoise_sym / rt_denoise_sym_device / rt_denoised_render / rt_denoised_render_device through the C ABI --
returned before a device is asked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref
import denoise_sym_ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rtamd.h")
FILTER_ARGS = ["cfg", "width", "height", "rgb", "variance", "aov", "out_rgb", "out_variance"]
RENDER_ARGS = ["s", "cam", "p", "cfg", "luma_mode", "aov_spp", "out_rgb", "out_noisy", "out_variance", "out_aov"]
SIGNATURES = {
    "rt_denoise_sym": FILTER_ARGS,
    "rt_denoise_sym_device": ["cfg", "width", "height"] + ["d_" + a for a in FILTER_ARGS[3:]] + ["hip_stream"],
    "rt_denoised_render": RENDER_ARGS + ["stats"],
    "rt_denoised_render_device": RENDER_ARGS[:6] + ["d_" + a for a in RENDER_ARGS[6:]] + ["hip_stream", "stats"],
}


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _random_inputs(h, w, seed):
    rng = np.random.default_rng(seed)
    c = rng.gamma(2.0, 0.3, size=(h, w, 3))
    v = rng.gamma(1.0, 0.02, size=(h, w))
    v[rng.random((h, w)) < 0.2] = 0.0
    g = rng.random((h, w, 8))
    return c, v, g


@pytest.mark.parametrize("guides", [None, 7])
@pytest.mark.parametrize("with_variance", [False, True])
def test_mode_0_of_the_restatement_is_denoise_ref(guides, with_variance):
    c, v, g = _random_inputs(11, 13, 2)
    v = v if with_variance else None
    aov = None if guides is None else g
    a = denoise_sym_ref.denoise(c, v, aov, mode=0, iterations=3)
    b = denoise_ref.denoise(c, v, aov, iterations=3)
    assert np.array_equal(a[0], b[0])
    assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1])


def _pair_weights(taps):
    """{(p, q): weight p gives q} over the in-image taps of a pass, p and q as (y, x)"""
    out = {}
    for dx, dy, w, valid in taps:
        for y, x in np.argwhere(valid):
            out[((y, x), (y + dy, x + dx))] = w[y, x]
    return out


def test_the_symmetric_stop_gives_every_pair_one_weight():
    """one pass without guides on a random 7 x 9 image: the weight p gives q is the weight q gives p, bit for bit, for every pair of the
    symmetric stop -- and not of rt_denoise's, whose stop is the centre's own variance"""
    c, v, _ = _random_inputs(7, 9, 5)
    cfg = dict(denoise_ref.DEFAULTS)
    sym = _pair_weights(denoise_sym_ref.pass_weights(c, v, None, 1, cfg, mode=1))
    assert len(sym) > 7 * 9 * 9 and all(sym[(q, p)] == w for (p, q), w in sym.items())
    one_sided = _pair_weights(denoise_sym_ref.pass_weights(c, v, None, 1, cfg, mode=0))
    assert sorted(one_sided) == sorted(sym)
    assert sum(one_sided[(q, p)] != w for (p, q), w in one_sided.items()) > len(one_sided) // 2


def test_a_bright_pixel_among_dark_ones_keeps_its_energy():
    """the case that darkens frames: one pixel drew a bright sample (large v_p), its neighbours are dark with v_q = 0.  rt_denoise's centre
    stop lets the bright pixel be averaged down (its stop is wide) while the dark ones reject it (theirs is eps): what the spike gives up
    leaves the frame.  With the symmetric stop the neighbours take the spike in with the weight it takes them, so most of it stays (each
    pixel still divides by its own W, so the sum is kept closely, not exactly)"""
    c = np.full((15, 15, 3), 0.1)
    v = np.zeros((15, 15))
    c[7, 7] = 5.0
    v[7, 7] = 6.0
    one_sided, _ = denoise_ref.denoise(c, v, None, iterations=1)
    sym, _ = denoise_sym_ref.denoise(c, v, None, iterations=1)
    assert one_sided[7, 7, 0] == sym[7, 7, 0] < 5.0 / 2              # both average the spike down, by the same weights (v_q = 0)
    assert np.max(np.abs(np.delete(one_sided[..., 0].ravel(), 7 * 15 + 7) - 0.1)) < 1e-8   # one-sided: no neighbour took any of it
    assert sym[7, 8, 0] > 0.2 and sym[6, 6, 0] > 0.15             # symmetric: they did
    lost_one, lost_sym = c.sum() - one_sided.sum(), c.sum() - sym.sum()
    assert lost_one > 0.1 * c.sum() and abs(lost_sym) < lost_one / 2


def test_the_symmetric_restatement_needs_a_variance():
    with pytest.raises(ValueError):
        denoise_sym_ref.denoise(np.zeros((3, 3, 3)))


# ---- the symbols in every binding ----------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_symbol_and_argument_order_in_header_ctypes_and_rust(name):
    import rtamd
    want = SIGNATURES[name]
    m = re.search(r"\bint %s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    assert m, "%s is not declared in rtamd.h" % name
    assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == want
    rs = open(os.path.join(ROOT, "rust-raytracer_amd", "rust", "rtamd_ffi.rs")).read()
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, rs, flags=re.S)
    assert m, "%s is not declared in rtamd_ffi.rs" % name
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == want
    sig = dict((s[0], s) for s in rtamd._SIGS)[name]
    assert sig[1] is C.c_int and len(sig[2]) == len(want)
    for arg, ty in zip(want, sig[2]):
        if arg in ("width", "height", "luma_mode", "aov_spp"):
            assert ty is C.c_int32, (name, arg)
        elif arg == "cfg":
            assert ty is C.POINTER(rtamd.rt_denoise_config), (name, arg)
        elif arg == "stats":
            assert ty is C.POINTER(rtamd.rt_stats), (name, arg)
        elif arg in ("hip_stream", "s") or arg.startswith("d_"):
            assert ty is C.c_void_p, (name, arg)
    assert hasattr(rtamd.lib(), name)


def test_cpp_wrapper_cli_and_docs_name_the_new_call():
    pkg = os.path.join(ROOT, "rust-raytracer_amd")
    hpp = open(os.path.join(pkg, "host_cpp", "rtamd.hpp")).read()
    main = open(os.path.join(pkg, "host_cpp", "main.cpp")).read()
    assert "rt_denoised_render(" in hpp and "render_denoised(" in main
    for flag in ("--denoise", "--aov-spp", "--luma-mode"):
        assert flag in main, flag
    rs = open(os.path.join(pkg, "rust", "rtamd_ffi.rs")).read()
    assert "pub fn render_denoised(&self" in rs and "pub fn denoise_sym(" in rs
    assert "rt_denoised_render" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sqrt(v_p + v_q)" in open(HEADER).read()                           # the formula, stated next to rt_denoise's


def test_rt_denoise_config_is_untouched():
    import rtamd
    assert C.sizeof(rtamd.rt_denoise_config) == 64
    c = rtamd.denoise_config()
    assert c.sigma_luma == 4.0 and list(c.reserved) == [0] * 5


# ---- rt_denoise_sym, rt_denoise_sym_device: argument errors -----------------------------------------------------------------------------
BAD_CONFIGS = [dict(iterations=0), dict(iterations=9), dict(normal_power_log2=-1), dict(normal_power_log2=17), dict(sigma_depth=0.0),
               dict(sigma_albedo=-1.0), dict(sigma_luma=float("nan")), dict(eps=0.0), dict(eps=float("inf")), dict(guides=8), dict(guides=-1)]
_dp = C.POINTER(C.c_double)


def _filter(fn_name, cfg, h=4, w=5, variance=True, aov=True, out_variance=True, same_out=False, rgb=True):
    import rtamd
    hb, wb = max(h, 1), max(w, 1)
    c, v, g = np.zeros((hb, wb, 3)), np.zeros((hb, wb)), np.zeros((hb, wb, 8))
    out, ov = np.zeros((hb, wb, 3)), np.zeros((hb, wb))
    ptrs = [c if rgb else None, v if variance else None, g if aov else None, c if same_out else out, ov if out_variance else None]
    if fn_name.endswith("_device"):
        args = [C.c_void_p(a.ctypes.data) if a is not None else None for a in ptrs] + [None]
    else:
        args = [a.ctypes.data_as(_dp) if a is not None else None for a in ptrs]
    return getattr(rtamd.lib(), fn_name)(C.byref(cfg) if cfg is not None else None, w, h, *args)


@pytest.mark.parametrize("fn_name", ["rt_denoise_sym", "rt_denoise_sym_device"])
def test_filter_argument_errors(fn_name):
    import rtamd
    cfg = rtamd.denoise_config()
    assert _filter(fn_name, cfg, variance=False, out_variance=False) == -1   # no variance: that call is rt_denoise
    assert "variance" in rtamd.lib().rt_last_error().decode()
    assert _filter(fn_name, None) == -1
    assert _filter(fn_name, cfg, rgb=False) == -1
    assert _filter(fn_name, cfg, h=0) == -1
    assert _filter(fn_name, cfg, w=-3) == -1
    assert _filter(fn_name, cfg, variance=False) == -1                        # out_variance without a variance input
    assert _filter(fn_name, cfg, same_out=True) == -1                         # output aliasing the input
    for bad in BAD_CONFIGS:
        assert _filter(fn_name, rtamd.denoise_config(**bad)) == -1, bad
    cfg.reserved[2] = 1
    assert _filter(fn_name, cfg) == -1
    assert "reserved" in rtamd.lib().rt_last_error().decode()


@pytest.mark.parametrize("fn_name", ["rt_denoise_sym", "rt_denoise_sym_device"])
def test_filter_good_arguments_without_a_device_report_no_device(fn_name):
    import rtamd
    if rtamd.device_count() > 0:
        pytest.skip("a HIP device is visible: the GPU tests cover this path")
    cfg = rtamd.denoise_config()
    for kw in (dict(), dict(aov=False), dict(out_variance=False)):
        assert _filter(fn_name, cfg, **kw) == -9, kw


def test_python_wrappers_take_symmetric():
    import rtamd
    with pytest.raises(rtamd.RtError) as e:
        rtamd.denoise(np.zeros((3, 4, 3)), None, None, symmetric=True)
    assert e.value.code == -1
    if rtamd.device_count() == 0:
        with pytest.raises(rtamd.RtError) as e:
            rtamd.denoise(np.zeros((3, 4, 3)), np.zeros((3, 4)), symmetric=True)
        assert e.value.code == -9
    with pytest.raises(rtamd.RtError) as e:
        rtamd.denoise_device(4, 3, 1 << 20, 2 << 20, symmetric=True)           # no variance pointer: refused before any pointer is read
    assert e.value.code == -1


# ---- rt_denoised_render, rt_denoised_render_device: argument errors ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube_scene():
    import rtamd
    return rtamd.select_scene(os.path.join(ROOT, "tests", "golden", "scenes", "cube.obj"), 1.0, 1)


def _render(fn_name, scene, cfg="default", luma_mode=1, aov_spp=1, rgb=True, aov=True, null=(), **params):
    import rtamd
    w, cam = scene
    kw = dict(width=8, height=8, spp=4)
    kw.update(params)
    p = rtamd.default_params(**kw)
    bufs = [np.zeros((8, 8, 3)), np.zeros((8, 8, 3)), np.zeros((8, 8)), np.zeros((8, 8, 8))]
    use = [rgb, True, True, aov]
    if fn_name.endswith("_device"):
        outs = [C.c_void_p(b.ctypes.data) if u else None for b, u in zip(bufs, use)] + [None]
    else:
        outs = [b.ctypes.data_as(_dp) if u else None for b, u in zip(bufs, use)]
    c = rtamd.denoise_config() if isinstance(cfg, str) else cfg
    return getattr(rtamd.lib(), fn_name)(None if "s" in null else w.h, None if "cam" in null else C.byref(cam.c), None if "p" in null else C.byref(p),
                                         C.byref(c) if c is not None else None, luma_mode, aov_spp, *outs, None)


@pytest.mark.parametrize("fn_name", ["rt_denoised_render", "rt_denoised_render_device"])
def test_render_argument_errors_come_before_the_device(fn_name, cube_scene):
    import rtamd
    call = lambda **kw: _render(fn_name, cube_scene, **kw)  # noqa: E731
    for name in ("s", "cam", "p"):
        assert call(null=(name,)) == -1, name
    assert call(rgb=False) == -1
    for spp in (0, 1, 3, 7, -2):
        assert call(spp=spp) == -1, spp
    assert call(world=2) == -1 and call(world=2, rank=1) == -1
    for mode in (-1, 2):
        assert call(luma_mode=mode) == -1, mode
    assert call(aov_spp=-1) == -1
    assert call(aov_spp=0, aov=True) == -1                                    # out_aov without guides
    assert "out_aov" in rtamd.lib().rt_last_error().decode()
    for bad in BAD_CONFIGS:
        assert call(cfg=rtamd.denoise_config(**bad)) == -1, bad
    cfg = rtamd.denoise_config()
    cfg.reserved[0] = 3
    assert call(cfg=cfg) == -1
    for bad in (dict(width=0), dict(height=-1), dict(max_depth=-1), dict(kernel=3), dict(kernel=7), dict(integrator=3), dict(time0=1.0, time1=0.5)):
        assert call(**bad) == -1, bad                                         # what rt_render refuses


@pytest.mark.parametrize("fn_name", ["rt_denoised_render", "rt_denoised_render_device"])
def test_render_good_arguments_without_a_device_report_no_device(fn_name, cube_scene):
    import rtamd
    if rtamd.device_count() > 0:
        pytest.skip("a HIP device is visible: the GPU tests cover this path")
    assert _render(fn_name, cube_scene) == -9
    assert _render(fn_name, cube_scene, cfg=None, luma_mode=0, aov_spp=0, aov=False, spp=2) == -9
    assert _render(fn_name, cube_scene, kernel=2, integrator=1) == -9


def test_render_denoised_native_checks_spp_like_the_composition(cube_scene):
    import rtamd
    w, cam = cube_scene
    for spp in (0, 1, 7):
        with pytest.raises(ValueError):
            w.render_denoised(cam, width=8, height=8, spp=spp, native=True)
    if rtamd.device_count() == 0:
        with pytest.raises(rtamd.RtError) as e:
            w.render_denoised(cam, width=8, height=8, spp=2, native=True)
        assert e.value.code == -9
