"""Env sampling -- the background as a light of integrator 1 (rt_scene_set_env_sampling) -- without a device: the
symbols are declared and exported, the record round-trips, bad configurations and calls after commit are argument errors, the
fingerprint tells enabled from not and two table sizes apart while a scene that leaves it off keeps the blob it had, and the
diagnostics fail with RT_ERR_NO_DEVICE on a GPU-less box."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_abi_symbols import HEADER, declared_symbols

RT_ERR_ARG = -1
RT_ERR_NO_DEVICE = -9


def _cfg(enabled=1, width=0, height=0):
    import rtamd
    return rtamd.rt_env_sampling(enabled, width, height)


def _scene10(commit=False):
    import rtamd
    return rtamd.load_scene_file(scene_path("scene_10.json"), commit=commit)


def test_header_declares_and_library_exports_the_env_sampling_entry_points():
    import rtamd
    for sym in ("rt_scene_set_env_sampling", "rt_scene_get_env_sampling", "rt_debug_env_table_device", "rt_debug_env_sample_device",
                "rt_debug_env_pdf_device"):
        assert sym in declared_symbols()
        assert sym in rtamd.ABI_SYMBOLS
        assert hasattr(C.CDLL(rtamd.LIB_PATH), sym)
    header = open(HEADER).read()
    assert re.search(r"typedef struct rt_env_sampling \{\s*int32_t enabled;.*?int32_t width, height;.*?\} rt_env_sampling;", header, flags=re.S)
    assert C.sizeof(rtamd.rt_env_sampling) == 12
    assert rtamd.lib().rt_abi_version() == 2
    rs = open(ROOT + "/rust-raytracer_amd/rust/rtamd_ffi.rs").read()
    assert re.search(r"pub struct rt_env_sampling \{\s*pub enabled: i32,\s*pub width: i32,\s*pub height: i32,\s*\}", rs)
    hpp = open(ROOT + "/rust-raytracer_amd/host_cpp/rtamd.hpp").read()
    assert "rt_scene_set_env_sampling" in hpp and "rt_scene_get_env_sampling" in hpp
    # the header no longer says that a background is never a light
    assert "is no\n * light" not in header and "is no light" not in header


def test_round_trip_and_python_helpers():
    world, _ = _scene10()
    assert world.env_sampling() == dict(enabled=False, width=0, height=0)
    world.set_sky()
    assert world.set_env_sampling() is world
    assert world.env_sampling() == dict(enabled=True, width=0, height=0)
    world.set_env_sampling(True, 64, 32)
    assert world.env_sampling() == dict(enabled=True, width=64, height=32)
    world.set_env_sampling(True, 8192, 8192)  # the largest table
    assert world.env_sampling() == dict(enabled=True, width=8192, height=8192)
    world.set_env_sampling(False, 16, 8)
    assert world.env_sampling() == dict(enabled=False, width=16, height=8)
    world.set_env_sampling(True, 16, 8)
    world.commit()
    assert world.env_sampling() == dict(enabled=True, width=16, height=8)  # readable after commit


@pytest.mark.parametrize("kw", [
    dict(width=-1, height=8), dict(width=8, height=-1), dict(width=-4, height=-4),
    dict(width=0, height=8), dict(width=8, height=0),
    dict(width=8193, height=8), dict(width=8, height=8193), dict(width=16384, height=16384),
    dict(enabled=2), dict(enabled=-1),
])
def test_bad_configurations_are_argument_errors(kw):
    world, _ = _scene10()
    world.set_sky()
    world.set_env_sampling(True, 32, 16)
    before = world.env_sampling()
    assert world.L.rt_scene_set_env_sampling(world.h, C.byref(_cfg(**kw))) == RT_ERR_ARG
    assert world.L.rt_last_error()
    assert world.env_sampling() == before  # a refused call leaves the scene as it was


def test_null_arguments_are_argument_errors():
    world, _ = _scene10()
    assert world.L.rt_scene_set_env_sampling(world.h, None) == RT_ERR_ARG
    assert world.L.rt_scene_set_env_sampling(None, C.byref(_cfg())) == RT_ERR_ARG
    assert world.L.rt_scene_get_env_sampling(world.h, None) == RT_ERR_ARG
    assert world.L.rt_scene_get_env_sampling(None, C.byref(_cfg())) == RT_ERR_ARG


def test_set_env_sampling_after_commit_is_refused():
    world, _ = _scene10()
    world.set_sky()
    world.commit()
    assert world.L.rt_scene_set_env_sampling(world.h, C.byref(_cfg())) == RT_ERR_ARG
    assert "immutable" in world.L.rt_last_error().decode()
    assert world.env_sampling()["enabled"] is False


def test_enabled_without_a_background_is_refused_at_commit():
    import rtamd
    world, _ = _scene10()
    world.set_env_sampling(True)  # the setter cannot know yet: the background may still come
    with pytest.raises(rtamd.RtError) as e:
        world.commit()
    assert e.value.code == RT_ERR_ARG and "background" in str(e.value)
    assert world.info()["committed"] == 0
    world.set_sky()  # ... and the scene is still a builder
    world.commit()
    assert world.info()["committed"] == 1
    w2, _ = _scene10()
    w2.set_env_sampling(False, 32, 16)  # disabled needs none
    w2.commit()


def _fp(world):
    world.commit()
    return world.fingerprint(), world.info()["bytes"]


def test_fingerprint_tells_the_switch_and_the_table_size_apart_and_off_changes_nothing():
    import rtamd

    def sky(**env):
        w, _ = _scene10()
        w.set_sky()
        if env:
            w.set_env_sampling(**env)
        return _fp(w)

    off = sky()
    assert sky(enabled=False) == off                      # the setter with enabled = 0: the blob of a scene that never called it
    assert sky(enabled=False, width=64, height=32) == off
    on = sky(enabled=True)
    assert on[0] != off[0] and on[1] == off[1] + 16       # the 16-byte record {1, W, H}
    a, b = sky(enabled=True, width=64, height=32), sky(enabled=True, width=32, height=16)
    assert len({off[0], on[0], a[0], b[0]}) == 4
    assert sky(enabled=True, width=256, height=128) == on  # automatic for a gradient is 256 x 128
    # a scene without a background: never calling the setter, or calling it with enabled = 0, leaves today's fingerprint
    loaded, _ = rtamd.load_scene_file(scene_path("scene_10.json"))
    ref = (loaded.fingerprint(), loaded.info()["bytes"])
    w, _ = _scene10()
    w.set_env_sampling(False)
    assert _fp(w) == ref


def test_automatic_size_follows_an_image_map():
    """one cell per texel, halved per axis until at most 4096 x 2048: seen through the fingerprint, which covers the record {1, W, H}"""
    def fp(shape, **env):
        w, _ = _scene10()
        tex = w.ImageTexture(np.full(shape + (3,), 7, dtype=np.uint8))
        w.set_background(texture=tex)
        w.set_env_sampling(True, **env)
        return _fp(w)[0]
    assert fp((32, 64)) == fp((32, 64), width=64, height=32)
    assert fp((32, 64)) != fp((32, 64), width=256, height=128)
    assert fp((10, 6000)) == fp((10, 6000), width=3000, height=5)       # halved once, both axes
    assert fp((2100, 100)) == fp((2100, 100), width=50, height=1050)     # too tall only: both axes are halved all the same
    w, _ = _scene10()
    tex = w.CheckerTexture(w.ConstantTexture((0.1, 0.2, 0.3)), w.ConstantTexture((0.9, 0.8, 0.7)))
    w.set_background(texture=tex)
    w.set_env_sampling(True)
    w2, _ = _scene10()
    tex = w2.CheckerTexture(w2.ConstantTexture((0.1, 0.2, 0.3)), w2.ConstantTexture((0.9, 0.8, 0.7)))
    w2.set_background(texture=tex)
    w2.set_env_sampling(True, 256, 128)
    assert _fp(w)[0] == _fp(w2)[0]


def test_pinned_fingerprints_hold_with_the_switch_off():
    import json
    import os
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "nested_transform_pins.json")))
    import rtamd
    for name in [k for k in pins if k.endswith(".json")]:
        w, _ = rtamd.load_scene_file(scene_path(name), commit=False)
        w.set_env_sampling(False, 128, 64)
        w.commit()
        assert "%016x" % w.fingerprint() == pins[name]["fingerprint"], name


def test_diagnostics_and_renders_need_a_device():
    import rtamd
    if rtamd.device_count() > 0:
        pytest.skip("a HIP device is visible: tests/test_env_sampling_gpu.py covers the diagnostics and the renders")
    w, cam = _scene10()
    w.set_sky()
    w.set_env_sampling(True, 16, 8)
    w.commit()
    L = w.L
    wd, ht = C.c_int(), C.c_int()
    dp = C.POINTER(C.c_double)
    assert L.rt_debug_env_table_device(w.h, 0, C.byref(wd), C.byref(ht), None) == RT_ERR_NO_DEVICE
    xi = np.full((4, 4), 0.5)
    out = np.zeros((4, 4))
    assert L.rt_debug_env_sample_device(w.h, 0, 4, xi.ctypes.data_as(dp), out.ctypes.data_as(dp)) == RT_ERR_NO_DEVICE
    assert L.rt_debug_env_pdf_device(w.h, 0, 4, xi.ctypes.data_as(dp), out.ctypes.data_as(dp)) == RT_ERR_NO_DEVICE
    for call in (lambda: w.debug_env_table(), lambda: w.debug_env_sample(xi), lambda: w.debug_env_pdf(xi[:, :3])):
        with pytest.raises(rtamd.RtError) as e:
            call()
        assert e.value.code == RT_ERR_NO_DEVICE
    assert L.rt_debug_env_table_device(None, 0, C.byref(wd), C.byref(ht), None) == RT_ERR_ARG
    p = rtamd.default_params(width=8, height=8, spp=2, integrator=1)
    img = np.zeros((8, 8, 3))
    assert L.rt_render(w.h, C.byref(cam.c), C.byref(p), img.ctypes.data_as(dp), None) == RT_ERR_NO_DEVICE


def test_host_cpp_binary_knows_the_env_sampling_option():
    import os
    exe = os.path.join(ROOT, "rust-raytracer_amd", "rtamd_render")
    if not os.path.exists(exe):
        pytest.skip("rtamd_render not built")
    scene = scene_path("scene_10.json")
    r = subprocess.run([exe, "--scene", scene, "--sky", "--env-sampling", "--describe"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "scene:" in r.stdout, r.stdout + r.stderr
    r2 = subprocess.run([exe, "--scene", scene, "--sky", "--describe"], capture_output=True, text=True, timeout=60)
    assert r2.returncode == 0
    n_env = int(re.search(r"(\d+) bytes flattened", r.stdout).group(1))
    n_sky = int(re.search(r"(\d+) bytes flattened", r2.stdout).group(1))
    assert n_env == n_sky + 16  # the 16-byte env record
    r3 = subprocess.run([exe, "--scene", scene, "--env-sampling", "--describe"], capture_output=True, text=True, timeout=60)
    assert r3.returncode == 1 and "error -1" in r3.stderr  # no background to sample
