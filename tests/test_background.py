"""Backgrounds for rays that miss the scene (rt_scene_set_background) without a device: the symbols are declared and
exported, bad backgrounds and calls after commit are argument errors, the record round-trips, a scene without a background keeps its
flattened blob and fingerprint, and the render entry points still fail with RT_ERR_NO_DEVICE on a GPU-less box."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_abi_symbols import HEADER, declared_symbols

RT_ERR_ARG = -1
RT_ERR_NO_DEVICE = -9


def _bg(kind=1, texture=0, color0=(0.5, 0.6, 0.7), color1=(0.0, 0.0, 0.0), scale=1.0):
    import rtamd
    b = rtamd.rt_background()
    b.kind, b.texture, b.scale = kind, texture, scale
    b.color0 = rtamd._arr3(color0)
    b.color1 = rtamd._arr3(color1)
    return b


def _scene10(commit=False):
    import rtamd
    return rtamd.load_scene_file(scene_path("scene_10.json"), commit=commit)


def test_header_declares_and_library_exports_the_background_entry_points():
    import rtamd
    for sym in ("rt_scene_set_background", "rt_scene_get_background", "rt_scene_parse_file"):
        assert sym in declared_symbols()
        assert sym in rtamd.ABI_SYMBOLS
        assert hasattr(C.CDLL(rtamd.LIB_PATH), sym)
    header = open(HEADER).read()
    assert re.search(r"typedef struct rt_background \{\s*int32_t kind;.*?int32_t texture;.*?double color0\[3\];.*?double color1\[3\];"
                     r".*?double scale;.*?\} rt_background;", header, flags=re.S)
    assert C.sizeof(rtamd.rt_background) == 64
    assert rtamd.lib().rt_abi_version() == 2
    rs = open(ROOT + "/rust-raytracer_amd/rust/rtamd_ffi.rs").read()
    assert re.search(r"pub struct rt_background \{\s*pub kind: i32,\s*pub texture: i32,\s*pub color0: \[c_double; 3\],\s*"
                     r"pub color1: \[c_double; 3\],\s*pub scale: c_double,\s*\}", rs)


@pytest.mark.parametrize("kw", [
    dict(kind=-1), dict(kind=4),
    dict(kind=3, texture=-1), dict(kind=3, texture=10 ** 6),
    dict(color0=(float("nan"), 0.0, 0.0)), dict(color0=(0.0, -0.5, 0.0)), dict(kind=2, color1=(0.0, 0.0, float("inf"))),
    dict(color1=(-1.0, 0.0, 0.0)),  # every colour is checked, whatever the kind reads
    dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
])
def test_bad_backgrounds_are_argument_errors(kw):
    world, _ = _scene10()
    before = world.background()
    assert world.L.rt_scene_set_background(world.h, C.byref(_bg(**kw))) == RT_ERR_ARG
    assert world.L.rt_last_error()
    assert world.background() == before  # a refused call leaves the scene as it was


def test_null_arguments_are_argument_errors():
    import rtamd
    world, _ = _scene10()
    assert world.L.rt_scene_set_background(world.h, None) == RT_ERR_ARG
    assert world.L.rt_scene_set_background(None, C.byref(_bg())) == RT_ERR_ARG
    assert world.L.rt_scene_get_background(world.h, None) == RT_ERR_ARG
    assert world.L.rt_scene_get_background(None, C.byref(rtamd.rt_background())) == RT_ERR_ARG


def test_set_background_after_commit_is_refused():
    world, _ = _scene10(commit=True)
    assert world.L.rt_scene_set_background(world.h, C.byref(_bg())) == RT_ERR_ARG
    assert "immutable" in world.L.rt_last_error().decode()
    assert world.background()["kind"] == 0


def test_round_trip_and_python_helpers():
    import rtamd
    world, _ = _scene10()
    assert world.background() == dict(kind=0, texture=0, color0=(0.0,) * 3, color1=(0.0,) * 3, scale=0.0)
    world.set_background(color=(0.25, 0.5, 1.0), scale=2.0)
    assert world.background() == dict(kind=1, texture=0, color0=(0.25, 0.5, 1.0), color1=(0.0,) * 3, scale=2.0)
    world.set_sky()
    assert world.background() == dict(kind=2, texture=0, color0=(1.0, 1.0, 1.0), color1=(0.5, 0.7, 1.0), scale=1.0)
    tex = world.CheckerTexture(world.ConstantTexture((0.1, 0.2, 0.3)), world.ConstantTexture((0.9, 0.8, 0.7)))
    world.set_background(texture=tex, scale=0.5)
    b = world.background()
    assert (b["kind"], b["texture"], b["scale"]) == (3, tex, 0.5)
    world.set_background()  # none of them: kind 0
    assert world.background()["kind"] == 0
    with pytest.raises(ValueError):
        world.set_background(color=(1, 1, 1), gradient=((1, 1, 1), (0, 0, 0)))
    with pytest.raises(rtamd.RtError):
        world.set_background(color=(1.0, -1.0, 1.0))
    world.set_background(color=(0.0, 0.0, 0.0))  # black is a background too (kind 1): it runs the background variants
    world.commit()
    assert world.background()["kind"] == 1


def _fp(world):
    world.commit()
    return world.fingerprint(), world.info()["bytes"]


def test_fingerprint_without_background_is_unchanged_and_every_background_differs():
    import rtamd
    loaded, _ = rtamd.load_scene_file(scene_path("scene_10.json"))
    ref = (loaded.fingerprint(), loaded.info()["bytes"])
    assert ref[0] != 0
    assert _fp(_scene10()[0]) == ref  # parse + commit == load
    w, _ = _scene10()
    w.set_background()  # kind 0 explicitly: no record
    assert _fp(w) == ref
    fps = set()
    for kw in (dict(color=(0.0, 0.0, 0.0)), dict(color=(0.5, 0.7, 1.0)), dict(color=(0.5, 0.7, 1.0), scale=2.0), dict(gradient=rtamd.SKY),
               dict(gradient=(rtamd.SKY[1], rtamd.SKY[0]))):
        w, _ = _scene10()
        w.set_background(**kw)
        fp, nbytes = _fp(w)
        assert fp != ref[0] and nbytes > ref[1], kw
        fps.add(fp)
    assert len(fps) == 5


def test_pinned_fingerprints_of_scene_files_hold_through_the_parse_path():
    """tests/golden/nested_transform_pins.json pins the fingerprints of the scene files (no background): rt_scene_parse_file + commit
    reaches the same blob as rt_scene_load_file."""
    import json
    import os
    import rtamd
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "nested_transform_pins.json")))
    files = [k for k in pins if k.endswith(".json")]
    assert len(files) >= 3
    for name in files:
        w, _ = rtamd.load_scene_file(scene_path(name), commit=False)
        assert w.info()["committed"] == 0
        w.commit()
        assert "%016x" % w.fingerprint() == pins[name]["fingerprint"], name
        assert w.info() == pins[name]["info"], name


def test_cornell_box_uncommitted_then_background():
    import rtamd
    cube = scene_path("cube.obj")
    w0, _ = rtamd.select_scene(cube, 1.5)
    w1, _ = rtamd.select_scene(cube, 1.5, commit=False)
    assert w1.info()["committed"] == 0
    w1.commit()
    assert w1.fingerprint() == w0.fingerprint()
    w2, _ = rtamd.select_scene(cube, 1.5, commit=False)
    w2.set_sky()
    w2.commit()
    assert w2.fingerprint() != w0.fingerprint()


def test_render_entry_points_need_a_device():
    import rtamd
    if rtamd.device_count() > 0:
        pytest.skip("a HIP device is visible: tests/test_background_gpu.py covers the renders")
    w, cam = _scene10()
    w.set_sky()
    w.commit()
    p = rtamd.default_params(width=8, height=8, spp=2)
    out = np.zeros((8, 8, 3))
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    L = w.L
    assert L.rt_render(w.h, C.byref(cam.c), C.byref(p), dp, None) == RT_ERR_NO_DEVICE
    frame = cam.frame()
    assert L.rt_render_camera_frame(w.h, C.byref(frame), C.byref(p), dp, None) == RT_ERR_NO_DEVICE
    assert L.rt_render_accumulate(w.h, C.byref(cam.c), C.byref(p), 0, 2, dp, None) == RT_ERR_NO_DEVICE
    cfg = rtamd.rt_adaptive_config(min_spp=2, reserved=0, threshold=0.0)
    assert L.rt_render_adaptive(w.h, C.byref(cam.c), C.byref(p), C.byref(cfg), dp, None, None) == RT_ERR_NO_DEVICE
    assert L.rt_render_multi(w.h, C.byref(cam.c), C.byref(p), 1, None, dp, None) == RT_ERR_NO_DEVICE


def test_host_cpp_binary_knows_the_background_options():
    import os
    exe = os.path.join(ROOT, "rust-raytracer_amd", "rtamd_render")
    if not os.path.exists(exe):
        pytest.skip("rtamd_render not built")
    r = subprocess.run([exe, "--scene", scene_path("scene_10.json"), "--sky", "--describe"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "scene:" in r.stdout, r.stdout + r.stderr
    r2 = subprocess.run([exe, "--scene", scene_path("scene_10.json"), "--describe"], capture_output=True, text=True, timeout=60)
    assert r2.returncode == 0
    n_sky = int(re.search(r"(\d+) bytes flattened", r.stdout).group(1))
    n_none = int(re.search(r"(\d+) bytes flattened", r2.stdout).group(1))
    assert n_sky == n_none + 64  # the 64-byte background record
    r3 = subprocess.run([exe, "--scene", scene_path("scene_10.json"), "--background", "0.1,0.2", "--describe"], capture_output=True, text=True, timeout=60)
    assert r3.returncode == 2
    r4 = subprocess.run([exe, "--scene", scene_path("scene_10.json"), "--background", "0.1,-0.2,0.3", "--describe"], capture_output=True, text=True,
                        timeout=60)
    assert r4.returncode == 1 and "error -1" in r4.stderr
