"""Temporal accumulation without a device: the rule of rt_temporal_accumulate as tests/temporal_ref.py restates it (running mean, a
one-pixel shift, every rejection reached by a crafted row, reset), the argument checks of the entry points and of rt_sequence_* through the
C ABI, the symbols in every binding, and the quality of the rule on oracle frames of a Cornell orbit (DESIGN.md s4l has the figures)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_cases as tc
import temporal_ref
from conftest import ROOT, scene_path

HEADER = os.path.join(ROOT, "include", "rtamd.h")
NEW_SYMBOLS = ["rt_default_temporal_config", "rt_temporal_accumulate", "rt_temporal_accumulate_device", "rt_sequence_create",
               "rt_sequence_destroy", "rt_sequence_reset", "rt_sequence_frames", "rt_sequence_frame"]


def _reset_of(k):
    l = temporal_ref.luminance(k["rgb"])
    return np.concatenate([k["rgb"], l[..., None], (l * l)[..., None], np.ones(l.shape + (1,))], axis=2)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,max_history", [(0.0, 4), (0.0, 32), (0.5, 32), (1.0, 32)])
def test_identical_camera_and_guides_give_the_running_mean(alpha, max_history):
    """Wsum == 1 exactly (one tap of weight 1), out = (1 - a) h + a rgb with a = max(alpha, 1 / n), n = min(n + 1, max_history)"""
    rng = np.random.default_rng(1)
    cam, g = tc.camera(), tc.plane_guides()
    frames = rng.uniform(0.0, 1.0, size=(7, tc.H, tc.W, 3))
    hist = mean = None
    for f, rgb in enumerate(frames):
        info = {}
        hist, var = temporal_ref.accumulate(rgb, g, cam, None, hist, g if f else None, cam if f else None, info=info, alpha=alpha,
                                            max_history=max_history)
        n = min(f + 1, max_history)
        a = max(alpha, 1.0 / n)
        mean = rgb if f == 0 else (1.0 - a) * mean + a * rgb
        assert np.all(hist[..., 5] == float(n))
        assert np.allclose(hist[..., 0:3], mean, rtol=0, atol=1e-12)
        if f:
            assert np.all(info["Wsum"] == 1.0) and info["kept"].all()
        if alpha == 0.0 and max_history == 32:   # the plain running mean, and the variance of its luminance from the two moments
            assert np.allclose(hist[..., 0:3], frames[:f + 1].mean(axis=0), rtol=0, atol=1e-12)
            ls = temporal_ref.luminance(frames[:f + 1])
            assert np.allclose(hist[..., 3], ls.mean(axis=0), atol=1e-12) and np.allclose(hist[..., 4], (ls * ls).mean(axis=0), atol=1e-12)
            assert np.allclose(var, np.maximum(0.0, (ls * ls).mean(axis=0) - ls.mean(axis=0) ** 2) / n, atol=1e-12)


def test_short_histories_take_the_given_variance():
    k = tc.base(n_prev=2.0)
    hist, var = temporal_ref.accumulate(**k, alpha=0.0)
    assert np.all(hist[..., 5] == 3.0) and np.array_equal(var, k["variance"] * (1.0 / 3.0))
    k = tc.base(n_prev=3.0)
    hist, var = temporal_ref.accumulate(**k, alpha=0.0)
    assert np.all(hist[..., 5] == 4.0)
    assert np.array_equal(var, np.fmax(0.0, hist[..., 4] - hist[..., 3] * hist[..., 3]) * 0.25)
    k["variance"] = None
    assert np.array_equal(temporal_ref.accumulate(**k, alpha=0.0)[1], var)


def test_a_camera_moved_by_one_pixel_shifts_the_history_by_one_pixel():
    k = tc.base(shift_px=1.0, n_prev=3.0)
    hist, _ = temporal_ref.accumulate(**k, alpha=0.0)
    assert np.all(hist[:, :-1, 5] == 4.0) and np.all(hist[:, -1, 5] == 1.0)   # n exact; the uncovered column restarts
    exp = 0.75 * k["prev_history"][:, 1:, 0:3] + 0.25 * k["rgb"][:, :-1]
    assert np.allclose(hist[:, :-1, 0:3], exp, rtol=0, atol=1e-9)
    assert np.array_equal(hist[:, -1], _reset_of(k)[:, -1])


@pytest.mark.parametrize("name", sorted(tc.REJECTIONS))
def test_each_rejection_resets_its_pixel_and_only_the_crafted_row_reaches_it(name):
    k, plain, cfg, (y, x) = tc.rejection(name)
    hist, var = temporal_ref.accumulate(**k, **cfg)
    assert np.array_equal(hist[y, x], _reset_of(k)[y, x]) and hist[y, x, 5] == 1.0
    assert var[y, x] == k["variance"][y, x]          # a = 1, n = 1 < 4: the frame's own variance
    if name == "outside_the_frame":                    # (nothing to edit: the control is the column beside it)
        assert hist[y, x - 1, 5] == 4.0
        return
    ctl, _ = temporal_ref.accumulate(**plain, **cfg)
    assert ctl[y, x, 5] == 4.0, "without the crafted value the pixel keeps its history"
    if name == "min_weight":                           # the light tap alone carries the history once min_weight lets it
        low, _ = temporal_ref.accumulate(**k, min_weight=0.1)
        assert low[y, x, 5] == 4.0 and np.allclose(low[y, x, 0:3], 0.75 * k["prev_history"][y, x, 0:3] + 0.25 * k["rgb"][y, x], atol=1e-12)
    others = np.ones((tc.H, tc.W), dtype=bool)
    others[y, max(0, x - 1):x + 2] = False
    assert np.array_equal(hist[others], ctl[others])


def test_reset_and_first_frame():
    k = tc.base()
    first, var = temporal_ref.accumulate(k["rgb"], k["aov"], k["cam_cur"], k["variance"])
    assert np.array_equal(first, _reset_of(k)) and np.array_equal(var, k["variance"])
    _, var0 = temporal_ref.accumulate(k["rgb"], k["aov"], k["cam_cur"])
    assert np.all(var0 == 0.0)                         # m2 - m1 m1 of one frame


def test_random_inputs_reach_both_outcomes():
    """the inputs of the GPU comparison keep a good part of the histories and reset a good part"""
    for (h, w, seed) in [(21, 37, 1), (16, 16, 2)]:
        info = {}
        hist, _ = temporal_ref.accumulate(**tc.random_inputs(h, w, seed), info=info)
        assert 0.15 < info["kept"].mean() < 0.85, info["kept"].mean()
        assert (hist[..., 5] == 32.0).any() and np.isfinite(hist).all()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
_dp = C.POINTER(C.c_double)


def _step(fn_name="rt_temporal_accumulate", cfg=None, w=5, h=4, null=(), prev="all", alias=None):
    import rtamd
    L = rtamd.lib()
    cfg = cfg if cfg is not None else rtamd.temporal_config()
    b = dict(rgb=np.zeros((4, 5, 3)), aov=np.zeros((4, 5, 8)), variance=np.zeros((4, 5)), prev_history=np.zeros((4, 5, 6)),
             prev_aov=np.zeros((4, 5, 8)), out_history=np.zeros((4, 5, 6)), out_variance=np.zeros((4, 5)))
    cam = [rtamd.rt_camera_frame(), rtamd.rt_camera_frame()]
    have_prev = {"all": (1, 1, 1), "none": (0, 0, 0), "cam_only": (1, 0, 0), "history_only": (0, 1, 0), "no_aov": (1, 1, 0)}[prev]
    p = {k: v.ctypes.data_as(_dp) for k, v in b.items()}
    if alias:
        p[alias[0]] = p[alias[1]]
    for k in null:
        p[k] = None
    args = [None if "cfg" in null else C.byref(cfg), w, h, C.byref(cam[0]) if have_prev[0] else None, None if "cam_cur" in null else C.byref(cam[1]),
            p["rgb"], p["aov"], p["variance"], p["prev_history"] if have_prev[1] else None, p["prev_aov"] if have_prev[2] else None,
            p["out_history"], p["out_variance"]]
    if fn_name.endswith("_device"):
        args = args[:5] + [C.c_void_p(C.cast(a, C.c_void_p).value) if a is not None else None for a in args[5:]] + [None]
    return getattr(L, fn_name)(*args)


STEP_FNS = ["rt_temporal_accumulate", "rt_temporal_accumulate_device"]
BAD_CONFIGS = [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(plane_tolerance=0.0), dict(plane_tolerance=float("nan")),
               dict(normal_min=-1.5), dict(normal_min=1.1), dict(normal_min=float("nan")), dict(albedo_tolerance=-0.1),
               dict(albedo_tolerance=float("nan")), dict(min_weight=0.0), dict(min_weight=1.5), dict(min_weight=float("nan")),
               dict(max_history=0), dict(max_history=65537)]


@pytest.mark.parametrize("fn_name", STEP_FNS)
@pytest.mark.parametrize("bad", BAD_CONFIGS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_bad_config_is_an_argument_error(fn_name, bad):
    import rtamd
    assert _step(fn_name, rtamd.temporal_config(**bad)) == -1
    c = C.c_void_p()
    assert rtamd.lib().rt_sequence_create(8, 8, -1, C.byref(rtamd.temporal_config(**bad)), C.byref(c)) == -1 and not c.value


@pytest.mark.parametrize("fn_name", STEP_FNS)
def test_bad_arguments_are_argument_errors(fn_name):
    import rtamd
    for name in ("cfg", "cam_cur", "rgb", "aov", "out_history"):
        assert _step(fn_name, null=(name,)) == -1, name
    for kw in (dict(w=1), dict(h=1), dict(w=0), dict(h=-4), dict(prev="cam_only"), dict(prev="history_only"), dict(prev="no_aov"),
               dict(alias=("out_history", "prev_history")), dict(alias=("out_variance", "variance")), dict(alias=("out_history", "aov"))):
        assert _step(fn_name, **kw) == -1, kw
    cfg = rtamd.temporal_config()
    cfg.reserved[4] = 1
    assert _step(fn_name, cfg) == -1 and "reserved" in rtamd.lib().rt_last_error().decode()


@pytest.mark.parametrize("fn_name", STEP_FNS)
def test_good_arguments_without_a_device_report_no_device(fn_name):
    import rtamd
    if rtamd.device_count() > 0:
        return   # (a HIP device is visible: tests/test_temporal_gpu.py covers this path)
    for kw in (dict(), dict(prev="none"), dict(null=("variance",)), dict(null=("out_variance",)), dict(cfg=rtamd.temporal_config(albedo_tolerance=float("inf")))):
        assert _step(fn_name, **kw) == -9, kw
    with pytest.raises(rtamd.RtError) as e:
        rtamd.temporal_accumulate(np.zeros((3, 4, 3)), np.zeros((3, 4, 8)), rtamd.rt_camera_frame())
    assert e.value.code == -9


def test_default_config_and_wrappers():
    import rtamd
    c = rtamd.temporal_config()
    for k, v in temporal_ref.DEFAULTS.items():
        assert getattr(c, k) == v, k
    assert list(c.reserved) == [0] * 5 and C.sizeof(rtamd.rt_temporal_config) == 64
    with pytest.raises(TypeError):
        rtamd.temporal_config(sigma=1.0)
    with pytest.raises(ValueError):
        rtamd.temporal_accumulate(np.zeros((3, 4, 3)), np.zeros((4, 3, 8)), rtamd.rt_camera_frame())


def _sequence_frame(q, scene, cam, luma_mode=1, aov_spp=2, null=(), alias=False, dn=None, **params):
    import rtamd
    p = rtamd.default_params(**dict(dict(width=8, height=8, spp=2), **params))
    out = {k: np.zeros((8, 8, n)) for k, n in (("rgb", 3), ("accum", 3), ("history", 6), ("variance", 1))}
    ptr = lambda k: None if k in null else out["rgb" if alias and k == "accum" else k].ctypes.data_as(_dp)   # noqa: E731
    return rtamd.lib().rt_sequence_frame(None if "q" in null else q, None if "s" in null else scene.h, None if "cam" in null else C.byref(cam.c),
                                         None if "p" in null else C.byref(p), C.byref(dn) if dn is not None else None, luma_mode, aov_spp,
                                         ptr("rgb"), ptr("accum"), ptr("history"), ptr("variance"), None)


def test_sequence_argument_rows_then_no_device():
    import rtamd
    L = rtamd.lib()
    q = C.c_void_p()
    for (w, h, dev) in [(1, 8, -1), (8, 1, -1), (0, 0, -1), (8, 8, -2), (65536, 65536, -1)]:
        assert L.rt_sequence_create(w, h, dev, None, C.byref(q)) == -1 and not q.value, (w, h, dev)
    assert L.rt_sequence_create(8, 8, -1, None, None) == -1
    assert L.rt_sequence_reset(None) == -1 and L.rt_sequence_frames(None) == -1
    L.rt_sequence_destroy(None)
    assert L.rt_sequence_create(8, 8, -1, None, C.byref(q)) == 0 and q.value
    try:
        assert L.rt_sequence_frames(q) == 0 and L.rt_sequence_reset(q) == 0
        world, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
        for name in ("q", "s", "cam", "p", "rgb"):
            assert _sequence_frame(q, world, cam, null=(name,)) == -1, name
        bad_dn = rtamd.denoise_config(iterations=0)
        for kw in (dict(width=9), dict(height=7), dict(aov_spp=0), dict(aov_spp=-1), dict(luma_mode=-2), dict(luma_mode=2), dict(spp=3), dict(spp=0),
                   dict(world=2), dict(world=2, rank=1), dict(kernel=3), dict(integrator=3), dict(max_depth=-1), dict(alias=True), dict(dn=bad_dn)):
            assert _sequence_frame(q, world, cam, **kw) == -1, kw
        # then what rt_denoised_render returns for the scene, before the device
        assert _sequence_frame(q, world, cam, kernel=6) == -10 and _sequence_frame(q, world, cam, integrator=2) == -10
        raw, raw_cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1, commit=False)
        assert _sequence_frame(q, raw, raw_cam) == -8
        import nested_scenes as ns
        for name in ("n5", "n6"):   # a moving sphere; ConstantMedium objects: no guides (aov_refuse)
            assert _sequence_frame(q, *ns.SCENES[name](rtamd.World())) == -10, name
        if rtamd.device_count() == 0:
            for mode in (-1, 0, 1):
                assert _sequence_frame(q, world, cam, luma_mode=mode) == -9
            assert _sequence_frame(q, world, cam, null=("accum", "history", "variance")) == -9
            assert L.rt_sequence_frames(q) == 0
    finally:
        L.rt_sequence_destroy(q)


def test_python_sequence_checks_its_arguments():
    import rtamd
    world, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    with pytest.raises(rtamd.RtError):
        rtamd.Sequence(world, 1, 8)
    with pytest.raises(TypeError):
        rtamd.Sequence(world, 8, 8, sigma=2.0)
    seq = rtamd.Sequence(world, 8, 8, alpha=0.1)
    assert seq.frames == 0
    seq.reset()
    with pytest.raises(ValueError):
        seq.frame(cam, 2, returns=("rgb", "noisy"))
    with pytest.raises(rtamd.RtError) as e:
        seq.frame(cam, 3)
    assert e.value.code == -1
    if rtamd.device_count() == 0:
        with pytest.raises(rtamd.RtError) as e:
            seq.frame(cam, 2)
        assert e.value.code == -9 and seq.frames == 0


def test_rtamd_render_sequence_without_a_device_fails_loudly(tmp_path):
    import subprocess
    import rtamd
    if rtamd.device_count() > 0:
        return   # (tests/test_temporal_gpu.py renders the frames)
    exe = os.path.join(ROOT, "rust-raytracer_amd", "rtamd_render")
    r = subprocess.run([exe, "--cube", scene_path("cube.obj"), "-w", "16", "-h", "16", "--spp", "2", "--sequence", "2", "--orbit-step", "1.5",
                        "-o", str(tmp_path / "turn.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "error -9" in r.stderr and os.listdir(tmp_path) == []


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
    for name in ("rt_sequence_create(", "rt_sequence_destroy(", "rt_sequence_frame(", "rt_sequence_reset(", "rt_sequence_frames(", "class Sequence",
                 "rt_temporal_accumulate("):
        assert name in hpp, name
    assert "impl Drop for Sequence" in rs and "pub struct Sequence" in rs
    assert rtamd.lib().rt_abi_version() == 2


def test_config_struct_has_the_same_fields_in_every_binding():
    import rtamd
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct rt_temporal_config \{(.*?)\} rt_temporal_config;", header, flags=re.S).group(1)
    fields = [re.sub(r"\[.*\]", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    assert fields == ["alpha", "plane_tolerance", "normal_min", "albedo_tolerance", "min_weight", "max_history", "reserved"]
    assert [f for f, _ in rtamd.rt_temporal_config._fields_] == fields
    rs = open(os.path.join(ROOT, "rust-raytracer_amd", "rust", "rtamd_ffi.rs")).read()
    body = re.search(r"pub struct rt_temporal_config \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == fields and "reserved: [i32; 5]" in body


# ---- quality, on the reference alone -------------------------------------------------------------------------------------------------
RECORDED_MSE_RATIO = 0.179   # accumulated / last noisy frame, against the 1024-spp frame of the last camera
ORBIT_STEP_DEG = 1.5


def test_accumulating_an_orbit_beats_doubling_the_samples():
    """Cornell 64x64, integrator 1, 8 spp per frame, 8 frames 1.5 degrees apart, seeds 100 + f, alpha 0: oracle frames and oracle guides
    (4 rays per pixel, the frame's seed) through temporal_ref; the reference is the oracle's 1024-spp frame of the last camera, seed 7.
    Measured: MSE ratio 0.179 (0.260 and 0.246 at 0 and 4 degrees per frame), 90 % of the pixels that hit something kept their history."""
    import oracle
    from test_denoise_gpu import _expected_aov, _recorded
    sc, rec = _recorded(lambda: oracle.cornell_box_scene(scene_path("cube.obj"), 1.0, 1))
    white = [m for m, (kind, t) in rec.mat.items() if kind == "lambertian" and rec.tex.get(t) == (0.75, 0.75, 0.75)][0]
    W = H = 64
    look_from, look_at = sc.camera["look_from"], sc.camera["look_at"]
    hist = prev_aov = prev_cam = None
    for f in range(8):
        sc.Camera(tc.orbit(look_from, look_at, ORBIT_STEP_DEG * f), look_at, (0.0, 1.0, 0.0), 50.0, 1.0, 0.0, 10.0)
        b = sc.camera_basis()
        cam = dict(origin=b[0:3], llc=b[3:6], hor=b[6:9], ver=b[9:12])
        rgb, _ = sc.render(W, H, 8, seed=100 + f, integrator=1)
        aov = _expected_aov(sc, rec, W, H, 4, 100 + f, white)
        info = {}
        hist, _ = temporal_ref.accumulate(rgb, aov, cam, None, hist, prev_aov, prev_cam, info=info, alpha=0.0)
        prev_aov, prev_cam = aov, cam
    ref, _ = sc.render(W, H, 1024, seed=7, integrator=1)
    ratio = np.mean((hist[..., 0:3] - ref) ** 2) / np.mean((rgb - ref) ** 2)
    kept = info["kept"][aov[..., 7] > 0].mean()
    print("MSE ratio %.4f, kept %.4f" % (ratio, kept))
    assert ratio <= 2.0 * RECORDED_MSE_RATIO and ratio < 0.5
    assert kept > 0.8
