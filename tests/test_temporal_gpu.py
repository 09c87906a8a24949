"""Temporal accumulation on the GPU.  The step (rt_temporal_accumulate, rt_temporal_accumulate_device) against tests/temporal_ref.py bit
for bit on uint64 views: seeded random frame pairs at sizes with partial blocks on both axes, one full block and the smallest frame, and
the crafted rows of tests/temporal_cases.py.  Sequence.frame against the composition of the host entries rt_denoised_render ->
rt_temporal_accumulate -> rt_denoise / rt_denoise_sym (existing tests hold rt_denoised_render's stages against the oracle), its automatic
reset on another scene, and its refusals."""
import os
import sys

import numpy as np
import pytest

import temporal_cases as tc
import temporal_ref
from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import configs  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(got, exp, what):
    bad = np.argwhere(_bits(got) != _bits(exp))
    assert bad.size == 0, "%s: %d values differ, first at %s: %r vs %r" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def _frames(k):
    """the inputs with the camera dicts turned into rt_camera_frame structs (the four fields the step reads; the rest stays 0)"""
    import rtamd

    def frame(c):
        if c is None:
            return None
        f = rtamd.rt_camera_frame()
        for name, key in (("origin", "origin"), ("lower_left_corner", "llc"), ("horizontal", "hor"), ("vertical", "ver")):
            for i in range(3):
                getattr(f, name)[i] = float(c[key][i])
        return f
    return dict(k, cam_cur=frame(k["cam_cur"]), cam_prev=frame(k.get("cam_prev")))


def _both(k, **cfg):
    import rtamd
    exp_h, exp_v = temporal_ref.accumulate(**k, **cfg)
    got_h, got_v = rtamd.temporal_accumulate(return_variance=True, **_frames(k), **cfg)
    return got_h, got_v, exp_h, exp_v


CONFIGS = [dict(), dict(alpha=0.0, max_history=8), dict(albedo_tolerance=float("inf"), normal_min=-1.0, plane_tolerance=0.2, min_weight=1.0)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "running_mean", "loose"])
@pytest.mark.parametrize("size", [(21, 37), (16, 16), (2, 2)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_step_matches_the_numpy_restatement(size, cfg):
    h, w = size
    k = tc.random_inputs(h, w, seed=h * 100 + w)
    got_h, got_v, exp_h, exp_v = _both(k, **cfg)
    _check(got_h, exp_h, "history")
    _check(got_v, exp_v, "variance")
    # without a variance input, and on a first frame
    k2 = dict(k, variance=None)
    got_h, got_v, exp_h, exp_v = _both(k2, **cfg)
    _check(got_h, exp_h, "history, no variance")
    _check(got_v, exp_v, "variance, no variance input")
    first = dict(rgb=k["rgb"], aov=k["aov"], variance=k["variance"], cam_cur=k["cam_cur"])
    got_h, got_v, exp_h, exp_v = _both(first, **cfg)
    _check(got_h, exp_h, "first frame")
    _check(got_v, exp_v, "first frame's variance")


@pytest.mark.parametrize("name", sorted(tc.REJECTIONS))
def test_crafted_rows(name):
    k, plain, cfg, (y, x) = tc.rejection(name)
    got_h, got_v, exp_h, exp_v = _both(k, **cfg)
    assert got_h[y, x, 5] == 1.0
    _check(got_h, exp_h, "history")
    _check(got_v, exp_v, "variance")
    got_h, got_v, exp_h, exp_v = _both(plain, **cfg)
    _check(got_h, exp_h, "history without the crafted value")


def test_shift_and_running_mean_on_the_device():
    k = tc.base(shift_px=1.0)
    got_h, got_v, exp_h, exp_v = _both(k, alpha=0.0)
    assert np.all(got_h[:, :-1, 5] == 4.0) and np.all(got_h[:, -1, 5] == 1.0)
    _check(got_h, exp_h, "history")
    _check(got_v, exp_v, "variance")


def test_device_twin_equals_the_host_entry():
    import torch
    import rtamd
    h, w = 21, 37
    k = _frames(tc.random_inputs(h, w, seed=5))
    exp_h, exp_v = rtamd.temporal_accumulate(return_variance=True, **k)
    dev = {n: torch.from_numpy(np.ascontiguousarray(k[n])).cuda() for n in ("rgb", "aov", "variance", "prev_history", "prev_aov")}
    out_h = torch.full((h, w, 6), -1.0, dtype=torch.float64, device="cuda")
    out_v = torch.full((h, w), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rtamd.temporal_accumulate_device(w, h, k["cam_cur"], dev["rgb"].data_ptr(), dev["aov"].data_ptr(), out_h.data_ptr(),
                                     d_variance_ptr=dev["variance"].data_ptr(), d_prev_history_ptr=dev["prev_history"].data_ptr(),
                                     d_prev_aov_ptr=dev["prev_aov"].data_ptr(), cam_prev=k["cam_prev"], d_out_variance_ptr=out_v.data_ptr())
    _check(out_h.cpu().numpy(), exp_h, "history")
    _check(out_v.cpu().numpy(), exp_v, "variance")
    # the optional pointers left out: a first frame, no variance in or out
    out_h.fill_(-1.0)
    torch.cuda.synchronize()
    rtamd.temporal_accumulate_device(w, h, k["cam_cur"], dev["rgb"].data_ptr(), dev["aov"].data_ptr(), out_h.data_ptr())
    _check(out_h.cpu().numpy(), rtamd.temporal_accumulate(k["rgb"], k["aov"], k["cam_cur"]), "first frame")


# ---- the sequence --------------------------------------------------------------------------------------------------------------------
W = H = 40
SPP, AOV_SPP = 4, 2
_CACHE = {}


def _cornell():
    if "cornell" not in _CACHE:
        _CACHE["cornell"] = configs.product("cornell")
    return _CACHE["cornell"]


def _orbit(cam, deg):
    import rtamd
    c = rtamd.rt_camera.from_buffer_copy(cam.c)
    lf = tc.orbit(tuple(cam.c.look_from), tuple(cam.c.look_at), deg)
    for i in range(3):
        c.look_from[i] = lf[i]
    return rtamd.Camera.from_struct(c)


def _stage_a():
    """rt_denoised_render's noisy frame, variance and guides of the three frames, once for all luma modes: (camera, noisy, variance, aov)"""
    if "stage_a" not in _CACHE:
        world, cam = _cornell()
        rows = []
        for f in range(3):
            c = _orbit(cam, 2.0 * f)
            _, noisy, var, aov = world.render_denoised(c, width=W, height=H, spp=SPP, aov_spp=AOV_SPP, seed=11 + f, integrator=1, native=True, luma_mode=0,
                                                           iterations=1)
            rows.append((c, noisy, var, aov))
        _CACHE["stage_a"] = rows
    return _CACHE["stage_a"]


@pytest.mark.parametrize("luma_mode", [-1, 0, 1])
def test_sequence_frame_is_the_composition_of_the_host_entries(luma_mode):
    import rtamd
    world, _ = _cornell()
    seq = rtamd.Sequence(world, W, H, alpha=0.1)
    hist = prev_aov = prev_cam = None
    for f, (cam, noisy, var, aov) in enumerate(_stage_a()):
        rgb, accum, history, variance, st = seq.frame(cam, SPP, seed=11 + f, aov_spp=AOV_SPP, luma_mode=luma_mode, integrator=1,
                                                      returns=("rgb", "accum", "history", "variance", "stats"))
        assert seq.frames == f + 1 and st["samples"] == W * H * SPP
        exp_h, exp_v = rtamd.temporal_accumulate(noisy, aov, cam, var, hist, prev_aov, prev_cam, return_variance=True, alpha=0.1)
        ref_h, ref_v = temporal_ref.accumulate(noisy, aov, temporal_ref.frame_of_struct(cam.frame()), var, hist, prev_aov,
                                               temporal_ref.frame_of_struct(prev_cam.frame()) if prev_cam else None, alpha=0.1)
        _check(exp_h, ref_h, "frame %d: the step on stage A's outputs against temporal_ref" % f)
        _check(exp_v, ref_v, "frame %d: the step's variance against temporal_ref" % f)
        _check(history, exp_h, "frame %d: history" % f)
        _check(variance, exp_v, "frame %d: variance" % f)
        _check(accum, exp_h[..., 0:3], "frame %d: accumulated colour" % f)
        if luma_mode < 0:
            _check(rgb, accum, "frame %d: unfiltered output" % f)
        else:
            _check(rgb, rtamd.denoise(accum, exp_v, aov, symmetric=luma_mode == 1), "frame %d: filtered output" % f)
        hist, prev_aov, prev_cam = exp_h, aov, cam
    # the history path ran, not only resets: the five diffuse walls of the box fill well over half of the frame and reproject exactly, and
    # each of the two steps loses only the pixels beside their edges and under the light -- a quarter of the frame is far below that
    assert (hist[..., 5] == 3.0).mean() > 0.25, "a good part of the frame keeps its history over two 2 degree steps"
    seq.reset()
    assert seq.frames == 0
    cam, noisy, var, aov = _stage_a()[0]
    history = seq.frame(cam, SPP, seed=11, aov_spp=AOV_SPP, luma_mode=-1, integrator=1, returns="history")
    assert np.all(history[..., 5] == 1.0) and seq.frames == 1


def test_default_seed_advances_with_the_frames():
    import rtamd
    world, cam = _cornell()
    seq = rtamd.Sequence(world, W, H)
    a = seq.frame(cam, 2, aov_spp=1, luma_mode=-1, returns="accum")
    b = seq.frame(cam, 2, aov_spp=1, luma_mode=-1, returns="history")
    first, _ = world.render(cam, width=W, height=H, spp=2, seed=1)
    second, _ = world.render(cam, width=W, height=H, spp=2, seed=2)
    _check(a, first, "frame 0 is rt_render's frame of seed 1")
    hit = b[..., 5] == 2.0
    # (a still camera reprojects a pixel onto itself up to rounding: the neighbours' bilinear weights are of the order of 1e-13)
    assert hit.mean() > 0.25 and np.allclose(b[hit][:, 0:3], 0.5 * (first[hit] + second[hit]), rtol=1e-9, atol=1e-9)


def test_another_scene_resets_the_history():
    import rtamd
    world, cam = _cornell()
    other, _ = rtamd.load_scene_file(scene_path("scene_10.json"))
    assert other.fingerprint() != world.fingerprint()
    seq = rtamd.Sequence(world, W, H)
    seq.frame(cam, 2, aov_spp=1, luma_mode=-1)
    h1 = seq.frame(cam, 2, aov_spp=1, luma_mode=-1, returns="history")
    assert seq.frames == 2 and (h1[..., 5] == 2.0).any()
    h2 = seq.frame(cam, 2, aov_spp=1, luma_mode=-1, returns="history", world=other)
    assert seq.frames == 1 and np.all(h2[..., 5] == 1.0)
    h3 = seq.frame(cam, 2, aov_spp=1, luma_mode=-1, returns="history", world=other)
    assert seq.frames == 2 and (h3[..., 5] == 2.0).any()


def test_refusals_come_before_the_device():
    import ctypes as C
    import nested_scenes as ns
    import rtamd
    world, cam = _cornell()
    seq = rtamd.Sequence(world, W, H)
    with pytest.raises(rtamd.RtError) as e:
        seq.frame(cam, 2, aov_spp=0)
    assert e.value.code == -1
    # a size mismatch: the params of a 40 x 40 frame to a sequence of 48 x 40
    bigger = rtamd.Sequence(world, W + 8, H)
    p = rtamd.default_params(width=W, height=H, spp=2)
    out = np.zeros((H, W + 8, 3))
    rc = rtamd.lib().rt_sequence_frame(bigger.h, world.h, C.byref(cam.c), C.byref(p), None, -1, 1, out.ctypes.data_as(C.POINTER(C.c_double)), None, None,
                                       None, None)
    assert rc == -1 and b"sequence" in rtamd.lib().rt_last_error() and bigger.frames == 0
    # a scene with ConstantMedium objects has no guides
    fog, fog_cam = ns.SCENES["n6"](rtamd.World())
    with pytest.raises(rtamd.RtError) as e:
        seq.frame(fog_cam, 2, world=fog)
    assert e.value.code == -10 and "ConstantMedium" in str(e.value) and seq.frames == 0


def test_rtamd_render_sequence_writes_the_frames_of_a_python_sequence(tmp_path):
    """rtamd_render --sequence N --orbit-step DEG: NAME_%03d.png per frame, the camera turned about look_at around the y axis, frame f with
    seed + f -- the frames rtamd.Sequence renders for the same cameras and seeds (luma mode 1, 4 guide rays: the tool's defaults)"""
    import subprocess
    import rtamd
    from PIL import Image
    exe = os.path.join(ROOT, "rust-raytracer_amd", "rtamd_render")
    r = subprocess.run([exe, "--cube", scene_path("cube.obj"), "-w", "24", "-h", "24", "--spp", "2", "--seed", "5", "--sequence", "2", "--orbit-step", "3",
                        "-o", str(tmp_path / "turn.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "frame 1 of 2" in r.stdout, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["turn_000.png", "turn_001.png"]
    world, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    seq = rtamd.Sequence(world, 24, 24)
    for f in range(2):
        exp = seq.frame(_orbit(cam, 3.0 * f), 2, seed=5 + f, returns="rgb")
        assert np.array_equal(np.asarray(Image.open(tmp_path / ("turn_%03d.png" % f))), rtamd.tonemap_u8(exp)), f
