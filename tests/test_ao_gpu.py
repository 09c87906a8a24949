"""rt_ao_render on the GPU: whole frames against tests/ao_ref.py bit for bit through both walks, the automatic walk, the
device entry point, the any-hit walk alone on the hard rays of tests/instance_scenes.py and tests/nested_scenes.py against
oracle.Scene.hit_batch, and the refusals.  tests/test_ao.py shows without a device that none of the comparisons is vacuous."""
import os
import subprocess

import numpy as np
import pytest

import ao_cases as ac
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_frame(got, exp, what):
    if not np.array_equal(_bits(got), _bits(exp)):
        bad = (_bits(got) != _bits(exp)).any(axis=2)
        y, x = np.argwhere(bad)[0]
        pytest.fail("%s: %d of %d pixels differ, first (%d, %d): got %r, expected %r" % (what, int(bad.sum()), bad.size, x, y, got[y, x].tolist(), exp[y, x].tolist()))


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("name", sorted(ac.FRAMES))
def test_frames_equal_the_reference_bit_for_bit(name, kernel):
    w, cam, _ = ac.pair(name)
    for ao_spp, K in ac.PARAMS:
        for dist in ac.distances(name):
            exp = ac.reference(name, ao_spp, K, dist)["ao"]
            got, st = w.render_ao(cam, ac.W, ac.H, ao_spp=ao_spp, rays_per_hit=K, max_distance=dist, seed=ac.SEED, kernel=kernel, t_min=ac.T_MIN)
            assert st["kernel_used"] == kernel
            _assert_frame(got, exp, "%s, kernel %d, ao_spp %d, K %d, max_distance %g" % (name, kernel, ao_spp, K, dist))
            assert (got[..., 4:7].max() > 0) == ac.has_background(name)


@pytest.mark.parametrize("name", ["cornell", "nested_n4"])
def test_automatic_walk_is_the_accel_walk(name):
    w, cam, _ = ac.pair(name)
    assert w.info()["accel_ok"] == 1
    auto, st = w.render_ao(cam, ac.W, ac.H, ao_spp=2, rays_per_hit=3, seed=ac.SEED, kernel=0)
    ref, st1 = w.render_ao(cam, ac.W, ac.H, ao_spp=2, rays_per_hit=3, seed=ac.SEED, kernel=1)
    assert st["kernel_used"] == 2 and st1["kernel_used"] == 1
    _assert_frame(auto, ref, name)
    for s in (st, st1):
        assert s["samples"] == ac.W * ac.H * 2 and s["launches"] == 1
        assert s["block_threads"] == 64 and s["grid_blocks"] == (ac.W * ac.H + 63) // 64
        assert s["kernel_ms"] > 0 and s["seconds"] > 0 and s["scene_bytes"] > 0


def test_device_entry_point_agrees_with_the_host_one():
    import torch
    import rtamd
    w, cam, _ = ac.pair("floor")
    host_frame, _ = w.render_ao(cam, ac.W, ac.H, ao_spp=2, rays_per_hit=3, max_distance=0.75, seed=ac.SEED, kernel=2)
    dev = torch.device("cuda", 0)
    out = torch.full((ac.H, ac.W, 8), -1.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    p = rtamd.default_params(width=ac.W, height=ac.H, seed=ac.SEED, kernel=2, t_min=ac.T_MIN, device=0)
    st = w.render_ao_device(cam, p, out.data_ptr(), ao_spp=2, rays_per_hit=3, max_distance=0.75, stream_ptr=stream.cuda_stream)
    torch.cuda.synchronize(dev)
    assert st["kernel_used"] == 2 and st["samples"] == ac.W * ac.H * 2
    _assert_frame(out.cpu().numpy(), host_frame, "device entry")


def test_cpp_host_writes_the_ao_image(tmp_path):
    """rtamd_render --ao (World::render_ao of rtamd.hpp over rt_ao_render): the PNG is visibility * coverage of the Python call with the
    same arguments, tone-mapped as a grey frame"""
    import rtamd
    from PIL import Image
    out = str(tmp_path / "ao.png")
    exe = os.path.join(ROOT, "rust-raytracer_amd", "rtamd_render")
    r = subprocess.run([exe, "--scene", scene_path("scene_10.json"), "-w", "48", "-h", "27", "--seed", "3", "--ao", out, "--ao-rays", "3", "--ao-distance", "2.5"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ambient occlusion (3 rays per hit): %d camera rays, kernel 2" % (48 * 27 * 4) in r.stdout, r.stdout + r.stderr
    w, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    ao, _ = w.render_ao(cam, 48, 27, ao_spp=4, rays_per_hit=3, max_distance=2.5, seed=3)
    grey = np.repeat((ao[..., 0] * ao[..., 7])[..., None], 3, axis=2)
    assert 0.0 < grey.mean() < 1.0
    assert np.array_equal(np.asarray(Image.open(out)), rtamd.tonemap_u8(grey))
    r = subprocess.run([exe, "--scene", scene_path("scene_10.json"), "-w", "16", "-h", "9", "--ao", out, "--ao-rays", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "error -1" in r.stderr                      # rays_per_hit out of range


# ---- the walk alone -----------------------------------------------------------------------------------------------------------------------
def _assert_walk(w, rays7, exp, t_min, what):
    for kernel in (1, 2):
        got = w.debug_occluded(rays7, t_min=t_min, kernel=kernel)
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, "%s, kernel %d: %d of %d rays differ, first row %d = %r: got %s" % (what, kernel, len(bad), len(exp), bad[0],
                                                                                                  rays7[bad[0]].tolist(), got[bad[0]])


@pytest.mark.parametrize("name", ac.WALK_SCENES)
def test_any_hit_walk_on_instance_rays(name):
    import instance_scenes as isc
    w = isc.world(name)
    for family in ac.WALK_FAMILIES:
        rays7, exp, t_min = ac.instance_rows(name, family)
        assert exp.any() and not exp.all()
        _assert_walk(w, rays7, exp, t_min, "%s / %s" % (name, family))


def test_any_hit_walk_on_shared_face_ties():
    rays7, exp, t_min = ac.tie_rows()
    assert exp.any() and not exp.all()
    _assert_walk(ac.tie_pair()[0], rays7, exp, t_min, "shared-face ties")


def test_any_hit_walk_at_the_exact_distance_of_a_cube_face():
    """t_max = the hit distance of a cube face that is its box's near face: World::hit misses (the reference culls the box), and so must
    both walks (found by tests/test_soup_gpu.py: the accel walk answered with the cube's own test alone)"""
    rays7, exp, t_min = ac.cube_face_rows()
    assert exp.any() and not exp.all()
    _assert_walk(ac.cube_pair()[0], rays7, exp, t_min, "cube faces")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_device_present():
    import rtamd
    _, cam, _ = ac.pair("floor")
    for w in (ac.media_world(), ac.moving_world()):
        for kernel in (0, 1, 2):
            with pytest.raises(rtamd.RtError) as e:
                w.render_ao(cam, 8, 8, kernel=kernel)
            assert e.value.code == ac.UNSUPPORTED
        with pytest.raises(rtamd.RtError) as e:
            w.debug_occluded(np.array([[0.0, 5.0, 0.0, 0.0, -1.0, 0.0, np.inf]]))
        assert e.value.code == ac.UNSUPPORTED
    w, cam, _ = ac.pair("floor")
    with pytest.raises(rtamd.RtError) as e:
        w.render_ao(cam, 8, 8, kernel=5)
    assert e.value.code == ac.ARG
    hw, hcam = ac.huge_world()
    with pytest.raises(rtamd.RtError) as e:
        hw.render_ao(hcam, 8, 8, kernel=2)
    assert e.value.code == ac.UNSUPPORTED
    with pytest.raises(rtamd.RtError) as e:
        hw.debug_occluded(np.array([[0.0, 5.0, 0.0, 0.0, -1.0, 0.0, np.inf]]), kernel=2)
    assert e.value.code == ac.UNSUPPORTED
    frame, st = hw.render_ao(hcam, 8, 8, ao_spp=1, rays_per_hit=1, kernel=0)      # the automatic choice: the reference-order walk
    assert st["kernel_used"] == 1 and frame[..., 7].max() == 1.0
