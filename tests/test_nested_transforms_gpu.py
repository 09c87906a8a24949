"""Nested Transforms on the GPU against the oracle, bit for bit (tests/nested_scenes.py: N1-N7 and the tie scene), through the
reference-order walk (kernel 1), the accel walk (kernel 2) and its LDS node table (kernel 3).  The automatic choice is kernel 2 (kernel 1
for N6: a medium under a Transform); kernels 5 / 6 have no chain walk and are refused with RT_ERR_UNSUPPORTED.  Hit maps: every pixel's
camera ray and one secondary ray from each hit (test_full_frames_gpu's _secondary_rays), fields 0-10 of rt_debug_hit_device; frames:
every pixel at a low spp through the automatic kernel and kernels 1 and 2."""
import zlib

import numpy as np
import pytest

import nested_scenes as ns
from test_full_frames_gpu import _assert_same, _secondary_rays

pytestmark = pytest.mark.gpu

W, H, SPP = 192, 128, 16
T_MIN = 1e-3
HIT_SCENES = ("n1", "n2", "n3", "n4", "n7")  # n5 has a moving sphere (debug_hit has no ray time), n6 media (no random stream)


def _both(name):
    import oracle
    import rtamd
    w, cam = ns.SCENES[name](rtamd.World())
    return w, cam, ns.SCENES[name](oracle.Scene())


def _debug_hit(world, rays, kernel):
    h, w_, _ = rays.shape
    flat = rays.reshape(-1, 6)
    ok = ~np.isnan(flat[:, 0])
    out = np.zeros((h * w_, 12))
    out[ok] = world.debug_hit(flat[ok], t_min=T_MIN, kernel=kernel)
    return out.reshape(h, w_, 12)


@pytest.mark.parametrize("name", HIT_SCENES)
def test_hit_map_matches_the_oracle(name):
    import rtamd
    w, _, o = _both(name)
    rays = o.camera_rays(W, H, seed=1, sample=0)
    rec = o.hit_batch(rays.reshape(-1, 6), t_min=T_MIN, n_workers=16).reshape(H, W, 12)
    assert rec[..., 0].mean() > 0.3  # (the box fills about a third of the 3:2 frame)
    sec = _secondary_rays(rays, rec, seed=zlib.crc32(name.encode()))
    hit = ~np.isnan(sec[..., 0])
    rec2 = np.zeros((H, W, 12))
    rec2[hit] = o.hit_batch(sec[hit], t_min=T_MIN, n_workers=16)
    for k in (1, 2, 3):
        _assert_same(_debug_hit(w, rays, k)[..., :11], rec[..., :11], "%s primary hits, kernel %d" % (name, k))
        _assert_same(_debug_hit(w, sec, k)[..., :11], rec2[..., :11], "%s secondary hits, kernel %d" % (name, k))
    for k in (5, 6):
        with pytest.raises(rtamd.RtError) as e:
            w.debug_hit(rays.reshape(-1, 6)[:64], t_min=T_MIN, kernel=k)
        assert e.value.code == -10


@pytest.mark.parametrize("name", sorted(ns.SCENES))
def test_whole_frame_matches_the_oracle(name):
    import rtamd
    w, cam, o = _both(name)
    shutter = (0.0, 1.0) if name == "n5" else (0.0, 0.0)
    exp, _ = o.render(W, H, SPP, seed=1, n_jobs=16, n_workers=16)
    assert float((exp != 0).any(axis=2).mean()) > 0.1
    auto = 1 if name == "n6" else 2
    for kernel in (0, 1, 2) if auto == 2 else (0, 1):
        img, st = w.render(cam, width=W, height=H, spp=SPP, seed=1, kernel=kernel, shutter=shutter)
        assert st["kernel_used"] == (auto if kernel == 0 else kernel) and st["samples"] == W * H * SPP
        _assert_same(img, exp, "%s %dx%dx%d kernel %d" % (name, W, H, SPP, kernel))
    for kernel in (5, 6) if auto == 2 else (2, 5, 6):
        with pytest.raises(rtamd.RtError) as e:
            w.render(cam, width=W, height=H, spp=1, seed=1, kernel=kernel, shutter=shutter)
        assert e.value.code == -10


def test_mixture_integrator_matches_the_oracle():
    w, cam, o = _both("n1")
    exp, _ = o.render(W, H, SPP, seed=1, n_jobs=16, n_workers=16, integrator=1)
    for kernel in (1, 2):
        img, st = w.render(cam, width=W, height=H, spp=SPP, seed=1, kernel=kernel, integrator=1)
        assert st["kernel_used"] == kernel
        _assert_same(img, exp, "n1 integrator 1, kernel %d" % kernel)


@pytest.mark.parametrize("kernel", [1, 2])
def test_sppm_matches_the_oracle(kernel):
    cfg = dict(iterations=2, photons_per_iter=4000, k_global=40, k_caustic=10)
    w, cam, o = _both("n1")
    img, st, tot, _ = w.render_sppm(cam, width=24, height=16, spp=2, seed=1, kernel=kernel, **cfg)
    eimg, est, etot = o.render_sppm(24, 16, 2, seed=1, n_workers=16, **cfg)
    assert tot == etot and tot[0] > 0
    assert np.array_equal(st, est), "per-pixel SPPM statistics differ"
    assert np.array_equal(img, eimg, equal_nan=True)


def test_shared_face_ties_match_the_oracle():
    """two cubes share the face x = 200, one at depth 1 and one at depth 3: rays from inside either cube aimed at that face"""
    import oracle
    import rtamd
    w, _ = ns.tie(rtamd.World())
    o = ns.tie(oracle.Scene())
    rays = ns.tie_rays()
    exp = o.hit_batch(rays, t_min=T_MIN, n_workers=16)
    assert exp[:, 0].mean() > 0.9
    for k in (1, 2, 3):
        got = w.debug_hit(rays, t_min=T_MIN, kernel=k)
        _assert_same(got[None, :, :11], exp[None, :, :11], "shared-face ties, kernel %d" % k)


def test_nested_torus_refuses_kernels_5_and_6():
    import rtamd
    w, cam = ns.n2(rtamd.World(), nu=64, nv=64)
    for k in (5, 6):
        with pytest.raises(rtamd.RtError) as e:
            w.render(cam, width=16, height=16, spp=1, seed=1, kernel=k)
        assert e.value.code == -10
    _, st = w.render(cam, width=16, height=16, spp=1, seed=1)
    assert st["kernel_used"] == 2
