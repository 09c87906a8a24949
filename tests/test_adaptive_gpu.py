"""Tile-adaptive sampling (rt_render_adaptive) on the GPU, checked exactly without the oracle: a tile that stops after n_T
samples is rt_render's frame at spp = n_T on that tile, bit for bit, so the stopping decisions can be restated on the host from plain
rt_render frames at spp 2h, 4h, ... -- e_T in the header's operation order, summed one pixel at a time (no np.sum: it adds pairwise)."""
import math

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu


def tile_error(I, A, tx, ty):
    """e_T of tile (tx, ty) from I = S_n / n and A = S_m / m ([H, W, 3] frames), as rtamd.h states it"""
    H, W = I.shape[:2]
    total, count = 0.0, 0
    for y in range(ty * 8, min(ty * 8 + 8, H)):
        for x in range(tx * 8, min(tx * 8 + 8, W)):
            ir, ig, ib = (float(v) for v in I[y, x])
            ar, ag, ab = (float(v) for v in A[y, x])
            s = (ir + ig) + ib
            total = total + (((abs(ir - ar) + abs(ig - ag)) + abs(ib - ab)) / math.sqrt(s) if s > 0 else 0.0)
            count += 1
    return total / float(count)


def schedule_tests(min_spp, spp):
    """the sample counts n after which the active tiles are tested: 2h, 4h, ... below spp"""
    n, out = min_spp, []
    while n < spp:
        out.append(n)
        n *= 2
    return out


def frames_for(world, cam, width, height, spp, min_spp, **kw):
    """rt_render frames at every sample count a tile can stop at, and at the half counts the tests compare with"""
    counts = {min_spp // 2, spp}
    for n in schedule_tests(min_spp, spp):
        counts.update((n, n // 2))
    return {n: world.render(cam, width=width, height=height, spp=n, **kw)[0] for n in sorted(counts)}


def predict(frames, min_spp, spp, threshold):
    """each tile's n_T, and the errors of the first test"""
    H, W = frames[spp].shape[:2]
    ty_n, tx_n = (H + 7) // 8, (W + 7) // 8
    n_t = np.full((ty_n, tx_n), spp, dtype=np.int32)
    active = [(ty, tx) for ty in range(ty_n) for tx in range(tx_n)]
    first = None
    for n in schedule_tests(min_spp, spp):
        errs = {t: tile_error(frames[n], frames[n // 2], t[1], t[0]) for t in active}
        if first is None:
            first = errs
        for t, e in errs.items():
            if e < threshold:
                n_t[t] = n
        active = [t for t in active if not errs[t] < threshold]
    return n_t, first


def median_nonzero(errs):
    nz = sorted(e for e in errs.values() if e > 0)
    assert nz, "every tile of the first test has e_T = 0"
    return nz[len(nz) // 2]


def assert_tiles_are_rt_render(img, tile_spp, frames):
    H, W = img.shape[:2]
    for ty in range(tile_spp.shape[0]):
        for tx in range(tile_spp.shape[1]):
            ref = frames[int(tile_spp[ty, tx])]
            sl = np.s_[ty * 8:min(ty * 8 + 8, H), tx * 8:min(tx * 8 + 8, W)]
            assert np.array_equal(img[sl], ref[sl]), "tile (%d, %d), n_T = %d" % (tx, ty, tile_spp[ty, tx])


def in_image_pixels(W, H):
    return np.array([[min(8, W - tx * 8) * min(8, H - ty * 8) for tx in range((W + 7) // 8)] for ty in range((H + 7) // 8)], dtype=np.int64)


def check_config(world, cam, width, height, spp, min_spp, kernel, integrator=0, min_distinct=2):
    kw = dict(kernel=kernel, integrator=integrator, seed=1)
    frames = frames_for(world, cam, width, height, spp, min_spp, **kw)
    _, first = predict(frames, min_spp, spp, 0.0)
    threshold = median_nonzero(first)
    want, _ = predict(frames, min_spp, spp, threshold)
    img, tile_spp, st = world.render_adaptive(cam, width, height, spp, min_spp=min_spp, threshold=threshold, **kw)
    assert st["kernel_used"] == (kernel or st["kernel_used"])
    assert tile_spp.shape == ((height + 7) // 8, (width + 7) // 8)
    assert np.array_equal(tile_spp, want), "n_T map differs from the host restatement"
    assert len(np.unique(tile_spp)) >= min_distinct, np.unique(tile_spp)
    assert_tiles_are_rt_render(img, tile_spp, frames)
    assert st["samples"] == int((tile_spp.astype(np.int64) * in_image_pixels(width, height)).sum())
    return img, tile_spp, st


def test_scene_10_decisions_and_pixels_are_exact():
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    check_config(world, cam, 96, 64, 64, 4, kernel=2, min_distinct=3)


def test_cornell_light_sampling_is_exact():
    import rtamd
    world, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    check_config(world, cam, 64, 64, 64, 4, kernel=0, integrator=1)


def test_cornell_torus_kernel_5_is_exact():
    import rtamd
    from rtamd import shapes
    world = rtamd.World()
    P, N, I = shapes.torus(24, 48)
    world.new(shapes.cornell_with_mesh(world, P, N, I), bvh_seed=1)
    cam = rtamd.Camera(((278, 278, -800), (278, 278, 278)), (0, 1, 0), 50, 1.0, 0.0, 10.0)
    _, _, st = check_config(world, cam, 64, 64, 32, 4, kernel=5)
    assert st["kernel_used"] == 5


def test_kernel_1_is_exact():
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    _, _, st = check_config(world, cam, 96, 64, 32, 4, kernel=1)
    assert st["kernel_used"] == 1


def test_partial_edge_tiles_are_exact():
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    check_config(world, cam, 100, 61, 32, 2, kernel=2)


def test_threshold_0_is_rt_render():
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    ref, _ = world.render(cam, width=96, height=64, spp=37, seed=3, kernel=2)
    img, tile_spp, st = world.render_adaptive(cam, 96, 64, 37, min_spp=4, threshold=0.0, seed=3, kernel=2)
    assert np.array_equal(img, ref)
    assert (tile_spp == 37).all()
    assert st["samples"] == 96 * 64 * 37
    assert st["launches"] >= 6   # [0,2) [2,4) [4,8) [8,16) [16,32) [32,37)


def test_background_tiles_stop_at_min_spp_and_fewer_samples_are_traced():
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    W, H, spp, min_spp = 96, 64, 64, 8
    frames = frames_for(world, cam, W, H, spp, min_spp, seed=1)
    _, first = predict(frames, min_spp, spp, 0.0)
    sky = [t for t, e in first.items() if e == 0.0]
    assert len(sky) >= 10, "scene_10 should see background-only tiles"
    for thr in (1e-12, 0.01, 1.0):
        img, tile_spp, st = world.render_adaptive(cam, W, H, spp, min_spp=min_spp, threshold=thr, seed=1)
        for t in sky:
            assert tile_spp[t] == min_spp
        assert st["samples"] == int((tile_spp.astype(np.int64) * in_image_pixels(W, H)).sum())
        assert st["samples"] < W * H * spp
        assert_tiles_are_rt_render(img, tile_spp, frames)


def test_result_does_not_depend_on_the_schedule(tuning):
    import rtamd
    world, cam = rtamd.load_scene_file(scene_path("scene_10.json"))
    args = (cam, 96, 64, 48)
    kw = dict(min_spp=4, threshold=0.05, seed=5, kernel=2)
    img0, map0, _ = world.render_adaptive(*args, **kw)
    img1, map1, _ = world.render_adaptive(*args, **kw)
    assert np.array_equal(img0, img1) and np.array_equal(map0, map1)
    assert len(np.unique(map0)) >= 2
    tuning(sub_spp=1)
    img2, map2, _ = world.render_adaptive(*args, **kw)
    tuning()
    img3, map3, st3 = world.render_adaptive(*args, spp_chunk=3, **kw)
    assert st3["launches"] > 8
    for img, m in ((img2, map2), (img3, map3)):
        assert np.array_equal(m, map0)
        assert np.array_equal(img, img0)


def test_kernel_6_and_sppm_are_refused():
    import rtamd
    world, cam = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    for kw in (dict(kernel=6), dict(integrator=2)):
        with pytest.raises(rtamd.RtError) as e:
            world.render_adaptive(cam, 32, 32, 16, min_spp=4, threshold=0.01, **kw)
        assert e.value.code == -10   # RT_ERR_UNSUPPORTED
