"""Shading, textures and object lights on the device, point by point: rt_debug_shade_device, rt_debug_light_sample_device and
rt_debug_light_pdf_device on the families of tests/shade_cases.py, every output equal to the oracle's bit for bit (a NaN equal to any
NaN: x86 and the GPU make different default NaNs), the unit-zero status and the number of draws included.  tests/test_shade_cases.py
shows without a device that the families reach the branches they aim at and that the oracle is right there."""
import numpy as np
import pytest

import shade_cases as sc

pytestmark = pytest.mark.gpu

_WORLD = {}


def world(noise=True):
    if noise not in _WORLD:
        _WORLD[noise] = sc.product_world(noise)
    return _WORLD[noise]


def draw_index(key, halves, limit=64):
    """the index of the u64 with these two 32-bit halves in the host's stream of `key`: the draws consumed before it"""
    import rtamd
    stream = rtamd.debug_rng(int(key[0]), int(key[1]), int(key[2]), limit, device=False)
    return stream.index((int(halves[0]) << 32) | int(halves[1]))


def compare(name, dev, ref, cols, rows=None):
    rows = np.ones(len(dev), dtype=bool) if rows is None else rows
    bad = rows & ~sc.same(dev[:, cols], ref[:, cols]).all(axis=1)
    assert not bad.any(), "%s: %d of %d rows differ in columns %s, first at row %d: device %r, oracle %r" % (
        name, bad.sum(), rows.sum(), cols, np.flatnonzero(bad)[0], dev[np.flatnonzero(bad)[0], cols], ref[np.flatnonzero(bad)[0], cols])


@pytest.mark.parametrize("name", list(sc.SHADE_FAMILIES))
def test_shade_equals_the_oracle(name):
    _shade_equals_the_oracle(name, True)


@pytest.mark.parametrize("name", [n for n in sc.SHADE_FAMILIES if n != "noise"])
def test_shade_without_a_noise_texture_equals_the_oracle(name):
    """the same families on the scene built without the marble (the materials keep their indices: the marble is the last one): a scene
    without a noise texture shades through the kernel form that holds no noise code (shade_eval_kernel<1>, as render_tiles chooses the
    GENERAL == 1 variants), which the families above never launch"""
    _shade_equals_the_oracle(name, False)


def _shade_equals_the_oracle(name, noise):
    w, _, _ = world(noise)
    o, _ = sc.oracle_scene(noise)
    f = sc.family(name)
    dev = w.debug_shade(f["rows"], f["keys"])
    ref, draws = o.shade(f["rows"], f["keys"])
    for what, col in (("scattered", 0), ("diffuse", 1), ("mixed", 11), ("continued", 12), ("status", 19)):
        print("%s %s: device %d, oracle %d of %d rows" % (name, what, dev[:, col].sum(), ref[:, col].sum(), len(dev)))
    compare(name, dev, ref, [19])
    ok = ref[:, 19] == 0                                   # where unit() met a zero vector the oracle stops: only the status compares
    compare(name, dev, ref, [0, 1, 11, 12], ok)
    compare(name, dev, ref, [8, 9, 10], ok)                # emitted
    compare(name, dev, ref, [2, 3, 4, 5, 6, 7], ok & (ref[:, 0] == 1))     # out_dir, att of a scattered ray
    compare(name, dev, ref, [16, 17, 18], ok)              # the mixture step's direction (out_dir without one)
    compare(name, dev, ref, [13, 14, 15], ok)              # beta: (1, 1, 1) unless continued
    compare(name, dev, ref, [20, 21], ok)                  # the next draw
    for i in np.flatnonzero(ok)[::max(1, ok.sum() // 400)]:
        assert draw_index(f["keys"][i], dev[i, 20:22]) == draws[i], (name, i)


def test_light_samples_equal_the_oracle():
    w, _, _ = world()
    o, _ = sc.oracle_scene()
    f = sc.family("light_samples")
    dev = w.debug_light_sample(f["o_light"], f["keys"])
    ref, draws = o.light_sample(f["o_light"], f["keys"])
    compare("light_samples", dev, ref, [3])
    ok = ref[:, 3] == 0
    assert ok.sum() > 250 and (~ok).sum() == 6
    compare("light_samples", dev, ref, [0, 1, 2, 4, 5], ok)
    for i in np.flatnonzero(ok):
        assert draw_index(f["keys"][i], dev[i, 4:6], 256) == draws[i], i


def test_light_pdfs_equal_the_oracle_light_by_light():
    w, _, _ = world()
    o, _ = sc.oracle_scene()
    rays = sc.family("light_pdf_rays")["rays"]
    mix = sc.family("mixture")
    final = o.shade(mix["rows"], mix["keys"])[0][:, 16:19]
    rays = np.concatenate([rays, np.concatenate([mix["rows"][:, 8:11], final], axis=1)])      # and the mixture rows' own rays
    dev = w.debug_light_pdf(rays)
    ref = o.light_pdf(rays)
    assert dev.shape == ref.shape == (len(rays), 3)
    for light in range(3):
        compare("pdf of light %d" % light, dev, ref, [light])


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("integrator", [0, 1])
def test_case_scene_frames_equal_the_oracle(kernel, integrator):
    """the render kernels run the functions the diagnostics drive: the case scene through kernels 1 and 2.  A scene with a noise texture
    renders with integrator 0 only, so integrator 1 gets the same scene without its marble sphere"""
    noise = integrator == 0
    w, cam, _ = world(noise)
    o, _ = sc.oracle_scene(noise)
    img, st = w.render(cam, width=32, height=32, spp=8, seed=5, kernel=kernel, integrator=integrator)
    ref, _ = o.render(32, 32, 8, seed=5, integrator=integrator)
    assert st["kernel_used"] == kernel
    assert np.array_equal(img, ref, equal_nan=True), "%d pixels differ" % (img != ref).any(axis=2).sum()
    assert img.max() > 0


def _marble_far(B):
    c = 2.0 ** 27
    marble = B.Lambertian(B.NoiseTexture(sc.NOISE_SCALE, sc.NOISE_SEED))
    return [B.Sphere((c, 0.0, 0.0), 1.0, marble), B.XZRectangle((c - 4.0, -4.0), (c + 4.0, 4.0), -1.0, marble),
            B.Sphere((c, 0.0, 0.0), 40.0, B.DiffuseLight(B.ConstantTexture((1.0, 1.0, 1.0))))]


@pytest.mark.parametrize("kernel", [1, 2])
def test_marble_sphere_at_2_to_the_27_equals_the_oracle(kernel):
    """the lattice rule at frame level: every octave of the marble beyond the first leaves the range of int at x = 2^27"""
    import oracle
    import rtamd
    c = 2.0 ** 27
    w = rtamd.World()
    w.new(_marble_far(w), bvh_seed=2)
    o = oracle.Scene()
    o.World(_marble_far(o), 2)
    cam = ((c + 0.5, 1.0, -5.0), (c, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, 1.0, 0.0, 5.0)
    o.Camera(*cam)
    try:
        img, st = w.render(rtamd.Camera((cam[0], cam[1]), *cam[2:]), width=24, height=24, spp=4, seed=3, kernel=kernel)
    except rtamd.RtError as e:
        assert kernel == 2 and e.code == -10, e            # RT_ERR_UNSUPPORTED: the accel does not take a camera this far out
        return
    ref, _ = o.render(24, 24, 4, seed=3)
    assert st["kernel_used"] == kernel
    assert np.array_equal(img, ref, equal_nan=True), "%d pixels differ" % (img != ref).any(axis=2).sum()
    assert len(np.unique(img)) > 100
