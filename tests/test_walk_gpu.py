"""The media walks and moving spheres on the device, ray by ray: rt_debug_walk_device on the families of tests/walk_cases.py.  For every
case and every kernel the scene admits -- 1: traverse over the reference-order program, 2: the accel walk (traverse2 / traverse2_media),
3: the same over the LDS NodeW table -- the hit record (hit, t, p, normal, front_face, u, v) equals the oracle's bit for bit (a NaN equal
to any NaN), the number of random draws read from "next draw" equals the oracle's, and kernels 2 and 3 equal kernel 1 in all 14 fields.
tests/test_walk_cases.py shows without a device that the families reach what they aim at and that the oracle is right there."""
import numpy as np
import pytest

import walk_cases as wc

pytestmark = pytest.mark.gpu


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def draw_counts(keys, halves, limit=32):
    """per row the index of the u64 with these two 32-bit halves in the host's stream of the row's key: the draws consumed before it"""
    import rtamd
    out = np.zeros(len(keys), dtype=np.int64)
    for i, (key, h) in enumerate(zip(keys, halves)):
        stream = rtamd.debug_rng(int(key[0]), int(key[1]), int(key[2]), limit, device=False)
        out[i] = stream.index((int(h[0]) << 32) | int(h[1]))
    return out


def first_bad(bad):
    return int(np.flatnonzero(bad)[0])


def check_family(fam):
    import rtamd
    for case in wc.family(fam):
        w, _ = case["build"](rtamd.World())
        _, _, ref, ref_draws = wc.oracle_walk(case)
        kernels = [1, 2, 3] if w.info()["accel_ok"] else [1]
        outs = {}
        for kernel in kernels:
            dev = w.debug_walk(case["rays"], case["keys"], t_min=case["t_min"], kernel=kernel)
            outs[kernel] = dev
            draws = draw_counts(case["keys"], dev[:, 12:14])
            print("%-48s kernel %d: %4d rows, hits device %d oracle %d, draws device %s oracle %s" % (
                case["name"], kernel, len(dev), dev[:, 0].sum(), ref[:, 0].sum(), np.bincount(draws).tolist(), np.bincount(ref_draws).tolist()))
            bad = ~same(dev[:, :11], ref[:, :11]).all(axis=1)
            assert not bad.any(), "%s kernel %d: %d of %d rows differ from the oracle, first at row %d: ray %r, device %r, oracle %r" % (
                case["name"], kernel, bad.sum(), len(dev), first_bad(bad), case["rays"][first_bad(bad)].tolist(), dev[first_bad(bad)].tolist(),
                ref[first_bad(bad)].tolist())
            bad = draws != ref_draws
            assert not bad.any(), "%s kernel %d: %d rows drew another number of times, first at row %d: device %d, oracle %d" % (
                case["name"], kernel, bad.sum(), first_bad(bad), draws[first_bad(bad)], ref_draws[first_bad(bad)])
        for kernel in kernels[1:]:
            bad = ~same(outs[kernel], outs[1]).all(axis=1)
            assert not bad.any(), "%s: kernel %d differs from kernel 1 in %d rows, first at row %d: %r against %r" % (
                case["name"], kernel, bad.sum(), first_bad(bad), outs[kernel][first_bad(bad)].tolist(), outs[1][first_bad(bad)].tolist())
        if case["name"] != "nested/fog_under_chain":
            assert kernels == [1, 2, 3], case["name"]              # only a medium under a Transform leaves the accel out


@pytest.mark.parametrize("fam", wc.MEDIA_FAMILIES)
def test_media_walks_equal_the_oracle(fam):
    check_family(fam)


@pytest.mark.parametrize("fam", wc.MOTION_FAMILIES)
def test_moving_spheres_equal_the_oracle(fam):
    check_family(fam)


def test_a_scene_without_media_or_motion_walks_as_debug_hit_does():
    """the spheres-only and general variants (GENERAL 0 and 1 without MEDIA): the 12 fields of rt_debug_hit_device, no draws"""
    import rtamd
    rng = np.random.default_rng(11)
    for general in (False, True):
        w = rtamd.World()
        m = w.Lambertian(w.ConstantTexture((0.5, 0.5, 0.5)))
        items = [w.Sphere(tuple(rng.uniform(-5.0, 5.0, 3)), float(rng.uniform(0.3, 1.5)), m) for _ in range(30)]
        if general:
            items.append(w.Cube((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), m))
        w.new(items, bvh_seed=3)
        n = 333
        o = rng.uniform(-8.0, 8.0, (n, 3))
        rays = np.concatenate([o, rng.uniform(-3.0, 3.0, (n, 3)) - o, rng.uniform(-5.0, 5.0, (n, 1))], axis=1)
        keys = np.stack([np.full(n, 9, dtype=np.uint64), np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)], axis=1)
        for kernel in (1, 2, 3):
            dev = w.debug_walk(rays, keys, t_min=1e-3, kernel=kernel)
            assert np.array_equal(dev[:, :12], w.debug_hit(rays[:, :6], t_min=1e-3, kernel=kernel), equal_nan=True), (general, kernel)
            assert not draw_counts(keys, dev[:, 12:14]).any()
            assert 0.3 < dev[:, 0].mean() < 1.0
