"""The instance walks of kernels 5 / 6 on explicit rays (tests/instance_scenes.py; tests/test_instance_scenes.py keeps these tests from going
vacuous).  rt_debug_hit_device runs them in one lane: kernel 6 the serving waves' blas_pass_q over the compact NodeQ / Tri32 records with the
ray mapped onto the instance's 16-bit grid, kernel 5 blas_pass over the Node2 records (kernel 5's in-lane fallback).  Closest-hit records of
every (scene, ray family): kernel 1 -- the reference-order program -- against the oracle in fields 0-10 (the oracle's prim_id counts other
things, test_walk_stack._check_hits), kernels 2, 3, 5 and 6 against kernel 1 in all twelve.  Then one small frame per scene through the
render kernels, which carry copies of the grid mapping that the one-lane walk does not run (pt_kernel_coop, coop_serve, wavefront.inc), also
with NodeQ read from global memory (top_nodes=0), through kernel 5's in-lane fallback (coop_pool=1) and with kernel 2's scene out of LDS."""
import numpy as np
import pytest

import instance_scenes as S

pytestmark = pytest.mark.gpu

PAIRS = [(n, f) for n in S.SCENES for f in S.families(n)]
ORACLE_FRAME = ("scale[250]", "small_in_big[4000]", "needle", "flat", "box")     # one scene of each family against the oracle's frame


def _differing(a, b):
    return np.flatnonzero(((a != b) & ~(np.isnan(a) & np.isnan(b))).any(axis=1))


@pytest.mark.parametrize("name,family", PAIRS)
def test_hit_records(name, family):
    F = S.rays(name, family)
    rays, t_max = F["rays"], F["t_max"]
    world = S.world(name)
    exp = S.ref(name)["full"].hit_batch(rays, t_min=S.T_MIN, t_max=t_max, n_workers=4)
    k1 = world.debug_hit(rays, t_min=S.T_MIN, t_max=t_max, kernel=1)
    failures = []
    bad = _differing(k1[:, :11], exp[:, :11])
    if len(bad):
        failures.append("kernel 1 differs from the oracle in %d of %d rows, first: ray %d %r\n  oracle   %r\n  kernel 1 %r" % (
            len(bad), len(rays), bad[0], rays[bad[0]].tolist(), exp[bad[0]].tolist(), k1[bad[0]].tolist()))
    for k in (2, 3, 5, 6):
        got = world.debug_hit(rays, t_min=S.T_MIN, t_max=t_max, kernel=k)
        bad = _differing(got, k1)
        print("%s %s: kernel %d differs from kernel 1 in %d of %d rows" % (name, family, k, len(bad), len(rays)))
        if len(bad):
            failures.append("kernel %d differs from kernel 1 in %d of %d rows, first: ray %d %r\n  kernel 1 %r\n  kernel %d %r" % (
                k, len(bad), len(rays), bad[0], rays[bad[0]].tolist(), k1[bad[0]].tolist(), k, got[bad[0]].tolist()))
    assert not failures, "%s, %s:\n" % (name, family) + "\n".join(failures)
    if family == "t_max":
        assert (k1[F["kind"] == 1, 0] == 0.0).all() and (k1[F["kind"] == 0, 0] == 1.0).all()


def _frame(world, cam, name, kernel, **kw):
    img, st = world.render(cam, width=kw.pop("size", 64), height=kw.pop("size2", 64), spp=kw.pop("spp", 4), seed=1, kernel=kernel,
                           t_min=S.spec(name)["t_min"], **kw)
    assert st["kernel_used"] == kernel, (name, kernel, st["kernel_used"])
    return img


def _assert_same(img, exp, what):
    bad = ((img != exp) & ~(np.isnan(img) & np.isnan(exp))).any(axis=2)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) = %s" % (what, int(bad.sum()), np.argwhere(bad)[0].tolist())


@pytest.mark.parametrize("name", S.SCENES)
def test_frames(name, tuning):
    world, cam = S.world(name), S.camera(name)
    exp = _frame(world, cam, name, 1)
    assert (exp != 0).any(), name
    # the camera's rays reach the instances: a fair share of the oracle's primary rays end on a triangle of one
    R = S.ref(name)
    primary = R["full"].camera_rays(64, 64).reshape(-1, 6)
    full = R["full"].hit_batch(primary, t_min=S.spec(name)["t_min"], n_workers=4)
    mesh = R["meshes"].hit_batch(primary, t_min=S.spec(name)["t_min"], n_workers=4)
    assert ((full[:, 0] == 1.0) & (mesh[:, 0] == 1.0) & (full[:, 1] == mesh[:, 1])).mean() > 0.05
    for k in (2, 5, 6):
        img = _frame(world, cam, name, k)
        _assert_same(img, exp, "%s: kernel %d against kernel 1" % (name, k))
        _assert_same(_frame(world, cam, name, k), img, "%s: kernel %d, the same render again" % (name, k))
    if name in ORACLE_FRAME:
        ref, _ = R["full"].render(32, 32, 2, seed=1, t_min=S.spec(name)["t_min"])
        _assert_same(_frame(world, cam, name, 1, size=32, size2=32, spp=2), ref, "%s: kernel 1 against the oracle" % name)
    for knobs, kernels in ((dict(top_nodes=0), (5, 6)), (dict(coop_pool=1), (5,)), (dict(no_lds=1), (2,))):
        tuning(**knobs)
        for k in kernels:
            _assert_same(_frame(world, cam, name, k), exp, "%s: kernel %d with %r" % (name, k, knobs))
        tuning()


def test_a_medium_still_refuses_the_instance_walks():
    import rtamd
    world = S.world(S.SCENES[0], medium=True)
    assert world.info()["accel_compact"] == 1
    rays = S.rays(S.SCENES[0], "near")["rays"][:64]
    with pytest.raises(rtamd.RtError) as e:
        world.debug_hit(rays, t_min=S.T_MIN, kernel=5)
    assert e.value.code == -10 and "RT_ERR_UNSUPPORTED" in str(e.value)
    assert "closest-hit queries on a scene with a ConstantMedium need the path's random stream" in str(e.value)
