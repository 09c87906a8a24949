"""rt_ao_render without a device: tests/ao_ref.py against facts that need no renderer, the non-vacuity of what
tests/test_ao_gpu.py compares, and everything the entry points decide on the host before they ask for a device."""
import ctypes as C

import numpy as np
import pytest

import ao_cases as ac
import ao_ref
import light_scenes as ls

INF = float("inf")
ARG, NOT_COMMITTED, NO_DEVICE, UNSUPPORTED = ac.ARG, ac.NOT_COMMITTED, ac.NO_DEVICE, ac.UNSUPPORTED


# ---- ao_ref itself ------------------------------------------------------------------------------------------------------------------------
def _lone_sphere():
    import oracle
    o = oracle.Scene()
    o.World([o.Sphere((0.0, 1.0, 0.0), 1.0, o.Lambertian(o.ConstantTexture((0.7, 0.3, 0.2))))], 1)
    o.Camera(*ls.SHADOW_CAM)
    return o


@pytest.fixture(scope="module")
def floor():
    return ac.pair("floor")[2]


def test_a_convex_body_does_not_occlude_itself():
    a = ao_ref.ao(_lone_sphere(), 24, 16, 2, 3)["ao"]
    covered = a[..., 7] > 0
    assert int(covered.sum()) == 27
    assert np.all(a[covered, 0] == 1.0)
    assert np.all(a[..., 4:7] == 0.0)                      # no background: ambient is exactly 0
    assert np.all(a[~covered] == 0.0)


def test_floor_and_ball_under_the_sky(floor):
    a = ao_ref.ao(floor, 24, 16, 2, 3)["ao"]
    vis = a[..., 0]
    assert int((a[..., 7] > 0).sum()) == 384
    assert int(((vis > 0) & (vis < 1)).sum()) == 81
    assert int((vis == 1.0).sum()) == 303
    assert abs(vis.mean() - 0.9358) < 5e-5
    assert np.all(a[..., 4:7] <= np.maximum(*np.array(ls.SKY)))      # a mean of gradient colours, times an open fraction <= 1
    assert np.all(np.sqrt((a[..., 1:4] ** 2).sum(axis=2)) <= vis + 1e-12)     # |sum of unit vectors| <= their number


def test_the_distance_cap_changes_the_frame(floor):
    far = ao_ref.ao(floor, 24, 16, 2, 3)["ao"]
    near = ao_ref.ao(floor, 24, 16, 2, 3, max_distance=0.75)["ao"]
    vis = near[..., 0]
    assert int(((vis > 0) & (vis < 1)).sum()) == 18
    assert abs(vis.mean() - 0.9857) < 5e-5
    assert np.all(vis >= far[..., 0])                      # a nearer cap only opens rays
    assert np.array_equal(near[..., 7], far[..., 7])


# ---- what test_ao_gpu.py compares is not vacuous ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.FRAMES))
def test_every_frame_has_both_kinds_of_rays_and_a_distance_that_matters(name):
    for ao_spp, K in ac.PARAMS:
        far, near = (ac.reference(name, ao_spp, K, d) for d in ac.distances(name))
        for r in (far, near):
            assert r["occluded"] > 0 and r["unoccluded"] > 0, (name, ao_spp, K)
        assert (far["ao"] != near["ao"]).any(), (name, ao_spp, K)
    amb = ac.reference(name, 2, 3, INF)["ao"][..., 4:7]
    assert (amb.max() > 0) == ac.has_background(name)


@pytest.mark.parametrize("name", ac.WALK_SCENES)
def test_every_ray_family_holds_both_answers(name):
    for family in ac.WALK_FAMILIES:
        rays7, exp, _ = ac.instance_rows(name, family)
        assert exp.any() and not exp.all(), (name, family)
        assert len(rays7) == len(exp) and len(rays7) > 3 * 30          # (among them rows at t, nextafter(t, 0) and nextafter(t, inf))


def test_the_tie_rays_hold_both_answers():
    rays7, exp, _ = ac.tie_rows()
    assert exp.any() and not exp.all()


# ---- host-side behaviour ---------------------------------------------------------------------------------------------------------------------
def test_default_config_and_struct_size():
    import rtamd
    c = rtamd.rt_ao_config()
    c.reserved[2] = 7
    rtamd.lib().rt_default_ao_config(C.byref(c))
    assert (c.ao_spp, c.rays_per_hit, c.max_distance, list(c.reserved)) == (4, 4, INF, [0, 0, 0, 0])
    assert C.sizeof(rtamd.rt_ao_config) == 4 + 4 + 8 + 4 * 4
    rtamd.lib().rt_default_ao_config(None)                 # a null pointer is ignored


def _call(w, cam, out=True, cfg=True, stats=True, device_entry=False, scene=True, camera=True, params=True, **kw):
    import rtamd
    L = rtamd.lib()
    c = rtamd.rt_ao_config()
    L.rt_default_ao_config(C.byref(c))
    pk = dict(width=8, height=8)
    for k, v in kw.items():
        if k in ("ao_spp", "rays_per_hit", "max_distance"):
            setattr(c, k, v)
        elif k == "reserved":
            c.reserved[v] = 1
        else:
            pk[k] = v
    p = rtamd.default_params(**pk)
    buf = np.zeros((8, 8, 8))
    st = rtamd.rt_stats()
    args = [w.h if scene else None, C.byref(cam.c) if camera else None, C.byref(p) if params else None, C.byref(c) if cfg else None]
    if device_entry:
        return L.rt_ao_render_device(*args, C.c_void_p(buf.ctypes.data if out else 0), None, C.byref(st) if stats else None)
    return L.rt_ao_render(*args, buf.ctypes.data_as(C.POINTER(C.c_double)) if out else None, C.byref(st) if stats else None)


@pytest.mark.parametrize("device_entry", [False, True])
def test_bad_arguments_are_refused_before_the_device(device_entry):
    import rtamd
    w, cam, _ = ac.pair("floor")
    bad = [dict(ao_spp=0), dict(ao_spp=-1), dict(ao_spp=4097), dict(rays_per_hit=0), dict(rays_per_hit=257), dict(max_distance=0.0),
           dict(max_distance=-1.0), dict(max_distance=float("nan")), dict(max_distance=-INF), dict(kernel=-1), dict(kernel=3), dict(kernel=5),
           dict(world=2), dict(rank=1), dict(world=2, rank=1), dict(width=0), dict(height=0), dict(out=False), dict(cfg=False), dict(scene=False),
           dict(camera=False), dict(params=False)] + [dict(reserved=i) for i in range(4)]
    for kw in bad:
        assert _call(w, cam, device_entry=device_entry, **kw) == ARG, kw
    if rtamd.device_count() == 0 and not device_entry:
        for kw in (dict(), dict(stats=False), dict(ao_spp=4096, rays_per_hit=256), dict(max_distance=1e-300), dict(kernel=1), dict(kernel=2)):
            assert _call(w, cam, **kw) == NO_DEVICE, kw
    if rtamd.device_count() == 0 and device_entry:
        assert _call(w, cam, device_entry=True) == NO_DEVICE


def test_unsupported_scenes_and_walks_are_refused_before_the_device():
    import rtamd
    _, cam, _ = ac.pair("floor")
    for w in (ac.media_world(), ac.moving_world()):
        for k in (0, 1, 2):
            assert _call(w, cam, kernel=k) == UNSUPPORTED
            assert _call(w, cam, kernel=k, device_entry=True) == UNSUPPORTED
        assert _call(w, cam, kernel=3) == ARG              # arguments first
    hw, hcam = ac.huge_world()
    assert _call(hw, hcam, kernel=2) == UNSUPPORTED
    w, cam, _ = ac.pair("floor")
    assert _call(w, cam, kernel=2, t_min=-1.0) == UNSUPPORTED                         # box32 needs t_min >= 0
    far = rtamd.Camera(((0.0, 1e9, 0.0), (0.0, 0.0, 0.0)), (0, 0, 1), 40, 1.0, 0.0, 10.0)
    assert _call(w, far, kernel=2) == UNSUPPORTED          # the camera lies beyond the origin bound of the f32 boxes
    uncommitted = ls.deferred_world()
    uncommitted.new([uncommitted.Sphere((0.0, 0.0, 0.0), 1.0, uncommitted.Lambertian(uncommitted.ConstantTexture((0.5, 0.5, 0.5))))])
    assert _call(uncommitted, cam) == NOT_COMMITTED
    if rtamd.device_count() == 0:
        assert _call(hw, hcam, kernel=0) == NO_DEVICE      # the automatic choice falls back to the reference-order walk
        assert _call(w, far, kernel=0) == NO_DEVICE
        with pytest.raises(rtamd.RtError) as e:
            w.render_ao(cam, 8, 8)
        assert e.value.code == NO_DEVICE


def test_debug_occluded_checks_its_arguments_before_the_device():
    import rtamd
    L = rtamd.lib()
    w, _, _ = ac.pair("floor")
    rays = np.array([[0.0, 5.0, 0.0, 0.0, -1.0, 0.0, INF]])
    out = np.zeros(1)
    dp = C.POINTER(C.c_double)

    def call(world=w, kernel=1, n=1, r=rays, o=out, t_min=1e-3):
        return L.rt_debug_occluded_device(world.h if world is not None else None, 0, kernel, n, r.ctypes.data_as(dp) if r is not None else None, t_min,
                                          o.ctypes.data_as(dp) if o is not None else None)
    for kw in (dict(world=None), dict(kernel=0), dict(kernel=3), dict(kernel=5), dict(n=0), dict(r=None), dict(o=None)):
        assert call(**kw) == ARG, kw
    uncommitted = ls.deferred_world()
    uncommitted.new([uncommitted.Sphere((0.0, 0.0, 0.0), 1.0, uncommitted.Lambertian(uncommitted.ConstantTexture((0.5, 0.5, 0.5))))])
    assert call(world=uncommitted) == NOT_COMMITTED
    for bad in (ac.media_world(), ac.moving_world()):
        assert call(world=bad) == UNSUPPORTED and call(world=bad, kernel=2) == UNSUPPORTED
    assert call(world=ac.huge_world()[0], kernel=2) == UNSUPPORTED
    assert call(kernel=2, t_min=-1.0) == UNSUPPORTED
    if rtamd.device_count() == 0:
        assert call() == NO_DEVICE and call(kernel=2) == NO_DEVICE
        with pytest.raises(rtamd.RtError) as e:
            w.debug_occluded(rays)
        assert e.value.code == NO_DEVICE


def test_cube_face_rows_hold_both_answers_at_the_exact_distance():
    """asked with t_max = its own hit distance, a cube face that lies on the reference's box is culled for some rays and kept for others
    (the box's slab arithmetic rounds apart from the face's own t); one double below it always misses, one above always hits"""
    rays7, exp, _ = ac.cube_face_rows()
    n = len(rays7) // 4
    assert exp[:n].all()
    at, below, above = exp[n:].reshape(-1, 3).sum(axis=0)
    assert 0 < at < n and below == 0 and above == n
