"""The scenes, parameter sets and explicit rays of tests/test_ao_gpu.py, and their expected values from the oracle (tests/ao_ref.py,
oracle.Scene.hit_batch).  tests/test_ao.py checks without a device that none of them is vacuous: every frame has occluded and
unoccluded rays, every finite max_distance changes its frame, every ray family holds both answers.  Everything is built once."""
import numpy as np

import ao_ref
import instance_scenes as isc
import light_scenes as ls
import nested_scenes as ns

W, H = 24, 16
SEED = 1
T_MIN = 1e-3
PARAMS = ((1, 1), (2, 3), (3, 4))      # (ao_spp, rays_per_hit)
INF = float("inf")
ARG, NOT_COMMITTED, NO_DEVICE, UNSUPPORTED = -1, -8, -9, -10      # rt_status codes the refusals answer with

# name -> (pair function of light_scenes, its arguments, the finite max_distance that flips some of the scene's occlusion rays)
FRAMES = {
    "floor": (ls.pair_floor, (ls.GRADIENT, None), 0.75),          # spheres and a rectangle
    "cornell": (ls.pair_cornell, (ls.CONSTANT,), 150.0),          # rectangles and the cube meshes under Transforms
    "room_obj_mesh": (ls.pair_room, ("obj_mesh", ls.CHECKER), 1.5),
    "nested_n4": (ls.pair_nested, ("n4", ls.NOISE), 150.0),        # chains (GENERAL == 3 in both walks) and a noise background
    "scene_10": (ls.pair_scene_10, (None,), 1.0),                  # no background: ambient is all zeros
}
_PAIRS = {}


def pair(name):
    """(rtamd.World, rtamd.Camera, oracle.Scene), built once"""
    if name not in _PAIRS:
        fn, args, _ = FRAMES[name]
        _PAIRS[name] = fn(*args)[:3]
    return _PAIRS[name]


def has_background(name):
    return name != "scene_10"


def distances(name):
    return (INF, FRAMES[name][2])


def reference(name, ao_spp, K, max_distance):
    return ao_ref.ao(pair(name)[2], W, H, ao_spp, K, max_distance, seed=SEED, t_min=T_MIN)


# ---- explicit rays for the walk alone --------------------------------------------------------------------------------------------------
WALK_SCENES = ("scale[0.001]", "scale[1]", "scale[250]", "scale[100000]", "needle", "flat", "box")
WALK_FAMILIES = ("near", "components", "graze", "t_max")
EXACT_ROWS = 300        # rays per family that are also asked at their exact hit distance and its two neighbours (ray by ray on the oracle)
_WALK = {}


def _rows(scene, rays, t_min, t_max0):
    """rays [n, 6] -> (rays7 [m, 7], expected bool [m]): every ray with the family's t_max (one oracle batch), then the first EXACT_ROWS
    rays that hit with t_max = t, nextafter(t, 0) and nextafter(t, inf) of the oracle's own closest hit, asked ray by ray"""
    rec = scene.hit_batch(rays, t_min, t_max=t_max0)
    rows = [np.concatenate([rays, np.full((len(rays), 1), t_max0)], axis=1)]
    exp = [rec[:, 0] != 0]
    hit = np.flatnonzero((rec[:, 0] != 0) & np.isfinite(rec[:, 1]) & (rec[:, 1] > t_min))[:EXACT_ROWS]
    for i in hit:
        t = rec[i, 1]
        for tm in (t, np.nextafter(t, 0.0), np.nextafter(t, INF)):
            rows.append(np.concatenate([rays[i], [tm]])[None, :])
            exp.append(scene.hit_batch(rays[i:i + 1], t_min, t_max=float(tm), n_workers=1)[:, 0] != 0)
    return np.ascontiguousarray(np.concatenate(rows, axis=0)), np.concatenate(exp)


def instance_rows(name, family):
    """-> (rays7, expected, t_min) for one family of one scene of tests/instance_scenes.py; origins within the accel's origin bound only"""
    key = (name, family)
    if key not in _WALK:
        R = isc.ref(name)
        f = isc.rays(name, family)
        rays = f["rays"]
        rays = rays[np.abs(rays[:, :3]).max(axis=1) <= 32.0 * R["extent"]]
        t_min = isc.spec(name)["t_min"]
        _WALK[key] = _rows(R["full"], rays, t_min, float(f["t_max"])) + (t_min,)
    return _WALK[key]


def tie_pair():
    if "tie" not in _PAIRS:
        import oracle
        import rtamd
        _PAIRS["tie"] = (ns.tie(rtamd.World())[0], None, ns.tie(oracle.Scene()))
    return _PAIRS["tie"]


def tie_rows():
    """-> (rays7, expected, t_min): nested_scenes.tie_rays() on the two cubes that share a face (a chain of depth 3: GENERAL == 3)"""
    if "tie" not in _WALK:
        _WALK["tie"] = _rows(tie_pair()[2], ns.tie_rays(), T_MIN, INF) + (T_MIN,)
    return _WALK["tie"]


def cube_pair():
    """a lone Cube (the reference's BVH box of a cube IS the cube: its faces lie on the box's faces) beside a sphere"""
    if "cube" not in _PAIRS:
        import oracle
        import rtamd

        def build(B):
            grey = B.Lambertian(B.ConstantTexture((0.5, 0.5, 0.5)))
            return [B.Cube((-1.13, 0.21, -0.87), (0.94, 1.92, 1.06), grey), B.Sphere((3.1, 1.2, 0.4), 0.9, grey)]
        w = rtamd.World()
        w.new(build(w), bvh_seed=1)
        o = oracle.Scene()
        o.World(build(o), 1)
        _PAIRS["cube"] = (w, None, o)
    return _PAIRS["cube"]


def cube_face_rows():
    """-> (rays7, expected, t_min): rays from outside the cube at points of its faces, each also asked with t_max = the oracle's own hit
    distance and its two neighbours.  At t_max = t the reference's box test culls the cube (aabb.rs:28-30: the box interval, clipped to the
    range, is a point), so World::hit misses where the cube's own test accepts: a walk over other boxes has to miss there too."""
    if "cube" not in _WALK:
        rng = np.random.default_rng(23)
        lo, hi = np.array((-1.13, 0.21, -0.87)), np.array((0.94, 1.92, 1.06))
        tgt = rng.uniform(lo, hi, (96, 3))
        axis, side = rng.integers(0, 3, 96), rng.integers(0, 2, 96)
        tgt[np.arange(96), axis] = np.where(side == 1, hi[axis], lo[axis])
        org = tgt + rng.uniform(-1.0, 1.0, (96, 3))
        org[np.arange(96), axis] = tgt[np.arange(96), axis] + np.where(side == 1, 1.0, -1.0) * rng.uniform(0.5, 4.0, 96)
        _WALK["cube"] = _rows(cube_pair()[2], np.concatenate([org, tgt - org], axis=1), T_MIN, INF) + (T_MIN,)
    return _WALK["cube"]


# ---- scenes the pass refuses ------------------------------------------------------------------------------------------------------------
def media_world():
    import rtamd
    w = rtamd.World()
    grey = w.Lambertian(w.ConstantTexture((0.5, 0.5, 0.5)))
    fog = w.ConstantMedium(0.2, w.Sphere((0.0, 1.0, 0.0), 1.0, grey), w.Isotropic(w.ConstantTexture((0.9, 0.9, 0.9))))
    w.new([w.Sphere((0.0, -100.0, 0.0), 100.0, grey), fog], bvh_seed=1)
    return w


def moving_world():
    import rtamd
    w = rtamd.World()
    grey = w.Lambertian(w.ConstantTexture((0.5, 0.5, 0.5)))
    w.new([w.Sphere((0.0, -100.0, 0.0), 100.0, grey), w.MovingSphere((0.0, 1.0, 0.0), (0.0, 1.5, 0.0), 0.0, 1.0, 0.5, grey)], bvh_seed=1)
    return w


def huge_world():
    """coordinates beyond 2^36 / 64: no accel (tests/test_parity_gpu.py)"""
    import rtamd
    S = 3.0e11
    w = rtamd.World()
    m = w.Lambertian(w.ConstantTexture((0.7, 0.6, 0.5)))
    w.new([w.Sphere((0.0, -1000.0 * S, 0.0), 1000.0 * S, m), w.Sphere((0.0, 1.0 * S, 0.0), 1.0 * S, m)], bvh_seed=1)
    assert w.info()["accel_ok"] == 0
    return w, rtamd.Camera(((0, 2 * S, -8 * S), (0, 1 * S, 0)), (0, 1, 0), 40, 1.5, 0.0, 8 * S)
