"""Scenes under a background, env sampling and area lights, built on both builders -- rtamd.World and the oracle's Scene -- for
tests/test_oracle_lights.py (the oracle alone, no device) and tests/test_light_frames_gpu.py (whole frames, HIP == oracle).  Every pair
function returns (rtamd.World committed, rtamd.Camera, oracle.Scene with its camera set, extra render keywords for the product)."""
import numpy as np

import area_ref
import nested_scenes as ns
from conftest import scene_path

SKY = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))
GRADIENT = dict(kind=2, gradient=SKY, scale=1.0)
NOISE = dict(kind=3, tex="noise", noise_scale=4.0, seed=3, scale=1.25)
CONSTANT = dict(kind=1, color=(0.3, 0.55, 0.9), scale=1.5)
CHECKER = dict(kind=3, tex="checker", c0=(0.1, 0.2, 0.3), c1=(0.9, 0.8, 0.7), scale=1.0)
BLACK = dict(kind=1, color=(0.0, 0.0, 0.0), scale=1.0)


def image_spec():
    rng = np.random.default_rng(5)
    return dict(kind=3, tex="image", image=rng.integers(0, 256, size=(9, 17, 3), dtype=np.uint8), scale=2.0)


def sun_spec():
    """tests/test_env_sampling_gpu.py's small sun: 64 x 32, (1, 1, 1) except a 4 x 4 block of (255, 255, 255)"""
    img = np.ones((32, 64, 3), dtype=np.uint8)
    img[6:10, 30:34] = 255
    return dict(kind=3, tex="image", image=img, scale=20.0)


# ---- one background spec on either builder --------------------------------------------------------------------------------------------
def _texture(B, spec):
    if spec["tex"] == "image":
        return B.ImageTexture(spec["image"])
    if spec["tex"] == "noise":
        return B.NoiseTexture(spec["noise_scale"], spec["seed"])
    return B.CheckerTexture(B.ConstantTexture(spec["c0"]), B.ConstantTexture(spec["c1"]))


def set_background(B, spec):
    """rt_scene_set_background / oracle.Scene.set_background from one spec dict(kind, scale, color | gradient | tex ...)"""
    scale = spec.get("scale", 1.0)
    if ns.is_oracle(B):
        if spec["kind"] == 1:
            B.set_background(1, color0=spec["color"], scale=scale)
        elif spec["kind"] == 2:
            B.set_background(2, color0=spec["gradient"][0], color1=spec["gradient"][1], scale=scale)
        else:
            B.set_background(3, texture=_texture(B, spec), scale=scale)
    elif spec["kind"] == 1:
        B.set_background(color=spec["color"], scale=scale)
    elif spec["kind"] == 2:
        B.set_background(gradient=spec["gradient"], scale=scale)
    else:
        B.set_background(texture=_texture(B, spec), scale=scale)


def deferred_world():
    """a World whose new() / set_root() leave the scene uncommitted, so that a background and env sampling can still be set"""
    import rtamd

    class Deferred(rtamd.World):
        def commit(self):
            return self
    return Deferred()


def finish_product(w, bg=None, env=None):
    import rtamd
    if bg is not None:
        set_background(w, bg)
    if env is not None:
        w.set_env_sampling(True, *env)
    rtamd.World.commit(w)
    return w


def finish_oracle(o, bg=None, env=None):
    if bg is not None:
        set_background(o, bg)
    if env is not None:
        o.set_env_sampling(*env)
    return o


def lower_area_lights(o, lights):
    """the oracle's area light list from its own object graph: tests/area_ref.lower_vertices over oracle.Scene.describe"""
    info = o.lowering_info()
    o.set_area_lights([area_ref.lower_vertices(o, obj, info) for obj in lights])


def _camera(args):
    import rtamd
    f, t, up, vfov, asp, ap, fd = args
    return rtamd.Camera((f, t), up, vfov, asp, ap, fd)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------
def pair_scene_10(bg, env=None):
    import oracle
    import rtamd
    w, cam = rtamd.load_scene_file(scene_path("scene_10.json"), commit=False)
    o = oracle.load_scene_file(scene_path("scene_10.json"), aspect=1.5)
    return finish_product(w, bg, env), cam.with_aspect(1.5), finish_oracle(o, bg, env), {}


def pair_cornell(bg, env=None, aspect=1.5):
    import oracle
    import rtamd
    w, cam = rtamd.select_scene(scene_path("cube.obj"), aspect, commit=False)
    o = oracle.cornell_box_scene(scene_path("cube.obj"), aspect, seed=1)
    return finish_product(w, bg, env), cam, finish_oracle(o, bg, env), {}


def pair_smoke(bg, env=None):
    import oracle
    from test_sppm_media_gpu import OB, _cornell_smoke
    w = deferred_world()
    items, lights = _cornell_smoke(w)
    w.new(items, lights=lights, bvh_seed=2)
    o = oracle.Scene()
    ob = OB(o)
    oitems, olights = _cornell_smoke(ob)
    o.World(oitems, 2)
    o.set_lights(olights, flux=[ob.desc[i][0] for i in olights], scale=[ob.desc[i][1] for i in olights])
    o.Camera(*ns.CORNELL_CAM)
    return finish_product(w, bg, env), _camera(ns.CORNELL_CAM), finish_oracle(o, bg, env), {}


def pair_book2(bg, env=None):
    import oracle
    from rtamd import shapes
    w = deferred_world()
    w.new(shapes.final_scene(w, n_boxes=5, n_cluster=60), bvh_seed=3)
    o = oracle.Scene()
    o.World(shapes.final_scene(o, n_boxes=5, n_cluster=60), 3)
    o.Camera(*shapes.FINAL_SCENE_CAMERA)
    o.set_shutter(*shapes.FINAL_SCENE_SHUTTER)
    return finish_product(w, bg, env), _camera(shapes.FINAL_SCENE_CAMERA), finish_oracle(o, bg, env), dict(shutter=shapes.FINAL_SCENE_SHUTTER)


def pair_nested(name, bg, env=None):
    import oracle
    w, cam = ns.SCENES[name](deferred_world())
    o = ns.SCENES[name](oracle.Scene())
    return finish_product(w, bg, env), cam, finish_oracle(o, bg, env), {}


FLOOR_ALBEDO = (0.6, 0.5, 0.4)
SHADOW_CAM = ((0.0, 6.0, 8.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0)


def floor_and_ball(B):
    """tests/test_env_sampling_gpu.py's floor with a ball on it: lit by the background alone (L = 0)"""
    return [B.XZRectangle((-1000.0, -1000.0), (1000.0, 1000.0), 0.0, B.Lambertian(B.ConstantTexture(FLOOR_ALBEDO))),
            B.Sphere((0.0, 1.0, 0.0), 1.0, B.Lambertian(B.ConstantTexture((0.7, 0.3, 0.2))))]


def pair_floor(bg, env):
    import oracle
    w = deferred_world()
    w.new(floor_and_ball(w), bvh_seed=1)
    o = oracle.Scene()
    o.World(floor_and_ball(o), 1)
    o.Camera(*SHADOW_CAM)
    return finish_product(w, bg, env), _camera(SHADOW_CAM), finish_oracle(o, bg, env), {}


AREA_VARIANTS = {
    "default": dict(),
    "nested": dict(nested=True),
    "sky_env": dict(bg=GRADIENT, env=(64, 32)),
    "sky": dict(bg=GRADIENT),
    "object_light": dict(object_light=True),
    "all": dict(nested=True, bg=GRADIENT, env=(64, 32), object_light=True),
}


def pair_area(bg=None, env=None, **kw):
    """tests/test_area_lights_gpu.py's scene (build_scene) on both sides"""
    import oracle
    import test_area_lights_gpu as ta
    w = deferred_world()
    items, olights, lights = ta.build_scene(w, **kw)
    w.new(items, lights=olights, area_lights=lights)
    o = oracle.Scene()
    oitems, oolights, alights = ta.build_scene(o, **kw)
    o.World(oitems, 1)
    if oolights:
        o.set_lights(oolights)
    lower_area_lights(o, alights)
    c = ta.CAM
    cam_args = (c["look_from"], c["look_at"], c["vup"], c["vfov"], c["aspect"], c["aperture"], c["focus"])
    o.Camera(*cam_args)
    return finish_product(w, bg, env), _camera(cam_args), finish_oracle(o, bg, env), {}


ROOM_CAM = ((0.0, 3.0, -9.0), (0.0, 1.5, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 9.0)


def _room(B):
    white = B.Lambertian(B.ConstantTexture((0.8, 0.8, 0.8)))
    red = B.Lambertian(B.ConstantTexture((0.8, 0.3, 0.3)))
    return [B.XZRectangle((-20.0, -20.0), (20.0, 20.0), 0.0, white), B.Sphere((0.0, 1.0, 0.0), 1.0, red)]


def room_cube(B):
    """a floor and a ball whose only light is an emissive Cube"""
    lt = B.Cube((-2.5, 2.0, -0.5), (-1.5, 3.0, 0.5), B.DiffuseLight(B.ConstantTexture((20.0, 20.0, 20.0))))
    return _room(B) + [lt], [lt]


def room_obj_mesh(B):
    """... an emissive OBJ mesh (cube.obj) under a rotated, non-uniformly scaled Transform"""
    em = B.DiffuseLight(B.ConstantTexture((20.0, 20.0, 20.0)))
    if ns.is_oracle(B):
        import oracle
        P, N, I = oracle.load_obj(scene_path("cube.obj"))
        mesh = B.Mesh(P, N, I, em, 1)
    else:
        mesh = B.Mesh_load_obj(scene_path("cube.obj"), em)
    lt = B.Transform((25.0, 40.0, -15.0), (0.5, 0.3, 0.7), (1.5, 3.0, 0.5), mesh)
    return _room(B) + [lt], [lt]


def room_coplanar(B):
    """... two overlapping coplanar emissive rectangles: a direction through the overlap has both terms in its pdf"""
    em = B.DiffuseLight(B.ConstantTexture((12.0, 12.0, 12.0)))
    a = B.XZRectangle((-1.5, -1.0), (0.5, 1.0), 4.0, em)
    b = B.XZRectangle((-0.5, -0.5), (1.5, 1.5), 4.0, em)
    return _room(B) + [a, b], [a, b]


def room_stacked(B):
    """... an object light above two area lights that overlap below it: a direction from the floor through all three has three non-zero
    terms in its pdf sum, so the order of the sum (object lights, then area lights) shows in the rounding"""
    em = B.DiffuseLight(B.ConstantTexture((9.0, 9.0, 9.0)))
    top = B.XZRectangle((-1.0, -1.0), (1.0, 1.0), 5.0, em)
    a = B.XZRectangle((-1.5, -1.0), (0.5, 1.0), 4.0, em)
    b = B.XZRectangle((-0.5, -0.5), (1.5, 1.5), 4.5, em)
    return _room(B) + [top, a, b], [a, b], [top]


ROOMS = {"cube": room_cube, "obj_mesh": room_obj_mesh, "coplanar": room_coplanar, "stacked": room_stacked}


def pair_room(name, bg=None, env=None):
    import oracle
    w = deferred_world()
    items, lights, *objl = ROOMS[name](w)
    w.new(items, lights=objl[0] if objl else (), area_lights=lights)
    o = oracle.Scene()
    oitems, olights, *oobjl = ROOMS[name](o)
    o.World(oitems, 1)
    if oobjl:
        o.set_lights(oobjl[0])
    lower_area_lights(o, olights)
    o.Camera(*ROOM_CAM)
    return finish_product(w, bg, env), _camera(ROOM_CAM), finish_oracle(o, bg, env), {}
