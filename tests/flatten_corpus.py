"""Scenes that between them run every stage of rt_scene_commit's flattener (csrc/host/flatten.cpp, accel.cpp): CORPUS maps a name to a
builder that returns a committed rtamd.World, REFUSALS to a builder of a scene with two defects at once (which one commit reports is
part of the contract), and recommit() is a scene whose first commit fails and whose second succeeds.  tests/test_flatten_pins.py replays
tests/golden/flatten_pins.json over them: per scene the fingerprint of the blob, rt_scene_info and -- with area lights --
rt_scene_area_light_tris, byte for byte; per refusal the status code and the message.

Record the file with the library of the commit whose behaviour is to be pinned:
    python tests/flatten_corpus.py --record --commit COMMIT
(RTAMD_LIB / RTAMD_HIP_RUNTIME=system select a host-only build, tests/asan/run_host_asan.sh has the recipe).  The builders are the
tests' own wherever one exists."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PINS = os.path.join(HERE, "golden", "flatten_pins.json")
for _p in (HERE, os.path.join(ROOT, "rust-raytracer_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import nested_scenes as ns  # noqa: E402
import test_area_lights as area  # noqa: E402
import test_cube_gpu as cube  # noqa: E402
import test_sppm_media_gpu as media  # noqa: E402

SCENES = os.path.join(HERE, "golden", "scenes")
NONE, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _world():
    import rtamd
    return rtamd.World()


def _scene_file(name, commit=True):
    import rtamd
    return rtamd.load_scene_file(os.path.join(SCENES, name), commit=commit)[0]


def _cornell(commit=True):
    import rtamd
    return rtamd.select_scene(os.path.join(SCENES, "cube.obj"), 1.0, 1, commit=commit)[0]


def _uncommitted(w, items, lights=(), seed=1):
    """World.new without its commit"""
    from rtamd import _chk
    _chk(w.L.rt_world_new(w.h, len(items), (C.c_int * len(items))(*items), seed))
    if lights:
        w.set_lights(list(lights))
    return w


def _items_and_lights(build, seed):
    w = _world()
    items, lights = build(w)
    return w.new(items, lights=lights, bvh_seed=seed)


def _single(kind):
    """a world that is ONE object: BVHNode::new puts it into both children, so it is emitted twice (a medium: two MediumDev records)"""
    w = _world()
    white = w.Lambertian(w.ConstantTexture((0.8, 0.8, 0.8)))
    obj = w.Sphere((0.0, 1.0, 0.0), 1.0, white)
    if kind == "medium":
        obj = w.ConstantMedium(0.5, obj, w.Isotropic(w.ConstantTexture((0.9, 0.9, 0.9))))
    return w.new([obj])


def _lights(kind):
    w = _world()
    white = w.Lambertian(w.ConstantTexture((0.8, 0.8, 0.8)))
    items = [w.XZRectangle((-6.0, -6.0), (6.0, 6.0), 0.0, white), w.Sphere((0.0, 1.0, 0.0), 1.0, white)]
    if kind == "sphere":          # rt_object_sphere_light, in the scene
        lt = w.SphereDiffuseLight((0.0, 5.0, 0.0), 0.3, (1.0, 0.9, 0.8), 500.0)
        items.append(lt)
    elif kind == "sphere_outside":  # named by the light list only
        lt = w.SphereDiffuseLight((0.0, 5.0, 0.0), 0.3, (1.0, 0.9, 0.8), 500.0)
    else:
        lt = w.XZRectLight((-1.0, -1.0), (1.0, 1.0), 5.0, (1.0, 1.0, 1.0), 100.0)
    return w.new(items, lights=[lt])


def _tenths_mesh(w, mat):
    """a tetrahedron with the vertex coordinate 0.1, which is no f32: its instance is entered inline"""
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.1, 0.25, 1.0]])
    return w.Mesh(pos, None, area.TETRA_IDX, mat, synthesize_normals=True, bvh_seed=2)


def _instances(reverse, as_list=False):
    """one deferrable instance (cube.obj: f32 vertices) and two inline ones (a mesh that is not f32, a sphere), in both orders; as_list:
    under a plain list as the root, which keeps the insertion order (BVHNode::new sorts its objects)"""
    w = _world()
    white = w.Lambertian(w.ConstantTexture((0.8, 0.8, 0.8)))
    inst = [w.Transform((0.0, 30.0, 0.0), ONE, (-3.0, 1.0, 0.0), w.Mesh_load_obj(os.path.join(SCENES, "cube.obj"), white)),
            w.Transform((10.0, 0.0, 20.0), (1.0, 2.0, 1.0), (0.0, 0.5, 0.0), _tenths_mesh(w, white)),
            w.Transform(NONE, (1.0, 0.5, 1.0), (3.0, 1.0, 0.0), w.Sphere((0.0, 0.0, 0.0), 1.0, white))]
    items = [w.XZRectangle((-9.0, -9.0), (9.0, 9.0), 0.0, white)] + (inst[::-1] if reverse else inst)
    if as_list:
        w.set_root(w.HitableList(items))
    else:
        w.new(items)
    info = w.info()
    assert info["accel_compact"] == 1 and info["accel_instances"] == 3, info
    return w


def _thin(kind):
    """an instance without extent along one axis: a single triangle, a planar mesh with z constant (f32 vertices)"""
    from rtamd import shapes
    w = _world()
    white = w.Lambertian(w.ConstantTexture((0.8, 0.8, 0.8)))
    if kind == "triangle":
        m = w.Mesh(np.array([[0.0, 0.0, 0.5], [1.0, 0.0, 0.5], [0.0, 1.0, 0.25]]), None, [(0, 1, 2)], white, synthesize_normals=True)
    else:
        P, N, I = shapes.sheet(4, (2.0, 1.0))
        m = w.Mesh(P[:, [0, 2, 1]] + np.array([0.0, 0.0, 0.75]), N[:, [0, 2, 1]], I, white, bvh_seed=2)
    w.new([w.XZRectangle((-9.0, -9.0), (9.0, 9.0), 0.0, white), w.Transform((0.0, 25.0, 0.0), ONE, (1.0, 2.0, 3.0), m)])
    assert w.info()["accel_compact"] == 1
    return w


def _edge(kind):
    """scenes on which the accel gives up or takes a rare path; the root is a plain list (BVHNode::new refuses an object without a box)"""
    w = _world()
    white = w.Lambertian(w.ConstantTexture((0.8, 0.8, 0.8)))
    ball = w.Sphere((0.0, 1.0, 0.0), 1.0, white)
    if kind == "boxless_transform":       # an empty list has no box, nor has a Transform over it
        items = [ball, w.Transform(NONE, ONE, (1.0, 0.0, 0.0), w.HitableList([]))]
    elif kind == "boxless_medium":
        items = [ball, w.ConstantMedium(0.5, w.HitableList([]), w.Isotropic(w.ConstantTexture((0.9, 0.9, 0.9))))]
    elif kind == "zero_extent":           # the world's largest |coordinate| is 0
        items = [w.Sphere(NONE, 0.0, white)]
    elif kind == "far_sphere":            # ray origins beyond 2^36
        items = [ball, w.Sphere((2.0e9, 0.0, 0.0), 1.0, white)]
    elif kind == "tiny_scale_instance":   # object-space ray origins beyond 2^36
        items = [ball, w.Transform(NONE, (1.0e-9, 1.0e-9, 1.0e-9), (3.0, 1.0, 0.0), w.Sphere(NONE, 1.0e9, white))]
    else:                                 # identical centroids: the BVH splits by index
        items = [w.Sphere((0.0, 1.0, 0.0), 0.25 * (k + 1), white) for k in range(6)]
    return w.set_root(w.HitableList(items))


def _background(kind):
    w = _scene_file("scene_10.json", commit=False)
    if kind == "color":
        w.set_background(color=(0.25, 0.5, 1.0), scale=2.0)
    elif kind == "gradient":
        w.set_sky()
    elif kind == "image":
        yy, xx = np.mgrid[0:8, 0:16]
        w.set_background(texture=w.ImageTexture(np.stack([xx * 16, yy * 32, xx + yy], axis=-1).astype(np.uint8)), scale=0.5)
    else:
        w.set_background(texture=w.CheckerTexture(w.ConstantTexture((0.1, 0.2, 0.3)), w.ConstantTexture((0.9, 0.8, 0.7))))
    return w.commit()


def _env(kind):
    w = _cornell(commit=False)
    if kind == "wide_image":     # wider than 4096: the automatic size is halved
        w.set_background(texture=w.ImageTexture(np.full((3, 4100, 3), 7, dtype=np.uint8)))
    elif kind == "tall_image":   # ... and so it is for one taller than 2048
        w.set_background(texture=w.ImageTexture(np.full((2100, 3, 3), 7, dtype=np.uint8)))
    elif kind == "checker":      # a texture that is no image: 256 x 128
        w.set_background(texture=w.CheckerTexture(w.ConstantTexture((0.1, 0.2, 0.3)), w.ConstantTexture((0.9, 0.8, 0.7))))
    else:
        w.set_sky()
    if kind == "explicit":
        w.set_env_sampling(True, 64, 32)
    else:
        w.set_env_sampling(True)
    return w.commit()


CORPUS = {}
for _k in sorted(ns.SCENES):
    CORPUS["nested_" + _k] = lambda k=_k: ns.SCENES[k](_world())[0]
CORPUS["nested_tie"] = lambda: ns.tie(_world())[0]
CORPUS["scene_10.yaml"] = lambda: _scene_file("scene_10.yaml")
CORPUS["media_cornell_smoke"] = lambda: _items_and_lights(media._cornell_smoke, 2)
CORPUS["media_cornell_smoke_book"] = lambda: _items_and_lights(media._cornell_smoke_book, 3)
CORPUS["media_sphere_fog"] = lambda: _items_and_lights(media._fogged_caustics(True), 1)
CORPUS["media_nested_fog"] = lambda: _items_and_lights(media._nested_fog, 4)
CORPUS["single_sphere"] = lambda: _single("sphere")
CORPUS["single_medium"] = lambda: _single("medium")
for _v in (0, 1):
    CORPUS["cube_instances_%d" % _v] = lambda v=_v: (lambda w: w.new(cube._build_with_instances(w, v), bvh_seed=3))(_world())
for _k in ("sphere", "sphere_outside", "rect_outside"):
    CORPUS["light_" + _k] = lambda k=_k: _lights(k)
CORPUS["instances_mixed"] = lambda: _instances(False)
CORPUS["instances_mixed_reversed"] = lambda: _instances(True)
CORPUS["instances_mixed_list"] = lambda: _instances(False, as_list=True)
CORPUS["instances_mixed_list_reversed"] = lambda: _instances(True, as_list=True)
CORPUS["thin_triangle"] = lambda: _thin("triangle")
CORPUS["thin_planar_mesh"] = lambda: _thin("planar")
for _k in area.CASES:
    CORPUS["area_" + _k] = lambda k=_k: area.build(k).commit()
    CORPUS["area_" + _k + "_off"] = lambda k=_k: area.build(k).commit(area=False)
for _k in ("color", "gradient", "image", "checker"):
    CORPUS["background_" + _k] = lambda k=_k: _background(k)
for _k in ("auto", "explicit", "wide_image", "tall_image", "checker"):
    CORPUS["env_" + _k] = lambda k=_k: _env(k)
for _k in ("boxless_transform", "boxless_medium", "zero_extent", "far_sphere", "tiny_scale_instance", "concentric_spheres"):
    CORPUS["edge_" + _k] = lambda k=_k: _edge(k)


# ---- scenes with two defects: which one does commit report? (builders return the World uncommitted) ---------------------------------
def _light_under_transform(w, items):
    lt = ns.light(w)
    items.append(w.Transform(NONE, ONE, (0.0, -1.0, 0.0), lt))
    return lt


def _refuse_light_and_env():
    w = _world()
    _, items = ns.walls(w)
    lt = _light_under_transform(w, items)
    return _uncommitted(w, items, [lt]).set_env_sampling(True)


def _refuse_area_and_env():
    s = area.Scene()
    md = s.w.MeshData(np.array([[0.0, 1.0, 0.0], [1.0, 1.0, 0.0], [2.0, 1.0, 0.0]]), np.tile([0.0, 1.0, 0.0], (3, 1)))
    s.light(s.w.HitableList([s.w.Triangle(md, 0, 1, 2, s.em), s.w.Triangle(md, 2, 1, 0, s.em)]))
    _uncommitted(s.w, s.items)
    return s.w.set_area_lights(s.lights).set_env_sampling(True)


def _refuse_depth_and_light():
    w = _world()
    white, items = ns.walls(w)
    lt = _light_under_transform(w, items)
    items.append(ns.nest(w, ns.chain(ns.MAX_DEPTH + 1), w.Cube((-60.0, -60.0, -60.0), (60.0, 60.0, 60.0), white)))
    return _uncommitted(w, items, [lt])


REFUSALS = {
    "light_under_transform+env_without_background": _refuse_light_and_env,
    "area_light_without_area+env_without_background": _refuse_area_and_env,
    "nine_levels+light_under_transform": _refuse_depth_and_light,
}


def refusal(name):
    """-> [status code, message] of committing REFUSALS[name]"""
    w = REFUSALS[name]()
    code = int(w.L.rt_scene_commit(w.h))
    return [code, w.L.rt_last_error().decode("utf-8", "replace")]


def unloadable(name="test.json"):
    """test.json is of an older schema (a Sphere without material): the loader refuses it before anything is flattened ->
    [status code, message]"""
    import rtamd
    h, cam = C.c_void_p(), rtamd.rt_camera()
    code = int(rtamd.lib().rt_scene_load_file(os.fsencode(os.path.join(SCENES, name)), C.byref(h), C.byref(cam)))
    return [code, rtamd.lib().rt_last_error().decode("utf-8", "replace")]


def recommit():
    """env sampling without a background: the first commit fails; with a sky the second gives the scene built cleanly ->
    [first status code, first message, fingerprint and info after the second commit, the same of a clean build]"""
    w = _cornell(commit=False).set_env_sampling(True, 64, 32)
    code = int(w.L.rt_scene_commit(w.h))
    msg = w.L.rt_last_error().decode("utf-8", "replace")
    w.set_sky().commit()
    clean = _cornell(commit=False).set_sky().set_env_sampling(True, 64, 32).commit()
    return {"first": [code, msg], "second": observe(w), "clean": observe(clean)}


def observe(w):
    """what a caller can see of a committed scene's flattening"""
    out = {"fingerprint": "%016x" % w.fingerprint(), "info": w.info()}
    tris = w.area_light_tris()
    if len(tris):
        out["area_tris"] = [t.tobytes().hex() for t in tris]
    return out


def record(commit):
    return {"recorded_on": commit, "what": "see tests/flatten_corpus.py", "scenes": {k: observe(CORPUS[k]()) for k in CORPUS},
            "refusals": {k: refusal(k) for k in REFUSALS}, "unloadable": {"test.json": unloadable()}, "recommit": recommit()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write tests/golden/flatten_pins.json from the loaded library")
    ap.add_argument("--commit", default="", help="the commit the loaded library was built from (recorded in the file)")
    ap.add_argument("--out", default=PINS)
    a = ap.parse_args()
    if not a.record:
        ap.error("nothing to do without --record")
    pins = record(a.commit)
    with open(a.out, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d scenes, %d refusals, %d bytes -> %s" % (len(pins["scenes"]), len(pins["refusals"]), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()
