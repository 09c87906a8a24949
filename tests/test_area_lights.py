"""Area lights -- emissive rectangles, cubes and meshes as lights of integrator 1 (rt_scene_set_area_lights) -- without a
device: the table rt_scene_commit lowers them to equals the numpy restatement (tests/area_ref.py) bit for bit, every refusal of the
header is an error of the right kind, and the fingerprint tells a scene with area lights from the same scene without them."""
import ctypes as C
import re

import numpy as np
import pytest

import area_ref
from conftest import ROOT, scene_path
from test_abi_symbols import HEADER, declared_symbols

RT_ERR_ARG = -1
RT_ERR_NOT_COMMITTED = -8
RT_ERR_NO_DEVICE = -9
RT_ERR_UNSUPPORTED = -10

# rt_scene_fingerprint of scene_10.json and of the Cornell box (bvh_seed 1), recorded on the commit before area lights existed
FP_SCENE_10 = 4515439981022265460
FP_CORNELL = 18314941300861624911

TETRA_POS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
TETRA_IDX = [(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)]


def trs(rot_deg, scale, translate):
    """M = T * S * Rx * Ry * Rz as a host would compose it (handed over with Transform_from_matrix, so the stored `trans` is this matrix)"""
    rx, ry, rz = np.radians(rot_deg)
    T = np.eye(4)
    T[:3, 3] = translate
    S = np.diag([scale[0], scale[1], scale[2], 1.0])
    RX = np.array([[1, 0, 0, 0], [0, np.cos(rx), -np.sin(rx), 0], [0, np.sin(rx), np.cos(rx), 0], [0, 0, 0, 1.0]])
    RY = np.array([[np.cos(ry), 0, np.sin(ry), 0], [0, 1, 0, 0], [-np.sin(ry), 0, np.cos(ry), 0], [0, 0, 0, 1.0]])
    RZ = np.array([[np.cos(rz), -np.sin(rz), 0, 0], [np.sin(rz), np.cos(rz), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    return T @ S @ RX @ RY @ RZ


class Scene:
    """A floor plus whatever the test adds; `lights` = the area light list, `info` = what area_ref.lower cannot read back."""

    def __init__(self):
        import rtamd
        self.w = rtamd.World()
        w = self.w
        self.em = w.DiffuseLight(w.ConstantTexture((4.0, 4.0, 4.0)))
        self.white = w.Lambertian(w.ConstantTexture((0.7, 0.7, 0.7)))
        self.items = [w.XZRectangle((-9.0, -9.0), (9.0, 9.0), 0.0, self.white)]
        self.lights = []
        self.info = {"trans": {}, "mesh": {}, "pos": TETRA_POS}

    def tetra(self, mat=None):
        w = self.w
        md = w.MeshData(TETRA_POS, np.tile([0.0, 1.0, 0.0], (4, 1)))
        return w.BVHNode_new([w.Triangle(md, a, b, c, self.em if mat is None else mat) for a, b, c in TETRA_IDX], bvh_seed=5)

    def transform(self, m, obj):
        t = self.w.Transform_from_matrix(m, obj)
        self.info["trans"][t] = m
        return t

    def light(self, obj, in_scene=True):
        if in_scene:
            self.items.append(obj)
        self.lights.append(obj)
        return obj

    def commit(self, area=True):
        self.w.new(self.items, area_lights=self.lights if area else ())
        return self.w


def obj_triangles(path):
    """positions (f32 values, as the OBJ loader keeps them) and the triangles' position indices, in file order"""
    pos, idx = [], []
    for line in open(path):
        f = line.split()
        if f and f[0] == "v":
            pos.append([float(np.float32(x)) for x in f[1:4]])
        elif f and f[0] == "f":
            v = [int(x.split("/")[0]) - 1 for x in f[1:]]
            idx += [(v[0], v[i], v[i + 1]) for i in range(1, len(v) - 1)]
    return np.array(pos, dtype=np.float64), idx


def build(case):
    s = Scene()
    w = s.w
    if case == "rect_xy_yz":
        s.light(w.XYRectangle((-1.0, 0.5), (2.0, 1.75), -3.0, s.em))
        s.light(w.YZRectangle((0.25, -1.0), (1.25, 0.5), 4.0, s.em))
    elif case == "cube":
        s.light(w.Cube((-1.0, 0.5, 2.0), (0.5, 1.0, 5.0), s.em))
    elif case == "obj_mesh":
        m = w.Mesh_load_obj(scene_path("cube.obj"), s.em)
        s.info["mesh"][m] = obj_triangles(scene_path("cube.obj"))
        s.items.append(w.Transform((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 3.0, 0.0), m))
        s.light(m, in_scene=False)  # the mesh itself is the light, where it was modelled (the scene shows it under a Transform)
    elif case == "tetra_bvh":
        s.light(s.tetra())
    elif case == "tetra_nested":
        inner = s.transform(trs((20.0, -35.0, 50.0), (1.5, 0.5, 2.0), (0.25, 1.0, -0.5)), s.tetra())
        s.light(s.transform(trs((-10.0, 15.0, 5.0), (0.75, 1.25, 1.0), (2.0, 3.0, 1.0)), inner))
    elif case == "list_with_degenerate":
        md = w.MeshData(np.array([[0.0, 1.0, 0.0], [1.0, 1.0, 0.0], [2.0, 1.0, 0.0], [0.0, 2.0, 1.0]]), np.tile([0.0, 1.0, 0.0], (4, 1)))
        s.info["pos"] = np.array([[0.0, 1.0, 0.0], [1.0, 1.0, 0.0], [2.0, 1.0, 0.0], [0.0, 2.0, 1.0]])
        tris = [w.Triangle(md, 0, 1, 3, s.em), w.Triangle(md, 0, 1, 2, s.em), w.Triangle(md, 1, 2, 3, s.em)]  # the middle one is a line
        s.light(w.HitableList(tris))
    elif case == "mixed":
        s.light(w.XZRectangle((-0.5, -0.5), (0.5, 0.5), 6.0, s.em))
        s.light(w.HitableList([w.Cube((3.0, 0.5, 0.0), (3.5, 1.0, 0.25), s.em), s.transform(trs((0, 30.0, 0), (1, 2, 1), (-3, 1, 0)), s.tetra())]))
    return s


CASES = ("rect_xy_yz", "cube", "obj_mesh", "tetra_bvh", "tetra_nested", "list_with_degenerate", "mixed")
N_TRIS = dict(rect_xy_yz=4, cube=12, obj_mesh=12, tetra_bvh=4, tetra_nested=4, list_with_degenerate=2, mixed=2 + 12 + 4)


def test_header_declares_and_library_exports_the_area_light_entry_points():
    import rtamd
    for sym in ("rt_scene_set_area_lights", "rt_scene_area_light_tris", "rt_debug_area_sample_device", "rt_debug_area_pdf_device"):
        assert sym in declared_symbols()
        assert sym in rtamd.ABI_SYMBOLS
        assert hasattr(C.CDLL(rtamd.LIB_PATH), sym)
    header = open(HEADER).read()
    assert re.search(r"typedef struct rt_area_tri \{\s*double a\[3\], e0\[3\], e1\[3\], n\[3\];\s*double area2;\s*uint32_t q;\s*int32_t light;.*?\} rt_area_tri;",
                     header, flags=re.S)
    assert C.sizeof(rtamd.rt_area_tri) == 112 and rtamd.AREA_TRI_DTYPE.itemsize == 112
    assert rtamd.rt_area_tri.q.offset == 104 and rtamd.rt_area_tri.light.offset == 108 and rtamd.rt_area_tri.area2.offset == 96
    assert rtamd.lib().rt_abi_version() == 2
    rs = open(ROOT + "/rust-raytracer_amd/rust/rtamd_ffi.rs").read()
    assert re.search(r"pub struct rt_area_tri \{\s*pub a: \[c_double; 3\],\s*pub e0: \[c_double; 3\],\s*pub e1: \[c_double; 3\],\s*pub n: \[c_double; 3\],"
                     r"\s*pub area2: c_double,\s*pub q: u32,\s*pub light: i32,\s*\}", rs)
    assert "pub fn set_area_lights" in rs
    hpp = open(ROOT + "/rust-raytracer_amd/host_cpp/rtamd.hpp").read()
    assert "rt_scene_set_area_lights" in hpp and "rt_scene_area_light_tris" in hpp


@pytest.mark.parametrize("case", CASES)
def test_lowered_table_equals_the_restatement_bit_for_bit(case):
    s = build(case)
    w = s.commit()
    got = w.area_light_tris()
    exp, totals = area_ref.lower(w, s.lights, s.info)
    assert len(got) == N_TRIS[case] == len(exp["q"])
    for k in area_ref.AREA_TRI_FIELDS:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.dtype == e.dtype and g.shape == e.shape, k
        assert g.tobytes() == e.tobytes(), k  # bit for bit (-0.0 and 0.0 differ)
    # q and the prefix sums: the largest triangle of a light has q = 2^32 - 1, none has 0, the totals are exact integers
    for li, total in enumerate(totals):
        q = got["q"][got["light"] == li].astype(np.uint64)
        a2 = got["area2"][got["light"] == li]
        assert q.max() == 4294967295 and q.min() >= 1 and int(q.sum()) == total
        assert np.array_equal(q, np.maximum(1.0, np.floor(a2 / a2.max() * 4294967295.0)).astype(np.uint64))
        assert int(np.cumsum(q, dtype=np.uint64)[-1]) == total
    assert np.all(got["area2"] > 0) and np.all(np.isfinite(got["area2"]))
    # lights appear in list order
    assert np.all(np.diff(got["light"]) >= 0) and got["light"][0] == 0 and got["light"][-1] == len(s.lights) - 1


def test_mesh_is_lowered_in_index_order_not_in_bvh_order():
    s = Scene()
    pos, idx = obj_triangles(scene_path("cube.obj"))
    m = s.light(s.w.Mesh(pos, None, idx, s.em, synthesize_normals=True, bvh_seed=3))
    s.info["mesh"][m] = (pos, idx)
    w = s.commit()
    got = w.area_light_tris()
    assert np.array_equal(got["a"], np.array([pos[i[0]] for i in idx]))
    kind, d = w.describe(s.lights[0])
    assert kind == "Mesh"
    bvh_order = area_ref.lower_vertices(w, d["children"][0], dict(s.info, pos=pos))  # what a walk of the inner BVH would give
    assert len(bvh_order) >= 12 and not np.array_equal(np.array([t[0] for t in bvh_order[:12]]), got["a"])


def test_capacity_and_uncommitted():
    import rtamd
    s = build("cube")
    buf = (rtamd.rt_area_tri * 12)()
    assert s.w.L.rt_scene_area_light_tris(s.w.h, 12, buf) == RT_ERR_NOT_COMMITTED
    w = s.commit()
    assert w.L.rt_scene_area_light_tris(w.h, 0, None) == 12
    assert w.L.rt_scene_area_light_tris(w.h, 5, buf) == 12  # writes min(capacity, N), returns N
    assert buf[4].q != 0 and buf[5].q == 0
    assert w.L.rt_scene_area_light_tris(None, 0, None) == RT_ERR_ARG
    assert w.L.rt_scene_area_light_tris(w.h, 3, None) == RT_ERR_ARG
    plain = build("cube").commit(area=False)
    assert len(plain.area_light_tris()) == 0


def _refused(s, objs, code=RT_ERR_ARG):
    arr = (C.c_int * len(objs))(*objs)
    assert s.w.L.rt_scene_set_area_lights(s.w.h, len(objs), arr) == code
    assert s.w.L.rt_last_error()


def test_set_area_lights_refusals():
    s = Scene()
    w = s.w
    ok = w.YZRectangle((0.0, 0.0), (1.0, 1.0), 2.0, s.em)
    s.light(ok)
    w.set_area_lights(s.lights)
    _refused(s, [ok, 12345])                                                 # an unknown id
    _refused(s, [-1])
    _refused(s, [w.Sphere((0.0, 1.0, 0.0), 0.5, s.em)])                       # a sphere
    _refused(s, [w.HitableList([ok, w.Sphere((0.0, 1.0, 0.0), 0.5, s.em)])])  # ... anywhere in the subtree
    _refused(s, [w.MovingSphere((0, 1, 0), (0, 2, 0), 0.0, 1.0, 0.5, s.em)])
    _refused(s, [w.ConstantMedium(0.5, w.Cube((0, 0, 0), (1, 1, 1), s.em), w.Isotropic(w.ConstantTexture((1, 1, 1))))])
    _refused(s, [w.XYRectangle((0.0, 0.0), (1.0, 1.0), 2.0, s.white)])        # a leaf that does not emit
    _refused(s, [w.Cube((0, 0, 0), (1, 1, 1), s.white)])
    _refused(s, [w.BVHNode_new([ok, s.tetra(mat=s.white)])])
    assert w.L.rt_scene_set_area_lights(w.h, 1, None) == RT_ERR_ARG
    assert w.L.rt_scene_set_area_lights(None, 0, None) == RT_ERR_ARG
    assert w.L.rt_scene_set_area_lights(w.h, -1, None) == RT_ERR_ARG
    # Transform chains: 8 levels are fine, 9 are not
    t = ok
    for level in range(8):
        t = w.Transform((0.0, 5.0, 0.0), (1.0, 1.0, 1.0), (0.1, 0.0, 0.0), t)
    w.set_area_lights([t])
    _refused(s, [w.Transform((0.0, 5.0, 0.0), (1.0, 1.0, 1.0), (0.1, 0.0, 0.0), t)])
    # a refused call leaves the list as it was; n == 0 clears it
    w.new(s.items)
    assert len(w.area_light_tris()) == 2 and np.all(w.area_light_tris()["light"] == 0)
    _refused(s, [ok])                                                        # a call after commit
    assert "immutable" in w.L.rt_last_error().decode()


def test_empty_list_clears():
    s = build("cube")
    s.w.set_area_lights(s.lights)
    s.w.set_area_lights([])
    s.w.new(s.items)
    assert len(s.w.area_light_tris()) == 0
    assert s.w.fingerprint() == build("cube").commit(area=False).fingerprint()


def _grid_mesh(s, n_tri):
    """a strip of n_tri emissive triangles as one mesh"""
    pos = np.array([[0.25 * (i // 2), 1.0 + (i % 2), 0.0] for i in range(n_tri + 2)])
    idx = [(i, i + 1, i + 2) for i in range(n_tri)]
    return s.w.Mesh(pos, np.tile([0.0, 0.0, 1.0], (len(pos), 1)), idx, s.em)


def test_commit_refusals():
    import rtamd
    s = Scene()
    s.light(_grid_mesh(s, 1024))
    assert len(s.commit().area_light_tris()) == 1024                         # the limit itself is fine
    s = Scene()
    s.light(_grid_mesh(s, 1025))
    with pytest.raises(rtamd.RtError) as e:
        s.commit()
    assert e.value.code == RT_ERR_UNSUPPORTED and "1024" in str(e.value)
    assert s.w.info()["committed"] == 0
    s = Scene()                                                               # ... counted over all area lights
    s.light(_grid_mesh(s, 1000))
    s.light(s.w.Cube((0, 0, 0), (1, 1, 1), s.em))
    s.light(s.w.Cube((2, 0, 0), (3, 1, 1), s.em))
    s.light(s.w.XYRectangle((0.0, 0.0), (1.0, 1.0), 2.0, s.em))
    with pytest.raises(rtamd.RtError) as e:
        s.commit()
    assert e.value.code == RT_ERR_UNSUPPORTED
    # an area light with no triangle of non-zero area
    s = Scene()
    w = s.w
    md = w.MeshData(np.array([[0.0, 1.0, 0.0], [1.0, 1.0, 0.0], [2.0, 1.0, 0.0]]), np.tile([0.0, 1.0, 0.0], (3, 1)))
    s.light(w.XYRectangle((0.0, 0.0), (1.0, 1.0), 2.0, s.em))
    s.light(w.HitableList([w.Triangle(md, 0, 1, 2, s.em), w.Triangle(md, 2, 1, 0, s.em)]))
    with pytest.raises(rtamd.RtError) as e:
        s.commit()
    assert e.value.code == RT_ERR_ARG and "area" in str(e.value)
    s = Scene()                                                               # a rectangle without extent
    s.light(s.w.YZRectangle((0.0, 0.0), (0.0, 1.0), 2.0, s.em))
    with pytest.raises(rtamd.RtError) as e:
        s.commit()
    assert e.value.code == RT_ERR_ARG


@pytest.mark.parametrize("case", ["rect_xy_yz", "tetra_nested", "mixed"])
def test_fingerprint(case):
    with_lights = build(case).commit().fingerprint()
    without = build(case).commit(area=False).fingerprint()
    assert with_lights != 0 and without != 0 and with_lights != without
    assert build(case).commit().fingerprint() == with_lights
    assert build(case).commit().info()["bytes"] > build(case).commit(area=False).info()["bytes"]
    # another list on the same scene is another fingerprint
    s = build(case)
    s.lights = s.lights[:1] if len(s.lights) > 1 else s.lights + [s.w.XYRectangle((0.0, 0.0), (1.0, 1.0), 9.0, s.em)]
    assert s.commit().fingerprint() not in (with_lights, without)


def test_scenes_without_area_lights_keep_their_fingerprints():
    """the blob of every scene that does not use the feature is what it was: scene_10 and the Cornell box, against values recorded
    before area lights existed"""
    import rtamd
    w, _ = rtamd.load_scene_file(scene_path("scene_10.json"))
    assert w.fingerprint() == FP_SCENE_10
    c, _ = rtamd.select_scene(scene_path("cube.obj"), 1.0, 1)
    assert c.fingerprint() == FP_CORNELL
    assert len(w.area_light_tris()) == 0 and len(c.area_light_tris()) == 0


def test_object_lights_keep_their_refusals():
    """rt_scene_set_lights is what it was: only spheres and XZ rectangles"""
    s = Scene()
    w = s.w
    for bad in (w.YZRectangle((0.0, 0.0), (1.0, 1.0), 2.0, s.em), w.Cube((0, 0, 0), (1, 1, 1), s.em), s.tetra()):
        arr = (C.c_int * 1)(bad)
        assert w.L.rt_scene_set_lights(w.h, 1, arr) == RT_ERR_ARG


def test_diagnostics_without_a_device():
    import rtamd
    expect = RT_ERR_NO_DEVICE if rtamd.device_count() == 0 else 0
    w = build("cube").commit()
    x = np.zeros((4, 7))
    out = np.zeros((4, 4))
    dp = C.POINTER(C.c_double)
    assert w.L.rt_debug_area_sample_device(w.h, 0, 4, x.ctypes.data_as(dp), out.ctypes.data_as(dp)) == expect
    assert w.L.rt_debug_area_pdf_device(w.h, 0, 4, x.ctypes.data_as(dp), out.ctypes.data_as(dp)) == expect
    assert w.L.rt_debug_area_pdf_device(w.h, 0, 0, x.ctypes.data_as(dp), out.ctypes.data_as(dp)) == (expect or RT_ERR_ARG)
