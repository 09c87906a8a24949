"""Scenes and configurations for the SPPM photon pass and eye pass, photon by photon and pixel by pixel (tests/test_sppm_trace_cases.py: the
families' construction on the oracle alone, no device; tests/test_sppm_trace_gpu.py: rt_debug_sppm_trace_device -- render_sppm's own light
table, variant choice, launches and grow-and-retry -- against oracle.Scene.sppm_iteration, bit for bit).

Whole SPPM frames see the two passes only through what the gather leaves behind, and never reach what the families below aim at: chunks
that are no multiple of a wave or of PHOTON_CHUNK, launches of less than a wave, one block and one block plus a photon, photon indices
beyond 2^32, a max_bounces that ends paths, several lights (one of weight zero) of both kinds, the clamps of S, every compiled variant of
both passes, stores that are exactly full or one short, and the second trip of the eye pass's grid-stride loop.

A case is a dict: name, scene (a key of SCENES: built once through BOTH builders -> (rtamd.World, rtamd.Camera, oracle.Scene)), width,
height, P (photons_per_iter), iteration, max_bounces, seed, tuning (rt_tuning fields for the call), capacity (None, or a function of the
oracle's counts -> the initial device capacities), launches (photon-pass launches expected), variant (the variant word expected: bit 0
accel, 1 LDS tables, 2 nested chain walk, 3 MEDIA), photons (False: an eye-only case).  Every case is a deterministic function of its name."""
import numpy as np

import nested_scenes as ns
from conftest import scene_path

ACCEL, LDS, NEST, MEDIA = 1, 2, 4, 8


class OB:
    """the oracle's builder has no light constructors: compose them as light.rs:74-86 / 134-146 do, and keep their flux and scale"""

    def __init__(self, o):
        self.o, self.desc = o, {}

    def __getattr__(self, n):
        return getattr(self.o, n)

    def XZRectLight(self, xz0, xz1, y, flux, scale):
        i = self.o.XZRectangle(xz0, xz1, y, self.o.DiffuseLight(self.o.ConstantTexture(flux)))
        self.desc[i] = (flux, scale)
        return i

    def SphereDiffuseLight(self, c, r, flux, scale):
        i = self.o.Sphere(c, r, self.o.DiffuseLight(self.o.ConstantTexture(flux)))
        self.desc[i] = (flux, scale)
        return i


def _pair(build, cam_args, bvh_seed=1):
    """build(B) -> (items, lights) on both builders: (rtamd.World, rtamd.Camera, oracle.Scene)"""
    import oracle
    import rtamd
    w = rtamd.World()
    items, lights = build(w)
    w.new(items, lights=lights, bvh_seed=bvh_seed)
    o = oracle.Scene()
    ob = OB(o)
    oitems, olights = build(ob)
    o.World(oitems, bvh_seed)
    o.set_lights(olights, flux=[ob.desc[i][0] for i in olights], scale=[ob.desc[i][1] for i in olights])
    o.Camera(*cam_args)
    f, t, up, vfov, asp, ap, fd = cam_args
    return w, rtamd.Camera((f, t), up, vfov, asp, ap, fd), o


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
CORNELL_CAM = ns.CORNELL_CAM
FAR_CAM = ((278.0, 278.0, -200000.0), (278.0, 278.0, 278.0), (0.0, 1.0, 0.0), 0.2, 1.5, 0.0, 10.0)     # beyond origin_limit2 = 64 x the extent
INSIDE_CAM = ((278.0, 278.0, -800.0), (278.0, 278.0, 278.0), (0.0, 1.0, 0.0), 30.0, 1.125, 0.0, 10.0)     # every pixel looks into the box, the last row too
GLASS_CAM = ((0.0, 4.0, -8.0), (0.0, 0.5, 0.0), (0, 1, 0), 40.0, 1.0, 0.25, 8.0)                        # aperture > 0: the lens draws


def _cornell(cam_args=None):
    """the reference's Cornell box through rt_scene_cornell_box and oracle.cornell_box_scene"""
    import oracle
    import rtamd
    cube = scene_path("cube.obj")
    w, cam = rtamd.select_scene(cube, 1.0, 1)
    o = oracle.cornell_box_scene(cube, 1.0, seed=1)
    if cam_args is not None:
        o.Camera(*cam_args)
        f, t, up, vfov, asp, ap, fd = cam_args
        cam = rtamd.Camera((f, t), up, vfov, asp, ap, fd)
    return w, cam, o


def _cornell_light(B):
    return B.XZRectLight((213.0, 227.0), (343.0, 332.0), 554.0, (1.0, 1.0, 1.0), 1000000.0)


def _cornell_smoke(B):
    """Cornell walls, the ceiling light, a glass ball and two axis-aligned Cube-bounded media, one dark and one light (world level)"""
    white, items = ns.walls(B)
    glass = B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0)))
    dark = B.Isotropic(B.ConstantTexture((0.05, 0.05, 0.05)))
    light = B.Isotropic(B.ConstantTexture((0.9, 0.9, 0.9)))
    lt = _cornell_light(B)
    items += [lt, B.Sphere((400.0, 90.0, 150.0), 70.0, glass),
              B.ConstantMedium(0.01, B.Cube((130.0, 0.0, 65.0), (295.0, 165.0, 230.0), white), dark),
              B.ConstantMedium(0.01, B.Cube((265.0, 0.0, 295.0), (430.0, 330.0, 460.0), white), light)]
    return items, [lt]


def _cornell_smoke_book(B):
    """the book's Cornell smoke: both fog boxes rotated and translated, the media under the Transforms (no accel: reference-order walks)"""
    white, items = ns.walls(B)
    dark = B.Isotropic(B.ConstantTexture((0.0, 0.0, 0.0)))
    light = B.Isotropic(B.ConstantTexture((1.0, 1.0, 1.0)))
    lt = _cornell_light(B)
    box1 = B.Transform((0.0, 15.0, 0.0), (1.0, 1.0, 1.0), (265.0, 0.0, 295.0),
                       B.ConstantMedium(0.01, B.Cube((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), white), dark))
    box2 = B.Transform((0.0, -18.0, 0.0), (1.0, 1.0, 1.0), (130.0, 0.0, 65.0),
                       B.ConstantMedium(0.01, B.Cube((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white), light))
    items += [lt, box1, box2]
    return items, [lt]


def _nested_fog(B):
    """nested Transforms (chains of 2 levels) beside and around media: a chain around a cube, a world-level fog whose boundary is a
    2-level chain of a cube, a fog sphere at world level"""
    white, items = ns.walls(B)
    L = [((0.0, 0.0, 10.0), (1.0, 1.3, 1.0), (0.0, 0.0, 0.0)), ((0.0, -20.0, 0.0), (1.0, 1.0, 1.0), (150.0, 0.0, 120.0))]
    box = ns.nest(B, L, B.Cube((0.0, 0.0, 0.0), (100.0, 100.0, 100.0), white))
    fog_box = B.ConstantMedium(0.012, ns.nest(B, [((0.0, 30.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((5.0, 0.0, 0.0), (1.1, 1.0, 0.9), (330.0, 0.0, 300.0))],
                                           B.Cube((0.0, 0.0, 0.0), (150.0, 300.0, 150.0), white)), B.Isotropic(B.ConstantTexture((0.8, 0.8, 0.9))))
    fog_ball = B.ConstantMedium(0.02, B.Sphere((400.0, 90.0, 120.0), 80.0, white), B.Isotropic(B.ConstantTexture((0.3, 0.6, 0.3))))
    lt = _cornell_light(B)
    items += [lt, box, fog_box, fog_ball]
    return items, [lt]


def _nested_boxes(B):
    """tests/nested_scenes.n1 with the ceiling light: each box Transform(Transform(cube)), both under an outer Transform of a BVHNode"""
    white, items = ns.walls(B)
    box1 = ns.nest(B, [((0.0, 0.0, 0.0), (1.0, 2.0, 1.0), (0.0, 0.0, 0.0)), ((0.0, 15.0, 0.0), (1.0, 1.0, 1.0), (265.0, 0.0, 295.0))],
                   B.Cube((0.0, 0.0, 0.0), (82.5, 82.5, 82.5), white))
    box2 = ns.nest(B, [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((0.0, -18.0, 0.0), (1.0, 1.0, 1.0), (130.0, 0.0, 65.0))],
                   B.Cube((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white))
    inner = B.BVHNode_new([box1, box2], 2) if isinstance(B, OB) else B.BVHNode_new([box1, box2], bvh_seed=2)
    group = B.Transform((0.0, 4.0, 0.0), (1.0, 1.0, 1.0), (10.0, 0.0, -12.0), inner)
    lt = _cornell_light(B)
    return items + [lt, group], [lt]


def _glass_and_metal(B):
    """the scene of tests/test_sppm.py's sphere-light test: a sphere light above a glass ball and a metal ball on a diffuse floor"""
    white = B.Lambertian(B.ConstantTexture((0.8, 0.8, 0.8)))
    items = [B.XZRectangle((-6.0, -6.0), (6.0, 6.0), 0.0, white),
             B.Sphere((0.0, 1.0, 0.0), 1.0, B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0)))),
             B.Sphere((2.2, 0.7, 0.5), 0.7, B.Metal(B.ConstantTexture((0.9, 0.9, 0.9)), 0.0))]
    light = B.SphereDiffuseLight((0.0, 5.0, 0.0), 0.3, (1.0, 0.9, 0.8), 500.0)
    return items + [light], [light]


# four lights in one list: sphere, rectangle of scale 0, rectangle, sphere.  A light's flux has one channel of its own (the zero light all
# three), and no material of the scene mixes channels, so a stored photon names its emitter by which power channels are not zero.
FOUR_LIGHTS = (("sphere", (1.0, 0.0, 0.0), 500.0), ("rect", (1.0, 1.0, 1.0), 0.0), ("rect", (0.0, 1.0, 0.0), 100.0), ("sphere", (0.0, 0.0, 1.0), 60.0))


def _four_lights(B):
    white = B.Lambertian(B.ConstantTexture((0.8, 0.8, 0.8)))
    items = [B.XZRectangle((-8.0, -8.0), (8.0, 8.0), 0.0, white), B.XYRectangle((-8.0, 0.0), (8.0, 8.0), 8.0, white),
             B.Sphere((0.0, 1.0, 0.0), 1.0, B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0))))]
    lights = [B.SphereDiffuseLight((-3.0, 4.0, 0.0), 0.3, FOUR_LIGHTS[0][1], FOUR_LIGHTS[0][2]),
              B.XZRectLight((-1.0, -1.0), (1.0, 1.0), 6.0, FOUR_LIGHTS[1][1], FOUR_LIGHTS[1][2]),
              B.XZRectLight((2.0, 1.0), (4.0, 3.0), 5.0, FOUR_LIGHTS[2][1], FOUR_LIGHTS[2][2]),
              B.SphereDiffuseLight((3.0, 3.0, -2.0), 0.4, FOUR_LIGHTS[3][1], FOUR_LIGHTS[3][2])]
    return items + lights, lights


def _one_light(scale):
    """a sphere light of flux (1, 0.5, 0.25) x scale above a floor: the largest power component is exactly `scale`"""
    def build(B):
        white = B.Lambertian(B.ConstantTexture((0.8, 0.8, 0.8)))
        light = B.SphereDiffuseLight((0.0, 3.0, 0.0), 0.5, (1.0, 0.5, 0.25), scale)
        return [B.XZRectangle((-6.0, -6.0), (6.0, 6.0), 0.0, white), light], [light]
    return build


S_EDGES = (("one", 1.0, 39), ("2p45", 2.0 ** 45, 0), ("2m30", 2.0 ** -30, 60))       # frexp(1.0) = 0.5 * 2^1: S = 40 - 1; the clamps 0 and 60

SCENES = {
    "cornell": _cornell,
    "cornell_far": lambda: _cornell(FAR_CAM),
    "cornell_inside": lambda: _cornell(INSIDE_CAM),
    "glass_and_metal": lambda: _pair(_glass_and_metal, GLASS_CAM),
    "smoke": lambda: _pair(_cornell_smoke, CORNELL_CAM, bvh_seed=2),
    "smoke_book": lambda: _pair(_cornell_smoke_book, CORNELL_CAM, bvh_seed=3),
    "nested_fog": lambda: _pair(_nested_fog, CORNELL_CAM, bvh_seed=4),
    "nested_boxes": lambda: _pair(_nested_boxes, CORNELL_CAM),
    "four_lights": lambda: _pair(_four_lights, GLASS_CAM),
}
for _name, _scale, _S in S_EDGES:
    SCENES["light_" + _name] = (lambda sc: (lambda: _pair(_one_light(sc), GLASS_CAM)))(_scale)

_SCENE, _CACHE, _ORACLE = {}, {}, {}


def scene(key):
    """(rtamd.World, rtamd.Camera, oracle.Scene) of SCENES[key], built once"""
    if key not in _SCENE:
        _SCENE[key] = SCENES[key]()
    return _SCENE[key]


def case(name, scene_key, width, height, P, iteration=0, max_bounces=4096, seed=1, variant=ACCEL | LDS, tuning=None, capacity=None, launches=1,
         photons=True, **extra):
    c = dict(name=name, scene=scene_key, width=int(width), height=int(height), P=int(P), iteration=int(iteration), max_bounces=int(max_bounces),
             seed=int(seed), variant=int(variant), tuning=dict(tuning or {}), capacity=capacity, launches=int(launches), photons=bool(photons))
    c.update(extra)
    return c


# ---- a. photon counts around the wave, the chunk and the block ----------------------------------------------------------------------------------
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2049, 4097)


def counts():
    return [case("counts_P%d_it%d" % (P, it), "cornell", 37, 21, P, it, seed=1 + it) for P in COUNTS for it in (0, 3)]


# ---- b. photon indices beyond 2^32 --------------------------------------------------------------------------------------------------------------
# at P = 1025: 4 190 208 ends 3 071 photons below 2^32; 4 190 211 * 1025 = 2^32 - 1 021, so that launch crosses 2^32 inside its last
# chunk; the others lie beyond it.  At P = 257 only 2^31 - 1 does.
FAR_ITERATIONS = (4190208, 4190211, 5000000, 2 ** 31 - 1)


def far_index():
    return [case("far_index_P%d_it%d" % (P, it), "cornell", 37, 21, P, it, seed=2) for P in (257, 1025) for it in FAR_ITERATIONS]


# ---- c. max_bounces that end paths --------------------------------------------------------------------------------------------------------------
BOUNCES = (1, 2, 3, 4096)


def bounces():
    out = [case("bounces_glass_%d" % mb, "glass_and_metal", 36, 24, 1025, 1, max_bounces=mb, seed=4) for mb in BOUNCES]
    out += [case("bounces_smoke_%d" % mb, "smoke", 36, 24, 1025, 1, max_bounces=mb, seed=4, variant=ACCEL | LDS | MEDIA) for mb in BOUNCES]
    return out


# ---- d. several lights, and the three edges of S ------------------------------------------------------------------------------------------------
def lights():
    out = [case("lights_four", "four_lights", 36, 24, 4097, 2, seed=5)]
    out += [case("lights_S_" + name, "light_" + name, 8, 6, 64, 0, seed=6, S=S) for name, _, S in S_EDGES]
    return out


def emitter_counts(rows):
    """photons of FOUR_LIGHTS' emitters in a map of the four-lights scene: (red sphere, zero rectangle, green rectangle, blue sphere)"""
    nz = rows[:, 3:6] != 0.0
    return (int((nz[:, 0] & ~nz[:, 1] & ~nz[:, 2]).sum()), int((~nz.any(axis=1)).sum()), int((~nz[:, 0] & nz[:, 1] & ~nz[:, 2]).sum()),
            int((~nz[:, 0] & ~nz[:, 1] & nz[:, 2]).sum()))


# ---- e. one scene per compiled variant ----------------------------------------------------------------------------------------------------------
VARIANTS = (
    ("accel_lds", "cornell", None, ACCEL | LDS),                       # photon_kernel<true, true>, eye_kernel<true>
    ("accel", "cornell", dict(no_lds=1), ACCEL),                       # photon_kernel<true, false>
    ("reference_order", "cornell_far", None, 0),                       # photon_kernel<false, false>, eye_kernel<false>
    ("nest", "nested_boxes", None, NEST),                              # photon_kernel_nest, eye_kernel_nest
    ("media_accel_lds", "smoke", None, ACCEL | LDS | MEDIA),           # photon_kernel_media<true, true>, eye_kernel_media<true>
    ("media_accel", "smoke", dict(no_lds=1), ACCEL | MEDIA),           # photon_kernel_media<true, false>
    ("media_reference_order", "smoke_book", None, MEDIA),              # photon_kernel_media<false, false>, eye_kernel_media<false>
    ("media_nest", "nested_fog", None, NEST | MEDIA),                  # photon_kernel_nest_media, eye_kernel_nest_media
)


def variants():
    return [case("variant_%s_P%d" % (name, P), key, 36, 24, P, 1, seed=7, variant=word, tuning=tun)
            for name, key, tun, word in VARIANTS for P in (65, 1025)]


# ---- f. stores that are exactly full, one short, and far too small ------------------------------------------------------------------------------
CAPACITIES = (("exact", lambda G, C_: (G, C_), 1), ("global_one_short", lambda G, C_: (G - 1, C_), 2),
              ("caustic_one_short", lambda G, C_: (G, C_ - 1), 2), ("one_each", lambda G, C_: (1, 1), 2))


def capacity():
    return [case("capacity_" + name, "cornell", 37, 21, 1025, 0, seed=8, capacity=fn, launches=n) for name, fn, n in CAPACITIES]


# ---- g. the second trip of the eye pass's grid-stride loop ---------------------------------------------------------------------------------------
STRIDE_WIDTH = 768


def stride(multi_processor_count=256):
    """an eye-only case of just above multi_processor_count * 8 * 256 pixels (the eye pass launches at most 8 blocks of 256 per CU)"""
    h = multi_processor_count * 8 * 256 // STRIDE_WIDTH + 1
    return [case("stride_%dx%d" % (STRIDE_WIDTH, h), "cornell_inside", STRIDE_WIDTH, h, 1, 0, seed=9, photons=False, launches=0, cus=multi_processor_count)]


FAMILIES = dict(a_counts=counts, b_far_index=far_index, c_bounces=bounces, d_lights=lights, e_variants=variants, f_capacity=capacity,
                g_stride=stride)


def family(name, *args):
    """the list of cases of family `name` (g_stride: for a device of args[0] CUs), built once"""
    key = (name,) + args
    if key not in _CACHE:
        _CACHE[key] = FAMILIES[name](*args)
    return _CACHE[key]


def oracle_run(c):
    """(global [n, 9], caustic [n, 9], points [W * H, 7], S) of the oracle's sppm_iteration for the case, computed once and read-only"""
    if c["name"] not in _ORACLE:
        _, _, o = scene(c["scene"])
        out = o.sppm_iteration(c["width"], c["height"], c["iteration"], c["P"], max_bounces=c["max_bounces"], seed=c["seed"])
        for a in out[:3]:
            a.setflags(write=False)
        _ORACLE[c["name"]] = out
    return _ORACLE[c["name"]]


def sorted_rows(rows):
    """a photon map as a multiset: 0.0 added to every value (a negative zero compares as the rest of the suite compares it), the rows
    sorted lexicographically by their nine uint64 patterns"""
    u = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 9) + 0.0).view(np.uint64)
    return u[np.lexsort(u.T[::-1])]
