"""Composed scenes for tests/test_soup_scenes.py (the corpus is not vacuous: the oracle alone, no device) and tests/test_soup_gpu.py (every
render kernel, integrator and residency, the hit and any-hit walks, the guide and ambient-occlusion passes: HIP == oracle bit for bit, or
the refusal include/rtamd.h documents).

The feature tests of this suite hold each feature to the oracle on scenes built by hand for that feature.  Here a seeded generator crosses
the features: recipe(index) draws one value on each axis of AXES, composes a scene from it and describes that scene as nested tuples of
plain Python values (no ids, no arrays: repr() of a recipe is its identity, and tests/golden/soup_pins.json pins a digest of it).
build(recipe) makes both sides of it, rtamd.World and oracle.Scene, which share the reference's constructor names.

CORPUS walks the indices 0, 1, 2, ... and keeps an index when its recipe shows a pair of values of two axes (legal together, see
legal_pair) that no kept recipe showed before, or fills a cell of CELLS (a kernel x integrator of the render matrix, or another entry point,
answering with a frame and not a refusal) that fewer than MIN_SCENES kept recipes fill; it ends when every legal pair has occurred and every
cell is full.  Its length is CORPUS_LENGTH.

expected() restates from the words of include/rtamd.h what every call on a recipe must do: RULES has one row per sentence, with the
header line it restates beside it.  Nothing here reads the library's own kernel selection.

Replaced indices.  REPLACED: recipes whose HIP frame or record differed from the oracle's in a way DESIGN.md s2 documents as measure zero
(shown from the oracle alone), at most two.  VACUOUS: recipes that failed a condition of tests/test_soup_scenes.py when the corpus was
written (a frame too dark, a primitive kind no test ray reaches, ...).  CORPUS passes over both.

SPPM.  The recipes rt_render_sppm renders have a sub-corpus of their own, SPPM_CORPUS, with its axes, cells, configuration and passed-over
tables (the last section of this file; tests/test_soup_sppm_scenes.py, tests/test_soup_sppm_gpu.py)."""
import hashlib

import numpy as np

REPLACED = {}   # index -> the ray and the measure-zero condition it meets
# index -> the condition of tests/test_soup_scenes.py its recipe failed
VACUOUS = {}

W, H, SPP, SEED, T_MIN = 20, 12, 8, 5, 1e-3   # 20 x 12: partial 8 x 8 tiles on both edges
FRAME = "frame"
ARG, UNSUPPORTED = -1, -10                     # rt_status (include/rtamd.h): RT_ERR_ARG, RT_ERR_UNSUPPORTED
N_EXPLICIT, N_PAIR_RAYS = 64, 32
EXACT_ROWS = 50                                # any-hit rows asked at the oracle's own t and its two neighbours

AXES = (
    ("root", ("list", "bvh")),                                     # HitableList in item order / World::new with a drawn bvh_seed
    ("spheres", (0, 1)), ("rects", (0, 1)), ("cube", (0, 1)),      # primitives, each present or absent
    ("small_mesh", (0, 1)),                                        # cube.obj: < 64 object-space nodes
    ("big_mesh", (0, 1)),                                          # shapes.torus(12, 16), f32 vertices: >= 64 nodes
    ("tris", (0, 1)),                                              # MeshData + Triangle under hand-wired BVHNodes
    ("depth", (0, 1, "chain")),                                    # Transforms over the meshes and one more object: none / one level / 2..4 nested
    ("special", ("none", "medium", "moving")),                     # a ConstantMedium (in a sphere, in a cube, or under the Transforms: drawn) / moving spheres, open shutter
    ("emitters", ("none", "object", "area", "both")),
    ("background", ("none", "constant", "gradient", "texture", "constant+env", "gradient+env", "texture+env")),
    ("coplanar", ("none", "rect_on_cube", "cubes")),
    ("scale", (0.01, 1.0, 100.0)),
)
AXIS_NAMES = tuple(a for a, _ in AXES)
PRIMITIVE_AXES = ("spheres", "rects", "cube", "small_mesh", "big_mesh", "tris")
GROUND_AXES = ("rects", "spheres", "cube", "tris")   # the kinds that can carry the scene's ground, in this order of preference


def legal_pair(a, va, b, vb):
    """may value va of axis a occur with value vb of axis b?  (Every other constraint of legal() takes three axes or more.)"""
    d = {a: va, b: vb}
    if d.get("emitters") == "none" and d.get("background") == "none":
        return False                                   # every recipe has a background or an emitter
    return True


def legal(ax):
    if sum(ax[k] for k in PRIMITIVE_AXES) < 2 or not any(ax[k] for k in GROUND_AXES):
        return False
    return all(legal_pair(a, ax[a], b, ax[b]) for i, a in enumerate(AXIS_NAMES) for b in AXIS_NAMES[i + 1:])


def all_pairs():
    """every legal pair ((axis a, value), (axis b, value)), a before b in AXES"""
    return {((a, va), (b, vb)) for i, (a, A) in enumerate(AXES) for b, B in AXES[i + 1:] for va in A for vb in B if legal_pair(a, va, b, vb)}


def pairs_of(ax):
    return {((a, ax[a]), (b, ax[b])) for i, a in enumerate(AXIS_NAMES) for b in AXIS_NAMES[i + 1:]}


# ---- drawing a recipe -------------------------------------------------------------------------------------------------------------------
def _f(v):
    return tuple(float(x) for x in v)


def _pick(rng, seq, weights=None):
    w = None if weights is None else np.asarray(weights, dtype=float) / float(sum(weights))
    return seq[int(rng.choice(len(seq), p=w))]


def _color(rng, lo=0.15, hi=0.95):
    return _f(rng.uniform(lo, hi, 3))


def _texture(rng, noise_ok, S):
    kind = _pick(rng, ("const", "checker", "image", "noise"), (5, 2, 2, 3 if noise_ok else 0))
    if kind == "const":
        return ("const", _color(rng))
    if kind == "checker":
        return ("checker", _color(rng), _color(rng))
    if kind == "image":
        return ("image", int(rng.integers(1, 1 << 30)))
    return ("noise", float(rng.uniform(2.0, 6.0) / S), int(rng.integers(1, 1000)))


def _material(rng, noise_ok, S):
    kind = _pick(rng, ("lambertian", "metal", "dielectric"), (4, 2, 1))
    if kind == "lambertian":
        return ("lambertian", _texture(rng, noise_ok, S))    # (only Lambertians and lights carry non-constant textures: tests read their albedo through oracle.scatter)
    if kind == "metal":
        return ("metal", ("const", _color(rng, 0.5, 0.95)), float(rng.uniform(0.0, 0.4)))
    return ("dielectric", 1.5, ("const", _color(rng, 0.9, 1.0)))


def _levels(rng, depth, at, S, size):
    """(rotate, scale, translate) innermost first: the outermost level rotates about all axes, scales non-uniformly (by S too) and moves
    the object to `at`; the inner levels of a chain turn, stretch and shift it a little in its own space"""
    n = 1 if depth == 1 else int(rng.integers(2, 5))
    out = [(_f(rng.uniform(-25.0, 25.0, 3)), _f(rng.uniform(0.8, 1.25, 3)), _f(rng.uniform(-0.2, 0.2, 3))) for _ in range(n - 1)]
    out.append((_f(rng.uniform(-40.0, 40.0, 3)), _f(rng.uniform(0.75, 1.2, 3) * size * S), _f(np.asarray(at) * S)))
    return tuple(out)


# Kernels 5 / 6 render a scene without a background only, so `none` is drawn as often as the six backgrounds together are not:
# three times the weight of each other value.  Every other axis is uniform.
WEIGHTS = {"background": (3, 1, 1, 1, 1, 1, 1)}


def _draw_axes(rng):
    return {a: _pick(rng, vals, WEIGHTS.get(a)) for a, vals in AXES}


def recipe(index):
    """the recipe of an index: a deterministic function of it"""
    for salt in range(1000):
        rng = np.random.default_rng([0x50C9, int(index), salt])
        ax = _draw_axes(rng)
        if legal(ax):
            return _compose(ax, rng)
    raise AssertionError("no legal draw for index %d" % index)


def _compose(ax, rng):
    S = float(ax["scale"])
    depth = ax["depth"]
    noise_ok = bool(rng.random() < 1.0 / 6.0)     # a noise texture makes a book-2 scene (integrator 0, kernels 1 / 2): keep most recipes free of it
    mat = lambda: _material(rng, noise_ok, S)  # noqa: E731
    grey = ("lambertian", ("const", _color(rng, 0.55, 0.8)))
    slots = [np.array([x, 0.0, z]) + np.concatenate([rng.uniform(-0.25, 0.25, 1), [0.0], rng.uniform(-0.25, 0.25, 1)])
             for z in (0.4, 3.7) for x in (-5.2, -2.6, 0.0, 2.6, 5.2)]
    order = [int(i) for i in rng.permutation(len(slots))]
    front = [i for i in order if i < 5]            # the row nearest the camera: the coplanar pair goes there, where primary rays see it
    items = []

    def slot(first_row=False):
        i = front[0] if first_row else order[0]
        order.remove(i)
        front[:] = [j for j in front if j != i]
        return slots[i]

    def placed(group, make_world, make_object, size, wrap):
        """an object at the next slot: in world space, or in its own space under `depth` levels of Transforms"""
        at = slot() + np.array([0.0, size + float(rng.uniform(0.02, 0.3)), 0.0])
        if not wrap or depth == 0:
            return make_world(group, at)
        return ("xf", group, _levels(rng, depth, at, S, size), make_object(group))

    def w_cube(m, grow=1.0):
        return lambda group, at: (lambda h: ("cube", group, _f((at - h) * S), _f((at + h) * S), m))(rng.uniform(0.6, 1.0, 3) * grow)

    def o_cube(m):
        return lambda group: (lambda h: ("cube", group, _f(-h), _f(h), m))(rng.uniform(0.7, 1.0, 3))

    pair = None
    if ax["coplanar"] != "none":                   # first: its slot is in the front row
        at = slot(True) + np.array([0.0, 1.0 + float(rng.uniform(0.02, 0.3)), 0.0])
        h = rng.uniform(0.7, 0.95, 3)
        lo, hi = at - h, at + h
        # The reference decides an exact tie for the object it visits later -- unless that object's own BVHNode box begins at the tied t and
        # is culled.  So the later object of a pair is a cube in a 1-object BVHNode (its box is the cube), entered through the
        # shared plane: the case the tie rule of the accel walks exists for.
        leaf = lambda d: ("leaf", d[1], int(rng.integers(1, 1000)), d)  # noqa: E731
        if ax["coplanar"] == "rect_on_cube":       # an XY rectangle lying on the cube's front face z = lo.z (the same double) and reaching beyond it
            a = leaf(("cube", "pair_a", _f(lo * S), _f(hi * S), mat()))
            r0, r1 = lo[:2] - rng.uniform(0.1, 0.4, 2) * h[:2], hi[:2] + rng.uniform(0.1, 0.4, 2) * h[:2]
            b = ("rect", "pair_b", 2, _f(r0 * S), _f(r1 * S), a[3][2][2], mat())
            a, b = b, a                            # the rectangle first: in item order, and in every sort of BVHNode::new (its box begins before the cube's on every axis)
        else:                                      # two cubes sharing the face x = mid (the same double on both)
            mid = float((at[0] + rng.uniform(-0.3, 0.3)) * S)
            lo2 = lo + rng.uniform(-0.2, 0.2, 3)
            hi2 = hi + rng.uniform(-0.2, 0.2, 3)
            a = leaf(("cube", "pair_a", _f(lo * S), (mid,) + _f(hi[1:] * S), mat()))
            b = leaf(("cube", "pair_b", (mid,) + _f(lo2[1:] * S), _f(hi2 * S), mat()))
        pair = (len(items), len(items) + 1)
        items += [a, b]
    ground = next(k for k in GROUND_AXES if ax[k])
    if ax["rects"]:
        y = float(rng.uniform(-0.05, 0.05))
        x0, x1, z0, z1 = float(rng.uniform(-7.6, -7.1)), float(rng.uniform(7.1, 7.6)), float(rng.uniform(-5.5, -4.5)), float(rng.uniform(7.4, 7.9))
        items.append(("rect", "rects:xz", 1, _f((x0 * S, z0 * S)), _f((x1 * S, z1 * S)), y * S, ("lambertian", _texture(rng, noise_ok, S))))
        items.append(("rect", "rects:xy", 2, _f((rng.uniform(-6.5, -5.5) * S, y * S)), _f((rng.uniform(5.5, 6.5) * S, rng.uniform(4.5, 5.5) * S)),
                      float(rng.uniform(7.0, 7.3) * S), mat()))
        items.append(("rect", "rects:yz", 0, _f((y * S, rng.uniform(-3.0, -2.0) * S)), _f((rng.uniform(4.5, 5.5) * S, rng.uniform(6.5, 7.0) * S)),
                      float(rng.uniform(-6.9, -6.6) * S), mat()))
    if ax["spheres"]:
        for _ in range(2):
            r = float(rng.uniform(0.6, 1.1))
            items.append(("sphere", "spheres", _f((slot() + np.array([0.0, r + rng.uniform(0.02, 0.3), 0.0])) * S), r * S, mat()))
        if ground == "spheres":
            R = float(rng.uniform(350.0, 450.0))
            items.append(("sphere", "spheres", _f((rng.uniform(-1.0, 1.0) * S, -R * S, rng.uniform(1.0, 3.0) * S)), R * S, grey))
    wrapped = False
    if ax["cube"]:
        m = mat()
        items.append(placed("cube", w_cube(m), o_cube(m), 1.0, True))
        wrapped = depth != 0
        if ground == "cube":
            items.append(("cube", "cube", _f((rng.uniform(-7.6, -7.1) * S, rng.uniform(-0.9, -0.5) * S, rng.uniform(-5.5, -4.5) * S)),
                          _f((rng.uniform(7.1, 7.6) * S, rng.uniform(-0.04, 0.04) * S, rng.uniform(7.4, 7.9) * S)), grey))
    for name, kind in (("small_mesh", "obj"), ("big_mesh", "torus")):
        if ax[name]:
            m, size = mat(), (0.75 if kind == "obj" else 0.8)
            extra = () if kind == "obj" else (int(rng.integers(1, 100)),)
            items.append(placed(name, lambda group, at: (kind, group, m) + extra + ((size * float(rng.uniform(0.85, 1.15)) * S, _f(at * S)),),
                                lambda group: (kind, group, m) + extra + (None,), size, True))
            wrapped = wrapped or depth != 0
    if ax["tris"]:                                 # a four-sided pyramid (and the ground, if no other kind carries it): one MeshData, hand-wired BVHNodes
        at = slot()
        base = [at + np.array([sx * rng.uniform(0.7, 1.1), rng.uniform(0.02, 0.2), sz * rng.uniform(0.7, 1.1)]) for sx, sz in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        apex = at + np.array([rng.uniform(-0.2, 0.2), rng.uniform(1.5, 2.2), rng.uniform(-0.2, 0.2)])
        verts = base + [apex]
        faces = [(0, 4, 1), (1, 4, 2), (2, 4, 3), (3, 4, 0)]
        if ground == "tris":
            y = float(rng.uniform(-0.05, 0.0))
            verts += [np.array([rng.uniform(-7.6, -7.1), y, rng.uniform(-5.5, -4.5)]), np.array([rng.uniform(7.1, 7.6), y, rng.uniform(-5.5, -4.5)]),
                      np.array([rng.uniform(7.1, 7.6), y, rng.uniform(7.4, 7.9)]), np.array([rng.uniform(-7.6, -7.1), y, rng.uniform(7.4, 7.9)])]
            faces += [(5, 7, 6), (5, 8, 7)]
        centre = np.mean(verts[:5], axis=0)
        normals = [(v - centre) / np.linalg.norm(v - centre) for v in verts[:5]] + [np.array([0.0, 1.0, 0.0])] * (len(verts) - 5)
        items.append(("tris", "tris", tuple(_f(v * S) for v in verts), tuple(_f(n) for n in normals), tuple(faces), grey if ground == "tris" else mat()))
    if depth != 0 and not wrapped:                 # no mesh and no cube: a sphere of its own under the Transforms
        r = float(rng.uniform(0.6, 1.0))
        m = mat()
        at = slot() + np.array([0.0, r + 0.3, 0.0])
        items.append(("xf", "wrapped", _levels(rng, depth, at, S, r), ("sphere", "wrapped", (0.0, 0.0, 0.0), 1.0, m)))
    shutter = None
    sp = ax["special"]
    if sp == "medium":
        sp = _pick(rng, ("medium_sphere", "medium_cube", "medium_xf"), (1, 1, 0 if depth == 0 else 1))   # (under a Transform where the recipe has any)
        albedo = _color(rng, 0.2, 0.95)
        at = slot() + np.array([0.0, 1.2, 0.0])
        white = ("lambertian", ("const", (0.7, 0.7, 0.7)))
        if sp == "medium_sphere":
            items.append(("medium", "special", float(rng.uniform(0.4, 0.9) / S), ("sphere", "special", _f(at * S), float(rng.uniform(0.9, 1.15) * S), white), albedo))
        elif sp == "medium_cube":
            items.append(("medium", "special", float(rng.uniform(0.4, 0.9) / S), w_cube(white)("special", at), albedo))
        else:                                      # the medium itself under the Transforms (kernel 1 only)
            items.append(("xf", "special", _levels(rng, depth, at, S, 1.0), ("medium", "special", float(rng.uniform(0.4, 0.9)), o_cube(white)("special"), albedo)))
    elif sp == "moving":
        shutter = (0.0, 1.0)
        for _ in range(2):
            r = float(rng.uniform(0.5, 0.9))
            c0 = slot() + np.array([0.0, r + rng.uniform(0.05, 0.4), 0.0])
            c1 = c0 + rng.uniform(-0.6, 0.6, 3) * np.array([1.0, 0.5, 1.0]) + np.array([0.0, 0.3, 0.0])
            items.append(("msphere", "special", _f(c0 * S), _f(c1 * S), r * S, mat()))
    lights, area = [], []
    em = ax["emitters"]
    if em in ("object", "both"):
        which = _pick(rng, ("rect", "sphere", "both"))
        if which in ("rect", "both"):
            lights.append(len(items))
            items.append(("xzlight", "emit", _f((rng.uniform(-4.0, -2.5) * S, rng.uniform(-2.0, -0.5) * S)), _f((rng.uniform(2.5, 4.0) * S, rng.uniform(3.5, 5.0) * S)),
                          float(rng.uniform(6.0, 6.5) * S), _f(rng.uniform(3.0, 6.0, 3))))
        if which in ("sphere", "both"):
            lights.append(len(items))
            items.append(("spherelight", "emit", _f((rng.uniform(2.5, 4.5) * S, rng.uniform(4.3, 5.0) * S, rng.uniform(0.0, 2.5) * S)), float(rng.uniform(1.1, 1.5) * S),
                          _f(rng.uniform(4.0, 8.0, 3))))
    if em in ("area", "both"):
        glow = ("light", ("const", _f(rng.uniform(4.0, 8.0, 3))))
        which = _pick(rng, ("xy", "yz", "cube", "mesh"))
        under = depth != 0 and bool(rng.random() < 0.6)
        air = np.array([rng.uniform(-4.0, -1.0), rng.uniform(4.4, 5.0), rng.uniform(1.0, 3.0)])
        if which == "xy":
            a, b, k = rng.uniform(-3.5, -2.0), rng.uniform(2.0, 3.5), rng.uniform(6.6, 6.9)
            d = ("rect", "emit", 2, _f((a * S, 0.8 * S)), _f((b * S, rng.uniform(3.5, 4.5) * S)), float(k * S), glow)
            if under:
                d = ("xf", "emit", ((_f(rng.uniform(-8.0, 8.0, 3)), _f(rng.uniform(0.9, 1.1, 3)), _f(rng.uniform(-0.2, 0.2, 3) * S)),), d)
        elif which == "yz":
            d = ("rect", "emit", 0, _f((rng.uniform(0.5, 1.0) * S, rng.uniform(-1.0, 0.0) * S)), _f((rng.uniform(3.5, 4.5) * S, rng.uniform(4.0, 5.5) * S)),
                 float(rng.uniform(6.2, 6.5) * S), glow)
            if under:
                d = ("xf", "emit", ((_f(rng.uniform(-8.0, 8.0, 3)), _f(rng.uniform(0.9, 1.1, 3)), _f(rng.uniform(-0.2, 0.2, 3) * S)),), d)
        elif which == "cube":
            d = ("xf", "emit", _levels(rng, 1, air, S, 1.3), o_cube(glow)("emit")) if under else w_cube(glow, 1.4)("emit", air)
        else:
            d = ("xf", "emit", _levels(rng, 1, air, S, 1.1), ("obj", "emit", glow, None)) if under else ("obj", "emit", glow, (1.1 * S, _f(air * S)))
        area.append(len(items))
        items.append(d)
    bg = env = None
    kind = ax["background"].split("+")[0]
    if kind == "constant":
        bg = ("constant", _color(rng, 0.3, 0.9), float(rng.uniform(0.8, 1.6)))
    elif kind == "gradient":
        bg = ("gradient", _color(rng, 0.6, 1.0), _color(rng, 0.3, 1.0), float(rng.uniform(0.8, 1.6)))
    elif kind == "texture":
        t = _pick(rng, ("checker", "image", "noise"), (1, 1, 1 if noise_ok else 0))
        tex = ("checker", _color(rng), _color(rng)) if t == "checker" else ("image", int(rng.integers(1, 1 << 30))) if t == "image" else \
              ("noise", float(rng.uniform(2.0, 6.0)), int(rng.integers(1, 1000)))
        bg = ("texture", tex, float(rng.uniform(0.8, 1.6)))
    if ax["background"].endswith("+env"):
        env = (32, 16)
    cam = (_f(np.array([rng.uniform(0.2, 0.6), rng.uniform(3.1, 3.5), rng.uniform(-12.9, -12.3)]) * S),
           _f(np.array([rng.uniform(-0.1, 0.3), rng.uniform(1.5, 1.9), rng.uniform(1.6, 2.2)]) * S), (0.0, 1.0, 0.0), float(rng.uniform(40.0, 44.0)), W / H,
           _pick(rng, (0.0, 0.06 * S)), float(rng.uniform(12.5, 14.0) * S))
    root = ("list",) if ax["root"] == "list" else ("bvh", int(rng.integers(1, 1000)))
    return (("axes", tuple((a, ax[a]) for a in AXIS_NAMES)), ("scale", S), ("camera", cam), ("shutter", shutter), ("root", root), ("items", tuple(items)),
            ("lights", tuple(lights)), ("area", tuple(area)), ("background", bg), ("env", env), ("pair", pair), ("rays", int(rng.integers(1, 1 << 30))))


def axes_of(rec):
    return dict(dict(rec)["axes"])


def digest(rec):
    return hashlib.sha256(repr(rec).encode()).hexdigest()[:24]


def _corpus():
    need, out, covered, i = all_pairs(), [], set(), 0
    count = {c: 0 for c in CELLS}
    while covered != need or min(count.values()) < MIN_SCENES:
        if i not in REPLACED and i not in VACUOUS:
            rec = recipe(i)
            p, c = pairs_of(axes_of(rec)), cells_of(rec)
            if p - covered or any(count[x] < MIN_SCENES for x in c):
                out.append(i)
                covered |= p
                for x in c:
                    count[x] += 1
        i += 1
    return tuple(out)


_CORPUS = []


def corpus():
    """the corpus' recipe indices (computed once)"""
    if not _CORPUS:
        _CORPUS.append(_corpus())
    return _CORPUS[0]


CORPUS_LENGTH = 62 # len(corpus()), written down: tests/test_soup_scenes.py holds it to the computed value


# ---- building both sides ------------------------------------------------------------------------------------------------------------------
class _Side:
    """one builder (rtamd.World or oracle.Scene) behind the calls build() makes; on the oracle it also records which object ids (the
    oracle's prim_id counts every hitable in builder order) belong to which group and material of the recipe"""

    def __init__(self, b, is_oracle):
        self.b, self.oracle = b, is_oracle
        self.last, self.ranges, self.ids = -1, [], {}
        self._tex, self._mat = {}, {}
        self.flux = {}

    def note(self, o, group, mat=None):
        self.ranges.append((self.last + 1, o, group, mat))
        self.last = max(self.last, o)
        self.ids.setdefault(group, []).append(o)
        return o

    def tex(self, t):
        if t not in self._tex:
            B = self.b
            if t[0] == "const":
                self._tex[t] = B.ConstantTexture(t[1])
            elif t[0] == "checker":
                self._tex[t] = B.CheckerTexture(B.ConstantTexture(t[1]), B.ConstantTexture(t[2]))
            elif t[0] == "image":
                self._tex[t] = B.ImageTexture(np.random.default_rng(t[1]).integers(0, 256, size=(5, 7, 3), dtype=np.uint8))
            else:
                self._tex[t] = B.NoiseTexture(t[1], t[2])
        return self._tex[t]

    def mat(self, m):
        if m not in self._mat:
            B = self.b
            if m[0] == "lambertian":
                self._mat[m] = B.Lambertian(self.tex(m[1]))
            elif m[0] == "metal":
                self._mat[m] = B.Metal(self.tex(m[1]), m[2])
            elif m[0] == "dielectric":
                self._mat[m] = B.Dielectric(m[1], self.tex(m[2]))
            else:
                self._mat[m] = B.DiffuseLight(self.tex(m[1]))
        return self._mat[m]

    def mesh(self, P, N, I, m, seed):
        return self.b.Mesh(P, N, I, self.mat(m), seed) if self.oracle else self.b.Mesh(P, N, I, self.mat(m), bvh_seed=seed)

    def obj(self, d, drop_medium):
        """the object of one description; None for a medium that is left out"""
        from conftest import scene_path
        from rtamd import shapes
        B, kind, group = self.b, d[0], d[1]
        if kind == "sphere":
            return self.note(B.Sphere(d[2], d[3], self.mat(d[4])), group, d[4])
        if kind == "rect":
            fn = (B.YZRectangle, B.XZRectangle, B.XYRectangle)[d[2]]
            return self.note(fn(d[3], d[4], d[5], self.mat(d[6])), group, d[6])
        if kind == "cube":
            return self.note(B.Cube(d[2], d[3], self.mat(d[4])), group, d[4])
        if kind == "msphere":
            return self.note(B.MovingSphere(d[2], d[3], 0.0, 1.0, d[4], self.mat(d[5])), group, d[5])
        if kind == "obj":
            m, bake = d[2], d[3]
            if bake is None and not self.oracle:
                return self.note(B.Mesh_load_obj(scene_path("cube.obj"), self.mat(m)), group, m)
            import oracle
            P, N, I = oracle.load_obj(scene_path("cube.obj"))
            if bake is not None:
                P = np.asarray(P) * bake[0] + np.asarray(bake[1])
            return self.note(self.mesh(P, N, I, m, 1), group, m)
        if kind == "torus":
            m, seed, bake = d[2], d[3], d[4]
            P, N, I = shapes.torus(12, 16)
            if bake is not None:
                P = P * bake[0] + np.asarray(bake[1])
            return self.note(self.mesh(P, N, I, m, seed), group, m)
        if kind == "tris":
            md = B.MeshData(np.asarray(d[2]), np.asarray(d[3]))
            nodes = [self.note(B.Triangle(md, a, b, c, self.mat(d[5])), group, d[5]) for a, b, c in d[4]]
            while len(nodes) > 1:                  # pairs, then pairs of pairs: BVHNode::construct by hand
                nodes = [self.note(B.BVHNode_construct(nodes[i], nodes[i + 1]), group) if i + 1 < len(nodes) else nodes[i] for i in range(0, len(nodes), 2)]
            return nodes[0]
        if kind == "medium":
            if drop_medium:
                return None
            boundary = self.obj(d[3], False)
            return self.note(B.ConstantMedium(d[2], boundary, B.Isotropic(self.tex(("const", d[4])))), group)
        if kind == "leaf":                         # BVHNode::new over one object: a node whose box is the object's
            child = self.obj(d[3], drop_medium)
            return self.note(B.BVHNode_new([child], d[2]) if self.oracle else B.BVHNode_new([child], bvh_seed=d[2]), group)
        if kind == "xf":
            child = self.obj(d[3], drop_medium)
            if child is None:
                return None
            for rot, sc, tr in d[2]:
                child = self.note(B.Transform(rot, sc, tr, child), group)
            return child
        if kind == "xzlight":
            if self.oracle:
                o = B.XZRectangle(d[2], d[3], d[4], B.DiffuseLight(B.ConstantTexture(d[5])))
            else:
                o = B.XZRectLight(d[2], d[3], d[4], d[5], 1.0)
            self.flux[o] = d[5]
            return self.note(o, group, ("light", ("const", d[5])))
        if kind == "spherelight":
            if self.oracle:
                o = B.Sphere(d[2], d[3], B.DiffuseLight(B.ConstantTexture(d[4])))
            else:
                o = B.SphereDiffuseLight(d[2], d[3], d[4], 1.0)
            self.flux[o] = d[4]
            return self.note(o, group, ("light", ("const", d[4])))
        raise KeyError(kind)

    def background(self, bg):
        B = self.b
        if bg[0] == "constant":
            B.set_background(1, color0=bg[1], scale=bg[2]) if self.oracle else B.set_background(color=bg[1], scale=bg[2])
        elif bg[0] == "gradient":
            B.set_background(2, color0=bg[1], color1=bg[2], scale=bg[3]) if self.oracle else B.set_background(gradient=(bg[1], bg[2]), scale=bg[3])
        else:
            B.set_background(3, texture=self.tex(bg[1]), scale=bg[2]) if self.oracle else B.set_background(texture=self.tex(bg[1]), scale=bg[2])


def _build_side(rec, side, drop_medium, close_shutter):
    r = dict(rec)
    B = side.b
    built = [side.obj(d, drop_medium) for d in r["items"]]
    ids = [o for o in built if o is not None]
    lights = [built[i] for i in r["lights"]]
    area = [built[i] for i in r["area"]]
    if side.oracle:
        B.set_root(B.HitableList(ids)) if r["root"][0] == "list" else B.World(ids, r["root"][1])
        if lights:
            B.set_lights(lights)
        if area:
            import light_scenes as ls
            ls.lower_area_lights(B, area)
    elif r["root"][0] == "list":
        if lights:
            B.set_lights(lights)
        if area:
            B.set_area_lights(area)
        B.set_root(B.HitableList(ids))
    else:
        B.new(ids, lights=lights, bvh_seed=r["root"][1], area_lights=area)
    if r["background"] is not None:
        side.background(r["background"])
    if r["env"] is not None:
        B.set_env_sampling(*r["env"]) if side.oracle else B.set_env_sampling(True, *r["env"])
    side.built = built
    return side


def build_oracle(rec, drop_medium=False, close_shutter=False):
    """-> the oracle's side (a _Side: .b is the oracle.Scene with camera and shutter set)"""
    import oracle
    r = dict(rec)
    side = _build_side(rec, _Side(oracle.Scene(), True), drop_medium, close_shutter)
    side.b.Camera(*r["camera"])
    if r["shutter"] is not None and not close_shutter:
        side.b.set_shutter(*r["shutter"])
    return side


def build_pair(rec):
    """-> (rtamd.World committed, rtamd.Camera, the oracle's _Side, render keywords of the product)"""
    import light_scenes as ls
    import rtamd
    r = dict(rec)
    w = _build_side(rec, _Side(ls.deferred_world(), False), False, False).b
    rtamd.World.commit(w)
    return w, ls._camera(r["camera"]), build_oracle(rec), (dict(shutter=r["shutter"]) if r["shutter"] is not None else {})


def build(rec):
    """-> (rtamd.World committed, rtamd.Camera, oracle.Scene, render keywords of the product)"""
    w, cam, side, kw = build_pair(rec)
    return w, cam, side.b, kw


# ---- test rays -----------------------------------------------------------------------------------------------------------------------------
def _secondary(rays, rec, seed):
    """tests/test_full_frames_gpu.py's secondary rays: from every primary hit a uniform direction in the hemisphere of the record's normal
    (even pixels) or the mirror reflection (odd pixels)"""
    n = rec[:, 5:8]
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(len(rays), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u = np.where((np.sum(u * n, axis=1) < 0.0)[:, None], -u, u)
    d = rays[:, 3:]
    m = d - 2.0 * np.sum(d * n, axis=1, keepdims=True) * n
    pix = np.arange(len(rays))
    out = np.concatenate([rec[:, 2:5], np.where((((pix % W) + (pix // W)) % 2 == 0)[:, None], u, m)], axis=1)
    return out[rec[:, 0] == 1.0]


def test_ray_parts(rec, side):
    """the scene's test rays as [(family, rays [n, 6])], from the oracle alone: the sample-0 camera rays, one secondary ray per primary hit, N_EXPLICIT rays
    from random points of the scene's volume towards its items and, for a coplanar pair, N_PAIR_RAYS rays aimed at the shared surface from either side
    of it (from inside the cubes too: two cubes share a face where only rays that travel inside them arrive)"""
    r = dict(rec)
    S = r["scale"]
    sc = side.b
    rays = sc.camera_rays(W, H, seed=SEED, sample=0).reshape(-1, 6)
    hit = hit_records(rec, side, rays)
    rng = np.random.default_rng(r["rays"])
    o = rng.uniform((-6.0, 0.2, -3.0), (6.0, 5.0, 7.0), (N_EXPLICIT, 3)) * S
    centres = [centre(d) for d in r["items"]]
    t = np.array([centres[k % len(centres)] for k in range(N_EXPLICIT)]) + rng.uniform(-0.9, 0.9, (N_EXPLICIT, 3)) * S
    d = t - o
    d[3::4] = -d[3::4]                              # every fourth one looks away from its item,
    d[3::4, 1] = np.abs(d[3::4, 1])                 # and upwards: most of these leave the scene
    t = o + d
    out = [("camera", rays), ("secondary", _secondary(rays, hit, r["rays"])), ("explicit", np.concatenate([o, t - o], axis=1))]
    if r["pair"] is not None:
        a, b = (d[3] if d[0] == "leaf" else d for d in (r["items"][r["pair"][0]], r["items"][r["pair"][1]]))
        if a[0] == "rect":
            a, b = b, a
        alo, ahi = np.array(a[2]), np.array(a[3])
        if b[0] == "rect":                         # points of the cube's face under the rectangle, seen from inside the cube and from in front of it
            tgt = np.concatenate([rng.uniform(alo[:2], ahi[:2], (N_PAIR_RAYS, 2)), np.full((N_PAIR_RAYS, 1), b[5])], axis=1)
            org = rng.uniform(alo, ahi, (N_PAIR_RAYS, 3))
            org[::2, 2] = alo[2] - rng.uniform(0.5, 3.0, (N_PAIR_RAYS + 1) // 2) * S
        else:                                      # points of the shared part of the face x = mid, from inside either cube
            blo, bhi = np.array(b[2]), np.array(b[3])
            lo, hi = np.maximum(alo[1:], blo[1:]), np.minimum(ahi[1:], bhi[1:])
            tgt = np.concatenate([np.full((N_PAIR_RAYS, 1), ahi[0]), rng.uniform(lo, hi, (N_PAIR_RAYS, 2))], axis=1)
            org = rng.uniform(alo, ahi, (N_PAIR_RAYS, 3))
            org[::2] = rng.uniform(blo, bhi, (N_PAIR_RAYS, 3))[::2]
        out.append(("pair", np.concatenate([org, tgt - org], axis=1)))
    return out


def test_rays(rec, side):
    """the scene's test rays [n, 6]: test_ray_parts, one after the other"""
    return np.ascontiguousarray(np.concatenate([a for _, a in test_ray_parts(rec, side)], axis=0))


def centre(d):
    """a point in the middle of an item, from its description"""
    kind = d[0]
    if kind in ("sphere", "msphere", "spherelight"):
        return np.array(d[2])
    if kind == "cube":
        return 0.5 * (np.array(d[2]) + np.array(d[3]))
    if kind in ("rect", "xzlight"):
        (a0, b0), (a1, b1), k = (d[3], d[4], d[5]) if kind == "rect" else (d[2], d[3], d[4])
        axis = d[2] if kind == "rect" else 1
        return np.insert(np.array([0.5 * (a0 + a1), 0.5 * (b0 + b1)]), axis, k)
    if kind in ("obj", "torus"):
        return np.array(d[-1][1])
    if kind == "tris":
        return np.mean(np.array(d[2][:5]), axis=0)
    if kind in ("medium", "leaf"):
        return centre(d[3])
    return np.array(d[2][-1][2])      # xf: where its outermost level moves it


RAY_TIME = 0.5


def ray_keys(n):
    return np.stack([np.full(n, SEED, dtype=np.uint64), np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)], axis=1)


def hit_records(rec, side, rays):
    """the oracle's closest-hit records [n, 12] of rays [n, 6]: hit_batch, or -- for a recipe with a medium or moving spheres, whose hit
    needs a random stream and a ray time -- walk() at RAY_TIME with the stream (SEED, row, 0), as the product's debug_walk is asked"""
    f = facts(rec)
    if f["media"] or f["moving"]:
        rays7 = np.concatenate([rays, np.full((len(rays), 1), RAY_TIME)], axis=1)
        return side.b.walk(rays7, ray_keys(len(rays)), t_min=T_MIN)[0]
    return side.b.hit_batch(rays, t_min=T_MIN)


def group_of(side, prim_ids):
    """the recipe group of each prim_id (the oracle's object id of the primitive that was hit)"""
    out = []
    for p in prim_ids:
        out.append(next((g for lo, hi, g, _ in side.ranges if lo <= p <= hi), None))
    return out


def material_of(side, prim_id):
    return next((m for lo, hi, _, m in side.ranges if lo <= prim_id <= hi), None)


def albedo(side, rays, hits):
    """[n, 3]: the texture value of the hit object's material at each hit (rays [n, 6], hits [n, 12] oracle records): the colour of a
    constant texture, else oracle.scatter's attenuation (a Lambertian) or emission (a light) at the record"""
    out = np.zeros((len(hits), 3))
    for j, h in enumerate(hits):
        m = material_of(side, int(h[11]))
        tex = m[2] if m[0] == "dielectric" else m[1]
        if tex[0] == "const":
            out[j] = tex[1]
        else:
            assert m[0] in ("lambertian", "light"), m
            s = side.b.scatter(side.mat(m), rays[j, :3], rays[j, 3:], h[2:5], h[5:8], h[8] != 0.0, uv=(h[9], h[10]))
            out[j] = s["attenuation"] if m[0] == "lambertian" else s["emitted"]
    return out


def expected_aov(side, aov_spp):
    """rt_render_aov restated over the oracle, as tests/test_denoise_gpu.py restates it: per pixel the hit records of the camera rays of
    samples 0 .. aov_spp - 1, summed in sample order and divided by the hits"""
    sums, hits = np.zeros((W * H, 7)), np.zeros(W * H)
    for s in range(aov_spp):
        rays = side.b.camera_rays(W, H, seed=SEED, sample=s).reshape(-1, 6)
        r = side.b.hit_batch(rays, t_min=T_MIN)
        hit = r[:, 0] != 0.0
        vals = np.zeros((len(r), 7))
        vals[:, 0:3] = r[:, 5:8]
        vals[:, 3] = r[:, 1]
        vals[hit, 4:7] = albedo(side, rays[hit], r[hit])
        sums[hit] += vals[hit]
        hits[hit] += 1.0
    out = np.zeros((W * H, 8))
    m = hits > 0
    out[m, :7] = sums[m] / hits[m][:, None]
    out[m, 7] = hits[m] / float(aov_spp)
    return out.reshape(H, W, 8)


def occlusion_rows(side, rays):
    """tests/ao_cases._rows: every ray with t_max = +inf, then the first EXACT_ROWS rays that hit with t_max = the oracle's own t, the
    double below it and the double above it, asked ray by ray -> (rays7 [m, 7], expected bool [m])"""
    inf = float("inf")
    rec = side.b.hit_batch(rays, T_MIN)
    rows, exp = [np.concatenate([rays, np.full((len(rays), 1), inf)], axis=1)], [rec[:, 0] != 0]
    for i in np.flatnonzero((rec[:, 0] != 0) & np.isfinite(rec[:, 1]) & (rec[:, 1] > T_MIN))[:EXACT_ROWS]:
        t = rec[i, 1]
        for tm in (t, np.nextafter(t, 0.0), np.nextafter(t, inf)):
            rows.append(np.concatenate([rays[i], [tm]])[None, :])
            exp.append(side.b.hit_batch(rays[i:i + 1], T_MIN, t_max=float(tm), n_workers=1)[:, 0] != 0)
    return np.ascontiguousarray(np.concatenate(rows, axis=0)), np.concatenate(exp)


def required_groups(rec):
    ax = axes_of(rec)
    out = [k for k in ("spheres", "cube", "small_mesh", "big_mesh", "tris") if ax[k]]
    return out + (["rects:xy", "rects:xz", "rects:yz"] if ax["rects"] else [])


# ---- the rules: what include/rtamd.h says every call does ----------------------------------------------------------------------------------
def _walk(d, fn):
    fn(d)
    if d[0] in ("xf", "medium", "leaf"):
        _walk(d[3], fn)


def _textures(rec):
    r = dict(rec)
    out = []

    def see(d):
        for x in d:
            if isinstance(x, tuple) and x and x[0] in ("lambertian", "metal", "dielectric", "light"):
                out.append(x[2] if x[0] == "dielectric" else x[1])
    for d in r["items"]:
        _walk(d, see)
    if r["background"] is not None and r["background"][0] == "texture":
        out.append(r["background"][1])
    return out


def facts(rec):
    """what the rules ask of a recipe, read from its description"""
    r = dict(rec)
    f = dict(media=False, media_xf=False, moving=False, nest=False, instances=0, f32_instance=False)

    def see(d):
        if d[0] == "medium":
            f["media"] = True
        elif d[0] == "msphere":
            f["moving"] = True
        elif d[0] == "xf":
            f["instances"] += 1                    # (a chain is refused by the rows about nested Transforms before its instances are counted)
            if len(d[2]) > 1:
                f["nest"] = True
            if d[3][0] == "medium":
                f["media_xf"] = True
            if len(d[2]) == 1 and d[3][0] in ("obj", "torus"):
                f["f32_instance"] = True           # cube.obj and shapes.torus hold f32 vertices
    for d in r["items"]:
        _walk(d, see)
    f["noise"] = any(t[0] == "noise" for t in _textures(rec))
    f["shutter"] = r["shutter"] is not None
    f["book2"] = f["moving"] or f["noise"] or f["shutter"]
    f["background"] = r["background"] is not None
    f["env"] = r["env"] is not None
    f["lights"] = len(r["lights"])
    f["area"] = len(r["area"])
    f["service"] = not f["media"] and not f["book2"] and not f["nest"] and f["f32_instance"] and 1 <= f["instances"] <= 64
    return f


# (entry points, condition on (facts, kernel, integrator), what the call does, the line of include/rtamd.h that says so and words of it).
# The first row that applies answers: for "render" that is the order include/rtamd.h gives with rt_render.
RULES = (
    ("render", lambda f, k, i: f["background"] and k in (5, 6), UNSUPPORTED, 298, "kernels 5 / 6 requested explicitly and rt_render_sppm* are RT_ERR_UNSUPPORTED for a scene with a"),
    ("render", lambda f, k, i: f["area"] and i == 1 and k in (5, 6), UNSUPPORTED, 374, "kernels 5 / 6 under integrator 1 and rt_render_sppm*"),
    ("render", lambda f, k, i: k in (5, 6) and f["media"], UNSUPPORTED, 213, "integrator 1, kernels 5 / 6, a medium inside a"),
    ("render", lambda f, k, i: k in (5, 6) and f["book2"], UNSUPPORTED, 179, "integrator 1 and kernels 5 / 6 are RT_ERR_UNSUPPORTED"),
    ("render", lambda f, k, i: k in (5, 6) and f["nest"], UNSUPPORTED, 227, "kernels 5 / 6 refuse it with RT_ERR_UNSUPPORTED"),
    ("render", lambda f, k, i: k == 5 and not f["service"], UNSUPPORTED, 93, "needs 1..64 instances, at least one of f32-vertex triangles"),
    ("render", lambda f, k, i: k == 6 and not f["service"], UNSUPPORTED, 95, "1..64 instances, at least one of f32-vertex triangles, as kernel 5"),
    ("render", lambda f, k, i: k == 2 and f["media_xf"], UNSUPPORTED, 228, "a ConstantMedium under a Transform, at any depth, renders through kernel 1 only"),
    ("render", lambda f, k, i: i == 1 and not f["lights"] and not f["area"] and not f["env"], ARG, 422, "integrator 1 on a scene without object lights, area lights and a sampled environment: RT_ERR_ARG"),
    ("render", lambda f, k, i: i == 1 and f["book2"], UNSUPPORTED, 423, "integrator 1 on a book-2 scene: RT_ERR_UNSUPPORTED"),
    ("render", lambda f, k, i: i == 1 and f["media"], UNSUPPORTED, 423, "integrator 1 on a scene with a ConstantMedium: RT_ERR_UNSUPPORTED"),
    ("render_aov", lambda f, k, i: f["media"] or f["moving"], UNSUPPORTED, 523, "Scenes with a ConstantMedium (the first hit needs the path's stream) or moving spheres (no ray time) are"),
    ("render_ao", lambda f, k, i: f["media"] or f["moving"], UNSUPPORTED, 612, "ConstantMedium or moving spheres, as rt_render_aov"),
    ("debug_hit", lambda f, k, i: f["media"] or f["moving"], UNSUPPORTED, 709, "a scene with moving spheres or a ConstantMedium"),
    ("debug_hit", lambda f, k, i: k in (5, 6) and not (f["f32_instance"] and not f["nest"]), UNSUPPORTED, 710, "kernels 5 / 6 on a scene without 1..64 instances"),
    ("debug_occluded", lambda f, k, i: f["media"] or f["moving"], UNSUPPORTED, 782, "scene with a ConstantMedium or moving spheres"),
    ("debug_walk", lambda f, k, i: k in (2, 3) and f["media_xf"], UNSUPPORTED, 770, "kernel 2 or 3 on a scene without an accel"),
    # rt_render_sppm: the first five rows in the order include/rtamd.h:433 gives (a background or area lights answer before the missing
    # object lights do); the kernel's own refusals come after the pre-pass and share one code
    ("render_sppm", lambda f, k, i: f["background"], UNSUPPORTED, 298, "rt_render_sppm* are RT_ERR_UNSUPPORTED for a scene with a"),
    ("render_sppm", lambda f, k, i: f["area"], UNSUPPORTED, 374, "rt_render_sppm* (the photon pass has no emitter for them) are RT_ERR_UNSUPPORTED"),
    ("render_sppm", lambda f, k, i: not f["lights"], ARG, 433, "a background, area lights (RT_ERR_UNSUPPORTED), a scene without object lights: RT_ERR_ARG, the book-2 kinds"),
    ("render_sppm", lambda f, k, i: f["moving"] or f["shutter"], UNSUPPORTED, 855, "RT_ERR_UNSUPPORTED (a background, area lights, moving spheres, noise"),
    ("render_sppm", lambda f, k, i: f["noise"], UNSUPPORTED, 856, "textures, a light inside a ConstantMedium), RT_ERR_ARG (no lights)"),
    ("render_sppm", lambda f, k, i: k == 5 and not f["service"], UNSUPPORTED, 93, "needs 1..64 instances, at least one of f32-vertex triangles"),
    ("render_sppm", lambda f, k, i: k == 2 and f["media_xf"], UNSUPPORTED, 228, "a ConstantMedium under a Transform, at any depth, renders through kernel 1 only"),
)
WITHHELD = "withheld"   # rt_render_sppm with kernel 6: not asked of any scene (reach_scenes.WITHHELD: the call hung on the device, cause not found)


def expected(rec, entry, kernel, integrator=0, no_lds=0):
    """FRAME, or the rt_status the call must fail with.  entry: "render", "render_aov", "render_ao", "debug_hit", "debug_occluded",
    "debug_walk", "render_sppm".  no_lds changes where the scene lives, never what a call does (rt_tuning: `how (never what) it renders`).
    "render_sppm" with kernel 6 is WITHHELD for every recipe: never a frame, and no test makes that call."""
    if entry == "render_sppm" and kernel == 6:
        return WITHHELD
    f = facts(rec)
    for entries, cond, result, _, _ in RULES:
        if entry in entries.split() and cond(f, kernel, integrator):
            return result
    return FRAME


def auto_kernel(rec, integrator, entry="render"):
    """the kernel the automatic choice (kernel 0) must report, in rt_params.kernel's words: 5 `when an instance's object-space BVH has >= 64
    nodes` (the torus under one Transform; cube.obj has fewer) and kernel 5 renders the call, else 2 `whenever the scene has a usable
    accel`, else 1; kernel 6 runs `by request only`.  entry: "render", or "render_sppm" (whose final pass chooses likewise)"""
    torus = []
    for d in dict(rec)["items"]:
        _walk(d, lambda x: torus.append(1) if x[0] == "xf" and len(x[2]) == 1 and x[3][0] == "torus" else None)
    if torus and expected(rec, entry, 5, integrator) == FRAME:
        return 5
    return 2 if expected(rec, entry, 2, integrator) == FRAME else 1


# What the corpus must reach beside the pairs: every cell of the render matrix, and every other entry point, gives a frame (records, rows)
# -- not a refusal -- on at least MIN_SCENES scenes; so does an automatic choice of kernel 5.
MIN_SCENES = 3
CELLS = tuple(("render", k, i) for k in (1, 2, 5, 6) for i in (0, 1)) + (("auto", 5, 0), ("debug_hit", 5, 0), ("debug_hit", 6, 0), ("debug_hit", 3, 0),
                                                                         ("debug_walk", 2, 0), ("debug_occluded", 2, 0), ("render_aov", 2, 0), ("render_ao", 2, 0))


def cells_of(rec):
    """the CELLS a recipe fills"""
    f = facts(rec)
    out = set()
    for entry, k, i in CELLS:
        if entry == "auto":
            ok = auto_kernel(rec, i) == k
        elif entry == "debug_walk":
            ok = (f["media"] or f["moving"]) and expected(rec, entry, k, i) == FRAME
        else:
            ok = expected(rec, entry, k, i) == FRAME
        if ok:
            out.add((entry, k, i))
    return out


def allowed_kernels(rec, integrator):
    """the kernels an automatic choice (kernel 0) may report for a recipe: those the rules let render it"""
    return {k for k in (1, 2, 5, 6) if expected(rec, "render", k, integrator) == FRAME}


# ---- SPPM on composed scenes (tests/test_soup_sppm_scenes.py without a device, tests/test_soup_sppm_gpu.py on one) --------------------------------------
# rt_render_sppm renders a recipe without a background, area lights, moving spheres, an open shutter and noise textures that has an object
# light (RULES).  SPPM_CORPUS walks the indices below SPPM_RANGE whose expected(rec, "render_sppm", 1) is FRAME, in increasing order, and keeps
# an index when its recipe shows a pair of sppm_axes values no kept recipe showed, or fills a cell of SPPM_CELLS that fewer than MIN_SCENES
# kept recipes fill; it ends when every pair that occurs among those indices (the ones passed over aside) has occurred and every cell is
# full.  It is written down here, so that importing this module draws no 4000 recipes; sppm_corpus() computes it and
# tests/test_soup_sppm_scenes.py holds the two equal.  No kernel 6: expected() answers WITHHELD for it.
SPPM_CFG = dict(iterations=3, photons_per_iter=20000, k_global=20, k_caustic=5)
SPPM_SPP = 2
SPPM_RANGE = 4000
SPPM_AXIS_NAMES = ("root",) + PRIMITIVE_AXES + ("depth", "special", "coplanar", "scale", "lights")
SPPM_CELLS = (("render_sppm", 1), ("render_sppm", 2), ("render_sppm", 5), ("auto", 5))
SPPM_REPLACED = {}   # index -> the measure-zero condition (RT_ERR_UNIT_ZERO) its recipe meets, shown from the oracle alone; at most two
# index -> the condition of tests/test_soup_sppm_scenes.py its recipe failed when the corpus was written
SPPM_VACUOUS = {94: "lit"}   # no specular surface: the caustic map stays empty, its radius^2 is 0 and the frame is NaN or black everywhere
SPPM_CORPUS = (2, 13, 173, 184, 203, 221, 225, 246, 250, 256, 319, 340, 364, 370, 393, 472, 484, 494, 515, 520, 532, 539, 584, 587, 716, 732, 781, 913,
               920, 1030, 1218, 1450)
SPPM_CORPUS_LENGTH = 32   # len(SPPM_CORPUS) == len(sppm_corpus()[0]), written down


def sppm_axes(rec):
    """the axis values the SPPM sub-corpus crosses: root, the six primitive axes, depth, special (none / medium / medium_xf: a medium under
    a Transform), coplanar, scale, and the kinds of the object lights (rect / sphere / both; none where the recipe has no object light)"""
    ax, f, r = axes_of(rec), facts(rec), dict(rec)
    out = {a: ax[a] for a in SPPM_AXIS_NAMES[:-1]}
    out["special"] = "medium_xf" if f["media_xf"] else "medium" if f["media"] else ax["special"]
    kinds = {r["items"][i][0] for i in r["lights"]}
    out["lights"] = "both" if len(kinds) == 2 else "rect" if kinds == {"xzlight"} else "sphere" if kinds else "none"
    return out


def sppm_pairs_of(rec):
    ax = sppm_axes(rec)
    return {((a, ax[a]), (b, ax[b])) for i, a in enumerate(SPPM_AXIS_NAMES) for b in SPPM_AXIS_NAMES[i + 1:]}


def sppm_cells(rec):
    """the SPPM_CELLS a recipe fills: ("render_sppm", k) where kernel k answers with a frame, ("auto", 5) where the automatic choice is kernel 5"""
    if expected(rec, "render_sppm", 1) != FRAME:
        return set()
    out = {("render_sppm", k) for k in (1, 2, 5) if expected(rec, "render_sppm", k) == FRAME}
    return out | ({("auto", 5)} if auto_kernel(rec, 0, "render_sppm") == 5 else set())


def sppm_eligible():
    """the indices below SPPM_RANGE that rt_render_sppm renders (through kernel 1), in increasing order (computed once)"""
    if not _SPPM:
        _SPPM.append(tuple(i for i in range(SPPM_RANGE) if expected(recipe(i), "render_sppm", 1) == FRAME))
    return _SPPM[0]


def sppm_corpus():
    """SPPM_CORPUS by its definition (computed once) -> (the kept indices, the pairs they must cover)"""
    if len(_SPPM) < 2:
        live = [i for i in sppm_eligible() if i not in SPPM_VACUOUS and i not in SPPM_REPLACED]
        pairs = {i: sppm_pairs_of(recipe(i)) for i in live}
        need = set().union(*pairs.values())
        out, covered, count = [], set(), {c: 0 for c in SPPM_CELLS}
        for i in live:
            if covered == need and min(count.values()) >= MIN_SCENES:
                break
            c = sppm_cells(recipe(i))
            if pairs[i] - covered or any(count[x] < MIN_SCENES for x in c):
                out.append(i)
                covered |= pairs[i]
                for x in c:
                    count[x] += 1
        _SPPM.append((tuple(out), need))
    return _SPPM[1]


_SPPM = []


def _medium_bounds(d, levels=()):
    """(centre, radius) of a sphere around every medium boundary in or under d, in world space.  A level p -> T + S (R p) takes the sphere
    (c, r) into the sphere (T, max(S) (|c| + r)) whatever R is"""
    out = []
    if d[0] == "medium":
        b = d[3]
        if b[0] == "sphere":
            c, rad = np.array(b[2]), float(b[3])
        else:
            assert b[0] == "cube", b[0]
            c, rad = 0.5 * (np.array(b[2]) + np.array(b[3])), 0.5 * float(np.linalg.norm(np.array(b[3]) - np.array(b[2])))
        for _, sc, tr in levels:
            c, rad = np.array(tr), max(abs(x) for x in sc) * (float(np.linalg.norm(c)) + rad)
        out.append((c, rad))
    elif d[0] == "xf":
        out += _medium_bounds(d[3], tuple(d[2]) + tuple(levels))
    elif d[0] == "leaf":
        out += _medium_bounds(d[3], levels)
    return out


def lights_clear_of_media(rec):
    """no object light of the recipe touches a sphere around any of its media, from the description alone: the least distance between a
    light's box and a medium's bounding sphere, in units of the recipe's scale (inf without a medium); > 0 is clear"""
    r = dict(rec)
    gap = float("inf")
    for i in r["lights"]:
        d = r["items"][i]
        if d[0] == "xzlight":
            lo, hi = np.array([d[2][0], d[4], d[2][1]]), np.array([d[3][0], d[4], d[3][1]])
        else:
            lo, hi = np.array(d[2]) - d[3], np.array(d[2]) + d[3]
        for item in r["items"]:
            for c, rad in _medium_bounds(item):
                gap = min(gap, (float(np.linalg.norm(np.maximum(np.maximum(lo - c, c - hi), 0.0))) - rad) / r["scale"])
    return gap


def build_oracle_sppm(rec):
    """build_oracle with every object light's flux and scale set: under SPPM a photon's power is flux x scale (build_oracle leaves both
    at the oracle's defaults, which path tracing never reads) -> the oracle's _Side"""
    side = build_oracle(rec)
    lights = [side.built[i] for i in dict(rec)["lights"]]
    side.b.set_lights(lights, flux=[side.flux[i] for i in lights], scale=[1.0] * len(lights))
    return side


def build_pair_sppm(rec):
    """-> (rtamd.World committed, rtamd.Camera, the oracle's _Side with flux and scale set)"""
    import light_scenes as ls
    import rtamd
    w = _build_side(rec, _Side(ls.deferred_world(), False), False, False).b
    rtamd.World.commit(w)
    return w, ls._camera(dict(rec)["camera"]), build_oracle_sppm(rec)
