"""One small world and explicit inputs for what a path does AFTER its hit (tests/test_shade_cases.py: the oracle alone against
independent references, no device; tests/test_shade_gpu.py: rt_debug_shade_device, rt_debug_light_sample_device and
rt_debug_light_pdf_device against the oracle, bit for bit).

Whole frames at random inputs reach the branches below with probability near zero: the checker's sign beside a zero of a sine (the device's
sin_sign_fast shortcut and its fallback), an ImageTexture at u, v on a texel boundary, the marble texture at coordinates beyond the range of
int, near_zero(normal + sample), Metal's dot == 0, the Dielectric's critical angle and its Schlick test against the draw, unit() of a
vector without a length, an object light seen from its surface, from inside, edge-on or through its exact corners, and the pdf sum over
three lights.  Every family here aims at one of them.

The world is ONE function of a builder (rtamd.World or oracle.Scene share the reference's constructor names).  Every family is a dict of
arrays -- rows [n, 17] and keys uint64 [n, 3] in the layout of rt_debug_shade_device (include/rtamd.h), or o_light [n, 4] / rays [n, 6] for
the light diagnostics -- and is a deterministic function of its name; the generators read the oracle's side only."""
import math
import struct

import numpy as np

PI = math.pi
IMG_SIZES = ((1, 1), (3, 2), (7, 5), (255, 1), (32, 16))          # (w, h): none but the last a power of two
FUZZ = (0.0, 0.3, 1.0)
IRS = (1.5, 1.0 / 1.5, 1.0, 2.4)
CHECK_COLORS = ((0.1, 0.2, 0.3), (0.9, 0.8, 0.7))                # CheckerTexture's .0 (sines < 0) and .1
NOISE_SCALE, NOISE_SEED = 4.0, 11
# the object lights, in list order: sphere, XZ rectangle, sphere -- all three on the ray from the origin straight up
LIGHT0 = ((0.0, 3.0, 0.0), 0.5)
LIGHT1 = ((-2.0, -1.5), (1.0, 2.5), 8.0)
LIGHT2 = ((0.25, 5.0, 0.125), 0.75)
CAMERA = ((0.0, 2.0, -10.0), (0.0, 2.0, 0.0), (0.0, 1.0, 0.0), 50.0, 1.0, 0.0, 10.0)
PERLIN_KEY = 0x243F6A8885A308D3


def is_oracle(B):
    return not hasattr(B, "XZRectLight")


def images():
    rng = np.random.default_rng(77)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for w, h in IMG_SIZES]


def build(B, noise=True):
    """-> (items, lights, ids): ids maps a material's name to its index.  noise=False leaves the marble out (a scene with a noise texture
    renders with integrator 0 only)"""
    ids = {}
    const = B.ConstantTexture((0.2, 0.5, 0.8))
    checker = B.CheckerTexture(B.ConstantTexture(CHECK_COLORS[0]), B.ConstantTexture(CHECK_COLORS[1]))
    ids["lamb"] = B.Lambertian(const)
    ids["lamb_checker"] = B.Lambertian(checker)
    for k, img in enumerate(images()):
        ids["lamb_image%d" % k] = B.Lambertian(B.ImageTexture(img))
    ids["light"] = B.DiffuseLight(B.ConstantTexture((5.0, 4.0, 3.0)))
    ids["light_checker"] = B.DiffuseLight(checker)
    for f in FUZZ:
        ids["metal%g" % f] = B.Metal(B.ConstantTexture((0.8, 0.7, 0.6)), f)
    for k, ir in enumerate(IRS):
        ids["glass%d" % k] = B.Dielectric(ir, B.ConstantTexture((1.0, 0.95, 0.9)))
    ids["iso"] = B.Isotropic(const)
    if noise:
        ids["lamb_noise"] = B.Lambertian(B.NoiseTexture(NOISE_SCALE, NOISE_SEED))
    lights = [B.Sphere(LIGHT0[0], LIGHT0[1], ids["light"]), B.XZRectangle(LIGHT1[0], LIGHT1[1], LIGHT1[2], ids["light"]),
              B.Sphere(LIGHT2[0], LIGHT2[1], ids["light_checker"])]
    items = list(lights) + [B.XZRectangle((-8.0, -8.0), (8.0, 8.0), 0.0, ids["lamb_checker"])]
    names = [n for n in ids if n not in ("light", "light_checker", "lamb_checker")]
    for k, n in enumerate(names):       # one small sphere per material, in two rows above the floor
        items.append(B.Sphere((-4.5 + 1.3 * (k % 8), 0.6 + 1.5 * (k // 8), 1.0 - 1.0 * (k // 8)), 0.6, ids[n]))
    return items, lights, ids


_PAIRS = {}


def oracle_scene(noise=True):
    import oracle
    if noise not in _PAIRS:
        o = oracle.Scene()
        items, lights, ids = build(o, noise)
        o.World(items, 3)
        o.set_lights(lights)
        o.Camera(*CAMERA)
        _PAIRS[noise] = (o, ids)
    return _PAIRS[noise]


def product_world(noise=True):
    """-> (rtamd.World committed, rtamd.Camera, ids)"""
    import rtamd
    w = rtamd.World()
    items, lights, ids = build(w, noise)
    w.new(items, lights=lights, bvh_seed=3)
    assert ids == oracle_scene(noise)[1]
    f, t, up, vfov, asp, ap, fd = CAMERA
    return w, rtamd.Camera((f, t), up, vfov, asp, ap, fd), ids


# ---- doubles -----------------------------------------------------------------------------------------------------------------------------
def ulps(x, k):
    """the double k steps from x in the order of the reals (k < 0: below)"""
    b = struct.unpack("<q", struct.pack("<d", float(x)))[0]
    i = b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)
    i += k
    b = i if i >= 0 else (-i) | (1 << 63)
    return struct.unpack("<d", struct.pack("<Q", b & 0xFFFFFFFFFFFFFFFF))[0]


def unit(v):
    """Vec3::unit as the device and the oracle compute it: x / sqrt(x x + y y + z z)"""
    x, y, z = (float(c) for c in v)
    l = math.sqrt(x * x + y * y + z * z)
    return np.array([x / l, y / l, z / l])


def _rows(mat, mix, ro, rd, p, n, ff, u=0.5, v=0.5):
    return [float(mat), float(mix)] + [float(c) for c in ro] + [float(c) for c in rd] + [float(c) for c in p] + [float(c) for c in n] + [float(ff), float(u), float(v)]


def _family(rows, keys, **extra):
    out = dict(rows=np.array(rows, dtype=np.float64).reshape(-1, 17), keys=np.array(keys, dtype=np.uint64).reshape(-1, 3))
    assert len(out["rows"]) == len(out["keys"]) and 0 < len(out["rows"]) < 6000
    out.update(extra)
    return out


UP = (0.0, 1.0, 0.0)
DOWN_RAY = ((0.0, 1.0, 0.0), (0.3, -1.0, 0.2))


# ---- textures ----------------------------------------------------------------------------------------------------------------------------
def checker_values():
    """the coordinates x whose 10 x lies at, beside and around a zero of the sine, and the ones no sine has a sign for"""
    xs = []
    for k in list(range(-40, 41)) + [1000, 26000, -26000, 82353, 82354, 82355, 10 ** 6, 10 ** 9]:
        x0 = float(k) * PI / 10.0
        xs.append(x0)
        xs += [ulps(x0, d) for d in (-50, -2, -1, 1, 2, 50)]
        # 1e-9 of the device's margin is in units of 10 x / pi: pi * 1e-10 = 3.14e-10 in x
        xs += [x0 + s * e for e in (1e-12, 1e-11, 1e-10, 3.1e-10, 3.2e-10, 1e-9) for s in (-1.0, 1.0)]
    special = [0.0, -0.0, 5e-324, -5e-324, 1e-200, -1e-200, 1e300, math.inf, -math.inf, math.nan]
    return xs, special


def checker():
    _, ids = oracle_scene()
    xs, special = checker_values()
    g1, g2 = 0.123, -0.2                                  # sin(1.23) > 0, sin(-2) < 0
    pts = []
    for x in xs + special:
        pts += [(x, g1, g2), (g1, g2, x), (x, x, x)]
    rows = [_rows(ids["lamb_checker"], 0, DOWN_RAY[0], DOWN_RAY[1], p, UP, 1) for p in pts]
    return _family(rows, [(1, i % 7, 0) for i in range(len(rows))], points=np.array(pts))


def image_uv(w, h):
    def axis(n):
        vals = [0.0, -0.0, 1.0, ulps(1.0, -1), ulps(1.0, 1), -0.25, -1e-300, 2.0, math.nan, math.inf, -math.inf, 5e-324]
        for k in range(n + 1):
            q = float(k) / float(n)
            vals += [q, ulps(q, -1), ulps(q, 1)]
        return vals
    U, V = axis(w), axis(h)
    return [(u, V[i % len(V)]) for i, u in enumerate(U)] + [(U[(3 * j + 1) % len(U)], v) for j, v in enumerate(V)]


def image():
    _, ids = oracle_scene()
    rows, tex = [], []
    for k, (w, h) in enumerate(IMG_SIZES):
        for u, v in image_uv(w, h):
            rows.append(_rows(ids["lamb_image%d" % k], 0, DOWN_RAY[0], DOWN_RAY[1], (0.1, 0.2, 0.3), UP, 1, u, v))
            tex.append(k)
    return _family(rows, [(2, i % 5, 1) for i in range(len(rows))], tex=np.array(tex))


def noise():
    _, ids = oracle_scene()
    rng = np.random.default_rng(31)
    lattice = [-3.0, -2.5, -1.0, -0.5, 0.0, -0.0, 0.5, 1.0, 2.5, 255.0, 255.5, 256.0, -255.5, -256.0, 1e-300, -1e-300]
    pts = [tuple(rng.choice(lattice, 3)) for _ in range(64)]
    pts += [(0.37, -1.81, 2.44), (-17.25, 3.5, 0.125)]
    g = (0.3, 0.7)
    for k in range(20, 36):
        for s in (1.0, -1.0):
            x = s * (2.0 ** k + 0.5)
            pts += [(x, g[0], g[1]), (g[0], x, g[1]), (g[0], g[1], x)]      # the last: NOISE_SCALE z is beyond rtamd-sin-1's range
            m = s * (2.0 ** k + float((37 * k) % 256) + 0.25)                # 2^k itself has index 0: these have every other one
            pts += [(m, g[0], g[1]), (g[0], m, g[1]), (m, -m, 0.7)]
    pts += [(2.0 ** 31 + 0.5,) * 3, (-(2.0 ** 33) - 0.5,) * 3, (2.0 ** 52 + 1.0, 0.3, 0.7), (2.0 ** 60, -(2.0 ** 70), 1e300), (1e18, 0.25, -1e18)]
    pts += [(math.inf, 0.3, 0.7), (0.3, -math.inf, 0.7), (0.3, 0.7, math.nan), (math.nan, math.inf, -math.inf)]
    rows = [_rows(ids["lamb_noise"], 0, DOWN_RAY[0], DOWN_RAY[1], p, UP, 1) for p in pts]
    return _family(rows, [(3, i % 3, 2) for i in range(len(rows))], points=np.array(pts))


# ---- materials ---------------------------------------------------------------------------------------------------------------------------
def sphere_sample(key):
    import oracle
    return oracle.sample_helper(0, key=tuple(int(k) for k in key))


NEAR_ZERO_OFFSETS = (0.5e-8, 0.99e-8, 1.01e-8, 2e-8)


def lambertian(mix=0, p=(0.0, 0.0, 0.0)):
    """normal = -unit(sample) exactly, and beside it: normal + unit(sample) is zero, below near_zero's 1e-8 on every axis, or above it on one"""
    _, ids = oracle_scene()
    rows, keys = [], []
    for i in range(32):
        key = (11, i, i % 3)
        n0 = -unit(sphere_sample(key))
        normals = [n0]
        for ax in range(3):
            for off in NEAR_ZERO_OFFSETS:
                n = n0.copy()
                n[ax] += off if (i + ax) % 2 else -off
                normals.append(n)
        for j, n in enumerate(normals):
            rows.append(_rows(ids["lamb"] if i % 2 else ids["light"], mix, DOWN_RAY[0], DOWN_RAY[1], p, n, (i + j) % 2))
            keys.append(key)
    return _family(rows, keys)


def metal():
    _, ids = oracle_scene()
    rows, keys, tag = [], [], []
    for i in range(16):
        key = (13, i, 5)
        rs = sphere_sample(key)
        n = (-rs[1], rs[0], 0.0)                         # dot(rs, n) == 0 exactly; (0, 0, 1) is perpendicular to it as well
        for f in FUZZ:
            m = ids["metal%g" % f]
            for name, length in (("len0", 0.0), ("len5e-324", 5e-324), ("len1e-200", 1e-200), ("len1", 1.0), ("len1e200", 1e200)):
                rows.append(_rows(m, 0, (0.0, 0.0, -1.0), (0.0, 0.0, length), (0.0, 0.0, 0.0), n, 1))
                tag.append(name)
            for a in (-2.0 ** -52, 2.0 ** -52):           # tilted by one ulp of 1 along the normal
                rows.append(_rows(m, 0, (0.0, 0.0, -1.0), (a * n[0], a * n[1], 1.0), (0.0, 0.0, 0.0), n, 1))
                tag.append("tilt")
            rows.append(_rows(m, 0, (0.0, 3.0, 0.0), (0.3, -0.5, -1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 1))
            rows.append(_rows(m, 0, (0.0, 3.0, 0.0), (0.3, -0.5, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0))
            tag += ["generic", "generic"]
            keys += [key] * 9
    return _family(rows, keys, tag=np.array(tag))


def _glass_row(ids, k, ff, t, length=1.0, key=(17, 0, 0)):
    """incidence with tan(angle) = t onto the normal (0, 1, 0)"""
    return _rows(ids["glass%d" % k], 0, (0.0, 1.0, 0.0), (t * length, -1.0 * length, 0.0), (0.0, 0.0, 0.0), UP, ff)


def _bisect(pred, lo, hi):
    """doubles lo < hi with pred(lo) != pred(hi) -> the adjacent pair where pred flips"""
    a, b = pred(lo), pred(hi)
    assert a != b
    while ulps(lo, 1) < hi:
        mid = lo + (hi - lo) * 0.5
        if mid <= lo or mid >= hi:
            mid = ulps(lo, 1)
        if pred(mid) == a:
            lo = mid
        else:
            hi = mid
    return lo, hi


def dielectric():
    o, ids = oracle_scene()
    rows, keys, tag = [], [], []

    def add(row, key, what):
        rows.append(row)
        keys.append(key)
        tag.append(what)
    rng = np.random.default_rng(19)
    over = []                                            # unit directions whose own dot product rounds above 1
    while len(over) < 4:
        d = rng.normal(size=3)
        u = unit(d)
        if u[0] * u[0] + u[1] * u[1] + u[2] * u[2] > 1.0:
            over.append((d, u))
    for k in range(len(IRS)):
        for ff in (1, 0):
            key = (17, k, ff)
            add(_glass_row(ids, k, ff, 0.0), key, "normal")
            add(_glass_row(ids, k, ff, 0.0, 1e-3), key, "normal")
            for d, u in over:
                add(_rows(ids["glass%d" % k], 0, (0.0, 1.0, 0.0), d, (0.0, 0.0, 0.0), -u, ff), key, "over1")
            add(_rows(ids["glass%d" % k], 0, (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), UP, ff), key, "cos0")
            add(_rows(ids["glass%d" % k], 0, (0.0, 1.0, 0.0), (0.0, 0.0, -3.0), (0.0, 0.0, 0.0), UP, ff), key, "cos0")
            ratio = (1.0 / IRS[k]) if ff else IRS[k]
            if ratio > 1.0:                              # the critical angle: total reflection consumes no draw
                def total(t):
                    return int(o.shade([_glass_row(ids, k, ff, t)], [key])[1][0]) == 0
                lo, hi = _bisect(total, 0.0, 10.0)
                for j in range(16):
                    add(_glass_row(ids, k, ff, ulps(lo, -j)), key, "critical")
                    add(_glass_row(ids, k, ff, ulps(hi, j)), key, "critical")
    n_schlick, i = 0, 0
    while n_schlick < 8:                                 # Schlick's reflectance against the draw, refraction possible (ir 1.5 from outside)
        key = (23, i, 1)
        i += 1

        def reflects(t):
            return o.shade([_glass_row(ids, 0, 1, t)], [key])[0][0, 3] > 0.0
        if reflects(0.0) or not reflects(1e4):
            continue
        lo, hi = _bisect(reflects, 0.0, 1e4)
        for j in range(8):
            add(_glass_row(ids, 0, 1, ulps(lo, -j)), key, "schlick")
            add(_glass_row(ids, 0, 1, ulps(hi, j)), key, "schlick")
        n_schlick += 1
    return _family(rows, keys, tag=np.array(tag))


def isotropic():
    _, ids = oracle_scene()
    rows = [_rows(ids["iso"], i % 2, DOWN_RAY[0], DOWN_RAY[1], (0.5, 1.0, -0.5), UP, i % 2) for i in range(8)]
    return _family(rows, [(29, i, 4) for i in range(8)])


# ---- object lights -----------------------------------------------------------------------------------------------------------------------
def basis_switch_origins():
    """origins from which unit(centre - o).x of light 0 is 0.9, the double below and the double above, on both sides"""
    c = np.array(LIGHT0[0])
    targets = {ulps(0.9, -1): None, 0.9: None, ulps(0.9, 1): None}
    out = []
    for sign in (1.0, -1.0):
        found = dict(targets)
        for k in range(-200, 201):
            o = np.array([-sign * ulps(1.8, k), c[1] - 2.0 * math.sqrt(1.0 - 0.81), c[2]])
            wx = abs(unit(c - o)[0])
            if wx in found and found[wx] is None:
                found[wx] = o
        out += [(wx, o) for wx, o in found.items()]
    return out


def light_origins():
    """-> [(origin, light index, what)]"""
    rng = np.random.default_rng(37)
    out = []
    for li, (c, r) in ((0, LIGHT0), (2, LIGHT2)):
        c = np.array(c)
        dirs = [np.array(d) for d in ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0))] + [unit(rng.normal(size=3)) for _ in range(3)]
        for d in dirs:
            out += [(c + r * d, li, "surface"), (c + r * (1.0 + 1e-12) * d, li, "surface"), (c + r * (1.0 - 1e-12) * d, li, "surface"),
                    (c + 0.3 * r * d, li, "inside"), (c + 1e8 * r * d, li, "far"), (c + 1e9 * r * d, li, "far"), (c + 4.0 * r * d, li, "generic")]
        out.append((c, li, "centre"))
    for wx, o in basis_switch_origins():
        if o is not None:
            out.append((o, 0, "basis"))
    (x0, z0), (x1, z1), y = LIGHT1
    for o in ((0.0, y, 0.0), (5.0, y, 0.0), (0.0, 2.0, 0.0), (0.3, 1.0, -0.2), (0.0, y - 0.0005, 0.5), (0.0, y + 0.0005, 0.5), (0.0, y + 1.0, 0.0), (x0, y - 3.0, z1)):
        out.append((np.array(o), 1, "rect"))
    return out


def light_samples():
    rows, keys, tag = [], [], []
    for j, (o, li, what) in enumerate(light_origins()):
        for s in range(3):
            rows.append([float(o[0]), float(o[1]), float(o[2]), float(li)])
            keys.append((41, j, s))
            tag.append(what)
    return dict(o_light=np.array(rows), keys=np.array(keys, dtype=np.uint64), tag=np.array(tag))


def edge_rays():
    """rays through the rectangle light's corners and edge midpoints exactly, one ulp inside and one ulp outside; every one at three lengths"""
    (x0, z0), (x1, z1), y = LIGHT1
    xm, zm = 0.5 * (x0 + x1), 0.5 * (z0 + z1)
    rays = []
    for o in ((0.0, 2.0, 0.0), (0.25, y - 4.0, 0.5)):      # (8 - o.y) / d.y == 1 exactly, so the hit point is o + d
        for tx, tz in ((x0, z0), (x0, z1), (x1, z0), (x1, z1), (x0, zm), (x1, zm), (xm, z0), (xm, z1)):
            d = (tx - o[0], y - o[1], tz - o[2])
            for kx, kz in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
                dd = (ulps(d[0], kx), d[1], ulps(d[2], kz))
                for s in (1.0, 1e-150, 1e150):
                    rays.append(list(o) + [c * s for c in dd])
    return np.array(rays)


def light_pdf_rays():
    """every direction the sample family produced, from its own origin, then the edge rays; own = the light that produced a row's direction (-1: none)"""
    o, _ = oracle_scene()
    fam = light_samples()
    out, _ = o.light_sample(fam["o_light"], fam["keys"])
    ok = out[:, 3] == 0.0
    sampled = np.concatenate([fam["o_light"][ok, :3], out[ok, :3]], axis=1)
    edges = edge_rays()
    own = np.concatenate([fam["o_light"][ok, 3].astype(int), np.full(len(edges), -1)])
    return dict(rays=np.concatenate([sampled, edges]), own=own)


def mixture():
    """the mixture step after a Diffuse scatter: the Lambertian family with the flag set, normals opposite to the lights, and a cosine of
    exactly 0 with and without a light in the direction"""
    _, ids = oracle_scene()
    base = lambertian(mix=1)
    rows, keys, tag = [list(r) for r in base["rows"]], [tuple(k) for k in base["keys"]], ["near_zero"] * len(base["rows"])
    for i in range(96):
        key = (43, i, 0)
        rows.append(_rows(ids["lamb"], 1, DOWN_RAY[0], DOWN_RAY[1], (0.0, 0.0, 0.0), UP, 1))
        rows.append(_rows(ids["lamb"], 1, DOWN_RAY[0], DOWN_RAY[1], (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), 1))
        keys += [key, key]
        tag += ["up", "opposite"]
    for i in range(48):                                  # normal + unit(sample) = (0, u.y, u.z), perpendicular to the normal (-u.x, 0, 0): cosine 0
        key = (47, i, 0)
        u = unit(sphere_sample(key))
        for p in ((0.0, 0.0, 0.0), (0.0, 7.0, 0.5)):       # the second lies right under the rectangle light
            rows.append(_rows(ids["lamb"], 1, DOWN_RAY[0], DOWN_RAY[1], p, (-u[0], 0.0, 0.0), 1))
            keys.append(key)
            tag.append("cos0")
    for i in range(16):                                  # in the rectangle light's plane: its samples are perpendicular to the normal, and t = 0 / 0
        rows.append(_rows(ids["lamb"], 1, DOWN_RAY[0], DOWN_RAY[1], (0.5 * i - 4.0, LIGHT1[2], 0.25), UP, 1))
        keys.append((53, i, 0))
        tag.append("in_plane")
    return _family(rows, keys, tag=np.array(tag))


SHADE_FAMILIES = dict(checker=checker, image=image, noise=noise, lambertian=lambertian, metal=metal, dielectric=dielectric, isotropic=isotropic,
                      mixture=mixture)
_CACHE = {}


def family(name):
    """the family `name` of SHADE_FAMILIES, "light_samples" or "light_pdf_rays", built once"""
    if name not in _CACHE:
        fn = SHADE_FAMILIES.get(name) or dict(light_samples=light_samples, light_pdf_rays=light_pdf_rays)[name]
        _CACHE[name] = fn()
    return _CACHE[name]


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def perlin_tables(seed):
    """a noise texture's tables from the stream (seed, PERLIN_KEY, 0): 256 unit vectors of three gen_range(-1, 1), then three permutations
    shuffled from the top by (u32 * (i + 1)) >> 32"""
    import oracle
    s = oracle.rng_u64(seed, PERLIN_KEY, 0, 768 + 3 * 255)
    vec = []
    for i in range(256):
        c = [(struct.unpack("<d", struct.pack("<Q", (1023 << 52) | (s[3 * i + a] >> 12)))[0] - 1.0) * 2.0 + -1.0 for a in range(3)]
        vec.append(unit(c))
    perm, at = [], 768
    for a in range(3):
        p = list(range(256))
        for i in range(255, 0, -1):
            t = ((s[at] >> 32) * (i + 1)) >> 32
            at += 1
            p[i], p[t] = p[t], p[i]
        perm.append(p)
    return vec, perm


def lattice_index(x):
    """the rule include/rtamd.h pins: floor(x) mod 256 of the mathematical integer for a finite x, 0 for a non-finite one"""
    return (math.floor(x) % 256) if math.isfinite(x) else 0


def marble(vec, perm, scale, p, det_sin):
    """noise_texture::value restated with Python integers for the lattice index"""
    def noise(q):
        f = [float(math.floor(c)) if math.isfinite(c) else c for c in q]
        u, v, w = (q[a] - f[a] for a in range(3))
        i, j, k = (lattice_index(c) for c in q)
        uu, vv, ww = u * u * (3.0 - 2.0 * u), v * v * (3.0 - 2.0 * v), w * w * (3.0 - 2.0 * w)
        acc = 0.0
        for di in range(2):
            for dj in range(2):
                for dk in range(2):
                    c = vec[perm[0][(i + di) & 255] ^ perm[1][(j + dj) & 255] ^ perm[2][(k + dk) & 255]]
                    wx, wy, wz = u - di, v - dj, w - dk
                    acc += (di * uu + (1 - di) * (1.0 - uu)) * (dj * vv + (1 - dj) * (1.0 - vv)) * (dk * ww + (1 - dk) * (1.0 - ww)) * (c[0] * wx + c[1] * wy + c[2] * wz)
        return acc
    acc, weight, q = 0.0, 1.0, [float(c) for c in p]
    for _ in range(7):
        acc += weight * noise(q)
        weight *= 0.5
        q = [c * 2.0 for c in q]
    return 0.5 * (1.0 + det_sin(scale * float(p[2]) + 10.0 * abs(acc)))


def same(a, b):
    """bit for bit, a NaN equal to any NaN (x86 and the GPU make different default NaNs); -0.0 differs from 0.0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))
