"""Explicit rays -- origin, direction, ray time -- with a random stream each, aimed at the two parts of the traversal that only whole
frames reached before: the media walk (traverse2_media and traverse<.., MEDIA>) and moving spheres (the per-lane ray time).
tests/test_walk_cases.py: the oracle against the plain restatement of tests/walk_ref.py, without a device, and the conditions that keep a
family aimed at what it is for; tests/test_walk_gpu.py: rt_debug_walk_device against the oracle, bit for bit.

A scene is a description -- nested tuples, see walk_ref.py, plus ("xform", rotate, scale, translate, obj), ("nest", levels, obj) and
("mesh",) for cube.obj -- built once for either builder (rtamd.World or oracle.Scene share the reference's constructor names).  A case is
dict(name, items, root, build, rays [n, 7], keys uint64 [n, 3], t_min) and a deterministic function of its name; root is "list" (a
HitableList in the order of items: the reference then has no box of its own around anything, and program order is list order) or
("bvh", seed) (World::new).  Scenes have at most 64 objects, batches at most 4096 rows and never a multiple of 64."""
import math
import os
import zlib

import numpy as np

SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")
MEDIA_FAMILIES = ("row_of_fogs", "densities", "coincident", "origins", "second_query", "boundaries", "bvh_roots", "nested")
MOTION_FAMILIES = ("sweep", "lanes", "static_twin", "fog_and_motion")
FAMILIES = MEDIA_FAMILIES + MOTION_FAMILIES
ORDERS = ("surfaces_first", "surfaces_last", "interleaved", "ascending", "descending", "shuffled")
LANE_TIMES = (0.0, 0.25, 0.5, 0.75, 1.0, 0.1, 0.9)


def is_oracle(B):
    return not hasattr(B, "XZRectLight")


# ---- building ----------------------------------------------------------------------------------------------------------------------------
def _make(B, d, mats):
    k = d[0]
    if k == "sphere":
        o = B.Sphere(d[1], d[2], mats[0])
    elif k == "msphere":
        o = B.MovingSphere(d[1], d[2], d[3], d[4], d[5], mats[0])
    elif k == "rect":
        ctor = (B.YZRectangle, B.XZRectangle, B.XYRectangle)[d[1]]
        o = ctor((d[2], d[3]), (d[4], d[5]), d[6], mats[0])
    elif k == "cube":
        o = B.Cube(d[1], d[2], mats[0])
    elif k == "list":
        o = B.HitableList([_make(B, x, mats) for x in d[1]])
    elif k == "medium":
        o = B.ConstantMedium(d[1], _make(B, d[2], mats), mats[1])
    elif k == "xform":
        o = B.Transform(d[1], d[2], d[3], _make(B, d[4], mats))
    elif k == "nest":
        o = _make(B, d[2], mats)
        for rot, sc, tr in d[1]:
            o = B.Transform(rot, sc, tr, o)
    elif k == "mesh":
        import oracle
        P, N, I = oracle.load_obj(os.path.join(SCENES, "cube.obj"))
        o = B.Mesh(P, N, I, mats[0], 5) if is_oracle(B) else B.Mesh(P, N, I, mats[0], bvh_seed=5)
    else:
        raise ValueError(k)
    return o


def build_scene(B, items, root):
    """-> (B rooted -- and committed, for the product --, owners): owners[k] = the object ids created for items[k], to which the oracle's
    prim_id of a hit on that item belongs"""
    mats = (B.Lambertian(B.ConstantTexture((0.6, 0.5, 0.4))), B.Isotropic(B.ConstantTexture((0.8, 0.8, 0.9))))
    ids, owners, last = [], [], -1
    for k, d in enumerate(items):
        same = [j for j in range(k) if items[j] is d]          # the same description object listed twice is ONE object of the scene
        if same:
            ids.append(ids[same[0]])
            owners.append(owners[same[0]])
            continue
        ids.append(_make(B, d, mats))
        owners.append(set(range(last + 1, ids[-1] + 1)))
        last = ids[-1]
    if root == "list":
        B.set_root(B.HitableList(ids))
    elif is_oracle(B):
        B.World(ids, root[1])
    else:
        B.new(ids, bvh_seed=root[1])
    return B, owners


def scaled(d, s):
    """the description with every length multiplied by s and every density divided by it"""
    k = d[0]
    v = lambda p: tuple(float(x) * s for x in p)
    if k == "sphere":
        return ("sphere", v(d[1]), d[2] * s)
    if k == "msphere":
        return ("msphere", v(d[1]), v(d[2]), d[3], d[4], d[5] * s)
    if k == "rect":
        return ("rect", d[1]) + tuple(float(x) * s for x in d[2:7])
    if k == "cube":
        return ("cube", v(d[1]), v(d[2]))
    if k == "list":
        return ("list", [scaled(x, s) for x in d[1]])
    if k == "medium":
        return ("medium", d[1] / s, scaled(d[2], s))
    if k == "xform":
        return ("xform", d[1], d[2], v(d[3]), scaled(d[4], s))
    if k == "mesh":                     # cube.obj has one size: a scaling Transform around it (none at scale 1)
        return d if s == 1.0 else ("xform", (0.0, 0.0, 0.0), (s, s, s), (0.0, 0.0, 0.0), d)
    raise ValueError("scaled(%s)" % k)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _case(name, items, root, o, d, time, t_min=1e-3, **meta):
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n = len(o)
    time = np.broadcast_to(np.asarray(time, dtype=np.float64), (n,))
    rays = np.concatenate([o, d, time[:, None]], axis=1)
    if n % 64 == 0:
        rays = rays[:-1]
        n -= 1
    assert 0 < n <= 4096 and n % 64 != 0 and len(items) <= 64, (name, n, len(items))
    assert np.isfinite(rays).all() and (rays[:, 3:6] != 0.0).any(axis=1).all(), name
    i = np.arange(n, dtype=np.uint64)
    keys = np.stack([np.full(n, zlib.crc32(name.encode()) | 1, dtype=np.uint64), i * np.uint64(7) + np.uint64(3), i % np.uint64(5)], axis=1)
    c = dict(name=name, items=items, root=root, rays=rays, keys=keys, t_min=float(t_min), build=lambda B: build_scene(B, items, root))
    c.update(meta)
    return c


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _disc(rng, n, radius):
    r, a = radius * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2.0 * math.pi, n)
    return r * np.cos(a), r * np.sin(a)


# -- media --
FOG_SPACING, N_FOGS = 1.5, 5
SMALL = ("sphere", (3.0, 0.0, 0.0), 0.45)                   # inside the third fog
# three more along the axis: a ray then meets several surfaces, of which one listed before a medium may lie behind the closest one and
# still in front of the medium's exit -- the only rows on which track_bound's widening and the order-restricted walk decide anything
MORE = [("sphere", (0.8, 0.0, 0.0), 0.35), ("sphere", (4.6, 0.0, 0.0), 0.35), ("sphere", (6.3, 0.0, 0.0), 0.35)]
WALL = ("rect", 0, -4.0, -4.0, 4.0, 4.0, 9.5)               # x = 9.5, behind the row
WALL_BACK = ("rect", 0, -4.0, -4.0, 4.0, 4.0, -5.5)


def fog_row(k, densities=None):
    densities = densities or [0.15] * k
    return [("medium", densities[i], ("sphere", (FOG_SPACING * i, 0.0, 0.0), 1.0)) for i in range(k)]


def ordered(fogs, surfaces, order, rng):
    if order == "surfaces_first":
        return surfaces + fogs
    if order == "surfaces_last":
        return fogs + surfaces
    if order == "ascending":            # (the surfaces in the middle)
        return fogs[:2] + surfaces + fogs[2:]
    if order == "descending":
        return fogs[::-1] + surfaces
    if order == "interleaved":
        out, s = [], list(surfaces)
        for i, f in enumerate(fogs):
            out.append(f)
            if i % 2 == 0 and s:
                out.append(s.pop(0))
        return out + s
    both = fogs + surfaces
    return [both[i] for i in rng.permutation(len(both))]


def axis_rays(rng, n, lateral=0.9, tilt=0.12):
    """rays along the row's axis, either way, from origins anywhere along it"""
    x = rng.uniform(-3.0, 8.5, n)
    y, z = _disc(rng, n, np.where(np.arange(n) % 3 != 0, lateral, 0.45 * lateral))      # a third of them close to the axis
    sign = np.where(rng.uniform(0.0, 1.0, n) < 0.8, 1.0, -1.0)
    d = np.stack([sign * rng.uniform(0.5, 2.0, n), rng.uniform(-tilt, tilt, n), rng.uniform(-tilt, tilt, n)], axis=1)
    return np.stack([x, y, z], axis=1), d


def row_of_fogs():
    out = []
    for order in ORDERS:
        name = "row_of_fogs/5/" + order
        rng = _rng(name)
        o, d = axis_rays(rng, 1100)
        out.append(_case(name, ordered(fog_row(N_FOGS), [SMALL] + MORE + [WALL, WALL_BACK], order, rng), "list", o, d, 0.0, n_media=N_FOGS))
    # a surface inside the second fog listed first and the nearest surface listed last: a ray from the left meets the nearest one (S) and,
    # behind it, surfaces that the list holds before the second and the third fog and that lie in front of those fogs' exits
    name = "row_of_fogs/5/nearest_last"
    rng = _rng(name)
    f = fog_row(N_FOGS)
    items = [("sphere", (1.9, 0.0, 0.0), 0.35), f[0], SMALL, f[1], MORE[1], f[2], MORE[2], f[3], MORE[0], f[4], WALL, WALL_BACK]
    o, d = axis_rays(rng, 1500)
    o[:, 0] = np.where(np.arange(len(o)) % 2 == 0, rng.uniform(-3.0, 0.3, len(o)), o[:, 0])          # half of them start left of every surface
    out.append(_case(name, items, "list", o, d, 0.0, n_media=N_FOGS))
    for k in range(N_FOGS):
        name = "row_of_fogs/%d/interleaved" % k
        rng = _rng(name)
        o, d = axis_rays(rng, 300)
        out.append(_case(name, ordered(fog_row(k), [SMALL] + MORE + [WALL, WALL_BACK], "interleaved", rng), "list", o, d, 0.0, n_media=k))
    return out


def densities():
    out = []
    for tag, dens in (("dense", [1e6] * 5), ("thin", [1e-9] * 5), ("mixed", [1e6, 1e-9, 0.15, 1e-9, 1e6]), ("mixed2", [1e-9, 0.4, 1e6, 0.15, 1e-9])):
        for order in ("surfaces_last", "shuffled"):
            name = "densities/%s/%s" % (tag, order)
            rng = _rng(name)
            o, d = axis_rays(rng, 500)
            out.append(_case(name, ordered(fog_row(5, dens), [SMALL] + MORE + [WALL, WALL_BACK], order, rng), "list", o, d, 0.0))
    return out


def ball_rays(rng, n, centre, radius, inside=0.3, aim=0.95):
    """rays at points within aim * radius of `centre`, from a shell around it or (a share of them) from inside"""
    c = np.asarray(centre, dtype=np.float64)
    tgt = c + _unit(rng.normal(size=(n, 3))) * (radius * aim * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0))
    far = c + _unit(rng.normal(size=(n, 3))) * rng.uniform(2.0, 4.0, (n, 1)) * radius
    near = c + _unit(rng.normal(size=(n, 3))) * rng.uniform(0.0, 0.9, (n, 1)) * radius
    o = np.where(rng.uniform(0.0, 1.0, (n, 1)) < inside, near, far)
    return o, (tgt - o) * rng.uniform(0.3, 3.0, (n, 1))


def coincident():
    ball = ("sphere", (0.0, 0.0, 0.0), 1.0)
    fog = ("medium", 0.6, ("sphere", (0.0, 0.0, 0.0), 1.0))
    fog_b = ("medium", 0.9, ("sphere", (0.0, 0.0, 0.0), 1.0))
    shell = ("sphere", (0.0, 0.0, 0.0), 6.0)                # encloses everything: every ray hits a surface
    out = []
    for tag, items in (("surface_before", [ball, fog, shell]), ("surface_after", [fog, ball, shell]), ("listed_twice", [fog, shell, fog]),
                       ("shared_geometry", [fog, fog_b, shell]), ("shared_geometry_and_surface", [fog_b, ball, fog, shell])):
        name = "coincident/" + tag
        o, d = ball_rays(_rng(name), 450, (0.0, 0.0, 0.0), 1.0)
        out.append(_case(name, items, "list", o, d, 0.0))
    return out


def origins():
    one = [("medium", 0.5, ("sphere", (0.0, 0.0, 0.0), 1.0)), ("rect", 0, -9.0, -9.0, 9.0, 9.0, 7.0)]
    three = [("medium", 0.2, ("sphere", (0.0, 0.0, 0.0), 3.0)), ("medium", 0.5, ("sphere", (0.0, 0.0, 0.0), 1.0)),
             ("medium", 0.3, ("sphere", (0.0, 0.0, 0.0), 2.0)), ("sphere", (0.0, 0.0, 0.0), 0.25), ("rect", 0, -9.0, -9.0, 9.0, 9.0, 7.0)]
    out = []
    for tag, items in (("one", one), ("three", three)):
        for t_min in (0.0, 1e-3, 0.5, 10.0):                # 10: beyond the exit of every medium for the unit-length share of the rays
            name = "origins/%s/t_min=%g" % (tag, t_min)
            rng = _rng(name)
            n = 120
            inside = _unit(rng.normal(size=(n, 3))) * rng.uniform(0.0, 2.9, (n, 1))
            on = np.array([(1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, -3.0), (-1.0, 0.0, 0.0), (0.0, -2.0, 0.0), (3.0, 0.0, 0.0)] * 20)   # exactly on a boundary
            behind = np.stack([rng.uniform(7.5, 9.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n)], axis=1)              # beyond the wall
            o = np.concatenate([inside, on, behind, behind])
            d = np.concatenate([_unit(rng.normal(size=(n, 3))), _unit(rng.normal(size=(len(on), 3))),
                                np.stack([rng.uniform(0.2, 1.0, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)], axis=1),   # pointing away
                                _unit(-behind + rng.normal(size=(n, 3)) * 0.3)])                                                        # and back in
            d[::3] *= 0.05                                   # a third of the rays are 20 times slower: t_min = 10 is then inside the media
            out.append(_case(name, items, "list", o, d, 0.0, t_min=t_min))
    return out


CHORDS = (0.5, 0.99, 1.01, 2.0)                             # times 1e-4 in t


def second_query():
    items = [("medium", 0.3, ("sphere", (0.0, 0.0, 0.0), 1.0)), ("sphere", (0.0, 0.0, 6.0), 2.5), ("rect", 2, -9.0, -9.0, 9.0, 9.0, 9.0)]
    out = []
    # by impact parameter: unit direction along z, so a chord of length L in t lies at b = sqrt(1 - (L / 2)^2) from the axis
    name = "second_query/impact"
    rng = _rng(name)
    n = 600
    mult = np.array(CHORDS)[np.arange(n) % 4] * rng.uniform(0.97, 1.0, n) ** np.where(np.arange(n) % 4 < 2, 1.0, -1.0)   # below 1: a little shorter, above: longer
    L = mult * 1e-4
    b = np.sqrt(1.0 - (L / 2.0) ** 2)
    a = rng.uniform(0.0, 2.0 * math.pi, n)
    o = np.stack([b * np.cos(a), b * np.sin(a), np.full(n, -4.0)], axis=1)
    d = np.tile([0.0, 0.0, 1.0], (n, 1))
    out.append(_case(name, items, "list", o, d, 0.0, t_min=1e-9, chord=L))
    # by direction length: the same geometric chords of 0.2 .. 2, in t divided by |d|
    for length in (1e-6, 1.0, 1e5):
        name = "second_query/length=%g" % length
        rng = _rng(name)
        n = 200
        bx, by = _disc(rng, n, 0.99)
        o = np.stack([bx, by, np.full(n, -4.0)], axis=1)
        d = np.tile([0.0, 0.0, length], (n, 1))
        out.append(_case(name, items, "list", o, d, 0.0, t_min=1e-9, chord=2.0 * np.sqrt(1.0 - bx * bx - by * by) / length))
    # the four multiples by direction length: rays close to the axis (a chord of 2 sqrt(1 - b^2) >= 1.99), |d| = chord / (multiple * 1e-4)
    name = "second_query/length_multiples"
    rng = _rng(name)
    n = 400
    mult = np.array(CHORDS)[np.arange(n) % 4] * rng.uniform(0.98, 1.0, n) ** np.where(np.arange(n) % 4 < 2, 1.0, -1.0)
    bx, by = _disc(rng, n, 0.05)
    geo = 2.0 * np.sqrt(1.0 - bx * bx - by * by)
    length = geo / (mult * 1e-4)
    o = np.stack([bx, by, np.full(n, -4.0)], axis=1)
    d = np.stack([np.zeros(n), np.zeros(n), length], axis=1)
    out.append(_case(name, items, "list", o, d, 0.0, t_min=1e-9, chord=mult * 1e-4))
    # the two around 1e-4 by direction length: |d| = 1e4 makes chords of 0 .. 2e-4
    name = "second_query/length=10000"
    rng = _rng(name)
    n = 500
    bx, by = _disc(rng, n, 0.99)
    o = np.stack([bx, by, np.full(n, -4.0)], axis=1)
    d = np.tile([0.0, 0.0, 1e4], (n, 1))
    chord = 2.0 * np.sqrt(1.0 - bx * bx - by * by) / 1e4
    keep = np.abs(chord / 1e-4 - 1.0) > 1e-3                 # (no row within rounding of the offset itself: the sides are told apart by intent)
    keep[-1] &= keep.sum() % 64 != 0
    out.append(_case(name, items, "list", o[keep], d[keep], 0.0, t_min=1e-9, chord=chord[keep]))
    return out


# boundary kinds that are not one world-space sphere: (description, centre, half-size)
def boundary_kinds():
    return [
        (("mesh",), (0.0, 0.0, 0.0), 1.0),
        (("cube", (4.0, -1.0, -1.0), (6.0, 1.0, 1.0)), (5.0, 0.0, 0.0), 1.0),
        (("xform", (20.0, 35.0, 10.0), (1.0, 1.0, 1.0), (10.0, 0.0, 0.0), ("cube", (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))), (10.0, 0.0, 0.0), 1.0),
        (("list", [("sphere", (14.6, 0.0, 0.0), 1.0), ("sphere", (15.4, 0.0, 0.0), 1.0)]), (15.0, 0.0, 0.0), 0.6),
        (("msphere", (20.0, -0.5, 0.0), (20.0, 0.5, 0.0), 0.0, 1.0, 1.2), (20.0, 0.0, 0.0), 0.7),
    ]


def boundary_items(rng=None, plain=False):
    """plain: only the kinds tests/walk_ref.py restates"""
    items = [("medium", 0.4 + 0.1 * i, b) for i, (b, _, _) in enumerate(boundary_kinds()) if not plain or b[0] not in ("mesh", "xform")]
    items += [("sphere", (7.5, 0.0, 0.0), 0.5), ("sphere", (17.5, 0.3, 0.0), 0.5), ("sphere", (10.0, 0.0, 0.0), 40.0)]
    return items if rng is None else [items[i] for i in rng.permutation(len(items))]


def boundary_rays(rng, n_each):
    """rays at points within 0.9 of each boundary's half-size of its centre (not grazing), from a shell 3 .. 6 half-sizes away or from inside"""
    o, d = [], []
    for _, c, h in boundary_kinds():
        c = np.asarray(c)
        tgt = c + rng.uniform(-0.9 * h, 0.9 * h, (n_each, 3))
        far = c + _unit(rng.normal(size=(n_each, 3))) * rng.uniform(3.0, 6.0, (n_each, 1))
        org = np.where(rng.uniform(0.0, 1.0, (n_each, 1)) < 0.25, c + rng.uniform(-0.5 * h, 0.5 * h, (n_each, 3)), far)
        o.append(org)
        d.append((tgt - org) * rng.uniform(0.5, 2.0, (n_each, 1)))
    return np.concatenate(o), np.concatenate(d)


def boundaries():
    out = []
    for tag in ("in_order", "shuffled", "plain"):
        name = "boundaries/" + tag
        rng = _rng(name)
        items = boundary_items(rng if tag != "in_order" else None, plain=tag == "plain")
        o, d = boundary_rays(rng, 150)
        out.append(_case(name, items, "list", o, d, rng.uniform(0.0, 1.0, len(o))))
    return out


def bvh_roots():
    out = []
    for scale in (1e-3, 1.0, 1e5):
        for seed in (1, 2, 3):
            name = "bvh_roots/fogs/scale=%g/seed=%d" % (scale, seed)
            rng = _rng(name)
            clutter = [("sphere", (float(rng.uniform(-2.0, 8.0)),) + tuple(float(x) for x in rng.uniform(-1.2, 1.2, 2)), float(rng.uniform(0.1, 0.25)))
                       for _ in range(24)]                  # small surfaces in and around the fogs: an accel walk of some depth
            items = [scaled(x, scale) for x in ordered(fog_row(N_FOGS), [SMALL] + MORE + [WALL, WALL_BACK] + clutter, "shuffled", rng)]
            o, d = axis_rays(rng, 400)
            out.append(_case(name, items, ("bvh", seed), o * scale, d * scale, 0.0))
            name = "bvh_roots/boundaries/scale=%g/seed=%d" % (scale, seed)
            rng = _rng(name)
            items = [scaled(x, scale) for x in boundary_items()]
            o, d = boundary_rays(rng, 80)
            out.append(_case(name, items, ("bvh", seed), o * scale, d * scale, rng.uniform(0.0, 1.0, len(o))))
    return out


def nested():
    from nested_scenes import chain
    levels = chain(3) + [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (6.0, 0.0, 0.0))]
    fog = ("medium", 0.5, ("sphere", (0.0, 0.0, 0.0), 1.0))
    box = ("nest", levels, ("cube", (-0.8, -0.8, -0.8), (0.8, 0.8, 0.8)))
    shell = ("sphere", (3.0, 0.0, 0.0), 30.0)
    out = []
    # a fog beside a cube under a chain: the chain walk (GENERAL == 3) with MEDIA, accel and all
    name = "nested/fog_beside_chain"
    rng = _rng(name)
    oa, da = ball_rays(rng, 200, (0.0, 0.0, 0.0), 1.0)
    ob, db = ball_rays(rng, 200, (7.0, -2.0, 2.0), 2.0, inside=0.0)
    out.append(_case(name, [fog, box, shell], "list", np.concatenate([oa, ob]), np.concatenate([da, db]), 0.0))
    # a fog under the chain itself, and a fog whose boundary is under it
    under = ("nest", levels, ("medium", 0.5, ("sphere", (0.0, 0.0, 0.0), 1.0)))
    around = ("medium", 0.7, ("nest", chain(2), ("sphere", (0.0, 0.0, 0.0), 1.0)))
    name = "nested/fog_under_chain"
    rng = _rng(name)
    oa, da = ball_rays(rng, 200, (0.0, 0.0, 0.0), 0.8)
    ob, db = ball_rays(rng, 200, (7.0, -2.0, 2.0), 1.5, inside=0.0)
    out.append(_case(name, [around, under, shell], "list", np.concatenate([oa, ob]), np.concatenate([da, db]), 0.0))
    # no fog: the chain walk alone, and with a moving sphere under a chain (its ray time read from the lane's slot)
    name = "nested/chain_alone"
    rng = _rng(name)
    o, d = ball_rays(rng, 300, (7.0, -2.0, 2.0), 2.0, inside=0.1)
    out.append(_case(name, [box, shell], ("bvh", 1), o, d, 0.0))
    mover = ("nest", chain(2), ("msphere", (-1.0, 0.0, 0.0), (1.0, 0.5, 0.0), 0.0, 1.0, 0.8))
    name = "nested/moving_under_chain"
    rng = _rng(name)
    import oracle
    probe, owners = build_scene(oracle.Scene(), [mover], "list")                       # where the chain puts the sweep: the oracle's box of it
    lo_hi = probe.bounding_box(max(owners[0]))
    mid, half = 0.5 * (lo_hi[:3] + lo_hi[3:]), 0.5 * float((lo_hi[3:] - lo_hi[:3]).max())
    oa, da = ball_rays(rng, 300, tuple(mid), 0.7 * half, inside=0.1)
    ob, db = ball_rays(rng, 100, (7.0, -2.0, 2.0), 2.0, inside=0.0)
    n = 400
    out.append(_case(name, [mover, box, shell], ("bvh", 2), np.concatenate([oa, ob]), np.concatenate([da, db]), np.array(LANE_TIMES)[np.arange(n) % 7]))
    return out


# -- moving spheres --
def centre(ms, time):
    """MovingSphere::center in the oracle's operations"""
    _, c0, c1, t0, t1, _ = ms
    s = (time - t0) / (t1 - t0)
    return tuple(c0[i] + (c1[i] - c0[i]) * s for i in range(3))


def sweep():
    out = []
    for t0, t1 in ((0.0, 1.0), (-2.5, 7.25)):
        ms = ("msphere", (0.0, 0.0, 0.0), (1000.0, 0.0, 0.0), t0, t1, 1.0)
        name = "sweep/[%g,%g]" % (t0, t1)
        rng = _rng(name)
        times = [t0, t1, float(np.nextafter(t0, t1)), float(np.nextafter(t1, t0)), 0.5 * (t0 + t1)] + [float(x) for x in rng.uniform(t0, t1, 45)]
        o, d, tm = [], [], []
        for time in times:
            c = np.array(centre(ms, time))
            for org in (c + np.array([30.0, 400.0, -250.0]), c + np.array([-2500.0, 10.0, 40.0]), c + _unit(rng.normal(size=3)) * 3.0,
                        c + rng.uniform(-0.5, 0.5, 3)):
                w = _unit(c - org) if np.abs(c - org).max() > 1.0 else np.array([0.0, 0.0, 1.0])
                side = _unit(np.cross(w, [0.3, 1.0, 0.2]))
                targets = [c, c + np.array([0.0, 1.0, 0.0]), c - np.array([0.0, 1.0, 0.0])]                       # the centre and the poles
                dist = math.sqrt(((c - org) ** 2).sum())
                for b in (1.0 + 1e-9, 1.0 - 1e-9, 1.0 + 1e-3, 1.0 - 1e-3, 1.5, -3.0):                              # the silhouette, and past it:
                    lateral = b * dist / math.sqrt(dist * dist - b * b) if dist > 3.5 else b                       # the ray passes the centre at |b|
                    targets.append(c + side * lateral)
                for tgt in targets:
                    o.append(org)
                    d.append((tgt - org) * rng.uniform(0.5, 2.0))
                    tm.append(time)
        out.append(_case(name, [ms], "list", o, d, tm, t_min=1e-3))
    return out


def lane_items(rng):
    a = ("msphere", (0.0, 0.0, 0.0), (10.0, 0.0, 0.0), 0.0, 1.0, 0.6)      # crosses the shared ray at time 0.5
    b = ("msphere", (5.0, -4.0, 3.0), (5.0, 12.0, 3.0), 0.0, 1.0, 0.6)     # at time 0.25
    c = ("sphere", (5.0, 0.0, 8.0), 1.0)                                    # behind both, always
    items = [a, b, c]
    for i in range(18):                                                     # the rest keep clear of the shared ray's line x = 5, y = 0
        c0 = np.array([rng.uniform(-12.0, 22.0), rng.choice([-1.0, 1.0]) * rng.uniform(3.5, 10.0), rng.uniform(-6.0, 14.0)])
        c1 = c0 + np.array([rng.uniform(-4.0, 4.0), 0.0, rng.uniform(-4.0, 4.0)])
        items.append(("msphere", tuple(c0), tuple(c1), 0.0, 1.0, float(rng.uniform(0.4, 1.2))))
    for i in range(19):
        c0 = (rng.uniform(-12.0, 22.0), rng.choice([-1.0, 1.0]) * rng.uniform(3.5, 10.0), rng.uniform(-6.0, 14.0))
        items.append(("sphere", tuple(float(x) for x in c0), float(rng.uniform(0.4, 1.2))))
    return items


def lanes():
    out = []
    for scale in (1e-3, 1.0, 1e5):
        for seed in (1, 2):
            name = "lanes/scale=%g/seed=%d" % (scale, seed)
            rng = _rng(name)
            base = lane_items(rng)
            n = 64 * 7 + 29
            time = np.array(LANE_TIMES)[np.arange(n) % 7]
            pick = rng.integers(0, len(base), n)
            tgt = np.zeros((n, 3))
            for i in range(n):                                              # at a sphere where it is at the row's time, or a little beside it
                s = base[pick[i]]
                c = centre(s, time[i]) if s[0] == "msphere" else s[1]
                tgt[i] = np.array(c) + _unit(rng.normal(size=3)) * s[-1] * rng.uniform(0.0, 1.6)
            o = np.stack([rng.uniform(-15.0, 25.0, n), rng.uniform(-12.0, 12.0, n), rng.uniform(-30.0, -10.0, n)], axis=1)
            d = (tgt - o) * rng.uniform(0.3, 2.0, (n, 1))
            o[64:128] = (5.0, 0.0, -20.0)                                   # one block of 64 rows shares a single ray and differs in time alone
            d[64:128] = (0.0, 0.0, 1.0)
            out.append(_case(name, [scaled(x, scale) for x in base], ("bvh", seed), o * scale, d * scale, time, shared_block=(64, 128)))
    return out


def static_twin():
    out = []
    still = ("msphere", (1.0, 2.0, 3.0), (1.0, 2.0, 3.0), 0.0, 1.0, 1.5)
    name = "static_twin/still"
    rng = _rng(name)
    o, d = ball_rays(rng, 200, (1.0, 2.0, 3.0), 1.5 * 1.2)
    out.append(_case(name, [still, ("sphere", (1.0, 2.0, 30.0), 20.0)], "list", o, d, rng.uniform(0.0, 1.0, len(o))))
    moving = ("msphere", (0.0, 0.0, 0.0), (3.0, 0.0, 0.0), 0.25, 2.0, 1.0)
    twin = ("sphere", (0.0, 0.0, 0.0), 1.0)
    for tag, items in (("moving_first", [moving, twin]), ("static_first", [twin, moving])):
        name = "static_twin/" + tag
        rng = _rng(name)
        o, d = ball_rays(rng, 300, (0.0, 0.0, 0.0), 1.2)
        time = np.where(np.arange(len(o)) % 3 == 0, rng.uniform(0.25, 2.0, len(o)), 0.25)       # two thirds exactly at time0: an exact tie
        out.append(_case(name, items, "list", o, d, time))
    return out


def fog_and_motion():
    items = [("medium", 0.3, ("sphere", (0.0, 0.0, 0.0), 2.0)), ("msphere", (-3.0, 0.0, 0.0), (3.0, 0.0, 0.0), 0.0, 1.0, 0.5),
             ("medium", 0.5, ("sphere", (2.5, 0.0, 0.0), 1.5)), ("msphere", (2.5, -2.0, 0.0), (2.5, 2.0, 0.5), 0.0, 1.0, 0.4),
             ("medium", 0.8, ("msphere", (-2.0, 1.0, 0.0), (-2.0, -1.0, 0.0), 0.0, 1.0, 1.0)), ("sphere", (0.0, 0.0, 0.0), 0.3),
             ("sphere", (0.0, 0.0, 0.0), 25.0)]
    out = []
    for root in ("list", ("bvh", 1), ("bvh", 2)):
        name = "fog_and_motion/%s" % (root if root == "list" else "bvh%d" % root[1])
        rng = _rng(name)
        o, d = ball_rays(rng, 500, (0.5, 0.0, 0.0), 3.0)
        out.append(_case(name, items, root, o, d, rng.uniform(0.0, 1.0, len(o))))
    return out


_GEN = dict(row_of_fogs=row_of_fogs, densities=densities, coincident=coincident, origins=origins, second_query=second_query,
            boundaries=boundaries, bvh_roots=bvh_roots, nested=nested, sweep=sweep, lanes=lanes, static_twin=static_twin,
            fog_and_motion=fog_and_motion)
_CACHE = {}


def family(name):
    """the cases of one family (built once, never changed)"""
    if name not in _CACHE:
        _CACHE[name] = _GEN[name]()
    return _CACHE[name]


_ORACLE = {}


def oracle_walk(case):
    """-> (oracle.Scene, owners, out [n, 12], draws [n]) of a case: computed once, shared by the tests"""
    import oracle
    if case["name"] not in _ORACLE:
        o, owners = case["build"](oracle.Scene())
        out, draws = o.walk(case["rays"], case["keys"], case["t_min"])
        out.setflags(write=False)
        draws.setflags(write=False)
        _ORACLE[case["name"]] = (o, owners, out, draws)
    return _ORACLE[case["name"]]
