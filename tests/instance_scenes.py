"""Scenes and explicit rays for the instance walks of kernels 5 / 6 (tests/test_instance_scenes.py, tests/test_instance_walks_gpu.py).

Those walks run an f32 slab test on a lossy second encoding of a deferred mesh instance (flat.h "Compact instance data": NodeQ boxes on a
16-bit grid padded by P, a thin axis widened, the ray mapped onto the grid once per request).  A pad that is slightly too small culls a
hit for rare rays only -- far origins, rays that graze a silhouette or run inside a box face -- so the scenes here put the encoding into
every regime it has (coordinate scales 1e-3 .. 1e5, a unit instance in a scene 100 .. 16 000 times its size where the widening takes over
and a grid cell is coarser than a triangle, a needle, flat instances, a dyadic box whose twin ties with it in every hit) and the ray
families aim at the instances from where the bound is tight.

Every scene is ONE function of a builder (rtamd.World or oracle.Scene: they share the reference's constructor names) and a mesh_fn, as
test_parity_gpu._random_instance_scene; everything random is seeded by the scene's and the family's name.  The ray generators read the
oracle's side only (the transforms it stored and its hit records): no device is needed to build a family."""
import zlib

import numpy as np

T_MIN = 1e-3
SCALES = (1e-3, 1.0, 250.0, 1e5)
RATIOS = (100, 4000, 16000)
SCENES = ["scale[%g]" % s for s in SCALES] + ["small_in_big[%d]" % r for r in RATIOS] + ["needle", "flat", "box"]
FAMILIES = ("near", "far", "components", "graze", "t_max")
GRAZE_EPS = (1e-3, 1e-6, 1e-9)
BOX_AT, BOX_SCALE, BOX_N = (3.0, 1.0, -2.0), 2.0, 4      # the box scene's instance: [3, 5] x [1, 3] x [-2, 0], mesh lines 0.5 apart


def families(name):
    return FAMILIES + (("lattice",) if name == "box" else ())


def world_mesh(B, P, N, I, mat, seed):
    return B.Mesh(P, N, I, mat, bvh_seed=seed)


def oracle_mesh(B, P, N, I, mat, seed):
    return B.Mesh(P, N, I, mat, seed)


def _rng(*what):
    return np.random.default_rng(zlib.crc32(" ".join(str(w) for w in what).encode()))


def _t(v):
    return tuple(float(x) for x in v)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------
def spec(name):
    """-> dict(instances=[(mesh, rotate, scale, translate, material, bvh_seed)], spheres=[(centre, radius, material)],
    rects=[(xz0, xz1, y, material)], cam=Camera::new's arguments, t_min=the frames' t_min).  Materials are named as items() makes them."""
    from rtamd import shapes
    tri = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0.0, 0.0, 1.0]] * 3), np.array([[0, 1, 2]], dtype=np.uint32))
    up = (0.0, 1.0, 0.0)
    if name.startswith("scale["):
        s = float(name[6:-1])
        rng = _rng(name)
        inst = []
        for k in range(3):
            sc = rng.uniform(0.5, 2.0, 3) * s
            if k == 1:
                sc[0] = -sc[0]       # mirrored
            inst.append((shapes.torus(12, 16), _t(rng.uniform(-180.0, 180.0, 3)), _t(sc), _t(rng.uniform(-5.0, 5.0, 3) * s), ("grey", "glass", "metal")[k], 11 + k))
        spheres = [(_t(rng.uniform(-6.0, 6.0, 3) * s), float(rng.uniform(0.3, 1.0) * s), ("light", "grey", "light", "glass")[k % 4]) for k in range(8)]
        rects = [((-8.0 * s, -8.0 * s), (8.0 * s, 8.0 * s), -6.0 * s, "light")]
        cam = ((0.0, 2.0 * s, -11.0 * s), (0.0, 0.0, 0.0), up, 60.0, 1.0, 0.0, 10.0 * s)
        return dict(instances=inst, spheres=spheres, rects=rects, cam=cam, t_min=T_MIN * min(s, 1.0))
    if name.startswith("small_in_big["):
        r = float(name[13:-1])
        at = (0.9 * r, 0.0, 0.0)
        cam = ((at[0] - 3.0, 2.5, -4.0), at, up, 40.0, 1.0, 0.0, 5.0)
        return dict(instances=[(shapes.torus(12, 16), (30.0, 20.0, 10.0), (1.0, 1.0, 1.0), at, "grey", 5)], spheres=[],
                    rects=[((-r, -r), (r, r), -2.0, "light")], cam=cam, t_min=T_MIN)
    if name == "needle":
        cam = ((4.0, 3.0, -33.0), (1.0, 0.0, -28.0), up, 50.0, 1.0, 0.0, 10.0)      # at the ring itself: its middle is a hole
        return dict(instances=[(shapes.torus(12, 16), (25.0, 40.0, 10.0), (1.0, 1e-3, 40.0), (0.0, 0.0, 0.0), "grey", 5)],
                    spheres=[((0.0, 40.0, -28.0), 35.0, "light")], rects=[], cam=cam, t_min=T_MIN)
    if name == "flat":
        cam = ((0.5, 2.6, 0.2), (0.5, 0.5, 0.25), (0.0, 0.0, 1.0), 90.0, 1.0, 0.0, 10.0)       # down onto both, from under the light
        return dict(instances=[(shapes.sheet(8), (20.0, 35.0, 10.0), (1.5, 1.0, 0.7), (-2.0, 0.5, 0.0), "grey", 6),
                               (tri, (15.0, 30.0, 0.0), (2.0, 2.0, 2.0), (1.5, 0.0, 1.0), "metal", 7)],
                    spheres=[((-0.5, 8.0, 0.5), 5.0, "light")], rects=[], cam=cam, t_min=T_MIN)
    if name == "box":
        sc = (BOX_SCALE,) * 3
        cam = ((9.0, 6.0, -8.0), (4.0, 2.0, -1.0), up, 40.0, 1.0, 0.0, 10.0)
        return dict(instances=[(shapes.box_mesh(BOX_N), (0.0, 0.0, 0.0), sc, BOX_AT, "metal", 8), (shapes.box_mesh(BOX_N), (0.0, 0.0, 0.0), sc, BOX_AT, "grey", 9)],
                    spheres=[], rects=[((-16.0, -24.0), (24.0, 24.0), 9.0, "light")], cam=cam, t_min=T_MIN)
    raise KeyError(name)


def items(B, name, mesh_fn, only=None, meshes_only=False, medium=False):
    """the scene's top-level hitables on builder B.  only=i: instance i alone; meshes_only: the instances alone; medium: plus a ConstantMedium."""
    sp = spec(name)
    tex = {k: B.ConstantTexture(c) for k, c in (("grey", (0.7, 0.7, 0.7)), ("metal", (0.8, 0.85, 0.9)), ("glass", (1.0, 1.0, 1.0)), ("light", (4.0, 4.0, 4.0)))}
    mats = {"grey": B.Lambertian(tex["grey"]), "metal": B.Metal(tex["metal"], 0.1), "glass": B.Dielectric(1.5, tex["glass"]), "light": B.DiffuseLight(tex["light"])}
    out = []
    for i, ((P, N, I), rot, sc, tr, mat, seed) in enumerate(sp["instances"]):
        if only is None or only == i:
            out.append(B.Transform(rot, sc, tr, mesh_fn(B, P, N, I, mats[mat], seed)))
    if only is None and not meshes_only:
        out += [B.Sphere(c, r, mats[m]) for c, r, m in sp["spheres"]]
        out += [B.XZRectangle(a, b, y, mats[m]) for a, b, y, m in sp["rects"]]
        if medium:
            c = np.asarray(sp["cam"][1])
            out.append(B.ConstantMedium(0.2, B.Sphere(_t(c), float(np.abs(c).max() * 0.1 + 1.0), mats["glass"]), B.Isotropic(tex["grey"])))
    return out


_REF, _WORLD, _RAYS = {}, {}, {}


def ref(name):
    """the oracle's side of a scene, built once: dict(full, meshes, solo=[instance i alone], verts=[world-space vertices], tris=[index triples],
    extent=largest absolute coordinate of the scene's reference box)"""
    if name not in _REF:
        import oracle
        out = dict(solo=[], verts=[], tris=[])
        for key, kw in (("full", {}), ("meshes", dict(meshes_only=True))):
            o = oracle.Scene()
            root = o.World(items(o, name, oracle_mesh, **kw), 3)
            out[key] = o
            if key == "full":
                o.Camera(*spec(name)["cam"])
                out["extent"] = float(np.abs(o.bounding_box(root)).max())
        for i in range(len(spec(name)["instances"])):
            o = oracle.Scene()
            o.World(items(o, name, oracle_mesh, only=i), 3)
            info = o.lowering_info()
            (M,), ((P, I),) = info["trans"].values(), info["mesh"].values()
            out["solo"].append(o)
            out["verts"].append(P @ M[:3, :3].T + M[:3, 3])
            out["tris"].append(np.array(I))
        _REF[name] = out
    return _REF[name]


def world(name, medium=False):
    """the product's side: a committed rtamd.World (built once per scene; the one with a medium is not kept)"""
    import rtamd
    if medium or name not in _WORLD:
        w = rtamd.World()
        w.new(items(w, name, world_mesh, medium=medium), bvh_seed=3)
        if medium:
            return w
        _WORLD[name] = w
    return _WORLD[name]


def camera(name):
    import rtamd
    f, t, up, vfov, asp, ap, fd = spec(name)["cam"]
    return rtamd.Camera((f, t), up, vfov, asp, ap, fd)


# ---- rays --------------------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _boxes(R, which):
    lo = np.array([v.min(axis=0) for v in R["verts"]])[which]
    hi = np.array([v.max(axis=0) for v in R["verts"]])[which]
    return 0.5 * (lo + hi), 0.5 * (hi - lo), np.linalg.norm(hi - lo, axis=1, keepdims=True)


def _targets(R, rng, which):
    """45 % points ON a random triangle of the ray's instance, the others anywhere in its bounds grown by half: `jittered around the instance`"""
    n = len(which)
    c, h, _ = _boxes(R, which)
    tgt = c + rng.uniform(-1.5, 1.5, (n, 3)) * h
    for k in np.flatnonzero(rng.random(n) < 0.45):
        V, T = R["verts"][which[k]], R["tris"][which[k]]
        b = rng.dirichlet((1.0, 1.0, 1.0))
        tgt[k] = b @ V[T[rng.integers(len(T))]]
    return tgt


def _near(R, rng, n):
    which = np.arange(n) % len(R["verts"])
    c, h, size = _boxes(R, which)
    u = _unit(rng, n)
    u[rng.random(n) < 0.7, 1] *= 0.35     # most of them near the instance's own level: a floor under it catches every ray that descends
    o = c + u * rng.uniform(1.0, 4.0, (n, 1)) * size
    inside = rng.random(n) < 0.25
    o[inside] = (c + rng.uniform(-1.0, 1.0, (n, 3)) * h)[inside]
    tgt = _targets(R, rng, which)
    return o, tgt


def _far_origins(R, rng, which, c):
    """8 .. 30 scene extents from the instance's centre: half of them in any direction, half within a few instance heights of the instance's own
    level (a scene-sized floor under the instance hides it from below and catches every ray from above that misses it)"""
    n = len(which)
    _, h, _ = _boxes(R, which)
    dist = rng.uniform(8.0, 30.0, (n, 1)) * R["extent"]
    o = c + _unit(rng, n) * dist
    slab = rng.random(n) < 0.5
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    level = c + np.stack([np.cos(phi) * dist[:, 0], rng.uniform(-1.0, 3.0, n) * h[:, 1], np.sin(phi) * dist[:, 0]], axis=1)
    o[slab] = level[slab]
    assert np.abs(o).max() <= 32.0 * R["extent"]
    return o


def _build(name, family):
    R = ref(name)
    rng = _rng(name, family)
    t_max, meta = float("inf"), {}
    if family == "near":
        o, tgt = _near(R, rng, 4000)
        rays = np.concatenate([o, tgt - o], axis=1)
    elif family == "far":
        which = np.arange(4000) % len(R["verts"])
        tgt = _targets(R, rng, which)
        o = _far_origins(R, rng, which, _boxes(R, which)[0])
        rays = np.concatenate([o, tgt - o], axis=1)
    elif family == "components":
        o, tgt = _near(R, rng, 4004)
        d = tgt - o
        for k in range(0, len(d), 7):       # one component exactly 0: the ray still passes through its target
            a = int(rng.integers(3))
            d[k, a] = 0.0
            o[k, a] = tgt[k, a]
        d[::11] *= 1e-6
        d[::13] *= 1e6
        rays = np.concatenate([o, d], axis=1)
    elif family == "graze":
        rays, meta = _graze(R, rng)
    elif family == "t_max":
        rays, t_max, meta = _finite_t_max(name, R)
    elif family == "lattice" and name == "box":
        rays, meta = _lattice()
    else:
        raise KeyError((name, family))
    return dict(rays=np.ascontiguousarray(rays), t_max=t_max, **meta)


def rays(name, family):
    """-> dict(rays [n, 6], t_max, ...), built once.  graze adds inst / eps (signed: > 0 inside) / far; t_max adds kind (0: t_max lies between the
    first and the second surface, 1: in front of the first); lattice adds kind (0: through mesh vertices and edges, 1: in a face plane, 2: along an edge)."""
    if (name, family) not in _RAYS:
        _RAYS[(name, family)] = _build(name, family)
    return _RAYS[(name, family)]


def _hull(p):
    """indices of the convex outline of the points p [n, 2], counter-clockwise (Andrew's monotone chain)"""
    order = np.lexsort((p[:, 1], p[:, 0]))

    def half(seq):
        out = []
        for i in seq:
            while len(out) >= 2:
                a, b = p[out[-2]], p[out[-1]]
                if (b[0] - a[0]) * (p[i][1] - a[1]) - (b[1] - a[1]) * (p[i][0] - a[0]) > 0.0:
                    break
                out.pop()
            out.append(i)
        return out[:-1]
    return half(list(order)) + half(list(order[::-1]))


def _graze(R, rng):
    """For every instance: from a near and from a far origin, look at its transformed vertices, take a vertex V of their convex outline and aim
    at V moved by eps x (the instance's size) -- inward along the median of a triangle that has V as a corner (the point lies in that triangle),
    outward along the outline's outer bisector at V (it lies outside the outline, so outside the silhouette)."""
    n_inst = len(R["verts"])
    per = 204 // n_inst
    out, inst, eps_of, far_of = [], [], [], []
    for i in range(n_inst):
        V, T = R["verts"][i], R["tris"][i]
        c, _, size = (x[0] for x in _boxes(R, [i]))
        size = float(size[0])
        for far in (0, 1):
            done = 0
            while done < per:
                if far:
                    o = _far_origins(R, rng, np.array([i]), c[None, :])[0]
                else:
                    o = c + _unit(rng, 1)[0] * rng.uniform(1.5, 4.0) * size
                w = (c - o) / np.linalg.norm(c - o)
                e1 = np.cross(w, rng.normal(size=3))
                e1 /= np.linalg.norm(e1)
                e2 = np.cross(w, e1)
                rel = V - o
                depth = rel @ w
                p = np.stack([rel @ e1, rel @ e2], axis=1) / depth[:, None]    # on the plane one unit in front of the origin
                hull = np.array(_hull(p))
                ua, ub = p[np.roll(hull, 1)] - p[hull], p[np.roll(hull, -1)] - p[hull]
                bis = ua / np.linalg.norm(ua, axis=1, keepdims=True) + ub / np.linalg.norm(ub, axis=1, keepdims=True)
                sharp = np.flatnonzero(np.linalg.norm(bis, axis=1) > 0.2)   # (a nearly straight piece of the outline has no safely outward direction)
                for j in rng.permutation(sharp)[:4]:
                    v = hull[j]
                    corner = T[(T == v).any(axis=1)]    # (where vertices coincide -- a box's edges -- the triangles of the one the outline names)
                    med = (p[corner].sum(axis=1) - 3.0 * p[v]) / 3.0
                    ea, eb = p[corner[:, 1]] - p[corner[:, 0]], p[corner[:, 2]] - p[corner[:, 0]]
                    area = np.abs(ea[:, 0] * eb[:, 1] - ea[:, 1] * eb[:, 0])
                    m = med[int(np.argmax(area))]
                    step = size / float(depth[v])       # the instance's size, seen on that plane
                    if np.linalg.norm(m) < 4e-3 * step or area.max() < 1e-4 * step * step or done == per:   # seen edge-on
                        continue
                    m = m / np.linalg.norm(m)
                    out_dir = -bis[j] / np.linalg.norm(bis[j])
                    for eps in GRAZE_EPS:
                        for sign, dirn in ((1.0, m), (-1.0, out_dir)):
                            q = p[v] + eps * step * dirn
                            out.append(np.concatenate([o, (w + q[0] * e1 + q[1] * e2) * float(depth[v])]))
                            inst.append(i)
                            eps_of.append(sign * eps)
                            far_of.append(far)
                    done += 1
    return np.array(out), dict(inst=np.array(inst), eps=np.array(eps_of), far=np.array(far_of))


def _finite_t_max(name, R):
    """The first 2 400 `near` rays that hit, each with its direction multiplied by the t at which it is to end, so that ONE t_max = 1 ends every
    ray where it should: even rows between the first and the second surface along the ray (the oracle's, twice as far as the first where there
    is no second, at most three times as far), odd rows half way to the first."""
    base = rays(name, "near")["rays"]
    t1 = R["full"].hit_batch(base, t_min=0.0)          # (the shortened rays see closer to their origins than t_min of the long ones)
    keep = np.flatnonzero((t1[:, 0] == 1.0) & np.isfinite(t1[:, 1]))[:2400]
    base, t1 = base[keep], t1[keep, 1]
    scaled = base.copy()
    scaled[:, 3:] *= t1[:, None]                       # the first surface now lies at t = 1 (within rounding)
    nxt = R["full"].hit_batch(scaled, t_min=1.0 + 1e-6)
    t2 = np.where(nxt[:, 0] == 1.0, nxt[:, 1] * t1, 5.0 * t1)
    kind = np.arange(len(base)) % 2
    end = np.where(kind == 0, np.minimum(0.5 * (t1 + t2), 3.0 * t1), 0.5 * t1)
    out = base.copy()
    out[:, 3:] *= end[:, None]
    return out, 1.0, dict(kind=kind)


def _lattice():
    """The box scene's dyadic rays: origins and directions are multiples of 1/8 (no input is rounded, every product of the triangle test is exact).
    kind 0: through the mesh's vertices, the midpoints of its edges and of its quads' diagonals (neighbouring triangles tie in t);
    kind 1: lying in a face's plane, through such points; kind 2: along the box's twelve edges and the mesh lines of its faces."""
    rng = _rng("box", "lattice")
    lo = np.array(BOX_AT)
    side = BOX_SCALE
    cell = side / BOX_N
    out, kind = [], []

    def dyadic(n):
        return rng.integers(1, 9, (n, 3)) / 8.0 * rng.choice([-1.0, 1.0], (n, 3))
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for face in (0.0, side):
            for i in range(2 * BOX_N + 1):
                for j in range(2 * BOX_N + 1):     # steps of half a cell: vertices, edge midpoints, quad centres
                    p = lo.copy()
                    p[axis] += face
                    p[u] += 0.5 * cell * i
                    p[v] += 0.5 * cell * j
                    for d in dyadic(4):
                        out.append(np.concatenate([p - 4.0 * d, d]))
                        kind.append(0)
                    if (i + j) % 3 == 0:
                        d = dyadic(1)[0]
                        d[axis] = 0.0
                        out.append(np.concatenate([p - 4.0 * d, d]))
                        kind.append(1)
            for line in range(BOX_N + 1):          # the face's mesh lines; the first and the last are edges of the box
                for along, across in ((u, v), (v, u)):
                    for sgn, length in ((1.0, 0.5), (-1.0, 2.0)):
                        p = lo.copy()
                        p[axis] += face
                        p[across] += cell * line
                        p[along] += (-1.0 if sgn > 0 else side + 1.5)
                        d = np.zeros(3)
                        d[along] = sgn * length
                        out.append(np.concatenate([p, d]))
                        kind.append(2)
    return np.array(out), dict(kind=np.array(kind))


# ---- lit instance scenes for whole frames under integrators 1 and 2 (tests/reach_scenes.py) -----------------------------------------------------
LIT_CAM = ((0.0, 4.0, -9.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 9.0)


def lit_items(B, n, inline, tie):
    """-> (items, lights): n instances of three small tori (f32 vertices: kernels 5 / 6 defer them; more than 32 instances take the 64-bit
    pending mask) in rings under a sphere light (B.SphereDiffuseLight: rtamd.World, or sppm_trace_cases.OB over the oracle), on a floor.
    inline: plus a Transform over a BVH of spheres, which kernels 5 / 6 enter in the lane.  tie: the floor is a rectangle (a scene with a
    rectangle or a cube takes the exact-tie variants), else a large sphere."""
    from rtamd import shapes

    def mesh(m, mat, seed):
        try:
            return B.Mesh(m[0], m[1], m[2], mat, bvh_seed=seed)
        except TypeError:
            return B.Mesh(m[0], m[1], m[2], mat, seed)

    grey = B.Lambertian(B.ConstantTexture((0.7, 0.7, 0.7)))
    red = B.Lambertian(B.ConstantTexture((0.7, 0.3, 0.2)))
    glass = B.Dielectric(1.5, B.ConstantTexture((1.0, 1.0, 1.0)))
    metal = B.Metal(B.ConstantTexture((0.8, 0.85, 0.9)), 0.1)
    objs = [mesh(shapes.torus(6, 8), grey, 1), mesh(shapes.torus(5, 10), glass, 2), mesh(shapes.torus(8, 6), metal, 3)]
    rng = _rng("lit", n)
    items = []
    for k in range(n):
        ring, a = k // 12, 2.0 * np.pi * (k % 12) / 12.0 + 0.3 * (k // 12)
        r = 1.6 + 1.3 * ring
        s = float(rng.uniform(0.35, 0.55))
        items.append(B.Transform(_t(rng.uniform(-180.0, 180.0, 3)), (s, s * float(rng.uniform(0.7, 1.3)), s),
                                 (float(r * np.cos(a)), 0.45 + 0.5 * (k % 3), float(r * np.sin(a))), objs[k % 3]))
    if inline:
        balls = [B.Sphere(_t(c), 0.12, glass if k % 3 == 0 else red) for k, c in enumerate(rng.uniform(-0.5, 0.5, size=(9, 3)))]
        try:
            grp = B.BVHNode_new(balls, bvh_seed=4)
        except TypeError:
            grp = B.BVHNode_new(balls, 4)
        items.append(B.Transform((10.0, 40.0, 0.0), (1.5, 1.0, 1.5), (0.0, 0.8, 0.0), grp))
    items.append(B.XZRectangle((-30.0, -30.0), (30.0, 30.0), 0.0, grey) if tie else B.Sphere((0.0, -1000.0, 0.0), 1000.0, grey))
    lt = B.SphereDiffuseLight((0.0, 7.5, 0.0), 3.0, (1.0, 1.0, 1.0), 300.0)  # (large: integrator 0 finds it at 1 spp in one pixel of five)
    return items + [lt], [lt]
