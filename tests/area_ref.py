"""numpy restatement of the area lights of integrator 1 (include/rtamd.h "area lights"): the lowering of objects to
world-space triangles, the quantised selection weights, the draw and the pdf.  Everything is elementwise f64 in the order the header pins
(numpy's elementwise + - * / sqrt round once, like the library built without contraction), so the results are compared bit for bit."""
import numpy as np

AREA_TRI_FIELDS = ("a", "e0", "e1", "n", "area2", "q", "light")


def xf_point(t, p):
    """vec3.rs:174-178 (w = 1) with the 4x4 row-major `t`"""
    t = np.asarray(t, dtype=np.float64).reshape(4, 4)
    return np.array([t[i, 0] * p[0] + t[i, 1] * p[1] + t[i, 2] * p[2] + t[i, 3] * 1.0 for i in range(3)], dtype=np.float64)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def lower_vertices(world, obj, info, xforms=()):
    """The (a, b, c) vertex triples of `obj` in lowering order, walking the object graph through World.describe.  info: what describe does
    not report -- 'trans': {transform id: 4x4}, 'pos': the vertex array of rt_object_triangle leaves, 'mesh': {mesh object id: (pos, idx)}."""
    kind, d = world.describe(obj)
    out = []

    def emit(a, b, c):
        tri = []
        for p in (a, b, c):
            p = np.asarray(p, dtype=np.float64)
            for t in reversed(xforms):  # innermost first
                p = xf_point(t, p)
            tri.append(p)
        out.append(tri)

    if kind == "Rect":
        a0, b0, a1, b1, k = d["v"][:5]
        corner = {2: lambda a, b: (a, b, k), 1: lambda a, b: (a, k, b), 0: lambda a, b: (k, a, b)}[d["axis"]]
        p00, p10, p01, p11 = corner(a0, b0), corner(a1, b0), corner(a0, b1), corner(a1, b1)
        emit(p00, p10, p11)
        emit(p00, p11, p01)
    elif kind == "Triangle":
        ia, ib, ic = (int(x) for x in d["v"][:3])
        pos = info["pos"]
        emit(pos[ia], pos[ib], pos[ic])
    elif kind == "Mesh":
        pos, idx = info["mesh"][obj]
        for ia, ib, ic in idx:  # the order of `indices`, not of the inner BVH
            emit(pos[ia], pos[ib], pos[ic])
    elif kind == "Transform":
        out += lower_vertices(world, d["children"][0], info, tuple(xforms) + (info["trans"][obj],))
    elif kind in ("Cube", "HitableList", "BVHNode"):
        for c in d["children"]:
            out += lower_vertices(world, c, info, xforms)
    else:
        raise ValueError("not an area light leaf: " + kind)
    return out


def lower(world, lights, info):
    """The table rt_scene_area_light_tris reports for the area light list `lights`, as a dict of arrays (AREA_TRI_FIELDS), and the
    per-light totals (python ints)."""
    rows = {k: [] for k in AREA_TRI_FIELDS}
    totals = []
    for li, obj in enumerate(lights):
        area2 = []
        for a, b, c in lower_vertices(world, obj, info):
            e0, e1 = b - a, c - a
            n = _cross(e0, e1)
            with np.errstate(all="ignore"):
                a2 = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
            if not (a2 > 0.0) or not np.isfinite(a2):
                continue  # degenerate: dropped
            for k, v in zip(("a", "e0", "e1", "n", "light"), (a, e0, e1, n, li)):
                rows[k].append(v)
            area2.append(a2)
        area2 = np.array(area2, dtype=np.float64)
        q = np.maximum(1.0, np.floor(area2 / area2.max() * 4294967295.0)).astype(np.uint64)
        rows["area2"] += list(area2)
        rows["q"] += [int(x) for x in q]
        totals.append(int(sum(int(x) for x in q)))
    tab = {k: np.array(rows[k], dtype=np.float64).reshape(-1, 3) for k in ("a", "e0", "e1", "n")}
    tab["area2"] = np.array(rows["area2"], dtype=np.float64)
    tab["q"] = np.array(rows["q"], dtype=np.uint32)
    tab["light"] = np.array(rows["light"], dtype=np.int32)
    return tab, totals


def table_of(tris):
    """the same dict from World.area_light_tris()'s record array"""
    return {k: np.array(tris[k]) for k in AREA_TRI_FIELDS}


def _lights(tab):
    """per light: (first, count, inclusive prefix sums uint64, total)"""
    out = []
    for li in range(int(tab["light"].max()) + 1):
        idx = np.nonzero(tab["light"] == li)[0]
        cum = np.cumsum(tab["q"][idx].astype(np.uint64), dtype=np.uint64)
        out.append((int(idx[0]), len(idx), cum, int(cum[-1])))
    return out


def sample(tab, o_xi):
    """rt_debug_area_sample_device's directions: o_xi [n, 7] = o, xi0 (the light), xi1..xi3 -> dir [n, 3]"""
    o_xi = np.asarray(o_xi, dtype=np.float64)
    lights = _lights(tab)
    m = len(lights)
    o, xi0, xi1, u, v = o_xi[:, :3], o_xi[:, 3], o_xi[:, 4], o_xi[:, 5].copy(), o_xi[:, 6].copy()
    li = np.minimum(m - 1, (xi0 * float(m)).astype(np.uint32).astype(np.int64))
    k = np.zeros(len(o), dtype=np.int64)
    for l, (first, count, cum, total) in enumerate(lights):
        sel = li == l
        t = np.minimum(np.uint64(total - 1), (xi1[sel] * float(total)).astype(np.uint64))
        k[sel] = first + np.searchsorted(cum, t, side="right")  # the first inclusive prefix sum that exceeds t
    flip = u + v > 1.0
    u[flip] = 1.0 - u[flip]
    v[flip] = 1.0 - v[flip]
    p = tab["a"][k] + (tab["e0"][k] * u[:, None] + tab["e1"][k] * v[:, None])
    return p - o


def tri_hit(a, e0, e1, o, d, t_min=0.001, t_max=np.inf):
    """Triangle::hit (mesh.rs:57-102) as the kernels compute it: (accepted, t)"""
    with np.errstate(all="ignore"):
        s0 = _cross(d, e1)
        dd = _dot(s0, e0)
        div = 1.0 / dd
        dv = o - a
        b1 = _dot(dv, s0) * div
        s1 = _cross(dv, e0)
        b2 = _dot(d, s1) * div
        t = _dot(e1, s1) * div
        reject = (dd == 0.0) | (b1 < 0.0) | (b1 > 1.0) | (b2 < 0.0) | (b1 + b2 > 1.0) | (t < t_min) | (t > t_max)
    return ~reject, t


def pdf(tab, rays):
    """rt_debug_area_pdf_device: rays [n, 6] = o, d -> the sum over all area lights, in list order, of each light's pdf"""
    rays = np.asarray(rays, dtype=np.float64)
    o, d = rays[:, :3], rays[:, 3:6]
    total_sum = np.zeros(len(rays), dtype=np.float64)
    with np.errstate(all="ignore"):
        d2 = _dot(d, d)
        dl = np.sqrt(d2)
        for first, count, cum, total in _lights(tab):
            s = np.zeros(len(rays), dtype=np.float64)
            for k in range(first, first + count):
                hit, t = tri_hit(tab["a"][k][None, :], tab["e0"][k][None, :], tab["e1"][k][None, :], o, d)
                area2 = tab["area2"][k]
                dist2 = (t * t) * d2
                cosine = np.abs(_dot(d, tab["n"][k][None, :]) / (dl * area2))
                term = ((float(tab["q"][k]) / float(total)) * dist2) / (cosine * (0.5 * area2))
                s = np.where(hit & (cosine > 0.0), s + term, s)
            total_sum = total_sum + s
    return total_sum
