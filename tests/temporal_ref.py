"""numpy restatement of rt_temporal_accumulate (include/rtamd.h), vectorised over the pixels, with the header's operation
order: f64, only + - * / floor fmin fmax fabs and comparisons, so the HIP kernel (built without contraction) must agree bit for bit.
Every lane computes every step; the tests of the rule are masks, and what an untaken lane computed (NaN, inf, an index clipped into the
image) is never selected."""
import numpy as np

DEFAULTS = dict(alpha=0.2, plane_tolerance=0.02, normal_min=0.9, albedo_tolerance=0.25, min_weight=0.25, max_history=32)


def camera_frame(look_from, look_at, vup, vfov, aspect, focus_dist=1.0):
    """{origin, llc, hor, ver} of Camera::new (the four fields the step reads); good enough for tests that build their own cameras"""
    look_from, look_at, vup = (np.asarray(v, dtype=np.float64) for v in (look_from, look_at, vup))
    theta = vfov * np.pi / 180.0
    hh = np.tan(theta / 2.0)
    vh = 2.0 * hh
    vw = aspect * vh
    w = look_from - look_at
    w = w / np.sqrt(w @ w)
    u = np.cross(vup, w)
    u = u / np.sqrt(u @ u)
    v = np.cross(w, u)
    hor = focus_dist * vw * u
    ver = focus_dist * vh * v
    llc = look_from - hor / 2.0 - ver / 2.0 - focus_dist * w
    return dict(origin=look_from, llc=llc, hor=hor, ver=ver)


def frame_of_struct(f):
    """the same dict from an rtamd.rt_camera_frame"""
    return dict(origin=np.array(f.origin[:]), llc=np.array(f.lower_left_corner[:]), hor=np.array(f.horizontal[:]), ver=np.array(f.vertical[:]))


def luminance(rgb):
    return (0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1]) + 0.0722 * rgb[..., 2]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def centre(cam, W, H, x, y, t):
    """the point at parameter t on the ray through the centre of pixel (x, y); x, y integer arrays, t an array of their shape"""
    u = (x.astype(np.float64) + 0.5) / np.float64(W - 1)
    v = (y.astype(np.float64) + 0.5) / np.float64(H - 1)
    st = 1.0 - v
    d = ((cam["llc"] + cam["hor"] * u[..., None]) + cam["ver"] * st[..., None]) - cam["origin"]
    return cam["origin"] + d * t[..., None]


def accumulate(rgb, aov, cam_cur, variance=None, prev_history=None, prev_aov=None, cam_prev=None, info=None, **cfg):
    """-> (history [H, W, 6], variance [H, W]).  info: a dict that receives the masks of the rule's stages (kept: the pixels that kept
    their history; Wsum)."""
    c = dict(DEFAULTS)
    c.update(cfg)
    rgb = np.asarray(rgb, dtype=np.float64)
    aov = np.asarray(aov, dtype=np.float64)
    H, W = rgb.shape[:2]
    l = luminance(rgb)
    out = np.concatenate([rgb, l[..., None], (l * l)[..., None], np.ones((H, W, 1))], axis=2)
    a = np.ones((H, W))
    kept = np.zeros((H, W), dtype=bool)
    Wsum = np.zeros((H, W))
    if prev_history is not None:
        prev_history = np.asarray(prev_history, dtype=np.float64)
        prev_aov = np.asarray(prev_aov, dtype=np.float64)
        with np.errstate(all="ignore"):
            y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            ok = aov[..., 7] > 0.0
            P = centre(cam_cur, W, H, x, y, aov[..., 3])
            q = P - cam_prev["origin"]
            D0 = cam_prev["llc"] - cam_prev["origin"]
            N0 = cross(cam_prev["hor"], cam_prev["ver"])
            s = dot(q, N0) / dot(D0, N0)
            ok &= s > 0.0
            r = q / s[..., None] - D0
            up = dot(r, cam_prev["hor"]) / dot(cam_prev["hor"], cam_prev["hor"])
            stp = dot(r, cam_prev["ver"]) / dot(cam_prev["ver"], cam_prev["ver"])
            fx = up * np.float64(W - 1) - 0.5
            fy = (1.0 - stp) * np.float64(H - 1) - 0.5
            ok &= (fx > -1.0) & (fx < np.float64(W)) & (fy > -1.0) & (fy < np.float64(H))
            fx = np.where(ok, fx, 0.0)   # (lanes that failed a test carry no index)
            fy = np.where(ok, fy, 0.0)
            fx0, fy0 = np.floor(fx), np.floor(fy)
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            wx, wy = fx - fx0, fy - fy0
            reach = P - cam_cur["origin"]
            reach2 = dot(reach, reach)
            nc = aov[..., 0:3]
            A = np.zeros((H, W, 5))
            nmin = np.full((H, W), np.inf)
            tol2 = np.float64(c["plane_tolerance"]) * np.float64(c["plane_tolerance"])
            for j in (0, 1):
                for i in (0, 1):
                    xq, yq = x0 + i, y0 + j
                    valid = ok & (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
                    b = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
                    valid &= b > 0.0
                    xc, yc = np.clip(xq, 0, W - 1), np.clip(yq, 0, H - 1)
                    h = prev_history[yc, xc]
                    gq = prev_aov[yc, xc]
                    valid &= (h[..., 5] > 0.0) & (gq[..., 7] > 0.0)
                    Pq = centre(cam_prev, W, H, xc, yc, gq[..., 3])
                    dn = dot(Pq - P, nc)
                    valid &= dn * dn <= tol2 * reach2
                    valid &= dot(nc, gq[..., 0:3]) >= c["normal_min"]
                    valid &= (np.abs(aov[..., 4] - gq[..., 4]) + np.abs(aov[..., 5] - gq[..., 5])) + np.abs(aov[..., 6] - gq[..., 6]) <= c["albedo_tolerance"]
                    Wsum = np.where(valid, Wsum + b, Wsum)
                    A = np.where(valid[..., None], A + b[..., None] * h[..., 0:5], A)
                    nmin = np.where(valid, np.fmin(nmin, h[..., 5]), nmin)
            kept = ok & (Wsum >= c["min_weight"])
            n = np.fmin(nmin + 1.0, np.float64(c["max_history"]))
            ak = np.fmax(np.float64(c["alpha"]), 1.0 / n)
            hm = A / Wsum[..., None]
            new = np.concatenate([rgb, l[..., None], (l * l)[..., None]], axis=2)
            blended = (1.0 - ak)[..., None] * hm + ak[..., None] * new
            out[..., 0:5] = np.where(kept[..., None], blended, out[..., 0:5])
            out[..., 5] = np.where(kept, n, 1.0)
            a = np.where(kept, ak, 1.0)
    with np.errstate(all="ignore"):
        temporal = np.fmax(0.0, out[..., 4] - out[..., 3] * out[..., 3])
    Vf = np.where(out[..., 5] < 4.0, np.asarray(variance, dtype=np.float64), temporal) if variance is not None else temporal
    if info is not None:
        info["kept"] = kept
        info["Wsum"] = Wsum
    return out, Vf * a
