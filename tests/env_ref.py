"""numpy restatement of the background B(d) and of env sampling (include/rtamd.h "background", "env sampling"): the unit
vector, Sphere::get_uv through the oracle's deterministic acos / atan2, the texel and checker reads, B(d) of kinds 1-3, rtamd-sin-1, and the
env table, its draw and its pdf.  Everything is elementwise f64 in the order the header pins, so the results are compared bit for bit --
with the kernels (tests/test_background_gpu.py, tests/test_env_sampling_gpu.py) and with the oracle (tests/test_oracle_lights.py)."""
import numpy as np

PI = 3.14159265358979323846264338327950288
FRAC_1_PI = 0.318309886183790671537767526745028724


# ---- B(d) restated ------------------------------------------------------------------------------------------------------------------
def _unit(d):
    ln = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    return np.stack([d[..., 0] / ln, d[..., 1] / ln, d[..., 2] / ln], axis=-1)


def _sphere_uv(u):
    import oracle
    flat = u.reshape(-1, 3)
    uu = np.empty(len(flat))
    vv = np.empty(len(flat))
    for i, (x, y, z) in enumerate(flat):
        theta = oracle.det_acos(-y)
        phi = oracle.det_atan2(-z, x) + PI
        uu[i] = phi * FRAC_1_PI * 0.5
        vv[i] = theta * FRAC_1_PI
    return uu.reshape(u.shape[:-1]), vv.reshape(u.shape[:-1])


def _texel(img, u, v):  # ImageTexture: nearest texel, v flipped, clamped (Q11)
    h, w, _ = img.shape
    u = np.minimum(np.maximum(u, 0.0), 1.0)
    v = 1.0 - np.minimum(np.maximum(v, 0.0), 1.0)
    x = np.minimum(np.floor(w * u).astype(np.int64), w - 1)
    y = np.minimum(np.floor(h * v).astype(np.int64), h - 1)
    return img[y, x].astype(np.float64) / 255.0


def _checker_sines(p):
    return np.sin(10.0 * p[..., 0]) * np.sin(10.0 * p[..., 1]) * np.sin(10.0 * p[..., 2])


def _checker(c0, c1, p):  # CheckerTexture: .0 when sin(10x) sin(10y) sin(10z) < 0
    s = _checker_sines(p)
    return np.where((s < 0.0)[..., None], np.asarray(c0, dtype=np.float64), np.asarray(c1, dtype=np.float64))


def _background(spec, d):
    """B(d) in the order rtamd.h pins, for directions d [..., 3]"""
    kind, scale = spec["kind"], spec.get("scale", 1.0)
    u = _unit(d)
    if kind == 1:
        c = np.broadcast_to(np.asarray(spec["color"], dtype=np.float64), u.shape)
    elif kind == 2:
        t = 0.5 * (u[..., 1] + 1.0)
        c0, c1 = (np.asarray(x, dtype=np.float64) for x in spec["gradient"])
        c = (1.0 - t)[..., None] * c0 + t[..., None] * c1
    elif spec["tex"] == "image":
        c = _texel(spec["image"], *_sphere_uv(u))
    elif spec["tex"] == "noise":  # rec.p = u; the texture's own value is not restated: spec["value"](points [n, 3]) -> [n, 3]
        c = np.asarray(spec["value"](u.reshape(-1, 3)), dtype=np.float64).reshape(u.shape)
    else:
        c = _checker(spec["c0"], spec["c1"], u)
    return scale * c


# ---- rtamd.h "env sampling" restated ---------------------------------------------------------------------------------------------------
def det_sin(x):
    """rtamd-sin-1 (csrc/common/detsin.h) in numpy f64: IEEE + - * only, element-wise, no contraction"""
    invpio2, pio2_1, pio2_2, pio2_2t = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050630396597660e-11, 2.02226624879595063154e-21
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    x = np.asarray(x, dtype=np.float64)
    t = np.where(x < 0.0, -x, x)
    n = (t * invpio2 + 0.5).astype(np.int64)
    fn = n.astype(np.float64)
    r1 = t - fn * pio2_1
    w2 = fn * pio2_2
    r2 = r1 - w2
    w = fn * pio2_2t - ((r1 - r2) - w2)
    y0 = r2 - w
    y1 = (r2 - y0) - w
    z = y0 * y0
    v = z * y0
    rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    sin_k = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1)
    rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    cos_k = 1.0 - (0.5 * z - (z * rc - y0 * y1))
    res = np.where((n & 1) == 0, sin_k, cos_k)
    res = np.where((n & 2) != 0, -res, res)
    return np.where(x < 0.0, -res, res)


def env_dir(u, v):
    """the inverse of Sphere::get_uv; returns (d [..., 3], sin theta)"""
    theta = PI * v
    phi = (2.0 * PI) * u
    st = det_sin(theta)
    ct = det_sin(theta + PI / 2.0)
    cp = det_sin(phi + PI / 2.0)
    sp = det_sin(phi)
    x, y, z = np.broadcast_arrays(-(cp * st), -ct, sp * st)
    return np.stack([x, y, z], axis=-1), st


def table_ref(spec, W, H):
    """q [H, W] of rtamd.h, and the mask of the cells the restatement can vouch for (all of them, except near a checker's zeros)"""
    u = np.broadcast_to(((np.arange(W) + 0.5) / W)[None, :], (H, W))
    v = np.broadcast_to(((np.arange(H) + 0.5) / H)[:, None], (H, W))
    d, st = env_dir(u, v)
    c = _background(spec, d)
    w = ((0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]) * st
    w = np.where(w > 0.0, w, 0.0)
    wmax = w.max()
    q = np.zeros((H, W), dtype=np.uint64)
    if wmax > 0.0:
        q = np.where(w > 0.0, np.maximum(1.0, np.floor((w / wmax) * 4294967295.0)), 0.0).astype(np.uint64)
    sure = np.ones((H, W), dtype=bool)
    if spec["kind"] == 3 and spec["tex"] == "checker":
        sure = np.abs(_checker_sines(_unit(d))) >= 1e-9
    return q, sure


def sample_ref(q, xi):
    """the draws of rtamd.h from the table q [H, W] for xi [n, 4]: (directions [n, 3], cells (i, j) [n, 2])"""
    H, W = q.shape
    q = q.astype(np.uint64)
    rowcum = np.cumsum(q.sum(axis=1, dtype=np.uint64), dtype=np.uint64)
    total = int(rowcum[-1])
    cum = np.cumsum(q, axis=1, dtype=np.uint64)
    ii = np.empty(len(xi), dtype=np.int64)
    jj = np.empty(len(xi), dtype=np.int64)
    for k, (x1, x2, _, _) in enumerate(xi):
        t = min(total - 1, int(x1 * float(total)))
        j = int(np.searchsorted(rowcum, np.uint64(t), side="right"))  # the first row whose inclusive prefix sum exceeds t
        rt = int(cum[j, -1])
        tc = min(rt - 1, int(x2 * float(rt)))
        ii[k] = int(np.searchsorted(cum[j], np.uint64(tc), side="right"))
        jj[k] = j
    d, _ = env_dir((ii + xi[:, 2]) / W, (jj + xi[:, 3]) / H)
    return d, np.stack([ii, jj], axis=1)


def pdf_ref(q, d):
    H, W = q.shape
    total = int(q.astype(np.uint64).sum(dtype=np.uint64))
    n = _unit(d)
    u, v = _sphere_uv(n)
    i = np.clip(np.floor(W * u).astype(np.int64), 0, W - 1)
    j = np.clip(np.floor(H * v).astype(np.int64), 0, H - 1)
    s2 = 1.0 - n[..., 1] * n[..., 1]
    ok = s2 > 0.0
    p = (((q[j, i].astype(np.float64) / float(total)) * float(W)) * float(H)) / (((2.0 * PI) * PI) * np.sqrt(np.where(ok, s2, 1.0)))
    return np.where(ok, p, 0.0)
