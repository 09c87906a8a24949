"""numpy restatement of rt_denoise (include/rtamd.h, csrc/device/denoise.hip), f64, in the kernel's own operation order, so that the
two agree bit for bit.  Every step below is one IEEE operation per pixel (the library is built with -ffp-contract=off); taps are visited
dy-major from -2 to 2, and a tap outside the image leaves the sums as they are."""
import numpy as np

H = (0.375, 0.25, 0.0625)
DEFAULTS = dict(iterations=5, normal_power_log2=7, sigma_depth=1.0, sigma_albedo=0.1, sigma_luma=4.0, eps=1e-10, guides=7)


def luminance(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def _shift(a, dx, dy):
    """a[y + dy, x + dx] at (y, x), and where that tap lies inside the image"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    valid = np.zeros((h, w), dtype=bool)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if ys.stop > ys.start and xs.stop > xs.start:
        out[yd, xd] = a[ys, xs]
        valid[yd, xd] = True
    return out, valid


def atrous_pass(c, v, aov, step, cfg):
    """one pass at `step`: c [H, W, 3], v [H, W] or None, aov [H, W, 8] or None -> (c', v' or None)"""
    use_n = aov is not None and cfg["guides"] & 1
    use_z = aov is not None and cfg["guides"] & 2
    use_a = aov is not None and cfg["guides"] & 4
    lp = luminance(c)
    lden = cfg["sigma_luma"] * np.sqrt(v) + cfg["eps"] if v is not None else None
    zden = cfg["sigma_depth"] * float(step)
    W = np.zeros(c.shape[:2])
    C = np.zeros(c.shape)
    V = np.zeros(c.shape[:2])
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, valid = _shift(c, step * dx, step * dy)
            h = H[abs(dx)] * H[abs(dy)]
            if dx == 0 and dy == 0:
                w = np.full(c.shape[:2], h)
            else:
                wn = wz = wa = wl = np.ones(c.shape[:2])
                if aov is not None:
                    gq, _ = _shift(aov, step * dx, step * dy)
                if use_n:
                    wn = np.fmax(0.0, (aov[..., 0] * gq[..., 0] + aov[..., 1] * gq[..., 1]) + aov[..., 2] * gq[..., 2])
                    for _ in range(cfg["normal_power_log2"]):
                        wn = wn * wn
                if use_z:
                    wz = 1.0 / (1.0 + np.abs(aov[..., 3] - gq[..., 3]) / zden)
                if use_a:
                    wa = 1.0 / (1.0 + ((np.abs(aov[..., 4] - gq[..., 4]) + np.abs(aov[..., 5] - gq[..., 5])) + np.abs(aov[..., 6] - gq[..., 6])) /
                                cfg["sigma_albedo"])
                if v is not None:
                    wl = 1.0 / (1.0 + np.abs(lp - luminance(cq)) / lden)
                w = h * wn * wz * wa * wl
            W = np.where(valid, W + w, W)
            C = np.where(valid[..., None], C + w[..., None] * cq, C)
            if v is not None:
                vq, _ = _shift(v, step * dx, step * dy)
                V = np.where(valid, V + (w * w) * vq, V)
    return C / W[..., None], (V / (W * W) if v is not None else None)


def denoise(rgb, variance=None, aov=None, **cfg):
    """-> (filtered rgb, filtered variance or None), as rt_denoise computes them"""
    c = dict(DEFAULTS)
    c.update(cfg)
    img = np.asarray(rgb, dtype=np.float64)
    v = None if variance is None else np.asarray(variance, dtype=np.float64)
    g = None if aov is None else np.asarray(aov, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(c["iterations"]):
            img, v = atrous_pass(img, v, g, 1 << i, c)
    return img, v
