"""numpy restatement of rt_denoise_sym (include/rtamd.h, csrc/device/denoise.hip): rt_denoise with the symmetric luminance stop
sigma_luma * sqrt(v_p + v_q) + eps, f64, in the kernel's own operation order, so that the two agree bit for bit.  Everything but that one
term is tests/denoise_ref.py's: its _shift, H and luminance are used as they are, and mode 0 below is denoise_ref.atrous_pass restated
(test_denoise_sym.py holds the two equal).  pass_weights returns the weight every pixel gives each of its 25 taps, for the symmetry check."""
import numpy as np

from denoise_ref import DEFAULTS, H, _shift, luminance


def pass_weights(c, v, aov, step, cfg, mode=1):
    """[(dx, dy, w [H, W], valid [H, W])] in tap order: w = the weight pixel p gives its tap q = p + step (dx, dy).  mode 0: rt_denoise's
    stop (v may be None: no luminance weight), mode 1: rt_denoise_sym's (v is required)"""
    if mode == 1 and v is None:
        raise ValueError("the symmetric stop needs a variance")
    use_n = aov is not None and cfg["guides"] & 1
    use_z = aov is not None and cfg["guides"] & 2
    use_a = aov is not None and cfg["guides"] & 4
    lp = luminance(c)
    lden = cfg["sigma_luma"] * np.sqrt(v) + cfg["eps"] if (v is not None and mode == 0) else None
    zden = cfg["sigma_depth"] * float(step)
    taps = []
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
                    if mode == 1:
                        vq, _ = _shift(v, step * dx, step * dy)
                        den = cfg["sigma_luma"] * np.sqrt(v + vq) + cfg["eps"]
                    else:
                        den = lden
                    wl = 1.0 / (1.0 + np.abs(lp - luminance(cq)) / den)
                w = h * wn * wz * wa * wl
            taps.append((dx, dy, w, valid))
    return taps


def atrous_pass(c, v, aov, step, cfg, mode=1):
    """one pass at `step`: c [H, W, 3], v [H, W] (mode 0: or None), aov [H, W, 8] or None -> (c', v' or None)"""
    W = np.zeros(c.shape[:2])
    C = np.zeros(c.shape)
    V = np.zeros(c.shape[:2])
    for dx, dy, w, valid in pass_weights(c, v, aov, step, cfg, mode):
        cq, _ = _shift(c, step * dx, step * dy)
        W = np.where(valid, W + w, W)
        C = np.where(valid[..., None], C + w[..., None] * cq, C)
        if v is not None:
            vq, _ = _shift(v, step * dx, step * dy)
            V = np.where(valid, V + (w * w) * vq, V)
    return C / W[..., None], (V / (W * W) if v is not None else None)


def denoise(rgb, variance=None, aov=None, mode=1, **cfg):
    """-> (filtered rgb, filtered variance or None), as rt_denoise_sym (mode 1) or rt_denoise (mode 0) computes them"""
    c = dict(DEFAULTS)
    c.update(cfg)
    img = np.asarray(rgb, dtype=np.float64)
    v = None if variance is None else np.asarray(variance, dtype=np.float64)
    g = None if aov is None else np.asarray(aov, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(c["iterations"]):
            img, v = atrous_pass(img, v, g, 1 << i, c, mode)
    return img, v
