"""Crafted inputs of the temporal step, shared by tests/test_temporal.py (the numpy restatement alone) and tests/test_temporal_gpu.py (the
kernel against it).  The cameras are chosen so that the reprojection is exact in f64: origin 0, lower-left corner (-1, -1, -1),
horizontal (2, 0, 0), vertical (0, 2, 0) and W - 1 = H - 1 = 8, so u = (x + 0.5) / 8 is exact, N0 = (0, 0, 4), and a fronto-parallel plane
at constant guide t = T = 4 gives s = T, r = (2 u, 2 st, 0), fx = x + (camera shift in pixels), fy = y without a rounding error."""
import numpy as np

W = H = 9
T = 4.0
NORMAL = (0.0, 0.0, 1.0)
ALBEDO = (0.5, 0.4, 0.3)


def camera(shift_px=0.0):
    """the exact camera, moved along `horizontal` by shift_px pixels of the plane at t = T: hor * (T / (W - 1)) per pixel = (1, 0, 0)"""
    o = np.array([shift_px * 2.0 * T / (W - 1), 0.0, 0.0])
    return dict(origin=o, llc=o + np.array([-1.0, -1.0, -1.0]), hor=np.array([2.0, 0.0, 0.0]), ver=np.array([0.0, 2.0, 0.0]))


def plane_guides():
    g = np.zeros((H, W, 8))
    g[..., 0:3] = NORMAL
    g[..., 3] = T
    g[..., 4:7] = ALBEDO
    g[..., 7] = 1.0
    return g


def base(shift_px=0.0, n_prev=3.0, seed=3):
    """a frame pair over the plane: (kwargs of temporal_ref.accumulate / rtamd.temporal_accumulate without the config)"""
    rng = np.random.default_rng(seed)
    hist = np.zeros((H, W, 6))
    hist[..., 0:3] = rng.uniform(0.1, 1.0, size=(H, W, 3))
    hist[..., 3] = rng.uniform(0.1, 1.0, size=(H, W))
    hist[..., 4] = hist[..., 3] ** 2 + rng.uniform(0.0, 0.1, size=(H, W))
    hist[..., 5] = n_prev
    return dict(rgb=rng.uniform(0.1, 1.0, size=(H, W, 3)), aov=plane_guides(), variance=rng.uniform(0.001, 0.01, size=(H, W)),
                prev_history=hist, prev_aov=plane_guides(), cam_cur=camera(shift_px), cam_prev=camera(0.0))


# One rejection each: name -> (shift in pixels, config, edit(inputs), pixel (y, x) that must reset).  Without the edit the pixel keeps its
# history (tests assert that too), so each row reaches exactly the test it is named after.
def _set(key, y, x, sl, value):
    def edit(k):
        k[key][y, x, sl] = value
    return edit


REJECTIONS = {
    # P = t d lies behind both cameras
    "behind_the_camera": (0.0, {}, _set("aov", 4, 4, 3, -T), (4, 4)),
    # the camera moved by one pixel: the last column looks at what the previous frame did not see (fx = W, and `fx < W` fails)
    "outside_the_frame": (1.0, {}, None, (4, W - 1)),
    # the tap's point lies half a T behind the pixel's tangent plane
    "plane": (0.0, {}, _set("prev_aov", 4, 4, 3, 1.5 * T), (4, 4)),
    "normal": (0.0, {}, _set("prev_aov", 4, 4, slice(0, 3), (1.0, 0.0, 0.0)), (4, 4)),
    "albedo": (0.0, {}, _set("prev_aov", 4, 4, 4, ALBEDO[0] + 0.3), (4, 4)),
    # fx = x + 0.875: the taps weigh 0.125 and 0.875; the heavy one (x + 1) has another normal, the light one alone is below min_weight
    "min_weight": (0.875, {}, _set("prev_aov", 4, 5, slice(0, 3), (1.0, 0.0, 0.0)), (4, 4)),
    "coverage_0": (0.0, {}, _set("aov", 4, 4, 7, 0.0), (4, 4)),
    "tap_coverage_0": (0.0, {}, _set("prev_aov", 4, 4, 7, 0.0), (4, 4)),
    "tap_history_n_0": (0.0, {}, _set("prev_history", 4, 4, 5, 0.0), (4, 4)),
    # guide t values for which the rule defines a reset: s = 0, and P = inf or NaN
    "t_0": (0.0, {}, _set("aov", 4, 4, 3, 0.0), (4, 4)),
    "t_inf": (0.0, {}, _set("aov", 4, 4, 3, np.inf), (4, 4)),
    "t_nan": (0.0, {}, _set("aov", 4, 4, 3, np.nan), (4, 4)),
    "t_inf_moved_camera": (0.5, {}, _set("aov", 4, 4, 3, np.inf), (4, 4)),
    "t_nan_moved_camera": (0.5, {}, _set("aov", 4, 4, 3, np.nan), (4, 4)),
}


def rejection(name):
    """-> (inputs with the edit, inputs without it, config, pixel)"""
    shift, cfg, edit, pix = REJECTIONS[name]
    k, plain = base(shift), base(shift)
    if edit:
        edit(k)
    return k, plain, cfg, pix


def orbit(look_from, look_at, deg):
    """look_from turned about look_at around the y axis by deg degrees (rtamd_render --orbit-step turns the same way)"""
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    d = np.asarray(look_from, dtype=np.float64) - np.asarray(look_at, dtype=np.float64)
    return tuple(np.asarray(look_at, dtype=np.float64) + np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]]))


def random_inputs(h, w, seed):
    """seeded random histories, guides and a camera pair that see the same noisy surface from nearby: most pixels reach the taps, a good
    part fails one test or another"""
    import temporal_ref
    rng = np.random.default_rng(seed)
    aspect = w / float(h)
    cam_prev = temporal_ref.camera_frame((0.3, 0.2, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, aspect)
    cam_cur = temporal_ref.camera_frame((0.3 + rng.uniform(-0.3, 0.3), 0.2 + rng.uniform(-0.3, 0.3), 5.0 + rng.uniform(-0.3, 0.3)),
                                        (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 0.0), (0.0, 1.0, 0.0), 40.0 + rng.uniform(-2, 2), aspect)

    def guides():
        g = np.zeros((h, w, 8))
        n = np.array([0.0, 0.0, 1.0]) + 0.25 * rng.standard_normal((h, w, 3))
        g[..., 0:3] = n / np.linalg.norm(n, axis=2, keepdims=True)
        g[..., 3] = 5.0 + rng.uniform(-0.15, 0.15, size=(h, w))   # about the plane z = 0 seen from z = 5 (|d| is near 1)
        g[..., 4:7] = 0.5 + rng.uniform(-0.1, 0.1, size=(h, w, 3))
        g[..., 7] = rng.integers(1, 5, size=(h, w)) / 4.0
        g[rng.random((h, w)) < 0.08] = 0.0   # pixels without a hit
        return g
    hist = np.zeros((h, w, 6))
    hist[..., 0:3] = rng.gamma(2.0, 0.3, size=(h, w, 3))
    hist[..., 3] = rng.gamma(2.0, 0.3, size=(h, w))
    hist[..., 4] = hist[..., 3] ** 2 + rng.gamma(1.0, 0.05, size=(h, w)) - 0.01   # (m2 - m1 m1 is negative now and then: the fmax)
    hist[..., 5] = rng.integers(0, 40, size=(h, w)).astype(np.float64)            # (0: no history; above max_history: the cap)
    return dict(rgb=rng.gamma(2.0, 0.3, size=(h, w, 3)), aov=guides(), variance=rng.gamma(1.0, 0.02, size=(h, w)), prev_history=hist,
                prev_aov=guides(), cam_cur=cam_cur, cam_prev=cam_prev)
