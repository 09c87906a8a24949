"""rt_ao_render restated over the oracle (include/rtamd.h "ambient occlusion"): oracle.camera_rays for the camera rays,
oracle.Scene.hit_batch for their first hits and for the occlusion rays, oracle.sample_helper(1, ..) for the unit vector a Lambertian
scatters with, oracle.Scene.background for B(d).  Every sum runs in (s, k) order from 0.0 in f64, as the kernel's.

ao(scene, W, H, ...) -> dict(ao [H, W, 8], occluded, unoccluded): the frame and how many occlusion rays went either way.  Results are
kept per (scene object, parameters): the tests share them and leave them unchanged."""
import numpy as np

AO_STREAM = 0x9E3779B97F4A7C15
_MASK = (1 << 64) - 1
_CACHE = {}


def directions(normals, pix, seed, s, K):
    """the K occlusion directions of each hit of sample s: normals [n, 3], pix [n] -> [n, K, 3]"""
    import oracle
    out = np.zeros((len(pix), K, 3))
    for i, (n, p) in enumerate(zip(normals, pix)):
        for k in range(K):
            u = oracle.sample_helper(1, key=((seed ^ AO_STREAM) & _MASK, int(p), s * K + k))
            v = n + u
            if abs(v[0]) < 1e-8 and abs(v[1]) < 1e-8 and abs(v[2]) < 1e-8:     # near_zero, vec3.rs:92-95
                v = n.copy()
            out[i, k] = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return out


def background(scene, d, has_background):
    """B(d) [n, 3]; zeros where the scene has no background (has_background False: the oracle is not asked -- it answers rc -1 there)"""
    if len(d) == 0 or not has_background:
        return np.zeros((len(d), 3))
    return scene.background(d)


def has_background(scene):
    """does oracle.Scene.background answer for this scene?  rc -1 is `no background`; any other failure is raised"""
    import oracle
    try:
        scene.background(np.array([[0.0, 1.0, 0.0]]))
        return True
    except oracle.OracleError as e:
        if "rc=-1 " not in str(e):
            raise
        return False


def ao(scene, W, H, ao_spp=4, rays_per_hit=4, max_distance=float("inf"), seed=1, t_min=1e-3):
    key = (id(scene), W, H, ao_spp, rays_per_hit, max_distance, seed, t_min)
    if key in _CACHE:
        return _CACHE[key][1]
    K = rays_per_hit
    npix = W * H
    open_n = np.zeros(npix)
    bent = np.zeros((npix, 3))
    amb = np.zeros((npix, 3))
    hits = np.zeros(npix)
    n_occ = n_open = 0
    has_bg = has_background(scene)
    for s in range(ao_spp):
        rays = scene.camera_rays(W, H, seed, sample=s).reshape(npix, 6)
        rec = scene.hit_batch(rays, t_min)
        pix = np.flatnonzero(rec[:, 0] != 0)
        if len(pix) == 0:
            continue
        p, n = rec[pix, 2:5], rec[pix, 5:8]
        d = directions(n, pix, seed, s, K)
        hits[pix] += 1.0
        for k in range(K):
            occ = scene.hit_batch(np.concatenate([p, d[:, k]], axis=1), t_min, t_max=max_distance)[:, 0] != 0
            free = ~occ
            n_occ += int(occ.sum())
            n_open += int(free.sum())
            B = background(scene, d[free, k], has_bg)
            open_n[pix[free]] += 1.0
            bent[pix[free]] += d[free, k]
            amb[pix[free]] += B
    out = np.zeros((npix, 8))
    hit = hits > 0
    N = hits[hit] * float(K)
    out[hit, 0] = open_n[hit] / N
    out[hit, 1:4] = bent[hit] / N[:, None]
    out[hit, 4:7] = amb[hit] / N[:, None]
    out[hit, 7] = hits[hit] / float(ao_spp)
    res = dict(ao=out.reshape(H, W, 8), occluded=n_occ, unoccluded=n_open)
    res["ao"].setflags(write=False)
    _CACHE[key] = (scene, res)      # (the scene is kept alive: its id is the key)
    return res
