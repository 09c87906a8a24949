"""The families of tests/shade_cases.py without a device: the ORACLE's shading, textures and object lights against independent references,
and the coverage every family promises -- so that tests/test_shade_gpu.py, which compares the device with the oracle on the same rows,
cannot pass vacuously.  Also the refusals of the three diagnostics, which are decided on the host."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import shade_cases as sc

RT_ERR_ARG, RT_ERR_NOT_COMMITTED, RT_ERR_NO_DEVICE = -1, -8, -9


def _shade(name):
    o, _ = sc.oracle_scene()
    f = sc.family(name)
    out, draws = o.shade(f["rows"], f["keys"])
    return f, out, draws


def test_families_are_deterministic_and_of_moderate_size():
    for name in list(sc.SHADE_FAMILIES) + ["light_samples", "light_pdf_rays"]:
        a = sc.family(name)
        sc._CACHE.pop(name)
        b = sc.family(name)
        for k in a:
            assert a[k].shape == b[k].shape and (a[k].dtype.kind in "US" and (a[k] == b[k]).all() or sc.same(a[k], b[k]).all() if a[k].dtype.kind == "f" else (a[k] == b[k]).all()), (name, k)
        assert len(next(iter(a.values()))) < 6000


def test_checker_sign_against_400_bit_sines():
    """CheckerTexture: .0 where the f64 product of the three correctly rounded sines of 10 p is negative, .1 elsewhere (a NaN sine included)"""
    import mpmath
    f, out, _ = _shade("checker")
    cache = {}

    def sin(a):
        if not math.isfinite(a):
            return math.nan
        if a not in cache:
            with mpmath.workprec(400):
                cache[a] = float(mpmath.sin(mpmath.mpf(a)))
        return cache[a]
    neg = np.array([sin(10.0 * p[0]) * sin(10.0 * p[1]) * sin(10.0 * p[2]) < 0.0 for p in f["points"]])
    want = np.where(neg[:, None], np.array(sc.CHECK_COLORS[0]), np.array(sc.CHECK_COLORS[1]))
    assert np.array_equal(out[:, 5:8], want), "%d of %d points disagree" % ((out[:, 5:8] != want).any(axis=1).sum(), len(want))
    assert neg.any() and not neg.all() and (out[:, 19] == 0).all()
    # the points straddle the device's fallback margin: 10 x / pi within 1e-9 of an integer, and farther
    r = 10.0 * f["points"][:, 0] / math.pi
    r = r[np.isfinite(r)]
    frac = np.abs(r - np.round(r))[np.abs(r) < 2.0 ** 18]
    assert (frac < 1e-9).sum() > 500 and ((frac > 1e-9) & (frac < 1e-8)).sum() > 100 and (np.abs(r) >= 2.0 ** 18).any()


def test_image_texel_against_exact_python():
    """ImageTexture: texel (min(floor(fl(w clamp(u))), w - 1), the same of 1 - clamp(v)), a NaN clamped to 0"""
    f, out, _ = _shade("image")
    imgs = sc.images()

    def clamp(x):
        return 0.0 if math.isnan(x) else min(max(x, 0.0), 1.0)
    want, cells = [], set()
    for row, k in zip(f["rows"], f["tex"]):
        w, h = sc.IMG_SIZES[k]
        x = min(int(math.floor(float(w) * clamp(row[15]))), w - 1)
        y = min(int(math.floor(float(h) * (1.0 - clamp(row[16])))), h - 1)
        want.append(imgs[k][y, x] / 255.0)
        cells.add((k, x, y))
    assert np.array_equal(out[:, 5:8], np.array(want))
    for k, (w, h) in enumerate(sc.IMG_SIZES):   # every column and every row of every image is read
        assert {c[1] for c in cells if c[0] == k} == set(range(w)) and {c[2] for c in cells if c[0] == k} == set(range(h))


def test_marble_against_a_restatement_with_integer_lattice_indices():
    """noise_texture::value with the lattice index floor(x) mod 256 of the mathematical integer (include/rtamd.h): Python integers"""
    import oracle
    f, out, _ = _shade("noise")
    vec, perm = sc.perlin_tables(sc.NOISE_SEED)
    det_sin = oracle.lib().orc_det_sin
    want = np.array([sc.marble(vec, perm, sc.NOISE_SCALE, p, det_sin) for p in f["points"]])
    assert sc.same(out[:, 5], want).all(), np.flatnonzero(~sc.same(out[:, 5], want))
    assert sc.same(out[:, 6], want).all() and sc.same(out[:, 7], want).all()
    big = np.abs(f["points"]).max(axis=1) >= 2.0 ** 25       # where 64 x leaves the range of int
    assert big.sum() > 100 and len(set(want[big & np.isfinite(f["points"]).all(axis=1)])) > 20   # ... and the value still varies
    assert (want[~np.isfinite(f["points"]).all(axis=1)] == 0.5).all()
    assert sc.lattice_index(-0.5) == 255 and sc.lattice_index(2.0 ** 31 + 0.5) == 0 and sc.lattice_index(-(2.0 ** 40) - 3.0) == 253 and sc.lattice_index(1e300) == 0


def test_lambertian_takes_both_sides_of_near_zero():
    f, out, draws = _shade("lambertian")
    n = f["rows"][:, 11:14]
    u = np.array([sc.unit(sc.sphere_sample(k)) for k in f["keys"]])
    d = n + u
    near = (np.abs(d) < 1e-8).all(axis=1)
    assert np.array_equal(out[:, 2:5], np.where(near[:, None], n, d))
    assert near.sum() > 64 and (~near).sum() > 64 and (d[near] == 0).all(axis=1).sum() == 32
    assert (out[:, 0] == 1).all() and (out[:, 1] == 1).all() and (out[:, 19] == 0).all()
    light = f["rows"][:, 0] == sc.oracle_scene()[1]["light"]
    assert light.any() and (out[light, 8:11] == (5.0, 4.0, 3.0)).all() and (out[~light, 8:11] == 0).all()
    assert np.array_equal(out[light, 5:8], np.full((light.sum(), 3), 1.0 * 0.318309886183790671537767526745028724))


def test_metal_absorbs_scatters_and_meets_vectors_without_length():
    f, out, draws = _shade("metal")
    rows, tag = f["rows"], f["tag"]
    zero = out[:, 19] == 1
    assert np.array_equal(zero, np.isin(tag, ["len0", "len5e-324", "len1e-200"]))      # |d|^2 underflows to 0 for all three
    ok = ~zero
    fuzz = np.array([sc.FUZZ[int(m) - sc.oracle_scene()[1]["metal0"]] for m in rows[:, 0]])
    want_scatter = np.zeros(len(rows), dtype=bool)
    for i in np.flatnonzero(ok):
        u = np.zeros(3) if tag[i] == "len1e200" else sc.unit(rows[i, 5:8])     # |d|^2 overflows: d / inf = 0
        n, rs = rows[i, 11:14], sc.sphere_sample(f["keys"][i])
        dn = u[0] * n[0] + u[1] * n[1] + u[2] * n[2]
        d = (u - n * (2.0 * dn)) + rs * fuzz[i]
        dot = d[0] * n[0] + d[1] * n[1] + d[2] * n[2]
        want_scatter[i] = dot > 0.0
        if want_scatter[i]:
            assert np.array_equal(out[i, 2:5], d)
        if tag[i] == "len1" and fuzz[i] in (0.0, 1.0):
            assert dot == 0.0                                                           # the exact zero: Absorb
    assert np.array_equal(out[ok, 0] == 1, want_scatter[ok])
    assert want_scatter.sum() > 50 and (ok & ~want_scatter).sum() > 50 and zero.sum() > 50
    assert (draws[ok] >= 2).all() and (out[:, 1] == 0).all()


def test_dielectric_families_hold_both_outcomes():
    f, out, draws = _shade("dielectric")
    tag, rows = f["tag"], f["rows"]
    assert (out[:, 19] == 0).all() and (out[:, 0] == 1).all() and set(draws) == {0, 1}
    reflected = out[:, 3] > 0                               # the normal is +y and the ray comes down, except for the rows named over1 / cos0
    crit = tag == "critical"
    assert crit.sum() == 3 * 32                             # ir 1.5 from inside, 1/1.5 from outside, 2.4 from inside
    for key in {tuple(k) for k in f["keys"][crit]}:
        m = crit & (f["keys"] == key).all(axis=1)
        assert (draws[m] == 0).sum() >= 12 and (draws[m] == 1).sum() >= 12
        assert reflected[m & (draws == 0)].all()           # total reflection: no draw
    # the draw is consumed exactly where refraction is possible: ratio * sin > 1 restated
    ids = sc.oracle_scene()[1]
    for i in np.flatnonzero(crit | (tag == "normal") | (tag == "schlick")):
        ir = sc.IRS[int(rows[i, 0]) - ids["glass0"]]
        ratio = (1.0 / ir) if rows[i, 14] else ir
        u = sc.unit(rows[i, 5:8])
        cos = min(-u[0] * 0.0 + -u[1] * 1.0 + -u[2] * 0.0, 1.0)
        assert draws[i] == (0 if ratio * math.sqrt(1.0 - cos * cos) > 1.0 else 1)
    sch = tag == "schlick"
    assert sch.sum() == 8 * 16 and (draws[sch] == 1).all()
    for key in {tuple(k) for k in f["keys"][sch]}:
        m = sch & (f["keys"] == key).all(axis=1)
        assert reflected[m].sum() >= 6 and (~reflected[m]).sum() >= 6
    over = tag == "over1"
    assert over.sum() == 32 and all(-(sc.unit(r[5:8]) * r[11:14]).sum() > 1.0 or True for r in rows[over])
    u = np.array([sc.unit(r[5:8]) for r in rows[over]])
    assert ((u * u)[:, 0] + (u * u)[:, 1] + (u * u)[:, 2] > 1.0).all()
    assert (tag == "cos0").sum() == 16 and np.isfinite(out[:, 2:5]).all()


def test_isotropic_scatters_into_the_sphere_sample():
    f, out, draws = _shade("isotropic")
    assert np.array_equal(out[:, 2:5], np.array([sc.sphere_sample(k) for k in f["keys"]]))
    assert (out[:, 0] == 1).all() and (out[:, 1] == 0).all() and (out[:, 11] == 0).all() and np.array_equal(out[:, 5:8], np.tile((0.2, 0.5, 0.8), (8, 1)))


def _pdf_reference(o, d):
    """light_pdf_value of the three lights restated: a hit within [0.001, inf) of the sphere / the rectangle, then the solid-angle density"""
    def sphere(c, r):
        oc = o - np.array(c)
        a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        hb = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2]
        cc = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - r * r
        disc = hb * hb - a * cc
        if disc < 0.0:
            return 0.0
        with np.errstate(all="ignore"):
            sq = np.sqrt(np.float64(disc))
            t = (-hb - sq) / np.float64(a)
            if not (t >= 0.001):
                t = (-hb + sq) / np.float64(a)
            if not (t >= 0.001):
                return 0.0
            co = np.array(c) - o
            cmax = np.sqrt(np.float64(1.0) - r * r / np.float64(co[0] * co[0] + co[1] * co[1] + co[2] * co[2]))
            return float(np.float64(1.0) / (2.0 * math.pi * (1.0 - cmax)))

    def rect(lo, hi, y):
        with np.errstate(all="ignore"):
            t = (np.float64(y) - o[1]) / np.float64(d[1])
            if t < 0.001 or t > math.inf:
                return 0.0
            p = o + d * t
            if p[0] < lo[0] or p[0] > hi[0] or p[2] < lo[1] or p[2] > hi[1]:
                return 0.0
            sq = np.float64(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            return float((t * t * sq) / (np.abs(d[1] / np.sqrt(sq)) * ((hi[0] - lo[0]) * (hi[1] - lo[1]))))
    return [sphere(*sc.LIGHT0), rect(*sc.LIGHT1), sphere(*sc.LIGHT2)]


def test_object_lights_from_where_they_go_wrong():
    o, _ = sc.oracle_scene()
    fam = sc.family("light_samples")
    out, draws = o.light_sample(fam["o_light"], fam["keys"])
    tag = fam["tag"]
    assert np.array_equal(out[:, 3] == 1, tag == "centre") and (tag == "centre").sum() == 6
    assert {"surface", "inside", "far", "basis", "rect", "generic"} <= set(tag)
    assert sorted(abs(wx) for wx, org in sc.basis_switch_origins() if org is not None) == sorted([sc.ulps(0.9, -1), 0.9, sc.ulps(0.9, 1)] * 2)
    rect = fam["o_light"][:, 3] == 1
    assert (draws[rect] == 2).all() and (draws[~rect & (out[:, 3] == 0)] >= 2).all() and (draws[~rect] > 2).any()
    # the rectangle's samples restated: (x0 + (x1 - x0) u, y, z0 + (z1 - z0) v) - o with the stream's two gen_range(0, 1)
    import oracle
    (x0, z0), (x1, z1), y = sc.LIGHT1
    for i in np.flatnonzero(rect):
        u, v = oracle.rng_range(*[int(k) for k in fam["keys"][i]], 2, 0.0, 1.0)
        assert np.array_equal(out[i, :3], np.array([x0 + (x1 - x0) * u, y, z0 + (z1 - z0) * v]) - fam["o_light"][i, :3])
    rays = sc.family("light_pdf_rays")
    pdf = o.light_pdf(rays["rays"])
    want = np.array([_pdf_reference(r[:3], r[3:]) for r in rays["rays"]])
    assert sc.same(pdf, want).all(), np.argwhere(~sc.same(pdf, want))[:10]
    own = rays["own"]
    sampled = own >= 0
    own_pdf = pdf[np.flatnonzero(sampled), own[sampled]]
    assert (own_pdf > 0).sum() * 2 >= sampled.sum(), "%d of %d sampled directions have a pdf > 0 for their own light" % ((own_pdf > 0).sum(), sampled.sum())
    assert np.isnan(pdf).any() and np.isinf(pdf).any()
    edge = pdf[~sampled, 1]
    assert (edge > 0).sum() > 100 and (edge == 0).sum() > 100    # through the exact edge and corner: inside; one ulp beyond: outside


def test_mixture_rows_continue_end_and_sum_three_terms_in_order():
    o, _ = sc.oracle_scene()
    f, out, draws = _shade("mixture")
    tag = f["tag"]
    assert (out[:, 11] == 1).all() and (out[:, 19] == 0).all()
    cont = out[:, 12] == 1
    assert cont.sum() > 100 and (~cont).sum() > 100
    assert (~cont[tag == "in_plane"]).sum() >= 4 and cont[tag == "opposite"].any() and (~cont[tag == "opposite"]).any()
    pdf = o.light_pdf(np.concatenate([f["rows"][:, 8:11], out[:, 16:19]], axis=1))
    # the weight restated from the per-light pdfs, added in list order
    n, d = f["rows"][:, 11:14], out[:, 16:19]
    with np.errstate(all="ignore"):
        ud = np.array([sc.unit(v) for v in d])
        cosine = n[:, 0] * ud[:, 0] + n[:, 1] * ud[:, 1] + n[:, 2] * ud[:, 2]
        spdf = np.where(cosine < 0, 0.0, cosine / math.pi)
        lp = ((0.0 + pdf[:, 0]) + pdf[:, 1]) + pdf[:, 2]
        wgt = spdf / (0.5 * (lp / 3.0) + 0.5 * spdf)
    assert np.array_equal(cont, wgt > 0)
    att = out[:, 5:8]
    assert sc.same(out[cont, 13:16], ((1.0 * att) * wgt[:, None])[cont]).all()
    zero_cos = (tag == "cos0") & (cosine == 0)              # the rows of that family that took the cosine half
    assert zero_cos.sum() >= 24 and (~cont[zero_cos]).all()
    assert np.isnan(wgt[zero_cos]).any() and (wgt[zero_cos] == 0).any()                      # 0 / 0 without a light there, 0 / pdf with one
    three = (pdf > 0).all(axis=1) & np.isfinite(pdf).all(axis=1)
    order = np.array([any(((0.0 + p[a]) + p[b]) + p[c] != ((0.0 + p[0]) + p[1]) + p[2] for a, b, c in itertools.permutations(range(3))) for p in pdf])
    assert (three & order).any(), "no row whose three pdf terms add up differently in another order (%d rows with three terms)" % three.sum()
    assert (three & order & cont).any()


def test_oracle_scatter_and_shade_agree():
    """orc_scatter, which the older tests call, and the batch entry point are one computation"""
    o, _ = sc.oracle_scene()
    for name in ("lambertian", "metal", "dielectric"):
        f, out, _ = _shade(name)
        for i in range(0, len(out), 7):
            r = f["rows"][i]
            if out[i, 19]:
                continue
            s = o.scatter(int(r[0]), r[2:5], r[5:8], r[8:11], r[11:14], bool(r[14]), (r[15], r[16]), key=tuple(int(k) for k in f["keys"][i]))
            assert s["scattered"] == bool(out[i, 0])
            if s["scattered"]:
                assert np.array_equal(s["dir"], out[i, 2:5]) and np.array_equal(s["attenuation"], out[i, 5:8])
            assert np.array_equal(s["emitted"], out[i, 8:11])


# ---- refusals of the diagnostics: decided on the host, before a device is asked for -------------------------------------------------------
def test_diagnostics_are_declared_exported_and_refuse_bad_arguments():
    import rtamd
    from test_abi_symbols import declared_symbols
    for sym in ("rt_debug_shade_device", "rt_debug_light_sample_device", "rt_debug_light_pdf_device"):
        assert sym in declared_symbols() and sym in rtamd.ABI_SYMBOLS and hasattr(C.CDLL(rtamd.LIB_PATH), sym)
    w, _, ids = sc.product_world()
    L, dp, kp = w.L, C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    rows = sc.family("isotropic")["rows"][:4].copy()
    rows[:, 1] = 1.0
    keys = np.ones((4, 3), dtype=np.uint64)
    out = np.zeros((4, 22))
    ol = np.array([[0.0, 0.0, 0.0, 1.0]] * 4)
    rays = np.array([[0.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * 4)

    def shade(h, n, x, k, y):
        return L.rt_debug_shade_device(h, 0, n, x.ctypes.data_as(dp) if x is not None else None, k.ctypes.data_as(kp) if k is not None else None,
                                       y.ctypes.data_as(dp) if y is not None else None)

    def sample(h, n, x, k, y):
        return L.rt_debug_light_sample_device(h, 0, n, x.ctypes.data_as(dp) if x is not None else None, k.ctypes.data_as(kp) if k is not None else None,
                                              y.ctypes.data_as(dp) if y is not None else None)

    def pdf(h, n, x, y):
        return L.rt_debug_light_pdf_device(h, 0, n, x.ctypes.data_as(dp) if x is not None else None, y.ctypes.data_as(dp) if y is not None else None)
    good = 0 if rtamd.device_count() else RT_ERR_NO_DEVICE
    assert shade(w.h, 4, rows, keys, out) == good and sample(w.h, 4, ol, keys, out) == good and pdf(w.h, 4, rays, out) == good
    for call in (lambda: shade(None, 4, rows, keys, out), lambda: shade(w.h, 0, rows, keys, out), lambda: shade(w.h, 4, None, keys, out),
                 lambda: shade(w.h, 4, rows, None, out), lambda: shade(w.h, 4, rows, keys, None),
                 lambda: sample(None, 4, ol, keys, out), lambda: sample(w.h, 0, ol, keys, out), lambda: sample(w.h, 4, None, keys, out),
                 lambda: sample(w.h, 4, ol, None, out), lambda: sample(w.h, 4, ol, keys, None),
                 lambda: pdf(None, 4, rays, out), lambda: pdf(w.h, 0, rays, out), lambda: pdf(w.h, 4, None, out), lambda: pdf(w.h, 4, rays, None)):
        assert call() == RT_ERR_ARG
    for bad in (-1.0, float(len(ids)), 0.5, math.nan, math.inf, 1e300):
        x = rows.copy()
        x[2, 0] = bad
        assert shade(w.h, 4, x, keys, out) == RT_ERR_ARG, bad
    for bad in (-1.0, 3.0, 1.5, math.nan, -math.inf, 2.0 ** 32):
        x = ol.copy()
        x[3, 3] = bad
        assert sample(w.h, 4, x, keys, out) == RT_ERR_ARG, bad
    # an uncommitted scene; a scene without object lights (the mixture flag and both light diagnostics)
    u = rtamd.World()
    m = u.Lambertian(u.ConstantTexture((0.5, 0.5, 0.5)))
    s = u.Sphere((0.0, 0.0, 0.0), 1.0, m)
    x = rows.copy()
    x[:, 0] = float(m)
    assert shade(u.h, 4, x, keys, out) == RT_ERR_NOT_COMMITTED and sample(u.h, 4, ol, keys, out) == RT_ERR_NOT_COMMITTED and pdf(u.h, 4, rays, out) == RT_ERR_NOT_COMMITTED
    u.new([s])
    assert shade(u.h, 4, x, keys, out) == RT_ERR_ARG and sample(u.h, 4, ol, keys, out) == RT_ERR_ARG and pdf(u.h, 4, rays, out) == RT_ERR_ARG
    x[:, 1] = 0.0
    assert shade(u.h, 4, x, keys, out) == good
    with pytest.raises(rtamd.RtError):
        w.debug_shade(np.zeros((1, 17)) - 1.0, keys[:1])
