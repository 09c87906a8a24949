"""The oracle's background, env sampling and area lights (oracle/rt_oracle.cpp, restated from include/rtamd.h) without a device: every
piece equals the numpy restatements (tests/env_ref.py, tests/area_ref.py) bit for bit, a scene that uses none of them renders the bits of
the oracle before it knew them, integrator 1 over area lights and the environment agrees with integrator 0 in expectation, and whole
paths equal an evaluation in Python floats in the header's order.  tests/test_light_frames_gpu.py then holds the kernels to this oracle."""
import math
import os

import numpy as np
import pytest

import area_ref
import env_ref
import light_scenes as ls
from conftest import GOLDEN, scene_path
from test_background_gpu import BG_SPECS
from test_env_sampling_gpu import AUTO, SPECS

PI = 3.14159265358979323846264338327950288


# ---- 1. B(d) ------------------------------------------------------------------------------------------------------------------------
def directions():
    """4096 directions of any length: random ones, the axes, straight up and down, nearly so, tiny and huge lengths"""
    rng = np.random.default_rng(21)
    d = rng.normal(size=(4096, 3)) * rng.uniform(0.05, 20.0, (4096, 1))
    d[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    d[6:10] = [[0, 3.5, 0], [0, -0.25, 0], [1e-9, 1.0, 0], [0, -1.0, 1e-12]]
    d[10:14] = [[0.0, 1e-150, 0.0], [0.0, -1e150, 0.0], [1e-17, -1.0, 1e-17], [-0.0, 1.0, -0.0]]  # u.y = +-1 exactly
    d[14:142] *= 1e-140   # sqlen near the bottom of the normal range (a sqlen of 0 is an error on both sides, not a colour)
    d[142:270] *= 1e150
    return d


def _noise_spec():
    import oracle
    side = oracle.Scene()
    tex = side.NoiseTexture(ls.NOISE["noise_scale"], ls.NOISE["seed"])
    spec = dict(ls.NOISE)
    spec["value"] = lambda p: np.array([[side.noise_value(tex, q)[2]] * 3 for q in p])  # the marble value at rec.p, white
    return spec


@pytest.mark.parametrize("name", sorted(BG_SPECS) + ["noise"])
def test_background_equals_the_restatement(name):
    import oracle
    spec = _noise_spec() if name == "noise" else BG_SPECS[name]
    o = oracle.Scene()
    ls.set_background(o, spec)
    d = directions()
    with np.errstate(all="ignore"):
        exp = env_ref._background(spec, d)
    got = o.background(d)
    assert np.isfinite(exp).all() and (exp >= 0).all() and (exp > 0).any()
    assert got.tobytes() == np.ascontiguousarray(exp).tobytes(), "%d directions differ" % int((got != exp).any(axis=1).sum())
    if name != "constant":
        assert len(np.unique(got, axis=0)) > 1


def test_background_refusals():
    import oracle
    o = oracle.Scene()
    for bad in (dict(kind=4), dict(kind=1, color0=(-1.0, 0, 0)), dict(kind=1, scale=float("inf")), dict(kind=3, texture=0)):
        with pytest.raises(oracle.OracleError):
            o.set_background(**bad)
    with pytest.raises(oracle.OracleError):
        o.set_env_sampling(0, 0)  # no background yet: rt_scene_commit refuses it
    with pytest.raises(oracle.OracleError):
        o.background(np.eye(3))


# ---- 2. the env table, its draw and its pdf --------------------------------------------------------------------------------------------
ENV_CASES = dict(SPECS)
ENV_CASES["gradient_37x19"] = (SPECS["gradient"][0], (37, 19))  # neither a power of two nor even
ENV_SIZE = dict(AUTO)
ENV_SIZE["gradient_37x19"] = (37, 19)


def env_draws(q):
    """xi [n, 4]: random ones, the ends of [0, 1), and values that land on the borders of rows and cells"""
    H, W = q.shape
    rng = np.random.default_rng(22)
    xi = rng.random((2048, 4))
    edge = [0.0, 1.0 - 2.0 ** -53, 0.5]
    k = 0
    for a in edge:
        for b in edge:
            xi[k] = [a, b, b, a]
            xi[k + 1] = [b, a, a, b]
            k += 2
    rowcum = np.cumsum(q.sum(axis=1, dtype=np.uint64), dtype=np.uint64)
    total = float(rowcum[-1])
    for j in range(min(H, 32)):  # xi1 * total lands on, just under and just over the row's prefix sum
        for e in (-1, 0, 1):
            xi[k, 0] = min(max((float(rowcum[j]) + e) / total, 0.0), 1.0 - 2.0 ** -53)
            k += 1
    row = np.cumsum(q[H // 2], dtype=np.uint64)
    for i in range(min(W, 32)):
        for e in (-1, 0, 1):
            xi[k, 0] = (float(rowcum[H // 2]) - 0.5) / total
            xi[k, 1] = min(max((float(row[i]) + e) / float(row[-1]), 0.0), 1.0 - 2.0 ** -53)
            k += 1
    assert k < 1024
    return xi


@pytest.mark.parametrize("name", sorted(ENV_CASES))
def test_env_table_draw_and_pdf_equal_the_restatement(name):
    import oracle
    spec, size = ENV_CASES[name]
    o = oracle.Scene()
    ls.set_background(o, spec)
    o.set_env_sampling(*(size if size is not None else (0, 0)))
    q, total = o.env_table()
    W, H = ENV_SIZE[name]
    assert q.shape == (H, W) and q.dtype == np.uint32
    ref, _ = env_ref.table_ref(spec, W, H)
    assert np.array_equal(q.astype(np.uint64), ref), "%d cells differ" % int((q.astype(np.uint64) != ref).sum())
    assert total == int(ref.sum(dtype=np.uint64)) and int(q.max()) == 4294967295 and (q > 0).all()
    xi = env_draws(q)
    got = o.env_sample(xi)
    d_ref, cells = env_ref.sample_ref(q, xi)
    assert got[:, :3].tobytes() == d_ref.tobytes(), "%d directions differ" % int((got[:, :3] != d_ref).any(axis=1).sum())
    assert len(np.unique(cells[:, 1])) >= min(H, 8) and len(np.unique(cells[:, 0])) > 1
    p_ref = env_ref.pdf_ref(q, d_ref)
    assert got[:, 3].tobytes() == p_ref.tobytes(), "%d pdfs differ" % int((got[:, 3] != p_ref).sum())
    # any direction, any length; straight up and down (s2 is not > 0) and a NaN answer 0
    d = np.concatenate([directions()[:1024], 3.5 * d_ref[:512]])
    d[20] = [float("nan"), 1.0, 0.0]
    d[21] = [0.0, float("nan"), 0.0]
    with np.errstate(all="ignore"):
        exp = env_ref.pdf_ref(q, d)
    pdf = o.env_pdf(d)
    assert pdf.tobytes() == exp.tobytes(), "%d pdfs differ" % int((pdf != exp).sum())
    assert (pdf[[2, 3, 6, 7, 10, 11, 13, 20, 21]] == 0.0).all() and (pdf > 0).sum() > 1000


def test_black_table_switches_the_strategy_off():
    import oracle
    o = oracle.Scene()
    o.World(ls.floor_and_ball(o), 1)
    o.Camera(*ls.SHADOW_CAM)
    ls.set_background(o, ls.BLACK)
    o.set_env_sampling(16, 8)
    q, total = o.env_table()
    assert total == 0 and not q.any()
    assert not o.env_sample(np.full((3, 4), 0.5)).any() and not o.env_pdf(np.eye(3)).any()
    with pytest.raises(oracle.OracleError):  # no object light, no area light, no environment strategy
        o.render(8, 8, 1, integrator=1)
    ls.set_background(o, ls.CONSTANT)  # the table follows the background
    assert o.env_table()[1] > 0
    o.render(8, 8, 1, integrator=1)


# ---- 3. area lights ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def area_pair():
    w, _, o, _ = ls.pair_area()
    return w, o


def test_area_table_equals_the_products_lowering(area_pair):
    w, o = area_pair
    tab = area_ref.table_of(w.area_light_tris())
    got, totals = o.area_light_tris()
    assert len(got["q"]) == 6
    for k in area_ref.AREA_TRI_FIELDS:
        assert got[k].dtype == tab[k].dtype and got[k].tobytes() == np.ascontiguousarray(tab[k]).tobytes(), k
    assert totals == [int(tab["q"][tab["light"] == l].astype(np.uint64).sum()) for l in (0, 1)]


def test_area_draw_and_pdf_equal_the_restatement(area_pair):
    import test_area_lights_gpu as ta
    _, o = area_pair
    tab, _ = o.area_light_tris()
    x = ta.sample_inputs()
    got = o.area_sample(x)
    exp = area_ref.sample(tab, x)
    assert got[:, :3].tobytes() == exp.tobytes()
    exp_pdf = area_ref.pdf(tab, np.concatenate([x[:, :3], exp], axis=1))
    assert got[:, 3].tobytes() == exp_pdf.tobytes()
    assert (got[:, 3] > 0.0).mean() > 0.99
    rays = ta.pdf_inputs(tab)
    pdf = o.area_pdf(rays)
    assert pdf.tobytes() == area_ref.pdf(tab, rays).tobytes()
    assert (pdf > 0.0).sum() > 1000 and (pdf == 0.0).sum() > 500


def test_degenerate_triangles_are_dropped_and_small_ones_get_q_1():
    import oracle
    o = oracle.Scene()
    a, b, c, d = (0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (2.0, 1.0, 0.0), (0.0, 2.0, 1.0)
    tiny = ((5.0, 1.0, 0.0), (5.0 + 2.0 ** -20, 1.0, 0.0), (5.0, 1.0 + 2.0 ** -20, 0.0))  # area2 = 2^-40 of the unit triangle's: below 2^-32
    unit = ((3.0, 1.0, 0.0), (4.0, 1.0, 0.0), (3.0, 2.0, 0.0))
    o.set_area_lights([[(a, b, d), (a, b, c), (b, c, d)], [unit, tiny, (a, a, a), ((0.0, 0.0, 0.0), (float("inf"), 0.0, 0.0), (0.0, 1.0, 0.0))]])
    tab, totals = o.area_light_tris()
    assert list(tab["light"]) == [0, 0, 1, 1]  # the line, the point and the infinite one are gone
    assert np.array_equal(tab["a"][1], b) and np.array_equal(tab["a"][3], tiny[0])
    assert list(tab["q"][2:]) == [4294967295, 1] and totals[1] == 4294967296
    assert int(tab["q"][:2].max()) == 4294967295 and totals[0] == int(tab["q"][:2].astype(np.uint64).sum())
    x = np.array([[3.2, 0.0, 0.0, 0.75, 1.0 - 2.0 ** -53, 0.25, 0.25], [3.2, 0.0, 0.0, 0.75, 0.5, 0.25, 0.25]])
    got = o.area_sample(x)  # the last unit of the prefix sum is the tiny triangle's
    assert got[:, :3].tobytes() == area_ref.sample(tab, x).tobytes()
    assert abs(got[0, 0] + x[0, 0] - 5.0) < 1e-5 and abs(got[1, 0] + x[1, 0] - 3.25) < 1e-12
    with pytest.raises(oracle.OracleError):
        o.set_area_lights([[(a, b, c)]])  # a light with no triangle of non-zero area


# ---- 4. nothing else moved --------------------------------------------------------------------------------------------------------------
def test_a_scene_without_the_features_renders_the_bits_it_had():
    """tests/golden/cornell_32x32_4spp_seed1_integrator1.npy was rendered by the oracle of the commit before it knew backgrounds, env
    sampling and area lights; tests/test_golden.py holds the integrator 0 frames"""
    import oracle
    gold = np.load(os.path.join(GOLDEN, "cornell_32x32_4spp_seed1_integrator1.npy"))
    o = oracle.cornell_box_scene(scene_path("cube.obj"), 1.0, seed=1)
    img, _ = o.render(32, 32, 4, seed=1, integrator=1)
    assert (gold > 0).any() and img.tobytes() == gold.tobytes()
    c = o.light_counters()
    assert c["n_pick_object"] > 0 and c["n_pick_area"] == c["n_pick_env"] == 0 and c["n_cosine_half"] > 0
    i0, _ = o.render(32, 32, 4, seed=1, integrator=0)
    o.set_background(0)
    o.set_area_lights([])
    again, _ = o.render(32, 32, 4, seed=1, integrator=1)
    assert again.tobytes() == gold.tobytes()
    assert o.render(32, 32, 4, seed=1, integrator=0)[0].tobytes() == i0.tobytes()
    ls.set_background(o, ls.BLACK)  # beta * 0 on a miss, and an env table whose total is 0
    o.set_env_sampling(0, 0)
    assert o.render(32, 32, 4, seed=1, integrator=1)[0].tobytes() == gold.tobytes()


# ---- 5. unbiased ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,picks", [
    ("L0_M2_E1", dict(bg=ls.GRADIENT, env=(64, 32)), dict(n_pick_object=False, n_pick_area=True, n_pick_env=True)),
    ("L1_M1_E0", dict(tetra=False, object_light=True), dict(n_pick_object=True, n_pick_area=True, n_pick_env=False)),
])
def test_oracle_mixture_equals_brute_force_in_expectation(name, kw, picks):
    """tests/test_mixture.py's criterion and sizes (24 x 24, 3000 spp of integrator 0 against 600 spp of integrator 1, max_depth 6)"""
    _, _, o, _ = ls.pair_area(**kw)
    bf, _ = o.render(24, 24, 3000, seed=1, integrator=0, max_depth=6)
    mx, _ = o.render(24, 24, 600, seed=2, integrator=1, max_depth=6)
    c = o.light_counters()
    for k, want in picks.items():
        assert (c[k] > 0) == want, (k, c)
    b4 = bf.reshape(4, 6, 4, 6, 3).mean(axis=(1, 3, 4))
    m4 = mx.reshape(4, 6, 4, 6, 3).mean(axis=(1, 3, 4))
    print("%s: means %.5f (integrator 1) %.5f (integrator 0); largest block difference %.4f" % (name, mx.mean(), bf.mean(), np.abs(m4 - b4).max()))
    assert mx.mean() == pytest.approx(bf.mean(), rel=0.05)
    assert np.allclose(m4, b4, rtol=0.25, atol=0.02)


# ---- 6. whole paths by hand -------------------------------------------------------------------------------------------------------------
HAND_BG = dict(kind=1, color=(0.25, 0.5, 1.0), scale=2.0)
HAND_FLOOR, HAND_WALL = (0.5, 0.625, 0.75), (0.75, 0.5, 0.25)
HAND_CAM = ((0.0, 2.0, 6.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 50.0, 1.0, 0.0, 10.0)


def _unit3(v):
    ln = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] / ln, v[1] / ln, v[2] / ln)


def _hand_path(o, albedo, q, n_strategies, ray, f64, rng, max_depth):
    """one path of integrator 1 with the environment as its only strategy, in Python floats: the hits come from the oracle's hit(), the
    draws from the path's stream (f64 / rng: draw k converted as gen::<f64>() / gen_range(-1, 1)), the env draw and pdf from
    tests/env_ref.py.  Returns (L, what happened)."""
    k = 2  # the pixel jitter
    while True:  # the lens sample (drawn though the aperture is 0): rejection in the unit disk
        a, b = rng[k], rng[k + 1]
        k += 2
        if not (a * a + b * b + 0.0 * 0.0 >= 1.0):
            break
    orig, d = ray
    beta, L = [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]
    B = [HAND_BG["scale"] * c for c in HAND_BG["color"]]
    seen = dict(bounces=0, light=0, cosine=0, miss=False, wgt=False)
    depth = max_depth
    while True:
        h = o.hit(orig, d)
        if h is None:
            L = [L[c] + beta[c] * B[c] for c in range(3)]
            seen["miss"] = True
            break
        if depth <= 0:
            break
        depth -= 1
        att = albedo[h["prim_id"]]
        n = [float(x) for x in h["normal"]]
        while True:  # Lambertian::scatter: normal + random_unit_vector() (Marsaglia)
            u, v = rng[k], rng[k + 1]
            k += 2
            r2 = u * u + v * v
            if r2 <= 1.0:
                break
        s = _unit3((2.0 * u * math.sqrt(1.0 - r2), 2.0 * v * math.sqrt(1.0 - r2), 1.0 - 2.0 * r2))
        nd = [n[0] + s[0], n[1] + s[1], n[2] + s[2]]
        assert not all(abs(x) < 1e-8 for x in nd)
        coin = f64[k]
        k += 1
        if coin < 0.5:
            li = min(n_strategies - 1, int(f64[k] * float(n_strategies)))
            k += 1
            assert li == 0  # the environment is strategy L + M = 0
            xi = np.array([f64[k:k + 4]])
            k += 4
            nd = [float(x) for x in env_ref.sample_ref(q, xi)[0][0]]
            seen["light"] += 1
        else:
            seen["cosine"] += 1
        un = _unit3(nd)
        cosine = n[0] * un[0] + n[1] * un[1] + n[2] * un[2]
        spdf = 0.0 if cosine < 0.0 else cosine / PI
        lp = 0.0 + float(env_ref.pdf_ref(q, np.array([nd]))[0])
        pdf_val = 0.5 * (lp / float(n_strategies)) + 0.5 * spdf
        wgt = spdf / pdf_val if pdf_val != 0.0 else float("nan")
        if not (wgt > 0.0):
            seen["wgt"] = True
            break
        beta = [(beta[c] * att[c]) * wgt for c in range(3)]
        orig, d = [float(x) for x in h["p"]], nd
        seen["bounces"] += 1
    return L, seen


def test_paths_by_hand_on_a_floor_and_a_wall_under_a_constant_background():
    """Every pixel of a 10 x 10 frame at 1 spp: camera ray, floor or wall, the mixture step with n = 1 (coin, index, four env draws or the
    cosine direction, pdf sum from 0.0, / n, weight), the next hit, ..., the miss that adds beta (x) B.  Exact."""
    import oracle
    W = H = 10
    SEED = 5
    o = oracle.Scene()
    floor = o.XZRectangle((-6.0, -6.0), (6.0, 6.0), 0.0, o.Lambertian(o.ConstantTexture(HAND_FLOOR)))
    wall = o.XYRectangle((-6.0, 0.0), (6.0, 6.0), -2.0, o.Lambertian(o.ConstantTexture(HAND_WALL)))
    o.World([floor, wall], 1)
    o.Camera(*HAND_CAM)
    ls.set_background(o, HAND_BG)
    o.set_env_sampling(8, 4)
    q, _ = o.env_table()
    assert np.array_equal(q.astype(np.uint64), env_ref.table_ref(HAND_BG, 8, 4)[0])
    img, _ = o.render(W, H, 1, seed=SEED, integrator=1, max_depth=3)
    cnt = o.light_counters()
    albedo = {floor: HAND_FLOOR, wall: HAND_WALL}
    tot = dict(light=0, cosine=0, miss_after=0, wgt=0, two=0, depth_end=0)
    for y in range(H):
        for x in range(W):
            pix = y * W + x
            f64 = oracle.rng_f64(SEED, pix, 0, 96)
            rng = oracle.rng_range(SEED, pix, 0, 96, -1.0, 1.0)
            L, seen = _hand_path(o, albedo, q, 1, o.camera_ray(W, H, x, y, seed=SEED, sample=0), f64, rng, 3)
            assert tuple(img[y, x]) == tuple(L), (x, y, seen)
            tot["light"] += seen["light"]
            tot["cosine"] += seen["cosine"]
            tot["miss_after"] += seen["miss"] and seen["bounces"] > 0
            tot["wgt"] += seen["wgt"]
            tot["two"] += seen["miss"] and seen["bounces"] >= 2
            tot["depth_end"] += (not seen["miss"]) and (not seen["wgt"])
    print(tot, cnt)
    assert tot["two"] > 0 and tot["light"] > 0 and tot["cosine"] > 0 and tot["wgt"] > 0 and tot["depth_end"] > 0
    assert cnt["n_pick_env"] == tot["light"] and cnt["n_cosine_half"] == tot["cosine"] and cnt["n_pick_object"] == cnt["n_pick_area"] == 0
    assert cnt["n_miss_after_bounce"] == tot["miss_after"] and cnt["n_wgt_end"] == tot["wgt"]
