"""The families of tests/walk_cases.py without a device: on every list-rooted row the oracle's walk (Scene.walk: the root's hit with a
ray time and a fresh stream per row) equals the plain restatement of tests/walk_ref.py bit for bit -- hit, t, the winning list item and the
number of draws -- and every family holds the rows it is for, so that tests/test_walk_gpu.py cannot pass vacuously.  Also the refusals of
rt_debug_walk_device, which are decided on the host."""
import ctypes as C
import math

import numpy as np
import pytest

import walk_cases as wc
import walk_ref

RT_ERR_ARG, RT_ERR_NOT_COMMITTED, RT_ERR_NO_DEVICE, RT_ERR_UNSUPPORTED = -1, -8, -9, -10

_REF = {}


def ref_rows(case):
    """walk_ref's answer and classification of every row of a restatable list-rooted case: computed once"""
    if case["name"] not in _REF:
        items = case["items"]
        rows = [walk_ref.walk(items, r, k, case["t_min"]) for r, k in zip(case["rays"], case["keys"])]
        cls = [walk_ref.classify(items, r, case["t_min"]) for r in case["rays"]]
        _REF[case["name"]] = (rows, cls)
    return _REF[case["name"]]


def restatable(case):
    return case["root"] == "list" and all(walk_ref.restatable(x) for x in case["items"])


def stats(case):
    _, _, out, draws = wc.oracle_walk(case)
    return dict(rows=len(out), hit_share=float(out[:, 0].mean()), draws=np.bincount(draws).tolist())


def test_families_are_deterministic_and_within_their_limits():
    assert set(wc.FAMILIES) == set(wc._GEN)
    names = set()
    for fam in wc.FAMILIES:
        again = wc._GEN[fam]()
        assert len(again) == len(wc.family(fam)) > 0
        for a, b in zip(wc.family(fam), again):
            assert a["name"] == b["name"] and a["name"] not in names and a["name"].startswith(fam + "/")
            names.add(a["name"])
            assert np.array_equal(a["rays"], b["rays"]) and np.array_equal(a["keys"], b["keys"]) and repr(a["items"]) == repr(b["items"])
            n = len(a["rays"])
            assert 0 < n <= 4096 and n % 64 != 0 and len(a["items"]) <= 64
            assert a["rays"].shape == (n, 7) and a["keys"].shape == (n, 3) and a["keys"].dtype == np.uint64
            assert np.isfinite(a["rays"]).all() and (a["rays"][:, 3:6] != 0.0).any(axis=1).all()
            assert len({tuple(k) for k in a["keys"].tolist()}) == n                    # keys differ per row


@pytest.mark.parametrize("fam", wc.FAMILIES)
def test_oracle_equals_the_restatement_on_list_rooted_rows(fam):
    checked = 0
    for case in wc.family(fam):
        s = stats(case)
        print("%-48s rows %4d  hit share %.3f  draws %s" % (case["name"], s["rows"], s["hit_share"], s["draws"]))
        if not restatable(case):
            continue
        _, owners, out, draws = wc.oracle_walk(case)
        rows, _ = ref_rows(case)
        for i, (hit, t, win, n_draws) in enumerate(rows):
            where = (case["name"], i)
            assert bool(out[i, 0]) == hit and draws[i] == n_draws, where
            if hit:
                assert out[i, 1] == t or (t != t and out[i, 1] != out[i, 1]), where     # the same double
                assert int(out[i, 11]) in owners[win], where                           # the same list item
            checked += 1
    if fam not in ("bvh_roots", "lanes", "nested"):                                    # (BVH-rooted, or under Transforms, throughout)
        assert checked > 0


def test_scenes_without_media_draw_nothing():
    for fam in ("sweep", "lanes", "static_twin"):
        for case in wc.family(fam):
            assert not wc.oracle_walk(case)[3].any(), case["name"]


def test_row_of_fogs_reaches_every_draw_count_and_every_sub_case():
    cases = [c for c in wc.family("row_of_fogs") if c["n_media"] == wc.N_FOGS]
    assert [c["name"].split("/")[-1] for c in cases] == list(wc.ORDERS) + ["nearest_last"]
    extra = cases.pop()
    total = {"s_before": 0, "limit_walk": 0, "beyond_exit": 0, "limit_clips": 0, "track_clips": 0}
    for case in cases:
        draws = wc.oracle_walk(case)[3]
        share = np.bincount(draws, minlength=wc.N_FOGS + 1) / len(draws)
        print(case["name"], "draw shares", np.round(share, 3).tolist())
        assert len(share) == wc.N_FOGS + 1 and (share >= 0.05).all(), (case["name"], share)
        _, cls = ref_rows(case)
        for k in total:
            total[k] += sum(k in c["cases"] for c in cls)
    print("rows per sub-case of a third-or-later crossed medium, over the six orders:", total)
    assert total["limit_walk"] >= 100 and total["s_before"] >= 100 and total["beyond_exit"] >= 100, total
    # and the rows on which those walks decide the answer (walk_ref.classify): mostly of the order built for them
    for k in total:
        total[k] += sum(k in c["cases"] for c in ref_rows(extra)[1])
    print("with nearest_last:", total)
    assert total["limit_clips"] >= 100 and total["track_clips"] >= 100, total
    for case in wc.family("row_of_fogs"):                                             # fewer media: no more draws than media
        assert wc.oracle_walk(case)[3].max() <= case["n_media"]
    assert not wc.oracle_walk([c for c in wc.family("row_of_fogs") if c["n_media"] == 0][0])[3].any()


def test_second_query_rows_lie_on_both_sides_of_the_offset():
    short = long_ = 0
    for case in wc.family("second_query"):
        draws = wc.oracle_walk(case)[3]
        _, cls = ref_rows(case)
        is_short = case["chord"] < 1e-4
        assert (np.abs(case["chord"] / 1e-4 - 1.0) > 1e-3).all()                       # no row within rounding of the offset itself
        for i, c in enumerate(cls):
            assert (c["crossed"] == []) == bool(is_short[i]), (case["name"], i)        # a chord below 1e-4 in t: the second query finds nothing
            assert draws[i] == (0 if is_short[i] else 1), (case["name"], i)            # and the medium is not entered although the surface is hit
            assert c["s_index"] >= 0
        short += int(is_short.sum())
        long_ += int((~is_short).sum())
    print("second_query: %d rows below 1e-4, %d above" % (short, long_))
    assert short >= 0.25 * (short + long_) and long_ >= 0.25 * (short + long_)
    impact = wc.family("second_query")[0]
    for case in (impact, [c for c in wc.family("second_query") if c["name"].endswith("length_multiples")][0]):
        m = case["chord"] / 1e-4                                                       # the four multiples, each within 4 % on its own side
        for lo, hi in ((0.48, 0.5), (0.95, 0.99), (1.01, 1.06), (2.0, 2.09)):
            assert ((m >= lo) & (m <= hi)).mean() == pytest.approx(0.25, abs=0.01), (case["name"], lo, hi)


def test_motion_families_hit_and_miss_and_the_shared_ray_tells_times_apart():
    for fam in ("sweep", "lanes"):
        for case in wc.family(fam):
            share = wc.oracle_walk(case)[2][:, 0].mean()
            assert 0.25 <= share <= 0.90, (case["name"], share)
    for case in wc.family("lanes"):
        a, b = case["shared_block"]
        assert a % 64 == 0 and b - a == 64                                             # one block of the diagnostic's launch
        rays = case["rays"][a:b]
        assert (rays[:, :6] == rays[0, :6]).all() and np.array_equal(rays[:, 6], np.array(wc.LANE_TIMES)[np.arange(a, b) % 7])
        out = wc.oracle_walk(case)[2][a:b]
        outcomes = {tuple(r) for r in out[:, [0, 1, 11]].tolist()}
        assert len(outcomes) >= 3, (case["name"], outcomes)
    for case in wc.family("sweep"):
        t0, t1 = case["items"][0][3], case["items"][0][4]
        times = set(case["rays"][:, 6].tolist())
        assert {t0, t1, float(np.nextafter(t0, t1)), float(np.nextafter(t1, t0)), 0.5 * (t0 + t1)} <= times and len(times) == 50
    under = [c for c in wc.family("nested") if c["name"] == "nested/moving_under_chain"][0]      # the ray time matters under a chain too
    import oracle
    still = under["rays"].copy()
    still[:, 6] = 0.0
    at_zero = under["build"](oracle.Scene())[0].walk(still, under["keys"], under["t_min"])[0]
    assert (at_zero[:, 1] != wc.oracle_walk(under)[2][:, 1]).sum() >= 50
    for case in wc.family("static_twin")[1:]:                                          # the exact tie at time0: the later list item wins
        _, owners, out, _ = wc.oracle_walk(case)
        tie = (case["rays"][:, 6] == 0.25) & (out[:, 0] == 1)
        assert tie.sum() > 100 and all(int(p) in owners[1] for p in out[tie, 11])


# ---- refusals: decided on the host, before a device is asked for -------------------------------------------------------------------------
def test_walk_diagnostic_is_declared_exported_and_refuses_bad_arguments():
    import rtamd
    from test_abi_symbols import declared_symbols
    assert "rt_debug_walk_device" in declared_symbols() and "rt_debug_walk_device" in rtamd.ABI_SYMBOLS and hasattr(C.CDLL(rtamd.LIB_PATH), "rt_debug_walk_device")
    case = wc.family("fog_and_motion")[1]                                              # BVH-rooted, media and moving spheres (times in [0, 1])
    w, _ = case["build"](rtamd.World())
    L, dp, kp = w.L, C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    rays, keys, out = case["rays"][:5].copy(), case["keys"][:5].copy(), np.zeros((5, 14))

    def walk(h, kernel, n, x, k, y, t_min=1e-3):
        return L.rt_debug_walk_device(h, 0, kernel, n, x.ctypes.data_as(dp) if x is not None else None, k.ctypes.data_as(kp) if k is not None else None,
                                      t_min, y.ctypes.data_as(dp) if y is not None else None)
    good = 0 if rtamd.device_count() else RT_ERR_NO_DEVICE
    assert w.info()["accel_ok"] == 1
    for kernel in (1, 2, 3):
        assert walk(w.h, kernel, 5, rays, keys, out) == good
    for call in (lambda: walk(None, 1, 5, rays, keys, out), lambda: walk(w.h, 1, 0, rays, keys, out), lambda: walk(w.h, 1, 5, None, keys, out),
                 lambda: walk(w.h, 1, 5, rays, None, out), lambda: walk(w.h, 1, 5, rays, keys, None), lambda: walk(w.h, 0, 5, rays, keys, out),
                 lambda: walk(w.h, 4, 5, rays, keys, out), lambda: walk(w.h, 7, 5, rays, keys, out), lambda: walk(w.h, -1, 5, rays, keys, out)):
        assert call() == RT_ERR_ARG
    for bad in (math.nan, math.inf, -math.inf, -1e-9, float(np.nextafter(1.0, 2.0)), 1e300):     # not finite, or outside [time0, time1] of a moving sphere
        x = rays.copy()
        x[3, 6] = bad
        assert walk(w.h, 1, 5, x, keys, out) == RT_ERR_ARG, bad
    for fine in (0.0, 1.0, 5e-324):
        x = rays.copy()
        x[3, 6] = fine
        assert walk(w.h, 1, 5, x, keys, out) == good, fine
    assert walk(w.h, 1, 5, rays, keys, out, t_min=-1.0) == good                        # kernel 1 takes any t_min
    assert walk(w.h, 2, 5, rays, keys, out, t_min=-1.0) == RT_ERR_UNSUPPORTED and walk(w.h, 3, 5, rays, keys, out, t_min=math.nan) == RT_ERR_UNSUPPORTED
    with pytest.raises(rtamd.RtError):
        w.debug_walk(rays, keys, kernel=9)
    # the tightest range of several moving spheres decides
    twin, _ = wc.family("static_twin")[1]["build"](rtamd.World())                      # [0.25, 2]
    x = rays.copy()
    x[:, 6] = 0.2
    assert walk(twin.h, 1, 5, x, keys, out) == RT_ERR_ARG
    x[:, 6] = 2.0
    assert walk(twin.h, 1, 5, x, keys, out) == good
    # a scene without moving spheres takes any finite time
    fogs, _ = wc.family("row_of_fogs")[0]["build"](rtamd.World())
    x[:, 6] = -1e300
    assert walk(fogs.h, 1, 5, x, keys, out) == good
    x[0, 6] = math.nan
    assert walk(fogs.h, 1, 5, x, keys, out) == RT_ERR_ARG
    # an uncommitted scene; a scene without an accel (a medium under a Transform: reference order only)
    u = rtamd.World()
    u.Sphere((0.0, 0.0, 0.0), 1.0, u.Lambertian(u.ConstantTexture((0.5, 0.5, 0.5))))
    assert walk(u.h, 1, 5, rays, keys, out) == RT_ERR_NOT_COMMITTED
    under, _ = wc.family("nested")[1]["build"](rtamd.World())
    assert under.info()["accel_ok"] == 0
    assert walk(under.h, 1, 5, rays, keys, out) == good and walk(under.h, 2, 5, rays, keys, out) == RT_ERR_UNSUPPORTED and walk(under.h, 3, 5, rays, keys, out) == RT_ERR_UNSUPPORTED
    # a NodeW table that does not fit in LDS beside the stacks: 12 000 spheres make some 12 000 nodes of 96 bytes
    big = rtamd.World()
    m = big.Lambertian(big.ConstantTexture((0.5, 0.5, 0.5)))
    big.new([big.Sphere((float(i % 100), float(i // 100), 0.0), 0.3, m) for i in range(12000)], bvh_seed=1)
    assert walk(big.h, 2, 5, rays, keys, out) == good and walk(big.h, 3, 5, rays, keys, out) == RT_ERR_UNSUPPORTED
    # rt_debug_hit_device keeps refusing both kinds of scene
    for scene in (w, fogs, twin):
        assert L.rt_debug_hit_device(scene.h, 1, 5, rays[:, :6].copy().ctypes.data_as(dp), 1e-3, math.inf, out.ctypes.data_as(dp)) in (RT_ERR_UNSUPPORTED, RT_ERR_NO_DEVICE)
