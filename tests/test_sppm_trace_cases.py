"""The families of tests/sppm_trace_cases.py without a device: on the oracle alone, each reaches what it is named for, so
tests/test_sppm_trace_gpu.py cannot pass vacuously; and the argument checks of rt_debug_sppm_trace_device, which are decided on the host."""
import ctypes as C

import numpy as np
import pytest

import sppm_trace_cases as tc


def _all_cases():
    return [c for fam in tc.FAMILIES for c in tc.family(fam)]


def test_every_case_has_a_name_of_its_own_and_a_scene():
    names = [c["name"] for c in _all_cases()]
    assert len(set(names)) == len(names) == 30 + 8 + 8 + 4 + 16 + 4 + 1
    assert {c["scene"] for c in _all_cases()} == set(tc.SCENES)


@pytest.mark.parametrize("fam", list(tc.FAMILIES))
def test_no_map_holds_a_nan_or_the_same_row_twice(fam):
    for c in tc.family(fam):
        g, cau, gp, S = tc.oracle_run(c)
        assert len(gp) == c["width"] * c["height"] and 0 <= S <= 60
        for rows in (g, cau):
            assert not np.isnan(rows).any(), c["name"]
            u = tc.sorted_rows(rows)
            assert not (u[1:] == u[:-1]).all(axis=1).any(), c["name"]             # a multiset compare would otherwise hide a swap of equals
        assert not np.isnan(gp).any() and (gp[gp[:, 0] == 0.0] == 0.0).all(), c["name"]   # a row without a gather point is all zeros
        assert set(np.unique(gp[:, 0])) <= {0.0, 1.0}


def test_counts_reach_the_wave_the_chunk_and_the_block():
    P = set(c["P"] for c in tc.family("a_counts"))
    assert {1, 63, 64, 65} <= P and {255, 256, 257} <= P and {1023, 1024, 1025} <= P and max(P) > 4 * 1024     # < wave; chunk +- 1; block +- 1; > 4 blocks
    assert {c["iteration"] for c in tc.family("a_counts")} == {0, 3}
    for c in tc.family("a_counts"):
        g, cau, gp, _ = tc.oracle_run(c)
        assert len(g) >= len(cau) and 100 < (gp[:, 0] != 0).sum() < len(gp), c["name"]
    big = [tc.oracle_run(c) for c in tc.family("a_counts") if c["P"] == 4097]
    assert all(len(g) > 4097 and len(cau) > 0 for g, cau, _, _ in big)
    assert len(tc.oracle_run(tc.family("a_counts")[0])[0]) <= 64                   # P = 1: one path


def test_far_index_lies_beyond_2_to_the_32():
    cases = tc.family("b_far_index")
    first = [c["iteration"] * c["P"] for c in cases]
    last = [c["iteration"] * c["P"] + c["P"] for c in cases]
    assert any(a < 2 ** 32 < b for a, b in zip(first, last))                       # one launch crosses 2^32 inside
    assert sum(a > 2 ** 32 for a in first) >= 3                                    # others lie wholly beyond it
    assert any(a > 2 ** 40 for a in first) and max(c["iteration"] for c in cases) == 2 ** 31 - 1
    # the 64-bit index matters: the photons of an iteration are not those of the iteration with the same index mod 2^32
    c = next(c for c in cases if c["P"] == 1025 and c["iteration"] == 5000000)
    _, _, o = tc.scene(c["scene"])
    wrapped = (5000000 * 1025) % 2 ** 32
    assert wrapped % 1025 != 0 or not np.array_equal(tc.oracle_run(c)[0], o.sppm_iteration(37, 21, wrapped // 1025, 1025, seed=c["seed"])[0])
    assert len(tc.oracle_run(c)[0]) > 1025
    # the eye stream's sample index is the iteration: other gather points than at iteration 0
    assert not np.array_equal(tc.oracle_run(c)[2], o.sppm_iteration(37, 21, 0, 1025, seed=c["seed"])[2])


@pytest.mark.parametrize("which", ["glass", "smoke"])
def test_bounces_cut_paths(which):
    runs = {c["max_bounces"]: tc.oracle_run(c) for c in tc.family("c_bounces") if ("_%s_" % which) in c["name"]}
    assert sorted(runs) == [1, 2, 3, 4096]
    n = {mb: len(r[0]) for mb, r in runs.items()}
    # (the glass scene is open above its flat floor: a second bounce there is inside the glass, on the metal or into the void, and stores nothing)
    assert 0 < n[1] < n[2] < n[3] < n[4096] if which == "smoke" else 0 < n[1] == n[2] < n[3] <= n[4096], n
    assert len(runs[1][1]) == 0 and len(runs[3][1]) > 0                            # a caustic photon needs a specular and a diffuse bounce
    valid = {mb: r[2][:, 0] != 0 for mb, r in runs.items()}
    assert (valid[4096] & ~valid[1]).sum() > 10 and not (valid[1] & ~valid[4096]).any()    # eye paths through glass or fog need more than one bounce


def test_lights_all_emit_and_the_zero_light_never_does():
    four = tc.family("d_lights")[0]
    g, cau, _, S = tc.oracle_run(four)
    n = tc.emitter_counts(g)
    assert n[1] == 0 and min(n[0], n[2], n[3]) >= 20 and sum(n) == len(g), n
    assert n[0] > n[2] > n[3]                                                      # the weights' order
    assert S == 40 - 9                                                             # the brightest: 500 = 0.98 * 2^9
    assert len(cau) > 0
    for c, (_, _, want) in zip(tc.family("d_lights")[1:], tc.S_EDGES):
        g, _, _, S = tc.oracle_run(c)
        assert S == want == c["S"] and len(g) > 0, c["name"]
        assert (g[:, 3:6] != 0).all() and np.isfinite(g).all()
    assert [c["S"] for c in tc.family("d_lights")[1:]] == [39, 0, 60]


def test_variants_table_names_all_eight_photon_and_six_eye_kernels():
    words = [w for _, _, _, w in tc.VARIANTS]
    assert len(set(words)) == 8                                                    # photon: <accel, lds> x 3, nest, each with a MEDIA twin
    assert len({w & ~tc.LDS for w in words}) == 6                                  # eye: no LDS bit
    assert {c["variant"] for c in tc.family("e_variants")} == set(words)
    for c in tc.family("e_variants"):
        g, _, gp, _ = tc.oracle_run(c)
        assert len(g) > c["P"] // 2 and (gp[:, 0] != 0).sum() > 50, c["name"]
    for _, key, _, word in tc.VARIANTS:                                            # what the selection reads from the scene
        w, _, _ = tc.scene(key)
        assert bool(w.info()["accel_ok"]) == bool(word & (tc.ACCEL | tc.NEST)) or key == "cornell_far", key


def test_capacity_counts_are_above_one():
    exp = [tc.oracle_run(c) for c in tc.family("f_capacity")]
    G, C_ = len(exp[0][0]), len(exp[0][1])
    assert G > 1 and C_ > 1
    assert all(len(e[0]) == G and len(e[1]) == C_ for e in exp)                    # one configuration, four capacities
    caps = [c["capacity"](G, C_) for c in tc.family("f_capacity")]
    assert caps == [(G, C_), (G - 1, C_), (G, C_ - 1), (1, 1)]
    assert [c["launches"] for c in tc.family("f_capacity")] == [1, 2, 2, 2]
    assert max(G, C_) + 1024 >= max(G, C_) and 2 * 1 < G                           # (1, 1): one retry fits because it is sized from the counts


def test_stride_case_lies_just_above_the_grid():
    for cus in (256, 304, 64):
        (c,) = tc.stride(cus)
        npix = c["width"] * c["height"]
        assert cus * 8 * 256 < npix <= cus * 8 * 256 + tc.STRIDE_WIDTH and not c["photons"]
    (c,) = tc.family("g_stride")
    _, _, gp, _ = tc.oracle_run(c)
    tail = gp[256 * 8 * 256:]
    assert 0 < len(tail) <= tc.STRIDE_WIDTH and (tail[:, 0] != 0).all() and (gp[:, 0] == 0).any()     # every pixel of the second trip holds a gather point


# ---- refusals of the device entry: decided on the host, before a device is asked for ---------------------------------------------------------
def test_trace_entry_checks_its_arguments_before_it_asks_for_a_device():
    import rtamd
    L = rtamd.lib()
    dp = C.POINTER(C.c_double)
    w, cam, _ = tc.scene("cornell")
    g, cau, pts = np.zeros((64, 9)), np.zeros((64, 9)), np.zeros((4 * 3, 7))

    def io(**kw):
        a = rtamd.rt_debug_sppm_trace()
        a.width, a.height, a.iteration, a.photons_per_iter, a.max_bounces, a.seed = 4, 3, 0, 2, 5, 1
        a.global_, a.global_rows, a.caustic, a.caustic_rows = g.ctypes.data_as(dp), 64, cau.ctypes.data_as(dp), 64
        a.points = pts.ctypes.data_as(dp)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(a, scene=w, camera=cam, device=0):
        return L.rt_debug_sppm_trace_device(scene.h if scene is not None else None, C.byref(camera.c) if camera is not None else None, device,
                                            C.byref(a) if a is not None else None)
    assert call(None) == -1                                        # a null struct
    assert call(io(), scene=None) == -1 and call(io(), camera=None) == -1
    for bad in (dict(width=1), dict(height=1), dict(width=0), dict(photons_per_iter=0), dict(max_bounces=0), dict(iteration=-1),
                dict(width=65536, height=65536), dict(capacity_global=2 ** 30 + 1), dict(global_=None), dict(caustic=None)):
        assert call(io(**bad)) == -1, bad                          # RT_ERR_ARG, with and without a device
    raw = rtamd.World()
    raw.Sphere((0.0, 0.0, 0.0), 1.0, raw.Lambertian(raw.ConstantTexture((0.5, 0.5, 0.5))))
    assert call(io(), scene=raw) == -8                             # RT_ERR_NOT_COMMITTED
    unlit, ucam = rtamd.load_scene_file(tc.scene_path("scene_10.json"))
    assert call(io(), scene=unlit, camera=ucam) == -1              # no lights: the render's own refusal, through the shared check
    if rtamd.device_count() > 0:
        return                                                     # a HIP device is visible: tests/test_sppm_trace_gpu.py runs the entry
    assert call(io()) == -9                                        # RT_ERR_NO_DEVICE
    with pytest.raises(rtamd.RtError) as e:
        w.debug_sppm_trace(cam, 4, 3, photons_per_iter=2)
    assert e.value.code == -9
