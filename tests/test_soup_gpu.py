"""The composed scenes of tests/soup_scenes.py through every kernel: one test per corpus scene, HIP against the oracle.

Every call on a scene -- rt_render through kernel 0 / 1 / 2 / 5 / 6 x integrator 0 / 1 (kernels 1 / 2 also with the scene out of LDS),
the closest-hit walks of kernels 1, 2, 3, 5 and 6 and the any-hit walks of kernels 1 / 2 on the scene's test rays, the guide buffers
and the ambient-occlusion pass through kernels 1 / 2 -- must give the oracle's answer bit for bit where soup_scenes.expected() says it
renders, and fail with exactly the predicted rt_status where the header says it is refused.  A different frame is never accepted.
tests/test_soup_scenes.py shows without a device that the scenes and rays reach what they aim at.

A failure names the recipe index, the call and the first differing pixel or ray: soup_scenes.build(soup_scenes.recipe(index)) rebuilds
the scene.  Scenes with a medium or moving spheres, whose closest hit needs a random stream and a ray time (rt_debug_hit_device refuses
them), have their test rays asked through rt_debug_walk_device instead.  rt_render_sppm runs on composed scenes too, never through
kernel 6 (soup_scenes.WITHHELD): here every call of it the header refuses, on the smallest configuration; tests/test_soup_sppm_gpu.py
holds the frames of the recipes it renders."""
import numpy as np
import pytest

import ao_ref
import soup_scenes as ss

pytestmark = pytest.mark.gpu

WF_WORKSPACE_MB = 256   # kernel 6: a small budget for its pools, as tests/test_parity_gpu.py's budget test sets one
AOV_SPP, AO_SPP, AO_RAYS = 2, 1, 2


def _first_bad(got, exp):
    bad = ((got != exp) & ~(np.isnan(got) & np.isnan(exp))).reshape(len(got), -1).any(axis=1)
    return int(bad.sum()), (int(np.flatnonzero(bad)[0]) if bad.any() else -1)


def _same_frame(got, exp, what):
    n, k = _first_bad(got.reshape(ss.W * ss.H, -1), exp.reshape(ss.W * ss.H, -1))
    if n:
        y, x = divmod(k, ss.W)
        raise AssertionError("%s: %d of %d pixels differ, first (x=%d, y=%d): hip=%s oracle=%s" % (what, n, ss.W * ss.H, x, y, got[y, x].tolist(), exp[y, x].tolist()))


def _same_rows(got, exp, rays, what):
    n, k = _first_bad(got, exp)
    if n:
        raise AssertionError("%s: %d of %d rays differ, first row %d: ray %r hip=%s oracle=%s" % (what, n, len(got), k, rays[k].tolist(), got[k].tolist(), exp[k].tolist()))


def _refused(code, what, fn):
    import rtamd
    try:
        fn()
    except rtamd.RtError as e:
        assert e.code == code, "%s: refused with %d (%s), the header says %d" % (what, e.code, e, code)
        return
    raise AssertionError("%s: ran, the header says it is refused with %d" % (what, code))


@pytest.mark.parametrize("index", ss.corpus())
def test_soup(index, tuning):
    rec = ss.recipe(index)
    w, cam, side, kw = ss.build_pair(rec)
    o = side.b
    counts = dict(frames=0, refusals=0, hit_records=0, occlusion_rows=0, guides=0, ao=0, sppm_refusals=0)
    frames, by_kernel = {}, {}

    def oracle_frame(integ):
        if integ not in frames:
            frames[integ] = o.render(ss.W, ss.H, ss.SPP, seed=ss.SEED, t_min=ss.T_MIN, integrator=integ)[0]
        return frames[integ]

    # ---- the render matrix ----
    for no_lds in (0, 1):
        tuning(no_lds=no_lds, wf_workspace_mb=WF_WORKSPACE_MB)
        for kernel in ((0, 1, 2, 5, 6) if no_lds == 0 else (1, 2)):
            for integ in (0, 1):
                what = "recipe %d: render(kernel=%d, integrator=%d, no_lds=%d)" % (index, kernel, integ, no_lds)
                exp = ss.expected(rec, "render", kernel, integ, no_lds)
                call = lambda: w.render(cam, width=ss.W, height=ss.H, spp=ss.SPP, seed=ss.SEED, t_min=ss.T_MIN, kernel=kernel, integrator=integ, **kw)  # noqa: E731
                if exp != ss.FRAME:
                    _refused(exp, what, call)
                    counts["refusals"] += 1
                    continue
                img, st = call()
                allowed = {kernel} if kernel else {ss.auto_kernel(rec, integ)} & ss.allowed_kernels(rec, integ)
                assert st["kernel_used"] in allowed, "%s: ran kernel %d, the header says %s" % (what, st["kernel_used"], sorted(allowed))
                by_kernel[(st["kernel_used"], integ)] = by_kernel.get((st["kernel_used"], integ), 0) + 1
                assert not (no_lds and st["scene_in_lds"]), what
                _same_frame(img, oracle_frame(integ), what)
                counts["frames"] += 1
    tuning()

    # ---- closest hits and the any-hit walk on the scene's test rays ----
    rays = ss.test_rays(rec, side)
    hits = ss.hit_records(rec, side, rays)
    f = ss.facts(rec)
    for kernel in (1, 2, 3, 5, 6):
        what = "recipe %d: debug_hit(kernel=%d)" % (index, kernel)
        exp = ss.expected(rec, "debug_hit", kernel)
        if exp != ss.FRAME:
            _refused(exp, what, lambda: w.debug_hit(rays, t_min=ss.T_MIN, kernel=kernel))
            counts["refusals"] += 1
        else:
            _same_rows(w.debug_hit(rays, t_min=ss.T_MIN, kernel=kernel)[:, :11], hits[:, :11], rays, what)
            counts["hit_records"] += len(rays)
    if f["media"] or f["moving"]:
        rays7 = np.concatenate([rays, np.full((len(rays), 1), ss.RAY_TIME)], axis=1)
        for kernel in (1, 2, 3):
            what = "recipe %d: debug_walk(kernel=%d)" % (index, kernel)
            exp = ss.expected(rec, "debug_walk", kernel)
            call = lambda: w.debug_walk(rays7, ss.ray_keys(len(rays)), t_min=ss.T_MIN, kernel=kernel)  # noqa: E731
            if exp != ss.FRAME:
                _refused(exp, what, call)
                counts["refusals"] += 1
            else:
                _same_rows(call()[:, :11], hits[:, :11], rays, what)
                counts["hit_records"] += len(rays)
    rows = expected_occ = None
    for kernel in (1, 2):
        what = "recipe %d: debug_occluded(kernel=%d)" % (index, kernel)
        exp = ss.expected(rec, "debug_occluded", kernel)
        if exp != ss.FRAME:
            _refused(exp, what, lambda: w.debug_occluded(np.concatenate([rays, np.full((len(rays), 1), np.inf)], axis=1), t_min=ss.T_MIN, kernel=kernel))
            counts["refusals"] += 1
            continue
        if rows is None:
            rows, expected_occ = ss.occlusion_rows(side, rays)
        got = w.debug_occluded(rows, t_min=ss.T_MIN, kernel=kernel)
        _same_rows(got.astype(float)[:, None], expected_occ.astype(float)[:, None], rows, what)
        counts["occlusion_rows"] += len(rows)

    # ---- the consumer passes ----
    aov = ao = None
    for kernel in (1, 2):
        what = "recipe %d: render_aov(kernel=%d, aov_spp=%d)" % (index, kernel, AOV_SPP)
        exp = ss.expected(rec, "render_aov", kernel)
        call = lambda: w.render_aov(cam, ss.W, ss.H, aov_spp=AOV_SPP, seed=ss.SEED, kernel=kernel, t_min=ss.T_MIN)  # noqa: E731
        if exp != ss.FRAME:
            _refused(exp, what, call)
            counts["refusals"] += 1
        else:
            got, st = call()
            aov = ss.expected_aov(side, AOV_SPP) if aov is None else aov
            assert st["kernel_used"] == kernel, what
            _same_frame(got, aov, what)
            counts["guides"] += 1
        what = "recipe %d: render_ao(kernel=%d, ao_spp=%d, rays_per_hit=%d)" % (index, kernel, AO_SPP, AO_RAYS)
        exp = ss.expected(rec, "render_ao", kernel)
        call = lambda: w.render_ao(cam, ss.W, ss.H, ao_spp=AO_SPP, rays_per_hit=AO_RAYS, seed=ss.SEED, kernel=kernel, t_min=ss.T_MIN)  # noqa: E731
        if exp != ss.FRAME:
            _refused(exp, what, call)
            counts["refusals"] += 1
        else:
            got, st = call()
            ao = ao_ref.ao(o, ss.W, ss.H, AO_SPP, AO_RAYS, seed=ss.SEED, t_min=ss.T_MIN)["ao"] if ao is None else ao
            assert st["kernel_used"] == kernel, what
            _same_frame(got, ao, what)
            counts["ao"] += 1

    # ---- what rt_render_sppm refuses (its frames: tests/test_soup_sppm_gpu.py) ----
    for kernel in (0, 1, 2, 5):
        exp = ss.expected(rec, "render_sppm", kernel)
        if exp != ss.FRAME:
            what = "recipe %d: render_sppm(kernel=%d)" % (index, kernel)
            _refused(exp, what, lambda: w.render_sppm(cam, width=8, height=8, spp=1, seed=ss.SEED, t_min=ss.T_MIN, kernel=kernel, iterations=1, photons_per_iter=500))
            counts["refusals"] += 1
            counts["sppm_refusals"] += 1
    assert counts["frames"] >= 3, "recipe %d: kernel 1 renders every recipe with integrator 0, in and out of LDS, and so does the automatic choice -- %s" % (index, counts)
    print("recipe %d: %s frames by (kernel, integrator): %s" % (index, " ".join("%s=%d" % kv for kv in counts.items()), sorted(by_kernel.items())))
