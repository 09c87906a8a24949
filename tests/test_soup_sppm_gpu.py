"""The composed scenes of tests/soup_scenes.py through rt_render_sppm, stage by stage: one test per scene of SPPM_CORPUS, HIP against the
oracle, everything bit for bit (a NaN equals only a NaN at the same pixel and channel).

Per scene, in this order, so that a failure names where a difference arises:
  1. the photon pass and the eye pass of iterations 0 and 1 (rt_debug_sppm_trace_device against oracle.sppm_iteration: both maps as
     multisets of rows, the gather points row for row, S, and the NEST and MEDIA bits of the variant word against the recipe's facts);
  2. whole renders through kernels 0, 1, 2 and 5 with the scene in LDS and kernels 1 and 2 out of it: where soup_scenes.expected() says
     FRAME the frame, the [H, W, 10] statistics and both photon totals are oracle.render_sppm's, else the call fails with exactly the
     predicted rt_status;
  3. rt_render_sppm_tiles_device over a 3-rank partition, stitched, is the one-call frame;
  4. the tuning switches sppm_photon_capacity=64 (grow-and-retry) and sppm_knn_candidates=0 (selection outside LDS) change nothing.
A difference in stage 1's maps lies in the photon pass, in its points in the eye pass; statistics that differ after stage 1 passed lie in
the gather, a frame that differs over equal statistics in the final pass.  tests/test_soup_sppm_scenes.py shows without a device that the
oracle's frames are finite and lit.  No call uses kernel 6 (soup_scenes.WITHHELD)."""
import numpy as np
import pytest

import soup_scenes as ss
import sppm_trace_cases as tc

pytestmark = pytest.mark.gpu

WORLD_SIZE = 3
P = ss.SPPM_CFG["photons_per_iter"]


def _first_bad(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    bad = ((got != exp) & ~(np.isnan(got) & np.isnan(exp))).reshape(len(got), -1).any(axis=1)
    return int(bad.sum()), (int(np.flatnonzero(bad)[0]) if bad.any() else -1)


def _same_pixels(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    n, k = _first_bad(got.reshape(ss.W * ss.H, -1), exp.reshape(ss.W * ss.H, -1))
    if n:
        y, x = divmod(k, ss.W)
        raise AssertionError("%s: %d of %d pixels differ, first (x=%d, y=%d): hip=%s oracle=%s" % (what, n, ss.W * ss.H, x, y, got[y, x].tolist(), exp[y, x].tolist()))


def _same_render(got, exp, what):
    """totals, then statistics, then the frame: the first that differs is the earliest stage that went wrong"""
    assert got[2] == exp[2], "%s, photon pass: totals hip=%s oracle=%s" % (what, got[2], exp[2])
    _same_pixels(got[1], exp[1], what + ", gather: statistics")
    _same_pixels(got[0], exp[0], what + ", final pass: frame")


def _refused(code, what, fn):
    import rtamd
    try:
        fn()
    except rtamd.RtError as e:
        assert e.code == code, "%s: refused with %d (%s), the header says %d" % (what, e.code, e, code)
        return
    raise AssertionError("%s: ran, the header says it is refused with %d" % (what, code))


def _trace(index, rec, w, cam, o, it):
    """stage 1 for one iteration -> (photons compared, points compared)"""
    what = "recipe %d, iteration %d" % (index, it)
    g, cau, gp, S = o.sppm_iteration(ss.W, ss.H, it, P, ss.SPPM_CFG["k_global"], ss.SPPM_CFG["k_caustic"], seed=ss.SEED)
    dev = w.debug_sppm_trace(cam, ss.W, ss.H, iteration=it, photons_per_iter=P, seed=ss.SEED)
    f = ss.facts(rec)
    assert not dev["unit_zero"], what
    assert dev["S"] == S, "%s: S hip=%d oracle=%d" % (what, dev["S"], S)
    assert bool(dev["variant"] & tc.NEST) == f["nest"] and bool(dev["variant"] & tc.MEDIA) == f["media"], "%s: variant %d, nest %s media %s" % (what, dev["variant"], f["nest"], f["media"])
    assert not (dev["variant"] & tc.NEST and dev["variant"] & tc.ACCEL), what
    for name, got, exp in (("global", dev["global"], g), ("caustic", dev["caustic"], cau)):
        a, b = tc.sorted_rows(got), tc.sorted_rows(exp)
        assert a.shape == b.shape, "%s, photon pass, %s map: %d photons, the oracle stores %d" % (what, name, len(a), len(b))
        bad = (a != b).any(axis=1)
        assert not bad.any(), "%s, photon pass, %s map: %d of %d sorted rows differ, first %d: hip=%r oracle=%r" % (
            what, name, bad.sum(), len(bad), np.flatnonzero(bad)[0], a[bad][0].view(np.float64).tolist(), b[bad][0].view(np.float64).tolist())
    pts = dev["points"] + 0.0
    bad = (pts.view(np.uint64) != (gp + 0.0).view(np.uint64)).any(axis=1)
    assert not bad.any(), "%s, eye pass: %d of %d gather points differ, first pixel %d: hip=%r oracle=%r" % (
        what, bad.sum(), len(bad), np.flatnonzero(bad)[0], pts[bad][0].tolist(), gp[bad][0].tolist())
    return len(g) + len(cau), len(pts)


@pytest.mark.parametrize("index", ss.SPPM_CORPUS)
def test_soup_sppm(index, tuning):
    import torch
    import rtamd
    from rtamd.distributed import TileLayout, stitch_host
    rec = ss.recipe(index)
    w, cam, side = ss.build_pair_sppm(rec)
    o = side.b
    counts = dict(photons=0, points=0, frames=0, refusals=0, stitched=0, switches=0)
    by_kernel = {}

    # ---- 1. the photon pass and the eye pass ----
    for it in (0, 1):
        n, m = _trace(index, rec, w, cam, o, it)
        counts["photons"] += n
        counts["points"] += m

    # ---- 2. whole renders ----
    exp = o.render_sppm(ss.W, ss.H, ss.SPPM_SPP, seed=ss.SEED, t_min=ss.T_MIN, n_workers=16, **ss.SPPM_CFG)
    render = lambda kernel: w.render_sppm(cam, width=ss.W, height=ss.H, spp=ss.SPPM_SPP, seed=ss.SEED, t_min=ss.T_MIN, kernel=kernel, **ss.SPPM_CFG)  # noqa: E731
    for no_lds in (0, 1):
        tuning(no_lds=no_lds)
        # (kernel 0 last: where kernel 5 has answered as predicted, the automatic choice has no scene on which it could take kernel 6)
        for kernel in ((1, 2, 5, 0) if no_lds == 0 else (1, 2)):
            what = "recipe %d: render_sppm(kernel=%d, no_lds=%d)" % (index, kernel, no_lds)
            want = ss.expected(rec, "render_sppm", kernel)
            if want != ss.FRAME:
                _refused(want, what, lambda: render(kernel))
                counts["refusals"] += 1
                continue
            got = render(kernel)
            used = kernel if kernel else ss.auto_kernel(rec, 0, "render_sppm")
            assert got[3]["kernel_used"] == used, "%s: ran kernel %d, the header says %d" % (what, got[3]["kernel_used"], used)
            assert not (no_lds and got[3]["scene_in_lds"]), what
            _same_render(got, exp, what)
            by_kernel[used] = by_kernel.get(used, 0) + 1
            counts["frames"] += 1
    tuning()

    # ---- 3. a 3-rank partition stitches to the one-call frame ----
    lay = TileLayout(ss.W, ss.H, WORLD_SIZE)
    parts = []
    for r in range(WORLD_SIZE):
        p = rtamd.default_params(width=ss.W, height=ss.H, spp=ss.SPPM_SPP, seed=ss.SEED, t_min=ss.T_MIN, rank=r, world=WORLD_SIZE)
        buf = torch.zeros(lay.stride * 64 * 3, dtype=torch.float64, device="cuda:0")
        w.render_sppm_tiles_device(cam, p, buf.data_ptr(), **ss.SPPM_CFG)
        parts.append(buf.cpu())
    _same_pixels(stitch_host(torch.cat(parts).numpy(), lay), exp[0], "recipe %d: %d ranks stitched" % (index, WORLD_SIZE))
    counts["stitched"] += 1

    # ---- 4. the tuning switches change how, never what ----
    for setting in (dict(sppm_photon_capacity=64), dict(sppm_knn_candidates=0)):
        tuning(**setting)
        _same_render(render(0), exp, "recipe %d: render_sppm under %s" % (index, setting))
        counts["switches"] += 1
    tuning()
    assert counts["frames"] >= 3 and by_kernel.get(1, 0) >= 2, "recipe %d: kernel 1 renders every scene in and out of LDS, and so does the automatic choice -- %s" % (index, counts)
    print("recipe %d: %s frames by kernel: %s totals %s" % (index, " ".join("%s=%d" % kv for kv in counts.items()), sorted(by_kernel.items()), exp[2]))
