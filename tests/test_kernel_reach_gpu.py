"""The render-kernel instantiations no other test launches (tests/reach_scenes.py: one case each), HIP against the oracle bit for bit.

Every case renders the smallest call that selects its instantiation and asserts, besides the frame, the preconditions of the
selection that a caller can see -- kernel_used, scene_in_lds, the scene's info() fields, and for the twins chosen by a tile count
(kernel 2's out-of-order fold, kernel 5's early fold) rtamd.tiles_owned against the waves of the call's own launch, on the side the
case needs -- so that a change to render_tiles' rules fails here instead of sending the case to another kernel unnoticed.  Which
kernel a case really launched is measured, not asserted: tools/launch_coverage.py profiles this file, and
tests/test_launch_coverage_record.py holds its record to the cases' names.

Small cases are 20 x 12 frames (partial tiles on both edges).  A case on the large side of a threshold takes the smallest frame
that crosses it, computed from the stats of an 8 x 8 probe render of the same call (no size is written down here), at 1 or 2 spp; it is
compared on tests/seeded_windows.py's windows through oracle.Scene.render(window=...) -- the four corners: first tile, last tile,
partial right and bottom tiles -- and then as a whole frame (the oracle takes a fraction of a second for it).  SPPM frames
(rt_render_sppm has no window) are compared whole: photon totals, the per-pixel statistics and the image.  Oracle frames are
computed once per (scene, call) and shared between the cases that differ in kernel or LDS residency only."""
import numpy as np
import pytest

import reach_scenes as rs
from seeded_windows import seeded_windows

pytestmark = pytest.mark.gpu

_ORACLE = {}
NONZERO_FLOOR = rs.NONZERO_FLOOR


def _oracle(case, W, H, spp, seed, cfg):
    key = (case.scene, case.mode, case.integrator, W, H, spp, seed)
    if key not in _ORACLE:
        o = rs.pair(case.scene)[2]
        if case.mode == "sppm":
            _ORACLE[key] = o.render_sppm(W, H, spp, seed=seed, n_workers=16, **cfg)
        else:
            _ORACLE[key] = o.render(W, H, spp, seed=seed, n_workers=16, integrator=case.integrator)[0]
    return _ORACLE[key]


def _render(case, W, H, spp, seed, cfg):
    """-> (image, stats dict, (per-pixel SPPM statistics, photon totals) or None)"""
    w, cam, _, kw = rs.pair(case.scene)
    if case.mode == "sppm":
        img, pix, tot, st = w.render_sppm(cam, width=W, height=H, spp=spp, seed=seed, kernel=case.kernel_id, **cfg)
        return img, st, (pix, tot)
    img, st = w.render(cam, width=W, height=H, spp=spp, seed=seed, kernel=case.kernel_id, integrator=case.integrator, **kw)
    return img, st, None


def _waves(st):
    return st["grid_blocks"] * st["block_threads"] // 64


def _tiles(W, H, spp):
    import rtamd
    return rtamd.tiles_owned(rtamd.default_params(width=W, height=H, spp=spp))


def _smallest_frame(tiles):
    """the smallest near-square frame of at least `tiles` 8 x 8 tiles whose last column and last row of tiles are partial"""
    tx = int(np.ceil(np.sqrt(tiles)))
    ty = -(-tiles // tx)
    return 8 * tx - 3, 8 * ty - 5


def _same(got, exp, what):
    if not np.array_equal(got, exp, equal_nan=True):
        bad = ((got != exp) & ~(np.isnan(got) & np.isnan(exp))).any(axis=-1)
        y, x = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d pixels differ, first (x=%d, y=%d): hip=%s oracle=%s" % (what, int(bad.sum()), bad.size, x, y, got[y, x].tolist(), exp[y, x].tolist()))


@pytest.mark.parametrize("case", rs.CASES, ids=[c.kernel.replace(" ", "") for c in rs.CASES])
def test_reach(case, tuning):
    w, _, o, _ = rs.pair(case.scene)
    info = w.info()
    if case.kernel_id == 1:
        assert info["committed"] == 1
    else:
        assert info["accel_ok"] == 1
    for k, v in rs.INSTANCE_INFO.get(case.scene, {}).items():
        assert info[k] == v, (k, info[k], v)
    if case.scene in ("n4", "n6", "nested_fog", "nested_fog_sky"):
        assert info["n_xforms"] >= 2  # nested chains
    tuning(no_lds=case.no_lds)
    large = case.side in ("fold", "late")
    cfg = rs.SPPM_LARGE if large else rs.SPPM_SMALL
    if large:
        _, probe, _ = _render(case, 8, 8, 1, 5, cfg)
        need = _waves(probe) * (2 if case.side == "late" else 1)
        W, H = _smallest_frame(need)
        spp = 2 if case.integrator == 0 else 1  # (integrator 0 finds the lamps by chance: 2 spp light one pixel in seven)
        assert _tiles(W, H, spp) >= need > _tiles(W - 8, H, spp)
    else:
        (W, H), spp = rs.SMALL, rs.SMALL_SPP[case.mode]
    seed = 5
    img, st, sppm = _render(case, W, H, spp, seed, cfg)
    tiles, waves = _tiles(W, H, spp), _waves(st)
    print("%s: %d x %d x %d spp, tiles %d, waves %d, kernel_ms %.3f" % (case.kernel, W, H, spp, tiles, waves, st["kernel_ms"]))
    assert st["kernel_used"] == case.kernel_id and st["scene_in_lds"] == rs.lds_of(case), st
    if case.side in ("pool", "early"):
        assert tiles < waves, (tiles, waves)
    elif case.side == "fold":
        assert tiles >= waves, (tiles, waves)
    elif case.side == "late":
        assert tiles >= 2 * waves, (tiles, waves)
    exp = _oracle(case, W, H, spp, seed, cfg)
    if sppm is not None:
        eimg, epix, etot = exp
        assert sppm[1] == etot and etot[0] > 0, (sppm[1], etot)
        assert np.array_equal(sppm[0], epix), "per-pixel SPPM statistics differ in %d pixels" % int((sppm[0] != epix).any(axis=2).sum())
        exp = eimg
    elif large:
        for x0, y0 in seeded_windows(W, H, seed):
            win = o.render(W, H, spp, seed=seed, window=(x0, y0, x0 + 8, y0 + 8), integrator=case.integrator)[0]
            _same(img[y0:y0 + 8, x0:x0 + 8], win, "%s window (%d, %d)" % (case.kernel, x0, y0))
    assert float((exp > 0).any(axis=2).mean()) > NONZERO_FLOOR
    _same(img, exp, case.kernel)
