"""What tests/test_instance_walks_gpu.py relies on, checked without a device: every scene of tests/instance_scenes.py commits with the accel and
the compact instance data of kernels 5 / 6, and every ray family does what its name says by the oracle alone -- a fair share of the rays hit,
a fair share of them END on a triangle of a deferrable instance, the grazing rays fall on the side of the silhouette they were aimed at, and
both kinds of finite-t_max ray occur.  A generator that drifts out of these bounds is what has to change, not the bound."""
import numpy as np
import pytest

import instance_scenes as S

PAIRS = [(n, f) for n in S.SCENES for f in S.families(n)]


def _hits(name, family, key="full"):
    F = S.rays(name, family)
    return F, S.ref(name)[key].hit_batch(F["rays"], t_min=S.T_MIN, t_max=F["t_max"], n_workers=4)


@pytest.mark.parametrize("name", S.SCENES)
def test_scene_commits_with_compact_instance_data(name):
    info = S.world(name).info()
    assert info["accel_ok"] == 1 and info["accel_compact"] == 1 and info["accel_instances"] == len(S.spec(name)["instances"]), info


@pytest.mark.parametrize("name,family", PAIRS)
def test_family_is_sized_seeded_and_within_the_origin_bound(name, family):
    F = S.rays(name, family)
    rays = F["rays"]
    assert 2000 <= len(rays) <= 6000 and np.isfinite(rays).all() and (rays[:, 3:] != 0.0).any(axis=1).all()
    assert np.array_equal(S._build(name, family)["rays"], rays)        # seeded: the same rays again
    # the accel is proven for origins up to 64 times the largest absolute box coordinate (origin_limit, accel.cpp): stay within half of it
    assert np.abs(rays[:, :3]).max() <= 32.0 * S.ref(name)["extent"]
    if family in ("far", "graze"):
        assert np.abs(rays[:, :3]).max() >= 8.0 * S.ref(name)["extent"]


@pytest.mark.parametrize("name,family", [p for p in PAIRS if p[1] not in ("lattice", "t_max")])
def test_a_fair_share_of_the_rays_hit(name, family):
    F, full = _hits(name, family)
    assert not np.isnan(full).any()
    assert 0.25 <= full[:, 0].mean() <= 0.95, full[:, 0].mean()
    if family != "graze":  # ... and at least a quarter END on a deferrable instance: the same t against the scene's meshes alone
        _, mesh = _hits(name, family, "meshes")
        on_instance = (full[:, 0] == 1.0) & (mesh[:, 0] == 1.0) & (full[:, 1] == mesh[:, 1])
        assert on_instance.mean() >= 0.25, on_instance.mean()


@pytest.mark.parametrize("name", S.SCENES)
def test_components_family_has_its_special_directions(name):
    d = S.rays(name, "components")["rays"][:, 3:]
    assert ((d[::7] == 0.0).sum(axis=1) >= 1).all()
    n = np.linalg.norm(d, axis=1)
    k = np.arange(len(n))
    typical = np.median(n)
    assert (n[(k % 11 == 0) & (k % 13 != 0)] < 1e-3 * typical).all() and (n[(k % 13 == 0) & (k % 11 != 0)] > 1e3 * typical).all()


@pytest.mark.parametrize("name", S.SCENES)
def test_grazing_rays_fall_on_their_side_of_the_silhouette(name):
    F = S.rays(name, "graze")
    R = S.ref(name)
    hit = np.zeros(len(F["rays"]), dtype=bool)
    for i, solo in enumerate(R["solo"]):            # against the instance alone: another instance may lie behind its silhouette
        sel = F["inst"] == i
        assert sel.any()
        hit[sel] = solo.hit_batch(F["rays"][sel], t_min=S.T_MIN, n_workers=4)[:, 0] == 1.0
    for far in (0, 1):
        at = F["far"] == far
        assert hit[at & (F["eps"] == 1e-3)].all() and not hit[at & (F["eps"] == -1e-3)].any()
        closest = at & (np.abs(F["eps"]) == 1e-9)
        assert hit[closest].any() and not hit[closest].all()
        for eps in S.GRAZE_EPS:
            assert (at & (F["eps"] == eps)).sum() == (at & (F["eps"] == -eps)).sum() > 0


@pytest.mark.parametrize("name", S.SCENES)
def test_both_kinds_of_finite_t_max_occur(name):
    F, full = _hits(name, "t_max")
    assert np.isfinite(F["t_max"])
    between, before = F["kind"] == 0, F["kind"] == 1
    assert between.sum() >= 1000 and before.sum() >= 1000
    assert (full[between, 0] == 1.0).all() and (full[between, 1] < F["t_max"]).all()     # the first surface, and nothing behind it
    assert (full[before, 0] == 0.0).all()                                                # a miss
    # without the limit every one of them hits, the `between` rays at the same t
    free = S.ref(name)["full"].hit_batch(F["rays"], t_min=S.T_MIN, n_workers=4)
    assert (free[:, 0] == 1.0).all() and np.array_equal(free[between, 1], full[between, 1]) and (free[before, 1] > F["t_max"]).all()
    # ... nor a second surface in front of the limit: the rest of each ray, from just behind its first surface to the limit, meets nothing
    start = full[between, 1] * (1.0 + 1e-6)
    rest = F["rays"][between][start < F["t_max"]].copy()
    start = start[start < F["t_max"]]
    assert len(rest) >= 1000
    rest[:, :3] += rest[:, 3:] * start[:, None]
    rest[:, 3:] *= (F["t_max"] - start)[:, None]
    assert (S.ref(name)["full"].hit_batch(rest, t_min=0.0, t_max=1.0, n_workers=4)[:, 0] == 0.0).all()


def test_lattice_rays_are_dyadic_and_of_three_kinds():
    F, full = _hits("box", "lattice")
    rays = F["rays"]
    assert np.array_equal(rays * 8.0, np.round(rays * 8.0))
    lo, hi = np.array(S.BOX_AT), np.array(S.BOX_AT) + S.BOX_SCALE
    for kind, zeros in ((0, 0), (1, 1), (2, 2)):
        sel = F["kind"] == kind
        assert sel.sum() >= 100 and ((rays[sel, 3:] == 0.0).sum(axis=1) == zeros).all()
    in_plane = rays[F["kind"] == 1]
    axis = np.argmax(in_plane[:, 3:] == 0.0, axis=1)
    coord = in_plane[np.arange(len(in_plane)), axis]
    assert ((coord == lo[axis]) | (coord == hi[axis])).all()         # the origin lies in a face's plane and the ray stays in it
    # kind 0 rays pass through a mesh vertex, an edge's midpoint or a quad's centre at t = 4 exactly
    through = rays[F["kind"] == 0]
    p = (through[:, :3] + 4.0 * through[:, 3:] - lo) / (0.5 * S.BOX_SCALE / S.BOX_N)
    assert np.array_equal(p, np.round(p)) and (p >= 0).all() and (p <= 2 * S.BOX_N).all()
    assert full[F["kind"] == 0, 0].mean() > 0.9
