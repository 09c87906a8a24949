"""The corpus of tests/soup_scenes.py is not vacuous (the oracle alone, no device): its pins hold, every legal pair of axis values occurs,
every oracle frame is finite and lit, every primitive kind a recipe holds is reached by one of its test rays, a medium and an open
shutter change their frames, a coplanar pair ties in the oracle's own per-object hits, the test rays hold both answers of the any-hit
query, and every row of the rules table cites a line of include/rtamd.h that carries its words."""
import json
import os

import numpy as np
import pytest

import soup_scenes as ss
from conftest import GOLDEN, ROOT
from reach_scenes import NONZERO_FLOOR

PINS = os.path.join(GOLDEN, "soup_pins.json")
_SIDES = {}


def side(i):
    """the oracle's side of recipe i and its test rays with their records, built once"""
    if i not in _SIDES:
        rec = ss.recipe(i)
        s = ss.build_oracle(rec)
        rays = ss.test_rays(rec, s)
        _SIDES[i] = (rec, s, rays, ss.hit_records(rec, s, rays))
    return _SIDES[i]


def test_the_pins_hold():
    """the corpus and a digest of every recipe's description: neither the generator nor the selection drifts unnoticed"""
    with open(PINS) as f:
        pins = json.load(f)
    assert list(ss.corpus()) == pins["corpus"] and len(ss.corpus()) == ss.CORPUS_LENGTH == len(pins["corpus"])
    assert {str(i): ss.digest(ss.recipe(i)) for i in ss.corpus()} == pins["digests"]


def test_pairwise_coverage_is_complete():
    need, seen = ss.all_pairs(), set()
    print("%5s %5s  %s" % ("index", "new", "axes"))
    for i in ss.corpus():
        ax = ss.axes_of(ss.recipe(i))
        assert ss.legal(ax), i
        new = ss.pairs_of(ax) - seen
        assert new or ss.cells_of(ss.recipe(i)), "recipe %d adds no pair and fills no cell" % i
        seen |= ss.pairs_of(ax)
        print("%5d %5d  %s" % (i, len(new), " ".join("%s=%s" % kv for kv in ax.items())))
    assert seen == need, sorted(need - seen)[:5]
    print("%d recipes cover %d pairs" % (len(ss.corpus()), len(need)))
    assert not set(ss.corpus()) & (set(ss.REPLACED) | set(ss.VACUOUS)) and len(ss.REPLACED) <= 2


def test_every_rule_cites_the_header():
    with open(os.path.join(ROOT, "include", "rtamd.h")) as f:
        lines = f.read().split("\n")
    for entries, _, result, line, words in ss.RULES:
        assert words in lines[line - 1], "include/rtamd.h:%d does not say %r" % (line, words)
        assert result in (ss.ARG, ss.UNSUPPORTED) and entries


def _frame(s, integrator):
    return s.b.render(ss.W, ss.H, ss.SPP, seed=ss.SEED, t_min=ss.T_MIN, integrator=integrator)[0]


@pytest.mark.parametrize("i", ss.corpus())
def test_frames_are_finite_and_lit(i):
    rec, s, _, _ = side(i)
    for integ in (0, 1):
        if ss.expected(rec, "render", 1, integ) != ss.FRAME:
            continue
        img = _frame(s, integ)
        assert np.isfinite(img).all(), "recipe %d integrator %d: a channel is not finite" % (i, integ)
        lit = float((img > 0).any(axis=2).mean())
        assert lit >= NONZERO_FLOOR, "recipe %d integrator %d: only %.3f of the frame is lit" % (i, integ, lit)


@pytest.mark.parametrize("i", ss.corpus())
def test_every_primitive_kind_is_reached(i):
    rec, s, rays, hits = side(i)
    groups = set(ss.group_of(s, hits[hits[:, 0] == 1.0, 11].astype(int)))
    assert None not in groups, "recipe %d: a prim_id outside every recorded object" % i
    missing = [g for g in ss.required_groups(rec) if g not in groups]
    assert not missing, "recipe %d: no test ray's closest hit is on %s (reached: %s)" % (i, missing, sorted(groups))


@pytest.mark.parametrize("i", [i for i in ss.corpus() if ss.facts(ss.recipe(i))["media"]])
def test_a_medium_changes_its_frame(i):
    rec, s, _, _ = side(i)
    assert not np.array_equal(_frame(s, 0), _frame(ss.build_oracle(rec, drop_medium=True), 0)), "recipe %d: the frame without its medium is the same" % i


@pytest.mark.parametrize("i", [i for i in ss.corpus() if ss.facts(ss.recipe(i))["moving"]])
def test_moving_spheres_change_their_frame(i):
    rec, s, _, _ = side(i)
    assert not np.array_equal(_frame(s, 0), _frame(ss.build_oracle(rec, close_shutter=True), 0)), "recipe %d: the frame with a closed shutter is the same" % i


@pytest.mark.parametrize("i", [i for i in ss.corpus() if dict(ss.recipe(i))["pair"] is not None])
def test_a_coplanar_pair_ties(i):
    """a test ray whose two nearest candidates tie: both objects of the pair answer the oracle's per-object hit with the same t, and that
    t is the t of the scene's closest hit"""
    rec, s, rays, hits = side(i)
    a, b = (s.built[k] for k in dict(rec)["pair"])
    ties = 0
    for ray, h in zip(rays, hits):
        if h[0] != 1.0:
            continue
        ha, hb = s.b.hit(ray[:3], ray[3:], t_min=ss.T_MIN, obj=a), s.b.hit(ray[:3], ray[3:], t_min=ss.T_MIN, obj=b)
        ties += int(ha is not None and hb is not None and ha["t"] == hb["t"] == h[1])
    print("recipe %d: %d rays tie" % (i, ties))
    assert ties >= 1, "recipe %d: no test ray ties on the coplanar pair" % i


@pytest.mark.parametrize("i", ss.corpus())
def test_the_explicit_rays_hold_both_answers_of_the_any_hit_query(i):
    """the explicit walk rays alone -- no camera ray that leaves for the background helps -- hit and miss; where the any-hit walk runs
    (no medium, no moving spheres) the rows it is asked hold both answers too, among them rows at the oracle's own t"""
    rec, s, _, _ = side(i)
    explicit = dict(ss.test_ray_parts(rec, s))["explicit"]
    hit = ss.hit_records(rec, s, explicit)[:, 0]
    assert len(explicit) == ss.N_EXPLICIT and 0 < hit.sum() < len(explicit), "recipe %d: %d of %d explicit rays hit" % (i, int(hit.sum()), len(explicit))
    if ss.expected(rec, "debug_occluded", 2) == ss.FRAME:
        rows, exp = ss.occlusion_rows(s, explicit)
        assert len(rows) > len(explicit) and exp[len(explicit):].any() and not exp[len(explicit):].all(), i


def test_every_cell_is_a_frame_on_several_scenes():
    """every kernel x integrator of the render matrix and every other entry point answers with a frame (records, rows), not a refusal, on
    at least MIN_SCENES scenes, and the automatic choice is kernel 5 on as many; the table is printed"""
    count = {c: [] for c in ss.CELLS}
    for i in ss.corpus():
        for c in ss.cells_of(ss.recipe(i)):
            count[c].append(i)
    for c in ss.CELLS:
        print("%-16s kernel %d integrator %d: %2d scenes %s" % (c[0], c[1], c[2], len(count[c]), count[c][:8]))
    assert all(len(v) >= ss.MIN_SCENES for v in count.values()) and ss.MIN_SCENES >= 3
    service = [i for i in count[("render", 5, 0)]]
    assert any(ss.axes_of(ss.recipe(i))["big_mesh"] for i in service) and any(not ss.axes_of(ss.recipe(i))["big_mesh"] for i in service)


def test_rules_spot_checks():
    """the table on calls whose answer the header states in so many words"""
    by = {}
    for i in ss.corpus():
        rec = ss.recipe(i)
        f = ss.facts(rec)
        by.setdefault((f["media"], f["moving"], f["nest"], f["background"]), rec)
    for (media, moving, nest, bg), rec in by.items():
        for k in (5, 6):
            if media or moving or nest or bg:
                assert ss.expected(rec, "render", k, 0) == ss.UNSUPPORTED
        if media or moving:
            assert ss.expected(rec, "render", 1, 1) in (ss.ARG, ss.UNSUPPORTED) and ss.expected(rec, "render_ao", 1) == ss.UNSUPPORTED
            assert ss.expected(rec, "render_aov", 2) == ss.UNSUPPORTED and ss.expected(rec, "debug_occluded", 1) == ss.UNSUPPORTED
        assert ss.expected(rec, "render", 1, 0) == ss.FRAME and ss.expected(rec, "render", 0, 0) == ss.FRAME
