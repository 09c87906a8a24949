"""The SPPM sub-corpus of tests/soup_scenes.py is what it says and is not vacuous (the oracle alone, no device): SPPM_CORPUS equals its
definition, its pairs are covered, its cells are full and its pins hold; every rule row cites a line of include/rtamd.h that carries its
words; no object light of an eligible recipe touches a medium; and under SPPM_CFG every scene's oracle frame is finite and lit, both photon
maps fill, and the pixels gather -- the reference's estimate is 0 / 0 = NaN where a map's radius^2 is 0, and a NaN that equals a NaN proves
nothing, so tests/test_soup_sppm_gpu.py compares only frames that pass CONDITIONS here."""
import json
import os

import numpy as np
import pytest

import soup_scenes as ss
from conftest import GOLDEN, ROOT

PINS = os.path.join(GOLDEN, "soup_pins.json")
N_WORKERS = 16
NPIX = ss.W * ss.H
# name -> the least value of the measure conditions() returns under it
CONDITIONS = dict(finite=0.90, lit=0.25, global_total=1, caustic_total=1, gathered=0.25, it0_global=1, it0_caustic=1, it0_valid=0.25)
_RUNS = {}


def run(i):
    """recipe i under SPPM_CFG on the oracle, computed once: (recipe, frame, statistics, totals, iteration 0's maps and points)"""
    if i not in _RUNS:
        rec = ss.recipe(i)
        o = ss.build_oracle_sppm(rec).b
        img, st, tot = o.render_sppm(ss.W, ss.H, ss.SPPM_SPP, seed=ss.SEED, t_min=ss.T_MIN, n_workers=N_WORKERS, **ss.SPPM_CFG)
        it0 = o.sppm_iteration(ss.W, ss.H, 0, ss.SPPM_CFG["photons_per_iter"], ss.SPPM_CFG["k_global"], ss.SPPM_CFG["k_caustic"], seed=ss.SEED)
        _RUNS[i] = (rec, img, st, tot, it0)
    return _RUNS[i]


def conditions(i):
    """the measures of CONDITIONS for recipe i"""
    _, img, st, tot, (g, c, gp, _) = run(i)
    finite = np.isfinite(img).all(axis=2)
    return dict(finite=float(finite.mean()), lit=float((finite & (np.where(finite[..., None], img, 0.0).sum(axis=2) > 0)).mean()),
                global_total=tot[0], caustic_total=tot[1], gathered=float((st[..., 4] > 0).mean()),
                it0_global=len(g), it0_caustic=len(c), it0_valid=float((gp[:, 0] != 0).mean()))


def test_the_corpus_is_its_definition_and_the_pins_hold():
    out, need = ss.sppm_corpus()
    assert ss.SPPM_CORPUS == out and ss.SPPM_CORPUS_LENGTH == len(out)
    with open(PINS) as f:
        pins = json.load(f)
    assert list(out) == pins["sppm_corpus"] and {str(i): ss.digest(ss.recipe(i)) for i in out} == pins["sppm_digests"]
    assert not set(out) & (set(ss.SPPM_VACUOUS) | set(ss.SPPM_REPLACED)) and len(ss.SPPM_REPLACED) <= 2
    assert set(ss.SPPM_VACUOUS) | set(ss.SPPM_REPLACED) <= set(ss.sppm_eligible())
    assert set(ss.SPPM_VACUOUS.values()) <= set(CONDITIONS)


def test_pairs_are_covered_and_cells_are_full():
    out, need = ss.sppm_corpus()
    seen, count = set(), {c: [] for c in ss.SPPM_CELLS}
    print("%5s %5s  %s" % ("index", "new", "axes"))
    for i in out:
        rec = ss.recipe(i)
        assert ss.expected(rec, "render_sppm", 1) == ss.FRAME and ss.expected(rec, "render_sppm", 0) == ss.FRAME, i
        new = ss.sppm_pairs_of(rec) - seen
        assert new or any(len(count[c]) < ss.MIN_SCENES for c in ss.sppm_cells(rec)), "recipe %d adds no pair and fills no cell" % i
        seen |= ss.sppm_pairs_of(rec)
        for c in ss.sppm_cells(rec):
            count[c].append(i)
        print("%5d %5d  %s" % (i, len(new), " ".join("%s=%s" % kv for kv in ss.sppm_axes(rec).items())))
    assert seen == need, sorted(need - seen)[:5]
    every = set().union(*(ss.sppm_pairs_of(ss.recipe(i)) for i in ss.sppm_eligible()))
    lost = every - need       # pairs only recipes that were passed over show
    print("%d recipes of %d eligible below %d cover %d pairs (%d more only on passed-over recipes)" % (len(out), len(ss.sppm_eligible()), ss.SPPM_RANGE, len(need), len(lost)))
    assert not lost, sorted(lost)[:5]
    for c in ss.SPPM_CELLS:
        print("%-12s kernel %d: %2d scenes %s" % (c[0], c[1], len(count[c]), count[c][:8]))
    assert all(len(v) >= ss.MIN_SCENES for v in count.values()) and ss.MIN_SCENES >= 3


def test_every_sppm_rule_cites_the_header():
    with open(os.path.join(ROOT, "include", "rtamd.h")) as f:
        lines = f.read().split("\n")
    rows = [r for r in ss.RULES if "render_sppm" in r[0].split()]
    assert len(rows) >= 7
    for _, _, result, line, words in rows:
        assert words in lines[line - 1], "include/rtamd.h:%d does not say %r" % (line, words)
        assert result in (ss.ARG, ss.UNSUPPORTED)
    # the order of the refusals, where two with different codes apply: a background or area lights answer before the missing lights
    assert "a background, area lights (RT_ERR_UNSUPPORTED), a scene without object lights: RT_ERR_ARG" in lines[433 - 1]


def test_rules_spot_checks():
    """the table on calls whose answer the header states in so many words; kernel 6 is never a frame"""
    seen = set()
    for i in range(400):
        rec = ss.recipe(i)
        f = ss.facts(rec)
        exp = [ss.expected(rec, "render_sppm", k) for k in (0, 1, 2, 5)]
        assert ss.expected(rec, "render_sppm", 6) == ss.WITHHELD != ss.FRAME
        if f["background"] or f["area"] or f["moving"] or f["noise"]:
            assert exp == [ss.UNSUPPORTED] * 4, i
        elif not f["lights"]:
            assert exp == [ss.ARG] * 4, i
        else:
            assert exp[0] == exp[1] == ss.FRAME, i
            assert exp[2] == (ss.UNSUPPORTED if f["media_xf"] else ss.FRAME) and (exp[3] == ss.FRAME) == f["service"], i
        if f["background"] and not f["lights"]:
            seen.add("background and no object light")
        seen.add(exp[1])
    assert "background and no object light" in seen and {ss.FRAME, ss.UNSUPPORTED} <= seen


def test_no_object_light_touches_a_medium():
    """`a light inside a ConstantMedium` does not arise: from the descriptions alone, the box of every object light of every eligible
    recipe lies clear of a sphere around every medium of it"""
    gaps = {i: ss.lights_clear_of_media(ss.recipe(i)) for i in ss.sppm_eligible()}
    with_media = {i: g for i, g in gaps.items() if np.isfinite(g)}
    print("%d eligible recipes hold a medium; the least gap is %.3f scene units (recipe %d)" % (len(with_media), min(with_media.values()), min(with_media, key=with_media.get)))
    assert len(with_media) >= 10 and min(with_media.values()) > 0.0
    assert all(np.isfinite(gaps[i]) == ss.facts(ss.recipe(i))["media"] for i in gaps)


@pytest.mark.parametrize("i", ss.SPPM_CORPUS)
def test_frames_are_finite_and_lit_and_the_maps_fill(i):
    got = conditions(i)
    print("recipe %d: %s" % (i, " ".join("%s=%.4g" % kv for kv in got.items())))
    for name, floor in CONDITIONS.items():
        assert got[name] >= floor, "recipe %d: %s is %.4g, below %.4g" % (i, name, got[name], floor)


@pytest.mark.parametrize("i", sorted(ss.SPPM_VACUOUS))
def test_a_vacuous_recipe_still_fails_its_condition(i):
    name = ss.SPPM_VACUOUS[i]
    got = conditions(i)
    print("recipe %d: %s" % (i, " ".join("%s=%.4g" % kv for kv in got.items())))
    assert got[name] < CONDITIONS[name], "recipe %d: %s is %.4g now" % (i, name, got[name])


def test_the_lights_flux_reaches_the_oracle():
    """build_oracle leaves every light's flux at the oracle's default (path tracing never reads it); under SPPM the photon power is
    flux x scale, and the frame of build_oracle_sppm differs from the frame without it"""
    i = ss.SPPM_CORPUS[0]
    plain = ss.build_oracle(ss.recipe(i)).b.render_sppm(ss.W, ss.H, ss.SPPM_SPP, seed=ss.SEED, t_min=ss.T_MIN, n_workers=N_WORKERS, **ss.SPPM_CFG)
    lit = np.isfinite(run(i)[1]).all(axis=2) & (run(i)[1] > 0).any(axis=2)
    assert lit.any() and not np.array_equal(plain[0][lit], run(i)[1][lit])


def _holds(rec, kind):
    out = []
    for d in dict(rec)["items"]:
        ss._walk(d, lambda x: out.extend(m for m in x if isinstance(m, tuple) and m and m[0] == "lambertian" and m[1][0] == kind))
    return bool(out)


def test_the_corpus_reaches_textures_caustics_at_every_scale_and_a_fog_under_a_transform():
    recs = {i: ss.recipe(i) for i in ss.SPPM_CORPUS}
    image = [i for i, r in recs.items() if _holds(r, "image")]
    checker = [i for i, r in recs.items() if _holds(r, "checker")]
    fog_xf = [i for i, r in recs.items() if ss.facts(r)["media_xf"]]
    print("image-textured Lambertians: %s\nchecker-textured: %s\na fog under a Transform: %s" % (image, checker, fog_xf))
    assert image and checker and fog_xf
    for scale in (0.01, 1.0, 100.0):
        caustic = [i for i, r in recs.items() if dict(r)["scale"] == scale and run(i)[3][1] > 0]
        print("scale %g: %d scenes store caustic photons" % (scale, len(caustic)))
        assert caustic, scale
    floors = {name: min(conditions(i)[name] for i in recs) for name in CONDITIONS}
    print("minima over the corpus: %s" % " ".join("%s=%.4g" % kv for kv in floors.items()))
