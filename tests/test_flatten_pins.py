"""What rt_scene_commit's flattener writes is the contract between the host and every kernel: for every scene of tests/flatten_corpus.py
the fingerprint of the blob, rt_scene_info and the lowered area-light triangles are what tests/golden/flatten_pins.json recorded (on the
commit named in the file), a scene with two defects is refused for the same one of them with the same words, and a commit that failed
leaves a scene that still commits to the blob of a clean build.  No device is needed."""
import json

import pytest

import flatten_corpus as fc

PINS = json.load(open(fc.PINS))


def test_the_file_pins_the_corpus():
    assert sorted(PINS["scenes"]) == sorted(fc.CORPUS) and sorted(PINS["refusals"]) == sorted(fc.REFUSALS)
    assert len(PINS["recorded_on"]) == 40


@pytest.mark.parametrize("name", sorted(fc.CORPUS))
def test_flattened_scene_is_unchanged(name):
    got, pin = fc.observe(fc.CORPUS[name]()), PINS["scenes"][name]
    assert got["fingerprint"] == pin["fingerprint"]
    assert got["info"] == pin["info"]
    assert got.get("area_tris") == pin.get("area_tris")


@pytest.mark.parametrize("name", sorted(fc.REFUSALS))
def test_the_same_defect_is_reported_first(name):
    assert fc.refusal(name) == PINS["refusals"][name]


def test_a_scene_file_of_the_older_schema_is_refused_by_the_loader():
    assert fc.unloadable("test.json") == PINS["unloadable"]["test.json"]


def test_a_failed_commit_leaves_the_scene_as_it_was():
    got, pin = fc.recommit(), PINS["recommit"]
    assert got == pin
    assert got["first"][0] < 0 and got["second"] == got["clean"] and got["second"]["info"]["committed"] == 1
