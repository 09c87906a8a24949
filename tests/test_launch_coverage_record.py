"""The record of which compiled kernels the GPU tests launch (tests/golden/kernel_launch_coverage.json), held to the tree without a
device: its kernels.hip universe is exactly the committed resource report's, every kernel has a status and none is `unreached`, the
`launched` entries name test files that exist, the `unreachable` ones a rule at a file:line that exists, the `too_large` ones a
measured time, the `withheld` ones (cases that hung on the device) their reason, and every instantiation a case of
tests/reach_scenes.py names was launched by tests/test_kernel_reach_gpu.py.

Regenerating the record (on a machine with an MI355X, from the repository root, on a built tree whose kernels.resource.txt names every
compiled kernel -- `make asm`; the file takes the new or changed rows, the others stay):
    python tools/launch_coverage.py                     # every file with gpu-marked tests, one rocprofv3 child each
or, split over several visits:
    python tools/launch_coverage.py --files tests/test_a.py ... --out part1.json
    python tools/launch_coverage.py --files tests/test_kernel_reach_gpu.py --out part2.json
    python tools/launch_coverage.py --merge part1.json part2.json
A kernel the record then shows `unreached` needs a case in tests/reach_scenes.py (CASES), or an entry in its UNREACHABLE / TOO_LARGE
tables if no valid call selects it / its smallest selecting workload is slower than the suite's slowest test.
`python tools/launch_coverage.py --table` prints the summary by kernel family."""
import json
import os
import re
import sys

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import launch_coverage as lc  # noqa: E402
import reach_scenes  # noqa: E402

STATUSES = ("launched", "unreachable", "too_large", "withheld", "unreached")


def _record():
    with open(os.path.join(GOLDEN, "kernel_launch_coverage.json")) as f:
        return json.load(f)


def test_the_universe_is_the_resource_report():
    rec = _record()
    with open(lc.RESOURCE) as f:
        names = lc.resource_names(f.read())
    assert len(names) == len(set(names))
    got = {m for m, k in rec["kernels"].items() if k["source"] == "kernels.hip"}
    assert got == set(names), "regenerate the record: only in it %s, only in kernels.resource.txt %s" % (sorted(got - set(names))[:4], sorted(set(names) - got)[:4])
    assert {k["source"] for k in rec["kernels"].values()} == {"kernels.hip", "denoise.hip"}
    shorts = [k["name"] for k in rec["kernels"].values()]
    assert len(shorts) == len(set(shorts))  # the short form names an instantiation uniquely
    assert [lc.short_name(d) for d in lc.demangle(sorted(rec["kernels"]))] == [rec["kernels"][m]["name"] for m in sorted(rec["kernels"])]
    if rec["kernel_source_sha16"] != lc.source_sha16():
        print("note: the record was measured on device sources %s, this tree has %s: it is stale for this build (python tools/launch_coverage.py)"
              % (rec["kernel_source_sha16"], lc.source_sha16()))


def test_every_kernel_has_a_status_and_none_is_unreached():
    rec = _record()
    assert rec["head"] and rec["rocprofv3"] and rec["names"] == "mangled"
    for m, k in rec["kernels"].items():
        assert k.get("status") in STATUSES, (m, k)
    assert [k["name"] for k in rec["kernels"].values() if k["status"] == "unreached"] == []


def test_launched_entries_name_test_files_that_exist():
    rec = _record()
    for k in rec["kernels"].values():
        if k["status"] == "launched":
            assert k["by"] and all(isinstance(n, int) and n > 0 for n in k["by"].values()), k
            for f in k["by"]:
                assert f in rec["runs"] and re.fullmatch(r"tests/test_\w+\.py", f) and os.path.isfile(os.path.join(ROOT, f)), (k["name"], f)
    for f, run in rec["runs"].items():
        assert run["rc"] == 0, "%s ended with status %s when the record was measured" % (f, run["rc"])


def test_unreachable_and_too_large_entries_carry_their_evidence():
    rec = _record()
    by_name = {k["name"]: k for k in rec["kernels"].values()}
    for name in list(reach_scenes.UNREACHABLE) + list(reach_scenes.TOO_LARGE) + list(reach_scenes.WITHHELD):
        assert name in by_name, "%s is no compiled kernel" % name
    for k in rec["kernels"].values():
        if k["status"] == "unreachable":
            assert (k["rule"], k["where"]) == tuple(reach_scenes.UNREACHABLE[k["name"]]) and len(k["rule"]) > 20, k
            path, line = k["where"].rsplit(":", 1)
            with open(os.path.join(ROOT, path)) as f:
                assert 1 <= int(line) <= len(f.readlines()), k["where"]
        if k["status"] == "too_large":
            assert k["seconds"] == reach_scenes.TOO_LARGE[k["name"]] and k["seconds"] > 0, k
        if k["status"] == "withheld":  # a case that hung on the device: left out, with its reason, until the cause is found
            assert k["reason"] == reach_scenes.WITHHELD[k["name"]] and len(k["reason"]) > 20, k


def test_every_reach_case_was_launched_by_the_reach_tests():
    rec = _record()
    by_name = {k["name"]: k for k in rec["kernels"].values()}
    names = [c.kernel for c in reach_scenes.CASES]
    assert len(names) == len(set(names))
    for name in names:
        k = by_name.get(name)
        assert k is not None, "%s is no compiled kernel" % name
        assert k["status"] == "launched" and k["by"].get(lc.REACH_FILE, 0) > 0, "%s: %s" % (name, {x: k.get(x) for x in ("status", "by")})
