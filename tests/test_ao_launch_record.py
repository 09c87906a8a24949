"""The kernels of csrc/device/ao.inc and which GPU tests launch them, held to the tree without a device.  Their
resource rows live in csrc/device/ao.resource.txt and their launch record in tests/golden/ao_launch_coverage.json, beside
kernels.resource.txt and kernel_launch_coverage.json, which hold every other kernel of kernels.hip and stay as they were: the two
reports share no kernel, every instantiation the host code can launch has a row, and every row was launched by tests/test_ao_gpu.py.

Regenerating (on a machine with an MI355X, from the repository root, on a built tree): `make asm` writes the rows of ao.inc's kernels
into ao.resource.txt and every other row into kernels.resource.txt; then
    python tools/launch_coverage.py --resource rust-raytracer_amd/csrc/device/ao.resource.txt --files tests/test_ao_gpu.py --out part.json
    python tools/launch_coverage.py --merge part.json --out tests/golden/ao_launch_coverage.json"""
import json
import os
import re
import sys

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import launch_coverage as lc  # noqa: E402

AO_RESOURCE = os.path.join(lc.PKG, "csrc", "device", "ao.resource.txt")
EXPECTED = sorted("%s<%s, %d>" % (k, a, g) for k in ("ao_kernel", "occluded_kernel") for a in ("false", "true") for g in (1, 3))


def _record():
    with open(os.path.join(GOLDEN, "ao_launch_coverage.json")) as f:
        return json.load(f)


def _rows():
    with open(AO_RESOURCE) as f:
        return f.read()


def test_the_record_holds_the_rows_of_the_ao_report_and_no_other_kernel():
    rec = _record()
    names = lc.resource_names(_rows())
    assert len(names) == len(set(names)) == 8 and set(names) == set(rec["kernels"])
    assert os.path.join(ROOT, rec["resource"]) == AO_RESOURCE and rec["names"] == "mangled" and rec["rocprofv3"] and rec["head"]
    assert {k["source"] for k in rec["kernels"].values()} == {"kernels.hip"}
    assert sorted(k["name"] for k in rec["kernels"].values()) == EXPECTED
    assert [lc.short_name(d) for d in lc.demangle(sorted(rec["kernels"]))] == [rec["kernels"][m]["name"] for m in sorted(rec["kernels"])]
    with open(lc.RESOURCE) as f:
        assert not set(names) & set(lc.resource_names(f.read()))      # the two reports share no kernel
    assert all(re.search(r"csrc/device/ao\.inc:\d+:", line) for line in _rows().splitlines())


def test_every_row_has_all_its_fields():
    blocks = re.split(r"(?=remark: \S+ Function Name:)", _rows())
    blocks = [b for b in blocks if b.strip()]
    assert len(blocks) == 8
    for b in blocks:
        for field in ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
                      "LDS Size [bytes/block]"):
            assert re.search(re.escape(field) + r": \d+ ", b), (field, b[:120])
        assert "LDS Size [bytes/block]: 0 " in b          # the walk stacks are dynamic LDS, sized by the launch


def test_every_kernel_was_launched_by_the_ao_gpu_tests():
    rec = _record()
    assert list(rec["runs"]) == ["tests/test_ao_gpu.py"] and rec["runs"]["tests/test_ao_gpu.py"]["rc"] == 0
    assert os.path.isfile(os.path.join(ROOT, "tests", "test_ao_gpu.py"))
    for m, k in rec["kernels"].items():
        assert k["status"] == "launched" and k["by"].get("tests/test_ao_gpu.py", 0) > 0, (m, k)


def test_the_host_code_launches_no_other_instantiation():
    """ao.inc picks its kernels through kernels.hip's WALK_PASS_KERNEL(K, accel, nest): the macro's instantiations of the two kernels it is
    given, and whatever the file spells out beside them, are the eight of the report"""
    with open(os.path.join(lc.PKG, "csrc", "device", "kernels.hip")) as f:
        macro = re.search(r"^#define WALK_PASS_KERNEL\(K, accel, nest\) (.*)$", f.read(), re.M).group(1)
    with open(os.path.join(lc.PKG, "csrc", "device", "ao.inc")) as f:
        src = f.read()
    picks = re.findall(r"\bWALK_PASS_KERNEL\((\w+),", src)
    assert sorted(picks) == ["ao_kernel", "occluded_kernel"]
    src += "".join("\n" + re.sub(r"\bK<", k + "<", macro) for k in picks)
    used = sorted(set(re.sub(r"\s+", " ", m) for m in re.findall(r"\b((?:ao|occluded)_kernel<(?:true|false), [13]>)", src)))
    assert used == EXPECTED
