"""What a caller sees of every render entry point when it is called wrongly: tests/golden/render_entry_table.json holds, for each entry
point, every defect that applies to it, every pair of defects at once and one valid call, the status code, rt_last_error() and what
became of a prefilled rt_stats -- recorded from the commit named in the file by tests/golden/make_render_entry_table.py, which also builds
and makes the calls here.  The order of an entry point's checks decides which of two errors a caller gets; this replays it row by row.
Runs where tests/test_multi_stub.py runs, inside tests/asan/run_host_asan.sh, once without a device and once on the stub's four fake
devices: against the real librtamd.so an entry point without a device check of its own would answer with a HIP message, not the stub's."""
import json
import os
import re
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)

pytestmark = pytest.mark.skipif("asan" not in os.path.basename(os.environ.get("RTAMD_LIB", "")),
                                reason="needs the sanitizer build and its device stub (run_host_asan.sh)")


def _table():
    return json.load(open(os.path.join(GOLDEN, "render_entry_table.json")))


def test_the_table_lists_every_render_entry_point_of_the_header():
    table = _table()
    header = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    declared = set(re.findall(r"\b(rt_(?:render|accum)\w*)\s*\(", header))
    assert declared and declared <= set(table["entries"]), sorted(declared - set(table["entries"]))
    import make_render_entry_table as gen
    assert list(gen.ENTRIES) == table["entries"] and gen.DEFECT_NAMES == table["defects"]
    assert os.path.getsize(os.path.join(GOLDEN, "render_entry_table.json")) < os.path.getsize(os.path.join(GOLDEN, "scenes", "bun315.obj"))


def test_every_call_of_the_table_answers_as_recorded():
    import make_render_entry_table as gen
    mode = int(os.environ.get("RTAMD_STUB_DEVICES") or 0)
    assert mode in gen.MODES
    want = [r for r in gen.decode(_table()) if r[3] == mode]
    got = gen.record(mode)
    assert len(want) > 1000 and [r[:3] for r in got] == [r[:3] for r in want]    # the same cases, in the same order
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, "%d of %d calls differ; (now, recorded): %r" % (len(diff), len(want), diff[:5])
