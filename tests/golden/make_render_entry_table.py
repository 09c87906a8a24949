"""Record tests/golden/render_entry_table.json: what a caller can observe of every render entry point when it is called wrongly -- the
status code, rt_last_error() and what became of an rt_stats prefilled with 0xAB bytes -- for every defect that applies to the entry point,
every PAIR of defects at once (the pair decides which check comes first) and one valid call.  Run on the sanitizer build
(tests/asan/run_host_asan.sh builds it) of the commit whose behaviour is to be pinned, in both of the stub's modes (no device; four fake
devices -- the stub reads RTAMD_STUB_DEVICES at every call, so one process records both):
    LD_PRELOAD="$(gcc -print-file-name=libasan.so) $(gcc -print-file-name=libubsan.so)" ASAN_OPTIONS=detect_leaks=0 RTAMD_HIP_RUNTIME=system \\
    RTAMD_LIB=$PWD/tests/asan/librtamd_host_asan.so python tests/golden/make_render_entry_table.py --commit COMMIT
tests/test_render_entry_errors.py imports this module and replays the table.

The file: "entries", "defects", "messages", "states" are name lists; a row is [entry, defect, defect, mode, code, message, stats state], all
but mode (the value of RTAMD_STUB_DEVICES, 0 = unset) and code indices into those lists, -1 for "no defect".  The message of a call that
set none is the sentinel this module plants before every call.  Stats states, one letter per rt_stats entry the call was given: A left
alone, Z zeroed, W written; "-" where the entry point has no rt_stats or it was passed as NULL.
The ABI exports no device allocator, so the *_device entry points get host pointers: the stub's render answers "rows are not device memory",
and that answer is what the table holds for their valid call."""
import argparse
import ctypes as C
import itertools
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TABLE = os.path.join(ROOT, "tests", "golden", "render_entry_table.json")
sys.path.insert(0, os.path.join(ROOT, "rust-raytracer_amd"))
import numpy as np  # noqa: E402
import rtamd  # noqa: E402

MODES = (0, 4)
W, H, SPP = 52, 28, 16                      # partial tiles on both edges; 7 x 4 tiles
TILE_DOUBLES = 7 * 4 * 64 * 3
SENTINEL = "null path"                      # rt_write_png(NULL, ...): a message no render entry point has
_dp = C.POINTER(C.c_double)

# entry point -> its arguments in order.  Kinds: s scene, cam, frame, p params, host buffers (out_rgb, out_aov, accum_state, tile_spp, stats_out,
# photons), "device" pointers that are host memory here (d_*), stream (always NULL), stats / mstats (one / four rt_stats), values.
ENTRIES = {
    "rt_render": ["s", "cam", "p", "out_rgb", "stats"],
    "rt_render_camera_frame": ["s", "frame", "p", "out_rgb", "stats"],
    "rt_render_tiles_device": ["s", "cam", "p", "d_tiles", "stream", "stats"],
    "rt_render_accumulate_device": ["s", "cam", "p", "begin", "end", "d_accum", "stream", "stats"],
    "rt_render_accumulate": ["s", "cam", "p", "begin", "end", "accum_state", "stats"],
    "rt_accum_finalize": ["p", "accum_state", "out_rgb"],
    "rt_accum_finalize_device": ["p", "d_accum", "d_tiles", "stream"],
    "rt_render_adaptive": ["s", "cam", "p", "acfg", "out_rgb", "tile_spp", "stats"],
    "rt_render_sppm": ["s", "cam", "p", "scfg", "out_rgb", "stats_out", "photons", "stats"],
    "rt_render_sppm_tiles_device": ["s", "cam", "p", "scfg", "d_tiles", "stream", "stats"],
    "rt_render_aov": ["s", "cam", "p", "aov_spp", "out_aov", "stats"],
    "rt_render_multi": ["s", "cam", "p", "n_devices", "device_ids", "out_rgb", "mstats"],
    "rt_render_multi_camera_frame": ["s", "frame", "p", "n_devices", "device_ids", "out_rgb", "mstats"],
    "rt_render_sppm_multi": ["s", "cam", "p", "scfg", "n_devices", "device_ids", "out_rgb", "mstats"],
    "rt_assemble_frame_device": ["p", "d_gathered", "stride", "d_frame", "stream"],
    "rt_tiles_total": ["p"],
    "rt_tiles_owned": ["p"],
    "rt_accum_state_doubles": ["p"],
}
WHOLE_FRAME = {"rt_accum_finalize", "rt_render_adaptive", "rt_render_sppm", "rt_render_aov", "rt_render_multi", "rt_render_multi_camera_frame",
               "rt_render_sppm_multi"}
POINTERS = ["s", "cam", "frame", "p", "out_rgb", "out_aov", "accum_state", "tile_spp", "stats_out", "photons", "d_tiles", "d_accum", "d_gathered",
            "d_frame", "acfg", "scfg", "device_ids", "stats", "mstats"]


def _set(field, value):
    def f(a):
        setattr(a["p"], field, value)
    return f


def _rank_is_world(a):
    a["p"].rank = a["p"].world


def _nan_frame(a):
    a["frame"].u[1] = math.nan


def _range(b, e):
    def f(a):
        a["begin"], a["end"] = b, e
    return f


def _odd_min_spp(a):
    a["acfg"].min_spp = 5


def _nan_threshold(a):
    a["acfg"].threshold = math.nan


def _n_devices_m2(a):
    a["n_devices"] = -2


def _bad_ordinal(a):
    a["device_ids"] = (C.c_int * 2)(0, 7)


# name -> (the argument it needs, the slot it changes, what it does).  Two defects whose slots are equal, or one inside the other
# ("p" and "p.width": a field of a struct that is not there), do not pair.
DEFECTS = {
    "uncommitted": ("s", "s.committed", None),
    "width=0": ("p", "p.width", _set("width", 0)),
    "spp=0": ("p", "p.spp", _set("spp", 0)),
    "max_depth=-1": ("p", "p.max_depth", _set("max_depth", -1)),
    "rank=world": ("p", "p.rank", _rank_is_world),
    "world=2": ("p", "p.world", _set("world", 2)),
    "kernel=3": ("p", "p.kernel", _set("kernel", 3)),
    "integrator=3": ("p", "p.integrator", _set("integrator", 3)),
    "time1<time0": ("p", "p.time", lambda a: (_set("time0", 1.0)(a), _set("time1", 0.0)(a))),
    "device=7": ("p", "p.device", _set("device", 7)),
    "nan frame": ("frame", "frame.u", _nan_frame),
    "range 3,3": ("begin", "range", _range(3, 3)),
    "range -1,4": ("begin", "range", _range(-1, 4)),
    "range 0,17": ("begin", "range", _range(0, 17)),
    "min_spp=5": ("acfg", "acfg.min_spp", _odd_min_spp),
    "threshold=nan": ("acfg", "acfg.threshold", _nan_threshold),
    "n_devices=-2": ("n_devices", "n_devices", _n_devices_m2),
    "device_ids=0,7": ("device_ids", "device_ids.0", _bad_ordinal),
}
DEFECT_NAMES = ["null " + k for k in POINTERS] + list(DEFECTS)
# a defect that crashes the recorded commit (a pointer it dereferences unchecked) is left out here, by (entry, defect): none was found
CRASHES = set()


def defects_of(entry):
    kinds = ENTRIES[entry]
    out = ["null " + k for k in POINTERS if k in kinds]
    for name, (needs, _, _) in DEFECTS.items():
        if needs in kinds and (name != "world=2" or entry in WHOLE_FRAME):
            out.append(name)
    return [d for d in out if (entry, d) not in CRASHES]


def _slot(d):
    return d[5:] if d.startswith("null ") else DEFECTS[d][1]


def cases_of(entry):
    """(), every defect, every pair of defects that can be present at once; in a fixed order"""
    ds = defects_of(entry)
    out = [()] + [(d,) for d in ds]
    for a, b in itertools.combinations(ds, 2):
        sa, sb = _slot(a).split("."), _slot(b).split(".")
        n = min(len(sa), len(sb))
        if sa[:n] != sb[:n]:
            out.append((a, b))
    return out


def header_functions():
    text = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    return set(re.findall(r"^\w[\w\s\*]*?\b(rt_\w+)\s*\(", text, re.M))


class Scenes:
    def __init__(self):
        path = os.path.join(ROOT, "tests", "golden", "scenes", "scene_10.json")
        self.committed, self.cam = rtamd.load_scene_file(path)
        self.uncommitted, _ = rtamd.load_scene_file(path, commit=False)


def _fresh_args(sc):
    L = rtamd.lib()
    a = {"s": sc.committed.h, "cam": rtamd.rt_camera.from_buffer_copy(sc.cam.c), "frame": sc.cam.frame(),
         "p": rtamd.default_params(width=W, height=H, spp=SPP, max_depth=5, seed=3),
         "out_rgb": np.zeros(W * H * 3), "out_aov": np.zeros(W * H * 8), "accum_state": np.zeros(TILE_DOUBLES),
         "tile_spp": np.zeros(7 * 4, dtype=np.int32), "stats_out": np.zeros(W * H * 10), "photons": (C.c_uint64 * 2)(),
         "d_tiles": np.zeros(TILE_DOUBLES), "d_accum": np.zeros(TILE_DOUBLES), "d_gathered": np.zeros(4 * TILE_DOUBLES), "d_frame": np.zeros(W * H * 3),
         "stride": 7 * 4, "stream": None, "begin": 0, "end": SPP, "aov_spp": 2, "n_devices": 2, "device_ids": (C.c_int * 2)(1, 0),
         "acfg": rtamd.rt_adaptive_config(), "scfg": rtamd.rt_sppm_config(),
         "stats": (rtamd.rt_stats * 1)(), "mstats": (rtamd.rt_stats * 4)()}
    L.rt_default_adaptive_config(C.byref(a["acfg"]))
    a["acfg"].min_spp = 4
    L.rt_default_sppm_config(C.byref(a["scfg"]))
    a["scfg"].iterations, a["scfg"].photons_per_iter = 1, 10
    for k in ("stats", "mstats"):
        C.memset(a[k], 0xAB, C.sizeof(a[k]))
    return a


def _ctypes_arg(kind, v, argtype):
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        return v.ctypes.data if argtype is C.c_void_p else v.ctypes.data_as(argtype)
    if isinstance(v, C.Structure):
        return C.byref(v)
    return v


def _stats_state(buf):
    raw = bytes(buf)
    n = C.sizeof(rtamd.rt_stats)
    return "".join("A" if e == b"\xab" * n else "Z" if e == bytes(n) else "W" for e in (raw[i:i + n] for i in range(0, len(raw), n)))


def call(sc, entry, defects):
    """-> (code, message, stats state) of `entry` called with `defects` present"""
    L = rtamd.lib()
    a = _fresh_args(sc)
    for d in defects:
        if d == "uncommitted":
            a["s"] = sc.uncommitted.h
        elif not d.startswith("null "):
            DEFECTS[d][2](a)
    for d in defects:
        if d.startswith("null "):
            a[d[5:]] = None
    fn = getattr(L, entry)
    args = [_ctypes_arg(k, a[k], t) for k, t in zip(ENTRIES[entry], fn.argtypes)]
    L.rt_write_png(None, 0, 0, None)
    code = int(fn(*args))
    msg = L.rt_last_error().decode("utf-8", "replace")
    which = [k for k in ENTRIES[entry] if k in ("stats", "mstats")]
    state = _stats_state(a[which[0]]) if which and a[which[0]] is not None else "-"
    return code, msg, state


def record(mode, sc=None):
    """every case of every entry point in stub mode `mode` -> [(entry, defect or None, defect or None, mode, code, message, state)]"""
    if mode:
        os.environ["RTAMD_STUB_DEVICES"] = str(mode)
    else:
        os.environ.pop("RTAMD_STUB_DEVICES", None)
    sc = sc or Scenes()
    rows = []
    for entry in ENTRIES:
        for ds in cases_of(entry):
            code, msg, state = call(sc, entry, ds)
            rows.append((entry, ds[0] if ds else None, ds[1] if len(ds) > 1 else None, mode, code, msg, state))
    return rows


def encode(rows, commit):
    entries, messages, states = list(ENTRIES), [], []

    def idx(lst, v):
        if v not in lst:
            lst.append(v)
        return lst.index(v)

    def d(v):
        return -1 if v is None else DEFECT_NAMES.index(v)
    out = [[entries.index(e), d(a), d(b), mode, code, idx(messages, msg), idx(states, st)] for e, a, b, mode, code, msg, st in rows]
    head = {"recorded_on": commit, "what": "see tests/golden/make_render_entry_table.py", "sentinel": SENTINEL, "entries": entries,
            "defects": DEFECT_NAMES, "messages": messages, "states": states}
    text = json.dumps(head, indent=1)[:-2] + ',\n "rows": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in out) + "\n ]\n}\n"
    return text


def decode(table):
    name = lambda i: None if i < 0 else table["defects"][i]  # noqa: E731
    return [(table["entries"][e], name(a), name(b), mode, code, table["messages"][m], table["states"][s]) for e, a, b, mode, code, m, s in table["rows"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="", help="the commit the loaded library was built from (recorded in the file)")
    ap.add_argument("--out", default=TABLE)
    a = ap.parse_args()
    missing = sorted(set(ENTRIES) - header_functions())
    if missing:
        sys.exit("include/rtamd.h does not declare: " + ", ".join(missing))
    if "asan" not in os.path.basename(rtamd.LIB_PATH):
        sys.exit("record on the sanitizer build (RTAMD_LIB=tests/asan/librtamd_host_asan.so), not on " + rtamd.LIB_PATH)
    sc = Scenes()
    rows = [r for mode in MODES for r in record(mode, sc)]
    with open(a.out, "w") as f:
        f.write(encode(rows, a.commit))
    print("%d rows, %d bytes -> %s" % (len(rows), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()
