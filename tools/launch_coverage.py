"""Which compiled kernels do the GPU tests launch?  A hand-run tool for the GPU machine (not a test): it runs every test file
that holds `gpu`-marked tests under `rocprofv3 --kernel-trace --stats` (kernel trace only: no counters, no other tracing), reads the
kernel names the profiler saw, and writes tests/golden/kernel_launch_coverage.json: for every kernel of the universe either
`launched` (with the test files that launched it and their call counts) or `unreached`; kernels that tests/reach_scenes.py lists as
UNREACHABLE (with the excluding rule and its file:line), TOO_LARGE (with the measured time) or WITHHELD (a case that hung on the device
and is left out until its cause is found, with the reason) get that status when nothing launched them.  tests/test_launch_coverage_record.py keeps the record honest without a device.

Universe: the `Function Name:` remarks of the committed csrc/device/kernels.resource.txt (`make asm`), plus the same remarks of an
offline compile of csrc/device/denoise.hip (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no device needed).

Names are compared MANGLED: rocprofv3 runs with --mangled-kernels, and the resource remarks hold mangled names.  (A trace name that
does not begin with _Z -- a profiler that ignored the flag -- is compared through the normalised demangled form up to the `(`
instead, see short_name().)  The record also stores each kernel's demangled short form, e.g. `pt_kernel<true, 1, 2, 0, false, true>`,
which is how tests/reach_scenes.py names an instantiation.

Every test file runs in one child process of its own, one at a time, under its own `timeout -k 10`; the tool checks every exit status.
A pytest status for failed tests is recorded and the run goes on; a time limit (124, 137), an abort (134), a segmentation fault (139)
or a HIP "illegal memory access" in the output ends the run: nothing more is started, and what was measured so far is written.
There is no retry.  Traces of the processes the tests start themselves (rtamd_render, bench.py) land in the same directory and count.

usage (from the repository root, on a machine with an MI355X):
  python tools/launch_coverage.py                              every file with gpu-marked tests -> the record
  python tools/launch_coverage.py --files tests/a.py tests/b.py --out part1.json     a subset -> a partial record
  python tools/launch_coverage.py --merge part1.json part2.json                      partial records -> the record (no device needed)
  python tools/launch_coverage.py --table                      the summary table of the committed record
  python tools/launch_coverage.py --resource rust-raytracer_amd/csrc/device/ao.resource.txt --files tests/test_ao_gpu.py \
         --out tests/golden/ao_launch_coverage.json            the record of another resource report (the kernels of csrc/device/ao.inc,
                                                               whose rows `make asm` keeps apart): its kernels alone are the universe
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust-raytracer_amd")
RESOURCE = os.path.join(PKG, "csrc", "device", "kernels.resource.txt")
RECORD = os.path.join(ROOT, "tests", "golden", "kernel_launch_coverage.json")
REACH_FILE = "tests/test_kernel_reach_gpu.py"
STOP_CODES = (124, 137, 134, 139)
FAMILIES = ("pt_kernel", "pt_kernel_coop", "pt_kernel_wf", "other")


def resource_names(text):
    """the mangled names of the `Function Name:` remarks, in file order"""
    return re.findall(r"Function Name: (\S+)", text)


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names)
    return out


def short_name(demangled):
    """`void rtamd::pt_kernel<true, 1, 2, 0, false, true>(rtamd::FlatView, ...)` -> `pt_kernel<true, 1, 2, 0, false, true>`"""
    s = demangled.strip()
    depth = 0
    for i, ch in enumerate(s):  # up to the `(` of the parameter list: the first one outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and not s.startswith("(anonymous", i):
            s = s[:i]
            break
    s = re.sub(r"^(void|static)\s+", "", s)
    s = re.sub(r"\s*\[clone [^\]]*\]", "", s)
    return re.sub(r"\s+", " ", s.replace("rtamd::", "").replace("(anonymous namespace)::", "")).strip()


def family(short):
    base = short.split("<")[0]
    return base if base in FAMILIES[:3] else "other"


def denoise_names():
    """mangled kernel names of denoise.hip: an offline compile for gfx950 with the resource remark (the object goes to a temp dir)"""
    tmp = tempfile.mkdtemp(prefix="launch_cov_dn_")
    try:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
               "-I" + os.path.join(PKG, "csrc"), "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(PKG, "csrc", "device", "denoise.hip"), "-o", os.path.join(tmp, "denoise.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("denoise.hip did not compile:\n" + r.stderr[-2000:])
        return resource_names(r.stderr)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def universe(resource=None):
    """{mangled: {"source", "name"}} for kernels.hip (the committed resource report) and denoise.hip (compiled now); resource: the rows
    of that report alone (a part of kernels.hip kept in a file of its own)"""
    with open(resource or RESOURCE) as f:
        k = resource_names(f.read())
    d = [] if resource else denoise_names()
    out = {}
    for src, names in (("kernels.hip", k), ("denoise.hip", d)):
        for m, dm in zip(names, demangle(names) if names else []):
            out[m] = {"source": src, "name": short_name(dm)}
    return out


def gpu_test_files():
    """every tests/test_*.py that holds a gpu mark, sorted"""
    out = []
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        with open(p) as f:
            if re.search(r"pytest\.mark\.gpu\b", f.read()):
                out.append(os.path.relpath(p, ROOT))
    return out


def read_traces(d):
    """{kernel name: calls} over every process that left a trace under d (the stats file of a process, else its trace rows)"""
    calls = {}
    seen = set()
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        seen.add(p[:-len("kernel_stats.csv")])
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        if p[:-len("kernel_trace.csv")] in seen:
            continue
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                calls[row["Kernel_Name"]] = calls.get(row["Kernel_Name"], 0) + 1
    return calls


def match(calls, uni):
    """trace names -> {mangled name of the universe: calls}; names outside the universe (torch's, RCCL's) are dropped"""
    by_short = {v["name"]: m for m, v in uni.items()}
    out = {}
    for name, n in calls.items():
        name = name[:-3] if name.endswith(".kd") else name
        m = name if name in uni else by_short.get(short_name(name)) if not name.startswith("_Z") else None
        if m is not None:
            out[m] = out.get(m, 0) + n
    return out


def tool_version():
    try:
        out = subprocess.run(["rocprofv3", "--version"], capture_output=True, text=True).stdout
        m = re.search(r"^\s*version:\s*(\S+)", out, re.M)
        r = re.search(r"^\s*rocm_version:\s*(\S+)", out, re.M)
        return "%s (rocm %s)" % (m.group(1) if m else "?", r.group(1) if r else "?")
    except OSError:
        return None


def git_head():
    try:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True)
        return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else None
    except OSError:
        return None


def source_sha16():
    sys.path.insert(0, ROOT)
    import bench
    return bench.kernel_source_sha16()


def run_file(rel, uni, limit, logdir, pytest_args):
    """one child: rocprofv3 around pytest -m gpu of one file.  -> (run entry, {mangled: calls}, stop?)"""
    d = tempfile.mkdtemp(prefix="launch_cov_")
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--mangled-kernels", "-d", d, "--output-format", "csv", "--",
           sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-p", "no:cacheprovider"] + pytest_args + [rel]
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace")
    secs = time.time() - t0
    if logdir:
        os.makedirs(logdir, exist_ok=True)
        with open(os.path.join(logdir, os.path.basename(rel) + ".log"), "w") as f:
            f.write(r.stdout)
    rc = r.returncode
    fault = "illegal memory access" in r.stdout
    stop = rc in STOP_CODES or rc < 0 or fault
    launched = match(read_traces(d), uni)
    shutil.rmtree(d, ignore_errors=True)
    tail = [ln for ln in r.stdout.splitlines() if re.search(r"\b(passed|failed|error|no tests ran)\b", ln)][-1:]
    entry = {"rc": rc, "seconds": round(secs, 1), "pytest": tail[0].strip(" =") if tail else None}
    if fault:
        entry["fault"] = "illegal memory access"
    print("%-44s rc %3d %7.1f s  %3d kernels  %s" % (rel, rc, secs, len(launched), entry["pytest"]), flush=True)
    return entry, launched, stop


def annotations():
    """(UNREACHABLE, TOO_LARGE, WITHHELD) of tests/reach_scenes.py, keyed by short name; empty where the module does not exist yet"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import reach_scenes
    except ImportError:
        return {}, {}, {}
    return tuple(dict(getattr(reach_scenes, k, {})) for k in ("UNREACHABLE", "TOO_LARGE", "WITHHELD"))


def finish(rec):
    """statuses from the launch counts and the annotations; kernels in a stable order"""
    unreachable, too_large, withheld = annotations()
    for m, k in rec["kernels"].items():
        by = {f: n for f, n in sorted(k.get("by", {}).items()) if n > 0}
        for key in ("by", "rule", "where", "seconds", "reason", "status"):
            k.pop(key, None)
        if by:
            k["status"], k["by"] = "launched", by
        elif k["name"] in unreachable:
            k["status"] = "unreachable"
            k["rule"], k["where"] = unreachable[k["name"]]
        elif k["name"] in too_large:
            k["status"] = "too_large"
            k["seconds"] = too_large[k["name"]]
        elif k["name"] in withheld:
            k["status"] = "withheld"
            k["reason"] = withheld[k["name"]]
        else:
            k["status"] = "unreached"
    return rec


def table(rec):
    """counts per family: launched (of which only by the reach cases = newly covered), unreachable, too large, withheld, unreached"""
    rows = {f: dict(total=0, launched=0, newly=0, unreachable=0, too_large=0, withheld=0, unreached=0) for f in FAMILIES}
    for k in rec["kernels"].values():
        r = rows[family(k["name"])]
        r["total"] += 1
        r[k["status"]] += 1
        if k["status"] == "launched" and list(k["by"]) == [REACH_FILE]:
            r["newly"] += 1
    lines = ["%-16s %6s %9s %14s %12s %10s %9s %10s" % ("family", "total", "launched", "newly covered", "unreachable", "too large", "withheld", "unreached")]
    for f in FAMILIES:
        r = rows[f]
        lines.append("%-16s %6d %9d %14d %12d %10d %9d %10d" % (f, r["total"], r["launched"], r["newly"], r["unreachable"], r["too_large"], r["withheld"], r["unreached"]))
    return "\n".join(lines)


def dumps(rec):
    """the record as JSON with one line per kernel and per run (sorted): a new measurement shows as the lines that changed"""
    one = lambda v: json.dumps(v, sort_keys=True)
    lines = ["{"]
    for key in sorted(k for k in rec if k not in ("kernels", "runs")):
        lines.append(" %s: %s," % (one(key), one(rec[key])))
    for key in ("runs", "kernels"):
        lines.append(" %s: {" % one(key))
        items = sorted(rec[key].items(), key=(lambda kv: (kv[1]["source"], kv[1]["name"])) if key == "kernels" else None)
        lines += ["  %s: %s%s" % (one(k), one(v), "," if i + 1 < len(items) else "") for i, (k, v) in enumerate(items)]
        lines.append(" }" + ("," if key == "runs" else ""))
    return "\n".join(lines + ["}"]) + "\n"


def write(rec, path, quiet=False):
    finish(rec)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path + ".tmp", "w") as f:
        f.write(dumps(rec))
    os.replace(path + ".tmp", path)
    if not quiet:
        print(table(rec))
        print("wrote", path)


def merge(paths):
    """partial records -> one: launch counts of different files are joined, a file measured twice keeps its LAST measurement"""
    out = None
    for p in paths:
        with open(p) as f:
            rec = json.load(f)
        if out is None:
            out = rec
            continue
        for f_, run in rec["runs"].items():
            out["runs"][f_] = run
            for k in out["kernels"].values():
                k.get("by", {}).pop(f_, None)
        for m, k in rec["kernels"].items():
            o = out["kernels"].setdefault(m, {"source": k["source"], "name": k["name"]})
            for f_, n in k.get("by", {}).items():
                o.setdefault("by", {})[f_] = n
        for key in ("kernel_source_sha16", "rocprofv3", "names"):
            out[key] = rec.get(key) or out.get(key)
        out["head"] = rec.get("head") or out.get("head")
    out["head"] = out.get("head") or git_head()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--files", nargs="+", help="run these test files only (default: every file with gpu-marked tests)")
    ap.add_argument("--merge", nargs="+", metavar="RECORD", help="join partial records instead of running anything")
    ap.add_argument("--table", action="store_true", help="print the summary table of --out and exit")
    ap.add_argument("--out", default=RECORD)
    ap.add_argument("--resource", default=None, help="another resource report whose kernels alone are the universe (the record names it)")
    ap.add_argument("--timeout", type=int, default=600, help="time limit of one child, seconds")
    ap.add_argument("--logs", default=None, help="directory for the children's output, one file each")
    ap.add_argument("--pytest-args", default="", help="further arguments for every pytest child, e.g. '--durations=0'")
    a = ap.parse_args()
    if a.table:
        with open(a.out) as f:
            print(table(finish(json.load(f))))
        return 0
    if a.merge:
        write(merge(a.merge), a.out)
        return 0
    uni = universe(a.resource)
    rec = {"head": git_head(), "kernel_source_sha16": source_sha16(), "rocprofv3": tool_version(), "names": "mangled", "runs": {},
           "kernels": {m: dict(v) for m, v in uni.items()}}
    if a.resource:
        rec["resource"] = os.path.relpath(os.path.abspath(a.resource), ROOT)
    stopped = False
    for rel in (a.files or gpu_test_files()):
        rel = os.path.relpath(os.path.abspath(rel), ROOT)
        entry, launched, stopped = run_file(rel, uni, a.timeout, a.logs, a.pytest_args.split())
        rec["runs"][rel] = entry
        for m, n in launched.items():
            rec["kernels"][m].setdefault("by", {})[rel] = n
        write(rec, a.out, quiet=True)  # (after every file: a run that is cut short leaves what it measured)
        if stopped:
            print("stopping: %s ended with status %d%s; nothing more is started" % (rel, entry["rc"], " and a GPU fault" if "fault" in entry else ""))
            break
    write(rec, a.out)
    return 3 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
