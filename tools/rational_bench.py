"""Cost of the rational (NURBS) trial and test functions in the element kernels (developer tool / profile source).

The rational volume of ``tests/geom_util.rational_volume``, p = 2 and 3, at 32^3, 48^3 and 64^3 elements.  Mass matrix,
stiffness matrix and nodal load are assembled in three ways, alternating in one process after a warm-up round:

  rational       ``rational=True``: the sum-factorised instantiations for psi = phi / W_h,
  plain_forms    the un-rationalised forms on the existing kernels -- the yardstick,
  rational_slow  ``rational=True`` through the plain O((p+1)^9) element kernel (TIGAR_ASM_LEGACY=1), at 32^3 only.

Two times per call: ``kernel_ms``, what the library's own events around the element kernels give (TIGAR_ASM_TIME=1, read
from the line on stderr, which also says which path ran), and ``wall_ms`` of the whole call (pattern, allocation and a
device synchronise included).  ``tg_quad_error`` is timed with and without the flag on the same patches (wall).  Medians
of the repeats with the spread max - min.

    python tools/rational_bench.py [--sizes 32,48,64] [--degrees 2,3] [--reps 5] [--out profiles/rational_bench.jsonl]
                                   [--resources NEW.txt --parent-resources PARENT.txt]

``--resources``: the output of ``hipcc -Rpass-analysis=kernel-resource-usage`` for csrc/tg_assemble.hip and csrc/tg_postproc.hip
(both files' remarks in one text file) of this tree and of the parent commit.  The first JSON line then lists registers,
LDS and scratch of the instantiations that are new and says whether every other kernel has the parent's figures.
"""
import argparse
import gc
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tigar_amd as t  # noqa: E402
from tigar_amd import NURBS as N, device as dev  # noqa: E402
from tigar_amd import common as tc  # noqa: E402
from geom_util import rational_volume  # noqa: E402

FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def parse_resources(path):
    """{kernel: {field: value}} from the remarks of -Rpass-analysis=kernel-resource-usage"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(?:[^:\s]+:\d+:\d+:\s+)?([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, r))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def resource_record(new_path, parent_path):
    new, old = parse_resources(new_path), parse_resources(parent_path)
    names = demangle(sorted(new))
    cmp_fields = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")
    added = {names[k]: {f: v.get(f) for f in FIELDS} for k, v in new.items() if k not in old}
    changed = {names[k]: {"parent": {f: old[k].get(f) for f in FIELDS}, "now": {f: v.get(f) for f in FIELDS}}
               for k, v in new.items() if k in old and any(v.get(f) != old[k].get(f) for f in cmp_fields)}
    return {"record": "kernel resources", "new_instantiations": added,
            "existing_kernels": len([k for k in new if k in old]), "existing_kernels_with_other_figures": changed,
            "kernels_gone": sorted(k for k in old if k not in new)}


class capture_stderr(object):
    """the library's fprintf(stderr, ...) of a block, read back as text"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def timed_assembly(fn):
    """(kernel ms from the library's line, wall ms, the path the line names)"""
    dev.sync()
    with capture_stderr() as cap:
        t0 = time.perf_counter()
        out = fn()
        dev.sync()
        wall = (time.perf_counter() - t0) * 1e3
    del out
    m = re.search(r"element kernels ([0-9.]+) ms \(([a-z-]+)\)", cap.text)
    return float(m.group(1)), wall, m.group(2)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "spread_ms": round(float(max(ts) - min(ts)), 4), "all_ms": [round(v, 4) for v in ts]}


def run(p, nel, reps, slow):
    kvs, C = rational_volume(p, (nel,) * 3)
    gen = t.EqualOrderSpline(tc.selfcomm, 1, N.NURBSControlMesh([p] * 3, kvs, C))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k]) for k in range(3)]
    dcp = [f.vector() for f in gen.cpFuncs]
    n = dcp[0].size()
    rng = np.random.default_rng(p * 100 + nel)
    fn = dev.DeviceVector(data=rng.standard_normal(n))
    calls = {"mass": lambda r: dev.assemble_mapped_matrix(uks, p, dcp, "mass", rational=r),
             "laplace": lambda r: dev.assemble_mapped_matrix(uks, p, dcp, "laplace", rational=r),
             "load": lambda r: dev.assemble_mapped_load(uks, p, dcp, fn, rational=r)}
    variants = [("rational", True, False), ("plain_forms", False, False)] + ([("rational_slow", True, True)] if slow else [])
    rec = {"record": "assembly", "p": p, "nel": nel, "fe_nodes": n, "reps": reps}
    os.environ["TIGAR_ASM_TIME"] = "1"
    for form, call in calls.items():
        ker = {v[0]: [] for v in variants}
        wall = {v[0]: [] for v in variants}
        path = {}
        for rep in range(reps + 1):                          # (round 0 warms up)
            for name, rat, legacy in variants:
                if legacy:
                    os.environ["TIGAR_ASM_LEGACY"] = "1"
                k_ms, w_ms, which = timed_assembly(lambda: call(rat))
                os.environ.pop("TIGAR_ASM_LEGACY", None)
                gc.collect()
                path[name] = which
                if rep:
                    ker[name].append(k_ms)
                    wall[name].append(w_ms)
        out = {name: {"path": path[name], "kernel": stats(ker[name]), "wall": stats(wall[name])} for name, _, _ in variants}
        out["kernel_ratio_rational_to_plain_forms"] = round(out["rational"]["kernel"]["median_ms"] / out["plain_forms"]["kernel"]["median_ms"], 4)
        if slow:
            out["kernel_ratio_slow_to_rational"] = round(out["rational_slow"]["kernel"]["median_ms"] / out["rational"]["kernel"]["median_ms"], 2)
        rec[form] = out
    os.environ.pop("TIGAR_ASM_TIME", None)
    # the error sums with and without the flag
    npts = dev.quad_count(uks, p + 1)
    e = dev.DeviceVector(data=rng.standard_normal(npts))
    ge = dev.DeviceVector(data=rng.standard_normal(3 * npts))
    te = {False: [], True: []}
    for rep in range(reps + 1):
        for rat in (True, False):
            dev.sync()
            t0 = time.perf_counter()
            dev.quad_error(uks, p, dcp, fn, e, ge, rational=rat)
            dev.sync()
            if rep:
                te[rat].append((time.perf_counter() - t0) * 1e3)
    rec["quad_error"] = {"points": npts, "rational": stats(te[True]), "plain": stats(te[False]),
                         "ratio": round(float(np.median(te[True]) / np.median(te[False])), 4)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,48,64")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-at", type=int, default=32, help="the size the plain kernel is timed at")
    ap.add_argument("--resources", default=None)
    ap.add_argument("--parent-resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rational_bench.jsonl"))
    args = ap.parse_args()
    info = dev.device_info()
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.resources and args.parent_resources:
            emit(resource_record(args.resources, args.parent_resources))
        for p in [int(v) for v in args.degrees.split(",")]:
            for nel in [int(v) for v in args.sizes.split(",")]:
                rec = run(p, nel, args.reps, nel == args.slow_at)
                rec["device"] = info["name"]
                emit(rec)


if __name__ == "__main__":
    main()
