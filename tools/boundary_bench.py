"""Cost of the boundary kernels (csrc/tg_boundary.hip) next to the volume kernels they were modelled on (developer tool /
profile source).

The face (2, 1) of the rational volume of ``tests/geom_util.rational_volume`` with 32^2, 48^2 and 64^2 face elements (one
layer of elements behind it), p = 2 and 3, nq = p + 1.  Every ending -- points, eval (with gradient and d_n), load (f_q and
fn_q), matrix (three coefficient arrays), matrix_add into the mapped Laplace matrix -- is timed next to ``tg_quad_eval``
and ``tg_quad_load`` on a volume with (nearly) the same number of points, alternating in one process after a warm-up round;
those two are existing code and serve as the yardstick.  Times are wall times of whole calls ending in a device
synchronise: at these sizes a call is a few launches (one per colour for load and matrix) of a few microseconds of device
work each, so the figures are launch and allocation overheads, not bandwidth.  Medians of the repeats, spread = max - min.

    python tools/boundary_bench.py [--sizes 32,48,64] [--degrees 2,3] [--reps 5] [--out profiles/boundary_bench.jsonl]
                                   [--resources NEW.txt --parent-resources PARENT.txt]

``--resources``: the remarks of ``hipcc -Rpass-analysis=kernel-resource-usage`` for csrc/tg_boundary.hip, csrc/tg_postproc.hip
and csrc/tg_assemble.hip of this tree, ``--parent-resources`` those of the last two files of the parent commit.  The first
JSON line then lists registers, LDS, occupancy and scratch of every new instantiation and says whether the existing
kernels kept the parent's figures.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tigar_amd as t  # noqa: E402
from tigar_amd import NURBS as N, device as dev  # noqa: E402
from tigar_amd import common as tc  # noqa: E402
from geom_util import rational_volume  # noqa: E402
from rational_bench import resource_record, stats  # noqa: E402


def patch(p, nels):
    kvs, C = rational_volume(p, nels)
    gen = t.EqualOrderSpline(tc.selfcomm, 1, N.NURBSControlMesh([p] * 3, kvs, C))
    g = gen.V.grids[0]
    return [np.asarray(g.vertices[k]) for k in range(3)], [f.vector() for f in gen.cpFuncs]


def run(p, nel, reps):
    nq = p + 1
    rng = np.random.default_rng(p * 100 + nel)
    uks, dcp = patch(p, (nel, nel, 1))
    n = dcp[0].size()
    npts = dev.face_count(uks, 2, nq)
    u = dev.DeviceVector(data=rng.standard_normal(n))
    a, b, c = (dev.DeviceVector(data=rng.standard_normal(npts)) for _ in range(3))
    out = dev.DeviceVector(n)
    lap = dev.assemble_mapped_matrix(uks, p, dcp, "laplace")
    # the yardstick: a volume with (nearly) as many points
    vuks, vdcp = patch(p, (nel, -(-nel // nq), 1))
    vn, vpts = vdcp[0].size(), dev.quad_count(vuks, nq)
    vu = dev.DeviceVector(data=rng.standard_normal(vn))
    vf = dev.DeviceVector(data=rng.standard_normal(vpts))
    calls = {
        "face_points": lambda: dev.face_points(uks, p, dcp, 2, 1, nq),
        "face_eval": lambda: dev.face_eval(uks, p, dcp, 2, 1, u, True, True, nq),
        "face_eval_rational": lambda: dev.face_eval(uks, p, dcp, 2, 1, u, True, True, nq, True),
        "face_load": lambda: dev.face_load(uks, p, dcp, 2, 1, a, b, out, nq),
        "face_load_rational": lambda: dev.face_load(uks, p, dcp, 2, 1, a, b, out, nq, True),
        "face_matrix": lambda: dev.face_matrix(uks, p, dcp, 2, 1, a, b, c, nq),
        "face_matrix_rational": lambda: dev.face_matrix(uks, p, dcp, 2, 1, a, b, c, nq, True),
        "face_matrix_add": lambda: dev.face_matrix_add(lap, uks, p, dcp, 2, 1, a, b, c, 1.0, nq),
        "quad_eval": lambda: dev.quad_eval(vuks, p, vdcp, vu, grad=True, nq=nq),
        "quad_load": lambda: dev.quad_load(vuks, p, vdcp, vf, nq=nq),
    }
    ts = {k: [] for k in calls}
    for rep in range(reps + 1):                              # (round 0 warms up)
        for name, call in calls.items():
            dev.sync()
            t0 = time.perf_counter()
            r = call()
            dev.sync()
            if rep:
                ts[name].append((time.perf_counter() - t0) * 1e3)
            del r
    rec = {"record": "boundary", "p": p, "nq": nq, "face_elements": nel * nel, "face_points": npts, "fe_nodes": n,
           "volume_elements": nel * -(-nel // nq), "volume_points": vpts, "reps": reps,
           "launches": {"face_points": 1, "face_eval": 1, "face_load": 4, "face_matrix": "1 pattern + 4", "face_matrix_add": "1 check + 4",
                        "quad_eval": 1, "quad_load": "4 (the non-empty colours of 8)"}}
    for name in calls:
        rec[name] = stats(ts[name])
    rec["ratio_face_eval_to_quad_eval"] = round(rec["face_eval"]["median_ms"] / rec["quad_eval"]["median_ms"], 3)
    rec["ratio_face_load_to_quad_load"] = round(rec["face_load"]["median_ms"] / rec["quad_load"]["median_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,48,64")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--parent-resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_bench.jsonl"))
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
                rec = run(p, nel, args.reps)
                rec["device"] = info["name"]
                emit(rec)


if __name__ == "__main__":
    main()
