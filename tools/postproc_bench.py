"""The quadrature-point kernels (csrc/tg_postproc.hip) beside the nodal load of csrc/tg_assemble.hip (developer tool /
profile source).

3-D p = 3 smooth non-affine rational volume (the map of tests/test_gpu_assembly.py::test_surface_and_volume_maps_match_oracle)
at 32^3, 48^3 and 64^3 elements, nq = p + 1.  In one process, warmed up, the four calls alternating, every sample = ``--inner``
calls ended by one device synchronise:

  tg_quad_error            L2 + H10 terms: u nodal, e and grad e at the points
  tg_quad_eval             values and Cartesian gradient
  tg_quad_load             load vector from point values
  tg_assemble_mapped_load  the closest kernel of the parent commit: same patch, same output when f_q = f_h(x_q)

    python tools/postproc_bench.py [--sizes 32,48,64] [--reps 5] [--inner 10] [--out profiles/postproc_bench.jsonl]

The samples are wall-clock times around the Python wrappers: they include the allocation of the outputs (caching
allocator) and, for tg_quad_error, a device allocation of the partial sums and the read-back of the three sums.  One JSON
line per size is written (the file is replaced): ms per call (median of the repeats, spread = max - min), the byte floor of each call
(the nodal vectors it reads, plus the point arrays it reads or writes, plus the nodal vector it writes), the bytes/s on that
floor, and the difference between tg_quad_load(tg_quad_eval(f)) and tg_assemble_mapped_load(f).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tigar_amd import device as dev  # noqa: E402


def timed(fn, inner):
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) * 1e3 / inner


def run(nel, reps, inner, seed=0):
    p, d = 3, 3
    uks = [np.linspace(0.0, 1.0, nel + 1)] * d
    ax = np.linspace(0.0, 1.0, nel * p + 1)
    X = [g.ravel(order="F") for g in np.meshgrid(ax, ax, ax, indexing="ij")]
    wgt = 1.0 + 0.2 * X[0] * X[1]
    cp = [dev.DeviceVector(data=c) for c in ((X[0] + 0.1 * X[1] * X[2]) * wgt, (X[1] + 0.2 * X[0] ** 2) * wgt,
                                             (X[2] * (1.0 + 0.3 * X[0])) * wgt, wgt)]
    nnodes = X[0].size
    npts = dev.quad_count(uks, p + 1)
    rng = np.random.default_rng(seed)
    u = dev.DeviceVector(data=np.sin(3.0 * X[0]) + X[1] * X[2])
    e = dev.DeviceVector(data=rng.standard_normal(npts))
    ge = dev.DeviceVector(data=rng.standard_normal(3 * npts))
    del X
    calls = {
        "tg_quad_error": (lambda: dev.quad_error(uks, p, cp, u, e, ge), 8 * (5 * nnodes + 4 * npts)),
        "tg_quad_eval": (lambda: dev.quad_eval(uks, p, cp, u, grad=True), 8 * (5 * nnodes + 4 * npts)),
        "tg_quad_load": (lambda: dev.quad_load(uks, p, cp, e), 8 * (4 * nnodes + npts + nnodes)),
        "tg_assemble_mapped_load": (lambda: dev.assemble_mapped_load(uks, p, cp, u), 8 * (5 * nnodes + nnodes)),
    }
    for fn, _ in calls.values():                                   # (warm-up)
        fn()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, (fn, _) in calls.items():
            ts[k].append(timed(fn, inner))
    rec = {"nel": nel, "p": p, "nq": p + 1, "fe_nodes": nnodes, "points": npts, "reps": reps, "inner": inner}
    for k, (_, floor) in calls.items():
        med = float(np.median(ts[k]))
        rec[k] = {"median_ms": med, "spread_ms": float(max(ts[k]) - min(ts[k])), "all_ms": [round(v, 4) for v in ts[k]],
                  "byte_floor": floor, "bytes_per_s_on_floor": floor / (med * 1e-3)}
    a = dev.quad_load(uks, p, cp, dev.quad_eval(uks, p, cp, u)).get_local()
    b = dev.assemble_mapped_load(uks, p, cp, u).get_local()
    rec["load_of_evaluated_interpolant_vs_nodal_load"] = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,48,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "postproc_bench.jsonl"))
    args = ap.parse_args()
    info = dev.device_info()
    with open(args.out, "w") as f:                                  # (one run = the file: no lines of earlier runs)
        for nel in [int(v) for v in args.sizes.split(",")]:
            rec = run(nel, args.reps, args.inner)
            rec["device"] = info["name"].strip() or "unnamed"
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
