"""Cost of the flow point kernels (csrc/tg_flow.hip, the block ending of csrc/tg_postproc.hip with b and c per block) next to
what they stand beside (developer tool / profile source).

``rational_volume`` of tests/geom_util.py with nel^3 elements, p = 2 and 3, nq = p + 1, four fields (u_1, u_2, u_3, p):

  * the law kernel ``tg_flow_points`` with all seven outputs (wall time of the call, which includes the allocation of the
    outputs, ended by a device synchronise; no a0, no f): bytes moved = (nF + nF nsd + nsd^2 in, nF + nF nsd + nF^2 (nsd^2 + 2 nsd
    + 1) + 2 out) 8 npts = 299 x 8 npts, and the rate next to the 6.3 TB/s of a device copy;
  * ``tg_coef_transform_system`` (one pass, the geometry once per point) next to nF^2 = 16 calls of ``tg_coef_transform`` on the
    blocks' data -- the yardstick;
  * one Newton step of the steady flow on the same patch (--newton elements per direction, p = 2) with the law on the device and
    with the same law as a host callable through ``SystemResidual`` (download, numpy, upload): state at the points, law and
    loads (residual), law, transform and assembly (tangent), PtAP, solve (the default direct solver).

Alternating repeats in one process after a warm-up round; medians, spread = max - min.

    python tools/flow_bench.py [--sizes 32] [--degrees 2,3] [--reps 5] [--newton 12] [--out profiles/flow_bench.jsonl]
                               [--resources NEW.txt --parent-resources PARENT.txt [--resources-only]]

``--resources`` / ``--parent-resources``: the remarks of ``hipcc -Rpass-analysis=kernel-resource-usage`` for csrc/tg_flow.hip,
csrc/tg_postproc.hip, csrc/tg_coef.hip and csrc/tg_assemble.hip of this tree and for the last three of the parent commit; the
first JSON line then lists the new kernels and says whether the existing ones kept their figures.
"""
import argparse
import gc
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
from tigar_amd import NURBS as N, device as dev, forms as F  # noqa: E402
from tigar_amd import common as tc  # noqa: E402
from geom_util import rational_volume  # noqa: E402
from rational_bench import resource_record, stats  # noqa: E402

RHO, MU = 1.0, 0.05
COPY_TBS = 6.3


def wall(fn):
    dev.sync()
    t0 = time.perf_counter()
    r = fn()
    dev.sync()
    return (time.perf_counter() - t0) * 1e3, r


def smooth_state(gen, amplitude):
    """nodal values of a smooth velocity and pressure of the given amplitude, field after field"""
    x = [f.vector().get_local() for f in gen.cpFuncs]
    return amplitude * np.concatenate([np.sin(2.0 * x[(i + 1) % 3] + i) * np.cos(x[i % 3]) for i in range(4)])


def run(p, nel, reps):
    nsd, nF = 3, 4
    kvs, C = rational_volume(p, (nel,) * 3)
    gen = t.EqualOrderSpline(tc.selfcomm, nF, N.NURBSControlMesh([p] * 3, kvs, C))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k]) for k in range(3)]
    dcp = [f.vector() for f in gen.cpFuncs]
    npts = dev.quad_count(uks, p + 1)
    u = t.Function(gen.V)
    u.vector().set_local(smooth_state(gen, 0.5))
    law = F.IncompressibleFlow(RHO, MU)
    pts, _, _, Uq, Gq = F._system_state(gen, gen.V, u, None, True, "flow_bench")
    metric = pts.metric
    times = {k: [] for k in ("law", "system_fused", "sixteen_scalar_transforms", "metric")}
    for rep in range(reps + 1):                              # (round 0 warms up)
        ms, out = wall(lambda: dev.flow_points(law.params(), nsd, Uq, Gq, metric, None, None, True, True, True))
        A, b, c, M = out[2:6]
        del out
        ms_m, Gm = wall(lambda: dev.quad_metric(uks, p, dcp))
        del Gm
        parts = []
        for blk in range(nF * nF):                           # the blocks' data as vectors of their own (not timed)
            one = []
            for v, each in ((A, nsd * nsd), (b, nsd), (c, nsd), (M, 1)):
                w = dev.DeviceVector(each * npts, zero=False)
                dev.vec_copy_range(w, 0, v, blk * each * npts, each * npts)
                one.append(w)
            parts.append(one)
        ms_f, coef = wall(lambda: dev.coef_transform_system(uks, p, dcp, nF, A, b, c, M, rational=True))
        del coef
        ms_16, sixteen = wall(lambda: [dev.coef_transform(uks, p, dcp, *one, a_kind=2, rational=True) for one in parts])
        del sixteen, parts, A, b, c, M
        gc.collect()
        if rep:
            for k, v in zip(times, (ms, ms_f, ms_16, ms_m)):
                times[k].append(v)
    each = nF + nF * nsd + nsd * nsd + nF + nF * nsd + nF * nF * (nsd * nsd + 2 * nsd + 1) + 2
    nbytes = each * 8 * npts
    rec = {"record": "flow point kernels", "p": p, "nel": nel, "points": npts, "fe_nodes": dcp[0].size(), "reps": reps,
           "law": dict(stats(times["law"]), bytes=nbytes, tb_per_s=round(nbytes / (np.median(times["law"]) * 1e-3) / 1e12, 3),
                       of_copy_rate=round(nbytes / (np.median(times["law"]) * 1e-3) / 1e12 / COPY_TBS, 3)),
           "metric": stats(times["metric"]),
           "transform": {k: stats(times[k]) for k in ("system_fused", "sixteen_scalar_transforms")}}
    fused, sixteen = rec["transform"]["system_fused"], rec["transform"]["sixteen_scalar_transforms"]
    rec["ratios"] = {"fused_transform_to_sixteen_scalar": round(fused["median_ms"] / sixteen["median_ms"], 3),
                     "fused_transform_gain_beyond_spread": bool(sixteen["median_ms"] - fused["median_ms"] > fused["spread_ms"] + sixteen["spread_ms"])}
    return rec


def newton_step(nel, reps):
    p, nF = 2, 4
    kvs, C = rational_volume(p, (nel,) * 3)
    gen = t.EqualOrderSpline(tc.selfcomm, nF, N.NURBSControlMesh([p] * 3, kvs, C))
    sp0 = gen.getScalarSpline(0)
    for f in range(3):
        for k in range(3):
            for side in (0, 1):
                gen.addZeroDofs(f, sp0.getSideDofs(k, side))
    gen.addZeroDofs(3, [0])
    spline = t.ExtractedSpline(gen, 2 * p, comm=gen.comm)
    # (the default direct solver: Jacobi-GMRES does not converge on this stabilised saddle-point system -- 10000 iterations
    # without progress at 16^3 elements)
    V = spline.V
    u = t.Function(V)
    u.vector().set_local(smooth_state(gen, 0.1))
    law = F.IncompressibleFlow(RHO, MU)
    pts = F.quadrature_points(spline, spline.V_control)
    G = F.point_unblock(pts.metric.get_local(), pts.npts, (3, 3))

    def host_residual(x, U, gU):
        s, Fx = law.host(U, gU, G)[:2]
        return Fx, s
    residuals = {"device_law": F.FlowResidual(u, spline, law, rational=True),
                 "host_callable": F.SystemResidual(u, spline, host_residual, lambda x, U, gU: law.host(U, gU, G)[2:6], rational=True)}
    out = {}
    for name, res in residuals.items():
        parts = {k: [] for k in ("residual", "tangent", "ptap", "solve")}
        for rep in range(reps + 1):
            ms_r, r = wall(lambda: res.assemble_vector(V))
            ms_t, K_fe = wall(lambda: res.tangent().assemble_matrix(V))
            ms_p, (K, b) = wall(lambda: (spline.extractMatrix(K_fe), spline.extractVector(r)))
            ms_s, _ = wall(lambda: spline.solveLinearSystem(K, b, t.Function(V)))
            del r, K_fe, K, b
            gc.collect()
            if rep:
                for k, v in zip(parts, (ms_r, ms_t, ms_p, ms_s)):
                    parts[k].append(v)
        rec = {k: stats(v) for k, v in parts.items()}
        total = sum(v["median_ms"] for v in rec.values())
        out[name] = {"parts": rec, "step_ms": round(total, 3), "shares_percent": {k: round(100.0 * v["median_ms"] / total, 1) for k, v in rec.items()}}
    return {"record": "newton step", "problem": "rational volume, p = 2, steady flow, rational, no-slip walls", "nel": nel,
            "points": pts.npts, "dofs": int(spline.M.shape[1]), "reps": reps, "solver": "default direct solver", **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--newton", type=int, default=12)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--parent-resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_bench.jsonl"))
    ap.add_argument("--resources-only", action="store_true", help="write the compiler's resource report alone (needs no GPU)")
    args = ap.parse_args()
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.resources and args.parent_resources:
            emit(resource_record(args.resources, args.parent_resources))
        if args.resources_only:
            return
        for p in [int(v) for v in args.degrees.split(",")]:
            for nel in [int(v) for v in args.sizes.split(",")]:
                emit(run(p, nel, args.reps))
        if args.newton > 0:
            emit(newton_step(args.newton, args.reps))


if __name__ == "__main__":
    main()
