"""Cost of the forms with point coefficients (csrc/tg_coef.hip and the coefficient endings of csrc/tg_postproc.hip) next to
the kernels they stand beside (developer tool / profile source).

``rational_volume`` of tests/geom_util.py with nel^3 elements, p = 2 and 3, nq = p + 1, random point coefficients:

  * element-kernel time (the library's TIGAR_ASM_TIME line) of ``tg_assemble_coef_matrix`` with the diffusion tensor only
    and with all four terms, from plain and from rational data, sum-factorised (the route of these shapes) and through the
    plain kernel (TIGAR_ASM_LEGACY=1), next to the Laplace twin on the same two routes.  The twin is the yardstick; the
    ratios are reported.
  * the transform pass ``tg_coef_transform`` on its own, and ``tg_quad_load_flux`` next to ``tg_quad_load`` (wall time of
    the call, ending in a device synchronise).
  * the shares of one Newton step of the quasilinear problem of tests/coef_problem.py on the quarter annulus (--newton
    elements per direction): evaluation at the points, the host law, residual, tangent, PtAP, solve.

Alternating repeats in one process after a warm-up round; medians, spread = max - min.

    python tools/coef_bench.py [--sizes 32,48,64] [--degrees 2,3] [--reps 5] [--newton 64] [--out profiles/coef_bench.jsonl]
                               [--resources NEW.txt --parent-resources PARENT.txt]

``--resources`` / ``--parent-resources``: the remarks of ``hipcc -Rpass-analysis=kernel-resource-usage`` for
csrc/tg_coef.hip, csrc/tg_postproc.hip and csrc/tg_assemble.hip of this tree and for the last two of the parent commit; the
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
from geom_util import rational_volume, quarter_annulus  # noqa: E402
from rational_bench import resource_record, stats, timed_assembly  # noqa: E402


def wall(fn):
    dev.sync()
    t0 = time.perf_counter()
    r = fn()
    dev.sync()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, r


def run(p, nel, reps):
    kvs, C = rational_volume(p, (nel,) * 3)
    gen = t.EqualOrderSpline(tc.selfcomm, 1, N.NURBSControlMesh([p] * 3, kvs, C))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k]) for k in range(3)]
    dcp = [f.vector() for f in gen.cpFuncs]
    npts = dev.quad_count(uks, p + 1)
    rng = np.random.default_rng(p * 100 + nel)
    rand = lambda k: dev.DeviceVector(data=rng.standard_normal(k * npts))
    A, b, c, m, s, Fq = rand(9), rand(3), rand(3), rand(1), rand(1), rand(3)
    coefs = {"diffusion": (A, None, None, None), "all_four": (A, b, c, m)}
    os.environ["TIGAR_ASM_TIME"] = "1"
    ker, tr, routes = {}, {}, {}
    variants = [(terms, rat) for terms in coefs for rat in (False, True)]
    twins = [("laplace", False, False), ("laplace_rational", True, False), ("laplace_plain_kernel", False, True),
             ("laplace_rational_plain_kernel", True, True)]
    loads = {"quad_load": lambda: dev.quad_load(uks, p, dcp, s), "quad_load_flux": lambda: dev.quad_load_flux(uks, p, dcp, s, Fq),
             "quad_load_rational": lambda: dev.quad_load(uks, p, dcp, s, rational=True),
             "quad_load_flux_rational": lambda: dev.quad_load_flux(uks, p, dcp, s, Fq, rational=True)}
    lt = {k: [] for k in loads}
    for rep in range(reps + 1):                              # (round 0 warms up)
        for terms, rat in variants:
            name = terms + ("_rational" if rat else "")
            ms, coef = wall(lambda: dev.coef_transform(uks, p, dcp, *coefs[terms], rational=rat))
            k_ms, _, which = timed_assembly(lambda: dev.assemble_coef_matrix(uks, p, dcp, coef))
            routes[name] = which
            os.environ["TIGAR_ASM_LEGACY"] = "1"
            kp_ms, _, which = timed_assembly(lambda: dev.assemble_coef_matrix(uks, p, dcp, coef))
            os.environ.pop("TIGAR_ASM_LEGACY", None)
            routes[name + "_plain_kernel"] = which
            del coef
            gc.collect()
            if rep:
                tr.setdefault(name, []).append(ms)
                ker.setdefault(name, []).append(k_ms)
                ker.setdefault(name + "_plain_kernel", []).append(kp_ms)
        for name, rat, legacy in twins:
            if legacy:
                os.environ["TIGAR_ASM_LEGACY"] = "1"
            k_ms, _, which = timed_assembly(lambda: dev.assemble_mapped_matrix(uks, p, dcp, "laplace", rational=rat))
            os.environ.pop("TIGAR_ASM_LEGACY", None)
            gc.collect()
            if rep:
                ker.setdefault(name, []).append(k_ms)
        for name, call in loads.items():
            ms, r = wall(call)
            del r
            if rep:
                lt[name].append(ms)
    os.environ.pop("TIGAR_ASM_TIME", None)
    rec = {"record": "coefficient forms", "p": p, "nel": nel, "points": npts, "fe_nodes": dcp[0].size(), "reps": reps,
           "routes": routes, "element_kernels": {k: stats(v) for k, v in ker.items()}, "transform": {k: stats(v) for k, v in tr.items()},
           "loads": {k: stats(v) for k, v in lt.items()}}
    med = lambda k: rec["element_kernels"][k]["median_ms"]
    rec["ratios"] = {
        "diffusion_to_laplace": round(med("diffusion") / med("laplace"), 3),
        "diffusion_rational_to_laplace_rational": round(med("diffusion_rational") / med("laplace_rational"), 3),
        "diffusion_to_laplace_rational": round(med("diffusion") / med("laplace_rational"), 3),
        "all_four_to_diffusion": round(med("all_four") / med("diffusion"), 3),
        "plain_kernels_diffusion_to_laplace": round(med("diffusion_plain_kernel") / med("laplace_plain_kernel"), 3),
        "diffusion_plain_kernel_to_sum_factorised": round(med("diffusion_plain_kernel") / med("diffusion"), 2),
        "load_flux_to_load": round(rec["loads"]["quad_load_flux"]["median_ms"] / rec["loads"]["quad_load"]["median_ms"], 3)}
    return rec


def newton_shares(nel, reps):
    import coef_problem as P
    kv, Pf = quarter_annulus(nel)
    gen = t.EqualOrderSpline(1, N.NURBSControlMesh([2, 2], [kv, kv], Pf))
    sp0 = gen.getScalarSpline(0)
    for direction in (0, 1):
        for side in (0, 1):
            gen.addZeroDofs(0, sp0.getSideDofs(direction, side))
    spline = t.ExtractedSpline(gen, 4)
    spline.setSolverOptions(linearSolver=t.PETScLUSolver(), relativeTolerance=1e-10, maxIters=25)
    u = t.Function(spline.V)
    res = F.QuasilinearResidual(u, spline, P.residual, P.tangent, f=P.rhs, rational=True)
    hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u)        # (also the warm-up; u is the solution now)
    V = spline.V
    parts = {k: [] for k in ("evaluation", "host_law", "residual", "tangent", "ptap", "solve")}
    for rep in range(reps):
        ms, (pts, uq, gq) = wall(lambda: res.state(V))
        parts["evaluation"].append(ms)
        t0 = time.perf_counter()
        flux, src = P.residual(pts.x, uq, gq)
        Aq, _, _, mq = P.tangent(pts.x, uq, gq)
        parts["host_law"].append((time.perf_counter() - t0) * 1e3)
        fq = pts.values(P.rhs)
        ms, r = wall(lambda: dev.quad_load_flux(pts.verts, pts.p, pts.cp, pts.values(src - fq.get_local()), pts.vector_values(flux),
                                               nq=pts.nq, rational=True))
        parts["residual"].append(ms)
        ms, A = wall(lambda: F.CoefficientForm(spline, Aq, None, None, mq, rational=True).assemble_matrix(V))
        parts["tangent"].append(ms)
        ms, (K, bb) = wall(lambda: (spline.extractMatrix(A), spline.extractVector(r)))
        parts["ptap"].append(ms)
        ms, _ = wall(lambda: spline.solveLinearSystem(K, bb, t.Function(V)))
        parts["solve"].append(ms)
    rec = {"record": "newton step", "problem": "quarter annulus, p = 2, rational", "nel": nel, "points": pts.npts,
           "dofs": int(spline.M.shape[1]), "newton_iterations": len(hist), "reps": reps,
           "parts": {k: stats(v) for k, v in parts.items()}}
    total = sum(v["median_ms"] for v in rec["parts"].values())
    rec["shares_percent"] = {k: round(100.0 * v["median_ms"] / total, 1) for k, v in rec["parts"].items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,48,64")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--newton", type=int, default=64)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--parent-resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coef_bench.jsonl"))
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
            for nel in [int(v) for v in args.sizes.split(",") if v]:
                rec = run(p, nel, args.reps)
                rec["device"] = info["name"]
                emit(rec)
        if args.newton:
            rec = newton_shares(args.newton, args.reps)
            rec["device"] = info["name"]
            emit(rec)


if __name__ == "__main__":
    main()
