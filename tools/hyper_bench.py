"""Cost of finite-strain elasticity at the points (csrc/tg_material.hip, the block ending of csrc/tg_postproc.hip, the block
driver of csrc/tg_coef.hip) next to what it stands beside (developer tool / profile source).

``rational_volume`` of tests/geom_util.py with nel^3 elements, p = 2 and 3, nq = p + 1, three displacement fields:

  * the law kernel ``tg_material_points`` per kind with all three outputs (wall time of the call, which ends in a device
    synchronise and includes the allocation of the outputs): bytes moved = (2 d^2 + d^4 + 1) 8 npts, and the rate next to
    the 6.3 TB/s of a device copy;
  * ``tg_coef_transform_blocks`` (one pass, the geometry once per point) next to nF^2 = 9 calls of ``tg_coef_transform`` on the
    blocks' tensors -- the yardstick;
  * ``tg_assemble_coef_blocks`` next to ``ElasticityForm(geometry=...).assemble_matrix`` (nine blocks each, then
    ``tg_csr_from_blocks``): wall time, and the sum of the nine element-kernel times of the library's TIGAR_ASM_TIME lines;
  * the shares of one Newton step of a neo-Hookean solid on the same patch (--newton elements per direction, p = 2): gradient
    of u at the points, the law (on the device, and the same law as a host callable: download, numpy, upload), residual
    loads, tangent (transform and assembly), PtAP, solve (CG with Jacobi to 1e-8).

Alternating repeats in one process after a warm-up round; medians, spread = max - min.

    python tools/hyper_bench.py [--sizes 32,48] [--degrees 2,3] [--reps 5] [--newton 24] [--out profiles/hyper_bench.jsonl]
                                [--resources NEW.txt --parent-resources PARENT.txt [--resources-only]]

``--resources`` / ``--parent-resources``: the remarks of ``hipcc -Rpass-analysis=kernel-resource-usage`` for
csrc/tg_material.hip, csrc/tg_postproc.hip, csrc/tg_coef.hip and csrc/tg_assemble.hip of this tree and for the last three of
the parent commit; the first JSON line then lists the new kernels and says whether the existing ones kept their figures.
"""
import argparse
import gc
import json
import os
import re
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
from rational_bench import capture_stderr, resource_record, stats  # noqa: E402

LAM, MU = 2.0, 1.0
COPY_TBS = 6.3


def wall(fn):
    dev.sync()
    t0 = time.perf_counter()
    r = fn()
    dev.sync()
    return (time.perf_counter() - t0) * 1e3, r


def timed_blocks(fn):
    """(wall ms, sum of the element-kernel ms of the library's lines, the routes they name)"""
    dev.sync()
    with capture_stderr() as cap:
        ms, out = wall(fn)
    del out
    found = re.findall(r"element kernels ([0-9.]+) ms \(([a-z-]+)\)", cap.text)
    return ms, sum(float(v) for v, _ in found), sorted(set(w for _, w in found)), len(found)


def smooth_state(gen, amplitude):
    """nodal values of a smooth displacement of the given amplitude, field after field"""
    x = [f.vector().get_local() for f in gen.cpFuncs]
    return amplitude * np.concatenate([np.sin(2.0 * x[(i + 1) % 3] + i) * np.cos(x[i]) for i in range(3)])


def run(p, nel, reps):
    kvs, C = rational_volume(p, (nel,) * 3)
    gen = t.EqualOrderSpline(tc.selfcomm, 3, N.NURBSControlMesh([p] * 3, kvs, C))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k]) for k in range(3)]
    dcp = [f.vector() for f in gen.cpFuncs]
    npts = dev.quad_count(uks, p + 1)
    u = t.Function(gen.V)
    u.vector().set_local(smooth_state(gen, 0.02))
    res = F.HyperelasticResidual(u, gen, F.NeoHookean(LAM, MU), rational=True)
    gradu = res.grad_u(gen.V)[3]
    law, tr, asm, routes = {}, {}, {}, {}
    os.environ["TIGAR_ASM_TIME"] = "1"
    elast = F.ElasticityForm(LAM, MU, geometry=gen, rational=True)
    for rep in range(reps + 1):                              # (round 0 warms up)
        for kind, name in enumerate(("linear", "st_venant_kirchhoff", "neo_hookean")):
            ms, out = wall(lambda: dev.material_points(kind, LAM, MU, 3, gradu, True, True, True))
            del out
            if rep:
                law.setdefault(name, []).append(ms)
        A = dev.material_points(2, LAM, MU, 3, gradu, False, True, False)[1]
        parts = []
        for b in range(9):                                   # the blocks' tensors as vectors of their own (not timed)
            v = dev.DeviceVector(9 * npts, zero=False)
            dev.vec_copy_range(v, 0, A, b * 9 * npts, 9 * npts)
            parts.append(v)
        ms_f, coef = wall(lambda: dev.coef_transform_blocks(uks, p, dcp, A, None, rational=True))
        ms_9, nine = wall(lambda: [dev.coef_transform(uks, p, dcp, v, a_kind=2, rational=True) for v in parts])
        del nine, parts, A
        gc.collect()
        w_ms, k_ms, which, nlines = timed_blocks(lambda: dev.assemble_coef_blocks(uks, p, dcp, coef))
        routes["blocks"] = which
        del coef
        gc.collect()
        we_ms, ke_ms, which, nlines_e = timed_blocks(lambda: elast.assemble_matrix(gen.V))
        routes["elasticity_form"] = which
        gc.collect()
        if rep:
            tr.setdefault("blocks_fused", []).append(ms_f)
            tr.setdefault("nine_scalar_transforms", []).append(ms_9)
            asm.setdefault("blocks_wall", []).append(w_ms)
            asm.setdefault("blocks_element_kernels", []).append(k_ms)
            asm.setdefault("elasticity_form_wall", []).append(we_ms)
            asm.setdefault("elasticity_form_element_kernels", []).append(ke_ms)
    os.environ.pop("TIGAR_ASM_TIME", None)
    nbytes = (2 * 9 + 81 + 1) * 8 * npts
    rec = {"record": "finite-strain point kernels", "p": p, "nel": nel, "points": npts, "fe_nodes": dcp[0].size(), "reps": reps,
           "routes": routes, "timing_lines_per_assembly": [nlines, nlines_e],
           "law": {k: dict(stats(v), bytes=nbytes, tb_per_s=round(nbytes / (np.median(v) * 1e-3) / 1e12, 3),
                           of_copy_rate=round(nbytes / (np.median(v) * 1e-3) / 1e12 / COPY_TBS, 3)) for k, v in law.items()},
           "transform": {k: stats(v) for k, v in tr.items()}, "assembly": {k: stats(v) for k, v in asm.items()}}
    med = lambda d, k: rec[d][k]["median_ms"]
    rec["ratios"] = {
        "fused_transform_to_nine_scalar": round(med("transform", "blocks_fused") / med("transform", "nine_scalar_transforms"), 3),
        "fused_transform_gain_beyond_spread": bool(med("transform", "nine_scalar_transforms") - med("transform", "blocks_fused") >
                                                   rec["transform"]["blocks_fused"]["spread_ms"] +
                                                   rec["transform"]["nine_scalar_transforms"]["spread_ms"]),
        "blocks_to_elasticity_form_wall": round(med("assembly", "blocks_wall") / med("assembly", "elasticity_form_wall"), 3),
        "blocks_to_elasticity_form_element_kernels": round(med("assembly", "blocks_element_kernels") /
                                                           med("assembly", "elasticity_form_element_kernels"), 3)}
    return rec


class HostLaw(object):
    """the neo-Hookean law as a user's host callable"""

    def __init__(self):
        self.law = F.NeoHookean(LAM, MU)

    def host(self, Fm):
        return self.law.host(Fm)


def newton_shares(nel, reps):
    p = 2
    kvs, C = rational_volume(p, (nel,) * 3)
    gen = t.EqualOrderSpline(tc.selfcomm, 3, N.NURBSControlMesh([p] * 3, kvs, C))
    sp0 = gen.getScalarSpline(0)
    for f in range(3):
        gen.addZeroDofs(f, sp0.getSideDofs(0, 0))
    spline = t.ExtractedSpline(gen, 2 * p, comm=gen.comm)
    solver = t.PETScKrylovSolver("cg", "jacobi")
    solver.parameters["relative_tolerance"] = 1e-8
    spline.setSolverOptions(linearSolver=solver)
    V = spline.V
    u = t.Function(V)
    u.vector().set_local(smooth_state(gen, 0.02))
    out = {}
    for name, material in (("device_law", F.NeoHookean(LAM, MU)), ("host_law", HostLaw())):
        res = F.HyperelasticResidual(u, spline, material, rational=True)
        parts = {k: [] for k in ("gradient", "law", "residual", "tangent", "ptap", "solve")}
        for rep in range(reps + 1):
            ms_g, (pts, g, nF, H) = wall(lambda: res.grad_u(V))
            ms_all, (_, _, _, P, A, _) = wall(lambda: res.law(V, stress=True, tangent=True))
            ms_r, r = wall(lambda: F._field_loads(pts, g.num_nodes(), nF, None, P, True))
            form = F.VectorCoefficientForm(spline, A, rational=True)
            form._symmetric_hint = True
            ms_t, K_fe = wall(lambda: form.assemble_matrix(V))
            ms_p, (K, b) = wall(lambda: (spline.extractMatrix(K_fe), spline.extractVector(r)))
            ms_s, _ = wall(lambda: spline.solveLinearSystem(K, b, t.Function(V)))
            del P, A, r, K_fe, K, b, form
            gc.collect()
            if rep:
                for k, v in zip(parts, (ms_g, ms_all - ms_g, ms_r, ms_t, ms_p, ms_s)):
                    parts[k].append(v)
        rec = {k: stats(v) for k, v in parts.items()}
        total = sum(v["median_ms"] for v in rec.values())
        out[name] = {"parts": rec, "step_ms": round(total, 3), "shares_percent": {k: round(100.0 * v["median_ms"] / total, 1) for k, v in rec.items()}}
    return {"record": "newton step", "problem": "rational volume, p = 2, neo-Hookean, rational, one face held", "nel": nel,
            "points": pts.npts, "dofs": int(spline.M.shape[1]), "reps": reps, "solver": "cg + jacobi, 1e-8", **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,48")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--newton", type=int, default=24)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--parent-resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyper_bench.jsonl"))
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
        info = dev.device_info()
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
