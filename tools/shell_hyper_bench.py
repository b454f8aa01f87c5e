"""Cost of the hyperelastic Kirchhoff-Love law (kind 1 of ``tg_shell_points``) and of the follower pressure
(``tg_shell_pressure_points``) next to what they stand beside: the St. Venant-Kirchhoff law (kind 0) on the same jets, and the
host route of ``ShellResidual`` (developer tool / profile source).

First line: the compiler's resource report (``hipcc -Rpass-analysis=kernel-resource-usage`` of csrc/tg_shell.hip for gfx950,
its remarks in the file ``--resources``) of both law kernels and of the pressure kernel.  Then, on the quarter-cylinder surface
of tests/jet_reference.py with nel^2 elements, p = 2 and 3, nq = p + 1:

  * ``tg_shell_points`` with all three outputs, kind 1 with 1 and with 4 thickness points and kind 0 on the same jets (wall time
    of the call, which ends in a device synchronise and includes the allocation of the outputs): both kinds move
    (36 read + 18 + 324 + 1 written) x 8 = 3032 bytes per point; the rate next to the 6.3 TB/s of a device copy;
  * the pressure kernel adding into s and T: (12 read + 15 read and written) x 8 = 336 bytes per point;
  * one Newton-step assembly of the inflated square (--newton elements per direction, p = 2, follower pressure) with the device
    law and with ``device_law=False``: jets, the law with the pressure on those jets (timed by itself), residual load, tangent
    (transform and assembly).

Alternating repeats in one process after a warm-up round; medians, spread = max - min.

    python tools/shell_hyper_bench.py [--sizes 128,256,512] [--degrees 2,3] [--reps 5] [--newton 64] [--resources REMARKS.txt]
                                      [--resources-only] [--out profiles/shell_hyper_bench.jsonl]
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

COPY_TBS = 6.3
LAW_BYTES = (36 + 18 + 324 + 1) * 8
PRESSURE_BYTES = (12 + 2 * 15) * 8
KERNELS = ("k_shell_points<0>", "k_shell_hyper_points", "k_shell_pressure_points")


def resource_record(path):
    from rational_bench import FIELDS, demangle, parse_resources
    res = parse_resources(path)
    names = demangle(sorted(res))
    out = {}
    for k, v in res.items():
        for want in KERNELS:
            if names[k].split("(")[0].replace("void ", "") == want:
                out[want] = {f: v.get(f) for f in FIELDS}
    return {"record": "kernel resources", "source": "csrc/tg_shell.hip", "arch": "gfx950", "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--newton", type=int, default=64)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shell_hyper_bench.jsonl"))
    ap.add_argument("--resources-only", action="store_true", help="write the compiler's resource report alone (needs no GPU)")
    args = ap.parse_args()
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.resources:
            emit(resource_record(args.resources))
        if args.resources_only:
            return
        measure(args, emit)


def measure(args, emit):
    import tigar_amd as t
    from tigar_amd import BSplines as B, device as dev, forms as F
    import jet_reference as JR
    import postproc_reference as R
    import shell_reference as SR
    import shell_hyper_reference as HR
    from rational_bench import stats

    def wall(fn):
        dev.sync()
        t0 = time.perf_counter()
        r = fn()
        dev.sync()
        return (time.perf_counter() - t0) * 1e3, r

    def rate(ms, nbytes, npts):
        tbs = nbytes * npts / (np.median(ms) * 1e-3) / 1e12
        return dict(stats(ms), bytes_per_point=nbytes, tb_per_s=round(tbs, 3), of_copy_rate=round(tbs / COPY_TBS, 3))

    info = dev.device_info()
    laws = {"kind0_svk": (0, (SR.E_MOD, SR.NU, SR.THICKNESS)), "kind1_nth1": (1, (HR.MU, SR.THICKNESS, 1)),
            "kind1_nth4": (1, (HR.MU, SR.THICKNESS, 4))}
    for p in [int(v) for v in args.degrees.split(",")]:
        for nel in [int(v) for v in args.sizes.split(",") if v]:
            uks = [np.linspace(0.0, 1.0, nel + 1)] * 2
            X = R.lagrange_nodes(uks, p)
            wx, wy, w = JR._arc_homogeneous(X[0])
            dcp = [dev.DeviceVector(data=np.ascontiguousarray(c)) for c in (wx, wy, w * 1.5 * X[1], w)]
            npts = dev.quad_count(uks, p + 1)
            Xj = dev.quad_geometry_jet(uks, p, dcp)
            Uj = dev.DeviceVector(data=1e-3 * np.random.default_rng(p + nel).standard_normal(18 * npts))
            s, Tq = dev.DeviceVector(18 * npts), dev.DeviceVector(324 * npts)
            rows = {k: [] for k in list(laws) + ["pressure"]}
            for rep in range(args.reps + 1):                   # (round 0 warms up)
                for name, (kind, par) in laws.items():
                    ms, out = wall(lambda: dev.shell_law_points(kind, par, Xj, Uj, True, True, True))
                    assert out[3] == 0
                    del out
                    gc.collect()
                    if rep:
                        rows[name].append(ms)
                ms, _ = wall(lambda: dev.shell_pressure_points(1.0, Xj, Uj, s, Tq))
                if rep:
                    rows["pressure"].append(ms)
            rec = {"record": "shell law kernels", "device": info["name"], "p": p, "nel": nel, "points": npts, "reps": args.reps}
            for name in laws:
                rec[name] = rate(rows[name], LAW_BYTES, npts)
            rec["pressure"] = rate(rows["pressure"], PRESSURE_BYTES, npts)
            rec["ratios"] = {k + "_to_kind0": round(rec[k]["median_ms"] / rec["kind0_svk"]["median_ms"], 3) for k in ("kind1_nth1", "kind1_nth4")}
            emit(rec)
            del Xj, Uj, s, Tq, dcp
            gc.collect()
    if args.newton:
        p, nel = 2, args.newton
        mesh = B.ExplicitBSplineControlMesh([p, p], [B.uniformKnots(p, -1., 1., nel)] * 2, extraDim=1)
        gen = t.EqualOrderSpline(3, mesh)
        sc = gen.getControlMesh().getScalarSpline()
        for side in (0, 1):
            for direction in (0, 1):
                for i in range(3):
                    gen.addZeroDofs(i, sc.getSideDofs(direction, side, nLayers=2))
        spline = t.ExtractedSpline(gen, 2 * p)
        V = spline.V
        u = t.Function(V)
        u.vector().set_local(1e-4 * np.random.default_rng(0).standard_normal(V.dim()))
        mat = F.KirchhoffLoveHyper(HR.MU, HR.THICKNESS)
        out = {}
        for name, flag in (("device_law", True), ("host_law", False)):
            res = F.ShellResidual(u, spline, mat, device_law=flag, pressure=1.0)
            parts = {k: [] for k in ("jets", "law_and_pressure", "residual_load", "tangent")}
            compute_jets = res.jets
            for rep in range(args.reps + 1):
                res.jets = compute_jets
                ms_j, state = wall(lambda: res.jets(V))
                res.jets = lambda V_, state=state: state            # the law alone, on the jets just computed
                ms_l, (pts, g, s, Tq, _) = wall(lambda: res.law(V, load=True, tangent=True))
                ms_r, r = wall(lambda: F.VectorJetLoadForm(s, spline).assemble_vector(V))
                form = F.VectorJetCoefficientForm(spline, Tq)
                form._symmetric_hint = False
                ms_t, K = wall(lambda: form.assemble_matrix(V))
                del s, Tq, r, K, form
                gc.collect()
                if rep:
                    for k, v in zip(parts, (ms_j, ms_l, ms_r, ms_t)):
                        parts[k].append(v)
            recp = {k: stats(v) for k, v in parts.items()}
            out[name] = {"parts": recp, "assembly_ms": round(sum(v["median_ms"] for v in recp.values()), 3)}
        emit({"record": "newton step assembly", "device": info["name"], "problem": "inflated clamped square, p = 2, neo-Hookean, "
              "4 thickness points, follower pressure", "nel": nel, "points": pts.npts, "reps": args.reps, **out})


if __name__ == "__main__":
    main()
