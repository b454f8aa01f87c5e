"""Cost of the point kernel of structural dynamics (``tg_point_dynamics``) and of a dynamic Newton iteration next to what they
stand beside (profiles/dynamics_bench.jsonl):

  * on the jets of the cylinder surface at 128^2, 256^2, 512^2 elements, p = 2, 3: the kernel as a dynamic RESIDUAL calls it
    (all 18 slots of s scaled, inertia and plane in the value slots), as a TANGENT calls it (the 9 value-value entries of T) and
    with ``e_out`` alone, next to ``tg_shell_points`` (kind 0, all three outputs) on the same jets -- wall time of the call
    (the residual and tangent calls end in the read-back of the active count, the law in that of its own count), median of
    5 alternating repeats after one warm-up round, with the spread; and next to the 6.3 TB/s of a device copy on the bytes
    each call moves (counted below; the law moves 3032 B per point);
  * the phases of one Newton iteration of a dynamic step at 64^2, p = 2 (St. Venant-Kirchhoff, a plane through the shell) next
    to the static step of the same build, every phase timed by itself as tools/shell_hyper_bench.py does: jets, law (load
    and tangent in one call, on the jets just computed), dynamics (the y_alpha combination and the two launches of
    ``tg_point_dynamics`` with their read-backs; nothing in the static step), load, tangent (transform and element loop),
    PtAP (M^T A M and M^T R) and the solve; the yardstick is the static ``ShellResidual`` step.

  python tools/dynamics_bench.py [--sizes 128,256,512] [--degrees 2,3] [--reps 5] [--newton 64]
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
# per point: u value slots 3, X0 3, w 3 read; s 18 read and written | u 3, X0 3 read; 9 entries of T read and written | w 3, 1
RESIDUAL_BYTES, TANGENT_BYTES, ENERGY_BYTES = (9 + 36) * 8, (6 + 18) * 8, 4 * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--newton", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamics_bench.jsonl"))
    args = ap.parse_args()
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        measure(args, emit)


def measure(args, emit):
    import tigar_amd as t
    from tigar_amd import BSplines as B, device as dev, forms as F, timeIntegration as TI
    import jet_reference as JR
    import postproc_reference as R
    import shell_reference as SR
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
    plane = (0.6, 0.0, -0.8, -0.1)
    for p in [int(v) for v in args.degrees.split(",")]:
        for nel in [int(v) for v in args.sizes.split(",") if v]:
            uks = [np.linspace(0.0, 1.0, nel + 1)] * 2
            X = R.lagrange_nodes(uks, p)
            wx, wy, w = JR._arc_homogeneous(X[0])
            dcp = [dev.DeviceVector(data=np.ascontiguousarray(c)) for c in (wx, wy, w * 1.5 * X[1], w)]
            npts = dev.quad_count(uks, p + 1)
            Xj = dev.quad_geometry_jet(uks, p, dcp)
            X0, _ = dev.quad_points(uks, p, dcp)
            rng = np.random.default_rng(p + nel)
            Uj = dev.DeviceVector(data=1e-3 * rng.standard_normal(18 * npts))
            W = dev.DeviceVector(data=rng.standard_normal(3 * npts))
            s, Tq, e = dev.DeviceVector(18 * npts), dev.DeviceVector(324 * npts), dev.DeviceVector(npts)
            calls = {
                "law_kind0": lambda: dev.shell_points(0, SR.E_MOD, SR.NU, SR.THICKNESS, Xj, Uj, True, True, True),
                "dynamics_residual": lambda: dev.point_dynamics(3, 6, npts, (1.5, 2.0, 1.0, 0.0, 1e3, 0.0, 0.0), plane, X0, Uj, W, s=s, count=True),
                "dynamics_tangent": lambda: dev.point_dynamics(3, 6, npts, (1.0, 0.0, 0.0, 2.0, 0.0, 1e3, 0.0), plane, X0, Uj, T=Tq, count=True),
                "dynamics_energy": lambda: dev.point_dynamics(3, 6, npts, (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), w=W, e=e)}
            rows = {k: [] for k in calls}
            active = None
            for rep in range(args.reps + 1):                   # (round 0 warms up)
                for name, call in calls.items():
                    ms, out = wall(call)
                    if name == "dynamics_residual":
                        active = out
                    del out
                    gc.collect()
                    if rep:
                        rows[name].append(ms)
            rec = {"record": "point dynamics kernel", "device": info["name"], "p": p, "nel": nel, "points": npts, "reps": args.reps,
                   "active_points": active, "measured_against": "tg_shell_points kind 0 on the same jets; %.1f TB/s of a device copy" % COPY_TBS}
            for name, nbytes in (("law_kind0", LAW_BYTES), ("dynamics_residual", RESIDUAL_BYTES), ("dynamics_tangent", TANGENT_BYTES),
                                 ("dynamics_energy", ENERGY_BYTES)):
                rec[name] = rate(rows[name], nbytes, npts)
            rec["ratios_to_law"] = {k: round(rec[k]["median_ms"] / rec["law_kind0"]["median_ms"], 4)
                                    for k in ("dynamics_residual", "dynamics_tangent", "dynamics_energy")}
            emit(rec)
            del Xj, Uj, W, s, Tq, e, dcp, X0, calls
            gc.collect()
    if args.newton:
        p, nel = 2, args.newton
        pb = SR.problem(p, (nel, nel), SR.cylinder_homogeneous(), clamp=(1, 0, 2))
        from tigar_amd import NURBS as N
        gen = t.EqualOrderSpline(3, N.NURBSControlMesh([p, p], pb["kvs"], pb["C"]))
        sc = gen.getScalarSpline(0)
        for i in range(3):
            gen.addZeroDofs(i, sc.getSideDofs(1, 0, nLayers=2))
        spline = t.ExtractedSpline(gen, 2 * p)
        spline.setSolverOptions(linearSolver=t.PETScLUSolver())
        V = spline.V
        mat = F.KirchhoffLoveSVK(SR.E_MOD, SR.NU, SR.THICKNESS)
        rng = np.random.default_rng(0)
        fs = [t.Function(V) for _ in range(4)]
        for f in fs:
            f.vector().set_local(1e-4 * rng.standard_normal(V.dim()))
        y, old = fs[0], fs[1:]
        static = F.ShellResidual(y, spline, mat, rational=True)
        it = TI.GeneralizedAlphaIntegrator(0.5, 0.01, y, old)
        dyn = F.DynamicResidual(static, it, 1.0, contact=F.PlanePenalty((1.0, 1.0, 0.0), 1.0, 1e3))
        out = {}
        g, nF, pts = dyn._scope(V, None, None)
        k, c = dyn.contact.stiffness, dyn.coefficients()
        for name, law_obj in (("static", static), ("dynamic", dyn._law)):
            dynamic = name == "dynamic"
            parts = {k_: [] for k_ in ("jets", "law", "dynamics", "load", "tangent", "ptap", "solve")}
            for rep in range(args.reps + 1):
                ms_d = 0.0
                if dynamic:                                        # y_alpha (w is at the points after round 0)
                    ms_d, w = wall(lambda: dyn._state(g, nF, pts))
                ms_j, state = wall(lambda: law_obj.jets(V))
                law_obj.jets = lambda V_, state=state: state        # the law alone, on the jets just computed
                ms_l, (_, _, s, Tq, _) = wall(lambda: law_obj.law(V, load=True, tangent=True))
                del law_obj.jets
                if dynamic:                                        # the two launches of an iteration, each with its read-back
                    af = dyn.scale
                    ms_1, _ = wall(lambda: dev.point_dynamics(3, 6, pts.npts, (1.0 / af, c["m_u"], 1.0, 0.0, k / af, 0.0, 0.0),
                                                              dyn.contact.plane(), pts.x_device, state[3], w, s=s, count=True))
                    ms_2, _ = wall(lambda: dev.point_dynamics(3, 6, pts.npts, (1.0, 0.0, 0.0, c["t_m"], 0.0, k, 0.0),
                                                              dyn.contact.plane(), pts.x_device, state[3], T=Tq, count=True))
                    ms_d += ms_1 + ms_2
                ms_r, r = wall(lambda: F.VectorJetLoadForm(s, spline, rational=True).assemble_vector(V))
                form = F.VectorJetCoefficientForm(spline, Tq, rational=True)
                form._symmetric_hint = True
                ms_t, K = wall(lambda: form.assemble_matrix(V))
                ms_p, (MTAM, MTb) = wall(lambda: (spline.assembleMatrix(K), spline.assembleVector(r)))
                du = t.Function(V)
                ms_s, _ = wall(lambda: spline.solveLinearSystem(MTAM, MTb, du))
                del s, Tq, r, K, form, MTAM, MTb, du, state
                gc.collect()
                if rep:
                    for k_, v in zip(parts, (ms_j, ms_l, ms_d, ms_r, ms_t, ms_p, ms_s)):
                        parts[k_].append(v)
            recp = {k_: stats(v) for k_, v in parts.items()}
            out[name] = {"parts": recp, "iteration_ms": round(sum(v["median_ms"] for v in recp.values()), 3),
                         "assembly_ms": round(sum(v["median_ms"] for k_, v in recp.items() if k_ != "solve"), 3)}
        out["dynamic_to_static"] = {k_: round(out["dynamic"][k_] / out["static"][k_], 4) for k_ in ("iteration_ms", "assembly_ms")}
        emit({"record": "newton iteration", "device": info["name"], "problem": "clamped quarter-cylinder strip, p = 2, St. Venant-Kirchhoff, "
              "generalized-alpha with a plane penalty; every phase timed by itself, law and tangent evaluated once for residual and "
              "matrix; w at the points already evaluated", "nel": nel, "dofs": int(spline.M.shape[1]), "points": pts.npts,
              "reps": args.reps, "measured_against": "the static ShellResidual step of this build", **out})

if __name__ == "__main__":
    main()
