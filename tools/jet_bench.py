"""Cost of the second-derivative point forms (csrc/tg_jet.hip) and of the Kirchhoff-Love law (csrc/tg_shell.hip) next to what
they stand beside (developer tool / profile source).

The quarter-cylinder surface of tests/jet_reference.py with nel^2 elements, p = 2 and 3, nq = p + 1:

  * the jet matrix kernel for ONE block (``tg_assemble_jet_blocks``, nF = 1: 36 point values per point) next to ``k_coef_matrix``
    of a 2-D ``CoefficientForm`` on the same patch (``tg_assemble_coef_matrix``: 9 point values per point): wall time, and the
    element-kernel time of the library's TIGAR_ASM_TIME line;
  * the law kernel ``tg_shell_points`` with all three outputs (wall time of the call, which ends in a device synchronise and
    includes the allocation of the outputs): bytes per point = (36 read + 18 + 324 + 1 written) x 8 = 3032, and the rate next
    to the 6.3 TB/s of a device copy;
  * one Newton step of a clamped strip (--newton elements per direction, p = 2) with the device law and with
    ``device_law=False``: jets, the law on those jets (timed by itself, not as a difference), residual load, tangent
    (transform and assembly).

Alternating repeats in one process after a warm-up round; medians, spread = max - min.

    python tools/jet_bench.py [--sizes 128,256,512] [--degrees 2,3] [--reps 5] [--newton 64] [--out profiles/jet_bench.jsonl]
                              [--resources NEW.txt --parent-resources PARENT.txt [--resources-only]]

``--resources`` / ``--parent-resources``: the remarks of ``hipcc -Rpass-analysis=kernel-resource-usage`` for csrc/tg_postproc.hip,
csrc/tg_coef.hip, csrc/tg_assemble.hip, csrc/tg_boundary.hip, csrc/tg_material.hip, csrc/tg_jet.hip and csrc/tg_shell.hip of this
tree and for the first five of the parent commit; the first JSON line then lists the new kernels and says whether the
existing ones kept their figures.
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

COPY_TBS = 6.3
LAW_BYTES = (36 + 18 + 324 + 1) * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--newton", type=int, default=64)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--parent-resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jet_bench.jsonl"))
    ap.add_argument("--resources-only", action="store_true", help="write the compiler's resource report alone (needs no GPU)")
    args = ap.parse_args()
    with open(args.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.resources and args.parent_resources:
            from rational_bench import resource_record
            emit(resource_record(args.resources, args.parent_resources))
        if args.resources_only:
            return
        measure(args, emit)


def measure(args, emit):
    import tigar_amd as t
    from tigar_amd import NURBS as N, device as dev, forms as F
    import jet_reference as JR
    import shell_reference as SR
    from rational_bench import capture_stderr, stats

    def wall(fn):
        dev.sync()
        t0 = time.perf_counter()
        r = fn()
        dev.sync()
        return (time.perf_counter() - t0) * 1e3, r

    def timed(fn):
        """(wall ms, element-kernel ms of the library's line)"""
        with capture_stderr() as cap:
            ms, out = wall(fn)
        del out
        found = re.findall(r"element kernels ([0-9.]+) ms \(([a-z-]+)\)", cap.text)
        return ms, sum(float(v) for v, _ in found)

    info = dev.device_info()
    mat = F.KirchhoffLoveSVK(SR.E_MOD, SR.NU, SR.THICKNESS)
    for p in [int(v) for v in args.degrees.split(",")]:
        for nel in [int(v) for v in args.sizes.split(",") if v]:
            uks = [np.linspace(0.0, 1.0, nel + 1)] * 2
            import postproc_reference as R
            X = R.lagrange_nodes(uks, p)
            wx, wy, w = JR._arc_homogeneous(X[0])
            dcp = [dev.DeviceVector(data=np.ascontiguousarray(c)) for c in (wx, wy, w * 1.5 * X[1], w)]
            npts = dev.quad_count(uks, p + 1)
            rng = np.random.default_rng(p + nel)
            Tq = dev.DeviceVector(data=rng.standard_normal(36 * npts))
            coef_jet = dev.jet_transform(uks, p, dcp, Tq, 1, rational=True)
            A = dev.DeviceVector(data=rng.standard_normal(9 * npts))
            b = dev.DeviceVector(data=rng.standard_normal(3 * npts))
            coef_c = dev.coef_transform(uks, p, dcp, A, b, b, None, a_kind=2, rational=True)
            Xj = dev.quad_geometry_jet(uks, p, dcp)
            Uj = dev.DeviceVector(data=1e-3 * rng.standard_normal(18 * npts))
            del Tq, A, b
            rows = {k: [] for k in ("jet_wall", "jet_kernel", "coef_wall", "coef_kernel", "law")}
            os.environ["TIGAR_ASM_TIME"] = "1"
            for rep in range(args.reps + 1):                   # (round 0 warms up)
                jw, jk = timed(lambda: dev.assemble_jet_blocks(uks, p, dcp, coef_jet, 1))
                gc.collect()
                cw, ck = timed(lambda: dev.assemble_coef_matrix(uks, p, dcp, coef_c))
                gc.collect()
                lw, out = wall(lambda: dev.shell_points(0, mat.E, mat.nu, mat.thickness, Xj, Uj, True, True, True))
                del out
                gc.collect()
                if rep:
                    for k, v in zip(rows, (jw, jk, cw, ck, lw)):
                        rows[k].append(v)
            os.environ.pop("TIGAR_ASM_TIME", None)
            rec = {"record": "second-derivative point kernels", "device": info["name"], "p": p, "nel": nel, "points": npts,
                   "fe_nodes": dcp[0].size(), "reps": args.reps, "matrix_one_block": {k: stats(v) for k, v in rows.items() if k != "law"},
                   "law": dict(stats(rows["law"]), bytes_per_point=LAW_BYTES,
                               tb_per_s=round(LAW_BYTES * npts / (np.median(rows["law"]) * 1e-3) / 1e12, 3),
                               of_copy_rate=round(LAW_BYTES * npts / (np.median(rows["law"]) * 1e-3) / 1e12 / COPY_TBS, 3))}
            rec["ratios"] = {"jet_to_coef_element_kernels": round(np.median(rows["jet_kernel"]) / np.median(rows["coef_kernel"]), 3),
                             "jet_to_coef_wall": round(np.median(rows["jet_wall"]) / np.median(rows["coef_wall"]), 3)}
            emit(rec)
            del coef_jet, coef_c, Xj, Uj, dcp
            gc.collect()
    if args.newton:
        p, nel = 2, args.newton
        pb = SR.problem(p, (nel, nel), SR.cylinder_homogeneous(), clamp=(1, 0, 2))
        gen = t.EqualOrderSpline(3, N.NURBSControlMesh([p, p], pb["kvs"], pb["C"]))
        spline = t.ExtractedSpline(gen, 2 * p)
        V = spline.V
        u = t.Function(V)
        u.vector().set_local(1e-3 * np.random.default_rng(0).standard_normal(V.dim()))
        out = {}
        for name, flag in (("device_law", True), ("host_law", False)):
            res = F.ShellResidual(u, spline, mat, rational=True, device_law=flag)
            parts = {k: [] for k in ("jets", "law", "residual_load", "tangent")}
            compute_jets = res.jets
            for rep in range(args.reps + 1):
                res.jets = compute_jets
                ms_j, state = wall(lambda: res.jets(V))
                res.jets = lambda V_, state=state: state            # the law alone, on the jets just computed
                ms_l, (pts, g, s, Tq, _) = wall(lambda: res.law(V, load=True, tangent=True))
                ms_r, r = wall(lambda: F.VectorJetLoadForm(s, spline, rational=True).assemble_vector(V))
                form = F.VectorJetCoefficientForm(spline, Tq, rational=True)
                form._symmetric_hint = True
                ms_t, K = wall(lambda: form.assemble_matrix(V))
                del s, Tq, r, K, form
                gc.collect()
                if rep:
                    for k, v in zip(parts, (ms_j, ms_l, ms_r, ms_t)):
                        parts[k].append(v)
            recp = {k: stats(v) for k, v in parts.items()}
            out[name] = {"parts": recp, "assembly_ms": round(sum(v["median_ms"] for v in recp.values()), 3)}
        emit({"record": "newton step assembly", "device": info["name"], "problem": "clamped quarter-cylinder strip, p = 2, rational",
              "nel": nel, "points": pts.npts, "reps": args.reps, **out})


if __name__ == "__main__":
    main()
