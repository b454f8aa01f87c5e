"""Fast diagonalization preconditioner at cfg3's size (256^3 elements, p = 3, every face Dirichlet, one GPU): the unmapped
Poisson case and the mapped one (bench.py's rational volume map).  One JSON line per case: setup s, coefficient fit ms,
ms per FD application and its TFLOP/s (2 n_k flops per entry and pass over the padded box), FD-CG iterations and solve s,
Jacobi-CG iterations and solve s on the same K and b.

    python tools/fd_bench.py [--nel 256] [--p 3] [--rtol 1e-6] [--cases unmapped,mapped]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nel", type=int, default=256)
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--cases", default="unmapped,mapped")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import tigar_amd as t
    from tigar_amd import BSplines as B, forms as F
    from tigar_amd import device as dev
    from tigar_amd.device import DeviceVector
    from bench import rational_volume_mesh
    p, nel = args.p, args.nel
    for case in args.cases.split(","):
        mapped = case == "mapped"
        cm = rational_volume_mesh(p, nel) if mapped else B.ExplicitBSplineControlMesh([p] * 3, [B.uniformKnots(p, 0.0, 1.0, nel)] * 3)
        gen = t.EqualOrderSpline(1, cm)
        sc = gen.getScalarSpline(0)
        for direction in range(3):
            for side in (0, 1):
                gen.addZeroDofs(0, sc.getSideDofs(direction, side))
        spline = t.ExtractedSpline(gen, 2 * p)
        if mapped:
            K = spline.assembleMatrix(F.LaplaceForm(geometry=gen))
            b = spline.assembleVector(F.NodalLoadForm(1.0, gen))
        else:
            K = spline.assembleMatrix(F.LaplaceForm())
            b = spline.assembleVector(F.SeparableLoadForm([lambda x: np.sin(np.pi * x)] * 3, scale=3 * np.pi ** 2))
        rec = {"case": case, "nel": nel, "p": p, "dofs": K.shape[0], "rtol": args.rtol}
        for pc in ("fast_diagonalization", "jacobi"):
            solver = t.PETScKrylovSolver("cg", pc)
            solver.parameters["relative_tolerance"] = args.rtol
            x = DeviceVector(K.shape[0])
            dev.sync()
            t0 = time.perf_counter()
            solver.solve(K, x, b)
            dev.sync()
            ts = time.perf_counter() - t0
            key = "fd" if pc != "jacobi" else "jacobi"
            rec[key + "_iterations"] = solver.last["iterations"]
            rec[key + "_solve_s"] = ts
            if pc != "jacobi":
                rec["fd_setup_s"] = solver.last["fd"]["setup_seconds"]
                rec["fd_fit_ms"] = 1e3 * solver.last["fd"]["fit_seconds"]
                rec["fd_coefficients"] = solver.last["fd"]["coefficients"][0]
                # the same solve again: setup reused
                x2 = DeviceVector(K.shape[0])
                dev.sync()
                t0 = time.perf_counter()
                solver.solve(K, x2, b)
                dev.sync()
                rec["fd_solve_reused_s"] = time.perf_counter() - t0
        fd = t.FastDiagonalization(K)
        z = DeviceVector(K.shape[0])
        fd.apply(b, z)
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fd.apply(b, z)
        dev.sync()
        ms = 1e3 * (time.perf_counter() - t0) / args.reps
        st = fd._setup
        flops = 0.0
        for off, lo, hi, per in st.blocks:
            npad = [(h - l + 15) // 16 * 16 for l, h in zip(lo, hi)]
            box = float(np.prod(npad))
            flops += 2 * sum(2.0 * nk * box for nk in npad)
        rec["fd_apply_ms"] = ms
        rec["fd_apply_tflops"] = flops / (ms * 1e-3) / 1e12
        rec["fd_apply_flop"] = flops
        print(json.dumps(rec), flush=True)
        del K, b, spline, gen, fd


if __name__ == "__main__":
    main()
