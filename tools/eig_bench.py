"""Block kernels and LOBPCG eigensolves (csrc/tg_eig.hip, tigar_amd/eigen.py) on the 3-D p = 3 Laplace K of a 64^3 patch,
all faces Dirichlet.  One JSON line per case:

  (a) tg_spmm at k in {1, 4, 8, 16, 32, 64} against k calls of tg_spmv on the same K; tg_block_gram at the same widths.
      GB/s = (12 nnz + 16 n k) bytes / time for the products, 16 n k / time for the Gram (X and Y read once).
  (b) SLEPcEigenSolver, 10 smallest pairs, "jacobi" against "fast_diagonalization": iterations, seconds, time split.

usage: python tools/eig_bench.py [--nel 64] [--p 3] [--reps 20] [--pairs 10] [--out profiles/eig_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps, dev):
    fn()
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nel", type=int, default=64)
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--widths", default="1,4,8,16,32,64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-solve", action="store_true")
    a = ap.parse_args()

    import tigar_amd as t
    from tigar_amd import BSplines as Bs, forms as F, device as dev

    d, p, nel = 3, a.p, a.nel
    gen = t.EqualOrderSpline(1, Bs.ExplicitBSplineControlMesh([p] * d, [Bs.uniformKnots(p, 0.0, 1.0, nel)] * d))
    sc = gen.getScalarSpline(0)
    for direction in range(d):
        for side in (0, 1):
            gen.addZeroDofs(0, sc.getSideDofs(direction, side))
    spline = t.ExtractedSpline(gen, 2 * p)
    t0 = time.perf_counter()
    K = spline.assembleMatrix(F.LaplaceForm(), diag=1.0 / t.DOLFIN_EPS)      # (the demo's zero-dof diagonal)
    Mb = spline.assembleMatrix(F.MassForm())
    dev.sync()
    t_asm = time.perf_counter() - t0
    n, nnz = K.shape[0], K.nnz
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rng = np.random.default_rng(0)
    for k in [int(s) for s in a.widths.split(",")]:
        X = dev.DeviceBlock(n, k, data=rng.standard_normal((n, k)))
        Y = dev.DeviceBlock(n, k, zero=False)
        t_mm = _timed(lambda: K.mult_block(X, Y), a.reps, dev)
        xs = [X.get_column(j) for j in range(k)]
        ys = [dev.DeviceVector(n, zero=False) for _ in range(k)]

        def spmvs():
            for j in range(k):
                K.mult(xs[j], ys[j])
        t_mv = _timed(spmvs, max(1, a.reps // max(1, k // 4)), dev)
        ok = all(np.allclose(Y.get_column(j).get_local(), ys[j].get_local(), rtol=1e-13, atol=1e-13 * 1e3)
                 for j in (0, k - 1))
        t_g = _timed(lambda: dev.block_gram(X, Y), a.reps, dev)
        bytes_mm = 12.0 * nnz + 16.0 * n * k
        emit({"case": "kernels", "nel": nel, "p": p, "n": n, "nnz": nnz, "k": k,
              "spmm_ms": 1e3 * t_mm, "spmm_GBps": bytes_mm / t_mm / 1e9,
              "spmv_x_k_ms": 1e3 * t_mv, "spmv_x_k_GBps": k * (12.0 * nnz + 16.0 * n) / t_mv / 1e9,
              "spmm_over_spmv_x_k": t_mm / t_mv, "columns_agree": bool(ok),
              "gram_ms": 1e3 * t_g, "gram_GBps": 16.0 * n * k / t_g / 1e9})
        del X, Y, xs, ys

    if not a.skip_solve:
        for pc in ("fast_diagonalization", "jacobi"):
            s = t.SLEPcEigenSolver(K, Mb)
            s.parameters["preconditioner"] = pc
            s.parameters["maximum_iterations"] = 3000
            s.parameters["error_on_nonconvergence"] = False
            t0 = time.perf_counter()
            nc = s.solve(a.pairs)
            sec = time.perf_counter() - t0
            lam = [s.get_eigenvalue(i)[0] for i in range(a.pairs)]
            emit({"case": "solve", "nel": nel, "p": p, "n": n, "pairs": a.pairs, "preconditioner": pc,
                  "converged": nc, "iterations": s.last["iterations"], "block_size": s.last["block_size"],
                  "seconds": sec, "split_seconds": s.last["seconds"], "max_residual": max(s.last["residuals"]),
                  "lambda_over_pi2": [v / np.pi ** 2 for v in lam], "assembly_seconds": t_asm})
    if out:
        out.close()


if __name__ == "__main__":
    main()
