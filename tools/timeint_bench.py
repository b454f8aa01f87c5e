"""The kernels of a time step against their composition from the older entry points (developer tool / profile source).

Unmapped 3-D p = 3 wave equation, all faces clamped, at 32^3, 48^3 and 64^3 elements (64^3: 300 763 dofs).  In one process,
warmed up, alternating, every sample = ``--inner`` calls ended by one device synchronise:

  (a) ``tg_spmv_pair`` (y = y0 - M xa - K xb) against two ``tg_spmv``, a copy of y0 and two ``tg_vec_axpy``;
  (b) ``tg_state_advance`` against 2 fills, 7 ``tg_vec_axpy`` and 4 copies (temporaries for x, the new velocity and the new
      acceleration, as tIGAr/timeIntegration.py:228-247 makes them, then the three assignments);
  (c) a step of ``LinearTransientProblem`` (generalized-alpha, RHO_INF = 0.5, DELTA_T = 1 / nel) under Jacobi-CG and under
      FD-CG: seconds of the rhs, solve and advance phases and iterations, with the fused right-hand side and with the two
      products.

    python tools/timeint_bench.py [--sizes 32,48,64] [--reps 5] [--inner 20] [--out profiles/timeint_bench.jsonl]

One JSON line per size is appended: times in ms per call (median of the repeats, spread = max - min), the bytes/s of the pair
kernel on its 20 B per stored entry and the share of the 6.3 TB/s of a streaming copy, and the check that both ways give the
same vectors up to rounding.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tigar_amd as t  # noqa: E402
from tigar_amd import BSplines as B, device as dev, forms as F, timeIntegration as TI  # noqa: E402

COPY_RATE = 6.3e12          # bytes/s of a streaming copy on the MI355X (float4 copy, measured)


def timed(fn, inner):
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) * 1e3 / inner


def stats(ts):
    return {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "all_ms": [round(v, 4) for v in ts]}


def alternate(f, g, reps, inner):
    f(), g()                                                    # (warm-up)
    tf, tg = [], []
    for _ in range(reps):
        tf.append(timed(f, inner))
        tg.append(timed(g, inner))
    return stats(tf), stats(tg)


def step_shares(spline, solver, dt, x0, v0, fused, steps):
    spline.setSolverOptions(linearSolver=solver)
    prob = TI.LinearTransientProblem(spline, stiffness=F.LaplaceForm(), mass=F.MassForm(), order=2, RHO_INF=0.5, DELTA_T=dt,
                                     x0=x0, xdot0=v0)
    prob.FUSED_RHS = fused
    prob.step(2)                                                # (warm-up: plans, preconditioner setup)
    rows = []
    for _ in range(steps):
        prob.step()
        rows.append(prob.last)
    out = {k: float(np.median([r[k] for r in rows])) * 1e3 for k in ("rhs_seconds", "solve_seconds", "advance_seconds")}
    out = {k.replace("_seconds", "_ms"): v for k, v in out.items()}
    total = sum(out.values())
    out.update({"iterations": [int(r["iterations"]) for r in rows], "rhs_share": out["rhs_ms"] / total,
                "solve_share": out["solve_ms"] / total, "advance_share": out["advance_ms"] / total,
                "rhs_spread_ms": float(np.ptp([r["rhs_seconds"] for r in rows])) * 1e3,
                "solve_spread_ms": float(np.ptp([r["solve_seconds"] for r in rows])) * 1e3})
    return out


def run(nel, reps, inner, steps, seed=0):
    p, d = 3, 3
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * d, [B.uniformKnots(p, 0.0, 1.0, nel)] * d))
    s0 = gen.getScalarSpline(0)
    for k in range(d):
        for side in (0, 1):
            gen.addZeroDofs(0, s0.getSideDofs(k, side))
    spline = t.ExtractedSpline(gen, 2 * p)
    K, M = spline.assembleMatrix(F.LaplaceForm()), spline.assembleMatrix(F.MassForm())
    n, nnz = K.shape[0], K.nnz
    rng = np.random.default_rng(seed)
    vec = lambda scale=1.0: dev.DeviceVector(data=rng.standard_normal(n) * scale)
    rec = {"nel": nel, "p": p, "dofs": n, "entries": nnz, "reps": reps, "inner": inner}

    # (a) the pair product
    pair = dev.CSRPair(M, K)
    xa, xb, y0 = vec(), vec(), vec()
    y_pair, y_two, tmp = dev.DeviceVector(n), dev.DeviceVector(n), dev.DeviceVector(n)

    def fused():
        pair.mult(xa, xb, y0=y0, y=y_pair)

    def composed():
        y_two[:] = y0
        M.mult(xa, tmp)
        y_two.axpy(-1.0, tmp)
        K.mult(xb, tmp)
        y_two.axpy(-1.0, tmp)

    a, b = alternate(fused, composed, reps, inner)
    ya, yb = y_pair.get_local(), y_two.get_local()
    rec["spmv_pair"] = {"tg_spmv_pair": a, "two_tg_spmv_copy_two_axpy": b, "speedup": b["median_ms"] / a["median_ms"],
                        "difference_exceeds_spread": bool(b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"])),
                        "bytes_per_s_on_20B_per_entry": 20.0 * nnz / (a["median_ms"] * 1e-3),
                        "share_of_copy_rate": 20.0 * nnz / (a["median_ms"] * 1e-3) / COPY_RATE,
                        "max_relative_difference": float(np.max(np.abs(ya - yb)) / np.max(np.abs(yb)))}
    ms, ks = alternate(lambda: M.mult(xa, tmp), lambda: K.mult(xb, tmp), reps, inner)
    rec["tg_spmv"] = {"M": ms, "K": ks}

    # (b) the state update
    c = np.array([2e4, -2e4, -0.9, 1e-4, 0.12, -0.12, -0.2])
    state = [vec(), vec(), vec(30.0), vec(900.0)]
    s_f = [v.copy() for v in state]
    s_c = [v.copy() for v in state]
    tx, tv, ta = dev.DeviceVector(n), dev.DeviceVector(n), dev.DeviceVector(n)

    def adv_fused():
        dev.state_advance(c, *s_f)

    def adv_composed():
        x, xo, vo, ao = s_c
        tx[:] = x
        tv.zero()
        for ci, w in zip(c[:4], (x, xo, vo, ao)):
            tv.axpy(ci, w)
        ta.zero()
        for ci, w in zip(c[4:], (tv, vo, ao)):
            ta.axpy(ci, w)
        xo[:] = tx
        vo[:] = tv
        ao[:] = ta

    # (one application each from the same state for the check; the timed repeats then iterate on their own copies, c[0] = -c[1]
    #  and x fixed keep the values bounded)
    adv_fused(), adv_composed()
    diff = max(float(np.max(np.abs(p_.get_local() - q_.get_local())) / np.max(np.abs(q_.get_local())))
               for p_, q_ in zip(s_f[1:], s_c[1:]))
    for dst, src in zip(s_f + s_c, state + state):
        dst[:] = src
    a, b = alternate(adv_fused, adv_composed, reps, inner)
    rec["state_advance"] = {"tg_state_advance": a, "2_fills_7_axpy_4_copies": b, "speedup": b["median_ms"] / a["median_ms"],
                            "bytes_per_s_on_7_vectors": 56.0 * n / (a["median_ms"] * 1e-3),
                            "max_relative_difference": diff}

    # (c) shares of a step
    dt = 1.0 / nel
    x0 = rng.standard_normal(n)
    x0[np.asarray(spline.zeroDofs, dtype=np.int64)] = 0.0
    x0d, v0d = dev.DeviceVector(data=x0), dev.DeviceVector(n)
    rec["step"] = {"DELTA_T": dt, "relative_tolerance": 1e-8}
    for name in ("jacobi", "fast_diagonalization"):
        for fused_rhs in (True, False):
            solver = t.PETScKrylovSolver("cg", name)
            solver.parameters["relative_tolerance"] = 1e-8
            rec["step"]["%s_%s" % (name, "pair" if fused_rhs else "two_products")] = \
                step_shares(spline, solver, dt, x0d, v0d, fused_rhs, steps)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,48,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "timeint_bench.jsonl"))
    args = ap.parse_args()
    info = dev.device_info()
    with open(args.out, "a") as f:
        for nel in [int(v) for v in args.sizes.split(",")]:
            rec = run(nel, args.reps, args.inner, args.steps)
            rec["device"] = info["name"]
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
