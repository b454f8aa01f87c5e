"""Bringing an FE matrix from the caller's dof order to the order of the node grid (developer tool / profile source).

3-D p = 3 Laplace matrices from ``forms`` at 32^3, 48^3 and 64^3 elements (64^3: 7 189 057 rows, 887 503 681 entries), handed in
in two caller orders: a seeded random permutation of the rows, and a blocked one (cells of 4^3 nodes shuffled, the nodes of a
cell kept together: the locality the numbering of an FE library has).  Alternating in one process, warmed up, every call
ended by a device synchronise:

  (a) ``DeviceCSR.gather_rows`` + ``DeviceCSR.permute_columns`` (two copies of A and a sort pass),
  (b) ``FEOrder.permute_matrix`` (tg_csr_permute_sym: one pass, rows sorted on chip),
  (c) for scale, the ``extractMatrix`` that follows on the grid-ordered matrix.

    python tools/fe_order_bench.py [--sizes 32,48,64] [--reps 5] [--out profiles/fe_order_bench.jsonl]

One JSON line per size: times in ms (median, and the spread max - min over the repeats), bytes/s of (b) on the floor
2 x (12 nnz + 8 nrows) bytes (A read once and written once) and its share of the 6.3 TB/s a streaming copy reaches, and the
check that (a) and (b) return the grid-ordered matrix (row pointers, and the product with a random vector bit for bit).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tigar_amd as t  # noqa: E402
from tigar_amd import BSplines as B, device as dev, forms as F  # noqa: E402
from tigar_amd.feorder import FEOrder  # noqa: E402

COPY_RATE = 6.3e12          # bytes/s of a streaming copy on the MI355X (float4 copy, measured)


def blocked_permutation(shape, cell, rng):
    """grid_of_fe of an order that walks shuffled cells of ``cell``^3 nodes, lexicographic inside a cell"""
    nx, ny, nz = shape
    ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    ix, iy, iz = (a.ravel(order="F") for a in (ix, iy, iz))                      # direction 0 fastest: the grid order
    cx, cy, cz = -(-nx // cell), -(-ny // cell), -(-nz // cell)
    cid = (ix // cell) + cx * ((iy // cell) + cy * (iz // cell))
    rank = rng.permutation(cx * cy * cz)
    local = (ix % cell) + cell * ((iy % cell) + cell * (iz % cell))
    return np.argsort(rank[cid] * cell ** 3 + local, kind="stable")


def timed(fn):
    dev.sync()
    t0 = time.perf_counter()
    out = fn()
    dev.sync()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ts):
    return {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "all_ms": [round(v, 3) for v in ts]}


def same_matrix(X, Y, x):
    if X.shape != Y.shape or X.nnz != Y.nnz:
        return False
    return bool(np.array_equal(X.mult(x).get_local().view(np.int64), Y.mult(x).get_local().view(np.int64)))


def run(nel, reps, seed=0):
    p, d = 3, 3
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * d, [B.uniformKnots(p, 0.0, 1.0, nel)] * d))
    s0 = gen.getScalarSpline(0)
    for k in range(d):
        for side in (0, 1):
            gen.addZeroDofs(0, s0.getSideDofs(k, side))
    spline = t.ExtractedSpline(gen, 2 * p)
    A = F.LaplaceForm().assemble_matrix(spline.V)
    n, nnz = A.shape[0], A.nnz
    floor = 2 * (12 * nnz + 8 * n)
    rng = np.random.default_rng(seed)
    x = dev.DeviceVector(data=rng.standard_normal(n))
    shape = spline.V.grids[0].shape()
    rec = {"nel": nel, "p": p, "rows": n, "entries": nnz, "floor_bytes": floor, "reps": reps}
    X = spline.V.tabulate_dof_coordinates()
    for kind in ("random", "blocked"):
        g = rng.permutation(n) if kind == "random" else blocked_permutation(shape, 4, rng)
        t_loc, order = timed(lambda: FEOrder.locate([spline.V.grids[0].axes], X[g]))
        assert np.array_equal(order.grid_of_fe, g)
        inv = order.fe_of_grid.astype(np.int64)
        Ac = order.permute_matrix(A, inverse=True)             # A as the caller would hand it in
        old = lambda: Ac.gather_rows(inv).permute_columns(g)
        new = lambda: order.permute_matrix(Ac)
        ok_a, ok_b = same_matrix(old(), A, x), same_matrix(new(), A, x)        # (warm-up and check)
        ta, tb = [], []
        for _ in range(reps):
            ta.append(timed(old)[0])
            tb.append(timed(new)[0])
        a, b = stats(ta), stats(tb)
        rec[kind] = {"locate_ms": round(t_loc, 3), "gather_rows+permute_columns": a, "tg_csr_permute_sym": b,
                     "speedup": a["median_ms"] / b["median_ms"],
                     "bytes_per_s": floor / (b["median_ms"] * 1e-3),
                     "share_of_copy_rate": floor / (b["median_ms"] * 1e-3) / COPY_RATE,
                     "results_equal_grid_matrix": [ok_a, ok_b]}
        del Ac, order
    spline.extractMatrix(A)                                    # (plans)
    tc = [timed(lambda: spline.extractMatrix(A))[0] for _ in range(max(2, reps // 2))]
    rec["extractMatrix"] = stats(tc)
    for kind in ("random", "blocked"):
        rec[kind]["share_of_extractMatrix"] = rec[kind]["tg_csr_permute_sym"]["median_ms"] / rec["extractMatrix"]["median_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,48,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "fe_order_bench.jsonl"))
    args = ap.parse_args()
    info = dev.device_info()
    with open(args.out, "w") as f:
        for nel in [int(v) for v in args.sizes.split(",")]:
            rec = run(nel, args.reps)
            rec["device"] = info["name"]
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
