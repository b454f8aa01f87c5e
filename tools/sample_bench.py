"""Cost of evaluation at caller-chosen points, of the lattice entry points and of the closest-point iteration (csrc/tg_sample.hip,
the lattice entries of csrc/tg_postproc.hip) next to their yardstick, the sum-factorised evaluation at the Gauss points
(developer tool / profile source).

``rational_volume`` of tests/geom_util.py with nel^3 elements, p = 2 and 3:

  * ``tg_lattice_eval`` at m = p + 1 equispaced abscissae next to ``tg_quad_eval`` at nq = p + 1: the same kernel with another
    table (the lattice call builds and uploads its table and the Gauss call keeps its own in a cache);
  * ``tg_point_eval`` at the parametric coordinates of the Gauss points in element-major order and at the same points shuffled,
    values alone and with the gradient, nF = 1 and 4 -- next to ``tg_quad_eval`` on the same point set, once per field;
  * ``tg_point_locate`` for --locate round-trip points x = F(xi), from the seed search (all elements up to 32768 seeds) and
    from a guess (the centre of the point's element, which is what the search finds): the difference is the search.

Every figure is the WALL TIME OF THE CALL in milliseconds, ended by a device synchronise; it includes the allocation of the
outputs from the library's pool.  Alternating repeats in one process after a warm-up round; medians, spread = max - min.
Bytes: the unavoidable traffic of the scattered kernel is xi in and the outputs out plus the nodal fields once,
(d + nF (1 + nsd [with the gradient])) 8 npts + (nsd + 1 + nF) 8 nnodes; the rate is set next to the 6.3 TB/s of a device copy.

    python tools/sample_bench.py [--sizes 32,48,64] [--degrees 2,3] [--reps 5] [--locate 262144] [--out profiles/sample_bench.jsonl]
                                 [--resources NEW.txt --parent-resources PARENT.txt [--resources-only]]

``--resources`` / ``--parent-resources``: the remarks of ``hipcc -Rpass-analysis=kernel-resource-usage`` for csrc/tg_sample.hip,
csrc/tg_postproc.hip, csrc/tg_assemble.hip, csrc/tg_boundary.hip and csrc/tg_coef.hip of this tree and for the last four of the
parent commit; the first JSON line then lists the new kernels and says whether the existing ones kept their figures.
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
from tigar_amd import NURBS as N, device as dev  # noqa: E402
from tigar_amd import common as tc  # noqa: E402
from geom_util import rational_volume  # noqa: E402
from rational_bench import resource_record, stats  # noqa: E402

COPY_TBS = 6.3


def wall(fn):
    dev.sync()
    t0 = time.perf_counter()
    r = fn()
    dev.sync()
    return (time.perf_counter() - t0) * 1e3, r


def gauss_xi(uks, nq):
    """the knot coordinates of the Gauss points, numbered as tg_quad_points: [3, npts]"""
    g = (np.polynomial.legendre.leggauss(nq)[0] + 1.0) / 2.0
    ax = [u[:-1, None] + np.diff(u)[:, None] * g[None, :] for u in uks]                    # [nel, nq]
    nel = [len(u) - 1 for u in uks]
    shape = (nel[2], nel[1], nel[0], nq, nq, nq)
    out = np.empty((3, int(np.prod(shape))))
    out[0] = np.broadcast_to(ax[0][None, None, :, None, None, :], shape).ravel()
    out[1] = np.broadcast_to(ax[1][None, :, None, None, :, None], shape).ravel()
    out[2] = np.broadcast_to(ax[2][:, None, None, :, None, None], shape).ravel()
    return out


def run(p, nel, reps, nlocate):
    nsd = d = 3
    kvs, C = rational_volume(p, (nel,) * 3)
    gen = t.EqualOrderSpline(tc.selfcomm, 1, N.NURBSControlMesh([p] * 3, kvs, C))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k]) for k in range(3)]
    dcp = [f.vector() for f in gen.cpFuncs]
    n = dcp[0].size()
    nq = p + 1
    npts = dev.quad_count(uks, nq)
    rng = np.random.default_rng(p * 100 + nel)
    u4 = dev.DeviceVector(data=rng.standard_normal(4 * n))
    u1 = dev.DeviceVector(n, zero=False)
    dev.vec_copy_range(u1, 0, u4, 0, n)
    tl = np.linspace(0.0, 1.0, nq)
    xi_h = gauss_xi(uks, nq)
    xi = {"ordered": dev.DeviceVector(data=xi_h.ravel()), "shuffled": dev.DeviceVector(data=xi_h[:, rng.permutation(npts)].ravel())}
    del xi_h
    calls = {"quad_eval": lambda: dev.quad_eval(uks, p, dcp, u1), "quad_eval_grad": lambda: dev.quad_eval(uks, p, dcp, u1, grad=True),
             "lattice_eval": lambda: dev.lattice_eval(uks, p, dcp, tl, u1),
             "lattice_eval_grad": lambda: dev.lattice_eval(uks, p, dcp, tl, u1, grad=True)}
    for order in xi:
        for nF, uu in ((1, u1), (4, u4)):
            for grad in (False, True):
                calls["point_eval_%s_nF%d%s" % (order, nF, "_grad" if grad else "")] = \
                    (lambda o=order, f=nF, v=uu, gr=grad: dev.point_eval(uks, p, dcp, xi[o], v, nF=f, grad=gr))
    times = {k: [] for k in calls}
    for rep in range(reps + 1):                              # (round 0 warms up)
        for k, fn in calls.items():
            ms, out = wall(fn)
            del out
            gc.collect()
            if rep:
                times[k].append(ms)
    rec = {"record": "evaluation", "figures": "wall time of the call, ms", "p": p, "nel": nel, "points": npts, "fe_nodes": n, "reps": reps,
           "calls": {k: stats(v) for k, v in times.items()}}
    med = {k: v["median_ms"] for k, v in rec["calls"].items()}
    spr = {k: v["spread_ms"] for k, v in rec["calls"].items()}
    rec["ratios"] = {"lattice_eval_to_quad_eval": round(med["lattice_eval"] / med["quad_eval"], 3),
                     "lattice_eval_within_spread_of_quad_eval": bool(abs(med["lattice_eval"] - med["quad_eval"]) <= spr["lattice_eval"] + spr["quad_eval"]),
                     "lattice_eval_grad_to_quad_eval_grad": round(med["lattice_eval_grad"] / med["quad_eval_grad"], 3)}
    for order in xi:
        for nF in (1, 4):
            for grad in (False, True):
                k = "point_eval_%s_nF%d%s" % (order, nF, "_grad" if grad else "")
                yard = nF * med["quad_eval_grad" if grad else "quad_eval"]           # the yardstick takes one call per field
                nbytes = (d + nF * (1 + (nsd if grad else 0))) * 8 * npts + (nsd + 1 + nF) * 8 * n
                rec["ratios"][k] = {"to_quad_eval_per_field": round(med[k] / yard, 3), "floor_bytes": nbytes,
                                    "tb_per_s": round(nbytes / (med[k] * 1e-3) / 1e12, 3),
                                    "of_copy_rate": round(nbytes / (med[k] * 1e-3) / 1e12 / COPY_TBS, 3)}
    del xi
    gc.collect()
    # closest points: round trips
    xi0 = np.stack([rng.uniform(uu[0], uu[-1], nlocate) for uu in uks])
    x = dev.point_eval(uks, p, dcp, dev.DeviceVector(data=xi0.ravel()), x=True)[0]
    centre = np.stack([0.5 * (uks[k][np.searchsorted(uks[k], xi0[k], side="right").clip(1, len(uks[k]) - 1) - 1]
                              + uks[k][np.searchsorted(uks[k], xi0[k], side="right").clip(1, len(uks[k]) - 1)]) for k in range(3)])
    guess = dev.DeviceVector(data=centre.ravel())
    lt = {"search_and_iterations": [], "iterations_from_the_element_centre": []}
    for rep in range(reps + 1):
        for k, gs in (("search_and_iterations", None), ("iterations_from_the_element_centre", guess)):
            ms, (xo, info) = wall(lambda: dev.point_locate(uks, p, dcp, x, gs, tol=1e-12, max_iter=50))
            if rep:
                lt[k].append(ms)
            else:
                h = info.get_local().reshape(3, nlocate)
                err = float(np.max(np.abs(xo.get_local().reshape(3, nlocate) - xi0)))
                check = {"max_iterations": int(h[1].max()), "all_converged": bool(np.all(h[2] == 0)), "max_xi_error": err}
                rec.setdefault("locate_check", {})[k] = check
            del xo, info
            gc.collect()
    rec["locate"] = {"points": nlocate, "max_seeds": 32768,
                     **{k: stats(v) for k, v in lt.items()}}
    a, b = rec["locate"]["search_and_iterations"], rec["locate"]["iterations_from_the_element_centre"]
    # (a difference of two call times: it holds the seed-centre kernel, the evaluation of the centres and an allocation as well;
    # its spread is the sum of the two spreads)
    rec["locate"]["seed_search_ms_by_difference"] = round(a["median_ms"] - b["median_ms"], 4)
    rec["locate"]["seed_search_spread_ms"] = round(a["spread_ms"] + b["spread_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,48,64")
    ap.add_argument("--degrees", default="2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--locate", type=int, default=262144)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--parent-resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.jsonl"))
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
                emit(run(p, nel, args.reps, args.locate))


if __name__ == "__main__":
    main()
