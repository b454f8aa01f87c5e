"""Time of the x, y and z stages of the Kronecker-form PtAP on the line kernels (developer tool): a 3-D patch streamed in
sub-slabs through ``SlabHotPath.assemble`` with the FE matrix materialised in row blocks and the tensor-pattern passes off
(``TIGAR_PTAP_TENSOR=0``), so that every stage goes through ``kronptap.contract`` -> ``device.ptap_kron`` (csrc/tg_ptap_box.hip).

    python tools/kron_stage_bench.py [p=3] [nel=96] [reps=2]

``device.ptap_kron`` is wrapped: the device is drained before and after every call, and the wall time of the call (host driver
+ reach scan + probe or cached capacity + kernel + ending) is booked on the contracted direction.  One warm-up assembly, then
`reps` timed ones.  Prints one JSON line: per direction the number of calls and the median / smallest call in ms, and the
median wall time of an assembly.
"""
import json
import os
import sys
import time

import numpy as np

os.environ["TIGAR_PTAP_TENSOR"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tigar_amd import device as dev, BSplines as B, forms as F  # noqa: E402
from tigar_amd.common import TensorFunctionSpace  # noqa: E402
from tigar_amd.dist import SlabHotPath  # noqa: E402


def main():
    p = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    nel = int(sys.argv[2]) if len(sys.argv) > 2 else 96
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    dev.device_info()
    basis = B.ExplicitBSplineControlMesh([p] * 3, [B.uniformKnots(p, 0., 1., nel)] * 3).getScalarSpline()
    grid = basis.generateMesh(degree=p)
    V = TensorFunctionSpace([grid], "Lagrange")
    lap = F.LaplaceForm()
    zd = basis.getSideDofs(2, 0) + basis.getSideDofs(2, 1)
    path = SlabHotPath(basis, grid)
    calls = {0: [], 1: [], 2: []}
    inner = dev.ptap_kron

    def timed(cur, cur_row0, dims_in, factors, *args, **kw):
        dev.sync()
        t0 = time.perf_counter()
        out = inner(cur, cur_row0, dims_in, factors, *args, **kw)
        dev.sync()
        k = [j for j, f in enumerate(factors) if f is not None]
        if len(k) == 1:
            calls[k[0]].append(time.perf_counter() - t0)
        return out
    dev.ptap_kron = timed
    walls = []
    for rep in range(reps + 1):
        for c in calls.values():
            if rep == 1:
                del c[:]                       # (drop the warm-up's calls)
        dev.sync()
        t0 = time.perf_counter()
        K, _ = path.assemble(lambda a, b: lap.assemble_matrix(V, a, b), None, zd, 1.0)
        dev.sync()
        walls.append(time.perf_counter() - t0)
        nnz = K.nnz
        del K
    out = {"workload": "3-D p=%d nel=%d, %d sub-slabs, line kernels (TIGAR_PTAP_TENSOR=0)" % (p, nel, len(path.sub_slabs())),
           "nnz_K": int(nnz), "assembly_ms_median": 1e3 * float(np.median(walls[1:]))}
    for k, name in enumerate("xyz"):
        out[name] = {"calls": len(calls[k]), "median_ms": 1e3 * float(np.median(calls[k])) if calls[k] else None,
                     "min_ms": 1e3 * float(np.min(calls[k])) if calls[k] else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
