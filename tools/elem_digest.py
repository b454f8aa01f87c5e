"""SHA-256 of the results of the element-split PtAP host driver (csrc/tg_elemsplit.hip: tg_elemplan_create / tg_elemplan_ptap)
-- developer tool: a change that is meant to leave the results bit for bit alone runs this file in both checkouts and compares
the two outputs line by line.

One JSON line per result: {"case", "pattern": sha256(row pointers | columns), "values": sha256(values), "nnz"}; a declined
product gives nulls.  Every case runs in a process of its own:
  shape    the shapes of ``test_element_split_product_matches_scipy`` (tests/test_gpu_elemsplit.py): first and second product
           and the product with zero dofs, with no switch set and with TIGAR_EL_MERGE=1 TIGAR_EL_VALU=1 TIGAR_EL_LISTS=1;
  chunk    the four cuts of ``test_chunks_of_cells_add_up_to_the_whole_product``: every chunk's K and the declined product of
           the matrix with a coupling outside the cells;
  star     the star meshes of that file: n = 40 twice, n = 70 (declined), n = 130 (no plan).
Inputs are seeded.

    python tools/elem_digest.py [--out profiles/elem_driver_digest.jsonl]
    python tools/elem_digest.py --compare A.jsonl B.jsonl
    python tools/kernel_trace.py --min-ms 0 -- python tools/elem_digest.py --in-process
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(3, 3, (5, 4, 6)), (3, 2, (7, 5, 6)), (2, 3, (17, 12)), (3, 1, (9, 8, 7)), (2, 2, (20, 15)), (3, 4, (3, 2, 4)), (2, 5, (7, 6)),
          (2, 7, (5, 4)), (3, 4, (5, 5, 3))]
CHUNKS = [(3, 2, (5, 4, 9), (0, 3, 4, 9)), (2, 3, (7, 12), (0, 5, 12)), (3, 3, (3, 3, 7), (0, 2, 5, 7)), (3, 1, (4, 4, 6), (0, 1, 2, 6))]
SWITCHES = {"TIGAR_EL_MERGE": "1", "TIGAR_EL_VALU": "1", "TIGAR_EL_LISTS": "1"}


def jobs():
    out = ["shape:%d:%d" % (i, s) for i in range(len(SHAPES)) for s in (0, 1)]
    out += ["chunk:%d" % i for i in range(len(CHUNKS))]
    out += ["star:40", "star:70", "star:130"]
    return out


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def emit(case, K):
    if K is None:
        print(json.dumps({"case": case, "pattern": None, "values": None, "nnz": None}), flush=True)
        return
    K = K.to_scipy().tocsr()
    K.sort_indices()
    rp, col = K.indptr.astype(np.int64), K.indices.astype(np.int64)
    print(json.dumps({"case": case, "pattern": sha(rp, col), "values": sha(K.data), "nnz": int(K.nnz)}), flush=True)


def noisy(A, rng):
    As = A.to_scipy().tocsr()
    As.sort_indices()
    As.data = As.data * (1.0 + 0.3 * rng.standard_normal(As.nnz)) + 0.01 * rng.standard_normal(As.nnz)
    return As


def run_shape(dev, job):
    import test_gpu_elemsplit as T
    from tigar_amd.elemptap import ElementSplitPtAP
    _, i, s = job.split(":")
    d, p, nels = SHAPES[int(i)]
    if int(s):
        os.environ.update(SWITCHES)
    A, M, cells = T._operands(d, p, nels)
    rng = np.random.default_rng(d * 10 + p)
    A2 = dev.DeviceCSR.from_scipy(noisy(A, rng))
    zd = np.unique(rng.integers(0, M.shape[1], 25)).astype(np.int32)
    name = "shape d=%d p=%d nels=%s switches=%s" % (d, p, "x".join(map(str, nels)), "set" if int(s) else "unset")
    plan = ElementSplitPtAP(M, cells)
    emit(name + " first", plan.ptap(A2))
    emit(name + " second", plan.ptap(A2))
    emit(name + " zero_dofs", plan.ptap(A2, zero_dofs=zd, diag=1.0))


def run_chunk(dev, job):
    import test_gpu_elemsplit as T
    from tigar_amd.elemptap import CellNodes, ElementChunk
    from tigar_amd.BSplines import ExplicitBSplineControlMesh, uniformKnots
    d, p, nels, cuts = CHUNKS[int(job.split(":")[1])]
    A, M, _ = T._operands(d, p, nels)
    As = noisy(A, np.random.default_rng(p + d))
    Ms = M.to_scipy().tocsr()
    grid = ExplicitBSplineControlMesh([p] * d, [uniformKnots(p, 0., 1., n) for n in nels]).getScalarSpline().generateMesh(degree=p)
    plane, per_layer = int(np.prod(grid.shape()[:-1])), int(np.prod(nels[:-1]))
    bad = As.tolil()
    bad[(cuts[1] * p) * plane + 1, As.shape[0] - 1] = 1.0
    bad = bad.tocsr()
    name = "chunk d=%d p=%d nels=%s" % (d, p, "x".join(map(str, nels)))
    for e0, e1 in zip(cuts[:-1], cuts[1:]):
        f0 = max(e0 - 1, 0)
        cells = CellNodes.from_grid(grid, [0] * (d - 1) + [f0], list(nels[:-1]) + [e1])
        r0, r1 = e0 * p * plane, (e1 * p + 1) * plane
        chunk = ElementChunk(cells, dev.DeviceCSR.from_scipy(Ms[r0:r1]), r0, own=((e0 - f0) * per_layer, (e1 - f0) * per_layer))
        chk = (r0, r1 if e1 == nels[-1] else e1 * p * plane)
        emit("%s layers %d..%d" % (name, e0, e1), chunk.ptap(dev.DeviceCSR.from_scipy(As[r0:r1]), r0, chk))
        emit("%s layers %d..%d coupling outside the cells" % (name, e0, e1), chunk.ptap(dev.DeviceCSR.from_scipy(bad[r0:r1]), r0, chk))


def run_star(dev, job):
    import test_gpu_elemsplit as T
    from tigar_amd.elemptap import CellNodes, ElementSplitPtAP
    n = int(job.split(":")[1])
    cells, Ms, As = T._star(n)
    try:
        plan = ElementSplitPtAP(dev.DeviceCSR.from_scipy(Ms), CellNodes.from_host(cells))
    except ValueError:
        return emit("star n=%d no plan" % n, None)
    A = dev.DeviceCSR.from_scipy(As)
    emit("star n=%d first" % n, plan.ptap(A))
    emit("star n=%d second" % n, plan.ptap(A))


def run_one(job):
    from tigar_amd import device as dev
    dev.device_info()
    {"shape": run_shape, "chunk": run_chunk, "star": run_star}[job.split(":")[0]](dev, job)


def compare(a, b):
    A = {r["case"]: r for r in map(json.loads, open(a))}
    B = {r["case"]: r for r in map(json.loads, open(b))}
    differ = 0
    for case in sorted(set(A) | set(B)):
        x, y = A.get(case), B.get(case)
        if x == y:
            continue
        differ += 1
        print("differs (%s): %s" % ("missing" if x is None or y is None else "PATTERN" if x["pattern"] != y["pattern"] else "values", case))
    print("elem_digest: %d of %d lines differ (%s against %s)" % (differ, len(set(A) | set(B)), a, b))
    return differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elem_driver_digest.jsonl"))
    ap.add_argument("--one", default=None, help="(internal) run this job in this process and print its lines")
    ap.add_argument("--in-process", action="store_true",
                    help="all cases in this process, lines to stdout (under tools/kernel_trace.py, which follows one process)")
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare[0], args.compare[1])
    if args.one:
        return run_one(args.one)
    if args.in_process:
        for job in jobs():
            saved = dict(os.environ)
            run_one(job)
            os.environ.clear()
            os.environ.update(saved)
        return
    lines = []
    for job in jobs():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", job], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             universal_newlines=True, timeout=300)
        if res.returncode != 0:          # (nothing more is started after a job that failed)
            sys.stderr.write(res.stderr[-2000:])
            raise SystemExit("elem_digest: job %s ended with %d" % (job, res.returncode))
        lines += [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("elem_digest: %d lines -> %s" % (len(lines), args.out))


if __name__ == "__main__":
    sys.exit(main())
