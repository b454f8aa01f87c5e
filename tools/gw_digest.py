"""SHA-256 of the results of the wave-per-row and cell-block PtAP host drivers (csrc/tg_ptap_wave.hip: tg_ptap_wave_plan /
tg_ptap_wave_numeric, tg_cellplan_ptap, tg_cellplan_ptap_extras, tg_foldplan_apply) -- developer tool: a change that is meant
to leave the results bit for bit alone runs this file in both checkouts and compares the two outputs line by line.

One JSON line per result: {"case", "pattern": sha256(row pointers | columns), "values": sha256(values), "nnz"}.  Every case
runs in a process of its own:
  lane     the lane-group grid of tests/test_gpu_ptap_wave.py (exact operands), fresh plan and placed rows, with and
           without zero dofs;
  retry    the inputs of tests/test_gpu_ptap_retry.py that overflow a table or a temporary (workgroup kernel, both wave
           stages, the decline, the cell-block gather), first and second product;
  cell     the shapes of ``test_cell_block_product_against_scipy``, first and second product, ``TIGAR_CELL_MERGE_HASH`` unset
           and set; ``lookup`` / ``large``: the cases of the look-up merge and the large-cell tests of that file;
  extras   the shapes of ``test_cell_blocks_plus_couplings_outside_the_blocks`` through ``ptap_extras`` (K and remainder);
  fold     ``test_extract_matrix_on_a_periodic_patch`` (nel 6, periodic in x): three products, the later ones by places.
Inputs are seeded.

    python tools/gw_digest.py [--out profiles/gw_driver_digest.jsonl] [--dump DIR]
    python tools/gw_digest.py --compare A.jsonl B.jsonl [--dumps DIR_A DIR_B]
    python tools/kernel_trace.py --min-ms 0 -- python tools/gw_digest.py --in-process
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

LANE_GROUPS = (3, 4, 5, 6)
CELLS = [(200, 16, 300, 9, 25), (333, 9, 150, 4, 16), (50, 27, 400, 27, 64), (64, 4, 40, 1, 8)]      # tests/test_gpu_cellptap.py
LOOKUP = [(64, 4, 40, 1, 8), (50, 27, 400, 27, 64)]
EXTRAS = [(300, 16, 260, 40), (500, 9, 200, 3), (120, 27, 350, 500)]
RETRY = ["hash", "hash-zd", "stage2", "decline", "stage1", "cells"]


def jobs():
    out = ["lane:%d:%d:%d" % (a, b, z) for a in LANE_GROUPS for b in LANE_GROUPS for z in (0, 1)]
    out += ["retry:" + r for r in RETRY]
    out += ["cell:%d:%d" % (i, h) for i in range(len(CELLS)) for h in (0, 1)]
    out += ["lookup:%d" % i for i in range(len(LOOKUP))] + ["large"]
    out += ["extras:%d" % i for i in range(len(EXTRAS))] + ["fold"]
    return out


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class Emit(object):
    def __init__(self, dump):
        self.dump = dump

    def __call__(self, case, K):
        if K is None:
            print(json.dumps({"case": case, "pattern": None, "values": None, "nnz": None}), flush=True)
            return
        K = K.to_scipy().tocsr() if hasattr(K, "to_scipy") else K.tocsr()
        K.sort_indices()
        rp, col = K.indptr.astype(np.int64), K.indices.astype(np.int64)
        if self.dump:
            np.savez(os.path.join(self.dump, case.replace("/", "_").replace(" ", "_") + ".npz"), indptr=rp, indices=col, data=K.data)
        print(json.dumps({"case": case, "pattern": sha(rp, col), "values": sha(K.data), "nnz": int(K.nnz)}), flush=True)


def twice(dev, emit, name, A, M, zd, diag):
    """a fresh plan, its product and a second product on the plan"""
    Ad, Md = dev.DeviceCSR.from_scipy(A), dev.DeviceCSR.from_scipy(M)
    MT = Md.transpose()
    plan = dev.ptap_symbolic(Ad, Md, MT)
    for which in ("first", "second"):
        emit("%s %s" % (name, which), dev.ptap_numeric(plan, Ad, Md, MT, zd, diag))


def run_lane(dev, job, emit):
    import ptap_wave_reference as R
    _, lg1, lg2, z = job.split(":")
    os.environ.update(TIGAR_PTAP_WAVE="1", TIGAR_PTAP_WAVE_LG1=lg1, TIGAR_PTAP_WAVE_LG2=lg2)
    M, A, info = R.lane_group_operands(R.exact_value_source(1))
    zd = R.lane_group_zero_dofs(R.structural(M, A)[0], info) if int(z) else None
    twice(dev, emit, "lane lg1=%s lg2=%s zero_dofs=%s" % (lg1, lg2, z), A, M, zd, 2.5 if int(z) else 1.0)


def run_retry(dev, job, emit):
    import test_gpu_ptap_retry as T
    which = job.split(":")[1]
    if which == "cells":
        from test_gpu_cellptap import _cells
        rng = np.random.default_rng(68)
        M, A = _cells(rng, 64, 4, 40, 1, 8)
        M = M.tolil()
        M[np.arange(0, 256, 4), 39] = rng.standard_normal(64)
        M = M.tocsr()
        M.sort_indices()
        return cell_twice(dev, emit, "retry cells", M, A, 4, np.array([2, 17], dtype=np.int32), 2.5)
    n, seed, wave, dense, extra, zd = {"hash": (2048, 1, "0", 2048, 0, None), "hash-zd": (2048, 1, "0", 2048, 0, [5, 1200]),
                                       "stage2": (2048, 2, "1", 160, 0, None), "decline": (2048, 1, "1", 2048, 0, None),
                                       "stage1": (8192, 4, "1", 0, 300, None)}[which]
    os.environ["TIGAR_PTAP_WAVE"] = wave
    rng = np.random.default_rng(seed)
    A, M = T.tridiagonal(n, rng, extra_row1=extra), T.banded_m(n, rng, dense_rows=dense)
    twice(dev, emit, "retry " + which, A, M, zd, 2.5 if zd else 1.0)


def cell_twice(dev, emit, name, M, A, b, zd, diag):
    from tigar_amd.cellptap import CellBlockPtAP
    Md, Ad = dev.DeviceCSR.from_scipy(M), dev.DeviceCSR.from_scipy(A)
    plan = CellBlockPtAP(Md, b)
    for which in ("first", "second"):
        emit("%s %s" % (name, which), plan.ptap(Ad, zd, diag))
    return plan


def run_cell(dev, job, emit):
    from test_gpu_cellptap import _cells
    parts = job.split(":")
    if parts[0] == "large":
        ncell, b, ncp, nf_lo, nf_hi = 6, 64, 100, 40, 64
    else:
        ncell, b, ncp, nf_lo, nf_hi = (CELLS if parts[0] == "cell" else LOOKUP)[int(parts[1])]
    if parts[0] == "lookup" or (parts[0] == "cell" and parts[2] == "1"):
        os.environ["TIGAR_CELL_MERGE_HASH"] = "1"
    rng = np.random.default_rng(ncell + b)
    M, A = _cells(rng, ncell, b, ncp, nf_lo, nf_hi)
    if parts[0] == "cell":
        zd = np.unique(rng.integers(0, ncp, size=7)).astype(np.int32)
    else:
        zd = np.unique(rng.choice(np.unique(M.indices), size=5 if parts[0] == "lookup" else 4)).astype(np.int32)
    name = "%s cells=%d b=%d ncp=%d nf=%d..%d merge_hash=%s" % (parts[0], ncell, b, ncp, nf_lo, nf_hi, os.environ.get("TIGAR_CELL_MERGE_HASH", "unset"))
    plan = cell_twice(dev, emit, name, M, A, b, zd, 2.5)
    if parts[0] == "large":
        import scipy.sparse as sp
        n = A.shape[0]
        r, c = np.array([0, 3, 70, 200, 383]), np.array([64, 130, 5, 10, 0])
        Ax = (A + sp.csr_matrix((rng.standard_normal(r.size), (r, c)), shape=(n, n))).tocsr()
        Ax.sort_indices()
        got = plan.ptap_extras(dev.DeviceCSR.from_scipy(Ax))
        emit(name + " extras", None if got is None else got[0])


def run_extras(dev, job, emit):
    import scipy.sparse as sp
    from test_gpu_cellptap import _cells
    from tigar_amd.cellptap import CellBlockPtAP
    ncell, b, ncp, nextra = EXTRAS[int(job.split(":")[1])]
    rng = np.random.default_rng(ncell + nextra)
    M, A = _cells(rng, ncell, b, ncp, 4, min(40, ncp // 3))
    n = A.shape[0]
    r, c = rng.integers(0, n, nextra), rng.integers(0, n, nextra)
    keep = (r // b) != (c // b)
    v = rng.standard_normal(nextra)
    v[0] = 1e9
    E = sp.csr_matrix((v[keep], (r[keep], c[keep])), shape=(n, n))
    E.sum_duplicates()
    Ax = (A + E).tocsr()
    Ax.sort_indices()
    plan, Ad = CellBlockPtAP(dev.DeviceCSR.from_scipy(M), b), dev.DeviceCSR.from_scipy(Ax)
    for which in ("first", "second"):
        K, R = plan.ptap_extras(Ad)
        emit("extras cells=%d b=%d extra=%d K %s" % (ncell, b, nextra, which), K)
        emit("extras cells=%d b=%d extra=%d remainder %s" % (ncell, b, nextra, which), R)


def run_fold(dev, emit):
    import tigar_amd as t
    from tigar_amd import BSplines as B, forms as F
    d, p, nel = 3, 2, 6
    kv = [B.uniformKnots(p, 0., 1., nel, k == 0) for k in range(d)]
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * d, kv))
    sp0 = gen.getScalarSpline(0)
    for direction in (1, 2):
        for side in (0, 1):
            gen.addZeroDofs(0, sp0.getSideDofs(direction, side))
    spline = t.ExtractedSpline(gen, 2 * p)
    A = F.LaplaceForm().assemble_matrix(spline.V)
    for which in ("first", "second", "third"):
        emit("fold periodic x nel=6 " + which, spline.extractMatrix(A, diag=1.5))


def run_one(job, dump):
    from tigar_amd import device as dev
    dev.device_info()
    emit = Emit(dump)
    kind = job.split(":")[0]
    if kind == "lane":
        run_lane(dev, job, emit)
    elif kind == "retry":
        run_retry(dev, job, emit)
    elif kind in ("cell", "lookup", "large"):
        run_cell(dev, job, emit)
    elif kind == "extras":
        run_extras(dev, job, emit)
    else:
        run_fold(dev, emit)


def compare(a, b, dumps):
    A = {r["case"]: r for r in map(json.loads, open(a))}
    Bm = {r["case"]: r for r in map(json.loads, open(b))}
    differ = 0
    for case in sorted(set(A) | set(Bm)):
        x, y = A.get(case), Bm.get(case)
        if x == y:
            continue
        differ += 1
        what = "missing" if x is None or y is None else "PATTERN" if x["pattern"] != y["pattern"] else "values"
        rel = ""
        if what == "values" and dumps:
            fn = case.replace("/", "_").replace(" ", "_") + ".npz"
            va, vb = (np.load(os.path.join(dd, fn))["data"] for dd in dumps)
            rel = " max |a - b| / max |a| = %.3e" % (np.max(np.abs(va - vb)) / np.max(np.abs(va)))
        print("differs (%s): %s%s" % (what, case, rel))
    print("gw_digest: %d of %d lines differ (%s against %s)" % (differ, len(set(A) | set(Bm)), a, b))
    return differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gw_driver_digest.jsonl"))
    ap.add_argument("--dump", default=None)
    ap.add_argument("--one", default=None, help="(internal) run this job in this process and print its lines")
    ap.add_argument("--in-process", action="store_true",
                    help="all cases in this process, lines to stdout (under tools/kernel_trace.py, which follows one process)")
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--dumps", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare[0], args.compare[1], args.dumps)
    if args.one:
        return run_one(args.one, args.dump)
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    if args.in_process:
        for job in jobs():
            saved = dict(os.environ)
            run_one(job, args.dump)
            os.environ.clear()
            os.environ.update(saved)
        return
    lines = []
    for job in jobs():
        cmd = [sys.executable, os.path.abspath(__file__), "--one", job] + (["--dump", args.dump] if args.dump else [])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
        if res.returncode != 0:
            sys.stderr.write(res.stderr[-2000:])
            raise SystemExit("gw_digest: job %s ended with %d" % (job, res.returncode))
        lines += [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("gw_digest: %d lines -> %s" % (len(lines), args.out))


if __name__ == "__main__":
    main()
