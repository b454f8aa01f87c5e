"""SHA-256 of the results of the Kronecker-stage PtAP driver (csrc/tg_ptap_box.hip: tg_ptap_kron, tg_ptap_kron_stage,
tg_ptap_kron_append) -- developer tool: a change that is meant to leave the results bit for bit alone runs this file in both
checkouts and compares the two outputs line by line.

One JSON line per result: {"case", "pattern": sha256(row pointers | columns), "values": sha256(values), "nnz"}.  Every case
runs in a process of its own, so that the capacity cache of the driver starts empty:
  routes     the cases of tests/test_gpu_kron_routes.py with their switches; the line and the box case of its endings test
             by each of the three endings; the stacked view that the box kernel has compacted; the declined stage;
  factored   the parametrisations of ``test_sum_factorised_ptap_equals_direct`` (tests/test_gpu_api.py) with the box kernels
             on: ``ptap_factored`` with every grouping of the directions, the slab-streamed assembly factored and direct,
             each with ``TIGAR_PTAP_ACCUM`` unset / ``int`` / ``float``.
Inputs are seeded.

    python tools/kron_digest.py [--out profiles/kron_driver_digest.jsonl] [--dump DIR]
    python tools/kron_digest.py --compare A.jsonl B.jsonl [--dumps DIR_A DIR_B]
    python tools/kernel_trace.py --min-ms 0 -- python tools/kron_digest.py --in-process

--in-process runs all cases in one process and prints the lines (the tracer follows one process); --dump keeps the
matrices (DIR/<case>.npz); --compare lists the lines that differ and, with the matrices of both runs, the largest
difference of the values relative to the largest entry where only the values differ.
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

SUM_FACTORISED = [(2, 2, 9), (2, 4, 5), (3, 2, 5), (3, 3, 4), (3, 4, 3), (1, 3, 7)]      # as tests/test_gpu_api.py
ACCUM = ["", "int", "float"]


def jobs():
    import test_gpu_kron_routes as R
    out = ["route:%d" % i for i in range(len(R.CASES))]
    out += ["ending:%d:%d" % (i, e) for i in (2, 6) for e in range(len(R.ENDINGS))]
    out += ["view", "decline"]
    out += ["factored:%d:%s" % (i, a) for i in range(len(SUM_FACTORISED)) for a in ACCUM]
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
        K = K.tocsr()
        K.sort_indices()
        rp, col = K.indptr.astype(np.int64), K.indices.astype(np.int64)
        if self.dump:
            np.savez(os.path.join(self.dump, case.replace("/", "_").replace(" ", "_") + ".npz"), indptr=rp, indices=col, data=K.data)
        print(json.dumps({"case": case, "pattern": sha(rp, col), "values": sha(K.data), "nnz": int(K.nnz)}), flush=True)


def run_route(dev, job, emit):
    import test_gpu_kron_routes as R
    parts = job.split(":")
    d, p, nel, groups, env, _ = R.CASES[int(parts[1])]
    how = R.ENDINGS[int(parts[2])] if parts[0] == "ending" else (True, False)
    os.environ.update(env)
    kx, A, _ = R.kron_case(d, p, nel)
    K = R.kron_chain(dev, kx, dev.DeviceCSR.from_scipy(A), R.ZD, R.DIAG, how[0], how[1], groups)
    emit("%s d=%d p=%d nel=%s groups=%s %s" % (job, d, p, nel, groups, " ".join("%s=%s" % kv for kv in sorted(env.items()))), K)


def run_view(dev, emit):
    import test_gpu_kron_routes as R
    kx, A, _ = R.kron_case(3, 2, 3)
    Ad = dev.DeviceCSR.from_scipy(A)
    plane = kx.ncp[0] * kx.nfe[1]
    n_x, half = plane * kx.nfe[2], (kx.nfe[2] // 2) * plane
    dims, fac = kx.dims(set()), [kx.M1[0], None, None]
    lo = dev.ptap_kron(Ad, 0, dims, fac, 0, half, intermediate=True)
    hi = dev.ptap_kron(Ad, 0, dims, fac, half, n_x, intermediate=True)
    view = dev.csr_vstack_view([lo, hi])
    os.environ["TIGAR_PTAP_LINE"] = "0"
    emit("view", dev.ptap_kron(view, 0, kx.dims({0}), [None, kx.M1[1], None], 0, kx.ncp[0] * kx.ncp[1] * kx.nfe[2]).to_scipy())


def run_decline(dev, emit):
    import scipy.sparse as sp
    import test_gpu_kron_routes as R
    n, m = 128, 4
    rng = np.random.default_rng(5)
    F = sp.lil_matrix((n, m))
    F[np.arange(n), np.arange(n) // 32] = 1.0
    F[:, 1] = 1.0
    F = F.tocsr()
    F.data = rng.standard_normal(F.nnz)
    K = dev.ptap_kron(dev.DeviceCSR.from_scipy(R.tridiagonal(n, rng)), 0, [n], [F], 0, m)
    emit("decline", None if K is None else K.to_scipy())


def run_factored(dev, job, emit):
    """the body of test_sum_factorised_ptap_equals_direct with TIGAR_PTAP_BOX=1, hashed instead of compared"""
    from oracle import tigar_oracle as O
    from tigar_amd import BSplines as B
    from tigar_amd.kronptap import KronExtraction, ptap_factored
    from tigar_amd.dist import SlabHotPath
    _, i, accum = job.split(":")
    d, p, nel = SUM_FACTORISED[int(i)]
    os.environ["TIGAR_PTAP_BOX"] = "1"
    if accum:
        os.environ["TIGAR_PTAP_ACCUM"] = accum
    basis = B.ExplicitBSplineControlMesh([p] * d, [B.uniformKnots(p, 0., 1., nel)] * d).getScalarSpline()
    grid = basis.generateMesh(degree=p)
    s = O.BSpline([p] * d, [O.uniform_knots(p, 0., 1., nel)] * d)
    Ao, bo, _, _ = O.poisson_fe_system(s, f1d=[lambda x: np.cos(x)] * d)
    rng = np.random.default_rng(7)
    Ao = Ao.tocsr().copy()
    Ao.data = Ao.data * (1.0 + 0.3 * rng.standard_normal(Ao.nnz))
    kx = KronExtraction(basis, grid)
    zd = basis.getSideDofs(0, 0) + basis.getSideDofs(d - 1, 1)
    nz, ncpz = grid.shape()[-1], basis.splines[-1].getNcp()
    name = "factored d=%d p=%d nel=%d accum=%s" % (d, p, nel, accum or "unset")
    for groups in [None] + ([[[0, 1], [2]], [[0], [1, 2]]] if d == 3 else []):
        emit("%s groups=%s" % (name, groups), ptap_factored(kx, dev.DeviceCSR.from_scipy(Ao), (0, nz), (0, nz), (0, ncpz), zd, 2.0, groups).to_scipy())
    for fac in (True, False):
        path = SlabHotPath(basis, grid, sub_planes=2, factored=fac)
        Ks, _ = path.assemble(lambda r0, r1: dev.DeviceCSR.from_scipy(Ao[r0:r1]), lambda r0, r1: dev.DeviceVector(data=bo[r0:r1]), zd, 2.0)
        emit("%s slabs factored=%s" % (name, fac), Ks.to_scipy())


def run_one(job, dump):
    from tigar_amd import device as dev
    dev.device_info()
    emit = Emit(dump)
    kind = job.split(":")[0]
    if kind in ("route", "ending"):
        run_route(dev, job, emit)
    elif kind == "view":
        run_view(dev, emit)
    elif kind == "decline":
        run_decline(dev, emit)
    else:
        run_factored(dev, job, emit)


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
    print("kron_digest: %d of %d lines differ (%s against %s)" % (differ, len(set(A) | set(Bm)), a, b))
    return differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_driver_digest.jsonl"))
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
            raise SystemExit("kron_digest: job %s ended with %d" % (job, res.returncode))
        lines += [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("kron_digest: %d lines -> %s" % (len(lines), args.out))


if __name__ == "__main__":
    main()
