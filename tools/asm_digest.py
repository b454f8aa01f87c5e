"""SHA-256 of the output bytes of every mapped element form (csrc/tg_assemble.hip, and the point-coefficient matrices of
csrc/tg_coef.hip that take its sum-factorised route) on the edge shapes of the tests (developer tool: a change that is meant
to leave the results bit for bit alone runs this file in both checkouts and compares the two outputs line by line).

One JSON line per (entry point, case, plain / rational, rows, switches); the row blocks of a case are hashed together, plane
after plane, into one line per entry point, and so are the d * d elasticity blocks.
  shapes    the 1-D, 2-D, surface and 3-D patches of ``PLAIN`` of tests/test_gpu_rational.py (nq below and above p + 1, the
            LDS edge at nq = 9) and the rational volumes of tests/test_gpu_assembly.py: ``assemble_mapped_matrix`` (mass,
            laplace, biharmonic), every ``assemble_mapped_elasticity_block``, ``assemble_mapped_load``, ``assemble_coef_matrix``,
            ``assemble_coef_blocks``;
  rows      on the volumes: whole matrices, and the row blocks of every single node plane from windows of the control functions;
  switches  each case of tests/test_gpu_asm_routes.py with its switches.
Inputs are seeded.

    python tools/asm_digest.py [--out profiles/asm_driver_digest.jsonl]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tigar_amd  # noqa: E402
from tigar_amd import device as dev, NURBS, common  # noqa: E402
from geom_util import rational_volume  # noqa: E402
import test_gpu_rational as RAT  # noqa: E402
import test_gpu_asm_routes as ROUTES  # noqa: E402

LAM, MU = 1.3, 0.7
# (p, elements): the sum-factorised cases, the window cases (p = 4: the plain kernel) and one line of 17 (two default pieces)
VOLUMES = [(1, (3, 2, 4)), (2, (3, 4, 3)), (3, (2, 3, 2)), (3, (1, 1, 1)), (2, (5, 1, 2)), (3, (3, 2, 4)), (2, (3, 3, 5)),
           (4, (2, 1, 3)), (2, (17, 1, 2)), (3, (33, 2, 1))]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def csr(m):
    m = m.to_scipy()
    return [m.indptr.astype(np.int64), m.indices.astype(np.int64), m.data]


def forms_of(uks, p, cp, nq, seed, emit, name, rows=None):
    """every entry point on one patch (rows: (row0, row1, first node, end node of the window of the control functions))"""
    d, nsd = len(uks), len(cp) - 1
    kw, tag, a, b = {}, None, 0, cp[0].size
    if rows is not None:
        row0, row1, a, b = rows
        kw, tag = dict(row0=row0, row1=row1, cp_node0=a), "%d:%d" % (row0, row1)
    dcp = [dev.DeviceVector(data=np.asarray(v[a:b], dtype=np.float64)) for v in cp]
    rng = np.random.default_rng(seed)
    fn = dev.DeviceVector(data=rng.standard_normal(cp[0].size)[a:b])
    for rat in (False, True):
        for form in ("mass", "laplace") + (("biharmonic",) if nsd == d and not rat else ()):
            emit("assemble_mapped_matrix:" + form, name, rat, tag, sha(*csr(dev.assemble_mapped_matrix(uks, p, dcp, form, nq=nq, rational=rat, **kw))))
        emit("assemble_mapped_load", name, rat, tag, sha(dev.assemble_mapped_load(uks, p, dcp, fn, nq=nq, rational=rat, **kw).get_local()))
        if nsd == d:                # the d * d blocks, (0, 0), (0, 1), ..., in one line
            blocks = [dev.assemble_mapped_elasticity_block(uks, p, dcp, i, j, LAM, MU, nq=nq, rational=rat, **kw) for i in range(d) for j in range(d)]
            emit("assemble_mapped_elasticity_block:all", name, rat, tag, sha(*[x for B in blocks for x in csr(B)]))
        if rows is not None:
            continue
        npts = dev.quad_count(uks, p + 1 if nq is None else nq)
        dv = lambda *shape: dev.DeviceVector(data=rng.standard_normal(int(np.prod(shape))))
        coef = dev.coef_transform(uks, p, dcp, dv(nsd * nsd, npts), dv(nsd, npts), dv(nsd, npts), dv(npts), a_kind=2, nq=nq, rational=rat)
        emit("assemble_coef_matrix", name, rat, tag, sha(*csr(dev.assemble_coef_matrix(uks, p, dcp, coef, nq=nq))))
        if nsd == d and d in (2, 3):
            blocks = dev.coef_transform_blocks(uks, p, dcp, dv(d ** 4, npts), dv(d * d, npts), nq=nq, rational=rat)
            emit("assemble_coef_blocks", name, rat, tag, sha(*csr(dev.assemble_coef_blocks(uks, p, dcp, blocks, nq=nq))))


def volume(p, nels, emit):
    kvs, C = rational_volume(p, nels)
    gen = tigar_amd.EqualOrderSpline(common.selfcomm, 1, NURBS.NURBSControlMesh([p] * 3, kvs, C))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k], dtype=np.float64) for k in range(3)]
    cp = [f.vector().get_local() for f in gen.cpFuncs]
    name = "volume_p%d_%dx%dx%d" % ((p,) + tuple(nels))
    forms_of(uks, p, cp, None, 1000 * p + sum(nels), emit, name)
    n0, n1, n2 = g.shape()
    plane = n0 * n1
    planes = {}                                # (entry, rational) -> the digests of its row blocks, plane after plane
    for z in range(n2):                        # single node planes, the control functions on the window their elements need
        e0 = z // p - 1 if (z > 0 and z % p == 0) else z // p
        e1 = min(nels[2], z // p + 1)
        forms_of(uks, p, cp, None, 1000 * p + sum(nels), lambda entry, case, rat, tag, digest: planes.setdefault((entry, rat), []).append(digest),
                 name, rows=(z * plane, (z + 1) * plane, e0 * p * plane, (e1 * p + 1) * plane))
    for (entry, rat), digests in planes.items():
        emit(entry, name, rat, "%d single planes" % n2, hashlib.sha256("".join(digests).encode()).hexdigest())


def switches(emit):
    class NS:
        pass
    T = NS()
    T.t, T.dev, T.N, T.c = tigar_amd, dev, NURBS, common
    for kernel, p, form, variant, env in ROUTES.ROWS:
        c = ROUTES._patch(T, p)
        dcp = [dev.DeviceVector(data=v) for v in c["cp"]]
        os.environ.update(env)
        try:
            out = ROUTES._run(T, c, dcp, form, variant)
        finally:
            for k in env:
                del os.environ[k]
        emit("route:%s:%s" % (form, variant), "p%d" % p, variant == "rational", " ".join("%s=%s" % kv for kv in sorted(env.items())), sha(*out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asm_driver_digest.jsonl"))
    args = ap.parse_args()
    dev.device_info()
    with open(args.out, "w") as f:
        def emit(entry, case, rational, rows, digest):
            f.write(json.dumps({"entry": entry, "case": case, "rational": rational, "rows": rows, "sha256": digest}) + "\n")
        for name in sorted(RAT.PLAIN):
            p, nq, uks, cp = RAT.PLAIN[name]()
            forms_of(uks, p, [np.asarray(v, dtype=np.float64) for v in cp], nq, len(name), emit, name)
        for p, nels in VOLUMES:
            volume(p, nels, emit)
        switches(emit)
    print("asm_digest: %d lines -> %s" % (sum(1 for _ in open(args.out)), args.out))


if __name__ == "__main__":
    main()
