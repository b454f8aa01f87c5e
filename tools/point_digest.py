"""SHA-256 of the output bytes of every point-kernel entry point (csrc/tg_postproc.hip, csrc/tg_boundary.hip and the plain
kernel of csrc/tg_coef.hip) on the edge shapes of the tests (developer tool: a change that is meant to leave the results
bit for bit alone runs this file in both checkouts and compares the two outputs line by line).

One JSON line per (entry point, case, plain / rational, face).  Volume cases: eight of ``CASES`` of
tests/test_gpu_postproc.py; face cases: all of ``CASES`` of tests/test_gpu_boundary.py, every face.  Inputs are seeded.

    python tools/point_digest.py [--out profiles/point_kernels_digest.jsonl]
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
from tigar_amd import device as dev  # noqa: E402
import test_gpu_postproc as VOL  # noqa: E402
import test_gpu_boundary as FACE  # noqa: E402

VOLUME_CASES = ["1d_p3_5", "2d_p2_6x5_full_and_partial_group", "2d_p3_3x2_nq2_fewer_points_than_nodes", "2d_p8_2x1_nq4",
                "3d_p2_3x2x4", "3d_p4_1x2x1_nq4", "surface_in_3d", "rational_volume_p2_2x3x2"]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def local(*vs):
    return [v.get_local() for v in vs if v is not None]


def volume(name, emit):
    p, nq, uks, cp = VOL.CASES[name]()
    nq = p + 1 if nq is None else nq
    d, nsd, n = len(uks), len(cp) - 1, np.asarray(cp[0]).size
    dcp = [dev.DeviceVector(data=np.asarray(v, dtype=np.float64)) for v in cp]
    npts = dev.quad_count(uks, nq)
    rng = np.random.default_rng(len(name))

    def dv(*shape):
        return dev.DeviceVector(data=rng.standard_normal(int(np.prod(shape))))
    u, fq, e, ge = dv(n), dv(npts), dv(npts), dv(nsd, npts)
    A1, A2, b, c, m, s, F = dv(npts), dv(nsd * nsd, npts), dv(nsd, npts), dv(nsd, npts), dv(npts), dv(npts), dv(nsd, npts)
    emit("quad_points", name, False, None, sha(*local(*dev.quad_points(uks, p, dcp, nq=nq))))
    for rat in (False, True):
        emit("quad_eval", name, rat, None, sha(*local(*dev.quad_eval(uks, p, dcp, u, grad=True, nq=nq, rational=rat))))
        emit("quad_load", name, rat, None, sha(*local(dev.quad_load(uks, p, dcp, fq, nq=nq, rational=rat))))
        emit("quad_error", name, rat, None, sha(np.array(dev.quad_error(uks, p, dcp, u, e, ge, nq=nq, rational=rat), dtype=np.float64)))
        for kind, A in ((0, None), (1, A1), (2, A2)):
            coef = dev.coef_transform(uks, p, dcp, A, b, c, m, a_kind=kind, nq=nq, rational=rat)
            emit("coef_transform_kind%d" % kind, name, rat, None, sha(*local(coef)))
            emit("assemble_coef_matrix_kind%d" % kind, name, rat, None, sha(dev.assemble_coef_matrix(uks, p, dcp, coef, nq=nq).to_scipy().data))
        emit("flux_transform", name, rat, None, sha(*local(dev.flux_transform(uks, p, dcp, s, F, nq=nq, rational=rat))))
        emit("quad_load_flux", name, rat, None, sha(*local(dev.quad_load_flux(uks, p, dcp, s, F, nq=nq, rational=rat))))
        if nsd == d and d in (2, 3):
            At, M = dv(d ** 4, npts), dv(d * d, npts)
            blocks = dev.coef_transform_blocks(uks, p, dcp, At, M, nq=nq, rational=rat)
            emit("coef_transform_blocks", name, rat, None, sha(*local(blocks)))
            emit("assemble_coef_blocks", name, rat, None, sha(dev.assemble_coef_blocks(uks, p, dcp, blocks, nq=nq).to_scipy().data))


def faces(name, emit):
    p, nq, uks, cp = FACE.CASES[name]()
    nq = p + 1 if nq is None else nq
    d, n = len(uks), np.asarray(cp[0]).size
    dcp = [dev.DeviceVector(data=np.asarray(v, dtype=np.float64)) for v in cp]
    for k in range(d):
        for side in (0, 1):
            face = "%d,%d" % (k, side)
            npts = dev.face_count(uks, k, nq)
            rng = np.random.default_rng(100 * k + side + len(name))
            u, a, b, c = (dev.DeviceVector(data=rng.standard_normal(m)) for m in (n, npts, npts, npts))
            start = rng.standard_normal(n)
            emit("face_points", name, False, face, sha(*local(*dev.face_points(uks, p, dcp, k, side, nq))))
            for rat in (False, True):
                emit("face_eval", name, rat, face, sha(*local(*dev.face_eval(uks, p, dcp, k, side, u, True, True, nq, rat))))
                out = dev.DeviceVector(data=start)
                dev.face_load(uks, p, dcp, k, side, a, b, out, nq, rat)
                emit("face_load", name, rat, face, sha(*local(out)))
                emit("face_matrix", name, rat, face, sha(dev.face_matrix(uks, p, dcp, k, side, a, b, c, nq, rat).to_scipy().data))
                lap = dev.assemble_mapped_matrix(uks, p, dcp, "laplace", rational=rat)
                ok = dev.face_matrix_add(lap, uks, p, dcp, k, side, a, b, c, scale=-0.75, nq=nq, rational=rat)
                emit("face_matrix_add", name, rat, face, sha(np.array([float(ok)]), lap.to_scipy().data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_kernels_digest.jsonl"))
    args = ap.parse_args()
    dev.device_info()
    with open(args.out, "w") as f:
        def emit(entry, case, rational, face, digest):
            f.write(json.dumps({"entry": entry, "case": case, "rational": rational, "face": face, "sha256": digest}) + "\n")
        for name in VOLUME_CASES:
            volume(name, emit)
        for name in sorted(FACE.CASES):
            faces(name, emit)
    print("point_digest: %d lines -> %s" % (sum(1 for _ in open(args.out)), args.out))


if __name__ == "__main__":
    main()
