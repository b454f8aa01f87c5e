"""Sequences of DIFFERENT FE matrices through one ExtractedSpline (developer tool): the plans the product caches between calls
-- symbolic products keyed by shape and nnz, tensor-pattern plans, fold plans keyed by a checksum of K_u's pattern, cell
plans -- must never serve a matrix they were not made for (the reference recomputes the symbolic product on every call,
tIGAr/common.py:1194-1195).  Per random patch: Laplace, random values on the pattern, two matrices with the SAME number of
hand-added couplings at different places, Laplace again, mass; each product against the oracle.

    python tests/fuzz/fuzz_sequences.py [--seed S] [--cases N] [--max-dofs R]

Under TIGAR_IMPLICIT_M=1 the patches with several fields go through the streamed field engine, which forms the product
block by block and skips the blocks it judges empty: the summary counts the cases in which a hand-added coupling is ALL an
off-diagonal block holds on the rows of the patch and sits off their first, middle and last node plane -- what three
probes of the block do not see (`streamed_couplings_off_the_probed_planes`)."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import tigar_oracle as O  # noqa: E402
import fuzz_parity as fz  # noqa: E402


def off_the_probed_planes(X, base, nf, pf, nz):
    """does an off-diagonal field block of X hold entries, all of them added by hand (not in ``base``) and none on the first,
    the middle or the last node plane of the rows?"""
    n1 = X.shape[0] // nf
    E = (X - base).tocoo()
    probed = {0, nz // 2, nz - 1}
    found = False
    for f in range(nf):
        for g in range(nf):
            if f == g or base[f * n1:(f + 1) * n1, g * n1:(g + 1) * n1].nnz:
                continue
            planes = set(((E.row[(E.row // n1 == f) & (E.col // n1 == g) & (E.data != 0)] % n1) // pf).tolist())
            found = found or (len(planes) > 0 and not (planes & probed))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--max-dofs", type=int, default=20000, help="largest number of FE rows (all fields) of a patch drawn")
    a = ap.parse_args()
    import tigar_amd as t
    from tigar_amd import BSplines as B, forms as F
    rng0 = np.random.default_rng(a.seed)
    bad = declined = off_probe = 0
    for i in range(a.cases):
        case = fz.draw_case(rng0, a.max_dofs)
        case["nfields"] = 1 if case["nfields"] == 1 else 2
        nf = case["nfields"]
        try:
            kvs = fz.knot_vectors(case, B.uniformKnots)
            gen = t.EqualOrderSpline(nf, B.ExplicitBSplineControlMesh(case["ps"], kvs))
            so = O.BSpline(case["ps"], kvs)
            gen.addZeroDofs(0, [0, 1])
            spline = t.ExtractedSpline(gen, 2 * max(case["ps"]))
            V1 = spline.V if nf == 1 else t.ExtractedSpline(t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh(case["ps"], kvs)), 2).V
            L = F.LaplaceForm().assemble_matrix(V1).to_scipy().tocsr()
            Mm = F.MassForm().assemble_matrix(V1).to_scipy().tocsr()
            if nf > 1:
                L, Mm = sp.block_diag([L] * nf, format="csr"), sp.block_diag([Mm] * nf, format="csr")
            Mo = O.generate_M_tensor(so, nfields=nf)
            rng = np.random.default_rng(case["val_seed"])
            R = L.copy()
            R.data = rng.standard_normal(R.nnz)
            n = L.shape[0]

            def extra(seed):
                r2 = np.random.default_rng(seed)
                for _ in range(500):
                    E = sp.csr_matrix((r2.standard_normal(3), (r2.integers(0, n, 3), r2.integers(0, n, 3))), shape=L.shape)
                    X = (R + E).tocsr()
                    if X.nnz == R.nnz + 3:          # three NEW positions: every variant has the same nnz
                        return X
                return None                         # (a patch of one element: the FE matrix is dense, nothing to add)
            seq = [("laplace", L), ("random", R), ("extra a", extra(1)), ("extra b", extra(2)), ("extra c", extra(3)),
                   ("laplace again", L), ("mass", Mm), ("extra a again", extra(1))]
            seq = [(nm, X) for nm, X in seq if X is not None]
            zd = list(spline.zeroDofs)
            idx = np.asarray(spline.localDofIndices(), dtype=np.int64)       # (several implicit fields: plane by plane)
            streamed = nf > 1 and bool(getattr(gen.M, "is_implicit", False))
            shape = V1.grids[0].shape()
            pf, nz = (int(np.prod(shape[:-1])) if len(shape) > 1 else 1), int(shape[-1])
            off_probe += streamed and any(nm.startswith("extra") and off_the_probed_planes(X, R, nf, pf, nz) for nm, X in seq)
            for name, A in seq:
                A = A.tocsr()
                A.sort_indices()
                K = spline.extractMatrix(A, diag=2.0).to_scipy()
                Ko = O.extract_matrix(Mo, A, zd, diag=2.0)
                if not np.array_equal(idx, np.arange(Ko.shape[0])):
                    Ko = Ko.tocsr()[idx][:, idx].tocsr()
                K.sort_indices(), Ko.sort_indices()
                e = abs(K - Ko).max() / abs(Ko).max()
                assert e <= 1e-12, "%s: values %g" % (name, e)
                assert np.array_equal(K.indptr, Ko.indptr) and np.array_equal(K.indices, Ko.indices), "%s: pattern" % name
        except Exception as ex:  # noqa: BLE001
            if isinstance(ex, ValueError) and "open knot vector in the slab direction" in str(ex):
                declined += 1        # documented limit: streamed with a periodic LAST direction
                continue
            bad += 1
            print(json.dumps({"failed": i, "error": "%s: %s" % (type(ex).__name__, str(ex)[:200]), "case": case}), flush=True)
    print(json.dumps({"cases": a.cases, "failed": bad, "declined_periodic_slab_direction": declined,
                      "streamed_couplings_off_the_probed_planes": int(off_probe), "seed": a.seed}))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
