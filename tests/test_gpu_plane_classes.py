"""-m gpu: the x and y passes of the tensor-pattern PtAP over a Kronecker-sum form contract ONE FE plane per class of
planes whose rows of the last-direction factor are equal bit for bit (tt_plane_classes, csrc/tg_tensor_body.h); the other
planes of the class share its B2 block in the z pass.  K must be byte for byte (indptr, indices, data) what it is with
TIGAR_TT_PLANE_CLASSES=0, where every plane is contracted; the contracted counts show that the shared path is taken."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = ("TIGAR_TT_PLANE_CLASSES", "TIGAR_IMPLICIT_M", "TIGAR_SUB_PLANES")


def _open_knots(p, verts):
    return [verts[0]] * p + list(verts) + [verts[-1]] * p


def _z_vertices(kind, n):
    """n elements on [0, 1] (all values exact in binary): uniform; graded (lengths (2 i + 1) / n^2, all different);
    uniform on the first half and graded on the second (lengths 1 / n, then (2 i + 1) / (2 (n/2)^2), all different
    from 1 / n for n = 8: 1, 3, 5, 7 against 4 thirty-seconds)"""
    if kind == "uniform":
        return [float(i) / n for i in range(n + 1)]
    if kind == "graded":
        return [float(i * i) / (n * n) for i in range(n + 1)]
    h = n // 2
    return [float(i) / n for i in range(h)] + [0.5 + 0.5 * float(i * i) / (h * h) for i in range(h + 1)]


def _spline(p, nels, zkind):
    import tigar_amd as t
    from tigar_amd import BSplines as B
    kvs = [B.uniformKnots(p, 0., 1., nels[0]), B.uniformKnots(p, 0., 1., nels[1]), _open_knots(p, _z_vertices(zkind, nels[2]))]
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * 3, kvs))
    sp0 = gen.getScalarSpline(0)
    for direction in range(3):
        for side in (0, 1):
            gen.addZeroDofs(0, sp0.getSideDofs(direction, side))
    return gen, t.ExtractedSpline(gen, 2 * p)


def _n_classes(z_factors, z0, z1):
    """classes of the planes [z0, z1): rows of the last-direction factors grouped by (length, bytes of every term)"""
    import scipy.sparse as sp
    Fs = [sp.csr_matrix(F) for F in z_factors]
    for F in Fs:
        F.sort_indices()
    keys = set()
    for q in range(z0, z1):
        keys.add(tuple(F.data[F.indptr[q]:F.indptr[q + 1]].tobytes() for F in Fs))
    return len(keys)


def _same_bytes(Ka, Kb):
    return Ka.indptr.tobytes() == Kb.indptr.tobytes() and Ka.indices.tobytes() == Kb.indices.tobytes() and \
        Ka.data.tobytes() == Kb.data.tobytes()


@pytest.fixture
def contracted(monkeypatch):
    """(z0, z1, planes contracted) of every tg_tensor_planes_kron call made while the fixture lives"""
    from tigar_amd.tensorptap import TensorPtAP
    calls = []
    inner = TensorPtAP.planes_kron

    def spy(self, packed, z0, z1):
        piece = inner(self, packed, z0, z1)
        if piece is not None:
            calls.append((int(z0), int(z1), piece.n_contracted))
        return piece
    monkeypatch.setattr(TensorPtAP, "planes_kron", spy)
    return calls


def _assemble(p, nels, zkind, form, sub_planes, classes):
    os.environ["TIGAR_IMPLICIT_M"] = "1"
    os.environ["TIGAR_SUB_PLANES"] = str(sub_planes)
    if classes is not None:
        os.environ["TIGAR_TT_PLANE_CLASSES"] = classes
    try:
        gen, spline = _spline(p, nels, zkind)
        K = spline.assembleMatrix(form, diag=2.0)
        assert getattr(gen.M, "is_implicit", False)
        return K.to_scipy(), [f[2] for f in form.factors(spline.V)]
    finally:
        for k in ENV:
            os.environ.pop(k, None)


@pytest.mark.parametrize("zkind", ["uniform", "graded", "half"])
@pytest.mark.parametrize("p,nels", [(3, (5, 4, 8)), (2, (6, 5, 8)), (1, (4, 4, 8))])
def test_K_is_byte_for_byte_that_of_contracting_every_plane(p, nels, zkind, contracted):
    """LaplaceForm (three terms) and MassForm (one), zero dofs on all faces, in sub-slabs of 2 and 3 dof planes (pieces
    that start and end inside a class; planes handed over by the ring) and in one sub-slab.  Uniform z knots: a handful
    of classes; graded: every plane is its own class and nothing is shared; half and half: both in one call."""
    from tigar_amd import forms as F
    nfe2 = p * nels[2] + 1
    for form in (F.LaplaceForm(), F.MassForm()):
        for sub in (2, 3, 64):
            del contracted[:]
            K_on, zf = _assemble(p, nels, zkind, form, sub, None)
            calls = list(contracted)
            del contracted[:]
            K_off, _ = _assemble(p, nels, zkind, form, sub, "0")
            calls_off = list(contracted)
            assert _same_bytes(K_on, K_off)
            # the fused path was taken, over every plane once, and contracted one plane per class of each call's planes
            assert calls and sum(z1 - z0 for z0, z1, _ in calls) == nfe2
            assert [c[2] for c in calls] == [_n_classes(zf, z0, z1) for z0, z1, _ in calls]
            assert [c[:2] for c in calls_off] == [c[:2] for c in calls] and all(n == z1 - z0 for z0, z1, n in calls_off)
            if sub == 64:
                assert [c[:2] for c in calls] == [(0, nfe2)]
                n = calls[0][2]
                if zkind == "uniform":
                    # first plane, last plane, the p - 1 nodes inside an element, the vertices between two elements
                    assert n == (p + 2 if p > 1 else 3) and n < nfe2
                elif zkind == "graded":
                    assert n == nfe2
                else:
                    assert (p + 2 if p > 1 else 3) < n < nfe2


def test_one_ulp_in_one_row_of_one_term_takes_the_plane_out_of_its_class():
    """planes_kron and the z stage directly: the factors of LaplaceForm at p = 3, elements (4, 3, 8), then with one
    value of an interior z row of the last term moved by one ulp"""
    import scipy.sparse as sp
    from tigar_amd import forms as F
    from tigar_amd.tensorptap import TensorPtAP
    p, nels = 3, (4, 3, 8)
    gen, spline = _spline(p, nels, "uniform")
    plan = TensorPtAP.for_extraction(spline._kron)
    assert plan is not None
    nfe2, ncp2 = p * nels[2] + 1, nels[2] + p
    zd = list(spline.zeroDofs)
    factors = [[sp.csr_matrix(m).copy() for m in term] for term in F.LaplaceForm().factors(spline.V)]
    moved = [[m.copy() for m in term] for term in factors]
    Fz = moved[2][2]                                           # last term, last direction: the 1-D stiffness matrix
    Fz.sort_indices()
    q = 13                                                     # node 1 of element 4: shares plane 1's blocks
    j = Fz.indptr[q] + 2
    Fz.data[j] = np.nextafter(Fz.data[j], np.inf)

    def run(fs, classes):
        if classes is not None:
            os.environ["TIGAR_TT_PLANE_CLASSES"] = classes
        try:
            packed = plan.pack_kron_factors(fs)
            assert packed is not None
            piece = plan.planes_kron(packed, 0, nfe2)
            assert piece is not None
            return plan.zstage([piece], 0, ncp2, zd, 2.0).to_scipy(), piece.n_contracted
        finally:
            os.environ.pop("TIGAR_TT_PLANE_CLASSES", None)

    K0, n0 = run(factors, None)
    K0_off, n0_off = run(factors, "0")
    K1, n1 = run(moved, None)
    K1_off, n1_off = run(moved, "0")
    assert n0 == 5 and n1 == 6 and n0_off == n1_off == nfe2
    assert _same_bytes(K0, K0_off) and _same_bytes(K1, K1_off)
    assert not _same_bytes(K0, K1)                             # (the ulp reaches K: plane 13 was really contracted on its own)


def test_blocks_with_different_bases_on_rows_and_columns_share_planes_too():
    """K_fg = M_f^T A M_g for the components of a div-conforming B-spline (degrees (1, 1, 1), elements (1, 1, 2); all
    fields extract to one Q_2 grid) with A the Laplace form's Kronecker sum on that grid: pair plans take the same
    x and y passes, so the same planes are shared"""
    from tigar_amd import BSplines as B, common as tc, device as dev, forms as F
    from tigar_amd.compatibleSplines import BSplineCompat
    from tigar_amd.kronptap import KronExtraction
    from tigar_amd.tensorptap import TensorPtAP
    dev.device_info()
    degs, nels = (1, 1, 1), (1, 1, 2)
    kv = [B.uniformKnots(degs[k], 0., 1. + 0.25 * k, nels[k]) for k in range(3)]
    gen = BSplineCompat(tc.selfcomm, B.ExplicitBSplineControlMesh(list(degs), kv), "RT", list(degs))
    kxs = [KronExtraction(gen.getFieldSpline(f), gen.V.grids[f]) for f in range(3)]
    g = gen.V.grids[0]
    V1 = type(gen.V)([g], gen.V.element)
    factors = F.LaplaceForm().factors(V1)
    nz = g.shape()[-1]
    want = _n_classes([f[2] for f in factors], 0, nz)
    assert want < nz
    for f in range(3):
        for gg in range(3):
            plan = TensorPtAP.for_pair(kxs[f], kxs[gg])
            assert plan is not None
            packed = plan.pack_kron_factors(factors)
            assert packed is not None
            Ks = []
            for classes in (None, "0"):
                if classes is not None:
                    os.environ["TIGAR_TT_PLANE_CLASSES"] = classes
                try:
                    piece = plan.planes_kron(packed, 0, nz)
                    assert piece is not None and piece.n_contracted == (want if classes is None else nz)
                    Ks.append(plan.zstage([piece], 0, kxs[f].ncp[2]).to_scipy())
                finally:
                    os.environ.pop("TIGAR_TT_PLANE_CLASSES", None)
            assert Ks[0].nnz == plan.k_nnz(0, kxs[f].ncp[2]) and _same_bytes(Ks[0], Ks[1])
