"""CPU: host side of the fast diagonalization preconditioner (tigar_amd/fastdiag.py): free-box detection and the 1-D
generalized eigendecompositions against a dense Kronecker P."""
import numpy as np
import pytest
import scipy.sparse as sp


def _faces(shape, faces):
    d = len(shape)
    idx = np.arange(int(np.prod(shape))).reshape(shape[::-1])
    out = []
    for k, side in faces:
        sl = [slice(None)] * d
        sl[d - 1 - k] = 0 if side == 0 else shape[k] - 1
        out.append(idx[tuple(sl)].ravel())
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


@pytest.mark.parametrize("shape", [(7, 5), (6, 5, 4)])
def test_free_box_whole_faces(shape):
    from tigar_amd.fastdiag import free_box
    d = len(shape)
    every = [(k, s) for k in range(d) for s in (0, 1)]
    assert free_box(_faces(shape, every), shape) == ([1] * d, [s - 1 for s in shape])
    assert free_box(_faces(shape, []), shape) == ([0] * d, list(shape))
    lo, hi = free_box(_faces(shape, [(0, 1), (d - 1, 0)]), shape)
    assert lo == [0] * (d - 1) + [1] and hi == [shape[0] - 1] + list(shape[1:])


def test_free_box_several_fields():
    from tigar_amd.common import AbstractExtractionGenerator  # noqa: F401  (package imports without a GPU)
    from tigar_amd.fastdiag import TensorStructure

    class KX(object):
        d, ncp = 2, [5, 4]
    shape = [5, 4]
    z = np.concatenate([_faces(shape, [(0, 0)]), 20 + _faces(shape, [(1, 1), (0, 1)])])
    ts = TensorStructure(KX(), 2, z, {})
    assert ts.boxes() == [([1, 0], [5, 4]), ([0, 0], [4, 3])]


def test_free_box_rejects_partial_faces_and_points():
    from tigar_amd.fastdiag import free_box
    shape = (6, 5)
    side = _faces(shape, [(0, 0)])
    with pytest.raises(ValueError, match="whole faces"):
        free_box(side[:3], shape)
    with pytest.raises(ValueError, match="whole faces"):
        free_box(np.array([13]), shape)
    with pytest.raises(ValueError, match="no free box"):
        free_box(np.arange(30), shape)


def _iga_1d(p, knots):
    """1-D IGA stiffness / mass of an open knot vector (scipy's B-spline evaluation, Gauss quadrature per span)"""
    from scipy.interpolate import BSpline
    t = np.asarray(knots, dtype=float)
    n = len(t) - p - 1
    xg, wg = np.polynomial.legendre.leggauss(p + 1)
    K, M = np.zeros((n, n)), np.zeros((n, n))
    for a, b in zip(t[:-1], t[1:]):
        if b <= a:
            continue
        x = 0.5 * (a + b) + 0.5 * (b - a) * xg
        w = 0.5 * (b - a) * wg
        N = np.array([BSpline(t, np.eye(n)[i], p)(x) for i in range(n)])
        dN = np.array([BSpline(t, np.eye(n)[i], p).derivative()(x) for i in range(n)])
        K += (dN * w) @ dN.T
        M += (N * w) @ N.T
    return K, M


def _kron(mats):
    out = np.ones((1, 1))
    for m in mats[::-1]:
        out = np.kron(out, m)
    return out


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_eig_reproduces_inverse(case):
    from tigar_amd.fastdiag import eig_1d
    from tigar_amd import BSplines as B
    if case == "2d":
        facs = [_iga_1d(2, B.uniformKnots(2, 0.0, 1.0, 5)),
                _iga_1d(3, [0, 0, 0, 0, 0.2, 0.5, 0.5, 0.9, 1, 1, 1, 1])]          # non-uniform, repeated interior knot
        coef = [1.0, 2.0, 0.3]
    else:
        facs = [_iga_1d(2, [0, 0, 0, 0.1, 0.4, 1, 1, 1]), _iga_1d(3, B.uniformKnots(3, 0.0, 2.0, 3)),
                _iga_1d(2, [0, 0, 0, 0.5, 0.5, 1, 1, 1])]
        coef = [1.0, 0.5, 2.0, 0.0]
    d = len(facs)
    Ks = [f[0][1:-1, 1:-1] for f in facs]
    Ms = [f[1][1:-1, 1:-1] for f in facs]
    P = coef[d] * _kron(Ms)
    for k in range(d):
        P = P + coef[k] * _kron([Ks[j] if j == k else Ms[j] for j in range(d)])
    QL = [eig_1d(Ks[k], Ms[k]) for k in range(d)]
    for k in range(d):
        Q, lam = QL[k]
        assert np.allclose(Q.T @ Ms[k] @ Q, np.eye(len(lam)), atol=1e-12)
    Q = _kron([q for q, _ in QL])
    lam = np.full(Q.shape[0], coef[d])
    for k in range(d):
        lam = lam + coef[k] * _kron([np.diag(QL[j][1]) if j == k else np.eye(len(QL[j][1])) for j in range(d)]).diagonal()
    Pinv = Q @ np.diag(1.0 / lam) @ Q.T
    ref = np.linalg.inv(P)
    assert np.linalg.norm(Pinv - ref) <= 1e-12 * np.linalg.norm(ref) * np.linalg.cond(P) ** 0 * 10
