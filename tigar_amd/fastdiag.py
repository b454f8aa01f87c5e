"""
Fast diagonalization (FD) preconditioner for CG on single tensor-product patches (Lynch, Rice & Thomas 1964; Sangalli &
Tani 2016 for IGA).

Per field, on the box of free dofs of its control grid:

    P    = sum_k c_k (M_{d-1} x .. x K_k x .. x M_0) + c_m (M_{d-1} x .. x M_0)
    P^-1 = (Q_{d-1} x .. x Q_0) diag(1 / (sum_k c_k lam_k[i_k] + c_m)) (Q_{d-1} x .. x Q_0)^T

with K_k / M_k the 1-D parametric IGA stiffness / mass matrices (``M1_k^T K_fe M1_k`` from the 1-D extraction factors of
``KronExtraction`` and ``forms.fe_matrices_1d``: exact, B-splines of degree p are degree-p polynomials per element) and
``Q_k, lam_k`` from the generalized eigenproblem ``K_k Q = M_k Q lam`` (``Q^T M_k Q = I``).  The host work here is the
free-box detection, the 1-D matrices and their eigendecompositions (cached on the spline); the application and the
preconditioned CG run on the device (csrc/tg_fd.hip).
"""
import time

import numpy as np

from . import device as _dev

MAX_FREE_1D = 4096


def free_box(zero_local, shape):
    """(lo, hi) per direction such that the dofs of a control grid of ``shape`` (direction 0 fastest) that are NOT in the
    box [lo, hi) are exactly ``zero_local`` (field-local indices).  ValueError when the zero set is not a union of whole
    faces (layers) of the grid."""
    shape = [int(s) for s in shape]
    n = int(np.prod(shape))
    mask = np.zeros(n, dtype=bool)
    z = np.asarray(zero_local, dtype=np.int64)
    if z.size:
        if z.min() < 0 or z.max() >= n:
            raise ValueError("zero dofs outside the field's control grid")
        mask[z] = True
    m = mask.reshape(shape[::-1])          # [i_{d-1}, ..., i_0]
    free = ~m
    if not free.any():
        raise ValueError("fast_diagonalization: every dof of a field is a zero dof (no free box)")
    lo, hi = [], []
    d = len(shape)
    for k in range(d):
        ax = d - 1 - k
        other = tuple(a for a in range(d) if a != ax)
        idx = np.nonzero(free.any(axis=other))[0]
        lo.append(int(idx[0]))
        hi.append(int(idx[-1]) + 1)
    box = np.zeros_like(free)
    box[tuple(slice(lo[d - 1 - a], hi[d - 1 - a]) for a in range(d))] = True
    if not np.array_equal(box, free):
        raise ValueError("fast_diagonalization: the zero dofs are not a union of whole faces of the control grid "
                         "(partial faces or single points)")
    return lo, hi


def iga_matrices_1d(kx, k):
    """(K_k, M_k): 1-D parametric IGA stiffness and mass of direction ``k`` of a ``KronExtraction``, dense"""
    from .forms import fe_matrices_1d
    g = kx.grid
    Mfe, Kfe = fe_matrices_1d(g.vertices[k], g.degree)
    M1 = kx.M1[k]
    if Mfe.shape[0] != M1.shape[0]:
        raise ValueError("fast_diagonalization: the node grid does not match the 1-D FE matrices")
    return (M1.T @ Kfe @ M1).toarray(), (M1.T @ Mfe @ M1).toarray()


def eig_1d(K1, M1):
    """generalized eigendecomposition K1 Q = M1 Q lam, Q^T M1 Q = I"""
    import scipy.linalg
    lam, Q = scipy.linalg.eigh(K1, M1)
    return np.ascontiguousarray(Q), lam


class TensorStructure(object):
    """What ``ExtractedSpline.extractMatrix`` attaches to the K it returns (``K.tensor_structure``) when the space is one
    tensor-product patch on one rank with M the Kronecker product of its 1-D factors: per field the dof offset, the
    control-grid shape and the 1-D extraction factors, plus the zero dofs; the free boxes are found when first asked for.
    Holds references only (the 1-D tables, the zero-dof array, the spline's small setup cache)."""

    def __init__(self, kx, nfields, zero_dofs, cache):
        self.kx = kx
        self.d = kx.d
        self.shape = [int(s) for s in kx.ncp]
        self.nfields = int(nfields)
        nper = int(np.prod(self.shape))
        self.offsets = [f * nper for f in range(self.nfields)]
        self.n = nper * self.nfields
        self.zero_dofs = np.zeros(0, dtype=np.int64) if zero_dofs is None else zero_dofs
        self._cache = cache

    def key(self):
        z = np.unique(np.asarray(self.zero_dofs, dtype=np.int64))
        return (self.nfields, tuple(self.shape), z.size, hash(z.tobytes()))

    def boxes(self):
        z = np.unique(np.asarray(self.zero_dofs, dtype=np.int64))
        out = []
        for f in range(self.nfields):
            o = self.offsets[f]
            zf = z[(z >= o) & (z < o + self.n // self.nfields)] - o
            out.append(free_box(zf, self.shape))
        return out


class _Setup(object):
    """host setup of one (zero-dof set, fields): boxes, 1-D eigendecompositions, the device object"""

    def __init__(self, ts):
        t0 = time.perf_counter()
        self.boxes = ts.boxes()
        self.d = ts.d
        self.nfields = ts.nfields
        self.blocks = []
        one_d = {}
        for f, (lo, hi) in enumerate(self.boxes):
            for k in range(ts.d):
                if hi[k] - lo[k] > MAX_FREE_1D:
                    raise ValueError("fast_diagonalization: direction %d has %d free functions (the host eigensolve "
                                     "takes at most %d)" % (k, hi[k] - lo[k], MAX_FREE_1D))
            per = []
            for k in range(ts.d):
                key = (k, lo[k], hi[k])
                if key not in one_d:
                    K1, M1 = iga_matrices_1d(ts.kx, k)
                    K1, M1 = K1[lo[k]:hi[k], lo[k]:hi[k]], M1[lo[k]:hi[k], lo[k]:hi[k]]
                    Q, lam = eig_1d(K1, M1)
                    one_d[key] = (Q, lam, np.diag(K1).copy(), np.diag(M1).copy())
                per.append(one_d[key])
            self.blocks.append((ts.offsets[f], lo, hi, per))
        self.eig_seconds = time.perf_counter() - t0
        self.device = _dev.DeviceFD(ts.n)
        for off, lo, hi, per in self.blocks:
            self.device.add_block(off, ts.shape, lo, hi, [p[0] for p in per], [p[1] for p in per], [p[2] for p in per],
                                  [p[3] for p in per])
        self.seconds = time.perf_counter() - t0

    def gram(self, b):
        """Gram matrix of the diagonals of the d + 1 terms over block b's free box (separable: products of 1-D sums)"""
        per = self.blocks[b][3]
        d = self.d
        G = np.ones((d + 1, d + 1))
        for a in range(d + 1):
            for c in range(d + 1):
                for k in range(d):
                    ta = per[k][2] if a == k else per[k][3]
                    tc = per[k][2] if c == k else per[k][3]
                    G[a, c] *= float(np.dot(ta, tc))
        return G


def fit_coefficients(G, rhs):
    """non-negative least squares min || sum_a c_a t_a - diag K || over c >= 0, from the Gram matrix G and the sums
    <diag K, t_a>"""
    from scipy.optimize import nnls
    s = np.sqrt(np.maximum(np.diag(G), 1e-300))
    Gs = G / np.outer(s, s)
    rs = rhs / s
    w, V = np.linalg.eigh(Gs)
    keep = w > w.max() * 1e-14
    A = (np.sqrt(w[keep])[:, None] * V[:, keep].T)
    bb = (V[:, keep].T @ rs) / np.sqrt(w[keep])
    c, _ = nnls(A, bb)
    return c / s


class FastDiagonalization(object):
    """The FD preconditioner of one K: ``FastDiagonalization(K)`` for a K that ``ExtractedSpline.extractMatrix`` /
    ``assembleMatrix`` returned (it carries ``K.tensor_structure``), or ``FastDiagonalization(spline, K=K)``.
    ``coefficients``: None = fitted to diag K (non-negative least squares), else ``(c_0, .., c_{d-1}, c_mass)`` for every
    field; ``scaling``: "diagonal" (D^-1/2 P^-1 D^-1/2, D = diag K / diag P) or "none".
    ``.apply(r, z)``, ``.coefficients`` (per field), ``.setup_seconds``, ``.setup_reused``, ``.fit_seconds``."""

    def __init__(self, spline_or_K, K=None, coefficients=None, scaling="diagonal"):
        if K is None:
            K = spline_or_K
        else:
            ts_spline = spline_or_K.tensor_structure() if hasattr(spline_or_K, "tensor_structure") else None
            if ts_spline is not None and getattr(K, "tensor_structure", None) is None:
                K.tensor_structure = ts_spline
        if scaling not in ("diagonal", "none"):
            raise ValueError("fd_scaling must be 'diagonal' or 'none', not %r" % (scaling,))
        ts = getattr(K, "tensor_structure", None)
        if ts is None:
            raise ValueError("fast_diagonalization: %s" % getattr(
                K, "tensor_structure_refusal",
                "K carries no tensor-product structure (only a K returned by ExtractedSpline.extractMatrix / "
                "assembleMatrix of a single tensor-product patch on one rank qualifies, not a matrix built or uploaded "
                "by hand)"))
        if not isinstance(K, _dev.DeviceCSR):
            raise ValueError("fast_diagonalization: K must be the DeviceCSR that extractMatrix returned")
        if K.shape[0] != ts.n:
            raise ValueError("fast_diagonalization: K has %d rows, the spline %d dofs" % (K.shape[0], ts.n))
        key = ts.key()
        self.setup_reused = key in ts._cache
        if not self.setup_reused:
            ts._cache.clear()                  # (one setup per spline: a new zero-dof set replaces the old one)
            ts._cache[key] = _Setup(ts)
        self._setup = st = ts._cache[key]
        self.setup_seconds = st.seconds
        self.d = st.d
        t0 = time.perf_counter()
        rhs = st.device.fit(K, st.nfields)
        coef = np.zeros((st.nfields, 4))
        self.coefficients = []
        for b in range(st.nfields):
            if coefficients is None:
                c = fit_coefficients(st.gram(b), np.concatenate([rhs[b, :self.d], rhs[b, 3:4]]))
                if not np.any(c > 0):
                    raise ValueError("fast_diagonalization: no non-negative combination of the 1-D stiffness / mass terms "
                                     "fits diag K of field %d (every coefficient fits <= 0)" % b)
            else:
                c = np.asarray(coefficients, dtype=np.float64).ravel()
                if c.size != self.d + 1 or np.any(c < 0) or not np.any(c > 0):
                    raise ValueError("fd_coefficients must be %d non-negative numbers (c_0 .. c_%d, c_mass), not all 0"
                                     % (self.d + 1, self.d - 1))
            coef[b, :self.d] = c[:self.d]
            coef[b, 3] = c[self.d]
            self.coefficients.append(tuple(float(v) for v in c))
        st.device.set_coefficients(coef, scaling == "diagonal")
        self.fit_seconds = time.perf_counter() - t0
        self.device = st.device
        self.scaling = scaling

    def apply(self, r, z):
        """z = B r (DeviceVectors of K's size, distinct)"""
        self.device.apply(r, z)
        return z
