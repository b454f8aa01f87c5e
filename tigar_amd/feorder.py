"""
FE operands in the caller's dof order.

Inside the package every FE object is numbered like the tensor node grid (``TensorFunctionSpace``: direction 0 fastest,
field after field).  An FE library numbers its dofs differently, so the matrices and vectors it assembles arrive in ITS
order.  ``FEOrder`` recognises the caller's node coordinates as a permutation of the node grid (``tg_nodes_locate``) and
brings operands to grid order / results to the caller's order on the device (``tg_csr_permute_sym``, ``tg_vec_permute``,
csrc/tg_feorder.hip).  The caller's order exists only at the boundary of ``ExtractedSpline``.

The module also holds the ONE conversion of duck-typed FE operands (``fe_matrix`` / ``as_device_csr`` /
``as_device_vector``) that ``extractMatrix`` / ``extractVector`` and the streamed engine share.
"""
import ctypes as C

import numpy

from . import _lib
from ._lib import check, handle, c_f64p, c_i32p, c_i64p
from .device import DeviceCSR, DeviceVector

DECLINED = 100


# ---- duck-typed operands ---------------------------------------------------------------------------------------------
def fe_matrix(A):
    """An FE matrix as the PtAP routes take it: a ``DeviceCSR``, a ``LazyFEMatrix`` or a scipy sparse matrix pass through;
    a PETSc-like object -- one with ``.mat()`` (dolfin ``PETScMatrix``) or itself with ``.getValuesCSR()`` and
    ``.getSize()`` (petsc4py ``Mat``) -- and a dense 2-D array become scipy CSR.  Anything else: ``TypeError``."""
    import scipy.sparse as sp
    from .implicit import LazyFEMatrix
    if isinstance(A, (DeviceCSR, LazyFEMatrix)) or sp.issparse(A):
        return A
    if hasattr(A, "mat") and callable(A.mat):
        A = A.mat()
    if hasattr(A, "getValuesCSR") and hasattr(A, "getSize"):
        indptr, indices, data = A.getValuesCSR()
        shape = tuple(int(v) for v in A.getSize())
        return sp.csr_matrix((numpy.asarray(data, dtype=numpy.float64), numpy.asarray(indices), numpy.asarray(indptr)),
                             shape=shape)
    if isinstance(A, numpy.ndarray) and A.ndim == 2:
        return sp.csr_matrix(A)
    raise TypeError("extractMatrix: a DeviceCSR, a scipy sparse matrix, a LazyFEMatrix or a PETSc-like matrix "
                    "(.mat() / .getValuesCSR() and .getSize()) is expected, not %s" % type(A).__name__)


def as_device_csr(A):
    """``fe_matrix(A)`` on the device (a ``LazyFEMatrix`` has no resident form: ``TypeError``)"""
    A = fe_matrix(A)
    if isinstance(A, DeviceCSR):
        return A
    if not hasattr(A, "tocsr"):
        raise TypeError("a LazyFEMatrix has no resident form")
    return DeviceCSR.from_scipy(A)


def as_device_vector(b):
    """An FE vector on the device: a ``DeviceVector`` as it is, a ``Function`` by its ``.vector()``, a PETSc-like object
    -- one with ``.vec()`` or itself with ``.getArray()`` --, one with ``.get_local()``, or an array (uploaded)."""
    if isinstance(b, DeviceVector):
        return b
    if hasattr(b, "vector") and callable(b.vector):
        return as_device_vector(b.vector())
    if hasattr(b, "vec") and callable(b.vec):
        b = b.vec()
    if hasattr(b, "getArray"):
        return DeviceVector(data=numpy.asarray(b.getArray(), dtype=numpy.float64))
    if hasattr(b, "get_local"):
        return DeviceVector(data=numpy.asarray(b.get_local(), dtype=numpy.float64))
    return DeviceVector(data=numpy.asarray(b, dtype=numpy.float64))


# ---- the caller's order ----------------------------------------------------------------------------------------------
class FEOrder(object):
    """The caller's FE dof order as a permutation of the node grid, resident on the device.  ``grid_of_fe[i]`` is the
    grid index of the caller's row i, ``fe_of_grid`` its inverse.  ``is_identity``: the caller numbers like the grid
    (then no operand is copied); ``max_snap``: the largest distance between a coordinate handed in and its node."""

    def __init__(self, _handle):
        self._h = _handle
        n, ident, snap = C.c_int64(), C.c_int(), C.c_double()
        check(_lib.lib().tg_feorder_info(self._h, C.byref(n), C.byref(ident), C.byref(snap)), "tg_feorder_info")
        self.n, self.is_identity, self.max_snap = int(n.value), bool(ident.value), float(snap.value)

    def __del__(self):
        try:
            if self._h:
                _lib.lib().tg_feorder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @staticmethod
    def _finish(rc, h, what):
        if rc == DECLINED:
            raise ValueError(_lib.lib().tg_last_error().decode())
        check(rc, what)
        return FEOrder(h)

    @staticmethod
    def locate(field_axes, x, fields=None, tol=1e-6):
        """The order of the rows whose node coordinates are ``x`` [nrows x d] on the space whose field f lives on the tensor
        grid of the axes ``field_axes[f]`` (d ascending arrays).  ``fields``: field of every row (needed with several
        fields).  A coordinate is accepted within ``tol`` x the smallest spacing of its axis.  ``ValueError`` with the
        reason (first offending row) when ``x`` is not a permutation of the node grid."""
        L = _lib.lib()
        nf = len(field_axes)
        d = len(field_axes[0])
        axes = [numpy.ascontiguousarray(a, dtype=numpy.float64) for fa in field_axes for a in fa]
        if any(len(fa) != d for fa in field_axes):
            raise ValueError("FEOrder.locate: every field needs %d axes" % d)
        x = numpy.ascontiguousarray(x, dtype=numpy.float64)
        if x.ndim == 1 and d == 1:
            x = x.reshape(-1, 1)
        if x.ndim != 2 or x.shape[1] != d:
            raise ValueError("FEOrder.locate: node coordinates of shape [rows, %d] are expected, got %s" % (d, x.shape))
        f = None
        if fields is not None:
            f = numpy.ascontiguousarray(fields, dtype=numpy.int32).reshape(-1)
            if f.shape[0] != x.shape[0]:
                raise ValueError("FEOrder.locate: %d field labels for %d rows" % (f.shape[0], x.shape[0]))
        elif nf > 1:
            raise ValueError("FEOrder.locate: the field of every row is needed when the space has several fields")
        lens = numpy.array([a.shape[0] for a in axes], dtype=numpy.int64)
        ptrs = (c_f64p * len(axes))(*[a.ctypes.data_as(c_f64p) for a in axes])
        h = handle()
        rc = L.tg_nodes_locate(d, nf, lens.ctypes.data_as(c_i64p), ptrs, x.ctypes.data_as(c_f64p),
                               f.ctypes.data_as(c_i32p) if f is not None else None, x.shape[0], float(tol), C.byref(h))
        return FEOrder._finish(rc, h, "tg_nodes_locate")

    @staticmethod
    def from_permutation(grid_of_fe):
        """The order given by ``grid_of_fe`` itself (``ValueError`` when it is no permutation of 0..n-1)"""
        g = numpy.ascontiguousarray(grid_of_fe, dtype=numpy.int32).reshape(-1)
        h = handle()
        rc = _lib.lib().tg_feorder_from_perm(g.ctypes.data_as(c_i32p), g.shape[0], C.byref(h))
        return FEOrder._finish(rc, h, "tg_feorder_from_perm")

    def _download(self, which):
        out = numpy.empty(self.n, dtype=numpy.int32)
        p = out.ctypes.data_as(c_i32p)
        check(_lib.lib().tg_feorder_download(self._h, p if which == 0 else None, p if which == 1 else None),
              "tg_feorder_download")
        return out

    @property
    def grid_of_fe(self):
        """host copy (int32) of the grid index of every caller row"""
        return self._download(0)

    @property
    def fe_of_grid(self):
        """host copy (int32) of the caller row of every grid index"""
        return self._download(1)

    def _permute(self, vec, out, to_caller):
        vec = as_device_vector(vec)
        if self.is_identity and out is None:
            return vec
        if out is None:
            out = DeviceVector(self.n, zero=False)
        if self.is_identity:
            if out is not vec:
                out[:] = vec
            return out
        check(_lib.lib().tg_vec_permute(self._h, vec._h, out._h, int(to_caller)), "tg_vec_permute")
        return out

    def to_grid(self, vec, out=None):
        """``vec`` in the caller's order -> grid order: y[grid_of_fe[i]] = vec[i] (the vector itself for the identity)"""
        return self._permute(vec, out, 0)

    def to_caller(self, vec, out=None):
        """``vec`` in grid order -> the caller's order: y[i] = vec[grid_of_fe[i]], into ``out`` when given"""
        return self._permute(vec, out, 1)

    def permute_matrix(self, A, inverse=False):
        """A on the caller's rows and columns -> grid order: B[grid_of_fe[i], grid_of_fe[j]] = A[i, j], values bit for bit,
        canonical CSR (``inverse``: grid order -> the caller's).  The matrix itself for the identity."""
        A = as_device_csr(A)
        if A.shape != (self.n, self.n):
            raise ValueError("FEOrder.permute_matrix: a %d x %d matrix is expected, got %d x %d" % ((self.n, self.n) + A.shape))
        if self.is_identity:
            return A
        h = handle()
        check(_lib.lib().tg_csr_permute_sym(self._h, A._h, int(bool(inverse)), C.byref(h)), "tg_csr_permute_sym")
        return DeviceCSR(h)
