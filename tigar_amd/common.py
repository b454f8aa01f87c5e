"""
The ``common`` module of tigar_amd: the reference's abstractions for generating extraction
data and using it in analysis (tIGAr/common.py), re-implemented MI355X-first.

What is kept: the ``AbstractExtractionGenerator`` / ``AbstractCoordinateChartSpline`` /
``AbstractMultiFieldSpline`` / ``EqualOrderSpline`` / ``FieldListSpline`` class tree, the
``AbstractScalarBasis`` / ``AbstractControlMesh`` plug-in interfaces, and
``ExtractedSpline`` with ``extractVector`` / ``extractMatrix`` / ``solveLinearSystem`` /
``setSolverOptions`` and the duck-typed ``linearSolver.solve(A, x, b)`` seam.

What changes: FEniCS objects are replaced by device-resident ones (``DeviceCSR`` for
``PETScMatrix``, ``DeviceVector`` for ``PETScVector``, ``TensorFunctionSpace`` for
``FunctionSpace`` on the implicit Q_p node grid).  FE assembly of forms is FEniCS's job
and is NOT part of this path; ``extractMatrix`` / ``extractVector`` accept any FE matrix /
vector on ``V`` (scipy.sparse / numpy inputs are uploaded).  Errors raise exceptions
instead of the reference's ``print("ERROR"); exit()``.
"""
import abc
import os
import sys
import time
import numpy
from numpy import array, zeros, arange

from . import device as _dev
from . import direct_plan as _plan
from .device import DeviceCSR, DeviceVector
from .feorder import FEOrder, as_device_csr as _as_device_csr, as_device_vector as _as_device_vector, fe_matrix as _fe_matrix

# ---- module-level configuration, same names as tIGAr/common.py:35-84 ---------------------
mpisize = int(os.environ.get("WORLD_SIZE", "1"))
mpirank = int(os.environ.get("RANK", "0"))


class _Comm(object):
    """Stand-in for an MPI communicator handle: one process per GPU.  ``transport`` is the host-side message
    layer (``tigar_amd.launch.Transport``), ``device()`` the device communicator of the Krylov solve (RCCL over
    xGMI, or host-staged where ranks share a GPU); both are created on first use from the launcher's
    environment (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT)."""

    def __init__(self, size, rank, transport=None, device_comm=None):
        self.size, self.rank = size, rank
        self._transport, self._device = transport, device_comm

    def transport(self):
        if self._transport is None:
            from .launch import SocketTransport, Transport
            self._transport = SocketTransport(self.rank, self.size) if self.size > 1 else Transport()
        return self._transport

    def device(self):
        if self.size > 1 and self._device is None:
            from .launch import device_comm
            self._device = device_comm(self.transport())
        return self._device

    def barrier(self):
        self.transport().barrier()


worldcomm = _Comm(mpisize, mpirank)
selfcomm = _Comm(1, 0)

INDEX_TYPE = 'int32'
DEFAULT_PREALLOC = 500
DEFAULT_DO_PERMUTATION = mpisize > 8
DEFAULT_BASIS_FUNC_IGNORE_EPS = 1e-15
EXTRACTION_DATA_FILE = "extraction-data.h5"
EXTRACTION_DATA_NPZ = "extraction-data.npz"       # what rounds 1-2 wrote in place of the HDF5 file (still read)
EXTRACTION_H5_PRIVATE = "/tigar_amd"               # group of extraction-data.h5 with this package's node-set description
EXTRACTION_INFO_FILE = "extraction-info.txt"
EXTRACTION_H5_MESH_NAME = "/mesh"


def EXTRACTION_H5_CONTROL_FUNC_NAME(dim):
    return "/control" + str(dim)


EXTRACTION_ZERO_DOFS_FILE = "zero-dofs.dat"
EXTRACTION_MAT_FILE = "extraction-mat.dat"
EXTRACTION_MAT_FILE_CTRL = "extraction-mat-ctrl.dat"
USE_DG_DEFAULT = True
USE_RECT_ELEM_DEFAULT = True
# The reference's FORM_MT=False trades speed for memory; on the GPU the explicit transpose is
# what makes M^T b and M^T A M scatter-free and deterministic, so it is always formed.
FORM_MT = True

DOLFIN_EPS = 3.0e-16


def generateMeshXMLFileName(comm):
    """name of the scratch mesh file of a communicator / rank pair (tIGAr/common.py:88-93; the product writes no such
    file -- the node grids are never serialised as XML -- but scripts that clean up after the reference call this)"""
    import hashlib
    s = repr(comm) + repr(getattr(comm, "rank", 0))
    return "mesh-" + str(hashlib.md5(s.encode("utf-8")).hexdigest()) + ".xml"


def near(a, b, eps=DOLFIN_EPS):
    """dolfin.near: |a-b| <= eps."""
    return abs(a - b) <= eps


_GAUSS_RULES = {
    1: ((0.0,), (2.0,)),
    2: ((-0.5773502691896257645091488, 0.5773502691896257645091488), (1.0, 1.0)),
    3: ((-0.77459666924148337703585308, 0.0, 0.77459666924148337703585308),
        (0.55555555555555555555555556, 0.88888888888888888888888889, 0.55555555555555555555555556)),
    4: ((-0.86113631159405257524, -0.33998104358485626481, 0.33998104358485626481, 0.86113631159405257524),
        (0.34785484513745385736, 0.65214515486254614264, 0.65214515486254614264, 0.34785484513745385736)),
}


def getQuadRule(n):
    """(points, weights) of the ``n``-point Gauss rule on (-1, 1) as lists of plain floats, n = 1..4
    (tIGAr/calculusUtils.py:412-457; through-thickness integration of the Kirchhoff-Love shell laws)"""
    if n not in _GAUSS_RULES:
        raise ValueError("getQuadRule: %r quadrature points; rules of 1 to 4 points are provided" % (n,))
    xi, w = _GAUSS_RULES[n]
    return list(xi), list(w)


def getQuadRuleInterval(n, L):
    """the ``n``-point rule on (-L/2, L/2) (tIGAr/calculusUtils.py:459-470)"""
    xi_hat, w_hat = getQuadRule(n)
    return [L * x / 2.0 for x in xi_hat], [L * w / 2.0 for w in w_hat]


# ---- FE-side stand-ins ------------------------------------------------------------------
class TensorNodeGrid(object):
    """The "mesh" of the extraction: a tensor-product grid of Lagrange nodes on the knot
    mesh (replaces the dolfin mesh of tIGAr/BSplines.py:505-569)."""

    def __init__(self, axes, vertices, degree, dg=False):
        self.axes = [numpy.ascontiguousarray(a, dtype=numpy.float64) for a in axes]
        self.vertices = vertices
        self.degree = degree
        self.dg = dg

    def dim(self):
        return len(self.axes)

    def shape(self):
        return [len(a) for a in self.axes]

    def num_nodes(self):
        n = 1
        for a in self.axes:
            n *= len(a)
        return n

    def coordinates(self):
        """[num_nodes, dim] parametric node coordinates, direction 0 fastest."""
        grids = numpy.meshgrid(*self.axes, indexing="ij")
        return numpy.stack([g.ravel(order="F") for g in grids], axis=1)


class MultiPatchNodeGrid(object):
    """Node set of a ``MultiBSpline``: the patches' node grids side by side, patch ``i`` shifted
    by 2*i along direction 0 (the reference's multi-patch mesh of disconnected elements,
    tIGAr/BSplines.py:734-860; each patch keeps element-local nodes)."""

    def __init__(self, patches):
        self.patches = list(patches)
        self.degree = self.patches[0].degree
        self.dg = True

    def dim(self):
        return self.patches[0].dim()

    def num_nodes(self):
        return sum(g.num_nodes() for g in self.patches)

    def coordinates(self):
        out = []
        for i, g in enumerate(self.patches):
            X = g.coordinates().copy()
            X[:, 0] += 2.0 * float(i)
            out.append(X)
        return numpy.vstack(out)


def _grid_to_arrays(g, key, data):
    """node grid -> entries of the ``extraction-data.npz`` archive under the prefix ``key`` (written by
    ``writeExtraction``, read back by ``_grid_from_arrays``)"""
    if isinstance(g, TensorNodeGrid):
        data[key + "_kind"] = numpy.array("tensor")
        data[key + "_degree"] = numpy.int64(g.degree)
        data[key + "_dg"] = numpy.int64(1 if g.dg else 0)
        data[key + "_dim"] = numpy.int64(g.dim())
        for k in range(g.dim()):
            data["%s_axis%d" % (key, k)] = numpy.asarray(g.axes[k])
            data["%s_vert%d" % (key, k)] = numpy.asarray(g.vertices[k], dtype=numpy.float64)
    elif isinstance(g, MultiPatchNodeGrid):
        data[key + "_kind"] = numpy.array("multipatch")
        data[key + "_npatches"] = numpy.int64(len(g.patches))
        for i, gp in enumerate(g.patches):
            _grid_to_arrays(gp, "%s_patch%d" % (key, i), data)
    elif type(g).__name__ == "BezierElementNodeGrid":
        data[key + "_kind"] = numpy.array("bezier")
        data[key + "_nel"] = numpy.int64(g.nel)
        data[key + "_degree"] = numpy.int64(g.degree)
    else:
        raise NotImplementedError("writeExtraction: node grid of type %s has no archive form" % type(g).__name__)


def _grid_from_arrays(data, key):
    kind = str(data[key + "_kind"]) if key + "_kind" in data else "tensor"       # (archives of round 1: tensor grids only)
    if kind == "tensor":
        dim = int(data[key + "_dim"])
        return TensorNodeGrid([data["%s_axis%d" % (key, k)] for k in range(dim)],
                              [data["%s_vert%d" % (key, k)] for k in range(dim)],
                              int(data[key + "_degree"]), bool(int(data[key + "_dg"])))
    if kind == "multipatch":
        return MultiPatchNodeGrid([_grid_from_arrays(data, "%s_patch%d" % (key, i))
                                   for i in range(int(data[key + "_npatches"]))])
    if kind == "bezier":
        from .RhinoTSplines import BezierElementNodeGrid
        return BezierElementNodeGrid(int(data[key + "_nel"]), int(data[key + "_degree"]))
    raise ValueError("extraction-data.npz: unknown node grid kind %r" % kind)


_CELL_NAMES = {1: "interval", 2: "quadrilateral", 3: "hexahedron"}


def _knot_mesh_arrays(g):
    """(coordinates [nv, d], topology [ncells, 2^d]) of the knot mesh under a tensor node grid: vertices and cells with
    direction 0 fastest, the vertices of a cell in lexicographic order -- the content of ``/mesh`` in extraction-data.h5
    (tIGAr/common.py:463).  The GROUP layout is dolfin's; whether dolfin's own quadrilateral / hexahedral meshes order
    the vertices of a cell this way has not been checked against dolfin (absent here), and nothing in this package
    depends on it: the node sets are rebuilt from the group ``/tigar_amd``."""
    d = g.dim()
    verts = [numpy.asarray(v, dtype=numpy.float64) for v in g.vertices]
    nv = [len(v) for v in verts]
    grids = numpy.meshgrid(*verts, indexing="ij")
    X = numpy.stack([q.ravel(order="F") for q in grids], axis=1)
    stride = numpy.cumprod([1] + nv[:-1])
    cells = numpy.meshgrid(*[numpy.arange(n - 1, dtype=numpy.int64) for n in nv], indexing="ij")
    base = sum(c.ravel(order="F") * int(stride[k]) for k, c in enumerate(cells))
    corners = numpy.zeros(1, dtype=numpy.int64)
    for k in range(d):                                 # lexicographic corners, direction 0 fastest
        corners = numpy.concatenate([corners, corners + int(stride[k])])
    return X, base[:, None] + corners[None, :]


def _kron_sum_is_symmetric(factors):
    """True when sum_t kron(F_t[d-1], ..., F_t[0]) is symmetric because of its 1-D factors: every term is a product of
    symmetric matrices, or its transpose (factor by factor) is another term of the sum (C^T x C + C x C^T).  1-D matrices:
    a few thousand entries, compared on the host."""
    if not factors:
        return False
    try:
        import scipy.sparse as _sp
        terms = [[_sp.csr_matrix(F) for F in t] for t in factors]

        def same(A, B):
            if A.shape != B.shape:
                return False
            D = abs(A - B)
            return (D.max() if D.nnz else 0.0) <= 1e-13 * max(abs(A).max() if A.nnz else 0.0, 1e-300)
        left = list(range(len(terms)))
        while left:
            t = left.pop(0)
            if all(same(F, F.T.tocsr()) for F in terms[t]):
                continue
            mate = next((u for u in left if len(terms[u]) == len(terms[t]) and
                         all(same(G, F.T.tocsr()) for F, G in zip(terms[t], terms[u]))), None)
            if mate is None:
                return False
            left.remove(mate)
        return True
    except Exception:
        return False


def _cell_dofs_arrays(g):
    """[ncells, (p+1)^d] node numbers of every knot-mesh cell, in this package's numbering (direction 0 fastest; a dolfin
    ``FunctionSpace`` on the same mesh numbers them its own way, which cannot be reproduced without dolfin)."""
    d, p = g.dim(), int(g.degree)
    nn = g.shape()
    step = p + 1 if g.dg else p
    nel = [(n // (p + 1)) if g.dg else ((n - 1) // max(p, 1)) for n in nn] if p > 0 else [n for n in nn]
    stride = numpy.cumprod([1] + nn[:-1])
    cells = numpy.meshgrid(*[numpy.arange(n, dtype=numpy.int64) for n in nel], indexing="ij")
    base = sum(c.ravel(order="F") * int(step * stride[k]) for k, c in enumerate(cells))
    loc = numpy.zeros(1, dtype=numpy.int64)
    for k in range(d):                                 # local nodes, direction 0 fastest
        loc = (loc[None, :] + (numpy.arange(p + 1, dtype=numpy.int64) * int(stride[k]))[:, None]).ravel()
    return base[:, None] + loc[None, :]


class _H5Archive(object):
    """the private group of extraction-data.h5 read like the npz archive of rounds 1-2 (arrays: datasets; strings and
    scalars: attributes of the group)"""

    def __init__(self, f):
        self.f = f

    def __contains__(self, key):
        return self.f.exists(EXTRACTION_H5_PRIVATE + "/" + key) or self.f.has_attr(EXTRACTION_H5_PRIVATE, key)

    def __getitem__(self, key):
        if self.f.exists(EXTRACTION_H5_PRIVATE + "/" + key):
            return self.f.read_dataset(EXTRACTION_H5_PRIVATE + "/" + key)
        if self.f.has_attr(EXTRACTION_H5_PRIVATE, key):
            return self.f.read_attr(EXTRACTION_H5_PRIVATE, key)
        raise KeyError(key)


class TensorFunctionSpace(object):
    """Stand-in for dolfin ``FunctionSpace``: ``nfields`` scalar Lagrange (or DG) fields
    on node grids that share one knot mesh.  Dofs are field-major, nodes lexicographic
    (dolfin's own numbering is unobservable downstream: K, M^T b and M U are invariant
    under FE row permutations -- SURVEY.md section 7 hard part 3)."""

    def __init__(self, grids, element):
        self.grids = list(grids)
        self.element = element

    def num_sub_spaces(self):
        return len(self.grids) if len(self.grids) > 1 else 0

    def dim(self):
        return sum(g.num_nodes() for g in self.grids)

    def field_offset(self, field):
        return sum(g.num_nodes() for g in self.grids[:field])

    def tabulate_dof_coordinates(self):
        """node coordinates of the dofs: the caller's array once ``setFENodes`` has taken it, else the node grid's"""
        nodes = self.__dict__.get("_fe_nodes")
        if nodes is not None:
            return nodes
        return numpy.vstack([g.coordinates() for g in self.grids])


class Function(object):
    """Stand-in for dolfin ``Function``: FE coefficients in HBM."""

    def __init__(self, V, local_range=None, vector=None):
        self.V = V
        # with several ranks a function holds the FE rows [r0, r1) its rank owns (set by the solve)
        self.local_range = local_range
        # (several fields with several ranks: one range per field, a list of (r0, r1))
        if local_range is not None and len(local_range) and isinstance(local_range[0], (tuple, list)):
            nloc = sum(int(b) - int(a) for a, b in local_range)
        else:
            nloc = V.dim() if local_range is None else local_range[1] - local_range[0]
        self._vec = vector if vector is not None else DeviceVector(nloc)
        self._ghoster = None          # set by the spline that drives a distributed solve (ExtractedSpline.ghostedVector)

    def vector(self):
        return self._vec

    def ghosted(self):
        """FE coefficients as a vector of the full length of V, valid on every row the forms of THIS rank read: its own
        rows plus the ghost rows held by the z-neighbours (dolfin's ghost update of a distributed Function [ext]; the
        reference's forms read the ghosted vector after ``u.assign``, tIGAr/common.py:1343).  One rank: the vector itself.
        The exchange happens ONCE per assembly: the spline that drives the solve stamps its assemblies
        (``ExtractedSpline._ghost_epoch``) and the ghosted vector is kept until the stamp changes -- the forms ask for it once
        per row block, and the number of row blocks differs from rank to rank (the exchanges of z-neighbours
        would no longer pair up)."""
        if self.local_range is None:
            return self._vec
        if self._ghoster is None:
            raise RuntimeError("a rank-local Function can only be read by forms after the spline that owns it has been "
                               "asked for a ghost update (ExtractedSpline.ghostedVector / solveNonlinearVariationalProblem)")
        owner = getattr(self._ghoster, "__self__", None)
        epoch = getattr(owner, "_ghost_epoch", None)
        cached = self.__dict__.get("_ghost_cache")
        if epoch is not None and cached is not None and cached[0] == epoch and cached[1] is self._vec:
            return cached[2]
        g = self._ghoster(self)
        if epoch is not None:
            self.__dict__["_ghost_cache"] = (epoch, self._vec, g)
        return g

    def invalidate_ghosts(self):
        """Forget the ghost rows fetched for the current assembly: call after changing the coefficients in place outside the
        drivers (``vector().axpy`` / ``set_local``) when a form, functional or error norm reads the function next --
        ``solveLinearSystem`` and the Newton update do it themselves."""
        self.__dict__.pop("_ghost_cache", None)

    def function_space(self):
        return self.V

    def rename(self, name, label):
        """dolfin's ``Function.rename``: the name output files carry (``File << u``, the demos' ``F0`` ... ``F3``)"""
        self._name, self._label = str(name), str(label)

    def name(self):
        return self.__dict__.get("_name", "f")

    def label(self):
        return self.__dict__.get("_label", "")

    def split(self):
        """one ``Function`` per field: copies of the fields' nodal values, each on its field's scalar space, named
        ``name_i`` (dolfin's ``u.split(deepcopy=True)``; a scalar function gives one copy of itself)"""
        if self.local_range is not None:
            raise NotImplementedError("Function.split: a rank-local function is not supported")
        out, off = [], 0
        for i, g in enumerate(self.V.grids):
            fi = Function(TensorFunctionSpace([g], self.V.element))
            _dev.vec_copy_range(fi.vector(), 0, self._vec, off, g.num_nodes())
            off += g.num_nodes()
            fi.rename("%s_%d" % (self.name(), i) if len(self.V.grids) > 1 else self.name(), self.label())
            out.append(fi)
        return out


def multTranspose(M, b):
    """Returns ``M^T*b`` (tIGAr/common.py:97-109)."""
    return M.mult_transpose(_as_device_vector(b))


def generateIdentityPermutation(ownRange, comm=worldcomm):
    """Index array of the ownership range (tIGAr/common.py:114-128)."""
    return arange(ownRange[0], ownRange[1], dtype=INDEX_TYPE)


# ---- extraction generators -----------------------------------------------------------------
class AbstractExtractionGenerator(object):
    """
    Minimal set of functions needed to write extraction operators for a spline
    (tIGAr/common.py:130-502).
    """

    __metaclass__ = abc.ABCMeta

    def __init__(self, comm, *args, fe_nodes=None, fe_fields=None, fe_node_tol=1e-6):
        """``fe_nodes`` / ``fe_fields`` / ``fe_node_tol``: the caller's FE dof order, see ``setFENodes``"""
        if not isinstance(comm, _Comm):
            args = (comm,) + args
            self.comm = worldcomm
        else:
            self.comm = comm
        self.customSetup(args)
        self.genericSetup()
        self.feOrder = None
        if fe_nodes is not None:
            self.setFENodes(fe_nodes, fe_fields, fe_node_tol)

    def setFENodes(self, x, fields=None, tol=1e-6):
        """Takes the FE dof order of the caller: ``x`` [V.dim() x d] are the node coordinates of its dofs (what
        ``V.tabulate_dof_coordinates()`` returns in an FE library), ``fields`` the field of every row (the dofs of
        ``V.sub(f)``; needed with several fields).  The rows must be a permutation of the node grid: every coordinate within
        ``tol`` x the smallest node spacing of its axis from a node (a condition, not a measurement: anything below 0.5 is
        unambiguous), every node named once -- else ``ValueError`` with the first offending row and the reason.
        Afterwards ``V.tabulate_dof_coordinates()`` returns ``x``, ``feOrder`` is set, and an ``ExtractedSpline`` made from
        this generator takes FE matrices / vectors and returns FE functions in the caller's order.  ``M``, ``MT``,
        ``cpFuncs`` and ``writeExtraction`` stay in the order of the node grid."""
        if getattr(self.comm, "size", 1) > 1:
            raise NotImplementedError("setFENodes: a caller-ordered FE space on several ranks is not supported")
        grids = self.V.grids
        for f, g in enumerate(grids):
            if not isinstance(g, TensorNodeGrid) or not getattr(g, "axes", None):
                raise ValueError("setFENodes: field %d does not live on a TensorNodeGrid (multi-patch and T-spline node sets "
                                 "are no permutation of one tensor grid)" % f)
            if getattr(g, "dg", False):
                raise ValueError("setFENodes: field %d is discontinuous (DG): several dofs share a node, so coordinates do "
                                 "not name them" % f)
        d = grids[0].dim()
        x = numpy.array(x, dtype=numpy.float64)
        if x.ndim == 1 and d == 1:
            x = x.reshape(-1, 1)
        if x.ndim != 2 or x.shape[1] != d:
            raise ValueError("setFENodes: wrong shape: node coordinates [%d x %d] are expected, got %s"
                             % (self.V.dim(), d, x.shape))
        if len(grids) > 1 and fields is None:
            raise ValueError("setFENodes: fe_fields (the field of every row) is needed for a space of %d fields" % len(grids))
        self.feOrder = FEOrder.locate([g.axes for g in grids], x, fields, tol)
        self.V._fe_nodes = x
        return self.feOrder

    def getComm(self):
        return self.comm

    def useDG(self):
        return USE_DG_DEFAULT

    def extractionElement(self):
        return "DG" if self.useDG() else "Lagrange"

    @abc.abstractmethod
    def customSetup(self, args):
        return

    @abc.abstractmethod
    def getNFields(self):
        return

    @abc.abstractmethod
    def getHomogeneousCoordinate(self, node, direction):
        return

    @abc.abstractmethod
    def generateMesh(self):
        return

    @abc.abstractmethod
    def getDegree(self, field):
        return

    @abc.abstractmethod
    def getNcp(self, field):
        return

    @abc.abstractmethod
    def getNsd(self):
        return

    def globalDof(self, field, localDof):
        retval = localDof
        for i in range(0, field):
            retval += self.getNcp(i)
        return retval

    def generatePermutation(self):
        total = sum(self.getNcp(i) for i in range(self.getNFields()))
        return generateIdentityPermutation((0, total), self.comm)

    # ``zeroDofs`` is a plain Python list in the reference (tIGAr/common.py:254-282; user code appends to it).  Large
    # index sets (6 faces x 259^2 at cfg3) are kept as numpy chunks behind it: the list is only materialised when
    # somebody reads the attribute, the path itself takes ``zeroDofsArray()``.
    @property
    def zeroDofs(self):
        chunks = self.__dict__.get("_zero_chunks", [])
        if chunks:
            self.__dict__["_zero_list"] = self.__dict__.get("_zero_list", []) + numpy.concatenate(chunks).tolist()
            self.__dict__["_zero_chunks"] = []
        return self.__dict__.setdefault("_zero_list", [])

    @zeroDofs.setter
    def zeroDofs(self, value):
        # (``self.zeroDofs += [dof]`` hands back the very list the getter returned: keep it, do not copy it per append)
        if value is not self.__dict__.get("_zero_list"):
            self.__dict__["_zero_list"] = list(value)
        self.__dict__["_zero_chunks"] = []

    def zeroDofsArray(self):
        """all zero dofs so far, in insertion order (duplicates kept), as one int64 array"""
        parts = [numpy.asarray(self.__dict__.get("_zero_list", []), dtype=numpy.int64)] + \
            self.__dict__.get("_zero_chunks", [])
        return numpy.concatenate(parts) if len(parts) > 1 else parts[0]

    @staticmethod
    def _index_array(dofs):
        # a list made by getSideDofs carries its numpy twin until the list is edited (every mutating method of the list
        # drops it): no pass over 67 000 Python integers per face at 256^3
        src = getattr(dofs, "array", None)
        if src is not None and type(dofs).__name__ == "_IndexList" and len(src) == len(dofs):
            return src
        return numpy.asarray(dofs, dtype=numpy.int64).reshape(-1)

    def addZeroDofsGlobal(self, newDofs):
        self.__dict__.setdefault("_zero_chunks", []).append(numpy.array(self._index_array(newDofs), dtype=numpy.int64))

    def addZeroDofs(self, field, newDofs):
        off = self.globalDof(field, 0)
        self.__dict__.setdefault("_zero_chunks", []).append(self._index_array(newDofs) + off)

    def getPrealloc(self, control):
        return DEFAULT_PREALLOC

    def getIgnoreEps(self):
        return DEFAULT_BASIS_FUNC_IGNORE_EPS

    @abc.abstractmethod
    def generateM_control(self):
        return

    @abc.abstractmethod
    def generateM(self):
        return

    def _homogeneousCoordinateArray(self):
        """P[I, i] = getHomogeneousCoordinate(I, i) (loop of tIGAr/common.py:373-375),
        vectorised when the control mesh offers it."""
        cm = getattr(self, "getControlMesh", None)
        if cm is not None and hasattr(self.getControlMesh(), "getHomogeneousCoordinates"):
            return numpy.asarray(self.getControlMesh().getHomogeneousCoordinates(), dtype=numpy.float64)
        ncp = self.getNcp(-1)
        P = numpy.empty((ncp, self.nsd + 1))
        for I in range(ncp):
            for i in range(self.nsd + 1):
                P[I, i] = self.getHomogeneousCoordinate(I, i)
        return P

    def genericSetup(self):
        """Common setup (tIGAr/common.py:321-383): node grids in place of the FE mesh and
        function spaces, M_control, M, and the FE-nodal control functions
        cpFuncs[i] = M_control * P[:, i]."""
        self.mesh = self.generateMesh()
        self.nsd = self.getNsd()
        elem = self.extractionElement()
        dg = (elem == "DG")
        self.V_control = TensorFunctionSpace([self._fieldGrid(-1, dg)], elem)
        self.V = TensorFunctionSpace([self._fieldGrid(i, dg) for i in range(self.getNFields())], elem)
        self.M_control = self.generateM_control()
        self.M = self.generateM()
        self.MT = self.generateMT()
        self.M._T = self.MT           # M.mult_transpose() goes through the explicit transpose
        # Kronecker form of M (single tensor B-spline field, filter dropped only exact zeros):
        # enables the sum-factorised M^T A M of tigar_amd/kronptap.py
        self._kron = None
        self._kron_scalar = None           # several fields on ONE tensor basis (EqualOrderSpline(nFields > 1)): its tables
        self._kron_fields = None           # several fields on different tensor bases: one set of tables per field
        if getattr(self.M, "is_implicit", False) and hasattr(self.M, "kxs"):
            self._kron_fields = self.M.kxs       # diag(M_0, ..., M_{nF-1}) on different bases, never stored
        elif getattr(self.M, "is_implicit", False) and getattr(self.M, "nfields", 1) > 1:
            self._kron_scalar = self.M.kx        # diag(M_s, ..., M_s), never stored
        elif getattr(self.M, "is_implicit", False):
            self._kron = self.M.kx
        elif self.getNFields() == 1 and (0, 0) in self._fast_blocks or (self.M is self.M_control
                                                                          and (-1, 0) in self._fast_blocks):
            basis, grid = self._fast_blocks.get((0, 0), self._fast_blocks.get((-1, 0)))
            kx = self._kron_tables(basis, grid)
            if kx is not None and kx.is_exact_for(self.M.nnz, self.getIgnoreEps()):
                self._kron = kx
        elif self.getNFields() > 1 and not getattr(self.M, "is_implicit", False):
            # every field block built by the tensor kernels from the same basis on the same node grid, and each block
            # exactly the Kronecker product of its 1-D factors (entry count checked): M = diag(M_s, ..., M_s)
            keys = []
            offset = 0
            for f in range(self.getNFields()):
                keys.append((f, offset))
                offset += self.getNcp(f)
            if all(k in self._fast_blocks for k in keys):
                b0, g0 = self._fast_blocks[keys[0]]
                same = all(self._fast_blocks[k][0] is b0 and self._fast_blocks[k][1].axes is not None and
                           all(numpy.array_equal(a, b) for a, b in zip(self._fast_blocks[k][1].axes, g0.axes))
                           for k in keys)
                kx = self._kron_tables(b0, g0) if same else None
                if kx is not None and self.M.nnz == self.getNFields() * kx.nnz_product and \
                        kx.products_stay_above(self.getIgnoreEps()):
                    self._kron_scalar = kx
                if self._kron_scalar is None:
                    # fields on DIFFERENT tensor bases (FieldListSpline, the components of a compatible spline:
                    # tIGAr/common.py:1949-1970, tIGAr/compatibleSplines.py:21-101): M = diag(M_0, ..., M_{nF-1}), every
                    # block exactly the Kronecker product of its own 1-D factors (entry count checked)
                    kxs = [self._kron_tables(*self._fast_blocks[k]) for k in keys]
                    if all(kx is not None and kx.products_stay_above(self.getIgnoreEps()) for kx in kxs) and \
                            self.M.nnz == sum(kx.nnz_product for kx in kxs):
                        self._kron_fields = kxs
        self.cpFuncs = []
        cm = self.getControlMesh() if hasattr(self, "getControlMesh") else None
        P = None
        self._slab_engine = None
        if self.comm.size > 1 and getattr(self.M_control, "is_implicit", False):
            # several ranks: every rank evaluates the control functions on the FE rows it owns only
            # (the reference's cpFuncs are distributed dolfin Functions, tIGAr/common.py:367-380)
            from .dist import SlabHotPath
            kx = self.M_control.kx
            self._slab_engine = SlabHotPath(kx.basis, kx.grid, self.comm.rank, self.comm.size, self.comm.device(),
                                            sub_planes="auto", eps=self.M_control.eps, kx=kx)
        # M_control a Kronecker product (implicit, or stored and checked entry count against the product of the
        # 1-D counts) and the control net a tensor product of 1-D factors: so is every control function
        kx_c = None
        if cm is not None and hasattr(cm, "homogeneousCoordinateFactors"):
            if getattr(self.M_control, "is_implicit", False):
                kx_c = self.M_control.kx
            elif self._kron is not None and self.M is self.M_control:
                kx_c = self._kron
        separable = kx_c is not None
        self._cp_source = {"kx": kx_c if separable else (self.M_control.kx if getattr(self.M_control, "is_implicit", False) else None),
                           "separable": separable, "P": []}
        for i in range(self.nsd + 1):
            if separable:
                # (M_z g_z) (x) (M_y g_y) (x) (M_x g_x) -- one write pass over the FE rows this rank owns
                kx = kx_c
                facs = cm.homogeneousCoordinateFactors(i)
                fe1d = [kx.M1[k] @ numpy.asarray(facs[k], dtype=numpy.float64) for k in range(kx.d)]
                rng = self._slab_engine.mine["u_rows"] if self._slab_engine is not None else None
                self.cpFuncs += [Function(self.V_control, rng,
                                          vector=_dev.vec_tensor3(fe1d, 1.0, rng[0] if rng else None, rng[1] if rng else None))]
                continue
            if cm is not None and hasattr(cm, "homogeneousCoordinateDeviceVector"):
                Pi = cm.homogeneousCoordinateDeviceVector(i)      # built in HBM from 1-D factors
            else:
                if P is None:
                    P = self._homogeneousCoordinateArray()
                Pi = DeviceVector(data=P[:, i])
            self._cp_source["P"].append(Pi)
            if self._slab_engine is not None:
                f = Function(self.V_control, self._slab_engine.mine["u_rows"])
                f._vec = self._slab_engine._prolong_tensor(Pi, 0)
            else:
                f = Function(self.V_control)
                self.M_control.mult(Pi, f.vector())               # stays in HBM
            self.cpFuncs += [f]
        self.zeroDofs = []

    def controlFunctionWindow(self, fa, fb):
        """The nsd+1 control functions cpFuncs[i] = M_control P[:, i] (tIGAr/common.py:367-380) on the FE node planes
        [fa, fb) of the last parametric direction, as DeviceVectors -- what the forms of a rank read when they assemble a
        block of FE rows on a mapped patch.  Evaluated from the control net (replicated on every rank) through the rows
        of M_control that belong to the window: no rank needs another rank's part of the control functions.  The last
        two windows are kept (the matrix and the vector form of one sub-slab ask for the same one)."""
        key = (int(fa), int(fb))
        cache = self.__dict__.setdefault("_cp_windows", [])
        for k_, v_ in cache:
            if k_ == key:
                return v_
        src = self.__dict__.get("_cp_source") or {}
        kx = src.get("kx")
        if kx is None:
            raise NotImplementedError("control functions on a window of FE planes: tensor-product control mesh")
        pf = int(numpy.prod(kx.nfe[:-1], dtype=numpy.int64)) if kx.d > 1 else 1
        out = []
        if src["separable"]:
            cm = self.getControlMesh()
            for i in range(self.nsd + 1):
                facs = cm.homogeneousCoordinateFactors(i)
                fe1d = [kx.M1[k] @ numpy.asarray(facs[k], dtype=numpy.float64) for k in range(kx.d)]
                out.append(_dev.vec_tensor3(fe1d, 1.0, key[0] * pf, key[1] * pf))
        else:
            # rows [fa, fb) of the last 1-D factor name the dof planes [k_lo, k_hi): only those planes of the control net
            # go through the plane-local passes
            Mz = kx.M1[-1][key[0]:key[1]].tocsr()
            k_lo, k_hi = int(Mz.indices.min()), int(Mz.indices.max()) + 1
            pd = int(numpy.prod(kx.ncp[:-1], dtype=numpy.int64)) if kx.d > 1 else 1
            for Pi in src["P"]:
                x = DeviceVector((k_hi - k_lo) * pd)
                _dev.vec_copy_range(x, 0, Pi, k_lo * pd, (k_hi - k_lo) * pd)
                dims = list(kx.ncp[:-1]) + [k_hi - k_lo]
                t = x
                for k in range(kx.d - 1):
                    t = _dev.tensor_apply_1d(t, dims, k, kx.M1[k])
                    dims[k] = kx.nfe[k]
                out.append(_dev.tensor_apply_1d(t, dims, kx.d - 1, Mz, col_shift=k_lo))
        cache.append((key, out))
        del cache[:-2]
        return out

    def _fieldGrid(self, field, dg):
        """Node grid of one scalar field (degree getDegree(field) on the shared knot mesh)."""
        raise NotImplementedError

    def applyPermutation(self, nparts=None, fe_owner=None):
        """Renumbers the IGA dofs with ``generatePermutation`` (tIGAr/common.py:407-433): the columns of M move
        (MatPermute with the identity on the rows: new column j = old column perm[j]) and the zero dofs are renamed
        (the AO of :425-433: old dof a becomes the j with perm[j] = a).  With one part -- and for tensor patches in
        z-slabs, whose dof slabs already follow the FE slabs -- the permutation is the identity and nothing moves."""
        kw = {}
        if nparts is not None or fe_owner is not None:
            kw = {"nparts": nparts, "fe_owner": fe_owner}
        self.permutation = perm = numpy.asarray(self.generatePermutation(**kw), dtype=numpy.int64)
        if perm.size == 0 or numpy.array_equal(perm, numpy.arange(perm.size)):
            return
        new_of_old = numpy.empty(perm.size, dtype=numpy.int64)
        new_of_old[perm] = numpy.arange(perm.size)
        self.M = self.M.permute_columns(new_of_old)
        self.MT = self.M.transpose()
        self._kron = None                      # (M is no Kronecker product in the new numbering)
        self._kron_scalar = None
        self._kron_fields = None
        self._fast_blocks = {}
        self.zeroDofs = new_of_old[self.zeroDofsArray()].tolist()

    def writeExtraction(self, dirname, doPermutation=DEFAULT_DO_PERMUTATION, nparts=None):
        """Writes the extraction data to ``dirname`` with the reference's file names and formats
        (tIGAr/common.py:435-502): ``extraction-mat.dat`` / ``extraction-mat-ctrl.dat`` (PETSc binary
        Mat of M / M_control), ``zero-dofs.dat`` (PETSc binary IS), ``extraction-info.txt`` (nsd,
        element type, number of fields, then degree and ncp of the control field and of each field).
        ``extraction-data.h5`` is written through libhdf5 (``tigar_amd/h5io.py``) with the groups dolfin's ``HDF5File``
        writes (tIGAr/common.py:460-467): ``/mesh`` (``coordinates``, ``topology`` with its ``celltype``, ``cell_indices``;
        tensor node sets) and ``/control<i>`` (``vector_0``, ``cell_dofs``, ``x_cell_dofs``, ``cells``, the element's
        ``signature``) -- in THIS package's node numbering (dolfin's own cannot be reproduced without dolfin; the layout
        follows dolfin 2019's HDF5File and is not pinned against a dolfin-written file) -- plus the group ``/tigar_amd``
        with the node-set description ``initFromFilesystem`` rebuilds the function spaces from."""
        from . import petscio
        if doPermutation:
            self.applyPermutation(nparts=nparts)      # (nparts: the number of ranks that will read the directory)
        os.makedirs(dirname, exist_ok=True)
        petscio.write_mat(os.path.join(dirname, EXTRACTION_MAT_FILE), self.M.to_scipy())
        petscio.write_mat(os.path.join(dirname, EXTRACTION_MAT_FILE_CTRL), self.M_control.to_scipy())
        petscio.write_is(os.path.join(dirname, EXTRACTION_ZERO_DOFS_FILE), numpy.asarray(self.zeroDofs, dtype=INDEX_TYPE))
        fs = str(self.getNsd()) + "\n" + self.extractionElement() + "\n" + str(self.getNFields()) + "\n"
        for i in range(-1, self.getNFields()):
            fs += str(self.getDegree(i)) + "\n" + str(self.getNcp(i)) + "\n"
        with open(os.path.join(dirname, EXTRACTION_INFO_FILE), "w") as f:
            f.write(fs)
        data = {"nfields": numpy.int64(self.getNFields())}
        for name, V in (("control", self.V_control), ("fields", self.V)):
            data[name + "_ngrids"] = numpy.int64(len(V.grids))
            data[name + "_element"] = numpy.array(V.element)
            for gi, g in enumerate(V.grids):
                _grid_to_arrays(g, "%s_%d" % (name, gi), data)
        from . import h5io
        if not h5io.available():
            # no libhdf5 on this machine: the archive rounds 1-2 wrote (still read by ExtractedSpline(dirname))
            import warnings
            warnings.warn("libhdf5 not found (TIGAR_HDF5_LIB): writing %s instead of %s" % (EXTRACTION_DATA_NPZ, EXTRACTION_DATA_FILE))
            for i, fn in enumerate(self.cpFuncs):
                data["control%d" % i] = fn.vector().get_local()
            numpy.savez(os.path.join(dirname, EXTRACTION_DATA_NPZ), **data)
            return
        with h5io.H5File(os.path.join(dirname, EXTRACTION_DATA_FILE), "w") as f:
            g0 = self.V_control.grids[0]
            cell_dofs = None
            if isinstance(g0, TensorNodeGrid):
                X, topo = _knot_mesh_arrays(g0)
                f.create_group(EXTRACTION_H5_MESH_NAME)
                f.write_dataset(EXTRACTION_H5_MESH_NAME + "/coordinates", X)
                f.write_dataset(EXTRACTION_H5_MESH_NAME + "/topology", topo,
                                attrs={"celltype": _CELL_NAMES[g0.dim()], "partition": numpy.zeros(1, dtype=numpy.uint64)})
                f.write_dataset(EXTRACTION_H5_MESH_NAME + "/cell_indices", numpy.arange(topo.shape[0], dtype=numpy.int64))
                cell_dofs = _cell_dofs_arrays(g0)
                family = {1: ("Lagrange", "Discontinuous Lagrange"), 2: ("Q", "DQ"), 3: ("Q", "DQ")}[g0.dim()][1 if g0.dg else 0]
                signature = "FiniteElement('%s', %s, %d)" % (family, _CELL_NAMES[g0.dim()], int(g0.degree))
            for i, fn in enumerate(self.cpFuncs):
                name = EXTRACTION_H5_CONTROL_FUNC_NAME(i)
                f.create_group(name)
                f.write_dataset(name + "/vector_0", fn.vector().get_local(), attrs={"partition": numpy.zeros(1, dtype=numpy.uint64)})
                if cell_dofs is not None:
                    f.write_dataset(name + "/cell_dofs", cell_dofs.ravel())
                    f.write_dataset(name + "/x_cell_dofs", numpy.arange(cell_dofs.shape[0] + 1, dtype=numpy.int64) * cell_dofs.shape[1])
                    f.write_dataset(name + "/cells", numpy.arange(cell_dofs.shape[0], dtype=numpy.int64))
                    f.write_attr(name, "signature", signature)
            f.create_group(EXTRACTION_H5_PRIVATE)
            for k, v in data.items():
                v = numpy.asarray(v)
                if v.dtype.kind in "US":
                    f.write_attr(EXTRACTION_H5_PRIVATE, k, str(v))
                elif v.ndim == 0:
                    f.write_attr(EXTRACTION_H5_PRIVATE, k, v.astype(numpy.int64 if v.dtype.kind in "iub" else numpy.float64))
                else:
                    f.write_dataset(EXTRACTION_H5_PRIVATE + "/" + k, v.astype(numpy.int64 if v.dtype.kind in "iub" else numpy.float64))


class AbstractCoordinateChartSpline(AbstractExtractionGenerator):
    """Spline with a single parametric coordinate chart (tIGAr/common.py:1435-1669)."""

    @abc.abstractmethod
    def getNodesAndEvals(self, x, field):
        return

    def _generate_block(self, field, col_offset, ncols, grid, support_only=False):
        """Rows of the extraction matrix for one field: kernel path for tensor B-splines,
        host-loop triplet fallback for arbitrary AbstractScalarBasis plug-ins (seam b-2).
        ``support_only``: every function ``getNodesAndEvals`` returns is kept whatever its value (the pattern
        ``generatePermutation`` works on, tIGAr/common.py:1621-1629), always as a stored matrix."""
        basis = self.getScalarSpline(field) if hasattr(self, "getScalarSpline") else None
        eps = -1.0 if support_only else self.getIgnoreEps()
        from .BSplines import BSpline
        if isinstance(basis, BSpline) and type(basis).getNodesAndEvals is BSpline.getNodesAndEvals:
            if support_only:
                return _dev.extract_csr_tensor(basis.splines, grid.axes, col_offset, ncols, eps)
            self._fast_blocks[(field, col_offset)] = (basis, grid)
            if field == -1 and (self._single_shared_field() or self._fields_on_control_basis()):
                lazy = self._implicit_block(basis, grid, eps, several_fields=not self._single_shared_field())
                if lazy is not None:
                    return lazy
            # exact Kronecker form (every product of stored 1-D entries passes the filter, checked on the 1-D
            # tables; periodic directions included as long as a node names no function twice): pencil walk with
            # closed-form row starts, same entries bit for bit
            kx = self._kron_tables(basis, grid)
            if kx is not None and kx.products_stay_above(eps) and kx.columns_distinct() \
                    and os.environ.get("TIGAR_EXTRACT_KRON", "1") != "0":
                return _dev.kron3_csr(kx.M1, None, None, col_offset, ncols)
            return _dev.extract_csr_tensor(basis.splines, grid.axes, col_offset, ncols, eps)
        if hasattr(basis, "extractBlockOnDevice") and type(self).getNodesAndEvals is AbstractMultiFieldSpline.getNodesAndEvals:
            # bases that bring their own batched device evaluation (Rhino T-splines: csrc/tg_bezier.hip)
            return basis.extractBlockOnDevice(grid, col_offset, ncols, eps)
        from .BSplines import MultiBSpline
        if isinstance(basis, MultiBSpline) and isinstance(grid, MultiPatchNodeGrid):
            # patch by patch with the tensor kernel; rows stack, columns shift by the patch offsets
            blocks = [_dev.extract_csr_tensor(sp.splines, g.axes, col_offset + basis.doffsets[i], ncols, eps)
                      for i, (sp, g) in enumerate(zip(basis.splines, grid.patches))]
            return blocks[0] if len(blocks) == 1 else _dev.csr_vstack(blocks)
        # generic path: the reference's row loop (tIGAr/common.py:1554-1571)
        X = grid.coordinates()
        rows, cols, vals = [], [], []
        for I in range(X.shape[0]):
            for c, v in self.getNodesAndEvals(X[I], field):
                rows.append(I)
                cols.append(int(c) + col_offset)
                vals.append(float(v))
        return _dev.csr_from_triplets(X.shape[0], ncols, rows, cols, vals, eps)

    def _single_shared_field(self):
        """one unknown field on the control mesh's own basis: M is M_control"""
        return False

    def _fields_on_control_basis(self):
        """every unknown field is discretised with the control mesh's scalar basis (EqualOrderSpline): M is the block
        diagonal of M_control"""
        return False

    def _kron_tables(self, basis, grid):
        """1-D extraction tables of a tensor basis on its grid (``KronExtraction``), built once per (basis, grid)"""
        cache = self.__dict__.setdefault("_kx_cache", {})
        key = (id(basis), id(grid))
        if key not in cache:
            from .kronptap import KronExtraction
            # the fields of an equal-order spline (and its control field) sit on node grids of equal content: one set of
            # 1-D tables serves them all (each KronExtraction evaluates the basis at every node of every direction)
            twin = None
            for (kx2, b2, g2) in cache.values():
                if kx2 is not None and b2 is basis and g2.degree == grid.degree and bool(g2.dg) == bool(grid.dg) and \
                        len(g2.axes) == len(grid.axes) and all(numpy.array_equal(a, b) for a, b in zip(g2.axes, grid.axes)):
                    twin = kx2
                    break
            try:
                cache[key] = (twin if twin is not None else KronExtraction(basis, grid), basis, grid)   # (objects kept alive with the key)
            except Exception:
                cache[key] = (None, basis, grid)
        return cache[key][0]

    def _implicit_block(self, basis, grid, eps, several_fields=False):
        """``ImplicitExtraction`` in place of the CSR block when M (and M^T) would not fit beside the rest of
        the path -- 24 B per entry against a third of the free HBM -- or when the patch is spread over several
        ranks (no rank ever holds all rows); TIGAR_IMPLICIT_M=1/0 forces / forbids it.  Only offered when M
        is exactly the Kronecker product of its 1-D factors (the filter of tIGAr/common.py:1569 dropped
        nothing but exact zeros)."""
        from .kronptap import KronExtraction
        from .implicit import ImplicitExtraction
        env = os.environ.get("TIGAR_IMPLICIT_M")
        if env == "0":
            return None
        kx = self._kron_tables(basis, grid)
        if kx is None or not kx.products_stay_above(eps):
            return None
        if self.comm.size == 1:
            # the sub-slab engine behind an implicit M cuts the LAST direction into slabs and needs an open knot vector
            # there (tigar_amd/dist.py: ZSlabLayout); a patch that is periodic in that direction keeps a stored M on one
            # rank -- also when TIGAR_IMPLICIT_M=1 asks for the implicit one
            s_last = kx.basis.splines[-1]
            kn, pl = numpy.asarray(s_last.knots, dtype=float), int(s_last.p)
            if not (numpy.all(kn[:pl + 1] == kn[0]) and numpy.all(kn[-(pl + 1):] == kn[-1])):
                return None
        if env != "1" and self.comm.size == 1:
            free_b = _dev.mem_info()[0] + _dev.pool_stats()[0]      # idle blocks of the caching allocator count as free
            nf = self.getNFields() if several_fields else 1
            if several_fields or 24.0 * nf * kx.nnz_product + 16.0 * nf * grid.num_nodes() <= free_b / 3.0:
                return None                     # (several fields on one rank: stored, block by block as before)
        return ImplicitExtraction(kx, eps)

    def generateM_control(self):
        """Extraction matrix of the scalar space of the control functions
        (tIGAr/common.py:1460-1514)."""
        self._fast_blocks = {}
        return self._generate_block(-1, 0, self.getNcp(-1), self.V_control.grids[0])

    def generateMT(self):
        """Explicit transpose of ``M`` (the reference's optional ``MT``, FORM_MT at
        tIGAr/common.py:84,358-360).  For tensor B-spline fields it is written directly by the
        transposed extraction kernel; otherwise ``M`` is transposed on the device."""
        nf = self.getNFields()
        if getattr(self.M, "is_implicit", False):
            return self.M.transpose()
        def transposed_block(basis, grid, fe_offset, fe_total):
            kx = self._kron_tables(basis, grid)
            if kx is not None and kx.products_stay_above(self.getIgnoreEps()) and kx.columns_distinct() \
                    and os.environ.get("TIGAR_EXTRACT_KRON", "1") != "0":
                return _dev.kron3_csr(kx.M1T, None, None, fe_offset, fe_total)
            return _dev.extract_csr_tensor_t(basis.splines, grid.axes, fe_offset, fe_total, self.getIgnoreEps())
        if self.M is self.M_control and (-1, 0) in self._fast_blocks:
            basis, grid = self._fast_blocks[(-1, 0)]
            return transposed_block(basis, grid, 0, grid.num_nodes())
        blocks = []
        offset = 0
        fe_total = self.V.dim()
        for field in range(nf):
            key = (field, offset)
            if key not in self._fast_blocks:
                return self.M.transpose()
            basis, grid = self._fast_blocks[key]
            blocks.append(transposed_block(basis, grid, self.V.field_offset(field), fe_total))
            offset += self.getNcp(field)
        return blocks[0] if len(blocks) == 1 else _dev.csr_vstack(blocks)

    def generateM(self, support_only=False):
        """Extraction matrix of the mixed space of all unknown fields
        (tIGAr/common.py:1516-1578): one row block per field, column offset = sum of the
        previous fields' ncp."""
        totalDofs = sum(self.getNcp(i) for i in range(self.getNFields()))
        if self.getNFields() > 1 and not support_only and self._fields_on_control_basis() and \
                getattr(getattr(self, "M_control", None), "is_implicit", False):
            # several ranks (or TIGAR_IMPLICIT_M=1): no rank holds all rows -- the block diagonal of the implicit
            # scalar operator stands in for the matrix
            from .implicit import BlockImplicitExtraction
            return BlockImplicitExtraction(self.M_control.kx, self.getNFields(), self.M_control.eps)
        if self.getNFields() > 1 and not support_only and not self._fields_on_control_basis():
            lazy = self._implicit_field_list()
            if lazy is not None:
                return lazy
        blocks = []
        offset = 0
        for field in range(self.getNFields()):
            blocks.append(self._generate_block(field, offset, totalDofs, self.V.grids[field], support_only))
            offset += self.getNcp(field)
        return blocks[0] if len(blocks) == 1 else _dev.csr_vstack(blocks)

    def _implicit_field_list(self):
        """``FieldListImplicitExtraction`` for fields on different tensor B-spline bases over ONE node grid when the patch is
        spread over several ranks (no rank ever holds all rows) or TIGAR_IMPLICIT_M=1 asks for it; every field's operator
        must be exactly the Kronecker product of its 1-D factors (the filter of tIGAr/common.py:1569 dropped nothing but
        exact zeros) and the slab direction must carry open knot vectors.  None otherwise (stored blocks)."""
        from .BSplines import BSpline
        from .implicit import FieldListImplicitExtraction
        env = os.environ.get("TIGAR_IMPLICIT_M")
        if env == "0" or (env != "1" and self.comm.size == 1):
            return None
        kxs = []
        g0 = self.V.grids[0]
        for field in range(self.getNFields()):
            basis, grid = self.getScalarSpline(field), self.V.grids[field]
            if not (isinstance(basis, BSpline) and type(basis).getNodesAndEvals is BSpline.getNodesAndEvals) or \
                    not isinstance(grid, TensorNodeGrid) or grid.dg or grid.degree != g0.degree or \
                    any(not numpy.array_equal(a, b) for a, b in zip(grid.axes, g0.axes)):
                return None
            kx = self._kron_tables(basis, grid)
            if kx is None or not kx.products_stay_above(self.getIgnoreEps()):
                return None
            s_last = basis.splines[-1]
            kn, pl = numpy.asarray(s_last.knots, dtype=float), int(s_last.p)
            if not (numpy.all(kn[:pl + 1] == kn[0]) and numpy.all(kn[-(pl + 1):] == kn[-1])):
                return None
            kxs.append(kx)
        return FieldListImplicitExtraction(kxs, self.getIgnoreEps())

    def feRowOwners(self, nparts):
        """Rank of every FE row when the FE side is cut into ``nparts`` pieces the way this package cuts it: every
        field's nodes in ``nparts`` contiguous runs of (nearly) equal length -- whole node planes first for a
        tensor grid -- and piece r of every field on rank r.  (The reference takes the ownership from dolfin's mesh
        partition, tIGAr/common.py:1598-1600, 1612-1618.)"""
        owners = []
        for field in range(self.getNFields()):
            n = self.V.grids[field].num_nodes()
            owners.append((numpy.arange(n, dtype=numpy.int64) * int(nparts)) // max(n, 1))
        return numpy.concatenate(owners).astype(numpy.int32)

    def generatePermutation(self, nparts=None, fe_owner=None):
        """Order of the IGA dofs that follows the partition of the FE rows (tIGAr/common.py:1583-1665): every dof
        goes to the rank that owns most of the FE nodes of its support (``scipy.stats.mode`` there: the lowest
        rank on a tie; the support is everything ``getNodesAndEvals`` returns, zeros included), and the dofs are
        sorted by that rank.  Returns ``perm`` with new dof j = old dof perm[j] (the argsort the reference hands to
        MatPermute); the sort is stable, so within a rank the dofs keep their order.

        ``nparts``: number of ranks the extraction is prepared for (default: the size of the communicator);
        ``fe_owner``: owner of every FE row when it is not ``feRowOwners(nparts)``.  One part, or an operator that
        is never stored (tensor patch in z-slabs: the slabs of dofs already follow the slabs of FE rows): identity."""
        total = sum(self.getNcp(i) for i in range(self.getNFields()))
        nparts = int(self.comm.size if nparts is None else nparts)
        if fe_owner is not None:
            fe_owner = numpy.asarray(fe_owner, dtype=numpy.int32)
            nparts = max(nparts, int(fe_owner.max()) + 1 if fe_owner.size else 1)
        if nparts <= 1 or getattr(self.M, "is_implicit", False):
            return generateIdentityPermutation((0, total), self.comm)
        if fe_owner is None:
            fe_owner = self.feRowOwners(nparts)
        owner = self.generateM(support_only=True).transpose().majority_owner(fe_owner, nparts)
        return numpy.argsort(owner, kind="stable").astype(INDEX_TYPE)


class AbstractScalarBasis(object):
    """Scalar basis functions on a manifold with unique coordinates
    (tIGAr/common.py:1673-1759)."""

    __metaclass__ = abc.ABCMeta

    @abc.abstractmethod
    def getNodesAndEvals(self, xi):
        return

    @abc.abstractmethod
    def getNcp(self):
        return

    @abc.abstractmethod
    def generateMesh(self, comm=worldcomm):
        return

    @abc.abstractmethod
    def getDegree(self):
        return

    def needsDG(self):
        return True

    @abc.abstractmethod
    def useRectangularElements(self):
        return

    def getPrealloc(self):
        return DEFAULT_PREALLOC


class AbstractControlMesh(object):
    """Mapping from parametric to physical space (tIGAr/common.py:1762-1791)."""

    __metaclass__ = abc.ABCMeta

    @abc.abstractmethod
    def getHomogeneousCoordinate(self, node, direction):
        return

    @abc.abstractmethod
    def getScalarSpline(self):
        return

    @abc.abstractmethod
    def getNsd(self):
        return


class AbstractMultiFieldSpline(AbstractCoordinateChartSpline):
    """General multi-field spline built from AbstractScalarBasis members
    (tIGAr/common.py:1794-1885)."""

    __metaclass__ = abc.ABCMeta

    @abc.abstractmethod
    def getControlMesh(self):
        return

    @abc.abstractmethod
    def getFieldSpline(self, field):
        return

    def getPrealloc(self, control):
        if control:
            return self.getScalarSpline(-1).getPrealloc()
        return max(self.getScalarSpline(i).getPrealloc() for i in range(self.getNFields()))

    def getScalarSpline(self, field):
        if field == -1:
            return self.getControlMesh().getScalarSpline()
        return self.getFieldSpline(field)

    def getNsd(self):
        return self.getControlMesh().getNsd()

    def getHomogeneousCoordinate(self, node, direction):
        return self.getControlMesh().getHomogeneousCoordinate(node, direction)

    def getNodesAndEvals(self, x, field):
        return self.getScalarSpline(field).getNodesAndEvals(x)

    def generateMesh(self):
        return self.getScalarSpline(-1).generateMesh(comm=self.comm)

    def getDegree(self, field):
        return self.getScalarSpline(field).getDegree()

    def getNcp(self, field):
        return self.getScalarSpline(field).getNcp()

    def useDG(self):
        for i in range(-1, self.getNFields()):
            if self.getScalarSpline(i).needsDG():
                return True
        return False

    def _fieldGrid(self, field, dg):
        basis = self.getScalarSpline(field)
        deg = self.getDegree(field)
        try:
            return basis.generateMesh(comm=self.comm, degree=deg, dg=dg)
        except TypeError:
            grid = basis.generateMesh(comm=self.comm)
            if not isinstance(grid, TensorNodeGrid):
                raise TypeError("scalar bases used with tigar_amd must return a TensorNodeGrid "
                                "from generateMesh()")
            return grid


class EqualOrderSpline(AbstractMultiFieldSpline):
    """All unknown fields discretised with the control mesh's scalar basis
    (tIGAr/common.py:1891-1946).  ``EqualOrderSpline(numFields, controlMesh)``."""

    def customSetup(self, args):
        self.numFields = args[0]
        self.controlMesh = args[1]

    def getNFields(self):
        return self.numFields

    def getControlMesh(self):
        return self.controlMesh

    def getFieldSpline(self, field):
        return self.getScalarSpline(-1)

    def _single_shared_field(self):
        return self.numFields == 1

    def _fields_on_control_basis(self):
        return True

    def generateM(self, support_only=False):
        # one unknown field on the control mesh's basis: M is M_control (same rows, same
        # columns) -- share the device object instead of building it twice
        if self.numFields == 1 and getattr(self, "M_control", None) is not None and not support_only:
            return self.M_control
        return AbstractMultiFieldSpline.generateM(self, support_only)

    def addZeroDofsByLocation(self, subdomain, field):
        """Homogeneous Dirichlet BCs on the DoFs of ``field`` whose control points lie in
        ``subdomain`` (object with ``inside(x, on_boundary)``); tIGAr/common.py:1915-1946."""
        P = self._homogeneousCoordinateArray()
        nsd = self.getNsd()
        for I in range(P.shape[0]):
            p = P[I, 0:nsd] / P[I, nsd]
            if subdomain.inside(p, False) or subdomain.inside(p, True):
                self.zeroDofs += [self.globalDof(field, I)]


class FieldListSpline(AbstractMultiFieldSpline):
    """Multi-field spline from a list of scalar bases (tIGAr/common.py:1949-1970).
    ``FieldListSpline(controlMesh, fields)``."""

    def customSetup(self, args):
        self.controlMesh = args[0]
        self.fields = args[1]

    def getNFields(self):
        return len(self.fields)

    def getControlMesh(self):
        return self.controlMesh

    def getFieldSpline(self, field):
        return self.fields[field]


# ---- solver seam (b-4) ---------------------------------------------------------------------
class PETScKrylovSolver(object):
    """Look-alike of dolfin's ``PETScKrylovSolver(method, preconditioner)`` running on the
    GPU; plugs into ``ExtractedSpline.linearSolver`` (tIGAr/common.py:1255-1258), as in
    ``PETScKrylovSolver("gmres","jacobi")`` at demos/taylor-green/taylor-green-3d.py:89-90.
    Defaults are dolfin's [ext]: rtol 1e-6, atol 1e-15, maxit 10000, error on
    non-convergence."""

    # dolfin's names [ext: krylov_solver_methods() / krylov_solver_preconditioners()] -> what runs here.  Methods: cg,
    # gmres, bicgstab as named; the others that dolfin lists map onto the closest of the three.  Preconditioners: "none",
    # "jacobi" as named; "chebyshev" = a fixed Chebyshev polynomial in D^-1 K (csrc/tg_krylov.hip, tg_pcg_cheb), which also
    # stands in for the names whose PETSc implementation is a triangular sweep or a factorisation (sor, ilu, icc, bjacobi
    # = ILU(0) per process, amg ...): the request is honoured with the strongest preconditioner this library has for the
    # method, and ``preconditioner_requested`` / ``note`` say so -- dolfin users pass those names through the reference's
    # seam (tIGAr/common.py:1255-1258, 1292-1302) and should get a solve, not a ValueError.
    METHODS = {"cg": "cg", "gmres": "gmres", "bicgstab": "bicgstab", "default": "gmres", "minres": "gmres", "tfqmr": "bicgstab",
               "richardson": "gmres"}
    STRONG_PCS = ("sor", "ilu", "icc", "bjacobi", "amg", "hypre_amg", "petsc_amg", "hypre_euclid", "hypre_parasails", "ml_amg")

    def __init__(self, method="cg", preconditioner="jacobi", comm=None):
        self.method_requested, self.preconditioner_requested = method, preconditioner
        if method not in self.METHODS:
            raise ValueError("unknown Krylov method %r (%s)" % (method, ", ".join(sorted(self.METHODS))))
        method = self.METHODS[method]
        note = None
        if preconditioner == "default":
            preconditioner = "jacobi"
        if preconditioner in self.STRONG_PCS:
            note = " (preconditioner %r requested: " % (preconditioner,)
            if method == "cg":
                preconditioner = "chebyshev"
                note += "the Chebyshev polynomial preconditioner stands in for it)"
            else:
                preconditioner = "jacobi"
                note += "Jacobi stands in for it with %s)" % method
        if preconditioner not in ("none", "jacobi", "chebyshev", "fast_diagonalization"):
            raise ValueError("unknown preconditioner %r (none, jacobi, chebyshev, fast_diagonalization, or one of dolfin's: "
                             "%s)" % (preconditioner, ", ".join(self.STRONG_PCS)))
        if preconditioner == "chebyshev" and method != "cg":
            raise ValueError("the Chebyshev polynomial preconditioner serves cg (a fixed symmetric polynomial)")
        if preconditioner == "fast_diagonalization" and (method != "cg" or self.method_requested != "cg"):
            raise ValueError("the fast diagonalization preconditioner serves cg only (a symmetric positive definite P)")
        self.method, self.preconditioner = method, preconditioner
        if method != self.method_requested and self.method_requested != "default":
            note = (note or "") + " (method %r requested: %s runs in its place)" % (self.method_requested, method)
        if note:
            # the request is honoured with a stand-in, and says so where the user sees it, not only in the
            # message of a failed solve
            import warnings
            warnings.warn("PETScKrylovSolver(%r, %r): running (%r, %r)%s" % (self.method_requested, self.preconditioner_requested,
                                                                            method, preconditioner, note), stacklevel=2)
        self.parameters = {"relative_tolerance": 1e-6, "absolute_tolerance": 1e-15,
                           "maximum_iterations": 10000, "error_on_nonconvergence": True,
                           "nonzero_initial_guess": False, "gmres_restart": 30,
                           # (not a dolfin parameter) products per application of the Chebyshev preconditioner
                           "chebyshev_degree": 8,
                           "report": False, "monitor_convergence": False,
                           # (not a dolfin parameter) give up with status -3 after 25 GMRES restart cycles without
                           # progress instead of running to the iteration limit as PETSc does; set by the default
                           # solver that stands in for the reference's direct LU on large systems
                           "stagnation_guard": False,
                           # (not dolfin parameters) fast_diagonalization: None = coefficients fitted to diag K, or
                           # (c_0, .., c_{d-1}, c_mass); "diagonal" = D^-1/2 P^-1 D^-1/2 with D = diag K / diag P, or "none"
                           "fd_coefficients": None, "fd_scaling": "diagonal"}
        self.comm = comm
        self.last = None
        self.note = note       # appended to the non-convergence message (who chose this solver / what stands in)

    REASONS = {-1: "iteration limit reached", -2: "breakdown (NaN / zero pivot in the recurrence)",
               -3: "stagnation (25 GMRES restart cycles without progress)"}

    def solve(self, A, x, b):
        """``x`` is the output; with ``parameters["nonzero_initial_guess"]`` it also holds the start vector
        (the convergence test stays relative to ||B b||, PETSc's default [ext])."""
        A, x, b = _as_device_csr(A), _as_device_vector(x), _as_device_vector(b)
        guess = bool(self.parameters["nonzero_initial_guess"])
        if self.preconditioner == "fast_diagonalization":
            return self._solve_fd(A, x, b, guess)

        def run(pc):
            return _dev.krylov_solve(
                A, b, x, self.method, pc, self.parameters["relative_tolerance"],
                self.parameters["absolute_tolerance"], self.parameters["maximum_iterations"],
                self.parameters["chebyshev_degree"] if pc == "chebyshev" else self.parameters["gmres_restart"],
                self.comm, nonzero_initial_guess=guess,
                stagnation_guard=bool(self.parameters.get("stagnation_guard", False)),
                # (a matrix this package assembled from a form that is symmetric by construction: the half-storage copy
                #  of a CG solve is not compared with the CSR product again, csrc/tg_symgrid.hip)
                symmetric=bool(getattr(A, "symmetric_by_construction", False)))

        x0 = None
        if self.preconditioner == "chebyshev" and guess:
            x0 = DeviceVector(x.size())
            _dev.vec_copy_range(x0, 0, x, 0, x.size())
        its, res, status = run(self.preconditioner)
        if status == -2 and self.preconditioner == "chebyshev":
            # the polynomial is built on an ESTIMATE of the largest eigenvalue of D^-1 K (a few power iterations); an estimate
            # that is too small makes the polynomial indefinite and the recurrence breaks down although K is fine.
            # Jacobi-CG needs no estimate: run it instead of reporting a breakdown.  A K or b that holds NaN breaks
            # it down as well and the status stays -2.
            import warnings
            warnings.warn("PETScKrylovSolver: Chebyshev-preconditioned CG broke down (eigenvalue estimate); "
                          "solving with Jacobi-CG instead", stacklevel=2)
            if x0 is not None:
                _dev.vec_copy_range(x, 0, x0, 0, x.size())
            its_c = its
            its, res, status = run("jacobi")
            return self._finish(its, res, status, "jacobi", fallback={"preconditioner": "jacobi", "after_iterations": its_c})
        return self._finish(its, res, status, self.preconditioner)


    def _solve_fd(self, A, x, b, guess):
        from .fastdiag import FastDiagonalization
        if self.comm is not None:
            raise ValueError("fast_diagonalization: several ranks are not supported (the transform of the slab direction "
                             "would need an all-to-all)")
        fd = FastDiagonalization(A, coefficients=self.parameters["fd_coefficients"], scaling=self.parameters["fd_scaling"])
        t0 = time.perf_counter()
        its, res, status = _dev.krylov_solve_fd(A, fd.device, b, x, self.parameters["relative_tolerance"],
                                                self.parameters["absolute_tolerance"],
                                                self.parameters["maximum_iterations"], nonzero_initial_guess=guess,
                                                symmetric=bool(getattr(A, "symmetric_by_construction", False)))
        return self._finish(its, res, status, "fast_diagonalization",
                            fd={"coefficients": fd.coefficients, "setup_seconds": fd.setup_seconds,
                                "setup_reused": fd.setup_reused, "fit_seconds": fd.fit_seconds, "scaling": fd.scaling,
                                "solve_seconds": time.perf_counter() - t0})

    def _finish(self, its, res, status, preconditioner, **extra):
        """records ``self.last`` (``preconditioner``: the one that ran; ``extra``: entries of that path) and raises on
        non-convergence"""
        self.last = {"iterations": its, "residual_norm": res, "status": status, "method": self.method,
                     "preconditioner": preconditioner, "method_requested": self.method_requested,
                     "preconditioner_requested": self.preconditioner_requested}
        self.last.update(extra)
        if status < 0 and self.parameters["error_on_nonconvergence"]:
            raise RuntimeError("Krylov solver (%s, %s) did not converge: %s after %d iterations, preconditioned "
                               "residual %.3e.%s" % (self.method, self.preconditioner,
                                                     self.REASONS.get(status, "status %d" % status), its, res,
                                                     self.note or ""))
        return its


KrylovSolver = PETScKrylovSolver


def _rcm_ordering(A):
    """(host matrix, reverse Cuthill-McKee permutation of its stored pattern, (kl, ku) of the reordered matrix) of a
    ``DeviceCSR``: the bandwidth-reducing ordering of the PATTERN on the host (symbolic step; the values stay on the device
    except for this download)"""
    import scipy.sparse as _sp
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    S = A.to_scipy()
    # (the STORED pattern: entries zeroed by MatZeroRowsColumns stay in the band storage, so they must stay in
    #  the graph -- scipy's sum of abs(S) would drop them and leave the boundary dofs isolated)
    ones = _sp.csr_matrix((numpy.ones(S.nnz, dtype=numpy.int8), S.indices, S.indptr), shape=S.shape)
    prm = numpy.asarray(reverse_cuthill_mckee((ones + ones.T).tocsr(), symmetric_mode=True), dtype=numpy.int64)
    inv = numpy.empty_like(prm)
    inv[prm] = numpy.arange(prm.size)
    coo = S.tocoo()
    dist = inv[coo.row] - inv[coo.col]
    return S, prm, (int(max(0, dist.max())), int(max(0, -dist.min())))


class PETScLUSolver(object):
    """Look-alike of dolfin's ``PETScLUSolver`` / ``LUSolver``: direct solve on the GPU by banded LU with partial
    pivoting (``tg_lu_solve``, LAPACK dgbtrf's storage and pivoting).  Plugs into ``ExtractedSpline.linearSolver``.
    IGA matrices of tensor-product patches are banded in the patch numbering; for other orderings (several fields
    numbered field after field) ``parameters["reorder"]`` (default "auto") applies a reverse Cuthill-McKee
    permutation of the pattern first.  Refuses systems whose band storage exceeds ``max_band_bytes``."""

    def __init__(self, method="default", comm=None):
        # ("symmetric", "reuse_factorization": dolfin users set them; accepted and ignored)
        self.parameters = {"reorder": "auto", "max_band_bytes": _plan.LU_SOLVER_MAX_BAND_BYTES, "report": False,
                           "symmetric": False, "reuse_factorization": False}
        self.last = None

    def band_cost(self, A):
        """(bytes of band storage, multiply-adds) of factorising ``A`` as it is numbered"""
        kl, ku, _ = _dev.lu_band_info(A)
        return _plan.lu_band_bytes(A.shape[0], kl, ku), _plan.lu_madds(A.shape[0], kl, ku)

    def solve(self, A, x, b, _ordering=None):
        """``_ordering``: ``_rcm_ordering(A)`` where the caller has it already"""
        A, x, b = _as_device_csr(A), _as_device_vector(x), _as_device_vector(b)
        n = A.shape[0]
        kl, ku, nb = _dev.lu_band_info(A)
        perm = None
        mode = self.parameters["reorder"]
        if mode is True or (mode == "auto" and _plan.auto_reorders(n, kl, ku)):
            S, prm, (kl2, ku2) = _ordering or _rcm_ordering(A)
            nb2 = _plan.lu_band_bytes(n, kl2, ku2)
            if nb2 < nb:       # (one re-upload, of the permuted matrix)
                A, perm, kl, ku, nb = DeviceCSR.from_scipy(S[prm][:, prm].tocsr()), prm, kl2, ku2, nb2
        if nb > self.parameters["max_band_bytes"]:
            raise MemoryError("direct solve: the band storage of this %d x %d system (half-bandwidths %d / %d) needs %.1f GB; "
                              "use a Krylov solver (PETScKrylovSolver) for systems of this size" % (n, n, kl, ku, nb / 2 ** 30))
        chol0 = _dev.prof_get(8)[1]
        if perm is not None:
            bp = DeviceVector(data=b.get_local()[perm])
            xp = DeviceVector(n)
            info = _dev.lu_solve(A, bp, xp)
            if info == 0:
                out = numpy.empty(n)
                out[perm] = xp.get_local()
                x.set_local(out)
        else:
            info = _dev.lu_solve(A, b, x)
        # (a symmetric positive definite system is factorised as L L^T -- blocked banded Cholesky on the matrix cores,
        #  csrc/tg_chol.hip -- instead of P A = L U; TIGAR_LU_CHOLESKY=0: always the LU)
        self.last = {"info": info, "kl": kl, "ku": ku, "band_bytes": nb, "reordered": perm is not None,
                     "factorisation": "cholesky" if _dev.prof_get(8)[1] > chol0 else "lu"}
        if info != 0:
            raise RuntimeError("direct solve: the matrix is singular (exact zero pivot in column %d)" % (info - 1))
        return 1


LUSolver = PETScLUSolver


class _DefaultSolver(object):
    """What runs when ``linearSolver`` is None.  The reference calls dolfin's ``solve`` there, i.e. a sparse direct LU
    (tIGAr/common.py:1255-1256 [ext]) -- every demo relies on it.  Here: the attempts of ``direct_plan.default_plan``
    in order.  The banded direct solver above whenever its cost is moderate (band storage <= 8 GiB and <= 4e12
    multiply-adds: all 2-D patches of the demos, small 3-D ones), as numbered or in the reverse Cuthill-McKee ordering
    (field-major systems of several fields, kl ~ n (nF-1)/nF: the saddle point and elasticity cases where the reference's
    direct solver matters); beyond that a symmetric positive definite system -- the common case -- still gets a direct
    solve, by the banded Cholesky factorisation (a quarter of the LU's multiply-adds, on the matrix cores, a third of its
    band; it declines what is not SPD and the next choice runs); otherwise Jacobi-preconditioned GMRES(30) (CG for the
    normal equations of ``FEtoIGA``) to a relative residual of 1e-12, bounded by PETSc's default 10 000 iterations and by
    the solver's stagnation guard, with an error message that names the deviation when it gives up."""

    def __init__(self, method="gmres"):
        self.method = method
        self.comm = None
        self.last = None

    def solve(self, A, x, b):
        A = _as_device_csr(A)
        n = A.shape[0]
        kl = ku = 0
        if self.comm is None:
            kl, ku, _ = _dev.lu_band_info(A)
        ordering = None
        for attempt in _plan.default_plan(n, A.nnz, kl, ku, self.comm is not None, os.environ.get("TIGAR_DEFAULT_SOLVER"),
                                          os.environ.get("TIGAR_LU_CHOLESKY")):
            if attempt == "cholesky":
                if _dev.chol_solve(A, _as_device_vector(b), _as_device_vector(x)):
                    self.last = {"solver": "lu", "factorisation": "cholesky", "info": 0, "kl": kl, "ku": ku,
                                 "band_bytes": _plan.chol_band_bytes(n, kl), "reordered": False}
                    return 1
            elif attempt == "krylov":
                return self._krylov(A, x, b)
            else:
                lu = PETScLUSolver()
                if attempt == "rcm":
                    ordering = _rcm_ordering(A)
                    if not _plan.lu_fits(n, *ordering[2]):
                        continue
                    lu.parameters["reorder"] = True
                lu.solve(A, x, b, _ordering=ordering)
                self.last = dict(lu.last, solver="lu")
                return 1

    def _krylov(self, A, x, b):
        ks = PETScKrylovSolver(self.method, "jacobi", comm=self.comm)
        ks.parameters["relative_tolerance"] = 1e-12
        ks.parameters["maximum_iterations"] = 10000
        ks.parameters["stagnation_guard"] = True
        ks.note = ("  (linearSolver=None: the reference would have run dolfin's direct LU here; this system is too large for "
                   "tigar_amd's banded direct solver, so Jacobi-%s was used -- set ExtractedSpline.linearSolver for "
                   "ill-conditioned systems)" % self.method.upper())
        ks.solve(A, x, b)
        self.last = dict(ks.last, solver=self.method)
        return ks.last["iterations"]


def _default_linear_solver(method="gmres"):
    return _DefaultSolver(method)


# ---- analysis side ---------------------------------------------------------------------------
class ExtractedSpline(object):
    """
    An extracted spline (tIGAr/common.py:667-1433), restricted to the hot path: the
    extraction operators, their application to FE matrices/vectors, and the linear solve.
    UFL form construction (``grad``, ``dx`` ...) needs FEniCS and is not provided here; the package's own forms
    (tigar_amd/forms.py) stand in for it, with ``rational=True`` for the reference's ``spline.rationalize`` of trial and
    test functions.

    With a generator that was given the caller's FE dof order (``fe_nodes=`` / ``setFENodes``) the spline carries
    ``feOrder``: assembled matrices / vectors handed in are taken in the caller's order and FE functions are returned in
    it.  ``M``, ``MT``, ``cpFuncs`` and everything the package's own forms assemble stay in the order of the node grid;
    K, M^T b and U are IGA objects and do not depend on the order.
    """

    def __init__(self, sourceArg, quadDeg=None, mesh=None, doPermutation=DEFAULT_DO_PERMUTATION,
                 comm=worldcomm):
        if isinstance(sourceArg, AbstractExtractionGenerator):
            self.initFromGenerator(sourceArg, quadDeg, doPermutation)
        else:
            self.initFromFilesystem(sourceArg, quadDeg, comm, mesh)
        self.genericSetup()

    def initFromFilesystem(self, dirname, quadDeg, comm, mesh=None):
        """Instance from the extraction data in directory ``dirname`` (tIGAr/common.py:748-894):
        ``extraction-info.txt``, the PETSc binary matrices and index set, and ``extraction-data.h5`` (control functions
        from ``/control<i>/vector_0``, node sets from the group ``/tigar_amd``; see ``writeExtraction``).  M is then an
        arbitrary sparse matrix: extractMatrix uses the general PtAP kernel."""
        from . import petscio
        self.quadDeg = quadDeg
        self.comm = comm
        with open(os.path.join(dirname, EXTRACTION_INFO_FILE), "r") as f:
            lines = f.read().split("\n")
        self.nsd = int(lines[0])
        self.elementType = lines[1]
        self.nFields = int(lines[2])
        self.p_control = int(lines[3])
        ncp_control = int(lines[4])
        self.p, ncp = [], []
        for i in range(self.nFields):
            self.p.append(int(lines[5 + 2 * i]))
            ncp.append(int(lines[6 + 2 * i]))
        h5_path, npz_path = os.path.join(dirname, EXTRACTION_DATA_FILE), os.path.join(dirname, EXTRACTION_DATA_NPZ)
        h5 = None
        if os.path.exists(h5_path):
            from . import h5io
            h5 = h5io.H5File(h5_path, "r")
            if not h5.exists(EXTRACTION_H5_PRIVATE):
                h5.close()
                raise IOError("%s carries no group %s: it was not written by this package.  Directories written by the "
                              "reference hold M in dolfin's own dof numbering, which cannot be matched to node positions "
                              "without dolfin" % (h5_path, EXTRACTION_H5_PRIVATE))
            data = _H5Archive(h5)
            control = [h5.read_dataset(EXTRACTION_H5_CONTROL_FUNC_NAME(i) + "/vector_0") for i in range(self.nsd + 1)]
        elif os.path.exists(npz_path):                     # directories written by rounds 1-2 of this package
            data = numpy.load(npz_path)
            control = [data["control%d" % i] for i in range(self.nsd + 1)]
        else:
            raise IOError("neither %s nor %s found" % (h5_path, npz_path))

        def space(name):
            grids = []
            for gi in range(int(data[name + "_ngrids"])):
                grids.append(_grid_from_arrays(data, "%s_%d" % (name, gi)))
            return TensorFunctionSpace(grids, str(data[name + "_element"]))
        self.mesh = mesh
        self.V_control = space("control")
        self.V = space("fields")
        self.cpFuncs = []
        for i in range(self.nsd + 1):
            f = Function(self.V_control)
            f.vector().set_local(control[i])
            self.cpFuncs.append(f)
        if h5 is not None:
            h5.close()
        self.M_control = DeviceCSR.from_scipy(petscio.read_mat(os.path.join(dirname, EXTRACTION_MAT_FILE_CTRL)))
        self.M = DeviceCSR.from_scipy(petscio.read_mat(os.path.join(dirname, EXTRACTION_MAT_FILE)))
        if self.M_control.shape != (self.V_control.dim(), ncp_control) or self.M.shape != (self.V.dim(), sum(ncp)):
            raise ValueError("extraction matrices in %s do not match extraction-info.txt" % dirname)
        self.zeroDofs = numpy.asarray(petscio.read_is(os.path.join(dirname, EXTRACTION_ZERO_DOFS_FILE)), dtype=INDEX_TYPE)
        self._kron = self._kron_scalar = self._kron_fields = None       # (M read from files: an arbitrary sparse matrix)
        self.feOrder = None

    def initFromGenerator(self, generator, quadDeg, doPermutation=DEFAULT_DO_PERMUTATION):
        """tIGAr/common.py:708-746 -- shares M, M_control, V, cpFuncs with the generator."""
        if doPermutation:
            generator.applyPermutation()
        self.quadDeg = quadDeg
        self.nsd = generator.getNsd()
        self.elementType = generator.extractionElement()
        self.nFields = generator.getNFields()
        self.p_control = generator.getDegree(-1)
        self.p = [generator.getDegree(i) for i in range(self.nFields)]
        self.mesh = generator.mesh
        self.cpFuncs = generator.cpFuncs
        self.V = generator.V
        self.V_control = generator.V_control
        self.M = generator.M
        self.M_control = generator.M_control
        self.comm = generator.getComm()
        self._generator_engine = getattr(generator, "_slab_engine", None)
        self._generator = generator
        self._kron = getattr(generator, "_kron", None)
        self._kron_scalar = getattr(generator, "_kron_scalar", None)
        self._kron_fields = getattr(generator, "_kron_fields", None)
        self.zeroDofs = generator.zeroDofsArray().astype(INDEX_TYPE)
        self.feOrder = getattr(generator, "feOrder", None)

    def genericSetup(self):
        self.setSolverOptions()
        self.MT = self.M.transpose()          # explicit M^T (cached on M by the generator)
        self._slab = None
        import weakref
        from .ptaproutes import ResidentPtAP
        me = weakref.proxy(self)              # (no reference cycle: what the spline holds on the device goes with its last user)
        self._ptap = ResidentPtAP(self.M, self.MT, self.nFields, self._kron, self._kron_scalar, self._kron_fields,
                                  grids=getattr(self.V, "grids", None), distributed=self._distributed(),
                                  slab=lambda: me._slab_path(), row_blocks=self._row_blocks_of,
                                  field_blocks=lambda A: me._block_producer(A), timers=lambda: getattr(me, "stage_timers", None))

    # -- streamed / distributed engine -------------------------------------------------------------
    def _implicit(self):
        return bool(getattr(self.M, "is_implicit", False))

    def _distributed(self):
        return self.comm is not None and getattr(self.comm, "size", 1) > 1

    def _slab_path(self):
        """The z-slab engine (``tigar_amd.dist.SlabHotPath``) behind extractMatrix / extractVector /
        solveLinearSystem when M is implicit or the patch is spread over several ranks: rows of K in
        sub-slabs of dof planes, only K resident (PETSc's row-block MatPtAP, tIGAr/common.py:1194-1195)."""
        if self._slab is None and getattr(self, "_generator_engine", None) is not None and self.nFields == 1:
            self._slab = self._generator_engine
        if self._slab is None:
            from .dist import FieldListSlabPath, FieldSlabPath, SlabHotPath
            dc = self.comm.device() if self._distributed() else None
            rank, world = (self.comm.rank, self.comm.size) if dc is not None else (0, 1)
            eps = getattr(self.M, "eps", DEFAULT_BASIS_FUNC_IGNORE_EPS)
            kx = self._kron if self._kron is not None else self._kron_scalar
            if kx is not None:
                # one field: the scalar engine; several fields on one tensor basis: the scalar engine per block, fields
                # interleaved plane by plane
                self._slab = SlabHotPath(kx.basis, kx.grid, rank, world, dc, sub_planes="auto", eps=eps, kx=kx) \
                    if self._kron is not None else \
                    FieldSlabPath(kx.basis, kx.grid, self.nFields, rank, world, dc, sub_planes="auto", eps=eps, kx=kx)
            elif self._kron_fields is not None:
                # fields on different tensor bases over one node grid: one split of the plane index, pair walks per block
                self._slab = FieldListSlabPath(self._kron_fields, rank, world, dc, sub_planes="auto", eps=eps)
            else:
                raise NotImplementedError("the streamed / multi-GPU path needs tensor-product B-spline fields (one basis, or "
                                          "several bases over one node grid)")
        return self._slab

    def localDofRange(self):
        """IGA dofs [g0, g1) owned by this rank (PETSc getOwnershipRange of MTAM's rows)."""
        if self._distributed() or (self._implicit() and self.nFields > 1):
            return self._slab_path().mine["dofs"]
        return (0, self.M.shape[1])

    def localDofIndices(self):
        """Reference (field-after-field) index of every entry of this rank's IGA vectors and rows of MTAM, in local order.
        One field: the contiguous range ``localDofRange()``.  Several fields on several ranks: the dofs are renumbered
        plane by plane across the fields so that a rank's block stays contiguous (``tigar_amd.dist.FieldSlabPath``) -- as
        the reference renumbers the IGA dofs for parallel runs (generatePermutation, tIGAr/common.py:1583-1665)."""
        sp_ = self._slab_path() if (self._distributed() or self._implicit()) else None
        if sp_ is not None and hasattr(sp_, "local_dof_indices"):
            return sp_.local_dof_indices()
        g0, g1 = self.localDofRange()
        return numpy.arange(g0, g1, dtype=numpy.int64)

    def localFERange(self):
        """FE rows whose prolongation u = M U this rank computes (several fields: one range per field)."""
        if self._distributed() or (self._implicit() and self.nFields > 1):
            return self._slab_path().mine["u_rows"]
        return (0, self.M.shape[0])

    # -- a-10
    def _caller_ordered(self):
        return self.feOrder is not None and not self.feOrder.is_identity

    def extractionMatrixFE(self):
        """M as a stored CSR matrix whose rows are in the caller's FE order (``self.M`` itself stays in grid order; it is
        returned as it is when the caller numbers like the grid)"""
        if not self._caller_ordered():
            return self.M
        if self._implicit():
            raise NotImplementedError("extractionMatrixFE: the extraction operator of this spline is never stored")
        return self.M.gather_rows(self.feOrder.grid_of_fe)

    def extractVector(self, b, applyBCs=True):
        """Apply extraction to an FE vector ``b``: ``M^T b``, zeroed at ``zeroDofs`` if
        ``applyBCs`` (tIGAr/common.py:1142-1160).  ``b`` is in the caller's FE order when the spline has an ``feOrder``."""
        if self._caller_ordered():
            from .implicit import LazyFEVector
            if isinstance(b, LazyFEVector):
                raise NotImplementedError("extractVector: a LazyFEVector produces rows of the node grid; a caller-ordered "
                                          "spline takes assembled vectors")
            b = self.feOrder.to_grid(b)
        return self._extract_vector_grid(b, applyBCs)

    def _extract_vector_grid(self, b, applyBCs=True):
        """``extractVector`` of a vector in grid order"""
        from .implicit import LazyFEVector
        if isinstance(b, LazyFEVector) or self._distributed() or (self._implicit() and self.nFields > 1):
            # (several fields with an implicit operator: the field-block engine and its plane-wise numbering, also on
            #  one rank -- K, M^T b and U must share it)
            if isinstance(b, LazyFEVector):
                rows = b.rows
            else:
                full = _as_device_vector(b)       # replicated FE vector: every rank takes its rows

                def rows(r0, r1):
                    piece = DeviceVector(r1 - r0)
                    _dev.vec_copy_range(piece, 0, full, r0, r1 - r0)
                    return piece
            return self._slab_path().assemble_vector(rows, self.zeroDofs if applyBCs else None,
                                                     getattr(self, "stage_timers", None))
        MTb = self.M.mult_transpose(_as_device_vector(b))
        if applyBCs:
            MTb.zero_entries(self.zeroDofs)
        return MTb

    def assembleVector(self, form, applyBCs=True):
        """``form``: anything with ``.assemble_vector(V)`` (see ``tigar_amd.forms``) or an
        already assembled FE vector (tIGAr/common.py:1162-1173).  With several ranks the form is
        asked for the FE rows each rank needs (``assemble_vector(V, row0, row1)``)."""
        if not self.__dict__.get("_in_system"):
            self._new_ghost_epoch()
        if hasattr(form, "assemble_vector"):
            if self._distributed():
                from .implicit import LazyFEVector
                b = LazyFEVector(lambda r0, r1: form.assemble_vector(self.V, r0, r1), self.V.dim())
            else:
                b = form.assemble_vector(self.V)
        else:
            return self.extractVector(form, applyBCs=applyBCs)       # (assembled by the caller: in the caller's order)
        return self._extract_vector_grid(b, applyBCs)                 # (the package's forms number the node grid)

    # -- a-11
    def extractMatrix(self, A, applyBCs=True, diag=1):
        """Apply extraction to an FE matrix ``A``: ``M^T A M`` (PtAP), then rows and columns
        of ``zeroDofs`` zeroed with ``diag`` on the diagonal (tIGAr/common.py:1176-1204).
        The symbolic plan is cached and reused while A's pattern is unchanged.  A K of a single tensor-product patch on
        one rank carries ``K.tensor_structure`` (what the fast diagonalization preconditioner needs, tigar_amd/fastdiag.py);
        otherwise ``K.tensor_structure_refusal`` says why not.  ``A`` is in the caller's FE order when the spline has an
        ``feOrder``; it is brought to grid order on the device first and reaches the same route as a grid-ordered A."""
        if self._caller_ordered():
            from .implicit import LazyFEMatrix
            if isinstance(A, LazyFEMatrix):
                raise NotImplementedError("extractMatrix: a LazyFEMatrix produces rows of the node grid; a caller-ordered "
                                          "spline takes assembled matrices")
            A = self.feOrder.permute_matrix(A)
        return self._extract_matrix_grid(A, applyBCs, diag)

    def _extract_matrix_grid(self, A, applyBCs=True, diag=1):
        """``extractMatrix`` of a matrix in grid order"""
        K = self._extract_matrix(_fe_matrix(A), applyBCs, diag)
        if isinstance(K, DeviceCSR):
            ts, why = self._tensor_structure(applyBCs)
            if ts is not None:
                K.tensor_structure = ts
            else:
                K.tensor_structure_refusal = why
        return K

    def tensor_structure(self):
        """the ``fastdiag.TensorStructure`` of this spline's K (zero dofs applied), or None"""
        return self._tensor_structure(True)[0]

    def _tensor_structure(self, applyBCs):
        """(descriptor, None) when the space qualifies for the fast diagonalization preconditioner, else (None, reason)"""
        if self._distributed():
            return None, "several ranks (the transform of the slab direction would need an all-to-all)"
        gen = getattr(self, "_generator", None)
        perm = getattr(gen, "permutation", None)
        if perm is not None and numpy.asarray(perm).size and \
                not numpy.array_equal(numpy.asarray(perm), numpy.arange(numpy.asarray(perm).size)):
            return None, "a dof permutation was applied to the generator (the dofs are no longer numbered as a tensor grid)"
        if self._kron_fields is not None and self._kron is None:
            return None, "fields on different bases (FieldListSpline / compatible spaces) are not supported"
        kx = self._kron if self._kron is not None else self._kron_scalar
        if kx is None:
            return None, ("the extraction operator is not the Kronecker product of 1-D B-spline factors (not a single "
                          "tensor-product patch)")
        if kx.d not in (2, 3):
            return None, "only 2-D and 3-D patches are supported"
        nf = self.nFields if self._kron is None else 1
        if self._kron is not None and self.nFields != 1:
            return None, "the extraction operator is not the Kronecker product of 1-D B-spline factors"
        cache = self.__dict__.setdefault("_fd_cache", {})
        from .fastdiag import TensorStructure
        return TensorStructure(kx, nf, self.zeroDofs if applyBCs else None, cache), None

    def _extract_matrix(self, A, applyBCs=True, diag=1):
        """which product forms M^T A M: ``tigar_amd.ptaproutes.ResidentPtAP`` (one ordered table of routes)"""
        return self._ptap.product(A, self.zeroDofs if applyBCs else None, diag)

    def _block_producer(self, A):
        """``a_block(f, g, r0, r1)`` for the field-block engine: rows [r0, r1) of block (f, g) of an FE matrix on the mixed
        space, columns of one field; None where the producer says the fields are not coupled.  Which fields an EXPLICIT matrix
        couples is counted (``a_block.is_empty``, read by ``dist._block_is_empty``): a coupling added by hand may sit on a few
        nodes.  ``block_rows`` of a LazyFEMatrix carry their maker's declaration (``dist.populates_every_plane``) or none; a
        LazyFEMatrix with ``rows`` only declares nothing and is asked for all its rows."""
        from .implicit import LazyFEMatrix
        nfe = self.V.dim() // self.nFields
        lazy = isinstance(A, LazyFEMatrix)
        if lazy and getattr(A, "block_rows", None) is not None:
            return A.block_rows
        rows = A.rows if lazy else self._row_blocks_of(A)

        def a_block(f, g, r0, r1):
            blk = rows(f * nfe + int(r0), f * nfe + int(r1))
            return blk.block(0, int(r1) - int(r0), g * nfe, (g + 1) * nfe)
        if not lazy:
            a_block.is_empty = self._explicit_block_is_empty(A, nfe)
        return a_block

    @staticmethod
    def _explicit_block_is_empty(A, nfe):
        """``is_empty(f, g, r0, r1)`` of an explicit FE matrix: no stored entry in rows [r0, r1) of block (f, g) -- the question
        ``ptaproutes.product_by_field_blocks`` asks of the whole block (``Afg.nnz == 0``), on the host for a scipy matrix,
        on the device for a DeviceCSR"""
        nfe = int(nfe)
        Ah = A if isinstance(A, DeviceCSR) else _fe_matrix(A).tocsr()

        def is_empty(f, g, r0, r1):
            a, b, c = f * nfe + int(r0), f * nfe + int(r1), g * nfe
            if isinstance(Ah, DeviceCSR):
                return Ah.block(a, b, c, c + nfe).nnz == 0
            return Ah[a:b, c:c + nfe].nnz == 0
        return is_empty

    @staticmethod
    def _row_blocks_of(A):
        """``rows(r0, r1)`` of an explicit FE matrix: DeviceCSR row blocks with global columns"""
        if isinstance(A, DeviceCSR):
            ncols = A.shape[1]
            return lambda r0, r1: A.block(int(r0), int(r1), 0, ncols)
        Ah = _fe_matrix(A)
        if not hasattr(Ah, "tocsr"):
            raise TypeError("extractMatrix: an assembled FE matrix is expected here, not %s" % type(A).__name__)
        Ah = Ah.tocsr()
        return lambda r0, r1: DeviceCSR.from_scipy(Ah[int(r0):int(r1)])

    def assembleMatrix(self, form, applyBCs=True, diag=1):
        """tIGAr/common.py:1206-1220.  When the assembled FE matrix cannot be resident next to K (implicit
        M: cfg3's A is 684 GB) or the patch is spread over several ranks, the form is asked for row blocks
        (``assemble_matrix(V, row0, row1)``) as the z-slab pipeline consumes them."""
        if not self.__dict__.get("_in_system"):
            self._new_ghost_epoch()
        if hasattr(form, "assemble_matrix"):
            if self._implicit() or self._distributed():
                from .implicit import LazyFEMatrix
                n = self.V.dim()
                fac = None
                if hasattr(form, "factors") and getattr(form, "geometry", None) is None and self.nFields == 1:
                    fac = form.factors(self.V)          # Kronecker sum of 1-D matrices: may be fused into the PtAP
                A = LazyFEMatrix(lambda r0, r1: form.assemble_matrix(self.V, r0, r1), (n, n), kron_factors=fac)
                if self.nFields > 1 and hasattr(form, "assemble_block"):
                    # forms on a mixed space hand out their field blocks (rows of one block, columns of one field); a block of
                    # an integral over the patch is structurally empty or has entries on every node plane
                    from .dist import populates_every_plane
                    A.block_rows = populates_every_plane(lambda f, g, r0, r1: form.assemble_block(self.V, f, g, r0, r1))
                    A.block_factors = form.block_factors(self.V) if hasattr(form, "block_factors") else None
            else:
                A = form.assemble_matrix(self.V)
            K = self._extract_matrix_grid(A, applyBCs=applyBCs, diag=diag)     # (the package's forms number the node grid)
        else:
            A = form
            K = self.extractMatrix(A, applyBCs=applyBCs, diag=diag)            # (assembled by the caller: in its order)
        proof = None
        if getattr(form, "symmetric", False) is True and isinstance(K, DeviceCSR) and self.nFields == 1 and \
                hasattr(form, "factors") and getattr(form, "geometry", None) is None:
            proof = getattr(A, "kron_factors", None) or form.factors(self.V)      # (what A was formed from, either way)
        if proof is not None and _kron_sum_is_symmetric(proof):
            # PROVED symmetric: A is a Kronecker sum whose terms are (checked here, on the 1-D matrices) symmetric or come with
            # their transposes, so M^T A M with MatZeroRowsColumns is symmetric to rounding.  Then the solver builds its
            # half-storage copy without comparing it with the CSR product (TG_KSP_SYMMETRIC).  Every other K -- mapped forms,
            # matrices handed in, subclasses of the forms -- is compared once (the result is kept on the matrix).
            K.symmetric_by_construction = True
        return K

    def assembleLinearSystem(self, lhsForm, rhsForm, applyBCs=True):
        # one ghost update of the rank-local functions the forms read serves both assemblies (Function.ghosted)
        self._new_ghost_epoch()
        self._in_system = True
        try:
            return (self.assembleMatrix(lhsForm, applyBCs), self.assembleVector(rhsForm, applyBCs))
        finally:
            self._in_system = False

    # -- a-12
    def solveLinearSystem(self, MTAM, MTb, u):
        """Solve ``MTAM*U = MTb`` and store ``M*U`` in the FE function ``u``; returns ``U``
        (tIGAr/common.py:1236-1263).  With ``linearSolver == None`` the reference calls dolfin's direct LU;
        here: the banded LU of csrc/tg_lu.hip while its band storage fits (``_DefaultSolver``), Jacobi-GMRES at
        tight tolerance beyond, with a message that says so.  On a spline with an ``feOrder`` ``u`` is written -- and a
        non-zero initial guess in it read -- in the caller's FE order."""
        reorder = self._caller_ordered()
        if reorder and (self._distributed() or (self._implicit() and self.nFields > 1)):
            raise NotImplementedError("solveLinearSystem: caller-ordered FE functions with the streamed field engine")
        MTU = DeviceVector(MTAM.shape[0])          # (local rows of MTAM: all of them on one rank)
        if self._distributed():
            self._require_columns_within_halo(MTAM)
        solver =self.linearSolver if self.linearSolver is not None else _default_linear_solver()
        if getattr(solver, "parameters", {}).get("nonzero_initial_guess", False):
            # the reference sizes AND seeds MTU = M^T u.vector() (tIGAr/common.py:1250-1254): a guess set in u is used.
            # Distributed or several implicit fields: through the slab engine, which gives the rank's rows of M^T u in
            # the numbering K and M^T b carry
            if self._distributed() or (self._implicit() and self.nFields > 1):
                MTU = self._initial_guess_through_slabs(u)
            else:
                self.M.mult_transpose(self.feOrder.to_grid(u) if reorder else _as_device_vector(u), MTU)
        if self._distributed() and getattr(solver, "comm", False) is None:
            solver.comm = self.comm.device()
        solver.solve(MTAM, MTU, MTb)
        if self._distributed() or (self._implicit() and self.nFields > 1):
            # u = M U on the FE rows this rank owns, U with its halo (tIGAr/common.py:1259-1261:
            # M*MTU followed by the ghost update)
            u_loc = self._slab_path().prolong(MTU)
            u._vec, u.local_range = u_loc, self._slab_path().mine["u_rows"]
        elif reorder:
            self.feOrder.to_caller(self.M.mult(MTU), out=_as_device_vector(u))
        else:
            self.M.mult(MTU, _as_device_vector(u))
        if hasattr(u, "invalidate_ghosts"):
            u.invalidate_ghosts()              # (new coefficients: ghost rows fetched before are stale)
        return MTU

    def _require_columns_within_halo(self, K):
        """Several ranks: the products of the Krylov solvers read the direction vector on this rank's dofs and the halo planes
        of its neighbours, addressed by K's column indices WITHOUT a range check.  The K of an assembled form stays inside; a
        coupling added by hand between far nodes (kept since the field engines count the entries of explicit blocks) does not
        -- the product would read outside the exchanged vector.  That is an error here, raised on every rank (one all-reduce
        of a flag per solve; the count is kept on the matrix).  Stored zeros outside (a far coupling zeroed with the boundary
        dofs) do not count."""
        dc = self.comm.device()
        if getattr(dc, "g0", None) is None:
            return                             # (no slab set on this communicator: nothing is exchanged through it)
        lo, hi = int(dc.g0 - dc.halo_lo), int(dc.g1 + dc.halo_hi)
        kept = getattr(K, "_beyond_halo", None)
        if kept is None or kept[0] != (lo, hi):
            n, ncols, far = K.shape[0], K.shape[1], 0
            for c0, c1 in ((0, lo), (hi, ncols)):
                if n > 0 and c1 > c0:
                    out = K.block(0, n, c0, c1)
                    if out.nnz:
                        far += int(numpy.count_nonzero(out.to_scipy().data))
            K._beyond_halo = kept = ((lo, hi), far)
        if dc.allreduce_sum([float(kept[1])])[0] > 0:
            raise NotImplementedError("solveLinearSystem on several ranks: K couples dofs that are further apart than the halo "
                                      "planes the Krylov vectors exchange (%d entries of this rank's rows lie outside the "
                                      "columns %d .. %d): a coupling added by hand between far nodes needs one rank" % (kept[1], lo, hi))

    # -- rank-local FE functions (tIGAr/common.py:1304-1348 runs on distributed PETSc vectors with ghost updates)
    def _register_ghosted(self, f):
        """``f`` is a rank-local Function whose ghost rows this spline fetches (weak reference, in registration order)"""
        import weakref
        f._ghoster = self.ghostedVector
        regs = self.__dict__.setdefault("_ghost_functions", [])
        regs[:] = [r for r in regs if r() is not None]
        if not any(r() is f for r in regs):
            regs.append(weakref.ref(f))

    def _new_ghost_epoch(self):
        """A new assembly: the ghost rows of every registered rank-local function are fetched NOW, by every rank -- also one
        whose slab holds no row block and whose forms therefore never ask (its neighbours would wait for it until the
        transport's time-out) -- and kept for the assembly (``Function.ghosted``)."""
        self._ghost_epoch = self.__dict__.get("_ghost_epoch", 0) + 1
        if self._distributed():
            for r in list(self.__dict__.get("_ghost_functions", [])):
                f = r()
                if f is not None and f.local_range is not None:
                    f.ghosted()

    def localFunction(self, u=None):
        """A Function that holds the FE rows this rank owns (``localFERange()``): a fresh one, or the rows of ``u`` cut out
        of a replicated full-length Function / vector.  The form objects read it through ``Function.ghosted()``."""
        rng = self.localFERange()
        f = Function(self.V, rng if self._distributed() else None)
        self._register_ghosted(f)
        if u is not None:
            src = _as_device_vector(u)
            if src.size() == f.vector().size():
                _dev.vec_copy_range(f.vector(), 0, src, 0, src.size())
            else:
                _dev.vec_copy_range(f.vector(), 0, src, int(rng[0]), int(rng[1]) - int(rng[0]))
        return f

    def gatherFunction(self, u):
        """The replicated, full-length Function of a rank-local one: every rank gets all FE rows (summed through the
        transport in rank order, the same bits everywhere).  After ``solveLinearSystem`` /
        ``solveNonlinearVariationalProblem`` on several ranks ``u.vector()`` holds THIS rank's FE rows only
        (``u.local_range``; the reference's distributed PETSc vector, tIGAr/common.py:1259-1261, 1343) -- code written for
        one rank that reads the whole solution (error norms, output) calls this first.  One rank, or a function that is
        already replicated: ``u`` itself."""
        vec = _as_device_vector(u)
        n = self.V.dim()
        if not self._distributed() or getattr(u, "local_range", None) is None or vec.size() == n:
            return u
        rng = u.local_range
        pieces = rng if (len(rng) and isinstance(rng[0], (tuple, list))) else [rng]
        host, full, pos = vec.get_local(), numpy.zeros(n), 0
        for (a, b) in pieces:
            a, b = int(a), int(b)
            full[a:b] = host[pos:pos + b - a]
            pos += b - a
        self.comm.transport().allreduce_sum(full)
        return Function(self.V, None, DeviceVector(data=full))

    def ghostedVector(self, u):
        """Full-length vector with the rank-local FE function ``u`` in place and the ghost rows the rank's forms read --
        the FE rows its rows of A couple to beyond its own, ``m_rows`` of its slab -- fetched from the z-neighbours
        (host-staged through the transport: one exchange per assembly, as dolfin's ghost update after ``u.assign``).
        Rows outside the window are zero."""
        vec = _as_device_vector(u)
        n = self.V.dim()
        if not self._distributed() or vec.size() == n:
            return vec
        if self.nFields != 1:
            raise NotImplementedError("ghost update of rank-local FE functions: one field")
        slab = self._slab_path()
        lay, world, rank = slab.layout, slab.world, slab.rank
        from .dist import split_range
        ranges = split_range(lay.ncp, world)
        own = [lay.slab(a, b)["u_rows"] for (a, b) in ranges]
        need = [lay.slab(a, b)["m_rows"] for (a, b) in ranges]
        # (a rank of a thin slab may own NO FE rows -- the layout reports (0, 0) -- but its forms still read a window: place
        #  the empty range where it belongs in the chain, at the end of the rows owned below it)
        pos = 0
        for r_ in range(world):
            if own[r_][1] <= own[r_][0]:
                own[r_] = (pos, pos)
            pos = own[r_][1]
        ua, ub = own[rank]
        if vec.size() != ub - ua:
            raise ValueError("ghostedVector: the function does not hold this rank's FE rows")
        host = vec.get_local()
        full = numpy.zeros(n)
        full[ua:ub] = host
        tr = self.comm.transport()
        # The transport links z-neighbours only, and a window may reach past the neighbour (slabs thinner than the
        # coupling), so the ghost rows travel in two sweeps along the chain of ranks.  The windows move upwards with the
        # rank, hence need[r-1] contains every row rank r wants from below (and need[r+1] every row it wants from above):
        # upwards, rank r first receives its lower ghost rows from r-1, then hands r+1 what that rank wants from below --
        # its own rows and, if the window is that long, rows it has just received; downwards likewise.  Which rows go
        # where follows from the layout alone.
        empty = numpy.zeros(0)
        if rank > 0 and ua > need[rank][0]:
            recv = numpy.zeros(ua - need[rank][0])
            tr.sendrecv(rank - 1, empty, recv, tag=71)
            full[need[rank][0]:ua] = recv
        if rank + 1 < world and own[rank + 1][0] > need[rank + 1][0]:
            tr.sendrecv(rank + 1, numpy.ascontiguousarray(full[need[rank + 1][0]:own[rank + 1][0]]), numpy.zeros(0), tag=71)
        if rank + 1 < world and need[rank][1] > ub:
            recv = numpy.zeros(need[rank][1] - ub)
            tr.sendrecv(rank + 1, empty, recv, tag=72)
            full[ub:need[rank][1]] = recv
        if rank > 0 and need[rank - 1][1] > own[rank - 1][1]:
            tr.sendrecv(rank - 1, numpy.ascontiguousarray(full[own[rank - 1][1]:need[rank - 1][1]]), numpy.zeros(0), tag=72)
        return DeviceVector(data=full)

    def globalNorm(self, v, kind="l2"):
        """Norm of an IGA vector over all ranks (PETSc VecNorm on the distributed M^T b, tIGAr/common.py:1330): the local
        sums go through the device communicator's all-reduce -- every rank gets the same bits."""
        if not self._distributed():
            return v.norm(kind)
        if kind != "l2":
            raise ValueError("globalNorm: l2")
        return float(numpy.sqrt(self.comm.device().allreduce_sum(numpy.array([v.inner(v)]))[0]))

    def _initial_guess_through_slabs(self, u):
        """The rank's rows of M^T u for a guess set in ``u``: a replicated full-length FE vector, or a Function that holds
        the rank's own FE rows as solveLinearSystem leaves it -- then with the ghost rows of the z-neighbours, so that the
        dofs next to a slab boundary get every contribution (the reference's MatMultTranspose on distributed vectors)"""
        vec = _as_device_vector(u)
        n = self.V.dim()
        if vec.size() == n:
            full = vec
        elif self.nFields == 1:
            full = self.ghostedVector(u)
        else:
            # several fields: the rank's own rows of every field in place (ghost rows count as zero: a guess, not a result)
            full = DeviceVector(n)
            off = 0
            for (a, b) in list(getattr(u, "local_range", None) or []):
                _dev.vec_copy_range(full, int(a), vec, off, int(b) - int(a))
                off += int(b) - int(a)

        def rows(r0, r1):
            piece = DeviceVector(r1 - r0)
            _dev.vec_copy_range(piece, 0, full, r0, r1 - r0)
            return piece
        return self._slab_path().assemble_vector(rows, None)

    def solveLinearVariationalProblem(self, residualForm, u, applyBCs=True):
        """``residualForm`` must be an ``Equation``-like object with ``.lhs`` / ``.rhs``
        forms (tIGAr/common.py:1266-1290)."""
        MTAM, MTb = self.assembleLinearSystem(residualForm.lhs, residualForm.rhs, applyBCs)
        return self.solveLinearSystem(MTAM, MTb, u)

    def setSolverOptions(self, maxIters=20, relativeTolerance=1e-5, linearSolver=None):
        """tIGAr/common.py:1292-1302."""
        self.maxIters = maxIters
        self.relativeTolerance = relativeTolerance
        self.linearSolver = linearSolver

    def FEtoIGA(self, u):
        """IGA dofs from the FE coefficients of ``u`` by the pseudo-inverse problem
        (M^T M) x = M^T u (tIGAr/common.py:968-994); uses ``self.linearSolver`` if set."""
        uv = _as_device_vector(u)
        MTtemp = self.extractVector(uv, applyBCs=False)
        ident = DeviceCSR.from_scipy(_scipy_identity(self.M.shape[0]))
        MTM = self._extract_matrix_grid(ident, applyBCs=False)       # (the identity is the same in every order)
        x = DeviceVector(self.M.shape[1])
        solver = self.linearSolver if self.linearSolver is not None else _default_linear_solver("cg")
        solver.solve(MTM, x, MTtemp)
        return x

    # -- projection, error norms, quadrature-point evaluation (csrc/tg_postproc.hip)
    def _point_scope(self, who, nfields=None, shared_dims=None):
        """Refuses what the quadrature-point operands and point forms do not cover.  They serve one mapped tensor-product
        patch held by one rank, in the order of the node grid, with continuous Q_p fields.  What differs between the kinds
        of point forms comes as data: ``nfields`` the number of fields they take (None: any), ``shared_dims`` the parametric
        dimensions d of those whose fields must lie on the control mesh's scalar basis and share one node grid."""
        no = NotImplementedError
        if self._distributed():
            raise no("%s: several ranks are not supported (the point values are numbered over the whole patch)" % who)
        if self._implicit():
            raise no("%s: the streamed engine asks its forms for row blocks, which the point forms do not hand out" % who)
        if self._caller_ordered():
            raise no("%s: a spline with the caller's FE dof order (feOrder) is not supported; the point kernels number the "
                     "node grid" % who)
        gen = getattr(self, "_generator", None)
        if isinstance(gen, FieldListSpline):
            raise no("%s: FieldListSpline spaces (fields on their own bases) are not supported" % who)
        on_control = getattr(gen, "_fields_on_control_basis", None)
        if shared_dims is not None and on_control is not None and not on_control():
            raise no("%s: the fields of %s are not discretised with the control mesh's scalar basis (FieldListSpline and "
                     "compatible spaces are not supported)" % (who, type(gen).__name__))
        grids = getattr(self.V, "grids", None)
        if grids is None or len(grids) != self.nFields or any(not isinstance(g, TensorNodeGrid) or g.dg for g in grids):
            raise no("%s: the FE fields are not continuous Q_p fields of a single tensor-product patch (FieldListSpline, "
                     "compatible, multi-patch, T-spline and DG spaces are not supported)" % who)
        if nfields is not None and self.nFields != nfields:
            raise no("%s: nFields = %d; %s" % (who, self.nFields, "only scalar spaces are supported" if nfields == 1 else
                     "on a patch with nsd = %d the displacement has as many fields as there are physical directions" % nfields))
        if shared_dims is not None:
            g = grids[0]
            if any(gi.degree != g.degree or gi.shape() != g.shape() for gi in grids[1:]):
                raise no("%s: the fields do not share one node grid (compatible spaces are not supported)" % who)
            if g.dim() not in shared_dims:
                raise no("%s: d = %d parametric directions; second-derivative point forms are provided for curves and "
                         "surfaces (d = 1, 2)" % (who, g.dim()))

    def _quadrature_scope(self, who):
        """the scalar point operands: one field"""
        self._point_scope(who, nfields=1)

    def _vector_quadrature_scope(self, who):
        """the point forms of a vector-valued unknown: nFields = nsd (``EqualOrderSpline(nsd, mesh)``)"""
        self._point_scope(who, nfields=self.nsd)

    def _jet_scope(self, who):
        """the second-derivative point forms (csrc/tg_jet.hip): nF >= 1 fields on the control basis sharing one node grid,
        d = 1 or 2 parametric directions and nsd >= d"""
        self._point_scope(who, shared_dims=(1, 2))

    def _system_quadrature_scope(self, who):
        """the point forms of a first-order system: nF >= 1 fields on the control basis sharing one node grid, d = 1, 2, 3"""
        self._point_scope(who, shared_dims=(1, 2, 3))

    def evaluateJetsAtQuadrature(self, u, nq=None, rational=False):
        """The JET of u_h (``rational``: of u_h / W_h) at the quadrature points: value, first parametric derivatives, second
        parametric derivatives in the order 00, 01, 11 -- ``spline.parametricGrad`` of the reference and its derivative, with
        respect to the patch's knot coordinates.  A DeviceVector of nJ * npts values (nJ = 3 for d = 1, 6 for d = 2),
        component alpha at alpha * npts + q, points numbered as ``quadraturePoints``; for nFields > 1 a list with one per
        field (``tg_quad_jet``)."""
        from . import forms
        who = "evaluateJetsAtQuadrature"
        self._jet_scope(who)
        pts = forms.quadrature_points(self, self.V_control, nq, who)
        uv = _as_device_vector(u)
        n = self.V.grids[0].num_nodes()
        if uv.size() != self.nFields * n:
            raise ValueError("%s: %d nodal values given, the space has %d" % (who, uv.size(), self.nFields * n))
        jet = lambda ui: _dev.quad_jet(pts.verts, pts.p, pts.cp, ui, nq=pts.nq, rational=rational)
        return jet(uv) if self.nFields == 1 else forms._field_by_field(uv, self.nFields, n, jet)

    def geometryJetsAtQuadrature(self, nq=None):
        """The jets of the physical coordinates x_c = N_c / W_h at the quadrature points: a DeviceVector of nsd * nJ * npts
        values, component alpha of coordinate c at (c nJ + alpha) npts + q (``tg_quad_geometry_jet``)."""
        from . import forms
        who = "geometryJetsAtQuadrature"
        self._jet_scope(who)
        pts = forms.quadrature_points(self, self.V_control, nq, who)
        return _dev.quad_geometry_jet(pts.verts, pts.p, pts.cp, nq=pts.nq)

    def quadraturePoints(self, nq=None):
        """The Gauss points of the patch (``nq`` per direction, p + 1 when None) as a ``forms.QuadraturePoints``: ``.x``
        (host array [npts, nsd], downloaded on first use), ``.x_device``, ``.weights`` (DeviceVector of w_q sqrt(det g)
        prod h_k), ``.nq``, ``.npts``; kept per ``nq`` and per set of control-function vectors (the geometry is taken as
        frozen: values written into those vectors in place after the first call are not noticed).  Numbering: element-major, elements and the nq^d points of an
        element lexicographic with direction 0 fastest."""
        from . import forms
        self._quadrature_scope("quadraturePoints")
        return forms.quadrature_points(self, self.V, nq, "quadraturePoints")

    def rationalize(self, u):
        """The FE ``Function`` with the nodal values u_i / w_i, w = ``cpFuncs[nsd]`` (tIGAr/common.py:923-932 divides the
        UFL expression by the weight function; the NURBS demo's "the solution would be u/F3").  This is the NODAL quotient:
        the interpolant of u_h / W_h on the FE nodes, what a file of nodal values for plotting needs.  The quotient at
        the quadrature points is ``evaluateAtQuadrature(u, rational=True)``; the norms take ``rational=True``."""
        uv = _as_device_vector(u)
        w = self.cpFuncs[self.nsd].vector()
        if uv.size() != w.size():
            raise ValueError("rationalize: %d nodal values given, the weight function has %d" % (uv.size(), w.size()))
        out = Function(self.V)
        uv.pointwise_divide(w, out=out.vector())
        return out

    def evaluateAtQuadrature(self, u, grad=False, nq=None, rational=False):
        """u_h at the quadrature points for an FE ``Function`` (or nodal vector) ``u``: a DeviceVector, or with ``grad``
        ``(values, [nsd DeviceVectors])`` with the components of the Cartesian gradient (``spline.grad``: pinv(DF) and
        the quotient rule of the rational map).  ``rational``: u_h / W_h and its gradient -- the reference's
        ``spline.rationalize(u)`` for the solution of the rational forms."""
        pts = self.quadraturePoints(nq)
        uv = _as_device_vector(u)
        if uv.size() != self.V.dim():
            raise ValueError("evaluateAtQuadrature: %d nodal values given, the space has %d" % (uv.size(), self.V.dim()))
        if not grad:
            return _dev.quad_eval(pts.verts, pts.p, pts.cp, uv, nq=pts.nq, rational=rational)
        val, g = _dev.quad_eval(pts.verts, pts.p, pts.cp, uv, grad=True, nq=pts.nq, rational=rational)
        comps = []
        for i in range(pts.nsd):
            c = DeviceVector(pts.npts, zero=False)
            _dev.vec_copy_range(c, 0, g, i * pts.npts, pts.npts)
            comps.append(c)
        return val, comps

    # -- evaluation at points the caller chooses, closest points, lattices, VTK files (csrc/tg_sample.hip, tigar_amd/vtkio.py)
    def _sample_patch(self, who):
        """(element vertices, degree, control functions, node grid) of the patch the sampling operands work on: the scope
        of the first-order systems (nF >= 1 fields on the control basis sharing one node grid)"""
        from . import forms
        self._system_quadrature_scope(who)
        g = self.V.grids[0]
        return forms._whole_patch(self, g, who, "the sampling operands") + (g,)

    def _sample_nodal(self, u, g, who, control=False):
        """(nodal DeviceVector, number of fields) of ``u`` on the spline's space (``control``: or on the scalar control space)"""
        uv, n = _as_device_vector(u), g.num_nodes()
        if uv.size() == self.nFields * n:
            return uv, self.nFields
        if control and uv.size() == n:
            return uv, 1
        raise ValueError("%s: %d nodal values given, the space has %d%s"
                         % (who, uv.size(), self.nFields * n, " (the scalar control space %d)" % n if control else ""))

    @staticmethod
    def _sample_points(a, ncomp, who, name):
        """(DeviceVector in the component-major layout, npts) of a host array [npts, ncomp] or a DeviceVector in that layout"""
        from . import forms
        if isinstance(a, DeviceVector):
            if a.size() % ncomp:
                raise ValueError("%s: %s holds %d values, not a multiple of %d" % (who, name, a.size(), ncomp))
            return a, a.size() // ncomp
        a = numpy.asarray(a, dtype=numpy.float64)
        if a.ndim == 1 and ncomp == 1:
            a = a[:, None]
        if a.ndim != 2 or a.shape[1] != ncomp:
            raise ValueError("%s: %s of shape %s; expected [npts, %d]" % (who, name, a.shape, ncomp))
        return DeviceVector(data=forms.point_block(a, a.shape[0], (ncomp,))), a.shape[0]

    @staticmethod
    def _sample_split(val, g, nF, nsd, npts):
        """the results of nF fields as the caller gets them: per field ``values`` or ``(values, [nsd gradient components])``,
        one such for nF = 1 and a list beyond"""
        def piece(src, off):
            c = DeviceVector(npts, zero=False)
            _dev.vec_copy_range(c, 0, src, off * npts, npts)
            return c
        out = []
        for i in range(nF):
            v = val if nF == 1 else piece(val, i)
            out.append(v if g is None else (v, [piece(g, i * nsd + K) for K in range(nsd)]))
        return out[0] if nF == 1 else out

    def evaluateAtPoints(self, u, xi, grad=False, rational=False):
        """u_h at the parametric points ``xi`` (host array [npts, d] of knot coordinates, or a DeviceVector of d * npts
        values, component-major) for an FE ``Function`` or nodal vector ``u``: a DeviceVector of npts values, with ``grad``
        ``(values, [nsd DeviceVectors])`` with the Cartesian gradient, for nFields > 1 a list with one such per field
        (``tg_point_eval``).  A point outside the parametric box gets NaN.  ``rational``: u_h / W_h and its gradient."""
        who = "evaluateAtPoints"
        verts, p, cp, g = self._sample_patch(who)
        uv, nF = self._sample_nodal(u, g, who)
        xiv, npts = self._sample_points(xi, len(verts), who, "xi")
        _, val, gr = _dev.point_eval(verts, p, cp, xiv, uv, nF=nF, grad=grad, rational=rational)
        return self._sample_split(val, gr, nF, len(cp) - 1, npts)

    def physicalPoints(self, xi):
        """x = F(xi) of the parametric points ``xi`` (as for ``evaluateAtPoints``): a host array [npts, nsd]"""
        from . import forms
        who = "physicalPoints"
        verts, p, cp, g = self._sample_patch(who)
        xiv, npts = self._sample_points(xi, len(verts), who, "xi")
        x = _dev.point_eval(verts, p, cp, xiv, x=True)[0]
        return forms.point_unblock(x.get_local(), npts, (len(cp) - 1,))

    def locatePoints(self, x, guess=None, tol=1e-12, maximum_iterations=50, max_seeds=32768):
        """The closest points of the patch to the physical points ``x`` (host array [npts, nsd] or a DeviceVector of nsd *
        npts values): the inverse map for points of the image, the projection for points off a curve or surface or outside.
        Damped Gauss-Newton steps from ``guess`` (parametric points as for ``evaluateAtPoints``) or from the nearest centre
        of at most ``max_seeds`` elements, until the step is below ``tol`` times the parametric range
        (``tg_point_locate``; without second derivatives: linear convergence for a point at a distance).  Returns a
        ``forms.LocatedPoints``."""
        from . import forms
        who = "locatePoints"
        verts, p, cp, g = self._sample_patch(who)
        if not tol > 0.0:
            raise ValueError("%s: tol = %r; a positive tolerance" % (who, tol))
        if int(maximum_iterations) != maximum_iterations or not 1 <= int(maximum_iterations) <= 100:
            raise ValueError("%s: maximum_iterations = %r; 1..100" % (who, maximum_iterations))
        if int(max_seeds) != max_seeds or int(max_seeds) < 1:
            raise ValueError("%s: max_seeds = %r; at least one seed" % (who, max_seeds))
        xv, npts = self._sample_points(x, len(cp) - 1, who, "x")
        gv = None
        if guess is not None:
            gv, ng = self._sample_points(guess, len(verts), who, "guess")
            if ng != npts:
                raise ValueError("%s: %d starting values for %d points" % (who, ng, npts))
        xi, info = _dev.point_locate(verts, p, cp, xv, gv, tol, maximum_iterations, max_seeds)
        return forms.LocatedPoints(xi, info, len(verts))

    def evaluateAtPhysicalPoints(self, u, x, grad=False, rational=False, **locate_options):
        """``evaluateAtPoints`` at the closest points of the patch to the physical points ``x``: ``(values..., located)``
        with what ``evaluateAtPoints`` returns followed by the ``forms.LocatedPoints`` (check ``located.distance``: a point
        off the patch is evaluated at its projection).  ``locate_options``: those of ``locatePoints``."""
        located = self.locatePoints(x, **locate_options)
        res = self.evaluateAtPoints(u, located.xi_device, grad=grad, rational=rational)
        return (res if isinstance(res, tuple) else (res,)) + (located,)

    def latticePoints(self, m=None):
        """The sampling lattice of the patch as a ``forms.LatticePoints``: ``m`` an int (that many equispaced abscissae per
        element and direction, the ends included; 1: the centre), a sequence of abscissae in [0, 1], or None: p + 1.  Kept
        per (abscissae, control-function vectors)."""
        from . import forms
        who = "latticePoints"
        self._system_quadrature_scope(who)
        return forms.lattice_points(self, self.V.grids[0], m, who)

    def evaluateAtLattice(self, u, m=None, grad=False, rational=False):
        """``evaluateAtQuadrature`` on the lattice ``latticePoints(m)`` in the place of the Gauss points, for nFields >= 1
        (a list with one result per field beyond one; ``tg_lattice_eval``)"""
        from . import forms
        who = "evaluateAtLattice"
        pts = self.latticePoints(m)
        g = self.V.grids[0]
        uv, nF = self._sample_nodal(u, g, who, control=True)
        n, nsd = g.num_nodes(), pts.nsd
        call = lambda ui: _dev.lattice_eval(pts.verts, pts.p, pts.cp, pts.t, ui, grad=grad, rational=rational)
        if nF == 1:
            res = call(uv)
            return self._sample_split(res[0], res[1], 1, nsd, pts.npts) if grad else res
        if not grad:
            return forms._field_by_field(uv, nF, n, call)
        return [self._sample_split(v, gr, 1, nsd, pts.npts) for v, gr in forms._field_by_field(uv, nF, n, call)]

    def writeVTK(self, path, fields, m=None, rational=False, displacement=None, time=None, encoding="raw"):
        """Writes ``fields`` = {name: Function | nodal vector} (on the spline's space or on the scalar control space) sampled
        on the lattice ``latticePoints(m)`` (m >= 2 points per element and direction) as a VTK XML unstructured grid of
        linear cells, (m - 1)^d per element: the points are the physical lattice points x = F(xi), plus the interpolated
        ``displacement`` (nsd fields) if given -- the deformed shell --, the data come from ``evaluateAtLattice``.  A
        function with nsd fields is written as one vector array, one field as the array ``name``, any other number as
        ``name_i`` per field.  ``path`` ending in .vtu: that file; in .pvd: a further step (stem000000.vtu, ...) of the
        collection, at ``time`` (the step number when None).  Returns the name of the .vtu file written."""
        from . import forms, vtkio
        who = "writeVTK"
        pts = self.latticePoints(m)
        if pts.m < 2:
            raise ValueError("%s: a lattice of %d point per element and direction has no cells; m >= 2" % (who, pts.m))
        nsd = pts.nsd

        def sampled(u):
            r = self.evaluateAtLattice(u, pts.t, rational=rational)
            return numpy.stack([v.get_local() for v in (r if isinstance(r, list) else [r])], axis=1)
        X = pts.x.copy()
        if displacement is not None:
            D = sampled(displacement)
            if D.shape[1] != nsd:
                raise ValueError("%s: the displacement has %d fields, the patch %d physical directions" % (who, D.shape[1], nsd))
            X += D
        data = {}
        for name, u in fields.items():
            A = sampled(u)
            if A.shape[1] == 1:
                data[str(name)] = A[:, 0]
            elif A.shape[1] == nsd and nsd <= 3:
                data[str(name)] = A
            else:
                for i in range(A.shape[1]):
                    data["%s_%d" % (name, i)] = A[:, i]
        cells, ctype = pts.cells()
        series = self.__dict__.setdefault("_vtk_series", {})
        return vtkio._series_step(str(path), series.setdefault(str(path), []), time,
                                  lambda f: vtkio.write_vtu(f, X, cells, ctype, data, encoding))

    def integrate(self, f, nq=None):
        """sum_q wdet_q f(x_q): the integral of ``f`` over the patch with the spline's measure; ``f`` as for
        ``forms.QuadratureLoadForm`` (callable on the points, number, point values, Function)."""
        pts = self.quadraturePoints(nq)
        return pts.weights.inner(pts.values(f, "integrate"))

    # -- boundary integrals (csrc/tg_boundary.hip): the reference's spline.ds and spline.n
    def boundaryPoints(self, direction, side, nq=None):
        """The Gauss points of the face (direction, side) -- numbered as ``getSideDofs`` -- as a ``forms.FacePoints``:
        ``.x`` (host array [npts, nsd], lazy), ``.x_device``, ``.weights`` (the surface weights, ``spline.ds``),
        ``.normals`` (the unit normal ``spline.n``, nsd * npts values, component-major), ``.h_normal``, ``.npts``, ``.nq``;
        kept per (face, nq, control-function vectors) like the volume points."""
        from . import forms
        self._quadrature_scope("boundaryPoints")
        return forms.face_points(self, self.V, direction, side, nq, "boundaryPoints")

    def evaluateAtBoundary(self, u, direction, side, grad=False, normal_derivative=False, nq=None, rational=False):
        """u_h at the points of a face for an FE ``Function`` (or nodal vector): a DeviceVector; with ``grad`` and / or
        ``normal_derivative`` a tuple ``(values[, [nsd DeviceVectors of the Cartesian gradient]][, d_n u])``.
        ``rational``: u_h / W_h."""
        pts = self.boundaryPoints(direction, side, nq)
        uv = _as_device_vector(u)
        if uv.size() != self.V.dim():
            raise ValueError("evaluateAtBoundary: %d nodal values given, the space has %d" % (uv.size(), self.V.dim()))
        val, g, dn = _dev.face_eval(pts.verts, pts.p, pts.cp, pts.direction, pts.side, uv, grad=grad,
                                    normal_derivative=normal_derivative, nq=pts.nq, rational=rational)
        out = [val]
        if grad:
            comps = []
            for i in range(pts.nsd):
                c = DeviceVector(pts.npts, zero=False)
                _dev.vec_copy_range(c, 0, g, i * pts.npts, pts.npts)
                comps.append(c)
            out.append(comps)
        if normal_derivative:
            out.append(dn)
        return out[0] if len(out) == 1 else tuple(out)

    def _boundary_faces(self, faces, who):
        from . import forms
        self._quadrature_scope(who)
        return forms.check_faces(faces, self.V.grids[0].dim(), who, forms._periodic_directions(self))

    def integrateBoundary(self, f, faces=None, nq=None):
        """sum over the faces of sum_q wsurf_q f(x_q): the integral of ``f`` over (part of) the boundary with
        ``spline.ds``.  ``f``: a callable on the points (of ``x`` or of ``(x, n)``), a number, a ``Function``, or a list
        with point values / one of these per face; ``faces=None``: all 2 d faces."""
        from . import forms
        faces = self._boundary_faces(faces, "integrateBoundary")
        total = 0.0
        for i, (k, s) in enumerate(faces):
            pts = self.boundaryPoints(k, s, nq)
            total += pts.weights.inner(forms._face_values(pts, forms._per_face(f, i, len(faces), "integrateBoundary"),
                                                          "integrateBoundary"))
        return total

    def boundaryFlux(self, u, faces=None, nq=None, rational=False):
        """sum over the faces of sum_q wsurf_q d_n u(x_q): the flux of grad u through (part of) the boundary"""
        faces = self._boundary_faces(faces, "boundaryFlux")
        total = 0.0
        for k, s in faces:
            pts = self.boundaryPoints(k, s, nq)
            total += pts.weights.inner(self.evaluateAtBoundary(u, k, s, normal_derivative=True, nq=nq, rational=rational)[1])
        return total

    def errorNorm(self, u, exact, kind="L2", exact_grad=None, nq=None, relative=False, rational=False):
        """Error of the FE ``Function`` (or nodal vector) ``u`` against ``exact`` in dolfin's ``errornorm`` kinds: "L2",
        "H10" (the seminorm of the Cartesian gradient) or "H1" = sqrt(L2^2 + H10^2).  ``exact`` / ``exact_grad``:
        callables on the physical points [npts, nsd] -> [npts] / [npts, nsd], numbers or point-value arrays;
        ``exact_grad`` is required for "H10" / "H1".  ``relative``: divided by the same norm of ``exact``.  ``rational=False``:
        ``u`` is taken un-rationalised (the polynomial spline pushed forward by the map), as the forms without the keyword
        take their unknown; ``rational=True``: the error of u_h / W_h, the reference's
        ``(spline.rationalize(u) - soln)**2`` for the solution of the forms with ``rational=True``."""
        if kind not in ("L2", "H10", "H1"):
            raise ValueError("errorNorm: unknown kind %r (L2, H10, H1)" % (kind,))
        if kind != "L2" and exact_grad is None:
            raise ValueError("errorNorm: kind %r needs exact_grad" % (kind,))
        pts = self.quadraturePoints(nq)
        uv = _as_device_vector(u)
        if uv.size() != self.V.dim():
            raise ValueError("errorNorm: %d nodal values given, the space has %d" % (uv.size(), self.V.dim()))
        e = pts.values(exact, "errorNorm: exact")
        ge = pts.vector_values(exact_grad, "errorNorm: exact_grad") if kind != "L2" else None
        s0, s1, e2 = _dev.quad_error(pts.verts, pts.p, pts.cp, uv, e, ge, nq=pts.nq, rational=rational)
        num = {"L2": s0, "H10": s1, "H1": s0 + s1}[kind]
        if not relative:
            return float(numpy.sqrt(num))
        g2 = _dev.quad_error(pts.verts, pts.p, pts.cp, None, None, ge, nq=pts.nq)[1] if kind != "L2" else 0.0
        den = {"L2": e2, "H10": g2, "H1": e2 + g2}[kind]
        return float(numpy.sqrt(num / den))

    def projectDofs(self, toProject, applyBCs=False, lumpMass=False, linearSolver=None, nq=None, rational=False):
        """IGA dofs of the L2 projection of ``toProject`` (given as for ``forms.QuadratureLoadForm``) onto the spline space
        (tIGAr/common.py:1392-1433).  Consistent: ``M^T A_mass M U = M^T b`` with the load and the mass matrix integrated by
        the same ``nq`` points, so that a function of the space is reproduced whatever the quadrature error; solved by
        ``linearSolver``, else ``self.linearSolver``, else the default solver; the extracted mass matrix is kept per
        ``(applyBCs, nq, zeroDofs)`` (``_projection_mass``; ``_projection_mass_builds`` counts the assemblies); like the
        quadrature points it is computed from the control functions as they are at the first call -- control functions
        overwritten in place afterwards are not noticed (new vectors are).  ``lumpMass``:
        ``U = M^T b ./ M^T (load of 1)``, the denominator extracted without the boundary conditions as in the reference
        (common.py:1416-1430); no matrix.  ``rational``: the projection in the rational space, as the reference projects
        (trial and test function rationalised, common.py:1408-1409): rational load, rational mass matrix, the dofs of the
        homogeneous function u_h = W_h u."""
        from . import forms
        self._quadrature_scope("projectDofs")
        nq = forms._check_nq(nq, int(self.V.grids[0].degree))
        rational = bool(rational)
        rhs = self.assembleVector(forms.QuadratureLoadForm(toProject, self, nq, rational=rational), applyBCs=applyBCs)
        if lumpMass:
            den = self.assembleVector(forms.QuadratureLoadForm(1.0, self, nq, rational=rational), applyBCs=False)
            return rhs.pointwise_divide(den)
        cache = self.__dict__.setdefault("_projection_mass", {})
        # (the zero dofs are part of the key: a spline whose zeroDofs were changed after a projection gets a new matrix)
        key = (bool(applyBCs), nq, numpy.asarray(self.zeroDofs).tobytes() if applyBCs else b"") + ((True,) if rational else ())
        if key not in cache:
            cache[key] = self.assembleMatrix(forms.MassForm(geometry=self, nq=nq, rational=rational), applyBCs=applyBCs)
            self._projection_mass_builds = self.__dict__.get("_projection_mass_builds", 0) + 1
        U = DeviceVector(cache[key].shape[0])
        solver = linearSolver if linearSolver is not None else \
            (self.linearSolver if self.linearSolver is not None else _default_linear_solver())
        solver.solve(cache[key], U, rhs)
        return U

    def project(self, toProject, applyBCs=False, rationalize=False, lumpMass=False, rational=False):
        """FE ``Function`` M * projectDofs(...) (tIGAr/common.py:1392-1433).  ``rational`` selects the space the projection
        is taken in (see ``projectDofs``); ``project(f, rational=True, rationalize=False)`` is the reference's
        ``project(f, rationalize=False)``: the homogeneous function u_h, whose quotient by the weight function approximates
        f.  ``rationalize`` (whether the RETURNED function is divided as well) keeps its meaning: with unit weights it
        changes nothing, with others ``rationalize=True`` is refused (``spline.rationalize(u)`` gives the nodal quotient)."""
        if rationalize:
            w = self.cpFuncs[self.nsd].vector().get_local()
            if numpy.max(numpy.abs(w - 1.0)) > 64 * numpy.finfo(numpy.float64).eps:      # (unit up to the extraction's rounding)
                raise NotImplementedError("project(rationalize=True): the control mesh has non-unit weights, and dividing the "
                                          "returned FE function by the weight function W_h is not implemented (the quotient "
                                          "is no function of the FE space); spline.rationalize(u) gives the nodal quotient, "
                                          "evaluateAtQuadrature(u, rational=True) the quotient at the quadrature points")
        U = self.projectDofs(toProject, applyBCs=applyBCs, lumpMass=lumpMass, rational=rational)
        u = Function(self.V)
        self.M.mult(U, u.vector())
        return u

    def solveNonlinearVariationalProblem(self, residualForm, J, u, referenceError=None, igaDoFs=None, absoluteTolerance=0.0,
                                         phaseSeconds=None):
        """Newton iteration of tIGAr/common.py:1304-1348, same control flow: assemble
        (M^T J M, M^T R) at the current ``u``, stop when ||M^T R|| / reference < relativeTolerance
        (reference = first norm unless given), else solve for the increment and ``u <- u - du``
        (``igaDoFs -= increment`` when IGA dofs are passed; they also seed ``u = M*igaDoFs``).
        ``residualForm`` / ``J`` are form objects whose ``assemble_vector`` / ``assemble_matrix``
        read the current state of ``u`` (as UFL forms reference their coefficient).  Prints the
        reference's progress line; non-convergence raises instead of the reference's exit().
        Returns the list of relative norms.  Two additions, both off by default: with ``absoluteTolerance`` > 0 the iteration
        also stops, before any solve, when the FIRST ||M^T R|| is at most that (the relative test divides by the first norm
        and cannot pass when the start is already converged; the history is then ``[1.0]``); ``phaseSeconds``, a dict, gets
        the seconds of the assemblies added under "assembly" and those of the solves under "solve" (three device
        synchronisations per iteration)."""
        if self._caller_ordered():
            raise NotImplementedError("solveNonlinearVariationalProblem: the forms read the Function in the order of the node "
                                      "grid; a caller-ordered spline is not supported")
        returningDoFs = igaDoFs is not None
        dist = self._distributed()
        if dist:
            # several ranks: u, du and igaDoFs are rank-local (FE rows localFERange(), dofs localDofRange()), the norm is
            # global, the forms read u through Function.ghosted() -- the reference's loop on distributed PETSc vectors.
            # NOTE: a replicated ``u`` handed in becomes rank-local IN PLACE (u.vector() = this rank's rows, u.local_range
            # set); ``gatherFunction(u)`` returns the full-length function again
            if u.local_range is None:
                loc = self.localFunction(u)          # a replicated Function: every rank keeps its rows
                u._vec, u.local_range = loc.vector(), loc.local_range
            self._register_ghosted(u)
            if returningDoFs:
                u._vec = self._slab_path().prolong(igaDoFs)
        uv = _as_device_vector(u)
        if returningDoFs and not dist:
            self.M.mult(igaDoFs, uv)
        history = []
        converged = False
        def clock():
            if phaseSeconds is None:
                return None
            _dev.sync()
            return time.perf_counter()
        for i in range(0, self.maxIters):
            t0 = clock()
            MTAM, MTb = self.assembleLinearSystem(J, residualForm)
            currentNorm = self.globalNorm(MTb, "l2")
            t1 = clock()
            if phaseSeconds is not None:
                phaseSeconds["assembly"] = phaseSeconds.get("assembly", 0.0) + (t1 - t0)
            if i == 0 and absoluteTolerance > 0.0 and currentNorm <= absoluteTolerance:
                history.append(1.0)
                converged = True
                break
            if i == 0 and referenceError is None:
                referenceError = currentNorm
            relativeNorm = currentNorm / referenceError
            history.append(relativeNorm)
            if mpirank == 0:
                print("Solver iteration: " + str(i) + " , Relative norm: " + str(relativeNorm))
                sys.stdout.flush()
            if relativeNorm < self.relativeTolerance:
                converged = True
                break
            du = Function(self.V, self.localFERange() if dist else None)
            igaIncrement = self.solveLinearSystem(MTAM, MTb, du)
            if phaseSeconds is not None:
                phaseSeconds["solve"] = phaseSeconds.get("solve", 0.0) + (clock() - t1)
            uv.axpy(-1.0, du.vector())
            if hasattr(u, "invalidate_ghosts"):
                u.invalidate_ghosts()
            if returningDoFs:
                igaDoFs.axpy(-1.0, igaIncrement)
        if not converged:
            raise RuntimeError("Nonlinear solver failed to converge.")
        return history



def _scipy_identity(n):
    import scipy.sparse as _sp
    return _sp.identity(n, format="csr")


class NewtonSolver(object):
    """Minimal stand-in for dolfin ``NewtonSolver`` [ext] driving an ``ExtractedNonlinearProblem``:
    ``parameters`` relative_tolerance / absolute_tolerance / maximum_iterations /
    relaxation_parameter; linear solves through ``linear_solver`` (``.solve(A,x,b)``) or the
    spline's."""

    def __init__(self, linear_solver=None):
        self.linear_solver = linear_solver
        self.parameters = {"relative_tolerance": 1e-9, "absolute_tolerance": 1e-10,
                           "maximum_iterations": 50, "relaxation_parameter": 1.0,
                           "error_on_nonconvergence": True}
        self.last = {}

    def solve(self, problem, x):
        prm = self.parameters
        r0 = None
        for it in range(int(prm["maximum_iterations"]) + 1):
            problem.form(None, None, None, x)
            b = problem.F(None, x)
            rn = b.norm("l2")
            r0 = rn if r0 is None else r0
            self.last = {"iterations": it, "residual": rn, "relative": rn / r0 if r0 > 0 else 0.0}
            if rn < prm["absolute_tolerance"] or (r0 > 0 and rn / r0 < prm["relative_tolerance"]):
                return it, True
            if it == int(prm["maximum_iterations"]):
                break
            A = problem.J(None, x)
            dx = DeviceVector(x.size())
            ls = self.linear_solver or problem.spline.linearSolver or _default_linear_solver()
            ls.solve(A, dx, b)
            x.axpy(-float(prm["relaxation_parameter"]), dx)
        if prm["error_on_nonconvergence"]:
            raise RuntimeError("Newton solver did not converge")
        return int(prm["maximum_iterations"]), False


class ExtractedNonlinearProblem(object):
    """Nonlinear problem posed on an extracted spline for external Newton/SNES-type solvers
    (tIGAr/common.py:504-545): ``form`` pushes the IGA dofs into the FE solution (M*x), ``F`` / ``J``
    return the extracted residual / tangent."""

    def __init__(self, spline, residual, tangent, solution, **kwargs):
        if getattr(spline, "feOrder", None) is not None and not spline.feOrder.is_identity:
            raise NotImplementedError("ExtractedNonlinearProblem: the forms read the solution Function in the order of the "
                                      "node grid; a caller-ordered spline is not supported")
        self.spline, self.residual, self.tangent, self.solution = spline, residual, tangent, solution

    def form(self, A, P, B, x):
        self.spline.M.mult(x, self.solution.vector())

    def F(self, b, x):
        return self.spline.assembleVector(self.residual)

    def J(self, A, x):
        return self.spline.assembleMatrix(self.tangent)


class ExtractedNonlinearSolver(object):
    """tIGAr/common.py:547-584: initial IGA dofs by ``FEtoIGA`` of the current solution, solve, then
    the FE representation of the result is stored in ``problem.solution``."""

    def __init__(self, problem, solver):
        self.problem, self.solver = problem, solver

    def solve(self):
        tempVec = self.problem.spline.FEtoIGA(self.problem.solution)
        self.solver.solve(self.problem, tempVec)
        self.problem.spline.M.mult(tempVec, self.problem.solution.vector())
        return tempVec


# the eigensolver look-alike (tigar_amd/eigen.py: block LOBPCG on the device)
from .eigen import SLEPcEigenSolver  # noqa: E402,F401
