"""
FE-side INPUT generators for tensor-product patches with identity geometry (parametric ==
physical, as with ``ExplicitBSplineControlMesh``).  In the reference these matrices and
vectors come from ``dolfin.assemble(form)`` (tIGAr/common.py:1162-1220), which is outside
the extraction hot path; this module produces the same objects for the Q_p Lagrange space
on the knot mesh so that the path can be driven (and benchmarked) without FEniCS:

    LaplaceForm()            a(u,v) = (grad u, grad v)     -> K1xM1xM1 + M1xK1xM1 + M1xM1xK1
    MassForm()               a(u,v) = (u, v)
    SeparableLoadForm(f1d)   L(v)   = (f, v) with f(x) = scale * prod_k f1d[k](x_k)
    QuadratureLoadForm(f, geometry)   L(v) = (f, v) on a mapped patch, f given at the quadrature points
    CoefficientForm(geometry, ...)    a(u,v) with diffusion, advection and reaction coefficients at the quadrature points
    QuasilinearResidual(u, geometry, residual, tangent)   Newton on a point-wise nonlinear flux / source

Quadrature: Gauss-Legendre with p+1 points per direction (what ``quadrature_degree = 2p``
selects on quads/hexes [ext], demos/poisson/poisson.py:89).  The d-dimensional objects are
expanded on the GPU (``tg_kron_sum_csr`` / ``tg_vec_tensor3``); they are NOT timed as part
of the hot path.
"""
import collections

import numpy
import scipy.sparse as sp

from . import device as _dev


def _gauss01(n):
    x, w = numpy.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def _lagrange01(p, t):
    nodes = numpy.arange(p + 1) / float(p)
    phi = numpy.ones((p + 1, len(t)))
    dphi = numpy.zeros((p + 1, len(t)))
    for a in range(p + 1):
        others = [m for m in range(p + 1) if m != a]
        for m in others:
            phi[a] *= (t - nodes[m]) / (nodes[a] - nodes[m])
        for m in others:
            term = numpy.full(len(t), 1.0 / (nodes[a] - nodes[m]))
            for q in others:
                if q != m:
                    term *= (t - nodes[q]) / (nodes[a] - nodes[q])
            dphi[a] += term
    return phi, dphi


def fe_matrices_1d(vertices, p, nq=None):
    """1-D CG Lagrange degree-p (mass, stiffness) on the mesh with the given vertices, as
    scipy CSR with identical (element-coupling) patterns."""
    nq = p + 1 if nq is None else nq
    t, w = _gauss01(nq)
    phi, dphi = _lagrange01(p, t)
    me = (phi * w) @ phi.T
    ke = (dphi * w) @ dphi.T
    v = numpy.asarray(vertices, dtype=numpy.float64)
    h = numpy.diff(v)
    nel = len(h)
    n = nel * p + 1
    loc = numpy.arange(p + 1)
    rows = (numpy.arange(nel)[:, None, None] * p + loc[None, :, None]) + 0 * loc[None, None, :]
    cols = (numpy.arange(nel)[:, None, None] * p + loc[None, None, :]) + 0 * loc[None, :, None]
    mvals = me[None, :, :] * h[:, None, None]
    kvals = ke[None, :, :] / h[:, None, None]
    Mm = sp.coo_matrix((mvals.ravel(), (rows.ravel(), cols.ravel())), shape=(n, n)).tocsr()
    Km = sp.coo_matrix((kvals.ravel(), (rows.ravel(), cols.ravel())), shape=(n, n)).tocsr()
    # force one shared structural pattern (coo->csr summation keeps explicit zeros)
    Mm.sort_indices()
    Km.sort_indices()
    return Mm, Km


def fe_gradient_1d(vertices, p, nq=None):
    """G[a,b] = int phi_a' phi_b of the 1-D CG Lagrange degree-p basis (scipy CSR on the element-coupling pattern of
    ``fe_matrices_1d``, explicit zeros kept): the mixed first-derivative factor of vector-valued forms."""
    nq = p + 1 if nq is None else nq
    t, w = _gauss01(nq)
    phi, dphi = _lagrange01(p, t)
    ge = (dphi * w) @ phi.T                          # (the 1/h of the derivative and the h of dx cancel)
    nel = len(vertices) - 1
    n = nel * p + 1
    loc = numpy.arange(p + 1)
    rows = (numpy.arange(nel)[:, None, None] * p + loc[None, :, None]) + 0 * loc[None, None, :]
    cols = (numpy.arange(nel)[:, None, None] * p + loc[None, None, :]) + 0 * loc[None, :, None]
    G = sp.coo_matrix((numpy.tile(ge, (nel, 1, 1)).ravel(), (rows.ravel(), cols.ravel())), shape=(n, n)).tocsr()
    G.sort_indices()
    return G


def fe_matrices_1d_ext(vertices, p, nq=None):
    """(mass, stiffness, S2[a,b] = int phi_a'' phi_b'', C[a,b] = int phi_a'' phi_b) element by
    element (no inter-element terms, as dolfin assembles ``inner(lap(u),lap(v))*dx``), all on one
    shared pattern."""
    nq = p + 1 if nq is None else nq
    t, w = _gauss01(nq)
    phi, dphi = _lagrange01(p, t)
    # second derivatives of the equispaced Lagrange basis by differentiating the interpolant
    nodes = numpy.arange(p + 1) / float(p)
    V = numpy.vander(nodes, p + 1, increasing=True)          # monomial coefficients of each basis fn
    coef = numpy.linalg.solve(V, numpy.eye(p + 1))           # coef[:, a] = monomial coeffs of phi_a
    d2 = numpy.zeros((p + 1, len(t)))
    for a in range(p + 1):
        for m in range(2, p + 1):
            d2[a] += coef[m, a] * m * (m - 1) * t ** (m - 2)
    me = (phi * w) @ phi.T
    ke = (dphi * w) @ dphi.T
    s2e = (d2 * w) @ d2.T
    ce = (d2 * w) @ phi.T
    v = numpy.asarray(vertices, dtype=numpy.float64)
    h = numpy.diff(v)
    nel = len(h)
    n = nel * p + 1
    loc = numpy.arange(p + 1)
    rows = (numpy.arange(nel)[:, None, None] * p + loc[None, :, None]) + 0 * loc[None, None, :]
    cols = (numpy.arange(nel)[:, None, None] * p + loc[None, None, :]) + 0 * loc[None, :, None]

    def asm(e, scale):
        A = sp.coo_matrix(((e[None, :, :] * scale[:, None, None]).ravel(), (rows.ravel(), cols.ravel())),
                          shape=(n, n)).tocsr()
        A.sort_indices()
        return A
    return asm(me, h), asm(ke, 1.0 / h), asm(s2e, 1.0 / h ** 3), asm(ce, 1.0 / h)


def fe_load_1d(vertices, p, f, nq=None):
    nq = p + 1 if nq is None else nq
    t, w = _gauss01(nq)
    phi, _ = _lagrange01(p, t)
    v = numpy.asarray(vertices, dtype=numpy.float64)
    nel = len(v) - 1
    b = numpy.zeros(nel * p + 1)
    for e in range(nel):
        h = v[e + 1] - v[e]
        b[e * p:e * p + p + 1] += (phi * w) @ f(v[e] + h * t) * h
    return b


def _single_grid(V):
    if len(V.grids) != 1:
        raise NotImplementedError("synthetic forms are provided for single-field spaces")
    g = V.grids[0]
    if g.dg:
        raise NotImplementedError("synthetic forms are provided for CG spaces")
    return g


def _memo(obj, V, build):
    """1-D factors depend only on the space: build once per (form, V)"""
    cache = obj.__dict__.setdefault("_cache", {})
    # keyed on what the factors are computed from (id(V) can be recycled after garbage collection)
    key = tuple((g.degree, bool(g.dg), tuple(numpy.asarray(v, dtype=numpy.float64).tobytes() for v in g.vertices))
                if hasattr(g, "vertices") else id(g) for g in V.grids)
    if key not in cache:
        cache[key] = build()
    return cache[key]


def _plane_window(g, row0, row1):
    """node planes [za, zb) of the last direction that hold the FE rows [row0, row1), and the planes [fa, fb) of the
    elements that touch them (whose control values the assembly reads)"""
    shape = g.shape()
    plane = int(numpy.prod(shape[:-1], dtype=numpy.int64)) if len(shape) > 1 else 1
    n_last, p = shape[-1], int(g.degree)
    nel = (n_last - 1) // p
    za, zb = int(row0) // plane, -(-int(row1) // plane)
    if zb <= za:
        return plane, za, zb, za, za
    e0 = za // p - 1 if (za > 0 and za % p == 0) else za // p
    e0 = min(e0, nel - 1)
    e1 = min(nel, (zb - 1) // p + 1)
    return plane, za, zb, e0 * p, e1 * p + 1


def _control_window(geometry, plane, fa, fb):
    """(the nsd+1 control functions as DeviceVectors, index of their first node): the functions themselves when they
    are held in full, else their values on the node planes [fa, fb) -- a rank of a distributed run holds only the rows
    it owns, and its forms read a window around them (``AbstractExtractionGenerator.controlFunctionWindow``)"""
    cpf = geometry.cpFuncs
    if all(getattr(fn, "local_range", None) is None for fn in cpf):
        return [fn.vector() for fn in cpf], 0
    gen = getattr(geometry, "_generator", geometry)
    return gen.controlFunctionWindow(fa, fb), fa * plane


def _need_geometry(who, geometry, rational):
    if rational and geometry is None:
        raise ValueError("%s: rational=True divides by the weight function of a mapped patch (geometry=...)" % who)
    return bool(rational)


def _mapped(geometry, V, form, row0=None, row1=None, grid=None, block=None, nq=None, rational=False):
    """dolfin.assemble stand-in on a mapped patch: ``geometry`` is a generator / ExtractedSpline
    whose ``cpFuncs`` (nsd+1 homogeneous control functions on the FE nodes of ``V_control``) define
    F = cpFuncs[i]/cpFuncs[nsd] (tIGAr/common.py:917-921); metric-based measure and gradient.  ``row0, row1``: the FE
    rows of a block only (global columns), as the z-slab pipeline asks for them.  ``form`` "elasticity": ``block`` =
    (i, j, lambda, mu), ``grid`` the node grid the fields share.  ``rational``: trial and test functions phi / W_h, W_h
    the weight function ``cpFuncs[nsd]`` -- the reference's ``spline.rationalize(TrialFunction(V))``."""
    g = _single_grid(V) if grid is None else grid
    gc = _single_grid(geometry.V_control)
    if gc.shape() != g.shape():
        raise ValueError("the geometry lives on a different node grid than the space")
    verts = [g.vertices[k] for k in range(g.dim())]
    n = g.num_nodes()

    def assemble(cp, **rows):
        if form == "elasticity":
            if len(cp) - 1 != g.dim():
                raise ValueError("the elasticity form needs as many physical as parametric directions")
            return _dev.assemble_mapped_elasticity_block(verts, g.degree, cp, block[0], block[1], block[2], block[3],
                                                         rational=rational, **rows)
        return _dev.assemble_mapped_matrix(verts, g.degree, cp, form, nq=nq, rational=rational, **rows)

    row0, row1 = (0 if row0 is None else int(row0)), (n if row1 is None else int(row1))       # (either may be left out)
    if (row0, row1) == (0, n):
        cp, node0 = _control_window(geometry, 1, 0, g.shape()[-1])
        if node0 == 0 and all(v.size() == n for v in cp):
            return assemble(cp)
        row0, row1 = 0, n
    plane, za, zb, fa, fb = _plane_window(g, row0, row1)
    cp, node0 = _control_window(geometry, plane, fa, fb)
    A = assemble(cp, row0=za * plane, row1=zb * plane, cp_node0=node0)
    if (za * plane, zb * plane) != (int(row0), int(row1)):           # (a range that cuts through node planes)
        A = A.block(int(row0) - za * plane, int(row1) - za * plane, 0, n)
    return A


class LaplaceForm(object):
    """a(u,v) = int grad u . grad v: on the parametric box (Kronecker sum of 1-D factors), or --
    with ``geometry`` (a generator or ExtractedSpline) -- in physical space on the mapped patch,
    grad and dx as ``spline.grad`` / ``spline.dx`` (tIGAr/common.py:917-945).  ``rational`` (mapped patch only): trial
    and test functions divided by the weight function, ``spline.rationalize(TrialFunction(V))`` of the reference's NURBS
    demos (demos/poisson/poisson-nurbs.py:121-124); the unknown's nodal values are then those of the homogeneous
    function u_h = W_h u."""

    def __init__(self, geometry=None, rational=False):
        # a(u, v) = a(v, u) for THIS class; a subclass that adds terms says so itself (not inherited)
        self.symmetric = type(self) is LaplaceForm
        self.geometry = geometry
        self.rational = _need_geometry("LaplaceForm", geometry, rational)

    def factors(self, V):
        def build():
            g = _single_grid(V)
            mk = [fe_matrices_1d(g.vertices[k], g.degree) for k in range(g.dim())]
            d = g.dim()
            return [[mk[k][1] if k == dd else mk[k][0] for k in range(d)] for dd in range(d)]
        return _memo(self, V, build)

    def assemble_matrix(self, V, row0=None, row1=None):
        if self.geometry is not None:
            return _mapped(self.geometry, V, "laplace", row0, row1, rational=self.rational)
        return _dev.kron_sum_csr(self.factors(V), row0, row1)


class ElasticityForm(object):
    """a(u,v) = int lambda div u div v + 2 mu eps(u):eps(v) on the parametric box of a d-field space (all fields on one
    CG node grid, dofs field after field -- the space of ``EqualOrderSpline(d, ...)``):
    block (i, j) = lambda int d_i phi_a d_j phi_b + mu int d_j phi_a d_i phi_b + delta_ij mu int grad phi_a . grad phi_b,
    each a Kronecker sum of 1-D factors (mass M, stiffness K, G[a,b] = int phi_a' phi_b) on the element-coupling pattern,
    written block by block by the Kronecker-sum kernel and put together on the device.  What a dolfin user writes as
    ``inner(sigma(u), eps(v))*dx`` for ``demos``-style linear elasticity on an identity-geometry patch.

    With ``geometry`` (a generator or ExtractedSpline with nsd == d): in physical space on the mapped patch --
    ``inner(sigma(u), spline.sym(spline.grad(v)))*spline.dx`` with the Cartesian derivatives of ``spline.grad`` /
    ``spline.div`` (tIGAr/common.py:1022-1040, calculusUtils.py:255-276); each block from the element kernels of
    csrc/tg_assemble.hip (no Kronecker factors: the PtAP takes the assembled blocks).  ``rational``: every component
    function divided by the weight function (see LaplaceForm); the space then holds the rigid motions."""

    def __init__(self, lmbda=1.0, mu=1.0, geometry=None, rational=False):
        # a(u, v) = a(v, u) for THIS class; a subclass that adds terms says so itself (not inherited)
        self.symmetric = type(self) is ElasticityForm
        self.lmbda, self.mu = float(lmbda), float(mu)
        self.geometry = geometry
        self.rational = _need_geometry("ElasticityForm", geometry, rational)

    def _grid(self, V):
        g = V.grids[0]
        if g.dg or len(V.grids) != g.dim() or any(
                gi.degree != g.degree or any(not numpy.array_equal(a, b) for a, b in zip(gi.axes, g.axes)) for gi in V.grids):
            raise NotImplementedError("ElasticityForm: as many fields as parametric directions, all on one CG node grid")
        return g

    def block_factors(self, V):
        """factors[i][j] = list of terms, each a list of d 1-D matrices (direction 0 first); None on a mapped patch"""
        if self.geometry is not None:
            return None

        def build():
            g = self._grid(V)
            d = g.dim()
            one = [fe_matrices_1d(g.vertices[k], g.degree) + (fe_gradient_1d(g.vertices[k], g.degree),) for k in range(d)]
            Mk, Kk, Gk = [o[0] for o in one], [o[1] for o in one], [o[2] for o in one]
            lam, mu = self.lmbda, self.mu
            out = [[None] * d for _ in range(d)]
            for i in range(d):
                for j in range(d):
                    if i == j:
                        terms = []
                        for k in range(d):
                            c = (lam + 2.0 * mu) if k == i else mu
                            terms.append([(c * Kk[q]) if q == k else Mk[q] for q in range(d)])
                    else:
                        # int d_i phi_a d_j phi_b: G in direction i, G^T in direction j; and the transposed pairing
                        t1 = [(lam * Gk[q]) if q == i else (Gk[q].T.tocsr() if q == j else Mk[q]) for q in range(d)]
                        t2 = [(mu * Gk[q].T.tocsr()) if q == i else (Gk[q] if q == j else Mk[q]) for q in range(d)]
                        terms = [t1, t2]
                    out[i][j] = terms
            return out
        return _memo(self, V, build)

    def assemble_block(self, V, i, j, row0=None, row1=None):
        """rows [row0, row1) of block (i, j) (fields i, j; columns of one field)"""
        if self.geometry is not None:
            return _mapped(self.geometry, V, "elasticity", row0, row1, grid=self._grid(V), block=(i, j, self.lmbda, self.mu),
                           rational=self.rational)
        return _dev.kron_sum_csr(self.block_factors(V)[i][j], row0, row1)

    def assemble_matrix(self, V, row0=None, row1=None):
        if row0 is not None or row1 is not None:
            raise NotImplementedError("row blocks of the elasticity form: use assemble_block")
        if self.geometry is not None:
            d = self._grid(V).dim()
            return _dev.csr_from_blocks([[self.assemble_block(V, i, j) for j in range(d)] for i in range(d)])
        fac = self.block_factors(V)
        d = len(fac)
        return _dev.csr_from_blocks([[_dev.kron_sum_csr(fac[i][j]) for j in range(d)] for i in range(d)])


class MassForm(object):
    """a(u,v) = int u v (``geometry``: see LaplaceForm; ``nq``: Gauss points per direction on the mapped patch, p + 1
    when None; ``rational``: see LaplaceForm)."""

    def __init__(self, geometry=None, nq=None, rational=False):
        # a(u, v) = a(v, u) for THIS class; a subclass that adds terms says so itself (not inherited)
        self.symmetric = type(self) is MassForm
        self.geometry = geometry
        self.rational = _need_geometry("MassForm", geometry, rational)
        if nq is not None and geometry is None:
            raise ValueError("MassForm: nq belongs to a mapped patch (geometry=...)")
        self.nq = nq

    def factors(self, V):
        g = _single_grid(V)
        return [[fe_matrices_1d(g.vertices[k], g.degree)[0] for k in range(g.dim())]]

    def assemble_matrix(self, V, row0=None, row1=None):
        if self.geometry is not None:
            return _mapped(self.geometry, V, "mass", row0, row1, nq=self.nq, rational=self.rational)
        return _dev.kron_sum_csr(self.factors(V), row0, row1)


class NodalLoadForm(object):
    """L(v) = int f_h v dx on the mapped patch, f_h = nodal interpolant of ``f``: a callable evaluated at the
    physical node positions x = F(node) (array of shape [nnodes, nsd] -> values), a number (constant load), or the node
    values themselves (array / DeviceVector on all FE nodes).  ``rational``: v the test functions phi / W_h (f_h stays
    the interpolant of the node values)."""

    def __init__(self, f, geometry, rational=False):
        self.f, self.geometry = f, geometry
        self.rational = _need_geometry("NodalLoadForm", geometry, rational)

    def _nodal_values(self, cp, node0, n_nodes):
        """f on the nodes [node0, node0 + n_nodes) that the control functions ``cp`` are given on"""
        if callable(self.f):
            # f at the physical node positions x = F(node): evaluated on the host (f is the user's Python function), once per
            # window of control functions -- the sub-slabs of one assembly and the assemblies of a Newton iteration ask for the
            # same windows again (keyed on the vectors' identity: a new geometry means new control functions)
            key = (tuple(id(v) for v in cp), int(node0), int(n_nodes))
            cache = self.__dict__.setdefault("_fnodal", {})
            if key not in cache:
                if len(cache) > 64:
                    cache.clear()
                c = [v.get_local() for v in cp]
                x = numpy.stack([c[i] / c[-1] for i in range(len(c) - 1)], axis=1)
                cache[key] = (_dev.DeviceVector(data=numpy.asarray(self.f(x), dtype=numpy.float64)), cp)   # (cp kept alive: ids)
            return cache[key][0]
        if numpy.isscalar(self.f):
            fn = _dev.DeviceVector(n_nodes, zero=False)
            fn.fill(float(self.f))
            return fn
        full = self.f if isinstance(self.f, _dev.DeviceVector) else _dev.DeviceVector(data=self.f)
        if node0 == 0 and full.size() == n_nodes:
            return full
        piece = _dev.DeviceVector(n_nodes, zero=False)
        _dev.vec_copy_range(piece, 0, full, node0, n_nodes)
        return piece

    def assemble_vector(self, V, row0=None, row1=None):
        g = _single_grid(V)
        verts = [g.vertices[k] for k in range(g.dim())]
        n = g.num_nodes()
        row0, row1 = (0 if row0 is None else int(row0)), (n if row1 is None else int(row1))   # (either may be left out)
        if (row0, row1) == (0, n):
            cp, node0 = _control_window(self.geometry, 1, 0, g.shape()[-1])
            if node0 == 0 and all(v.size() == n for v in cp):
                return _dev.assemble_mapped_load(verts, g.degree, cp, self._nodal_values(cp, 0, n), rational=self.rational)
            row0, row1 = 0, n
        plane, za, zb, fa, fb = _plane_window(g, row0, row1)
        cp, node0 = _control_window(self.geometry, plane, fa, fb)
        if node0 == 0 and cp[0].size() == n:
            fn = self._nodal_values(cp, 0, n)
        else:
            fn = self._nodal_values(cp, node0, cp[0].size())
        b = _dev.assemble_mapped_load(verts, g.degree, cp, fn, row0=za * plane, row1=zb * plane, cp_node0=node0,
                                      rational=self.rational)
        if (za * plane, zb * plane) != (int(row0), int(row1)):
            piece = _dev.DeviceVector(int(row1) - int(row0), zero=False)
            _dev.vec_copy_range(piece, 0, b, int(row0) - za * plane, int(row1) - int(row0))
            b = piece
        return b


def _whole_patch(geometry, g, who, operands="quadrature-point operands"):
    """(element vertices, degree, control functions) of a patch with the node grid ``g`` whose control functions this rank
    holds in full"""
    if _single_grid(geometry.V_control).shape() != g.shape():
        raise ValueError("the geometry lives on a different node grid than the space")
    cp, node0 = _control_window(geometry, 1, 0, g.shape()[-1])
    if node0 != 0 or any(v.size() != g.num_nodes() for v in cp):
        raise NotImplementedError("%s: the control functions are spread over several ranks; %s are provided on one rank"
                                  % (who, operands))
    return [g.vertices[k] for k in range(g.dim())], int(g.degree), cp


def _per_points(obj, slot, pts, build):
    """``build()``: the point data of a callable, computed once per ``QuadraturePoints`` object and kept on ``obj`` under
    ``slot``, one set of points at a time (``pts`` is kept alive next to the value: its id is the key)"""
    cache = obj.__dict__.setdefault(slot, {})
    if id(pts) not in cache:
        cache.clear()
        cache[id(pts)] = (build(), pts)
    return cache[id(pts)][0]


def _check_nq(nq, p):
    nq = p + 1 if nq is None else nq
    most = _dev.assemble_limits()[1]
    if int(nq) != nq or not 1 <= int(nq) <= most:
        raise ValueError("nq = %r: 1..%d Gauss points per direction" % (nq, most))
    return int(nq)


# ---- the point-data reader: what a caller gives at the points -> one device array, point index last -------------------------
def _same_bits(a, b):
    a, b = numpy.ascontiguousarray(a, dtype=numpy.float64), numpy.ascontiguousarray(b, dtype=numpy.float64)
    return a.shape == b.shape and bool(numpy.array_equal(a.view(numpy.int64), b.view(numpy.int64)))


def point_array(v, npts, shape, who="point data"):
    """``v`` as a float64 array ``[npts] + shape``: one block of the component ``shape`` serves every point; anything else
    but ``[npts] + shape`` is a ValueError naming the given and the expected shape.  Host only."""
    v, shape = numpy.asarray(v, dtype=numpy.float64), tuple(int(s) for s in shape)
    if shape and v.shape == shape:
        v = numpy.broadcast_to(v, (npts,) + shape)
    if v.shape != (npts,) + shape:
        raise ValueError("%s: an array of shape %s for %d points; expected %s%s"
                         % (who, v.shape, npts, (npts,) + shape, " or %s" % (shape,) if shape else ""))
    return v


def point_block(v, npts, shape, perm=None, swap=None, who="point data"):
    """The host half of the reader: ``v`` (``point_array``) as the contiguous 1-D array of the device layout -- the
    component axes in the order ``perm`` (a permutation of range(len(shape)); None: as given), the point index last and
    fastest.  With ``swap`` (a permutation of the component axes) returns ``(array, symmetric)``: whether ``v`` equals, BIT
    FOR BIT, itself with the component axes so permuted (-0.0 differs from 0.0, a NaN equals itself)."""
    v = point_array(v, npts, shape, who)
    order = range(len(shape)) if perm is None else perm
    flat = numpy.ascontiguousarray(v.transpose(tuple(1 + a for a in order) + (0,))).ravel()
    if swap is None:
        return flat
    return flat, _same_bits(v, v.transpose((0,) + tuple(1 + a for a in swap)))


def point_unblock(flat, npts, shape):
    """the reverse of ``point_block`` without ``perm``: device layout (point index last) -> ``[npts] + shape``"""
    k = len(shape)
    return numpy.ascontiguousarray(numpy.asarray(flat).reshape(tuple(shape) + (npts,)).transpose((k,) + tuple(range(k))))


def _on_points(f, pts):
    """what ``f`` gives at the points: a callable is called on ``x [npts, nsd]``, on a face with ``(x, n)`` when it takes two"""
    if not callable(f):
        return f
    return f(pts.x, pts.n) if hasattr(pts, "normals") and _argcount(f) >= 2 else f(pts.x)


def _point_data(f, pts, shape, who, perm=None, swap=None, hint=None, pre=None):
    """The device half of the reader: the DeviceVector of ``f`` in the layout of ``point_block`` (with ``swap``:
    ``(DeviceVector, symmetric)``).  A DeviceVector is taken as it is after a length check, its symmetry is ``hint`` when
    one is set and is read from its bits otherwise; anything else (a callable of the points, an array, one block) goes
    through ``point_block`` (after ``pre``, where a form reshapes what it was given) and one upload."""
    if not isinstance(f, _dev.DeviceVector):
        v = numpy.asarray(_on_points(f, pts), dtype=numpy.float64)
        out = point_block(v if pre is None else pre(v), pts.npts, shape, perm, swap, who)
        return _dev.DeviceVector(data=out) if swap is None else (_dev.DeviceVector(data=out[0]), out[1])
    each = int(numpy.prod(shape, dtype=numpy.int64))
    if f.size() != each * pts.npts:
        raise ValueError("%s: %d values given, expected %d per point at %d points = %d"
                         % (who, f.size(), each, pts.npts, each * pts.npts))
    if swap is None:
        return f
    if hint is not None:
        return f, bool(hint)
    order = list(range(len(shape)) if perm is None else perm)
    h = f.get_local().reshape(tuple(shape[a] for a in order) + (pts.npts,))
    return f, _same_bits(h, h.transpose(tuple(order.index(swap[a]) for a in order) + (len(order),)))


class QuadraturePoints(object):
    """The Gauss points of a mapped patch, element-major (elements and the nq^d points of an element lexicographic with
    direction 0 fastest): ``x`` host array [npts, nsd] (downloaded on first use), ``x_device`` (nsd * npts values,
    component-major), ``weights`` = w_q sqrt(det g) prod h_k as a DeviceVector, ``nq``, ``npts``, ``nsd``."""

    def __init__(self, verts, p, cp, nq):
        self.verts, self.p, self.cp, self.nq, self.nsd = verts, p, cp, nq, len(cp) - 1
        self.x_device, self.weights = _dev.quad_points(verts, p, cp, nq)
        self.npts = self.weights.size()
        self._x = self._metric = None

    @property
    def x(self):
        if self._x is None:
            self._x = point_unblock(self.x_device.get_local(), self.npts, (self.nsd,))
        return self._x

    @property
    def metric(self):
        """the element metric G = 4 P P^T, P = DF g^-1, as a DeviceVector of nsd^2 npts values, G_KL at (K nsd + L) npts + q
        (``tg_quad_metric``): d xi / d x of the bi-unit parent element contracted over the parametric index; computed on
        first use and kept like ``weights``"""
        if self._metric is None:
            self._metric = _dev.quad_metric(self.verts, self.p, self.cp, self.nq)
        return self._metric

    def values(self, f, who="f"):
        """point values of ``f`` as a DeviceVector: a callable on ``x`` [npts, nsd] -> [npts], a number, the values
        themselves (array / DeviceVector), or a Function of the space (evaluated by ``tg_quad_eval``)"""
        if hasattr(f, "vector") and hasattr(f, "function_space"):
            return _dev.quad_eval(self.verts, self.p, self.cp, f.vector(), nq=self.nq)
        if isinstance(f, _dev.DeviceVector):
            if f.size() != self.npts:
                raise ValueError("%s: %d point values given, the patch has %d quadrature points" % (who, f.size(), self.npts))
            return f
        if callable(f):
            v = numpy.asarray(f(self.x), dtype=numpy.float64)
            if v.shape != (self.npts,):
                raise ValueError("%s: the callable returned an array of shape %s for %d points; expected (%d,)"
                                 % (who, v.shape, self.npts, self.npts))
            return _dev.DeviceVector(data=v)
        if numpy.ndim(f) == 0:
            v = _dev.DeviceVector(self.npts, zero=False)
            v.fill(float(f))
            return v
        v = numpy.asarray(f, dtype=numpy.float64)
        if v.shape != (self.npts,):
            raise ValueError("%s: an array of shape %s given, the patch has %d quadrature points" % (who, v.shape, self.npts))
        return _dev.DeviceVector(data=v)

    def vector_values(self, f, who="f"):
        """point values of a vector field (nsd * npts, component-major): a callable ``x -> [npts, nsd]``, an array
        [npts, nsd], a sequence of nsd numbers, or a DeviceVector already in that layout"""
        return _point_data(f, self, (self.nsd,), who)


def quadrature_points(geometry, V, nq=None, who="quadrature points"):
    """the ``QuadraturePoints`` of the patch of ``geometry`` (a generator or ExtractedSpline), kept on it per nq and per
    set of control-function vectors: new vectors give new points, values overwritten in place are not noticed"""
    verts, p, cp = _whole_patch(geometry, _single_grid(V), who)
    nq = _check_nq(nq, p)
    cache = geometry.__dict__.setdefault("_quad_points", {})
    key = (nq, tuple(id(v) for v in cp))
    if key not in cache:
        cache[key] = QuadraturePoints(verts, p, cp, nq)
    return cache[key]


def lattice_abscissae(m, p):
    """the abscissae of a sampling lattice: ``m`` None: p + 1 equispaced with the ends; an int: that many equispaced with the
    ends (1: the element centre); a sequence: the abscissae themselves, increasing within [0, 1]"""
    most = _dev.assemble_limits()[1]
    m = p + 1 if m is None else m
    if numpy.ndim(m) == 0:
        if int(m) != m or not 1 <= int(m) <= most:
            raise ValueError("m = %r: 1..%d lattice points per element and direction" % (m, most))
        return numpy.array([0.5]) if int(m) == 1 else numpy.linspace(0.0, 1.0, int(m))
    t = numpy.asarray(m, dtype=numpy.float64)
    if t.ndim != 1 or not 1 <= t.size <= most:
        raise ValueError("lattice abscissae of shape %s: a sequence of 1..%d numbers" % (t.shape, most))
    if not (numpy.all(t >= 0.0) and numpy.all(t <= 1.0)) or numpy.any(numpy.diff(t) <= 0.0):
        raise ValueError("lattice abscissae %r: increasing numbers within [0, 1]" % (t.tolist(),))
    return numpy.ascontiguousarray(t)


class LatticePoints(object):
    """The tensor lattice of ``m`` abscissae ``t`` per element and direction on a mapped patch, numbered as the Gauss points
    (element-major, direction 0 fastest; with the ends among the abscissae the points on shared element faces come once per
    element): ``x`` host array [npts, nsd] (downloaded on first use), ``x_device`` (nsd * npts, component-major), ``t``,
    ``m``, ``npts``, ``nsd``, ``values(f)`` as on ``QuadraturePoints`` and ``cells()`` for a viewer."""

    def __init__(self, verts, p, cp, t):
        self.verts, self.p, self.cp, self.t, self.m, self.nsd = verts, p, cp, t, len(t), len(cp) - 1
        self.x_device = _dev.lattice_points(verts, p, cp, t)
        self.npts = _dev.quad_count(verts, self.m)
        self._x = None

    @property
    def x(self):
        if self._x is None:
            self._x = point_unblock(self.x_device.get_local(), self.npts, (self.nsd,))
        return self._x

    def values(self, f, who="f"):
        """point values of ``f`` as a DeviceVector: as ``QuadraturePoints.values``, a Function of the space evaluated by
        ``tg_lattice_eval``"""
        if hasattr(f, "vector") and hasattr(f, "function_space"):
            return _dev.lattice_eval(self.verts, self.p, self.cp, self.t, f.vector())
        return QuadraturePoints.values(self, f, who)

    def cells(self):
        """((m - 1)^d nelem linear cells [ncells, 2^d] in VTK's vertex order, the VTK cell type): ``vtkio.lattice_cells``"""
        from . import vtkio
        d = len(self.verts)
        return vtkio.lattice_cells([len(v) - 1 for v in self.verts], self.m, d), vtkio.CELL_TYPE_OF_DIM[d]


def lattice_points(geometry, g, m=None, who="lattice points"):
    """the ``LatticePoints`` of the patch of ``geometry`` with the node grid ``g``, kept on it per set of abscissae and of
    control-function vectors, like the quadrature points"""
    verts, p, cp = _whole_patch(geometry, g, who, "the sampling operands")
    t = lattice_abscissae(m, p)
    cache = geometry.__dict__.setdefault("_lattice_points", {})
    key = (t.tobytes(), tuple(id(v) for v in cp))
    if key not in cache:
        cache[key] = LatticePoints(verts, p, cp, t)
    return cache[key]


class LocatedPoints(object):
    """What ``ExtractedSpline.locatePoints`` found: ``xi`` host array [npts, d] (lazy) and ``xi_device`` (d * npts,
    component-major) inside the parametric box, ``distance`` |x - F(xi)|, ``iterations``, ``status`` (0 converged, 1
    iteration limit, 2 input not finite, 3 singular DF^T DF) as host arrays, ``converged`` = all status 0, ``npts``."""

    def __init__(self, xi_device, info, d):
        self.xi_device, self.d = xi_device, d
        self.npts = xi_device.size() // d
        h = info.get_local().reshape(3, self.npts)
        self.distance, self.iterations, self.status = h[0].copy(), h[1].astype(numpy.int64), h[2].astype(numpy.int64)
        self._xi = None

    @property
    def xi(self):
        if self._xi is None:
            self._xi = point_unblock(self.xi_device.get_local(), self.npts, (self.d,))
        return self._xi

    @property
    def converged(self):
        return bool(numpy.all(self.status == 0))


class QuadratureLoadForm(object):
    """L(v) = sum_q wdet_q f(x_q) v(xi_q) on the mapped patch: the load of ``f`` itself, not of its nodal interpolant
    (``NodalLoadForm``).  ``f``: a callable on the physical points ``[npts, nsd] -> [npts]`` (evaluated on the host once
    per geometry), a number, the ``npts`` point values (array / DeviceVector, numbered as ``QuadraturePoints``), or a
    ``Function`` on the space.  ``nq`` Gauss points per direction (p + 1 when None).  ``rational``: v the test functions
    phi / W_h; a ``Function`` given as ``f`` is still read un-rationalised -- hand in
    ``spline.evaluateAtQuadrature(f, rational=True)`` for its rational values.  ``flux``: adds int F . grad v dx with the
    Cartesian gradient (``tg_quad_load_flux``); ``F`` a callable ``x -> [npts, nsd]``, an array of that shape, nsd numbers
    or a DeviceVector of nsd * npts values, component-major; ``f`` may then be None."""

    def __init__(self, f, geometry, nq=None, rational=False, flux=None):
        self.f, self.geometry, self.nq, self.flux = f, geometry, nq, flux
        self.rational = _need_geometry("QuadratureLoadForm", geometry, rational)
        if flux is not None and geometry is None:
            raise ValueError("QuadratureLoadForm: the flux term is integrated on a mapped patch (geometry=...)")

    def point_values(self, V):
        pts = quadrature_points(self.geometry, V, self.nq, "QuadratureLoadForm")
        if callable(self.f) and not hasattr(self.f, "vector"):
            return pts, _per_points(self, "_fq", pts, lambda: pts.values(self.f, "QuadratureLoadForm"))
        return pts, pts.values(self.f, "QuadratureLoadForm")

    def assemble_vector(self, V, row0=None, row1=None):
        if self.flux is not None:
            _point_scope(self.geometry, V, "QuadratureLoadForm", "scalar")
        _whole_rows(_single_grid(V).num_nodes(), row0, row1, "QuadratureLoadForm", "patch")
        if self.flux is None:
            pts, fq = self.point_values(V)
            return _dev.quad_load(pts.verts, pts.p, pts.cp, fq, nq=pts.nq, rational=self.rational)
        pts, fq = self.point_values(V) if self.f is not None else \
            (quadrature_points(self.geometry, V, self.nq, "QuadratureLoadForm"), None)
        if callable(self.flux):
            Fq = _per_points(self, "_Fq", pts, lambda: pts.vector_values(self.flux, "QuadratureLoadForm: flux"))
        else:
            Fq = pts.vector_values(self.flux, "QuadratureLoadForm: flux")
        return _dev.quad_load_flux(pts.verts, pts.p, pts.cp, fq, Fq, nq=pts.nq, rational=self.rational)


class SeparableLoadForm(object):
    """L(v) = int f v with f = scale * prod_k f1d[k](x_k)."""

    def __init__(self, f1d, scale=1.0):
        self.f1d, self.scale = list(f1d), float(scale)

    def vectors_1d(self, V):
        def build():
            g = _single_grid(V)
            return [fe_load_1d(g.vertices[k], g.degree, self.f1d[k]) for k in range(g.dim())]
        return _memo(self, V, build)

    def assemble_vector(self, V, row0=None, row1=None):
        return _dev.vec_tensor3(self.vectors_1d(V), self.scale, row0, row1)


class BiharmonicForm(object):
    """a(u,v) = int (lap u)(lap v), element-wise (demos/biharmonic/biharmonic.py:100-103), 2-D:
    S2xM + MxS2 + C^T x C + C x C^T with C[a,b] = int phi_a'' phi_b.  With ``geometry`` (nsd == d, 2-D or 3-D): on the
    mapped patch, lap = spline.div(spline.grad(.)) with the second derivatives of the (rational) map
    (tIGAr/common.py:1022-1040; csrc/tg_assemble.hip, plain element kernel)."""

    def __init__(self, geometry=None):
        # a(u, v) = a(v, u) for THIS class; a subclass that adds terms says so itself (not inherited)
        self.symmetric = type(self) is BiharmonicForm
        self.geometry = geometry

    def factors(self, V):
        g = _single_grid(V)
        if g.dim() != 2:
            raise NotImplementedError("BiharmonicForm is provided for 2-D patches")
        (Mx, _, S2x, Cx), (My, _, S2y, Cy) = [fe_matrices_1d_ext(g.vertices[k], g.degree) for k in range(2)]
        return [[S2x, My], [Mx, S2y], [Cx.T.tocsr(), Cy], [Cx, Cy.T.tocsr()]]

    def assemble_matrix(self, V, row0=None, row1=None):
        if self.geometry is not None:
            return _mapped(self.geometry, V, "biharmonic", row0, row1)
        return _dev.kron_sum_csr(self.factors(V), row0, row1)


class SumOfSeparableLoads(object):
    """L(v) = int f v with f = sum_t scale_t * prod_k f1d_t[k](x_k)."""

    def __init__(self, terms):
        self.terms = [SeparableLoadForm(f1d, scale) for f1d, scale in terms]

    def assemble_vector(self, V, row0=None, row1=None):
        out = None
        for t in self.terms:
            v = t.assemble_vector(V, row0, row1)
            if out is None:
                out = v
            else:
                out.axpy(1.0, v)
        return out


class Equation(object):
    """``lhs == rhs`` stand-in for ufl.equation.Equation (tIGAr/common.py:1277-1283)."""

    def __init__(self, lhs, rhs):
        self.lhs, self.rhs = lhs, rhs


class SemilinearResidual(object):
    """Residual of  -lap u + g(u) = f  in group-FE (product approximation) form on the scalar Q_p
    space:  R_a = sum_b K_ab u_b + sum_b M_ab (g(u_b) - f_b), with K, M the stiffness and mass
    matrices (identity geometry, or mapped with ``geometry``), ``u`` the current FE ``Function`` (read
    at assembly time, as a UFL form reads its coefficient), ``g`` / ``dg`` callables mapping a
    ``DeviceVector`` of nodal values to one (``lambda v: v.pointwise_mult(v).pointwise_mult(v)``).
    ``tangent()`` gives the matching Jacobian form  J = K + M diag(g'(u)).  K and M are assembled
    once and reused by every Newton step (fixed sparsity)."""

    def __init__(self, u, f_nodal, g, dg, geometry=None):
        self.u, self.g, self.dg, self.geometry = u, g, dg, geometry
        self.f = f_nodal if isinstance(f_nodal, _dev.DeviceVector) else _dev.DeviceVector(data=f_nodal)
        self._KM = None

    def _matrices(self, V):
        if self._KM is None:
            self._KM = (LaplaceForm(self.geometry).assemble_matrix(V), MassForm(self.geometry).assemble_matrix(V))
        return self._KM

    def _row_blocks(self, V, row0, row1):
        """rows [row0, row1) of K and M (cut once per row range: a Newton loop asks for the same blocks every step)"""
        key = (int(row0), int(row1))
        if getattr(self, "_blocks", None) is None or self._blocks[0] != key:
            K, Mm = self._matrices(V)
            n = K.shape[1]
            self._blocks = (key, K.block(key[0], key[1], 0, n), Mm.block(key[0], key[1], 0, n))
        return self._blocks[1], self._blocks[2]

    def assemble_vector(self, V, row0=None, row1=None):
        K, Mm = self._matrices(V)
        # (a rank-local u: its ghosted form -- own rows + the rows of the z-neighbours this rank's rows couple to)
        uv = self.u.ghosted() if hasattr(self.u, "ghosted") else self.u.vector()
        if row0 is not None and (row0, row1) != (0, K.shape[0]):
            K, Mm = self._row_blocks(V, row0, row1)
        r = K.mult(uv)
        t = self.g(uv)
        t.axpy(-1.0, self.f)
        r.axpy(1.0, Mm.mult(t))
        return r

    def tangent(self):
        return _SemilinearTangent(self)


class _SemilinearTangent(object):
    def __init__(self, res):
        self.res = res

    def assemble_matrix(self, V, row0=None, row1=None):
        K, Mm = self.res._matrices(V)
        uv = self.res.u.ghosted() if hasattr(self.res.u, "ghosted") else self.res.u.vector()
        if row0 is not None and (row0, row1) != (0, K.shape[0]):
            K, Mm = self.res._row_blocks(V, row0, row1)
        return K.combine(1.0, Mm, 1.0, self.res.dg(uv))


# ---- volume forms with point coefficients (csrc/tg_coef.hip) ---------------------------------------------------------------
_SCOPE_OF_KIND = {"scalar": "_quadrature_scope", "vector": "_vector_quadrature_scope", "jet": "_jet_scope",
                  "system": "_system_quadrature_scope"}


def _point_scope(geometry, V, who, kind):
    """What a point form of ``kind`` works on, or the refusal with its reason.  An ExtractedSpline says itself what its
    point operands serve (one rank, the order of the node grid, ...: ``_point_scope`` there), the generator whether its
    fields lie on the control mesh's scalar basis.
      "scalar": one scalar field; returns None.
      "vector": a displacement, nF = nsd = d fields (d = 2 plane strain, or 3) on one continuous Q_p node grid, dofs field
                after field (``EqualOrderSpline(d, mesh)``); returns (node grid, nF).
      "jet":    nF >= 1 fields on one such grid of a patch with d = 1, 2 and nsd >= d; returns (node grid, nF, nJ).
      "system": nF >= 1 fields on one such grid of a patch with d = 1, 2, 3 and nsd >= d, nF independent of nsd
                (``EqualOrderSpline(nF, mesh)``); returns (node grid, nF)."""
    if geometry is None:
        raise ValueError("%s: point data live on a mapped patch (geometry=...)" % who)
    scope = getattr(geometry, _SCOPE_OF_KIND[kind], None)
    if scope is not None:
        scope(who)
    _fields_of_the_patch(geometry, who)
    if kind == "scalar":
        return None
    g = _one_shared_grid(V, who)
    nF, nsd, d = len(V.grids), len(geometry.cpFuncs) - 1, g.dim()
    if kind == "jet":
        if d not in (1, 2):
            raise NotImplementedError("%s: d = %d parametric directions; second-derivative point forms are provided for "
                                      "curves and surfaces (d = 1, 2)" % (who, d))
        if nsd < d:
            raise NotImplementedError("%s: nsd = %d physical directions on a patch of d = %d parametric ones" % (who, nsd, d))
        return g, nF, _dev.jet_size(d)
    if kind == "system":
        if nsd < d:
            raise NotImplementedError("%s: nsd = %d physical directions on a patch of d = %d parametric ones" % (who, nsd, d))
        return g, nF
    if nsd != d or d not in (2, 3):
        raise NotImplementedError("%s: nsd = %d physical directions on a patch of d = %d parametric ones; a solid has "
                                  "nsd = d = 2 (plane strain) or 3" % (who, nsd, d))
    if nF != nsd:
        raise NotImplementedError("%s: nFields = %d; the displacement has nsd = %d fields" % (who, nF, nsd))
    return g, nF


def _tensor_values(pts, A, who):
    """(kind, DeviceVector, symmetric) of a diffusion given at the points: kind 1 = one value per point, 2 = an nsd x nsd
    tensor per point (component (i, j) of point q at (i nsd + j) npts + q)"""
    if isinstance(A, _dev.DeviceVector):
        if A.size() == pts.npts:
            return 1, A, True
    elif hasattr(A, "vector") and hasattr(A, "function_space") or numpy.ndim(A) == 0 and not callable(A):
        return 1, pts.values(A, who), True
    else:
        A = numpy.asarray(_on_points(A, pts), dtype=numpy.float64)
        if A.shape == (pts.npts,):
            return 1, _dev.DeviceVector(data=A), True
    return (2,) + _point_data(A, pts, (pts.nsd, pts.nsd), who, swap=(1, 0))


class CoefficientForm(object):
    """a(u, v) = int grad v . (A grad u) + (b . grad v) u + v (c . grad u) + m u v dx on the mapped patch, with coefficients
    given AT THE QUADRATURE POINTS: ``diffusion`` A, ``flux_velocity`` b, ``velocity`` c, ``reaction`` m (u the trial
    function = column, v the test function = row; grad and dx as ``spline.grad`` / ``spline.dx``).  What a user of the
    reference writes as ``kappa*inner(spline.grad(u), spline.grad(v))*spline.dx``, an advection-diffusion-reaction operator,
    or the Newton tangent of a scalar quasilinear equation (``QuasilinearResidual``).

    Every coefficient: a number, a callable of the points ``x [npts, nsd]``, or point values (array / DeviceVector,
    numbered as ``QuadraturePoints``); the scalar ones (an isotropic ``diffusion``, ``reaction``) also a ``Function`` of the
    space, read at assembly time.  ``diffusion`` may be ``[npts, nsd, nsd]`` (or a callable returning that, or one nsd x nsd
    matrix): a full tensor per point, which need not be symmetric.  Vectors: ``[npts, nsd]``, nsd numbers, or a
    DeviceVector of nsd * npts values, component-major.  ``nq`` Gauss points per direction (p + 1 when None).
    ``rational``: trial and test functions phi / W_h.

    ``symmetric`` is True only when the inputs prove it: A isotropic or bitwise equal to its transpose, and b and c both
    absent or bitwise equal.  The matrix lies on the element-coupling pattern with its certificate, as every mapped form's:
    the PtAP routes, plan caches and solvers serve it unchanged.  One rank, all rows (``tg_coef_transform``,
    ``tg_assemble_coef_matrix``)."""

    def __init__(self, geometry, diffusion=None, flux_velocity=None, velocity=None, reaction=None, nq=None, rational=False):
        if geometry is None:
            raise ValueError("CoefficientForm: point coefficients live on a mapped patch (geometry=...)")
        self.geometry, self.nq, self.rational = geometry, nq, bool(rational)
        self.diffusion, self.flux_velocity, self.velocity, self.reaction = diffusion, flux_velocity, velocity, reaction

    @staticmethod
    def _is_function(f):
        return hasattr(f, "vector") and hasattr(f, "function_space")

    def coefficients(self, V):
        """(points, kind of A, A, b, c, m, symmetric) with the point data as DeviceVectors (None = absent).  What does not
        depend on a Function is computed once per set of points."""
        who = "CoefficientForm"
        _point_scope(self.geometry, V, who, "scalar")
        pts = quadrature_points(self.geometry, V, self.nq, who)

        def static():
            kind, A, symA = 0, None, True
            if self.diffusion is not None and not self._is_function(self.diffusion):
                kind, A, symA = _tensor_values(pts, self.diffusion, who + ": diffusion")
            b = pts.vector_values(self.flux_velocity, who + ": flux_velocity") if self.flux_velocity is not None else None
            c = pts.vector_values(self.velocity, who + ": velocity") if self.velocity is not None else None
            m = None
            if self.reaction is not None and not self._is_function(self.reaction):
                m = pts.values(self.reaction, who + ": reaction")
            symbc = (b is None and c is None) or (b is not None and c is not None and
                                                   (b is c or _same_bits(b.get_local(), c.get_local())))
            return kind, A, b, c, m, bool(symA and symbc)
        kind, A, b, c, m, sym = _per_points(self, "_static", pts, static)
        if self._is_function(self.diffusion):
            kind, A = 1, pts.values(self.diffusion, who + ": diffusion")
        if self._is_function(self.reaction):
            m = pts.values(self.reaction, who + ": reaction")
        return pts, kind, A, b, c, m, sym

    @property
    def symmetric(self):
        return self.coefficients(self.geometry.V_control)[6]

    def assemble_matrix(self, V, row0=None, row1=None):
        _point_scope(self.geometry, V, "CoefficientForm", "scalar")
        _whole_rows(_single_grid(V).num_nodes(), row0, row1, "CoefficientForm", "patch")
        pts, kind, A, b, c, m, _ = self.coefficients(V)
        coef = _dev.coef_transform(pts.verts, pts.p, pts.cp, A, b, c, m, a_kind=kind, nq=pts.nq, rational=self.rational)
        return _dev.assemble_coef_matrix(pts.verts, pts.p, pts.cp, coef, nq=pts.nq)


class QuasilinearResidual(object):
    """Residual of a scalar quasilinear equation  -div flux(x, u, grad u) + source(x, u, grad u) = f  in weak form,
    R(v) = int flux . grad v + source v - f v dx, with the nonlinearity evaluated AT THE QUADRATURE POINTS (what
    ``derivative(residual, u)`` of the reference works on; ``SemilinearResidual`` is the group-FE product approximation).

    ``residual(x, u_q, grad_q) -> (flux [npts, nsd] | None, source [npts] | None)`` and
    ``tangent(x, u_q, grad_q) -> (A, b, c, m)`` = (d flux / d grad u [npts, nsd, nsd] or [npts], d flux / d u [npts, nsd],
    d source / d grad u [npts, nsd], d source / d u [npts]), any of them None, are host callables of the points
    ``x [npts, nsd]`` and of ``u`` and its Cartesian gradient there.  ``u``: the current FE ``Function``, read at assembly
    time through the kernel of ``evaluateAtQuadrature(u, grad=True, rational=...)``.  ``f``: as for
    ``QuadratureLoadForm``.  ``assemble_vector`` is the flux load minus the load of ``f``; ``tangent()`` the form whose
    ``assemble_matrix`` is the ``CoefficientForm`` of the tangent data.  Runs under ``solveNonlinearVariationalProblem``
    and inside ``Sum`` with the boundary forms.  ``rational``: u = u_h / W_h, tested against phi / W_h."""

    def __init__(self, u, geometry, residual, tangent, f=None, nq=None, rational=False):
        if geometry is None:
            raise ValueError("QuasilinearResidual: point coefficients live on a mapped patch (geometry=...)")
        self.u, self.geometry, self.residual, self._tangent = u, geometry, residual, tangent
        self.f, self.nq, self.rational = f, nq, bool(rational)
        self._load = QuadratureLoadForm(f, geometry, nq, rational=rational) if f is not None else None

    def state(self, V):
        """(points, u at the points [npts], its Cartesian gradient [npts, nsd]) on the host"""
        who = "QuasilinearResidual"
        _point_scope(self.geometry, V, who, "scalar")
        pts = quadrature_points(self.geometry, V, self.nq, who)
        uv = _nodal_vector(self.u, 1, _single_grid(V).num_nodes(), who)
        val, g = _dev.quad_eval(pts.verts, pts.p, pts.cp, uv, grad=True, nq=pts.nq, rational=self.rational)
        return pts, val.get_local(), point_unblock(g.get_local(), pts.npts, (pts.nsd,))

    def assemble_vector(self, V, row0=None, row1=None):
        _point_scope(self.geometry, V, "QuasilinearResidual", "scalar")
        _whole_rows(_single_grid(V).num_nodes(), row0, row1, "QuasilinearResidual", "patch")
        pts, uq, gq = self.state(V)
        out = _law_result(self.residual(pts.x, uq, gq), "QuasilinearResidual", "residual(x, u, grad u)",
                          "(flux or None, source or None)", [None] * 2)
        F = pts.vector_values(out[0], "QuasilinearResidual: flux") if out[0] is not None else None
        s = pts.values(out[1], "QuasilinearResidual: source") if out[1] is not None else None
        r = _dev.quad_load_flux(pts.verts, pts.p, pts.cp, s, F, nq=pts.nq, rational=self.rational)
        if self._load is not None:
            r.axpy(-1.0, self._load.assemble_vector(V))
        return r

    def tangent(self):
        return _QuasilinearTangent(self)


class _QuasilinearTangent(object):
    """``symmetric`` is that of the last assembled tangent and False before the first assembly: the tangent data depend on
    the state, so nothing is proved until they have been seen.  A ``Sum`` reads the attribute when it is BUILT and so takes
    this term for non-symmetric, which is the safe side; on a mapped patch the attribute informs the caller only
    (``assembleMatrix`` uses it for forms without a geometry)."""

    def __init__(self, res):
        self.res, self.geometry, self.symmetric = res, res.geometry, False

    def assemble_matrix(self, V, row0=None, row1=None):
        res = self.res
        _point_scope(res.geometry, V, "QuasilinearResidual.tangent", "scalar")
        _whole_rows(_single_grid(V).num_nodes(), row0, row1, "QuasilinearResidual.tangent", "patch")
        pts, uq, gq = res.state(V)
        out = _law_result(res._tangent(pts.x, uq, gq), "QuasilinearResidual", "tangent(x, u, grad u)",
                          "(A, b, c, m), any of them None", [None] * 4)
        form = CoefficientForm(res.geometry, out[0], out[1], out[2], out[3], nq=res.nq, rational=res.rational)
        A = form.assemble_matrix(V)
        self.symmetric = form.coefficients(V)[6]
        return A


# ---- vector-valued unknowns with point tangents: finite-strain elasticity (csrc/tg_material.hip) ----------------------------
def _shared_grid(V):
    """the node grid of a space whose fields share one continuous Q_p node grid of a tensor-product patch, or None"""
    g = V.grids[0]
    if getattr(g, "dg", True) or not hasattr(g, "axes") or any(
            gi.degree != g.degree or gi.dg or len(gi.axes) != len(g.axes) or
            any(not numpy.array_equal(a, b) for a, b in zip(gi.axes, g.axes)) for gi in V.grids[1:]):
        return None
    return g


def _one_shared_grid(V, who):
    """``_shared_grid`` or the refusal"""
    g = _shared_grid(V)
    if g is None:
        raise NotImplementedError("%s: the fields of the space must share one continuous Q_p node grid of a tensor-product "
                                  "patch (compatible, FieldList, multi-patch, T-spline and DG spaces are not supported)" % who)
    return g


def _vector_points(geometry, nq, who):
    """the quadrature points of the patch (those of the scalar space the fields share)"""
    return quadrature_points(geometry, geometry.V_control, nq, who)


def _nodal_vector(u, nF, n, who):
    """the nodal DeviceVector of a Function (or the vector itself), holding nF fields of n values"""
    uv = u.vector() if hasattr(u, "vector") else u
    if uv.size() != nF * n:
        raise ValueError("%s: u holds %d nodal values, the space has %s" % (who, uv.size(), n if nF == 1 else "%d fields of %d" % (nF, n)))
    return uv


def _field_by_field(uv, nF, n, call, size=None):
    """``call(u_i)`` for the nF fields of the nodal vector ``uv``, each copied into one scratch vector of n values.  With
    ``size`` the results (DeviceVectors of that many values) are gathered field after field in one DeviceVector, else
    they are returned as a list.  A tuple of sizes: ``call`` returns that many DeviceVectors, each gathered in one of its
    own, in the order of the tuple."""
    ui = _dev.DeviceVector(n, zero=False)
    sizes = size if isinstance(size, tuple) else (size,)
    outs = [[] if s is None else _dev.DeviceVector(nF * s, zero=False) for s in sizes]
    for i in range(nF):
        _dev.vec_copy_range(ui, 0, uv, i * n, n)
        parts = call(ui)
        for out, s, part in zip(outs, sizes, parts if isinstance(size, tuple) else (parts,)):
            if s is None:
                out.append(part)
            else:
                _dev.vec_copy_range(out, i * s, part, 0, s)
    return tuple(outs) if isinstance(size, tuple) else outs[0]


def _values_at_points(pts, nodal, nF, n, rational):
    """the nF fields of a nodal vector at the points, field after field (``tg_quad_eval``)"""
    return _field_by_field(nodal, nF, n, lambda ui: _dev.quad_eval(pts.verts, pts.p, pts.cp, ui, nq=pts.nq, rational=rational), pts.npts)


def _law_result(out, who, call, names, shapes):
    """what a host law returned: a tuple of len(shapes) entries, each brought to a float64 array of the given shape (None:
    the entry is handed on as it is)"""
    if not isinstance(out, tuple) or len(out) != len(shapes):
        raise ValueError("%s: %s returns %s" % (who, call, names))
    arrays = [o if s is None else numpy.asarray(o, dtype=numpy.float64) for o, s in zip(out, shapes)]
    if any(s is not None and a.shape != tuple(s) for a, s in zip(arrays, shapes)):
        raise ValueError("%s: %s returned shapes %s; %s has shapes %s" % (
            who, call, ", ".join(str(getattr(a, "shape", None)) for a in arrays), names, ", ".join(str(s) for s in shapes)))
    return arrays


class _LawTangent(object):
    """The tangent form of a ``_PointLawResidual``: the form the residual makes of its point tangent at the current state
    (``_tangent_form``).  ``symmetric`` is the residual's ``_law_symmetric()``: True for a built-in law (the tangent derives
    from an energy: major symmetry by the law, in the matrix to rounding); for a host law that of the last assembled tangent
    and False before the first assembly (see ``_QuasilinearTangent``).  Row blocks are refused before the law runs."""

    def __init__(self, res):
        self.res, self.geometry, self.symmetric = res, res.geometry, res._law_symmetric()

    def _form(self, V, row0, row1, block):
        res = self.res
        g, nF, pts = res._scope(V, res._who + ".tangent", row0, row1, block)
        form = res._tangent_form(pts, nF, res.law(V, False, True).tangent)
        form._symmetric_hint = self.symmetric = res._law_symmetric()
        return form

    def assemble_block(self, V, i, j, row0=None, row1=None):
        return self._form(V, row0, row1, True).assemble_block(V, i, j, row0, row1)

    def assemble_matrix(self, V, row0=None, row1=None):
        return self._form(V, row0, row1, False).assemble_matrix(V, row0, row1)


# [npts, nF, nK, nF, nK] point tangents (A[q, i, K, j, L], T[q, i, alpha, j, beta]) go to the device block by block, in
# the order (i, j, K, L, q) that ``tg_coef_transform_blocks`` and ``tg_jet_transform`` read; their major symmetry swaps (i, K)
# with (j, L)
_BLOCK_ORDER, _MAJOR_SWAP = (0, 2, 1, 3), (2, 3, 0, 1)


_SlotScaling = collections.namedtuple("_SlotScaling", "coef sigma after")


class _PointLawResidual(object):
    """A residual whose integrand is a law at the points: u is evaluated there field by field (with ``_keeps_u`` its point
    values stay in ``_u_points``; off for a residual the user built), the law -- ``_device_law``, or ``_host_law`` whose arrays
    are uploaded -- gives (load, tangent, psi), inadmissible points are refused, and the point data go through
    ``_load_vector`` and ``_tangent_form``.  ``ShellResidual`` and ``HyperelasticResidual`` say these, their scope (``_kind``,
    ``_check_space``), and where the value slots of the point data live, which is all ``DynamicResidual`` asks:
      ``nJ``, ``_value_load(out)``   the stride of the slots, and the vector whose value slots take inertia and penalty
      ``_slot_scaling(af, m_u, k)``  ``_SlotScaling``: ``coef`` of ``tg_point_dynamics`` for R / alpha_f, ``sigma`` = what the kernel
                                 multiplies the law's load by, ``after`` = the factor of the assembled vector (None: none).
                                 A shell: sigma = 1 / alpha_f; a solid: every value term times alpha_f, 1 / alpha_f after
      ``_load_vector(V, out, values, sigma)``   the load vector with those values; a load assembled by itself times ``sigma``
      ``_value_tangent``, ``_tangent_form``     the value-value entries of the tangent, and the form with them"""
    _who = _kind = _names = nJ = None
    _keeps_u, _u_points = False, None

    def __init__(self, u, geometry, material, known, builtin, body_force, nq, rational, device_law=True):
        if geometry is None:
            raise ValueError("%s: point data live on a mapped patch (geometry=...)" % self._who)
        if not callable(getattr(material, "host", None)):
            raise ValueError("%s: unknown material %r; %s" % (self._who, material, known))
        self.u, self.geometry, self.material, self.builtin = u, geometry, material, bool(builtin)
        self.body_force, self.nq, self.rational = body_force, nq, bool(rational)
        self.device_law = bool(device_law) and self.builtin
        self._host_symmetric = False

    def _arguments(self):
        """the keywords of the constructor, as the object holds them now"""
        return dict(body_force=self.body_force, nq=self.nq, rational=self.rational)

    def _at(self, u, keeps_u=False):
        """The same residual at another ``u``: built from the arguments this object holds now.  It shares no cache with
        this object and does not modify it.  ``keeps_u``: it keeps the point values of u of its last evaluation."""
        other = type(self)(u, self.geometry, self.material, **self._arguments())
        other._keeps_u = bool(keeps_u)
        return other

    def _check_space(self, g, nF, who):
        """a refusal of the space that ``_point_scope`` does not know"""

    def _scope(self, V, who, row0=None, row1=None, block=False):
        """(node grid, nF, points) of the space, or the refusal: of the scope, of row blocks, of the space"""
        g, nF = _point_scope(self.geometry, V, who, self._kind)[:2]
        _whole_rows((1 if block else nF) * g.num_nodes(), row0, row1, who, "patch")
        self._check_space(g, nF, who)
        return g, nF, _vector_points(self.geometry, self.nq, who)

    def _law(self, at, load, tangent, energy):
        """(load, tangent, psi) of the evaluation ``at`` as DeviceVectors (None where not asked for)"""
        if self.device_law:
            return self._device_law(at, load, tangent, energy)
        pts, who = at.pts, self._who
        loadh, Th, psih, shape = self._host_law(at, load or tangent)
        s = _point_data(loadh, pts, shape, "%s: %s" % (who, self._names[0])) if load else None
        T = None
        if tangent:
            T, self._host_symmetric = _point_data(Th, pts, shape + shape, "%s: %s" % (who, self._names[1]), _BLOCK_ORDER, _MAJOR_SWAP)
        return s, T, (_dev.DeviceVector(data=psih) if energy else None)

    def _law_symmetric(self):
        """whether the law's tangent is symmetric: by the law, or by the bits of a host law's last tangent"""
        return True if self.builtin else bool(self._host_symmetric)

    def assemble_vector(self, V, row0=None, row1=None):
        self._scope(V, self._who, row0, row1)
        return self._load_vector(V, self.law(V))

    def energy(self, V=None):
        if V is None:
            V = self.u.function_space()
        out = self.law(V, False, False, True)
        return out.pts.weights.inner(out.psi)

    def tangent(self):
        return _LawTangent(self)


def _det_inv(F):
    """(det F, F^-1) of [npts, n, n] matrices, n = 2, 3, by cofactors: any float dtype (numpy.linalg has no longdouble)"""
    n = F.shape[-1]
    cof = numpy.empty_like(F)
    if n == 2:
        cof[:, 0, 0], cof[:, 0, 1], cof[:, 1, 0], cof[:, 1, 1] = F[:, 1, 1], -F[:, 1, 0], -F[:, 0, 1], F[:, 0, 0]
        J = F[:, 0, 0] * F[:, 1, 1] - F[:, 0, 1] * F[:, 1, 0]
    else:
        for i in range(3):
            for K in range(3):
                i1, i2, K1, K2 = (i + 1) % 3, (i + 2) % 3, (K + 1) % 3, (K + 2) % 3
                cof[:, i, K] = F[:, i1, K1] * F[:, i2, K2] - F[:, i1, K2] * F[:, i2, K1]
        J = F[:, 0, 0] * cof[:, 0, 0] + F[:, 0, 1] * cof[:, 0, 1] + F[:, 0, 2] * cof[:, 0, 2]
    return J, cof.transpose(0, 2, 1) / J[:, None, None]


class _Material(object):
    """A built-in law: evaluated on the device by ``tg_material_points`` (``kind``), and on the host by ``host(F)`` for
    deformation gradients ``F [npts, nsd, nsd]`` of any float dtype -> (P [npts, nsd, nsd], A [npts, nsd, nsd, nsd, nsd] with
    A[q, i, K, j, L] = d P_iK / d F_jL, psi [npts])."""
    kind = None

    def __init__(self, lmbda, mu):
        self.lmbda, self.mu = float(lmbda), float(mu)


class LinearElastic(_Material):
    """psi = lambda/2 (tr eps)^2 + mu eps:eps with eps = sym grad u: small strain, the law of ``ElasticityForm``"""
    kind = 0

    def host(self, F):
        F = numpy.asarray(F)
        dt, n = F.dtype.type, F.shape[-1]
        lam, mu, I = dt(self.lmbda), dt(self.mu), numpy.eye(n, dtype=F.dtype)
        eps = dt(0.5) * (F + F.transpose(0, 2, 1)) - I
        tr = numpy.einsum("qii->q", eps)
        P = lam * tr[:, None, None] * I + dt(2) * mu * eps
        A = lam * numpy.einsum("iK,jL->iKjL", I, I) + mu * (numpy.einsum("ij,KL->iKjL", I, I) + numpy.einsum("iL,jK->iKjL", I, I))
        psi = dt(0.5) * lam * tr * tr + mu * numpy.einsum("qij,qij->q", eps, eps)
        return P, numpy.broadcast_to(A, (F.shape[0],) + A.shape).copy(), psi


class StVenantKirchhoff(_Material):
    """S = lambda tr E I + 2 mu E with E = (C - I)/2, P = F S; defined for any F"""
    kind = 1

    def host(self, F):
        F = numpy.asarray(F)
        dt, n = F.dtype.type, F.shape[-1]
        lam, mu, I = dt(self.lmbda), dt(self.mu), numpy.eye(n, dtype=F.dtype)
        E = dt(0.5) * (numpy.einsum("qaK,qaL->qKL", F, F) - I)
        trE = numpy.einsum("qii->q", E)
        S = lam * trE[:, None, None] * I + dt(2) * mu * E
        P = numpy.einsum("qia,qaK->qiK", F, S)
        B = numpy.einsum("qia,qja->qij", F, F)
        A = numpy.einsum("ij,qKL->qiKjL", I, S) + lam * numpy.einsum("qiK,qjL->qiKjL", F, F) + \
            mu * (numpy.einsum("qiL,qjK->qiKjL", F, F) + numpy.einsum("KL,qij->qiKjL", I, B))
        psi = dt(0.5) * lam * trE * trE + mu * numpy.einsum("qij,qij->q", E, E)
        return P, A, psi


class NeoHookean(_Material):
    """compressible neo-Hookean, psi = mu/2 (tr C - nsd) - mu ln J + lambda/2 (ln J)^2; needs J > 0"""
    kind = 2

    def host(self, F):
        F = numpy.asarray(F)
        dt, n = F.dtype.type, F.shape[-1]
        lam, mu, I = dt(self.lmbda), dt(self.mu), numpy.eye(n, dtype=F.dtype)
        J, Fi = _det_inv(F)
        if numpy.any(~(J > 0)):
            raise ValueError("NeoHookean: %d points with J <= 0 (smallest J = %g)" % (int(numpy.sum(~(J > 0))), float(numpy.min(J))))
        lnJ = numpy.log(J)
        FiT = Fi.transpose(0, 2, 1)
        c1 = (mu - lam * lnJ)[:, None, None]
        P = mu * F - c1 * FiT
        A = mu * numpy.einsum("ij,KL->iKjL", I, I)[None] + c1[:, :, :, None, None] * numpy.einsum("qLi,qKj->qiKjL", Fi, Fi) + \
            lam * numpy.einsum("qKi,qLj->qiKjL", Fi, Fi)
        psi = dt(0.5) * mu * (numpy.einsum("qiK,qiK->q", F, F) - dt(n)) - mu * lnJ + dt(0.5) * lam * lnJ * lnJ
        return P, A, psi


class VectorCoefficientForm(object):
    """a(u, v) = int d_K v_i A_iKjL d_L u_j + v_i M_ij u_j dx on the mapped patch for a vector-valued unknown: nF = nsd = d
    fields on one continuous Q_p node grid, dofs field after field (the space of ``ElasticityForm``); grad and dx as
    ``spline.grad`` / ``spline.dx``.  The tangent of a solid, ``derivative(derivative(psi*spline.dx, u), u)`` of the reference.

    ``tangent``: ``[npts, nF, nsd, nF, nsd]`` point values A[q, i, K, j, L] (numbered as ``QuadraturePoints``), a callable of
    the points ``x [npts, nsd]`` returning that, or a DeviceVector in the block layout -- A_iKjL at
    (((i nF + j) nsd + K) nsd + L) npts + q.  ``reaction``: ``[npts, nF, nF]`` (or one nF x nF matrix, a callable, or a
    DeviceVector with M_ij at (i nF + j) npts + q): inertia and spring terms.  ``nq`` Gauss points per direction (p + 1 when
    None).  ``rational``: every component function phi / W_h.

    ``symmetric`` is True only when the bits prove it: A[i, K, j, L] == A[j, L, i, K] and M[i, j] == M[j, i] at every point.
    One pass brings all nF^2 blocks to the reference element (``tg_coef_transform_blocks``), each block is then a scalar
    coefficient form on the element-coupling pattern (``tg_assemble_coef_blocks``); peak point data (d^4 + 16 d^2) npts
    doubles in 3-D.  One rank, all rows."""

    def __init__(self, geometry, tangent, reaction=None, nq=None, rational=False):
        if geometry is None:
            raise ValueError("VectorCoefficientForm: point tangents live on a mapped patch (geometry=...)")
        if tangent is None:
            raise ValueError("VectorCoefficientForm: no tangent")
        self.geometry, self.tangent, self.reaction, self.nq, self.rational = geometry, tangent, reaction, nq, bool(rational)
        # (set by a caller who proves the symmetry: HyperelasticResidual by its law, of a reaction it wrote on the device)
        self._symmetric_hint = self._reaction_hint = None

    def coefficients(self, V):
        """(points, A, M, symmetric) with the point data as DeviceVectors in the block layout (M None = absent): computed
        once per set of points"""
        who = "VectorCoefficientForm"
        g, nF = _point_scope(self.geometry, V, who, "vector")
        pts = _vector_points(self.geometry, self.nq, who)
        return _per_points(self, "_static", pts, lambda: self._static_coefficients(pts, nF, who))

    def _static_coefficients(self, pts, nF, who):
        A, sym = _point_data(self.tangent, pts, (nF, pts.nsd, nF, pts.nsd), who + ": tangent", _BLOCK_ORDER, _MAJOR_SWAP,
                             hint=self._symmetric_hint)
        M, symM = None, True
        if self.reaction is not None:
            M, symM = _point_data(self.reaction, pts, (nF, nF), who + ": reaction", swap=(1, 0), hint=self._reaction_hint)
        return pts, A, M, bool(sym and symM)

    @property
    def symmetric(self):
        return self.coefficients(self.geometry.V)[3]

    def _transformed(self, V):
        pts, A, M, _ = self.coefficients(V)
        return pts, _dev.coef_transform_blocks(pts.verts, pts.p, pts.cp, A, M, nq=pts.nq, rational=self.rational)

    def assemble_block(self, V, i, j, row0=None, row1=None):
        """block (i, j): test field i, trial field j (all rows of the field)"""
        g, nF = _point_scope(self.geometry, V, "VectorCoefficientForm", "vector")
        if not (0 <= int(i) < nF and 0 <= int(j) < nF):
            raise ValueError("VectorCoefficientForm: block (%r, %r) of a %d-field space" % (i, j, nF))
        _whole_rows(g.num_nodes(), row0, row1, "VectorCoefficientForm", "patch")
        pts, coef = self._transformed(V)
        return _dev.assemble_coef_matrix(pts.verts, pts.p, pts.cp, _dev.coef_block(pts.verts, coef, int(i), int(j), pts.nq), nq=pts.nq)

    def assemble_matrix(self, V, row0=None, row1=None):
        g, nF = _point_scope(self.geometry, V, "VectorCoefficientForm", "vector")
        _whole_rows(nF * g.num_nodes(), row0, row1, "VectorCoefficientForm", "patch")
        pts, coef = self._transformed(V)
        return _dev.assemble_coef_blocks(pts.verts, pts.p, pts.cp, coef, nq=pts.nq)


def _field_loads(pts, n, nF, s, F, rational):
    """the nF component loads of int s_i v_i + F_iK d_K v_i, written field after field: nF calls of ``tg_quad_load_flux``;
    ``s``: list of nF DeviceVectors (or None), ``F``: DeviceVector with F_iK at (i nsd + K) npts + q (or None)"""
    out = _dev.DeviceVector(nF * n, zero=False)
    size = pts.nsd * pts.npts
    Fi = _dev.DeviceVector(size, zero=False) if F is not None else None
    for i in range(nF):
        if F is not None:
            _dev.vec_copy_range(Fi, 0, F, i * size, size)
        if F is None and (s is None or s[i] is None):
            part = _dev.DeviceVector(n)
        else:
            part = _dev.quad_load_flux(pts.verts, pts.p, pts.cp, s[i] if s is not None else None, Fi, nq=pts.nq, rational=rational)
        _dev.vec_copy_range(out, i * n, part, 0, n)
    return out


def _field_values(pts, f, nF, who, scale=1.0):
    """nF DeviceVectors of the components of a vector field at the points: a callable ``x -> [npts, nF]`` (on a face also
    of ``(x, n)``), an array of that shape, or nF numbers"""
    v = scale * point_block(_on_points(f, pts), pts.npts, (nF,), who=who)
    return [_dev.DeviceVector(data=v[c * pts.npts:(c + 1) * pts.npts]) for c in range(nF)]


class VectorLoadForm(object):
    """L(v) = int f . v + flux : grad v dx on the space of ``VectorCoefficientForm``: ``f`` ``[npts, nF]`` (or a callable of the
    points returning that, nF numbers, or None), ``flux`` ``[npts, nF, nsd]`` (flux[q, i, K] pairs with d_K v_i; a callable,
    or a DeviceVector with flux_iK at (i nsd + K) npts + q).  The component loads are written field after field.
    ``rational``: v_i the functions phi / W_h."""

    def __init__(self, f, geometry, flux=None, nq=None, rational=False):
        if geometry is None:
            raise ValueError("VectorLoadForm: point values live on a mapped patch (geometry=...)")
        if f is None and flux is None:
            raise ValueError("VectorLoadForm: neither f nor flux given")
        self.f, self.geometry, self.flux, self.nq, self.rational = f, geometry, flux, nq, bool(rational)

    def assemble_vector(self, V, row0=None, row1=None):
        who = "VectorLoadForm"
        g, nF = _point_scope(self.geometry, V, who, "vector")
        n = g.num_nodes()
        _whole_rows(nF * n, row0, row1, who, "patch")
        pts = _vector_points(self.geometry, self.nq, who)

        def static():
            s = _field_values(pts, self.f, nF, who + ": f") if self.f is not None else None
            return s, (_point_data(self.flux, pts, (nF, pts.nsd), who + ": flux") if self.flux is not None else None)
        s, F = _per_points(self, "_static", pts, static)
        return _field_loads(pts, n, nF, s, F, self.rational)


_SolidGradient = collections.namedtuple("_SolidGradient", "pts g nF H")
_SolidLaw = collections.namedtuple("_SolidLaw", "pts g nF load tangent psi")


class HyperelasticResidual(_PointLawResidual):
    """Residual of finite-strain elasticity on the mapped patch, R(v) = int P(F) : grad v - f . v dx with F = I + grad u: what
    ``derivative(psi*spline.dx, u)`` of the reference gives for a solid.  The reference configuration is the patch
    (x = F_geom(xi), grad = ``spline.grad``); ``u`` the displacement ``Function`` on the space of ``ElasticityForm`` (nF = nsd
    = d fields, d = 2 is plane strain), read at assembly time.

    ``material``: ``LinearElastic``, ``StVenantKirchhoff`` or ``NeoHookean`` -- evaluated at the points ON THE DEVICE
    (``tg_material_points``): grad u, P and the tangent never leave it -- or any object with
    ``host(F [npts, nsd, nsd]) -> (P [npts, nsd, nsd], A [npts, nsd, nsd, nsd, nsd], psi [npts])``, a host law whose arrays
    are uploaded and go through the same transform and assembly.  ``body_force``: as ``f`` of ``VectorLoadForm``.

    ``assemble_vector``: grad u per field by the kernel of ``evaluateAtQuadrature(grad=True)``, the law, then the flux loads.
    ``tangent()``: the form of A = dP/dF (``VectorCoefficientForm``); for a built-in material ``symmetric`` is True, proved by
    the law (A derives from an energy); for a host law it is what the bits of the last assembled tangent prove.
    ``energy(V)`` = sum_q wdet_q psi_q.  A neo-Hookean state with J <= 0 somewhere raises ``RuntimeError`` naming the number
    of such points and the smallest J.  Runs under ``solveNonlinearVariationalProblem`` and inside ``Sum`` with
    ``BoundaryLoadForm`` tractions.  ``rational``: u_i = u_h,i / W_h, tested against phi / W_h."""

    _who, _kind, _names, nJ = "HyperelasticResidual", "vector", ("P", "A"), 1

    def __init__(self, u, geometry, material, body_force=None, nq=None, rational=False):
        _PointLawResidual.__init__(self, u, geometry, material, "LinearElastic, StVenantKirchhoff, NeoHookean, or an object with "
                                   "host(F) -> (P, A, psi)", isinstance(material, _Material) and material.kind in (0, 1, 2),
                                   body_force, nq, rational)

    def grad_u(self, V):
        """(points, node grid, nF, DeviceVector with d u_i / d x_K at (i nsd + K) npts + q)"""
        g, nF, pts = self._scope(V, self._who)
        n, size = g.num_nodes(), pts.nsd * pts.npts
        uv = _nodal_vector(self.u, nF, n, self._who)
        both = lambda ui: _dev.quad_eval(pts.verts, pts.p, pts.cp, ui, grad=True, nq=pts.nq, rational=self.rational)
        if self._keeps_u:                       # the values the kernel writes next to the gradient
            self._u_points, H = _field_by_field(uv, nF, n, both, (pts.npts, size))
        else:
            H = _field_by_field(uv, nF, n, lambda ui: both(ui)[1], size)
        return _SolidGradient(pts, g, nF, H)

    def law(self, V, stress=True, tangent=False, energy=False):
        """(points, node grid, nF, P, A, psi) at the current state, as DeviceVectors (None where not asked for)"""
        at = _SolidGradient(*self.grad_u(V))
        return _SolidLaw(at.pts, at.g, at.nF, *self._law(at, stress, tangent, energy))

    def _device_law(self, at, stress, tangent, energy):
        m = self.material
        P, A, psi, nbad, jmin = _dev.material_points(m.kind, m.lmbda, m.mu, at.pts.nsd, at.H, stress, tangent, energy)
        if nbad > 0:
            raise RuntimeError("HyperelasticResidual: %d quadrature points with J <= 0 (smallest J = %g): %s is not "
                               "defined there" % (nbad, jmin, type(m).__name__))
        return P, A, psi

    def _host_law(self, at, loads):
        nsd, npts = at.pts.nsd, at.pts.npts
        F = point_unblock(at.H.get_local(), npts, (nsd, nsd)) + numpy.eye(nsd)
        Ph, Ah, psih = _law_result(self.material.host(F), self._who, "material.host(F)", "(P, A, psi)",
                                   [(npts, nsd, nsd), (npts, nsd, nsd, nsd, nsd), (npts,)])
        return Ph, Ah, psih, (nsd, nsd)

    def _body_force(self, pts, nF):
        """-f at the points, one DeviceVector per field (None without a body force): once per set of points"""
        if self.body_force is None:
            return None
        return _per_points(self, "_fq", pts, lambda: _field_values(pts, self.body_force, nF, self._who + ": body_force", scale=-1.0))

    def _load_vector(self, V, out, values=None, sigma=1.0):
        """the load of the flux P next to a value load: of -f, or of the ``values`` of ``_value_load``, which hold -f
        already (``sigma`` has nothing to scale here: the body force is among the values)"""
        pts, nF, npts = out.pts, out.nF, out.pts.npts
        if values is None:
            s = self._body_force(pts, nF)
        else:
            s = [_dev.DeviceVector(npts, zero=False) for _ in range(nF)]
            for i in range(nF):
                _dev.vec_copy_range(s[i], 0, values, i * npts, npts)
        return _field_loads(pts, out.g.num_nodes(), nF, s, out.load, self.rational)

    # -- the value slots: the stress is a flux, so they are vectors of their own (nJ = 1) next to P and A, and every term
    #    they hold is multiplied by alpha_f; the assembled vector is divided once
    def _value_load(self, out):
        pts, nF, npts = out.pts, out.nF, out.pts.npts
        s = _dev.DeviceVector(nF * npts)
        for i, fi in enumerate(self._body_force(pts, nF) or ()):
            _dev.vec_copy_range(s, i * npts, fi, 0, npts)
        return s

    def _slot_scaling(self, af, m_u, k):
        return _SlotScaling((1.0, af * m_u, af, 0.0, k, 0.0, 0.0), 1.0, 1.0 / af if af != 1.0 else None)

    def _value_tangent(self, pts, nF, tangent=None):
        return _dev.DeviceVector(nF * nF * pts.npts)

    def _tangent_form(self, pts, nF, tangent, values=None):
        """the ``VectorCoefficientForm`` of A (None: of zeros) with the value-value entries as its reaction: they were
        written on the device, density and k n (x) n, and are symmetric by construction"""
        if tangent is None:
            tangent = _dev.DeviceVector(nF ** 4 * pts.npts)
        form = VectorCoefficientForm(self.geometry, tangent, reaction=values, nq=self.nq, rational=self.rational)
        form._reaction_hint = None if values is None else True
        return form


# ---- first-order systems: nF fields with the four point terms per block (tg_coef_transform_system) --------------------------
def _system_block(f, pts, shape, who, perm=None):
    """(DeviceVector, its values on the host in the device layout as [components in the order ``perm``] + [npts], or None for
    a DeviceVector, which is taken as it is after a length check) of one term of a system form"""
    if isinstance(f, _dev.DeviceVector):
        return _point_data(f, pts, shape, who), None
    flat = point_block(numpy.asarray(_on_points(f, pts), dtype=numpy.float64), pts.npts, shape, perm, who=who)
    order = range(len(shape)) if perm is None else perm
    return _dev.DeviceVector(data=flat), flat.reshape(tuple(shape[a] for a in order) + (pts.npts,))


class SystemCoefficientForm(object):
    """a(u, v) = sum_ij int d_K v_i A_iKjL d_L u_j + d_K v_i b_iKj u_j + v_i c_ijL d_L u_j + v_i m_ij u_j dx on the mapped patch for
    a FIRST-ORDER SYSTEM: nF >= 1 fields on the control mesh's scalar basis sharing one continuous Q_p node grid, dofs field
    after field (``EqualOrderSpline(nF, mesh)``), d = 1, 2, 3, nsd >= d, nF independent of nsd; u the trial function = column,
    v the test function = row.  Coupled advection-diffusion-reaction, thermoelasticity, or the tangent of a stabilised flow
    (``FlowResidual``).

    ``diffusion`` A ``[npts, nF, nsd, nF, nsd]``, ``flux_velocity`` b ``[npts, nF, nsd, nF]``, ``velocity`` c
    ``[npts, nF, nF, nsd]``, ``reaction`` m ``[npts, nF, nF]``; each an array (or one block for every point), a callable of the
    points ``x [npts, nsd]`` returning one, None, or a DeviceVector in the device layout: A_iKjL at
    (((i nF + j) nsd + K) nsd + L) npts + q, b_iKj at ((i nF + j) nsd + K) npts + q, c_ijL at ((i nF + j) nsd + L) npts + q, m_ij
    at (i nF + j) npts + q.  ``nq`` Gauss points per direction (p + 1 when None).  ``rational``: every field phi / W_h.

    ``symmetric`` is True only when the bits prove all of: A[i, K, j, L] == A[j, L, i, K], b[i, K, j] == c[j, i, K] (both absent,
    or both given) and m[i, j] == m[j, i], at every point.  One pass brings all nF^2 blocks to the reference element
    (``tg_coef_transform_system``), each block is then a scalar coefficient form on the element-coupling pattern
    (``tg_assemble_coef_system``).  One rank, all rows."""

    def __init__(self, geometry, diffusion=None, flux_velocity=None, velocity=None, reaction=None, nq=None, rational=False):
        if geometry is None:
            raise ValueError("SystemCoefficientForm: point coefficients live on a mapped patch (geometry=...)")
        self.geometry, self.nq, self.rational = geometry, nq, bool(rational)
        self.diffusion, self.flux_velocity, self.velocity, self.reaction = diffusion, flux_velocity, velocity, reaction
        self._symmetric_hint = None              # (set by a caller who knows: FlowResidual, whose tangent is not symmetric)

    def coefficients(self, V):
        """(points, nF, A, b, c, M, symmetric) with the point data as DeviceVectors in the device layout (None = absent):
        computed once per set of points"""
        who = "SystemCoefficientForm"
        g, nF = _point_scope(self.geometry, V, who, "system")
        pts = _vector_points(self.geometry, self.nq, who)
        return _per_points(self, "_static", pts, lambda: self._static_coefficients(pts, nF, who))

    def _static_coefficients(self, pts, nF, who):
        nsd = pts.nsd
        terms = (("diffusion", self.diffusion, (nF, nsd, nF, nsd), _BLOCK_ORDER), ("flux_velocity", self.flux_velocity, (nF, nsd, nF), (0, 2, 1)),
                 ("velocity", self.velocity, (nF, nF, nsd), None), ("reaction", self.reaction, (nF, nF), None))
        dev, host = [], []
        for name, f, shape, perm in terms:
            v, h = (None, None) if f is None else _system_block(f, pts, shape, "%s: %s" % (who, name), perm)
            dev.append(v)
            host.append(h)
        if self._symmetric_hint is not None:
            sym = bool(self._symmetric_hint)
        else:
            A, b, c, M = [h if h is not None or v is None else v.get_local().reshape(h_shape + (pts.npts,))
                          for v, h, h_shape in zip(dev, host, ((nF, nF, nsd, nsd), (nF, nF, nsd), (nF, nF, nsd), (nF, nF)))]
            sym = (A is None or _same_bits(A, A.transpose(1, 0, 3, 2, 4))) and (M is None or _same_bits(M, M.transpose(1, 0, 2))) and \
                ((b is None and c is None) or (b is not None and c is not None and _same_bits(b, c.transpose(1, 0, 2, 3))))
        return (pts, nF) + tuple(dev) + (bool(sym),)

    @property
    def symmetric(self):
        return self.coefficients(self.geometry.V)[6]

    def _transformed(self, V):
        pts, nF, A, b, c, M, _ = self.coefficients(V)
        return pts, nF, _dev.coef_transform_system(pts.verts, pts.p, pts.cp, nF, A, b, c, M, nq=pts.nq, rational=self.rational)

    def assemble_block(self, V, i, j, row0=None, row1=None):
        """block (i, j): test field i, trial field j (all rows of the field)"""
        g, nF = _point_scope(self.geometry, V, "SystemCoefficientForm", "system")
        if not (0 <= int(i) < nF and 0 <= int(j) < nF):
            raise ValueError("SystemCoefficientForm: block (%r, %r) of a %d-field space" % (i, j, nF))
        _whole_rows(g.num_nodes(), row0, row1, "SystemCoefficientForm", "patch")
        pts, nF, A, b, c, M, _ = self.coefficients(V)
        # the one-field transform of the block's own data: the bits of that block in the transform of all nF^2 (tested)
        blk, nsd, npts = int(i) * nF + int(j), pts.nsd, pts.npts
        own = []
        for v, each in ((A, nsd * nsd), (b, nsd), (c, nsd), (M, 1)):
            w = None
            if v is not None:
                w = _dev.DeviceVector(each * npts, zero=False)
                _dev.vec_copy_range(w, 0, v, blk * each * npts, each * npts)
            own.append(w)
        coef = _dev.coef_transform_system(pts.verts, pts.p, pts.cp, 1, *own, nq=pts.nq, rational=self.rational)
        return _dev.assemble_coef_matrix(pts.verts, pts.p, pts.cp, coef, nq=pts.nq)

    def assemble_matrix(self, V, row0=None, row1=None):
        g, nF = _point_scope(self.geometry, V, "SystemCoefficientForm", "system")
        _whole_rows(nF * g.num_nodes(), row0, row1, "SystemCoefficientForm", "patch")
        pts, nF, coef = self._transformed(V)
        return _dev.assemble_coef_system(pts.verts, pts.p, pts.cp, nF, coef, nq=pts.nq)


class SystemLoadForm(object):
    """L(v) = sum_i int s_i v_i + F_iK d_K v_i dx on the space of ``SystemCoefficientForm``: ``f`` = s ``[npts, nF]`` (or a callable
    of the points returning that, nF numbers, or None), ``flux`` ``[npts, nF, nsd]`` (a callable, or a DeviceVector with F_iK at
    (i nsd + K) npts + q).  nF calls of ``tg_quad_load_flux``, written field after field.  ``rational``: v_i = phi / W_h."""

    def __init__(self, f=None, geometry=None, flux=None, nq=None, rational=False):
        if geometry is None:
            raise ValueError("SystemLoadForm: point values live on a mapped patch (geometry=...)")
        if f is None and flux is None:
            raise ValueError("SystemLoadForm: neither f nor flux given")
        self.f, self.geometry, self.flux, self.nq, self.rational = f, geometry, flux, nq, bool(rational)

    def assemble_vector(self, V, row0=None, row1=None):
        who = "SystemLoadForm"
        g, nF = _point_scope(self.geometry, V, who, "system")
        n = g.num_nodes()
        _whole_rows(nF * n, row0, row1, who, "patch")
        pts = _vector_points(self.geometry, self.nq, who)

        def static():
            s = _field_values(pts, self.f, nF, who + ": f") if self.f is not None else None
            return s, (_point_data(self.flux, pts, (nF, pts.nsd), who + ": flux") if self.flux is not None else None)
        s, F = _per_points(self, "_static", pts, static)
        return _field_loads(pts, n, nF, s, F, self.rational)


def _system_state(geometry, V, u, nq, rational, who):
    """(points, node grid, nF, values of the nF fields [nF npts], their Cartesian gradients [(i nsd + K) npts + q]) of ``u``:
    field by field through ``tg_quad_eval``"""
    g, nF = _point_scope(geometry, V, who, "system")
    pts = _vector_points(geometry, nq, who)
    n = g.num_nodes()
    uv = _nodal_vector(u, nF, n, who)
    both = lambda ui: _dev.quad_eval(pts.verts, pts.p, pts.cp, ui, grad=True, nq=pts.nq, rational=rational)
    Uq, Gq = _field_by_field(uv, nF, n, both, (pts.npts, pts.nsd * pts.npts))
    return pts, g, nF, Uq, Gq


class SystemResidual(object):
    """Residual of a first-order system  -d_K flux_iK(x, U, grad U) + source_i(x, U, grad U) = f_i  in weak form,
    R(v) = sum_i int flux_iK d_K v_i + source_i v_i - f_i v_i dx, on the space of ``SystemCoefficientForm``, the nonlinearity
    evaluated AT THE QUADRATURE POINTS by host callables: the vector analogue of ``QuasilinearResidual``.

    ``residual(x, U [npts, nF], G [npts, nF, nsd]) -> (flux [npts, nF, nsd] | None, source [npts, nF] | None)`` and
    ``tangent(x, U, G) -> (A, b, c, m)`` = (d flux / d grad U ``[npts, nF, nsd, nF, nsd]``, d flux / d U ``[npts, nF, nsd, nF]``,
    d source / d grad U ``[npts, nF, nF, nsd]``, d source / d U ``[npts, nF, nF]``), any of them None.  ``u``: the current FE
    ``Function``, read at assembly time; ``f``: as for ``SystemLoadForm``.  ``tangent()``: the form whose matrix is the
    ``SystemCoefficientForm`` of the tangent data; its ``symmetric`` is that of the last assembled tangent (False before).
    Runs under ``solveNonlinearVariationalProblem`` and inside ``Sum``.  ``rational``: U_i = u_h,i / W_h, tested against phi / W_h."""

    def __init__(self, u, geometry, residual, tangent, f=None, nq=None, rational=False):
        if geometry is None:
            raise ValueError("SystemResidual: point coefficients live on a mapped patch (geometry=...)")
        self.u, self.geometry, self.residual, self._tangent = u, geometry, residual, tangent
        self.f, self.nq, self.rational = f, nq, bool(rational)
        self._load = SystemLoadForm(f, geometry, nq=nq, rational=rational) if f is not None else None

    def state(self, V):
        """(points, node grid, nF, U [npts, nF], its Cartesian gradient [npts, nF, nsd]) on the host"""
        pts, g, nF, Uq, Gq = _system_state(self.geometry, V, self.u, self.nq, self.rational, "SystemResidual")
        return pts, g, nF, point_unblock(Uq.get_local(), pts.npts, (nF,)), point_unblock(Gq.get_local(), pts.npts, (nF, pts.nsd))

    def assemble_vector(self, V, row0=None, row1=None):
        who = "SystemResidual"
        g, nF = _point_scope(self.geometry, V, who, "system")
        _whole_rows(nF * g.num_nodes(), row0, row1, who, "patch")
        pts, g, nF, Uq, Gq = self.state(V)
        F, s = _law_result(self.residual(pts.x, Uq, Gq), who, "residual(x, U, grad U)", "(flux or None, source or None)", [None] * 2)
        Fd = _point_data(F, pts, (nF, pts.nsd), who + ": flux") if F is not None else None
        sd = _field_values(pts, s, nF, who + ": source") if s is not None else None
        r = _field_loads(pts, g.num_nodes(), nF, sd, Fd, self.rational)
        if self._load is not None:
            r.axpy(-1.0, self._load.assemble_vector(V))
        return r

    def tangent(self):
        return _SystemTangent(self)


class _SystemTangent(object):
    """see ``_QuasilinearTangent``: ``symmetric`` is that of the last assembled tangent"""

    def __init__(self, res):
        self.res, self.geometry, self.symmetric = res, res.geometry, False

    def _form(self, V, rows, row0, row1):
        res, who = self.res, "SystemResidual.tangent"
        g, nF = _point_scope(res.geometry, V, who, "system")
        _whole_rows((nF if rows else 1) * g.num_nodes(), row0, row1, who, "patch")
        pts, g, nF, Uq, Gq = res.state(V)
        out = _law_result(res._tangent(pts.x, Uq, Gq), "SystemResidual", "tangent(x, U, grad U)", "(A, b, c, m), any of them None",
                          [None] * 4)
        form = SystemCoefficientForm(res.geometry, out[0], out[1], out[2], out[3], nq=res.nq, rational=res.rational)
        self.symmetric = form.coefficients(V)[6]
        return form

    def assemble_block(self, V, i, j, row0=None, row1=None):
        return self._form(V, False, row0, row1).assemble_block(V, i, j)

    def assemble_matrix(self, V, row0=None, row1=None):
        return self._form(V, True, row0, row1).assemble_matrix(V)


# ---- incompressible flow: equal-order velocity and pressure, SUPG / PSPG / LSIC (csrc/tg_flow.hip) ---------------------------
class IncompressibleFlow(object):
    """The stabilised incompressible Navier-Stokes law at the points, nF = nsd + 1 fields (u_1 .. u_nsd, p) of equal order:
    Galerkin + SUPG + PSPG + LSIC (Bazilevs, Calo, Cottrell, Hughes, Reali, Scovazzi, CMAME 197 (2007) 173-201, without the
    cross- and Reynolds-stress terms).  ``density`` rho > 0 and ``viscosity`` mu >= 0 are constants, nu = mu / rho.  With
    a = c_a u + a0 (the acceleration of a time integrator; zero for a steady problem), f the body force per unit mass and G the
    element metric (``QuadraturePoints.metric``):

        r_i   = rho (a_i + u_L d_L u_i - f_i) + d_i p             strong momentum residual, viscous term OMITTED
        tau_M = (4 / dt^2 + u . G u + C_I nu^2 G:G)^(-1/2)         tau_C = 1 / (tau_M tr G)         (4 / dt^2 = 0 when steady)
        s_i   = rho (a_i + u_L d_L u_i - f_i)
        F_iK  = mu (d_K u_i + d_i u_K) - p d_iK + tau_M u_K r_i + rho tau_C (d_L u_L) d_iK
        s_p   = d_L u_L                                           F_pK = (tau_M / rho) r_K

    and R(v, q) = int s_i v_i + F_iK d_K v_i + s_p q + F_pK d_K q dx.  The viscous part of r needs Cartesian second derivatives,
    which the point kernels do not form; without it the stabilisation is consistent only up to O(tau_M mu lap u), which limits
    the spatial order to about 2.  The tangent is the EXACT derivative of (s, F) with respect to (u, grad u, p, grad p), the
    dependence of tau on u included, so that Newton on the discrete problem converges quadratically.

    ``C_I``: the constant of the element-wise inverse estimate in tau_M.  The default 36 is the value Bazilevs et al. (2007) use
    with quadratic NURBS; it is a parameter of the method, not a number tuned to the tests -- higher degrees ask for a larger one.

    Evaluated on the device by ``tg_flow_points``; ``host`` is the same law in numpy for any float dtype, and any object with
    such a ``host`` serves ``FlowResidual`` through the same path."""

    def __init__(self, density, viscosity, C_I=36.0):
        self.density, self.viscosity, self.C_I = float(density), float(viscosity), float(C_I)
        if not self.density > 0.0 or not self.viscosity >= 0.0 or not self.C_I >= 0.0:
            raise ValueError("IncompressibleFlow: density > 0, viscosity >= 0 and C_I >= 0 (density = %r, viscosity = %r, C_I = %r)"
                             % (density, viscosity, C_I))

    def params(self, c_a=0.0, dt4=0.0):
        return (self.density, self.viscosity, float(c_a), float(dt4), self.C_I)

    def host(self, U, gradU, G, c_a=0.0, a0=None, f=None, dt4=0.0):
        """``U [npts, nsd + 1]``, ``gradU [npts, nsd + 1, nsd]``, ``G [npts, nsd, nsd]``, ``a0`` / ``f`` ``[npts, nsd]`` or None ->
        (s [npts, nF], F [npts, nF, nsd], A [npts, nF, nsd, nF, nsd], b [npts, nF, nsd, nF], c [npts, nF, nF, nsd],
        m [npts, nF, nF], tau [npts, 2]) in the dtype of ``U``"""
        U, gradU, G = numpy.asarray(U), numpy.asarray(gradU), numpy.asarray(G)
        dt = U.dtype.type
        npts, nF = U.shape
        n = nF - 1
        rho, mu, ca, CI, d4 = dt(self.density), dt(self.viscosity), dt(c_a), dt(self.C_I), dt(dt4)
        I = numpy.eye(n, dtype=U.dtype)
        u, p, H, gp = U[:, :n], U[:, n], gradU[:, :n, :], gradU[:, n, :]
        acc = ca * u + numpy.einsum("qL,qiL->qi", u, H)
        if a0 is not None:
            acc = acc + numpy.asarray(a0, dtype=U.dtype)
        if f is not None:
            acc = acc - numpy.asarray(f, dtype=U.dtype)
        sm = rho * acc
        r = sm + gp
        div = numpy.einsum("qii->q", H)
        Gu = numpy.einsum("qKL,qL->qK", G, u)
        nu = mu / rho
        tM = dt(1) / numpy.sqrt(d4 + numpy.einsum("qK,qK->q", u, Gu) + CI * nu * nu * numpy.einsum("qKL,qKL->q", G, G))
        tC = dt(1) / (tM * numpy.einsum("qKK->q", G))
        dtM = -(tM ** 3)[:, None] * Gu
        dtC = -(tC / tM)[:, None] * dtM
        s = numpy.zeros((npts, nF), dtype=U.dtype)
        F = numpy.zeros((npts, nF, n), dtype=U.dtype)
        s[:, :n], s[:, n] = sm, div
        F[:, :n, :] = mu * (H + H.transpose(0, 2, 1)) + tM[:, None, None] * numpy.einsum("qK,qi->qiK", u, r) + \
            ((rho * tC * div - p)[:, None, None] * I)
        F[:, n, :] = (tM / rho)[:, None] * r
        A = numpy.zeros((npts, nF, n, nF, n), dtype=U.dtype)
        b = numpy.zeros((npts, nF, n, nF), dtype=U.dtype)
        c = numpy.zeros((npts, nF, nF, n), dtype=U.dtype)
        m = numpy.zeros((npts, nF, nF), dtype=U.dtype)
        R = rho * (H + ca * I)                                                  # d r_i / d u_j
        m[:, :n, :n] = R
        c[:, :n, :n, :] = rho * numpy.einsum("ij,qL->qijL", I, u)
        c[:, n, :n, :] = I
        b[:, :n, :, :n] = numpy.einsum("qj,qK,qi->qiKj", dtM, u, r) + tM[:, None, None, None] * (
            numpy.einsum("Kj,qi->qiKj", I, r) + numpy.einsum("qK,qij->qiKj", u, R)) + \
            rho * numpy.einsum("q,iK,qj->qiKj", div, I, dtC)
        b[:, :n, :, n] = -I
        b[:, n, :, :n] = (numpy.einsum("qj,qK->qKj", dtM, r) + tM[:, None, None] * R) / rho
        A[:, :n, :, :n, :] = mu * (numpy.einsum("ij,KL->iKjL", I, I) + numpy.einsum("iL,jK->iKjL", I, I)) + \
            rho * tM[:, None, None, None, None] * numpy.einsum("ij,qK,qL->qiKjL", I, u, u) + \
            rho * tC[:, None, None, None, None] * numpy.einsum("iK,jL->iKjL", I, I)
        A[:, :n, :, n, :] = tM[:, None, None, None] * numpy.einsum("qK,iL->qiKL", u, I)
        A[:, n, :, :n, :] = tM[:, None, None, None] * numpy.einsum("Kj,qL->qKjL", I, u)
        A[:, n, :, n, :] = (tM / rho)[:, None, None] * I
        return s, F, A, b, c, m, numpy.stack([tM, tC], axis=1)


_FlowLaw = collections.namedtuple("_FlowLaw", "pts g nF load tangent tau")


class FlowResidual(_PointLawResidual):
    """Residual of the stabilised incompressible Navier-Stokes equations on the mapped patch (``IncompressibleFlow`` has the
    formulas): ``u`` the ``Function`` of the nF = nsd + 1 fields (u_1 .. u_nsd, p) on ``EqualOrderSpline(nsd + 1, mesh)``,
    nsd = d = 2 or 3, read at assembly time.  ``law``: an ``IncompressibleFlow`` -- evaluated at the points ON THE DEVICE
    (``tg_flow_points``): the point values, the law's loads and the tangent never leave it -- or any object with such a
    ``host``, whose arrays are uploaded and go through the same loads and the same ``SystemCoefficientForm``.  ``body_force``:
    f per unit mass, ``[npts, nsd]``, a callable of the points, or nsd numbers.

    ``assemble_vector``: values and gradients field by field (``tg_quad_eval``), the metric ``pts.metric``, the law, then nF flux
    loads.  ``tangent()``: the ``SystemCoefficientForm`` of the law's A, b, c, m; ``symmetric`` is False.  For a time integrator:
    ``c_a`` (d acceleration / d velocity), ``a0`` (its history part, a DeviceVector of nsd npts values, or None) and ``dt4`` =
    4 / dt^2 are attributes, zero for the steady problem.  Runs under ``solveNonlinearVariationalProblem`` and inside ``Sum``.
    ``rational``: every field u_h,i / W_h, tested against phi / W_h."""

    _who, _kind, _names, nJ = "FlowResidual", "system", ("(s, F)", "(A, b, c, m)"), 1

    def __init__(self, u, geometry, law, body_force=None, nq=None, rational=False):
        _PointLawResidual.__init__(self, u, geometry, law, "IncompressibleFlow, or an object with host(U, gradU, G, c_a, a0, f, dt4) -> "
                                   "(s, F, A, b, c, m, tau)", isinstance(law, IncompressibleFlow), body_force, nq, rational)
        self.c_a, self.a0, self.dt4 = 0.0, None, 0.0

    def _at(self, u, keeps_u=False):
        other = _PointLawResidual._at(self, u, keeps_u)
        other.c_a, other.a0, other.dt4 = self.c_a, self.a0, self.dt4
        return other

    def _check_space(self, g, nF, who):
        nsd, d = len(self.geometry.cpFuncs) - 1, g.dim()
        if d == 1 or nsd != d:
            raise NotImplementedError("%s: nsd = %d physical directions on a patch of d = %d parametric ones; the flow law is "
                                      "provided for nsd = d = 2 or 3" % (who, nsd, d))
        if nF != nsd + 1:
            raise NotImplementedError("%s: nFields = %d; the flow has nsd + 1 = %d fields (the velocity components, then the "
                                      "pressure)" % (who, nF, nsd + 1))

    def _force(self, pts):
        if self.body_force is None:
            return None
        return _per_points(self, "_fq", pts, lambda: _point_data(self.body_force, pts, (pts.nsd,), self._who + ": body_force"))

    def law(self, V, load=True, tangent=False, tau=False):
        """(points, node grid, nF, (s, F), (A, b, c, m), tau) at the current state as DeviceVectors, None where not asked for"""
        g, nF, pts = self._scope(V, self._who)
        pts, g, nF, Uq, Gq = _system_state(self.geometry, V, self.u, self.nq, self.rational, self._who)
        nsd, npts, fq = pts.nsd, pts.npts, self._force(pts)
        if self.a0 is not None and self.a0.size() != nsd * npts:
            raise ValueError("%s: a0 holds %d values, expected nsd npts = %d" % (self._who, self.a0.size(), nsd * npts))
        if self.device_law:
            s, F, A, b, c, M, t = _dev.flow_points(self.material.params(self.c_a, self.dt4), nsd, Uq, Gq, pts.metric, self.a0, fq,
                                                   load, tangent, tau)
        else:
            un = lambda v, shape: None if v is None else point_unblock(v.get_local(), npts, shape)
            out = self.material.host(un(Uq, (nF,)), un(Gq, (nF, nsd)), un(pts.metric, (nsd, nsd)), c_a=self.c_a,
                                     a0=un(self.a0, (nsd,)), f=un(fq, (nsd,)), dt4=self.dt4)
            sh, Fh, Ah, bh, ch, mh, th = _law_result(out, self._who, "law.host(U, gradU, G, ...)", "(s, F, A, b, c, m, tau)", [
                (npts, nF), (npts, nF, nsd), (npts, nF, nsd, nF, nsd), (npts, nF, nsd, nF), (npts, nF, nF, nsd), (npts, nF, nF), (npts, 2)])
            up = lambda v, shape, perm=None: _dev.DeviceVector(data=point_block(v, npts, shape, perm))
            s, F = (up(sh, (nF,)), up(Fh, (nF, nsd))) if load else (None, None)
            A, b, c, M = (up(Ah, (nF, nsd, nF, nsd), _BLOCK_ORDER), up(bh, (nF, nsd, nF), (0, 2, 1)), up(ch, (nF, nF, nsd)),
                          up(mh, (nF, nF))) if tangent else (None,) * 4
            t = up(th, (2,)) if tau else None
        return _FlowLaw(pts, g, nF, (s, F) if load else None, (A, b, c, M) if tangent else None, t)

    def _law_symmetric(self):
        return False

    def _load_vector(self, V, out, values=None, sigma=1.0):
        pts, nF, npts = out.pts, out.nF, out.pts.npts
        s, F = out.load
        si = [_dev.DeviceVector(npts, zero=False) for _ in range(nF)]
        for i in range(nF):
            _dev.vec_copy_range(si[i], 0, s, i * npts, npts)
        return _field_loads(pts, out.g.num_nodes(), nF, si, F, self.rational)

    def energy(self, V=None):
        raise NotImplementedError("FlowResidual: the flow law derives from no energy")

    def _tangent_form(self, pts, nF, tangent, values=None):
        form = SystemCoefficientForm(self.geometry, *tangent, nq=self.nq, rational=self.rational)
        form._symmetric_hint = False
        return form


# ---- second-derivative point forms (csrc/tg_jet.hip): spline.parametricGrad of the reference and its derivative ------------
class VectorJetCoefficientForm(object):
    """a(u, v) = sum_q wdet_q sum_ij (jet v_i)^T T_ij (jet u_j) on the mapped patch: point data acting on the JETS of trial and
    test functions -- value, first and second derivatives (order 00, 01, 11) with respect to the patch's parametric
    coordinates, ``spline.parametricGrad`` of the reference and its derivative.  nF >= 1 fields on one continuous Q_p node
    grid, dofs field after field; d = 1, 2 and nsd >= d (a surface in space); nF need not equal d or nsd.  The tangent of a
    Kirchhoff-Love shell; its (0, 0) entries alone are a mass term.

    ``T``: ``[npts, nF, nJ, nF, nJ]`` point values T[q, i, alpha, j, beta] (row: test field i, column: trial field j;
    numbered as ``QuadraturePoints``), a callable of the points ``x [npts, nsd]`` returning that, or a DeviceVector with
    T_ij^{alpha beta} at ((i nF + j) nJ^2 + alpha nJ + beta) npts + q.  ``nq`` Gauss points per direction (p + 1 when None).
    ``rational``: every component function phi / W_h.  ``symmetric`` is True only when the bits prove it:
    T[i, alpha, j, beta] == T[j, beta, i, alpha] at every point.  One pass brings all nF^2 blocks to the reference element
    (``tg_jet_transform``), each block is then assembled on the element-coupling pattern (``tg_assemble_jet_blocks``).
    One rank, all rows."""
    _who = "VectorJetCoefficientForm"

    def __init__(self, geometry, T, nq=None, rational=False):
        if geometry is None:
            raise ValueError("%s: point data live on a mapped patch (geometry=...)" % self._who)
        if T is None:
            raise ValueError("%s: no point data" % self._who)
        self.geometry, self.T, self.nq, self.rational = geometry, T, nq, bool(rational)
        self._symmetric_hint = None          # (set by a caller whose law proves the symmetry: ShellResidual)

    def _space(self):
        return self.geometry.V

    def _shape(self, v, nF, nJ):
        """brings what the caller gave to [npts, nF, nJ, nF, nJ]"""
        return v

    def coefficients(self, V):
        """(points, nF, T as a DeviceVector in the block layout, symmetric): computed once per set of points"""
        g, nF, nJ = _point_scope(self.geometry, V, self._who, "jet")
        pts = _vector_points(self.geometry, self.nq, self._who)
        return _per_points(self, "_static", pts, lambda: self._static_coefficients(pts, nF, nJ))

    def _static_coefficients(self, pts, nF, nJ):
        T, sym = _point_data(self.T, pts, (nF, nJ, nF, nJ), self._who, _BLOCK_ORDER, _MAJOR_SWAP, hint=self._symmetric_hint,
                             pre=lambda v: self._shape(v, nF, nJ))
        return pts, nF, T, sym

    @property
    def symmetric(self):
        return self.coefficients(self._space())[3]

    def assemble_block(self, V, i, j, row0=None, row1=None):
        """block (i, j): test field i, trial field j (all rows of the field)"""
        g, nF, nJ = _point_scope(self.geometry, V, self._who, "jet")
        if not (0 <= int(i) < nF and 0 <= int(j) < nF):
            raise ValueError("%s: block (%r, %r) of a %d-field space" % (self._who, i, j, nF))
        _whole_rows(g.num_nodes(), row0, row1, self._who, "patch")
        pts, nF, T, _ = self.coefficients(V)
        each = nJ * nJ * pts.npts
        Tij = _dev.DeviceVector(each, zero=False)
        _dev.vec_copy_range(Tij, 0, T, (int(i) * nF + int(j)) * each, each)
        coef = _dev.jet_transform(pts.verts, pts.p, pts.cp, Tij, 1, nq=pts.nq, rational=self.rational)
        return _dev.assemble_jet_blocks(pts.verts, pts.p, pts.cp, coef, 1, nq=pts.nq)

    def assemble_matrix(self, V, row0=None, row1=None):
        g, nF, nJ = _point_scope(self.geometry, V, self._who, "jet")
        _whole_rows(nF * g.num_nodes(), row0, row1, self._who, "patch")
        pts, nF, T, _ = self.coefficients(V)
        coef = _dev.jet_transform(pts.verts, pts.p, pts.cp, T, nF * nF, nq=pts.nq, rational=self.rational)
        return _dev.assemble_jet_blocks(pts.verts, pts.p, pts.cp, coef, nF, nq=pts.nq)


class JetCoefficientForm(VectorJetCoefficientForm):
    """a(u, v) = sum_q wdet_q (jet v)^T T (jet u) for a scalar unknown: ``VectorJetCoefficientForm`` with nF = 1.  ``T``:
    ``[npts, nJ, nJ]`` (row alpha: test, column beta: trial), a callable of the points returning that, or a DeviceVector
    with T^{alpha beta} at (alpha nJ + beta) npts + q."""
    _who = "JetCoefficientForm"

    def _space(self):
        return self.geometry.V_control

    def _shape(self, v, nF, nJ):
        if nF != 1:
            raise NotImplementedError("JetCoefficientForm: nFields = %d; VectorJetCoefficientForm takes several fields" % nF)
        if v.shape == (nJ, nJ):
            return v.reshape(1, nJ, 1, nJ)
        return v.reshape(v.shape[0], 1, nJ, 1, nJ) if v.ndim == 3 and v.shape[1:] == (nJ, nJ) else v


class VectorJetLoadForm(object):
    """L(v) = sum_q wdet_q sum_i s_i . jet v_i on the space of ``VectorJetCoefficientForm``: ``s`` ``[npts, nF, nJ]`` (value slot
    first, then the first and second parametric derivatives), a callable of the points returning that, nF x nJ numbers, or a
    DeviceVector with s_i^alpha at (i nJ + alpha) npts + q.  The component loads are written field after field
    (``tg_jet_load_transform``, ``tg_quad_load_jet``).  ``rational``: v_i the functions phi / W_h."""
    _who = "VectorJetLoadForm"

    def __init__(self, s, geometry, nq=None, rational=False):
        if geometry is None:
            raise ValueError("%s: point values live on a mapped patch (geometry=...)" % self._who)
        if s is None:
            raise ValueError("%s: no point values" % self._who)
        self.s, self.geometry, self.nq, self.rational = s, geometry, nq, bool(rational)

    def _shape(self, v, nF, nJ):
        return v

    def point_values(self, pts, nF, nJ):
        return _point_data(self.s, pts, (nF, nJ), self._who, pre=lambda v: self._shape(v, nF, nJ))

    def assemble_vector(self, V, row0=None, row1=None):
        g, nF, nJ = _point_scope(self.geometry, V, self._who, "jet")
        _whole_rows(nF * g.num_nodes(), row0, row1, self._who, "patch")
        pts = _vector_points(self.geometry, self.nq, self._who)
        s = _per_points(self, "_static", pts, lambda: self.point_values(pts, nF, nJ))
        st = _dev.jet_load_transform(pts.verts, pts.p, pts.cp, s, nF, nq=pts.nq, rational=self.rational)
        return _dev.quad_load_jet(pts.verts, pts.p, pts.cp, st, nF, nq=pts.nq)


class JetLoadForm(VectorJetLoadForm):
    """L(v) = sum_q wdet_q s . jet v for a scalar space: ``s`` ``[npts, nJ]``, a callable returning that, nJ numbers, or a
    DeviceVector with s^alpha at alpha npts + q."""
    _who = "JetLoadForm"

    def _shape(self, v, nF, nJ):
        if nF != 1:
            raise NotImplementedError("JetLoadForm: nFields = %d; VectorJetLoadForm takes several fields" % nF)
        if v.shape == (nJ,):
            return v.reshape(1, nJ)
        return v.reshape(v.shape[0], 1, nJ) if v.ndim == 2 and v.shape[1] == nJ else v


# ---- Kirchhoff-Love shells: the law on the host (demos/kl-shell-svk of the reference) ------------------------------------
def _cross(a, b):
    return numpy.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                        a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


_KL_SLOT = {(0, 0): 3, (0, 1): 4, (1, 0): 4, (1, 1): 5}            # second-derivative slots of the jet


def _kl_dot(a, b):
    return numpy.einsum("qc,qc->q", a, b)


def _kl_jets(who, Xjet, ujet):
    """the two jets in their common float dtype, after the shape check: (dtype, Xjet, ujet)"""
    Xjet, ujet = numpy.asarray(Xjet), numpy.asarray(ujet)
    dt = numpy.result_type(Xjet.dtype, ujet.dtype).type
    Xjet, ujet = Xjet.astype(dt), ujet.astype(dt)
    npts = Xjet.shape[0]
    if Xjet.shape != (npts, 3, 6) or ujet.shape != (npts, 3, 6):
        raise ValueError("%s: jets of shape [npts, 3, 6] (nsd = 3, d = 2); got %s and %s" % (who, Xjet.shape, ujet.shape))
    return dt, Xjet, ujet


def _kl_normal_floor(Xjet, ujet):
    """mask of the points whose reference or current normal is not defined"""
    X1, X2 = Xjet[:, :, 1], Xjet[:, :, 2]
    x1, x2 = X1 + ujet[:, :, 1], X2 + ujet[:, :, 2]
    nrm = lambda v: numpy.sqrt(numpy.einsum("qc,qc->q", v, v))
    floor = 1e-14 * nrm(X1) * nrm(X2)
    return ~((nrm(_cross(X1, X2)) >= floor) & (nrm(_cross(x1, x2)) >= floor))


def _kl_surface(jet):
    """((x_,0, x_,1), unit normal, |x_,0 x x_,1|, metric [q, 2, 2], curvature x_,ab . a_3 [q, 2, 2]) of a configuration"""
    dot = _kl_dot
    g1, g2 = jet[:, :, 1], jet[:, :, 2]
    n = _cross(g1, g2)
    J = numpy.sqrt(dot(n, n))
    n3 = n / J[:, None]
    met = numpy.stack([numpy.stack([dot(g1, g1), dot(g1, g2)], 1), numpy.stack([dot(g1, g2), dot(g2, g2)], 1)], 1)
    cur = numpy.empty_like(met)
    for (a, b) in ((0, 0), (0, 1), (1, 0), (1, 1)):
        cur[:, a, b] = dot(jet[:, :, _KL_SLOT[(a, b)]], n3)
    return (g1, g2), n3, J, met, cur


def _kl_inverse(m):
    """inverse of symmetric [q, 2, 2] matrices (the entry (0, 1) is read for both off-diagonal places)"""
    det = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 0, 1]
    inv = numpy.empty_like(m)
    inv[:, 0, 0], inv[:, 1, 1], inv[:, 0, 1], inv[:, 1, 0] = m[:, 1, 1] / det, m[:, 0, 0] / det, -m[:, 0, 1] / det, -m[:, 0, 1] / det
    return inv


def _kl_variations(xjet, g, a3, am, nres, mres, quadratic):
    """(s, T) of an energy psi(eps, kappa) per unit reference area at the configuration ``xjet`` (tangents ``g``, normal
    ``a3``, metric ``am``) from its resultants n^ab = d psi / d eps_ab, m^ab = d psi / d kappa_ab and ``quadratic(De, Dk)``,
    the part of T that holds the second derivatives of psi:  T = quadratic + n : D2 eps + m : D2 kappa, with
    De[q, a, b, i, alpha], Dk[q, a, b, i, alpha] the derivatives of eps_ab, kappa_ab with respect to jet(u)_i^alpha."""
    dt = xjet.dtype.type
    npts = xjet.shape[0]
    half = dt(0.5)
    slot, ein, dot = _KL_SLOT, numpy.einsum, _kl_dot
    g1, g2 = g
    # current contravariant basis and Christoffel symbols Gamma^c_ab = x_,ab . a^c
    ai = _kl_inverse(am)
    gup = [ai[:, c, 0, None] * g1 + ai[:, c, 1, None] * g2 for c in range(2)]       # a^c
    # ---- first variation.  delta eps_ab = sym(delta x_,a . x_,b); delta kappa_ab = -(delta x_,ab - Gamma^c_ab delta x_,c) . a_3
    s = numpy.zeros((npts, 3, 6), dtype=dt)
    Gam = numpy.empty((npts, 2, 2, 2), dtype=dt)                   # [q, c, a, b]
    for a in range(2):
        for b in range(2):
            xab = xjet[:, :, slot[(a, b)]]
            for c in range(2):
                Gam[:, c, a, b] = dot(xab, gup[c])
    for a in range(2):
        for b in range(2):
            s[:, :, 1 + a] += nres[:, a, b, None] * g[b]
            s[:, :, slot[(a, b)]] -= mres[:, a, b, None] * a3
            for c in range(2):
                s[:, :, 1 + c] += (mres[:, a, b] * Gam[:, c, a, b])[:, None] * a3
    # ---- second variation
    De = numpy.zeros((npts, 2, 2, 3, 6), dtype=dt)
    Dk = numpy.zeros((npts, 2, 2, 3, 6), dtype=dt)
    for a in range(2):
        for b in range(2):
            De[:, a, b, :, 1 + a] += half * g[b]
            De[:, a, b, :, 1 + b] += half * g[a]
            Dk[:, a, b, :, slot[(a, b)]] -= a3
            for c in range(2):
                Dk[:, a, b, :, 1 + c] += Gam[:, c, a, b, None] * a3
    T = quadratic(De, Dk)
    I3 = numpy.eye(3, dtype=dt)
    for a in range(2):
        for b in range(2):                                         # n^ab delta x_,a . delta x_,b
            T[:, :, 1 + a, :, 1 + b] += nres[:, a, b, None, None] * I3
    # m^ab D2 kappa_ab = -m^ab (w_,ab . D a_3[v] + v_,ab . D a_3[w] + x_,ab . D2 a_3[w, v]) with the variations of the normal
    #   D a_3[v] = -a^c (a_3 . v_,c),      D a^c[v] = -(a^c . v_,d) a^d + a^cd (a_3 . v_,d) a_3
    for a in range(2):
        for b in range(2):
            sl = slot[(a, b)]
            for c in range(2):                                     # -m^ab w_,ab . D a_3[v]: row (k, sl), column (i, 1 + c)
                blk = ein("q,qk,qi->qki", mres[:, a, b], gup[c], a3)
                T[:, :, sl, :, 1 + c] += blk
                T[:, :, 1 + c, :, sl] += blk.transpose(0, 2, 1)
    # with M = m^ab x_,ab:  -M . D2 a_3[w, v] = (M . D a^c[v]) (a_3 . w_,c) + (M . a^c) (D a_3[v] . w_,c)
    #   = -(M . a^d)(a_3 . w_,c)(a^c . v_,d) + a^cd (M . a_3)(a_3 . w_,c)(a_3 . v_,d) - (M . a^c)(a^d . w_,c)(a_3 . v_,d)
    # row: w, field i, slot 1 + c; column: v, field j, slot 1 + d
    Mv = sum(mres[:, a, b, None] * xjet[:, :, slot[(a, b)]] for a in range(2) for b in range(2))
    M3 = dot(Mv, a3)
    for c in range(2):
        for d_ in range(2):
            Mac, Mad = dot(Mv, gup[c]), dot(Mv, gup[d_])
            T[:, :, 1 + c, :, 1 + d_] += -ein("q,qi,qj->qij", Mad, a3, gup[c]) + ein("q,qi,qj->qij", ai[:, c, d_] * M3, a3, a3) \
                - ein("q,qi,qj->qij", Mac, gup[d_], a3)
    return s, T


class KirchhoffLoveSVK(object):
    """St. Venant-Kirchhoff Kirchhoff-Love shell of ``thickness`` h (demos/kl-shell-svk/dynamic-tspline.py:135-212 of the
    reference), d = 2, nsd = nF = 3.  With the reference surface X(xi) and x = X + u:
      A_ab = X_,a . X_,b,  A_3 = X_,1 x X_,2 / |.|,  B_ab = X_,ab . A_3;  a_ab, a_3, b_ab likewise from x;
      eps_ab = (a_ab - A_ab)/2,  kappa_ab = B_ab - b_ab,
      C^abcd = E/(1 - nu^2) [nu A^ab A^cd + (1 - nu)/2 (A^ac A^bd + A^ad A^bc)],
      psi = h/2 eps:C:eps + h^3/24 kappa:C:kappa   per unit reference area.
    ``host(Xjet, ujet)``: jets ``[npts, 3, 6]`` (value | ,0 ,1 | ,00 ,01 ,11) of any float dtype -> (psi [npts],
    s = d psi / d jet(u) [npts, 3, 6] with the value slot zero, T = d^2 psi / d jet(u)^2 [npts, 3, 6, 3, 6]), from closed
    forms: the first and second variations of a_3, and delta b_ab = (delta x_,ab - Gamma^c_ab delta x_,c) . a_3.
    Degenerate points (|X_,1 x X_,2| or |x_,1 x x_,2| below 1e-14 |X_,1| |X_,2|) raise ``RuntimeError`` naming their number."""
    kind = 0
    inadmissible = "with a degenerate surface normal"

    def __init__(self, E, nu, thickness):
        self.E, self.nu, self.thickness = float(E), float(nu), float(thickness)

    def params(self):
        """the parameters of ``tg_shell_points`` for this kind"""
        return (self.E, self.nu, self.thickness)

    @staticmethod
    def degenerate(Xjet, ujet):
        """mask of the points whose reference or current normal is not defined"""
        return _kl_normal_floor(Xjet, ujet)

    def host(self, Xjet, ujet):
        dt, Xjet, ujet = _kl_jets("KirchhoffLoveSVK", Xjet, ujet)
        bad = self.degenerate(Xjet, ujet)
        if numpy.any(bad):
            raise RuntimeError("KirchhoffLoveSVK: %d points with a degenerate surface normal" % int(numpy.sum(bad)))
        E, nu, h = dt(self.E), dt(self.nu), dt(self.thickness)
        half, one = dt(0.5), dt(1)
        ein = numpy.einsum
        _, _, _, Am, Bm = _kl_surface(Xjet)
        xjet = Xjet + ujet
        g, a3, _, am, bm = _kl_surface(xjet)
        # contravariant reference metric and the material tensor
        Ai = _kl_inverse(Am)
        Cm = (E / (one - nu * nu)) * (nu * ein("qab,qcd->qabcd", Ai, Ai) +
                                      half * (one - nu) * (ein("qac,qbd->qabcd", Ai, Ai) + ein("qad,qbc->qabcd", Ai, Ai)))
        eps, kap = half * (am - Am), Bm - bm
        nres = h * ein("qabcd,qcd->qab", Cm, eps)                     # membrane forces  n^ab
        mres = (h * h * h / dt(12)) * ein("qabcd,qcd->qab", Cm, kap)  # bending moments  m^ab
        psi = half * ein("qab,qab->q", nres, eps) + half * ein("qab,qab->q", mres, kap)
        # psi = f(eps(jet), kappa(jet)):  T = De^T (h C) De + Dk^T (h^3/12 C) Dk + n : D2 eps + m : D2 kappa
        s, T = _kl_variations(xjet, g, a3, am, nres, mres, lambda De, Dk:
                              h * ein("qabiA,qabcd,qcdjB->qiAjB", De, Cm, De) + (h * h * h / dt(12)) * ein("qabiA,qabcd,qcdjB->qiAjB", Dk, Cm, Dk))
        return psi, s, T


class KirchhoffLoveHyper(object):
    """Incompressible neo-Hookean Kirchhoff-Love shell of ``thickness`` h, the energy integrated through the thickness with
    the ``n_thickness``-point rule of ``getQuadRuleInterval`` (demos/kl-shell-hyper/kl-hyper.py:98-215 of the reference),
    d = 2, nsd = nF = 3.  With A, B, a, b the metrics and curvatures of ``KirchhoffLoveSVK``, at the thickness point xi:
      Gm = A - 2 xi B,  gm = a - 2 xi b                        the truncated metrics,
      G_b = A_b + xi d_b A_3 = (I - xi B A^-1)_bd A_d          (Weingarten),   G^a = (Gm^-1)_ab G_b,
      e_0, e_1: Gram-Schmidt on G_0, G_1,   R_ia = e_i . G^a,   C_2D = I + Chat,  Chat = R (gm - Gm) R^T,
      psi(xi) = mu/2 (tr C_2D + 1 / det C_2D - 3) = mu/2 (tr Chat - t / (1 + t)),   t = tr Chat + det Chat
    (the multiplier term of the demo vanishes: C_22 = 1 / det C_2D makes J = 1), psi = sum_k w_k psi(xi_k) per unit
    reference area.  gm - Gm = 2 (eps + xi kappa) is formed from the strains, so small strains do not cancel.
    Chat is affine in (eps, kappa) and R depends on the reference alone:
      d psi(xi) / d Chat = mu/2 (t (2 + t) I - adj Chat) / (1 + t)^2,
      d2 psi(xi) / d Chat2 = mu/2 (2 adj C (x) adj C / (1 + t)^3 - L / (1 + t)^2),   L = d adj C / d C,
    pulled back by R to F = d psi(xi) / d gm and H; n = 2 sum w F, m = 2 sum w xi F, D_ee = 4 sum w H, D_ek = 4 sum w xi H,
    D_kk = 4 sum w xi^2 H, and s, T follow with the kinematic variations of ``KirchhoffLoveSVK``.
    ``host(Xjet, ujet)`` as there.  ``degenerate``: the points that fail the normal floors of ``KirchhoffLoveSVK`` or have
    det Gm(xi_k) <= 0 or det C_2D(xi_k) <= 0 at some thickness point."""
    kind = 1
    inadmissible = "with a degenerate surface normal, or with det Gm <= 0 or det C_2D <= 0 at a thickness point"

    def __init__(self, mu, thickness, n_thickness=4):
        from .common import getQuadRuleInterval
        if n_thickness not in (1, 2, 3, 4):
            raise ValueError("KirchhoffLoveHyper: n_thickness = %r; rules of 1 to 4 thickness points are provided" % (n_thickness,))
        self.mu, self.thickness, self.n_thickness = float(mu), float(thickness), int(n_thickness)
        self.rule = getQuadRuleInterval(self.n_thickness, self.thickness)

    def params(self):
        """the parameters of ``tg_shell_points`` for this kind"""
        return (self.mu, self.thickness, float(self.n_thickness))

    @staticmethod
    def _frame(Am, Bm, Ai, xi):
        """(R [q, 2, 2], det Gm) at the thickness coordinate xi, from the reference surface alone"""
        ein = numpy.einsum
        one = Am.dtype.type(1)
        Q = -xi * ein("qbc,qcd->qbd", Bm, Ai)
        Q[:, 0, 0] += one
        Q[:, 1, 1] += one
        Gg = ein("qbc,qcd,qed->qbe", Q, Am, Q)                          # G_b . G_e
        Gm = Am - (xi + xi) * Bm
        detGm = Gm[:, 0, 0] * Gm[:, 1, 1] - Gm[:, 0, 1] * Gm[:, 0, 1]
        l0 = numpy.sqrt(Gg[:, 0, 0])
        Eg = numpy.zeros_like(Am)                                       # e_i . G_b: upper triangular
        Eg[:, 0, 0], Eg[:, 0, 1] = l0, Gg[:, 0, 1] / l0
        Eg[:, 1, 1] = numpy.sqrt((Gg[:, 0, 0] * Gg[:, 1, 1] - Gg[:, 0, 1] * Gg[:, 0, 1]) / Gg[:, 0, 0])
        return ein("qib,qba->qia", Eg, _kl_inverse(Gm)), detGm

    def _through(self, dt, Am, Bm, eps, kap):
        """yields (xi, w, R, det Gm, Chat, t) per thickness point"""
        Ai = _kl_inverse(Am)
        for xi, w in zip(*self.rule):
            xi, w = dt(xi), dt(w)
            R, detGm = self._frame(Am, Bm, Ai, xi)
            Ch = numpy.einsum("qia,qab,qjb->qij", R, dt(2) * (eps + xi * kap), R)
            tr = Ch[:, 0, 0] + Ch[:, 1, 1]
            t = tr + (Ch[:, 0, 0] * Ch[:, 1, 1] - Ch[:, 0, 1] * Ch[:, 0, 1])
            yield xi, w, R, detGm, Ch, tr, t

    def degenerate(self, Xjet, ujet):
        """mask of the inadmissible points"""
        dt, Xjet, ujet = _kl_jets("KirchhoffLoveHyper", Xjet, ujet)
        bad = _kl_normal_floor(Xjet, ujet)
        with numpy.errstate(all="ignore"):
            _, _, _, Am, Bm = _kl_surface(Xjet)
            _, _, _, am, bm = _kl_surface(Xjet + ujet)
            for _, _, _, detGm, _, _, t in self._through(dt, Am, Bm, dt(0.5) * (am - Am), Bm - bm):
                bad = bad | ~(detGm > 0) | ~(dt(1) + t > 0)
        return bad

    def host(self, Xjet, ujet):
        dt, Xjet, ujet = _kl_jets("KirchhoffLoveHyper", Xjet, ujet)
        bad = self.degenerate(Xjet, ujet)
        if numpy.any(bad):
            raise RuntimeError("KirchhoffLoveHyper: %d inadmissible points (a degenerate surface normal, or det Gm <= 0 or "
                               "det C_2D <= 0 at a thickness point)" % int(numpy.sum(bad)))
        npts = Xjet.shape[0]
        half, one, two, hmu = dt(0.5), dt(1), dt(2), dt(0.5) * dt(self.mu)
        ein = numpy.einsum
        _, _, _, Am, Bm = _kl_surface(Xjet)
        xjet = Xjet + ujet
        g, a3, _, am, bm = _kl_surface(xjet)
        eps, kap = half * (am - Am), Bm - bm
        I2 = numpy.eye(2, dtype=dt)
        # L = d adj C / d C of a symmetric 2 x 2 matrix: adj C = tr(C) I - C
        Lh = ein("ij,kl->ijkl", I2, I2) - half * (ein("ik,jl->ijkl", I2, I2) + ein("il,jk->ijkl", I2, I2))
        psi = numpy.zeros(npts, dtype=dt)
        nres, mres = numpy.zeros((npts, 2, 2), dtype=dt), numpy.zeros((npts, 2, 2), dtype=dt)
        Dee, Dek, Dkk = (numpy.zeros((npts, 2, 2, 2, 2), dtype=dt) for _ in range(3))
        for xi, w, R, _, Ch, tr, t in self._through(dt, Am, Bm, eps, kap):
            delta = one + t
            psi += w * hmu * (tr - t / delta)
            adjh = numpy.empty_like(Ch)
            adjh[:, 0, 0], adjh[:, 1, 1], adjh[:, 0, 1], adjh[:, 1, 0] = Ch[:, 1, 1], Ch[:, 0, 0], -Ch[:, 0, 1], -Ch[:, 0, 1]
            Fh = (hmu / (delta * delta))[:, None, None] * ((t * (two + t))[:, None, None] * I2 - adjh)
            adjC = adjh + I2
            Hh = (two * hmu / (delta * delta * delta))[:, None, None, None, None] * ein("qij,qkl->qijkl", adjC, adjC) \
                - (hmu / (delta * delta))[:, None, None, None, None] * Lh
            F = ein("qia,qij,qjb->qab", R, Fh, R)
            H = ein("qkc,qld,qabkl->qabcd", R, R, ein("qia,qjb,qijkl->qabkl", R, R, Hh))
            nres += (two * w) * F
            mres += (two * w * xi) * F
            Dee += (dt(4) * w) * H
            Dek += (dt(4) * w * xi) * H
            Dkk += (dt(4) * w * xi * xi) * H
        def quadratic(De, Dk):
            """De^T D_ee De + De^T D_ek Dk + Dk^T D_ek^T De + Dk^T D_kk Dk, through d n / d jet and d m / d jet"""
            dn = ein("qabcd,qcdjB->qabjB", Dee, De) + ein("qabcd,qcdjB->qabjB", Dek, Dk)
            dm = ein("qcdab,qcdjB->qabjB", Dek, De) + ein("qabcd,qcdjB->qabjB", Dkk, Dk)
            return ein("qabiA,qabjB->qiAjB", De, dn) + ein("qabiA,qabjB->qiAjB", Dk, dm)
        s, T = _kl_variations(xjet, g, a3, am, nres, mres, quadratic)
        return psi, s, T


def shell_pressure_host(pressure, Xjet, ujet):
    """The follower pressure of demos/kl-shell-hyper/kl-hyper.py:231 per unit reference area, dWext = -P sqrt(det a / det A)
    a_3 . v = -P (x_,1 x x_,2) . v / |X_,1 x X_,2|: (s, T) of the jets [npts, 3, 6] in their dtype -- s in the value slot, T in
    the (value, first-derivative) entries alone, without a transpose: the tangent of a follower load is not symmetric."""
    dt, Xjet, ujet = _kl_jets("shell_pressure_host", Xjet, ujet)
    npts = Xjet.shape[0]
    xjet = Xjet + ujet
    X1, X2, x1, x2 = Xjet[:, :, 1], Xjet[:, :, 2], xjet[:, :, 1], xjet[:, :, 2]
    N = _cross(X1, X2)
    c = -dt(pressure) / numpy.sqrt(_kl_dot(N, N))
    s = numpy.zeros((npts, 3, 6), dtype=dt)
    T = numpy.zeros((npts, 3, 6, 3, 6), dtype=dt)
    s[:, :, 0] = c[:, None] * _cross(x1, x2)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3           # eps_ijk = +1, eps_ikj = -1
        # d (x_,1 x x_,2)_i = eps_ijk (dx_,1j x_,2k + x_,1j dx_,2k)
        T[:, i, 0, j, 1] += c * x2[:, k]
        T[:, i, 0, k, 1] -= c * x2[:, j]
        T[:, i, 0, k, 2] += c * x1[:, j]
        T[:, i, 0, j, 2] -= c * x1[:, k]
    return s, T


_ShellJets = collections.namedtuple("_ShellJets", "pts g Xjet ujet")
_ShellLaw = collections.namedtuple("_ShellLaw", "pts g load tangent psi")


class ShellResidual(_PointLawResidual):
    """Residual of a Kirchhoff-Love shell on the mapped patch, R(v) = D psi[v] - f . v per unit reference area: what
    ``derivative(psi*spline.dx, u)`` of the reference gives for the energy of demos/kl-shell-svk.  The reference surface is the
    patch (d = 2, nsd = 3); ``u`` the displacement ``Function`` on nF = 3 fields of its scalar space, read at assembly time.

    ``material``: ``KirchhoffLoveSVK`` or ``KirchhoffLoveHyper`` -- evaluated at the points ON THE DEVICE (``tg_shell_points``
    with the material's ``kind`` and ``params()``): the jets, s and the 324 npts tangent values never leave it;
    ``device_law=False`` sends it through its ``host`` method instead -- or any object with
    ``host(Xjet, ujet) -> (psi, s, T)``, a host law whose arrays are uploaded and go through the same transform and
    assembly.  ``assemble_vector`` evaluates the jets of the geometry and of u (``tg_quad_geometry_jet``, ``tg_quad_jet``),
    calls the law, and returns the jet load of s minus the load of ``body_force`` (a value-slot entry of a
    ``VectorJetLoadForm``: ``[npts, 3]``, a callable of the points, or 3 numbers; per unit reference area).
    ``pressure``: a follower pressure P, dWext = -P sqrt(det a / det A) a_3 . v (demos/kl-shell-hyper/kl-hyper.py:231): a
    number, or a callable without arguments read at every assembly (``lambda: P * stepper.t`` follows a ``LoadStepper``); its
    load and its tangent are added to the law's outputs at the points (``tg_shell_pressure_points``; in numpy on the host
    route).  ``tangent()``: the ``VectorJetCoefficientForm`` of T; ``symmetric`` True for the two built-in laws (T derives from
    an energy) unless there is a pressure -- a follower load has no potential, the direct solver then takes the LU -- and for
    another host law what the bits of the last assembled tangent prove.  ``energy(V)`` = sum_q wdet_q psi_q, the strain
    energy.  Inadmissible points -- a degenerate normal (|X_,1 x X_,2| or |x_,1 x x_,2| below 1e-14 |X_,1| |X_,2|), for
    ``KirchhoffLoveHyper`` also det Gm <= 0 or det C_2D <= 0 at a thickness point; the material's ``degenerate`` on the host
    route -- raise ``RuntimeError`` naming their number.  ``rational``: u_i = u_h,i / W_h, tested against phi / W_h."""

    _who, _kind, _names, nJ = "ShellResidual", "jet", ("s", "T"), 6

    def __init__(self, u, geometry, material, body_force=None, nq=None, rational=False, device_law=True, pressure=None):
        # a law of the device: the material names its kind, its parameters and its inadmissible points
        builtin = getattr(material, "kind", None) in _dev.SHELL_KINDS.values() and callable(getattr(material, "params", None))
        _PointLawResidual.__init__(self, u, geometry, material, "KirchhoffLoveSVK, KirchhoffLoveHyper, or an object with "
                                   "host(Xjet, ujet) -> (psi, s, T)", builtin, body_force, nq, rational, device_law)
        self.pressure = pressure if pressure is None or callable(pressure) else float(pressure)
        self._load = None
        if body_force is not None:
            self._load = VectorJetLoadForm(self._force_jets, geometry, nq=nq, rational=rational)

    def _arguments(self):
        return dict(_PointLawResidual._arguments(self), device_law=self.device_law, pressure=self.pressure)

    def _pressure(self):
        """the follower pressure now: a number, or None"""
        return float(self.pressure()) if callable(self.pressure) else self.pressure

    def _refuse(self, nbad):
        if nbad > 0:
            raise RuntimeError("ShellResidual: %d quadrature points %s" % (nbad, getattr(
                self.material, "inadmissible", KirchhoffLoveSVK.inadmissible)))

    def _force_jets(self, x):
        f = self.body_force
        s = numpy.zeros((x.shape[0], 3, 6))
        s[:, :, 0] = point_array(f(x) if callable(f) else f, x.shape[0], (3,), "ShellResidual: body_force")
        return s

    def _check_space(self, g, nF, who):
        nsd = len(self.geometry.cpFuncs) - 1
        if g.dim() != 2 or nsd != 3 or nF != 3:
            raise NotImplementedError("%s: a shell is a surface in space with a displacement of three fields (d = %d, nsd = %d, "
                                      "nFields = %d)" % (who, g.dim(), nsd, nF))

    def jets(self, V):
        """(points, node grid, Xjet, ujet): the jets of the reference surface and of the three displacement fields as
        DeviceVectors of 18 npts values (component alpha of coordinate / field c at (6 c + alpha) npts + q)"""
        g, nF, pts = self._scope(V, self._who)
        uv = _nodal_vector(self.u, nF, g.num_nodes(), self._who)
        X = _per_points(self, "_Xjet", pts, lambda: _dev.quad_geometry_jet(pts.verts, pts.p, pts.cp, nq=pts.nq))
        jet = lambda ui: _dev.quad_jet(pts.verts, pts.p, pts.cp, ui, nq=pts.nq, rational=self.rational)
        U = _field_by_field(uv, nF, g.num_nodes(), jet, self.nJ * pts.npts)
        if self._keeps_u:                       # the value slots of the jets
            self._u_points = U
        return _ShellJets(pts, g, X, U)

    def law(self, V, load=True, tangent=False, energy=False):
        """(points, node grid, s, T, psi) at the current state, as DeviceVectors in the layouts of ``tg_jet_load_transform``
        and ``tg_jet_transform`` (None where not asked for)"""
        at = _ShellJets(*self.jets(V))
        return _ShellLaw(at.pts, at.g, *self._law(at, load, tangent, energy))

    def _device_law(self, at, load, tangent, energy):
        m, P = self.material, self._pressure()
        s, T, psi, nbad = _dev.shell_law_points(m.kind, m.params(), at.Xjet, at.ujet, load, tangent, energy)
        self._refuse(nbad)
        if P is not None and (load or tangent):
            _dev.shell_pressure_points(P, at.Xjet, at.ujet, s, T)
        return s, T, psi

    def _host_law(self, at, loads):
        npts, P = at.pts.npts, self._pressure()
        Xh, Uh = point_unblock(at.Xjet.get_local(), npts, (3, 6)), point_unblock(at.ujet.get_local(), npts, (3, 6))
        self._refuse(int(numpy.sum(getattr(self.material, "degenerate", KirchhoffLoveSVK.degenerate)(Xh, Uh))))
        psih, sh, Th = _law_result(self.material.host(Xh, Uh), self._who, "material.host(Xjet, ujet)", "(psi, s, T)",
                                   [(npts,), (npts, 3, 6), (npts, 3, 6, 3, 6)])
        if P is not None and loads:
            sp, Tp = shell_pressure_host(P, Xh, Uh)
            sh, Th = sh + sp, Th + Tp
        return sh, Th, psih, (3, 6)

    def _law_symmetric(self):
        return _PointLawResidual._law_symmetric(self) and self.pressure is None      # a follower load has no potential

    def _load_vector(self, V, out, values=None, sigma=1.0):
        """the jet load of s minus ``sigma`` times the load of f, which is assembled by itself (``values`` are the value
        slots of s: there is nothing to put back)"""
        r = VectorJetLoadForm(out.load, self.geometry, nq=self.nq, rational=self.rational).assemble_vector(V)
        if self._load is not None:
            r.axpy(-sigma, self._load.assemble_vector(V))
        return r

    # -- the value slots: they sit inside s and T, at stride nJ = 6, so the point kernel scales s itself (sigma = 1 / alpha_f)
    def _value_load(self, out):
        return out.load

    def _slot_scaling(self, af, m_u, k):
        return _SlotScaling((1.0 / af, m_u, 1.0, 0.0, k / af, 0.0, 0.0), 1.0 / af, None)

    def _value_tangent(self, pts, nF, tangent=None):
        return tangent if tangent is not None else _dev.DeviceVector(nF * nF * 36 * pts.npts)

    def _tangent_form(self, pts, nF, tangent, values=None):
        """the ``VectorJetCoefficientForm`` of T, or of the ``values`` of ``_value_tangent``: T with its value-value entries"""
        return VectorJetCoefficientForm(self.geometry, tangent if values is None else values, nq=self.nq, rational=self.rational)


# ---- structural dynamics (csrc/tg_dynamics.hip): inertia, mass damping and a rigid plane at the points ----------------------
class PlanePenalty(object):
    """The rigid half-space n . x >= ``offset`` enforced by a penalty: with the gap g = offset - n . x of a material point at
    x = X + u and g+ = max(g, 0), the energy is stiffness/2 g+^2 per unit reference measure, the force on the body
    stiffness g+ n (``contactForce`` of demos/kl-shell-svk/dynamic-tspline.py is n = e_3, offset = 0).  ``normal`` is
    normalised on construction, so ``offset`` is the signed distance of the plane from the origin along it."""

    def __init__(self, normal, offset, stiffness):
        n = numpy.asarray(normal, dtype=numpy.float64).ravel()
        length = float(numpy.sqrt(numpy.sum(n * n))) if n.size in (2, 3) else 0.0
        if not (length > 0.0 and numpy.isfinite(length)):
            raise ValueError("PlanePenalty: normal = %r; two or three numbers that are not all zero" % (normal,))
        if not float(stiffness) > 0.0:
            raise ValueError("PlanePenalty: stiffness = %r must be positive" % (stiffness,))
        self.normal, self.offset, self.stiffness = n / length, float(offset), float(stiffness)

    def plane(self):
        """(n[0..nsd), offset): the plane as ``device.point_dynamics`` takes it"""
        return tuple(float(v) for v in self.normal) + (self.offset,)

    def gap(self, x):
        """g = offset - n . x at the positions ``x [npts, nsd]`` (host)"""
        x = numpy.asarray(x)
        return x.dtype.type(self.offset) - x @ self.normal.astype(x.dtype)


class DynamicResidual(object):
    """Residual of nonlinear structural dynamics on the mapped patch, the formulation of
    demos/kl-shell-svk/dynamic-tspline.py:100-293 of the reference:

        R(y)[v] = int rho (yddot_alpha + a_M ydot_alpha) . v + D psi(y_alpha)[v] - loads(y_alpha, t_alpha) . v
                      - k g+(X + y_alpha) n . v
        dR/dy   = rho (c_a + a_M c_v) M + alpha_f [K_law + K_pressure + k [g > 0] n (x) n](y_alpha)

    ``static``: a ``ShellResidual`` or a ``HyperelasticResidual`` whose ``u`` is the Function ``integrator`` solves for; its
    law, pressure and body force are evaluated at the alpha-level state y_alpha by the same residual at another u: one of the
    same class built from the arguments ``static`` holds at this moment, which reads the alpha-level vector, keeps the point
    values of u of its last evaluation and shares no cache with the object handed in -- that one is neither modified nor
    read again.  All that is asked of the law is where the value slots of its point data live: inside s and T at stride 6
    (a shell), or in vectors of their own next to P and A (a solid).  A ``pressure`` callable is read at every assembly and
    finds the time of the loads in ``dyn.t_alpha``; a ``body_force`` callable is a function of the points alone, evaluated
    once per set of points by the static classes and not again.
    ``integrator``: a second-order ``GeneralizedAlphaIntegrator``, or a ``BackwardEulerIntegrator`` with two old functions
    (alpha_f = 1, its own ``xdot()`` and ``xddot()``).  ``density``: mass per unit reference measure (rho h of a shell, rho of
    a solid); ``mass_damping`` = a_M; ``contact``: a ``PlanePenalty`` or None.  c_a and c_v, the coefficients of y in
    yddot_alpha and ydot_alpha, are read from the integrator's ``LinearCombination.split``.

    DIVISION BY alpha_f: ``assemble_vector`` returns R / alpha_f and ``tangent()`` the form of (dR/dy) / alpha_f, so that the
    tangent values of the law are used as the law kernel wrote them (y_alpha moves by alpha_f dy): only the nF^2 value-value
    entries of the point tangent and the value-slot loads are modified.  Newton iterates and RELATIVE norms are those of the
    reference's forms; absolute norms are 1 / alpha_f times the reference's.  The factor is ``dyn.scale`` = alpha_f.

    Inertia is affine in y_alpha: rho (yddot_alpha + a_M ydot_alpha) / alpha_f = m_u y_alpha + w with w a combination of the
    old state.  w is brought to the points once per time step (keyed on ``integrator.t``; ``invalidate()`` after the old state
    was changed by hand); after that an assembly runs the point evaluations of ``static`` and one ``tg_point_dynamics`` --
    between the law and the load / tangent assembly, on the value slots the law kernel left on the device.

    ``tangent()``: ``assemble_matrix``, ``assemble_block``, ``geometry``; ``symmetric`` that of the static tangent (inertia
    and the penalty are symmetric, a follower pressure gives False).  ``energy()``: {"strain", "kinetic", "contact", "total"}
    at the current level ``integrator.x`` with ``xdot()`` for the velocity.  ``active_points()``: the number of points in
    contact at the last assembly.  One rank, all rows, the order of the node grid."""

    def __init__(self, static, integrator, density, mass_damping=0.0, contact=None):
        from . import timeIntegration as _ti
        who = "DynamicResidual"
        if not isinstance(static, _PointLawResidual):
            raise NotImplementedError("%s: static = %r; a ShellResidual or a HyperelasticResidual carries the law" % (who, static))
        if isinstance(integrator, _ti.GeneralizedAlphaIntegrator):
            self._gen_alpha = True
        elif isinstance(integrator, _ti.BackwardEulerIntegrator):
            self._gen_alpha = False
        else:
            raise ValueError("%s: integrator = %r; a GeneralizedAlphaIntegrator or a BackwardEulerIntegrator" % (who, integrator))
        if integrator.systemOrder != 2:
            raise ValueError("%s: a first-order integrator has no acceleration; structural dynamics is a second-order system "
                             "(oldFunctions = [y_old, ydot_old%s])" % (who, ", yddot_old" if self._gen_alpha else ""))
        if _ti._vec_of(static.u) is not _ti._vec_of(integrator.x):
            raise ValueError("%s: static.u is not the Function the integrator solves for (integrator.x)" % who)
        if not float(density) > 0.0:
            raise ValueError("%s: density = %r must be positive (mass per unit reference measure)" % (who, density))
        if contact is not None and not isinstance(contact, PlanePenalty):
            raise ValueError("%s: contact = %r; a PlanePenalty or None" % (who, contact))
        nsd = len(static.geometry.cpFuncs) - 1
        if contact is not None and contact.normal.size != nsd:
            raise ValueError("%s: the plane's normal has %d components, the patch lies in %d dimensions" % (who, contact.normal.size, nsd))
        self.static, self.integrator, self.geometry = static, integrator, static.geometry
        self.density, self.mass_damping, self.contact = float(density), float(mass_damping), contact
        self.rational, self.nq = static.rational, static.nq
        self.scale = float(integrator.ALPHA_F) if self._gen_alpha else 1.0
        self._ti = _ti
        self._law = static._at(None, keeps_u=True)      # reads y_alpha
        self._now = static._at(integrator.x)            # reads the current level (energy)
        self._ya, self._w, self._w_key, self._nactive = None, None, None, 0

    # -- the coefficients of a step
    @property
    def t_alpha(self):
        """the time the loads are evaluated at: t_{n+1} - (1 - alpha_f) DELTA_T"""
        it = self.integrator
        return it.t - (1.0 - self.scale) * float(it.DELTA_T)

    def _inertia(self):
        """(c_M, the rest): rho-free yddot_alpha + a_M ydot_alpha = c_M y + rest, c_M = c_a + a_M c_v"""
        it = self.integrator
        if self._gen_alpha:
            e = it.xddot_alpha() + self.mass_damping * it.xdot_alpha()
        else:
            e = it.xddot() + self.mass_damping * it.xdot()
        return e.split(it.x)

    def coefficients(self):
        """{"c_a", "c_v", "c_M", "m_u", "t_m"}: c_a, c_v the coefficients of y in yddot_alpha and ydot_alpha, c_M = c_a + a_M c_v,
        m_u = rho c_M / alpha_f^2 what multiplies y_alpha in R / alpha_f, t_m = rho c_M / alpha_f what multiplies the mass
        matrix in (dR/dy) / alpha_f"""
        it, af = self.integrator, self.scale
        c_a = (it.xddot_alpha() if self._gen_alpha else it.xddot()).coefficient(it.x)
        c_v = (it.xdot_alpha() if self._gen_alpha else it.xdot()).coefficient(it.x)
        c_M = self._inertia()[0]
        return {"c_a": c_a, "c_v": c_v, "c_M": c_M, "m_u": self.density * c_M / (af * af), "t_m": self.density * c_M / af}

    def invalidate(self):
        """forget the old-state part of the inertia at the points (the old functions were changed without ``advance()``)"""
        self._w_key = None

    def _scope(self, V, row0, row1, block=False):
        return self._law._scope(V, "DynamicResidual", row0, row1, block)

    def _state(self, g, nF, pts):
        """y_alpha into the vector the law reads (one ``tg_vec_lincomb``), and, once per step, w at the points"""
        it, ti, af = self.integrator, self._ti, self.scale
        size = nF * g.num_nodes()
        if self._ya is None or self._ya.size() != size:
            self._ya = _dev.DeviceVector(size, zero=False)
            self._law.u = self._ya
        if ti._vec_of(it.x).size() != size:
            raise ValueError("DynamicResidual: the unknown holds %d nodal values, the space has %d fields of %d"
                             % (ti._vec_of(it.x).size(), nF, g.num_nodes()))
        ti.x_alpha(af, it.x, it.x_old).evaluate(out=self._ya)
        key = (it.t, id(pts))
        if self._w_key != key:
            c_M, rest = self._inertia()
            expr = (self.density / af) * (rest - (c_M * (1.0 - af) / af) * ti.LinearCombination.of(it.x_old))
            self._w = _values_at_points(pts, expr.evaluate(out=_dev.DeviceVector(size, zero=False)), nF, g.num_nodes(), self.rational)
            self._w_key, self._w_pts = key, pts
        return self._w

    def _plane(self):
        return self.contact.plane() if self.contact is not None else None

    def _stiffness(self):
        return self.contact.stiffness if self.contact is not None else 0.0

    def _dynamics(self, pts, nF, coef, w=None, s=None, T=None):
        """the one launch of an assembly, on the value slots of the law and the point values of u it kept; the count of
        active points is read back only with a plane"""
        law = self._law
        n = _dev.point_dynamics(nF, law.nJ, pts.npts, coef, self._plane(), pts.x_device if self.contact is not None else None,
                                law._u_points, w, s, T, None, count=self.contact is not None)
        self._nactive = n if n is not None else 0

    def active_points(self):
        """the number of quadrature points in contact (g > 0) at the last assembly"""
        return self._nactive

    def assemble_vector(self, V, row0=None, row1=None):
        g, nF, pts = self._scope(V, row0, row1)
        w = self._state(g, nF, pts)
        law, c = self._law, self.coefficients()
        out = law.law(V)
        s = law._value_load(out)
        scaling = law._slot_scaling(self.scale, c["m_u"], self._stiffness())
        self._dynamics(pts, nF, scaling.coef, w=w, s=s)
        r = law._load_vector(V, out, s, scaling.sigma)
        return r if scaling.after is None else _dev.vec_lincomb(r, [scaling.after], [r])

    def energy(self, V=None, y=None, ydot=None):
        """{"strain", "kinetic", "contact", "total"} at the current level: sum_q wdet psi(y), rho/2 |ydot|^2 with ``xdot()`` of the
        integrator, k/2 g+(X + y)^2; the last two through ``e_out`` of ``tg_point_dynamics``.  ``y`` / ``ydot``: another
        state (Functions or nodal vectors) in the place of ``integrator.x`` and ``xdot()`` -- after ``advance()`` the formulas
        of the integrator no longer describe the step just taken, the old functions do."""
        it, ti = self.integrator, self._ti
        if V is None:
            V = it.x.function_space()
        g, nF, pts = self._scope(V, None, None)
        at = lambda nodal: _values_at_points(pts, nodal, nF, g.num_nodes(), self.rational)
        self._now.u = it.x if y is None else y
        out = {"strain": float(self._now.energy(V))}
        vq = at(it.xdot().evaluate() if ydot is None else ti._vec_of(ydot))
        e = _dev.DeviceVector(pts.npts, zero=False)
        _dev.point_dynamics(nF, 1, pts.npts, (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, self.density), w=vq, e=e)
        out["kinetic"] = float(pts.weights.inner(e))
        out["contact"] = 0.0
        if self.contact is not None:
            uq = at(ti._vec_of(self._now.u))
            _dev.point_dynamics(nF, 1, pts.npts, (1.0, 0.0, 0.0, 0.0, self.contact.stiffness, 0.0, 0.0), self._plane(), pts.x_device,
                                u=uq, e=e)
            out["contact"] = float(pts.weights.inner(e))
        out["total"] = out["strain"] + out["kinetic"] + out["contact"]
        return out

    def tangent(self):
        return _DynamicTangent(self)

    def mass_form(self):
        """the form of density * mass matrix (the value-value entries of the point tangent alone): ``assemble_matrix(V)``"""
        return _DynamicMass(self)


class _DynamicTangent(_LawTangent):
    """The tangent form (dR/dy) / alpha_f of a ``DynamicResidual``: the form of the law's tangent at y_alpha -- its class, its
    symmetry, its transform and assembly -- with rho (c_a + a_M c_v) / alpha_f and k [g > 0] n (x) n added to its value-value
    entries at the points (a solid: as the reaction of the form)."""

    def __init__(self, dyn):
        self.dyn = dyn
        _LawTangent.__init__(self, dyn._law)

    def _form(self, V, row0, row1, block):
        dyn, law = self.dyn, self.res
        g, nF, pts = dyn._scope(V, row0, row1, block)
        dyn._state(g, nF, pts)
        c = dyn.coefficients()
        tangent = law.law(V, False, True).tangent
        values = law._value_tangent(pts, nF, tangent)
        dyn._dynamics(pts, nF, (1.0, 0.0, 0.0, c["t_m"], 0.0, dyn._stiffness(), 0.0), T=values)
        form = law._tangent_form(pts, nF, tangent, values)
        # (the symmetry: the law's, a host law's bits, a pressure's False; inertia and the penalty are symmetric)
        form._symmetric_hint = self.symmetric = law._law_symmetric()
        return form


class _DynamicMass(object):
    """density * int y . v of a ``DynamicResidual``: the form of the tangent on point data with nothing but density in the nF
    value-value diagonal entries (written by ``tg_point_dynamics`` into zeros)"""
    symmetric = True

    def __init__(self, dyn):
        self.dyn, self.geometry = dyn, dyn.geometry

    def assemble_matrix(self, V, row0=None, row1=None):
        dyn, law = self.dyn, self.dyn._law
        g, nF, pts = dyn._scope(V, row0, row1)
        values = law._value_tangent(pts, nF)
        _dev.point_dynamics(nF, law.nJ, pts.npts, (1.0, 0.0, 0.0, dyn.density, 0.0, 0.0, 0.0), T=values)
        form = law._tangent_form(pts, nF, None, values)
        form._symmetric_hint = True
        return form.assemble_matrix(V)


# ---- boundary integrals on a mapped patch (csrc/tg_boundary.hip): spline.ds and spline.n of the reference -----------------
def _periodic_directions(geometry):
    """directions whose knot vector is not open (the faces there are no boundary), as far as the geometry tells"""
    gen = getattr(geometry, "_generator", geometry)
    mesh = getattr(gen, "controlMesh", None)
    try:
        splines = mesh.getScalarSpline().splines
    except Exception:
        return set()
    out = set()
    for k, s in enumerate(splines):
        kn, p = numpy.asarray(getattr(s, "knots", ()), dtype=float), int(getattr(s, "p", 0))
        if kn.size and not (numpy.all(kn[:p + 1] == kn[0]) and numpy.all(kn[-(p + 1):] == kn[-1])):
            out.add(k)
    return out


def check_faces(faces, d, who, periodic=()):
    """the faces as a list of (direction, side): None = all 2 d faces of a d-dimensional patch, one pair, or a sequence of
    pairs; ValueError for anything else, for a face outside 0 <= direction < d, side in {0, 1}, and for a face of a
    periodic direction"""
    if faces is None:
        faces = [(k, s) for k in range(d) if k not in periodic for s in (0, 1)]
        if not faces:
            raise ValueError("%s: every direction of the patch is periodic; it has no boundary" % who)
        return faces
    try:
        if len(faces) == 2 and all(numpy.ndim(v) == 0 for v in faces):
            faces = [tuple(faces)]
        faces = [tuple(f) for f in faces]
    except TypeError:
        raise ValueError("%s: faces = %r: (direction, side) pairs expected" % (who, faces))
    if not faces:
        raise ValueError("%s: no face given" % who)
    for f in faces:
        if len(f) != 2 or any(isinstance(v, bool) or int(v) != v for v in f):
            raise ValueError("%s: face %r: a (direction, side) pair of integers expected" % (who, f))
        if not (0 <= f[0] < d and f[1] in (0, 1)):
            raise ValueError("%s: face %r: 0 <= direction < %d and side 0 or 1" % (who, f, d))
        if f[0] in periodic:
            raise ValueError("%s: face %r: direction %d of the patch is periodic; it has no boundary there" % (who, f, f[0]))
    if len(set(faces)) != len(faces):
        raise ValueError("%s: a face is listed twice" % who)
    return [(int(k), int(s)) for k, s in faces]


def _need_boundary_geometry(who, geometry):
    if geometry is None:
        raise ValueError("%s: boundary integrals are taken on a mapped patch (geometry=...)" % who)


def _face_grid(V, who):
    """(node grid, number of fields) of a space whose fields share one CG node grid"""
    g = _one_shared_grid(V, who)
    if g.dim() not in (2, 3):
        raise NotImplementedError("%s: faces are provided for 2-D and 3-D patches" % who)
    return g, len(V.grids)


def _fields_of_the_patch(geometry, who):
    """Refuses a geometry whose generator puts its fields on bases of their own (FieldListSpline, compatible spaces):
    their FE fields may share one node grid and still are not the Q_p functions of the patch that the face kernels
    integrate.  The node grid alone does not tell, so the generator is asked."""
    gen = getattr(geometry, "_generator", geometry)
    on_control = getattr(gen, "_fields_on_control_basis", None)
    if on_control is not None and not on_control():
        raise NotImplementedError("%s: the fields of %s are not discretised with the control mesh's scalar basis "
                                  "(FieldListSpline and compatible spaces are not supported)" % (who, type(gen).__name__))


def _whole_rows(n, row0, row1, who, over="face"):
    if (0 if row0 is None else int(row0), n if row1 is None else int(row1)) != (0, n):
        raise NotImplementedError("%s: row blocks (several ranks, streamed operands) are not supported; the point values "
                                  "are numbered over the whole %s" % (who, over))


class FacePoints(QuadraturePoints):
    """The Gauss points of the face (direction, side) of a mapped patch, face-element-major (the face elements and the
    nq^(d-1) points of one lexicographic in the remaining directions with the lower direction fastest): ``x`` host array
    [npts, nsd] (downloaded on first use), ``x_device`` and ``normals`` (nsd * npts values, component-major; the unit
    normal DF g^-1 N / |.|), ``weights`` = w_q sqrt(det g_hat (g_hat^-1)_kk) (the reference's surfaceJacobian times the face
    element's parametric area), ``h_normal`` = 1 / sqrt((g_hat^-1)_kk) (the thickness of the boundary element normal to
    the face), ``n`` (host [npts, nsd]), ``nq``, ``npts``, ``nsd``, ``direction``, ``side``."""

    def __init__(self, verts, p, cp, nq, direction, side):
        self.verts, self.p, self.cp, self.nq, self.nsd = verts, p, cp, nq, len(cp) - 1
        self.direction, self.side = int(direction), int(side)
        self.x_device, self.weights, self.normals, self.h_normal = _dev.face_points(verts, p, cp, direction, side, nq)
        self.npts = self.weights.size()
        self._x = self._n = None

    @property
    def metric(self):
        raise NotImplementedError("the element metric is provided at the points of the volume, not of a face")

    @property
    def n(self):
        if self._n is None:
            self._n = point_unblock(self.normals.get_local(), self.npts, (self.nsd,))
        return self._n

    def values(self, f, who="f"):
        """as ``QuadraturePoints.values``; a Function of the space is evaluated by ``tg_face_eval``"""
        if hasattr(f, "vector") and hasattr(f, "function_space"):
            return _dev.face_eval(self.verts, self.p, self.cp, self.direction, self.side, f.vector(), nq=self.nq)[0]
        return QuadraturePoints.values(self, f, who)


def face_points(geometry, V, direction, side, nq=None, who="boundary points"):
    """the ``FacePoints`` of one face of the patch of ``geometry``, kept on it per (face, nq, control-function vectors)"""
    _need_boundary_geometry(who, geometry)
    g, _ = _face_grid(V, who)
    _fields_of_the_patch(geometry, who)
    (direction, side), = check_faces((direction, side), g.dim(), who, _periodic_directions(geometry))
    verts, p, cp = _whole_patch(geometry, g, who, "boundary operands")
    nq = _check_nq(nq, p)
    cache = geometry.__dict__.setdefault("_face_points", {})
    key = (direction, side, nq, tuple(id(v) for v in cp))
    if key not in cache:
        cache[key] = FacePoints(verts, p, cp, nq, direction, side)
    return cache[key]


def _argcount(f):
    import inspect
    try:
        return len([q for q in inspect.signature(f).parameters.values()
                    if q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD) and q.default is q.empty])
    except (TypeError, ValueError):
        return 1


def _per_face(f, i, nfaces, who):
    """the data of face i: a list holds one entry per face, anything else serves every face"""
    if isinstance(f, list):
        if len(f) != nfaces:
            raise ValueError("%s: a list of %d entries given for %d faces" % (who, len(f), nfaces))
        return f[i]
    return f


def _face_values(pts, f, who):
    """scalar point values on a face; a callable may take (x) or (x, n)"""
    if callable(f) and not hasattr(f, "vector") and _argcount(f) >= 2:
        v = numpy.asarray(f(pts.x, pts.n), dtype=numpy.float64)
        if v.shape != (pts.npts,):
            raise ValueError("%s: the callable returned an array of shape %s for %d points; expected (%d,)"
                             % (who, v.shape, pts.npts, pts.npts))
        return _dev.DeviceVector(data=v)
    return pts.values(f, who)


class BoundaryLoadForm(object):
    """L(v) = int_faces f v ds on the mapped patch, ds and the unit normal n as ``spline.ds`` / ``spline.n`` of the
    reference.  ``faces``: (direction, side) pairs numbered as ``getSideDofs``, one pair, or None = all faces.  ``f``: a
    callable of the points ``x [npts, nsd] -> [npts]``, or of ``(x, n)`` when it takes two arguments; a number; point
    values (numbered as ``FacePoints``); a ``Function``; or a list with one of these per face (a list always means that).  On a space of several
    fields sharing one node grid (the space of ``ElasticityForm``) ``f`` gives [npts, nF] -- a traction -- and the
    component loads are written field after field.  ``fn``: adds int fn d_n v ds (the Nitsche right-hand side).
    ``rational``: v the functions phi / W_h."""

    def __init__(self, f, geometry, faces=None, nq=None, rational=False, fn=None):
        _need_boundary_geometry("BoundaryLoadForm", geometry)
        self.f, self.fn, self.geometry, self.faces, self.nq = f, fn, geometry, faces, nq
        self.rational = bool(rational)

    @classmethod
    def pressure(cls, p, geometry, faces=None, nq=None, rational=False):
        """the traction f = -p n of a pressure ``p`` (a number, or a callable of the points)"""
        def traction(x, n):
            pv = numpy.asarray(p(x), dtype=numpy.float64) if callable(p) else numpy.full(x.shape[0], float(p))
            return -pv[:, None] * n
        return cls(traction, geometry, faces, nq, rational)

    def _components(self, pts, f, nF):
        if nF == 1:
            return [_face_values(pts, f, "BoundaryLoadForm")]
        return _field_values(pts, f, nF, "BoundaryLoadForm")

    def assemble_vector(self, V, row0=None, row1=None):
        g, nF = _face_grid(V, "BoundaryLoadForm")
        n = g.num_nodes()
        _whole_rows(nF * n, row0, row1, "BoundaryLoadForm")
        faces = check_faces(self.faces, g.dim(), "BoundaryLoadForm", _periodic_directions(self.geometry))
        if self.fn is not None and nF != 1:
            raise NotImplementedError("BoundaryLoadForm: the normal-derivative term is provided for scalar spaces")
        parts = [_dev.DeviceVector(n) for _ in range(nF)]
        for i, (k, s) in enumerate(faces):
            pts = face_points(self.geometry, V, k, s, self.nq, "BoundaryLoadForm")
            comps = self._components(pts, _per_face(self.f, i, len(faces), "BoundaryLoadForm"), nF) \
                if self.f is not None else [None] * nF
            fn = _face_values(pts, _per_face(self.fn, i, len(faces), "BoundaryLoadForm"), "BoundaryLoadForm: fn") \
                if self.fn is not None else None
            for c in range(nF):
                _dev.face_load(pts.verts, pts.p, pts.cp, k, s, comps[c], fn, parts[c], nq=pts.nq, rational=self.rational)
        if nF == 1:
            return parts[0]
        out = _dev.DeviceVector(nF * n, zero=False)
        for c in range(nF):
            _dev.vec_copy_range(out, c * n, parts[c], 0, n)
        return out


class _FaceMatrixForm(object):
    """what the boundary matrix forms share: the point coefficients (a, b, c) per face, the assembly on the face pattern
    and the in-place addition into a matrix that holds the entries"""

    def _setup(self, who, geometry, faces, nq, rational):
        _need_boundary_geometry(who, geometry)
        self.geometry, self.faces, self.nq, self.rational = geometry, faces, nq, bool(rational)

    def _faces(self, V):
        who = type(self).__name__
        g = _single_grid(V)
        _face_grid(V, who)
        faces = check_faces(self.faces, g.dim(), who, _periodic_directions(self.geometry))
        return g, [(i, face_points(self.geometry, V, k, s, self.nq, who)) for i, (k, s) in enumerate(faces)]

    def assemble_matrix(self, V, row0=None, row1=None):
        g, faces = self._faces(V)
        _whole_rows(g.num_nodes(), row0, row1, type(self).__name__)
        A = None
        for i, pts in faces:
            a, b, c = self.coefficients(pts, i, len(faces))
            if A is None:
                A = _dev.face_matrix(pts.verts, pts.p, pts.cp, pts.direction, pts.side, a, b, c, nq=pts.nq,
                                     rational=self.rational)
            elif not _dev.face_matrix_add(A, pts.verts, pts.p, pts.cp, pts.direction, pts.side, a, b, c, nq=pts.nq,
                                          rational=self.rational):
                A = A.add(_dev.face_matrix(pts.verts, pts.p, pts.cp, pts.direction, pts.side, a, b, c, nq=pts.nq,
                                           rational=self.rational))
        return A

    def add_into(self, A, V, scale=1.0):
        """adds ``scale`` times the form's entries in place into ``A``; False, with ``A`` unchanged, when the pattern of
        ``A`` lacks entries of one of the faces"""
        g, faces = self._faces(V)
        todo = [(pts, self.coefficients(pts, i, len(faces))) for i, pts in faces]
        # the pattern of every face first (a call without coefficients only looks), then the additions
        for pts, _ in todo:
            if not _dev.face_matrix_add(A, pts.verts, pts.p, pts.cp, pts.direction, pts.side, nq=pts.nq):
                return False
        for pts, (a, b, c) in todo:
            _dev.face_matrix_add(A, pts.verts, pts.p, pts.cp, pts.direction, pts.side, a, b, c, scale=scale, nq=pts.nq,
                                 rational=self.rational)
        return True


class BoundaryMassForm(_FaceMatrixForm):
    """a(u, v) = int_faces alpha u v ds (a Robin term).  ``alpha``: as ``f`` of ``BoundaryLoadForm`` on a scalar space."""

    def __init__(self, alpha, geometry, faces=None, nq=None, rational=False):
        self._setup("BoundaryMassForm", geometry, faces, nq, rational)
        self.alpha = alpha
        self.symmetric = type(self) is BoundaryMassForm

    def coefficients(self, pts, i, nfaces):
        return _face_values(pts, _per_face(self.alpha, i, nfaces, "BoundaryMassForm"), "BoundaryMassForm: alpha"), None, None


class NitscheForm(_FaceMatrixForm):
    """a(u, v) = int_faces (gamma u v - d_n u v -+ u d_n v) ds: a Dirichlet condition imposed weakly; the minus sign is the
    symmetric variant.  ``penalty``: a number C, meaning gamma = C p^2 / h_n with the thickness h_n of the boundary
    element normal to the face, or point values / a callable for gamma itself.  ``load(g)`` is the matching right-hand
    side int (gamma g v -+ g d_n v) ds."""

    def __init__(self, geometry, faces, penalty, symmetric=True, nq=None, rational=False):
        self._setup("NitscheForm", geometry, faces, nq, rational)
        self.penalty = penalty
        self.symmetric = bool(symmetric) and type(self) is NitscheForm
        self._sign = -1.0 if symmetric else 1.0

    def gamma(self, pts, i=0, nfaces=1):
        pen = _per_face(self.penalty, i, nfaces, "NitscheForm")
        if numpy.ndim(pen) == 0 and not callable(pen) and not isinstance(pen, _dev.DeviceVector):
            one = _dev.DeviceVector(pts.npts, zero=False)
            one.fill(float(pen) * float(pts.p) ** 2)
            return one.pointwise_divide(pts.h_normal)
        return _face_values(pts, pen, "NitscheForm: penalty")

    def coefficients(self, pts, i, nfaces):
        minus = _dev.DeviceVector(pts.npts, zero=False)
        minus.fill(-1.0)
        other = minus
        if self._sign > 0:
            other = _dev.DeviceVector(pts.npts, zero=False)
            other.fill(1.0)
        return self.gamma(pts, i, nfaces), minus, other

    def load(self, g):
        """L(v) = int_faces (gamma g v -+ g d_n v) ds for the Dirichlet data ``g`` (as ``f`` of ``BoundaryLoadForm``)"""
        return _NitscheLoad(self, g)


class _NitscheLoad(object):
    def __init__(self, form, g):
        self.form, self.g = form, g

    def assemble_vector(self, V, row0=None, row1=None):
        F = self.form
        g, faces = F._faces(V)
        _whole_rows(g.num_nodes(), row0, row1, "NitscheForm.load")
        out = _dev.DeviceVector(g.num_nodes())
        for i, pts in faces:
            gq = _face_values(pts, _per_face(self.g, i, len(faces), "NitscheForm.load"), "NitscheForm.load")
            fq = F.gamma(pts, i, len(faces)).pointwise_mult(gq)
            fnq = gq
            if F._sign < 0:
                fnq = gq.copy()
                fnq.axpy(-2.0, gq)
            _dev.face_load(pts.verts, pts.p, pts.cp, pts.direction, pts.side, fq, fnq, out, nq=pts.nq, rational=F.rational)
        return out


class Sum(object):
    """sum_t c_t form_t for ``(coefficient, form)`` pairs or bare forms (coefficient 1): ``assemble_matrix`` and
    ``assemble_vector``.  Matrices: the first volume term is assembled; ``BoundaryMassForm`` and ``NitscheForm`` terms are
    added in place (``tg_face_matrix_add``) when its pattern holds their entries -- every mapped form's does -- so that
    the sum keeps the pattern certificate of the volume term; otherwise, and for further volume terms,
    ``DeviceCSR.combine`` on equal patterns, else ``DeviceCSR.add``.  ``symmetric`` is true only if every term's is."""

    def __init__(self, *terms):
        if not terms:
            raise ValueError("Sum: no term given")
        self.terms = []
        for t in terms:
            c, form = (t if isinstance(t, tuple) else (1.0, t))
            if isinstance(t, tuple) and (len(t) != 2 or numpy.ndim(t[0]) != 0):
                raise ValueError("Sum: a term is a form or a (coefficient, form) pair")
            if not (hasattr(form, "assemble_matrix") or hasattr(form, "assemble_vector")):
                raise ValueError("Sum: %r has neither assemble_matrix nor assemble_vector" % (form,))
            self.terms.append((float(c), form))
        kinds = set(hasattr(f, "assemble_matrix") for _, f in self.terms)
        if len(kinds) != 1:
            raise ValueError("Sum: matrix forms and vector forms cannot be added")
        self.symmetric = all(getattr(f, "symmetric", False) is True for _, f in self.terms)
        self.in_place = 0          # face terms the last assemble_matrix added in place

    @staticmethod
    def _axpby(A, a, B, b):
        """a A + b B: on one pattern if the two share it, else on the union"""
        try:
            return A.combine(a, B, b)
        except _dev.TigarHipError:
            if a != 1.0:
                A = A.combine(a, A, 0.0)
            return A.add(B if b == 1.0 else B.combine(b, B, 0.0))

    def assemble_matrix(self, V, row0=None, row1=None):
        if not hasattr(self.terms[0][1], "assemble_matrix"):
            raise TypeError("Sum: the terms are vector forms")
        volume = [(c, f) for c, f in self.terms if not isinstance(f, _FaceMatrixForm)]
        faces = [(c, f) for c, f in self.terms if isinstance(f, _FaceMatrixForm)]
        self.in_place = 0
        A = None
        for c, f in volume:
            B = f.assemble_matrix(V, row0, row1)
            if A is None:
                A = B if c == 1.0 else B.combine(c, B, 0.0)
            else:
                A = self._axpby(A, 1.0, B, c)
        for c, f in faces:
            if A is None:
                B = f.assemble_matrix(V, row0, row1)
                A = B if c == 1.0 else B.combine(c, B, 0.0)
                continue
            _whole_rows(_single_grid(V).num_nodes(), row0, row1, "Sum")
            if f.add_into(A, V, c):
                self.in_place += 1
            else:
                A = self._axpby(A, 1.0, f.assemble_matrix(V), c)
        return A

    def assemble_vector(self, V, row0=None, row1=None):
        if not hasattr(self.terms[0][1], "assemble_vector"):
            raise TypeError("Sum: the terms are matrix forms")
        out = None
        for c, f in self.terms:
            v = f.assemble_vector(V, row0, row1)
            if out is None:
                out = v
                if c != 1.0:
                    out = v.copy()
                    out.zero()
                    out.axpy(c, v)
            else:
                out.axpy(c, v)
        return out
