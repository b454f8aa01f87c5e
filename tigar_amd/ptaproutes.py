"""Which product forms M^T A M for a resident extraction operator (``ExtractedSpline.extractMatrix``,
tIGAr/common.py:1176-1204): ONE ordered table of routes ``(name, applies, run)``, walked per call.
``applies(call)`` says whether the route is to be tried for this M and this A; ``run(call)`` returns K or None ("declined",
the plans' rc == 100) and the next route is asked.  ``K.ptap_route`` names the route that formed K (for the tests; nothing
else reads it).  A new route is one more entry of ``ResidentPtAP.routes`` at the place its precedence asks for, its plan
cache (if any) next to the others in ``reset()``."""
import os

import numpy

from . import device as _dev
from .device import DeviceCSR
from .feorder import as_device_csr
from .implicit import LazyFEMatrix
from .tensorptap import TensorPtAP, TensorPtAP2D, plan_or_unwrapped


def first_route(routes, call):
    """K of the first route of the table that applies and does not decline, named after it"""
    for name, applies, run in routes:
        if applies(call):
            K = run(call)
            if K is not None:
                if not hasattr(K, "ptap_route"):          # (a route with a variant has named K itself: "walks2d+fold")
                    K.ptap_route = name
                return K
    raise RuntimeError("no PtAP route took the product")


class _Call(object):
    """one ``product``: the operands, what is asked about A, and the switches that steer the routing -- read once per call,
    when the call is made (README: every switch is read when the call it affects is made)"""

    def __init__(self, A, zero_dofs, diag):
        self.raw, self.zd, self.diag = A, zero_dofs, float(diag)
        on = lambda name: os.environ.get(name, "1") != "0"
        self.factored, self.unwrap, self.cells = on("TIGAR_PTAP_FACTORED"), on("TIGAR_PTAP_UNWRAP"), on("TIGAR_PTAP_CELLS")
        self.elements = os.environ.get("TIGAR_PTAP_ELEMENTS", "1")             # ("2": the element split at any size)

    @property
    def A(self):
        """A on the device (the slab engine takes the FE matrix as it was handed in)"""
        self.raw = as_device_csr(self.raw)
        return self.raw


def empty_block(r, c):
    import scipy.sparse as _sp
    return DeviceCSR.from_scipy(_sp.csr_matrix((int(r), int(c))))


def general_once(A, M, MT):
    """M^T A M by the general kernels, symbolic plan not kept"""
    return _dev.ptap_numeric(_dev.ptap_symbolic(A, M, MT), A, M, MT)


def kron_stages(kx, A, zd=None, diag=1.0, stored=None):
    """the scalar machinery for a Kronecker M (``ptap_factored`` on the whole patch): 3-D line walks, pattern split (entries
    outside the element-coupling pattern apart), else the dense-box or the general line kernels, in one or several stages"""
    from .kronptap import default_groups, ptap_factored
    groups = default_groups(kx.d, max(s1.p for s1 in kx.basis.splines))
    return ptap_factored(kx, A, (0, kx.nfe[-1]), (0, kx.nfe[-1]), (0, kx.ncp[-1]), zd, diag, groups, stored=stored)


def walk_planes(plan, Afg, kx, min_step, nnz):
    """block M_f^T A_fg M_g by the 3-D line walks: the x / y passes over the FE planes in steps, then the z pass.  None when
    the block does not carry the element-coupling pattern.  ``nnz``: the entries the step is sized for."""
    nz, kz = int(kx.nfe[-1]), int(kx.ncp[-1])
    # FE planes per call of the x / y passes: their first intermediate is about 2.5 x the block's own bytes
    step = max(min_step, min(nz, int(2.0e10 // max(1.0, 12.0 * 2.5 * nnz / nz))))
    pieces = []
    for z0 in range(0, nz, step):
        pc = plan.planes(Afg, 0, z0, min(nz, z0 + step))
        if pc is None:
            return None
        pieces.append(pc)
    return plan.zstage(pieces, 0, kz)


def product_by_field_blocks(A, kxs, walks, general, zd, diag):
    """M^T A M for M = diag(M_f), field f on the tensor basis ``kxs[f]``, dofs field after field: block (f, g) of the result
    is M_f^T A_fg M_g, computed on the block cut out of A (tg_csr_block) -- ``walks(f, g, A_fg)`` where the patch and the
    block qualify (None: declined), ``general(f, g, A_fg)`` otherwise; both return (K_fg, how).  The blocks are put together
    (tg_csr_from_blocks) and MatZeroRowsColumns is applied to the whole (tIGAr/common.py:1194-1200).  None when A is not a
    matrix on this mixed space.  ``K.ptap_block_routes[f][g]`` says how each block was formed."""
    nF = len(kxs)
    fo = numpy.concatenate([[0], numpy.cumsum([int(numpy.prod(kx.nfe, dtype=numpy.int64)) for kx in kxs])])
    co = numpy.concatenate([[0], numpy.cumsum([int(numpy.prod(kx.ncp, dtype=numpy.int64)) for kx in kxs])])
    if A.shape != (int(fo[-1]), int(fo[-1])):
        return None
    blocks, how = [], []
    for f in range(nF):
        blocks.append([])
        how.append([])
        for g in range(nF):
            Afg = A.block(int(fo[f]), int(fo[f + 1]), int(fo[g]), int(fo[g + 1]))
            if Afg.nnz == 0:
                # fields f and g are not coupled by this form: no entries in this block of the product either
                done = (empty_block(co[f + 1] - co[f], co[g + 1] - co[g]), "empty")
            else:
                done = walks(f, g, Afg) or general(f, g, Afg)
            blocks[f].append(done[0])
            how[f].append(done[1])
            del Afg, done
    K = _dev.csr_from_blocks(blocks)
    del blocks
    if zd is not None and len(zd):
        K.zero_rows_cols(numpy.asarray(zd, dtype=numpy.int32), diag)
    K.ptap_block_routes = how
    return K


class ResidentPtAP(object):
    """The products that form K = M^T A M for one extraction operator ``M`` (``MT``: its transpose; M may be implicit), and
    the order in which they are asked.  ``kron`` / ``kron_scalar`` / ``kron_fields``: the ``KronExtraction`` of a single
    tensor-product field / of the scalar basis several fields share / of each field on its own basis (None where absent);
    ``grids``: the meshes of the FE space (element split); ``slab``: a callable that yields the streamed engine
    (``dist.SlabHotPath`` and its field forms), ``row_blocks(A)`` / ``field_blocks(A)`` what it consumes, ``timers`` a callable
    for its stage timers.  The plans depend on M only and are kept here; A is verified on the device at every call."""

    def __init__(self, M, MT, nFields=1, kron=None, kron_scalar=None, kron_fields=None, grids=None, distributed=False,
                 slab=None, row_blocks=None, field_blocks=None, timers=lambda: None):
        self.M, self.MT, self.nFields = M, MT, int(nFields)
        self.kron, self.kron_scalar, self.kron_fields, self.grids = kron, kron_scalar, kron_fields, grids
        self.distributed, self.implicit = bool(distributed), bool(getattr(M, "is_implicit", False))
        self._slab, self._row_blocks, self._field_blocks, self._timers = slab, row_blocks, field_blocks, timers
        # several fields on one scalar basis (EqualOrderSpline(nFields > 1)): block by block
        self.by_blocks = kron is None and kron_scalar is not None
        self.reset()
        self.kx2 = kx2 = kron if kron is not None else kron_scalar           # (what a 2-D patch walks on)
        self.routes = [
            ("slab", self._slab_applies, self._slab_product),
            ("walks2d", lambda c: kx2 is not None and kx2.d == 2 and not c.A.is_loose() and c.factored, self._walks2d),
            ("field-blocks", lambda c: self.by_blocks and c.factored, lambda c: self.field_blocks(c.A, c.zd, c.diag)),
            ("field-list", lambda c: kron is None and not self.by_blocks and kron_fields is not None and c.factored,
             lambda c: self.field_list(c.A, c.zd, c.diag)),
            ("kron", lambda c: kron is not None and c.factored, self._kron_product),
            ("slab-general", lambda c: self.implicit, self._slab_general),
            ("cells", lambda c: c.cells, self._cells),
            ("elements", lambda c: c.elements != "0" and not c.A.is_loose(), self._elements),
            ("general", lambda c: True, self._general),
        ]

    def reset(self):
        """forget every plan (another M: a new ``ResidentPtAP`` is the usual way)"""
        self.cell_plans = {}                 # CellBlockPtAP (or None: M is not cell-local at this size) per block size
        self.remainder_cache = {}            # symbolic plan of the couplings outside the cell blocks
        self.element_plan = None             # (M, ElementSplitPtAP or None)
        self.general_plan = self.general_key = None

    def product(self, A, zero_dofs, diag=1.0):
        """K = M^T A M with the rows and columns ``zero_dofs`` zeroed and ``diag`` on their diagonal"""
        return first_route(self.routes, _Call(A, zero_dofs, diag))

    # -- 0 / 5: the streamed engine ----------------------------------------------------------------------------------
    def _slab_applies(self, c):
        # (several fields with an implicit operator, also on one rank: the field-block engine and its plane-wise
        #  numbering -- the same guard as extractVector / solveLinearSystem, so that K, M^T b and U share it;
        #  an explicit A -- FEtoIGA's identity, an uploaded matrix -- is cut into the blocks the engine asks for)
        return isinstance(c.raw, LazyFEMatrix) or self.distributed or (self.implicit and self.nFields > 1)

    def _slab_product(self, c):
        A = c.raw
        if self.nFields > 1 and self.kron is None and (self.kron_scalar is not None or self.kron_fields is not None):
            return self._slab().assemble_matrix(self._field_blocks(A), c.zd, c.diag, self._timers(),
                                                block_factors=getattr(A, "block_factors", None))
        # an assembled FE matrix handed to every rank (the reference's A is a distributed PETSc matrix whose
        # rows MatPtAP redistributes, tIGAr/common.py:1194-1195): every rank cuts the row blocks of its slab out
        # of its copy -- on the device when it is a DeviceCSR, on the host (then uploaded) when it is scipy
        lazy = isinstance(A, LazyFEMatrix)
        return self._slab().assemble_matrix(A.rows if lazy else self._row_blocks(A), c.zd, c.diag, self._timers(),
                                            a_factors=A.kron_factors if lazy else None)

    def _slab_general(self, c):
        # an implicit operator that is not to be used as a Kronecker product (TIGAR_PTAP_FACTORED=0) with an assembled A: the
        # streamed engine materialises M chunk by chunk and takes its general stages -- element chunks, or the row-wise
        # kernels for a matrix they decline (round 6; until then: NotImplementedError)
        return self._slab().assemble_matrix(self._row_blocks(c.A), c.zd, c.diag, self._timers())

    # -- 1: 2-D line walks -------------------------------------------------------------------------------------------
    def _walks2d(self, c):
        # 2-D tensor patches (one or several fields on one basis): the whole product in two line-walk passes when A
        # carries the element-coupling pattern (verified on the device; csrc/tg_tensor_body.h)
        nF = self.nFields if self.by_blocks else 1
        plan, ku = plan_or_unwrapped(TensorPtAP2D, self.kx2, nF, unwrap=c.unwrap)
        if plan is None or ku is None:
            return plan.ptap(c.A, c.zd, c.diag) if plan is not None else None
        # periodic directions (tIGAr/BSplines.py:204-212): the walks on the space before the wrapped functions
        # are identified, then K = R^T K_u R (kronptap.KronExtraction.unwrapped / fold)
        K_u = plan.ptap(c.A, None, 1.0)
        if K_u is None:
            return None
        K = ku.fold(K_u, c.zd, c.diag, nfields=nF)
        K.ptap_route = "walks2d+fold"
        return K

    # -- 2 / 3: several fields, block by block -----------------------------------------------------------------------
    def field_blocks(self, A, zd, diag, tensor=True):
        """Several fields on ONE tensor basis (M = diag(M_s, ..., M_s)): the scalar tensor-pattern passes
        (csrc/tg_tensor_body.h) where the patch and the block qualify, else the scalar machinery for a Kronecker M;
        ``tensor=False``: the general kernels on the scalar operands (whose per-row tables hold a scalar row's
        intermediate, not that of nFields of them)."""
        kx, nF = self.kron_scalar, self.nFields
        plan = TensorPtAP.for_extraction(kx) if tensor else None
        nfe = int(numpy.prod(kx.nfe, dtype=numpy.int64))
        ncp = int(numpy.prod(kx.ncp, dtype=numpy.int64))
        scalar = {}

        def walks(f, g, Afg):
            Kfg = walk_planes(plan, Afg, kx, kx.basis.splines[-1].p, A.nnz / float(nF * nF)) if plan is not None else None
            return (Kfg, "walks3d") if Kfg is not None else None

        def general(f, g, Afg):
            if tensor:
                return kron_stages(kx, Afg), "kron"
            if not scalar:
                scalar["M"] = self.M.block(0, nfe, 0, ncp)
                scalar["MT"] = scalar["M"].transpose()
                scalar["elem"] = self._element_plan_for(scalar["M"])
            if scalar["elem"] is not None and not Afg.is_loose():
                # (every block of an assembled matrix on the mixed space couples nodes of common cells of the scalar mesh)
                Kfg = scalar["elem"].ptap(Afg, None, 1.0)
                if Kfg is not None:
                    return Kfg, "elements"
            return general_once(Afg, scalar["M"], scalar["MT"]), "general"

        return product_by_field_blocks(A, [kx] * nF, walks, general, zd, diag)

    def field_list(self, A, zd, diag):
        """Fields on DIFFERENT tensor bases (M = diag(M_f)): block (f, g) = M_f^T A_fg M_g by the line walks with separate
        row- and column-side weights where the pair qualifies (all fields on one Q_P node grid, degrees <= 3 in 3-D:
        ``TensorPtAP.for_pair``, <= 4 in 2-D: ``TensorPtAP2D.for_pair``; csrc/tg_tensor_body.h), by the general kernels on
        the scalar operands otherwise."""
        kxs = self.kron_fields
        nfe = [int(numpy.prod(kx.nfe, dtype=numpy.int64)) for kx in kxs]
        ncp = [int(numpy.prod(kx.ncp, dtype=numpy.int64)) for kx in kxs]
        fo, co = numpy.concatenate([[0], numpy.cumsum(nfe)]), numpy.concatenate([[0], numpy.cumsum(ncp)])
        scalar = {}

        def walks(f, g, Afg):
            plan = TensorPtAP.for_pair(kxs[f], kxs[g]) if (kxs[f].d == 3 and not Afg.is_loose()) else None
            if plan is not None:
                Kfg = walk_planes(plan, Afg, kxs[f], int(kxs[f].grid.degree), Afg.nnz)
                if Kfg is not None:
                    return Kfg, "walks3d"
            if kxs[f].d == 2 and not Afg.is_loose():
                # 2-D compatible splines (demos/taylor-green/taylor-green-2d.py): the block in two walks
                plan2 = TensorPtAP2D.for_pair(kxs[f], kxs[g])
                Kfg = plan2.ptap(Afg) if plan2 is not None else None
                if Kfg is not None:
                    return Kfg, "walks2d"
            return None

        def general(f, g, Afg):
            for q in (f, g):
                if q not in scalar:
                    Mq = self.M.block(int(fo[q]), int(fo[q + 1]), int(co[q]), int(co[q + 1]))
                    scalar[q] = (Mq, Mq.transpose())
            if f == g:
                return general_once(Afg, *scalar[f]), "general"
            # the general kernels form P^T A P with ONE operator: block (0, 1) of the product on the two-field space
            # diag(M_f, M_g) with A_fg as its only non-zero block
            zero = empty_block
            Mp = _dev.csr_from_blocks([[scalar[f][0], zero(nfe[f], ncp[g])], [zero(nfe[g], ncp[f]), scalar[g][0]]])
            Ap = _dev.csr_from_blocks([[zero(nfe[f], nfe[f]), Afg], [zero(nfe[g], nfe[f]), zero(nfe[g], nfe[g])]])
            return general_once(Ap, Mp, Mp.transpose()).block(0, ncp[f], ncp[f], ncp[f] + ncp[g]), "general"

        return product_by_field_blocks(A, kxs, walks, general, zd, diag)

    # -- 4: Kronecker-structured M -----------------------------------------------------------------------------------
    def _kron_product(self, c):
        # (the unwrapping of periodic directions is taken inside ``ptap_factored`` as well)
        return kron_stages(self.kron, c.A, c.zd, c.diag, stored=None if self.implicit else (self.M, self.MT))

    # -- 6: cell-local FE spaces -------------------------------------------------------------------------------------
    def _cells(self, c):
        # cell-local FE spaces (T-splines, multi-patch B-splines: meshes of disconnected cells): an assembled A is block
        # diagonal with one dense block per cell and the product is a sum of small dense triple products
        # (tigar_amd/cellptap.py); the plan depends on M only and is kept, A is verified on the device at every call
        from .cellptap import CellBlockPtAP, block_size_of, cell_size_with_extras, remainder_product
        b = block_size_of(c.A)
        extras = not b
        b = b or cell_size_with_extras(c.A)
        if not b or c.A.shape[0] != self.M.shape[0]:
            return None
        if b not in self.cell_plans:
            try:
                self.cell_plans[b] = CellBlockPtAP(self.M, b)
            except ValueError:
                self.cell_plans[b] = None
        plan = self.cell_plans[b]
        if plan is None or not extras:
            return plan.ptap(c.A, c.zd, c.diag) if plan is not None else None
        # couplings outside the cell blocks (contact / penalty terms added by hand: the reason extractMatrix takes
        # any A, tIGAr/common.py:1175; demos/kl-shell-svk/reef-knot.py:455-467): A = D + R on the device, the
        # dense blocks D through the cell-block product, the few entries of R through the general kernels, the
        # two added on the union of their patterns (= the structural product of A), then MatZeroRowsColumns
        parts = plan.ptap_extras(c.A)
        if parts is None or parts[0] is None:
            return None
        KD, R = parts
        KR = remainder_product(R, self.M, self.remainder_cache)
        K = KD.add(KR if KR is not None else empty_block(*KD.shape))
        del KD, KR
        if c.zd is not None and len(c.zd):
            K.zero_rows_cols(numpy.asarray(c.zd, dtype=numpy.int32), c.diag)
        K.ptap_route = "cells+extras"
        return K

    # -- 7: connected meshes, one dense block per element ------------------------------------------------------------
    def _elements(self, c):
        """the element-split cell-block product (tigar_amd/elemptap.py), or None when it does not apply: one field on one
        mesh whose cells hold at most 125 nodes (the cells' node lists are the dofmap of the FE space), a system large
        enough for the plan to pay (``TIGAR_PTAP_ELEMENTS=2``: any size), every entry of A between nodes of a common cell
        (what dolfin assembles on the Q_p / P_p mesh of the extraction, with an M that is used as a general CSR matrix;
        others fall through to the general kernels)"""
        n = self.M.shape[0]
        if self.nFields != 1 or not self.grids or len(self.grids) != 1 or c.A.shape != (n, n):
            return None
        if self.element_plan is None or self.element_plan[0] is not self.M:
            self.element_plan = (self.M, self._element_plan_for(self.M))
        return self.element_plan[1].ptap(c.A, c.zd, c.diag) if self.element_plan[1] is not None else None

    def _element_plan_for(self, M):
        """ElementSplitPtAP for the scalar extraction operator ``M`` on the (first) mesh of the FE space, or None"""
        switch = os.environ.get("TIGAR_PTAP_ELEMENTS", "1")
        if switch == "0" or not self.grids or (M.shape[0] < 20000 and switch != "2"):
            return None
        g = self.grids[0]
        if (int(g.degree) + 1) ** g.dim() > 125 or int(g.degree) < 1 or getattr(g, "dg", False) or g.num_nodes() != M.shape[0]:
            return None
        from .elemptap import ElementSplitPtAP, CellNodes
        try:
            return ElementSplitPtAP(M, CellNodes.from_grid(g))       # (the dofmap of V, generated on the device)
        except (ValueError, _dev.TigarHipError):
            return None

    # -- 8: any M, any A -----------------------------------------------------------------------------------------------
    def _general(self, c):
        """symbolic / numeric product of the general kernels; the symbolic plan is kept while shape and entry count of A stay"""
        A, key = c.A, (c.A.shape, c.A.nnz)
        fresh = self.general_plan is None or self.general_key != key
        if fresh:
            self.general_plan, self.general_key = _dev.ptap_symbolic(A, self.M, self.MT), key
        try:
            return _dev.ptap_numeric(self.general_plan, A, self.M, self.MT, c.zd, c.diag)
        except _dev.TigarHipError:
            if fresh and self.by_blocks:
                # rows of the whole product beyond the general kernels' per-row tables (three fields at p = 3 in 3-D):
                # the same kernels block by block, on the scalar operands
                self.general_plan = self.general_key = None
                K = self.field_blocks(A, c.zd, c.diag, tensor=False)
                if K is not None:
                    return K
            if fresh:
                raise
            # same shape and nnz but another sparsity pattern than the cached plan's: the reference
            # recomputes the symbolic product on every call (tIGAr/common.py:1194-1195) -- plan again
            self.general_plan = _dev.ptap_symbolic(A, self.M, self.MT)
            return _dev.ptap_numeric(self.general_plan, A, self.M, self.MT, c.zd, c.diag)
