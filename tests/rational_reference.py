"""Host reference of the RATIONAL forms and point kernels (``rational=True``: trial and test functions psi_a = phi_a / W_h,
W_h the interpolated weight function -- the reference's ``spline.rationalize(TrialFunction(V))``,
demos/poisson/poisson-nurbs.py:121-124).

A plain element loop with the conventions of ``oracle.tigar_oracle.mapped_fe_system`` (equispaced Lagrange nodes,
Gauss-Legendre with nq points per direction, direction 0 fastest, parametric gradients divided by the element sizes).
The rational functions are formed DIRECTLY -- psi and its Cartesian gradient at every point, then the integrals -- and not
through the transformed coefficient tensor the kernels use, so that kernels and reference do not share the algebra.
Matrices in float64; ``RationalPoints`` (values at the points, loads from point values, error sums) in longdouble on top
of ``postproc_reference.Reference``.
"""
import numpy as np
import scipy.sparse as sp

from oracle import tigar_oracle as O
import postproc_reference as R

LD = np.longdouble


def _element_tables(uks, p, nq):
    d = len(uks)
    t, w = O.gauss_legendre(nq)
    phi1, dphi1 = O.lagrange_1d(p, t)
    nel = [len(u) - 1 for u in uks]
    n = [e * p + 1 for e in nel]
    p1 = p + 1
    loc = np.array(np.unravel_index(np.arange(p1 ** d), (p1,) * d, order="F")).T
    qs = np.array(np.unravel_index(np.arange(nq ** d), (nq,) * d, order="F")).T
    return d, w, phi1, dphi1, nel, n, loc, qs


def _elements(uks, p, cp, nq):
    """per element: global nodes g, psi[a][q], Cartesian gradient of psi [i][a][q], weight s[q] = w sqrt(det g), and the
    un-rationalised phi[a][q]"""
    d, w, phi1, dphi1, nel, n, loc, qs = _element_tables(uks, p, nq)
    nsd = len(cp) - 1
    nloc, nqt = loc.shape[0], qs.shape[0]
    cpa = [np.asarray(c, dtype=np.float64) for c in cp]
    for e in np.ndindex(*nel[::-1]):
        el = e[::-1]
        h = [uks[k][el[k] + 1] - uks[k][el[k]] for k in range(d)]
        g = np.zeros(nloc, dtype=np.int64)
        stride = 1
        for k in range(d):
            g += stride * (el[k] * p + loc[:, k])
            stride *= n[k]
        PH = np.ones((nloc, nqt))
        for k in range(d):
            PH = PH * phi1[loc[:, k]][:, qs[:, k]]
        GR = np.zeros((nloc, nqt, d))
        for k in range(d):
            gk = dphi1[loc[:, k]][:, qs[:, k]] / h[k]
            for m in range(d):
                if m != k:
                    gk = gk * phi1[loc[:, m]][:, qs[:, m]]
            GR[:, :, k] = gk
        wq = np.ones(nqt)
        for k in range(d):
            wq = wq * w[qs[:, k]] * h[k]
        Nv = [cpa[c][g] @ PH for c in range(nsd + 1)]
        dNv = [np.einsum("a,aqk->qk", cpa[c][g], GR) for c in range(nsd + 1)]
        W, dW = Nv[nsd], dNv[nsd]
        DF = np.stack([(dNv[i] * W[:, None] - Nv[i][:, None] * dW) / (W * W)[:, None] for i in range(nsd)], axis=1)   # [q][i][k]
        met = np.einsum("qik,qim->qkm", DF, DF)
        s = wq * np.sqrt(np.abs(np.linalg.det(met)))
        pinv = np.einsum("qkm,qim->qki", np.linalg.inv(met), DF)                    # (g^-1 DF^T)[k][i]
        PS = PH / W[None, :]                                                          # psi = phi / W
        GPS = GR / W[None, :, None] - PH[:, :, None] * (dW / (W * W)[:, None])[None, :, :]    # quotient rule, parametric
        PG = np.einsum("aqk,qki->iaq", GPS, pinv)                                     # Cartesian gradient of psi
        yield g, PS, PG, s, PH


def rational_fe_system(uks, p, cp, nq=None, fnodal=None, fq=None):
    """(Mass, Stiff, nodal load or None, point load or None) in the rational space: M_ab = int psi_a psi_b, K_ab = int grad psi_a
    . grad psi_b (Cartesian gradients), b_a = int f_h psi_a with f_h = sum_b fnodal_b phi_b the (un-rationalised) nodal
    interpolant, c_a = sum_q s_q fq_q psi_a(xi_q) for point values ``fq`` (element-major)."""
    nq = p + 1 if nq is None else nq
    N = int(np.prod([(len(u) - 1) * p + 1 for u in uks]))
    rows, cols, mv, kv = [], [], [], []
    b = np.zeros(N) if fnodal is not None else None
    c = np.zeros(N) if fq is not None else None
    for i, (g, PS, PG, s, PH) in enumerate(_elements(uks, p, cp, nq)):
        nloc, nqt = PS.shape
        rows.append(np.repeat(g, nloc))
        cols.append(np.tile(g, nloc))
        mv.append(np.einsum("q,aq,bq->ab", s, PS, PS).ravel())
        kv.append(np.einsum("q,iaq,ibq->ab", s, PG, PG).ravel())
        if b is not None:
            np.add.at(b, g, PS @ (s * (np.asarray(fnodal)[g] @ PH)))
        if c is not None:
            np.add.at(c, g, PS @ (s * np.asarray(fq)[i * nqt:(i + 1) * nqt]))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    Mm = sp.coo_matrix((np.concatenate(mv), (rows, cols)), shape=(N, N)).tocsr()
    Km = sp.coo_matrix((np.concatenate(kv), (rows, cols)), shape=(N, N)).tocsr()
    Mm.sort_indices()
    Km.sort_indices()
    return Mm, Km, b, c


def rational_elasticity_fe_system(uks, p, cp, lmbda, mu, nq=None):
    """a(u,v) = int lambda div u div v + 2 mu eps(u):eps(v) dx with every component in the rational space (nsd == d), fields
    one after the other: block (i, j) = lambda (d_i psi_a, d_j psi_b) + mu (d_j psi_a, d_i psi_b) + delta mu (grad psi_a,
    grad psi_b)"""
    d = len(uks)
    if len(cp) - 1 != d:
        raise ValueError("nsd == d")
    nq = p + 1 if nq is None else nq
    N = int(np.prod([(len(u) - 1) * p + 1 for u in uks]))
    rows, cols, vals = [], [], []
    for g, PS, PG, s, PH in _elements(uks, p, cp, nq):
        nloc = PS.shape[0]
        gg = np.einsum("maq,nbq,q->mnab", PG, PG, s)
        lap = sum(gg[k, k] for k in range(d))
        for i in range(d):
            for j in range(d):
                blk = lmbda * gg[i, j] + mu * gg[j, i] + (mu * lap if i == j else 0.0)
                rows.append(np.repeat(i * N + g, nloc))
                cols.append(np.tile(j * N + g, nloc))
                vals.append(blk.ravel())
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(d * N, d * N)).tocsr()
    A.sort_indices()
    return A


def physical_nodes(cp):
    """[nnodes, nsd] positions of the FE nodes, cp[i] / cp[nsd] (exact at the nodes: the basis is interpolatory)"""
    c = [np.asarray(v, dtype=np.float64) for v in cp]
    return np.stack([c[i] / c[-1] for i in range(len(c) - 1)], axis=1)


class RationalPoints(R.Reference):
    """``postproc_reference.Reference`` (longdouble) with the rational endings: u = u_h / W_h at the points with its Cartesian
    gradient, the load tested against phi / W_h, the error sums of u"""

    def __init__(self, uks, p, cp, nq=None):
        R.Reference.__init__(self, uks, p, cp, nq)
        self._w = np.asarray(cp[-1], dtype=LD)

    def eval_rational(self, u):
        """(u_h / W_h [npts], its Cartesian gradient [npts, nsd])"""
        u = np.asarray(u, dtype=LD)
        V, G = [], []
        for (g, PH, GR, aPH, aGR), (DF, eDF, gi, egi) in zip(self.elements, self._geo):
            W, dW = self._w[g] @ PH, np.einsum("a,aqk->qk", self._w[g], GR)
            uh, duh = u[g] @ PH, np.einsum("a,aqk->qk", u[g], GR)
            V.append(uh / W)
            du = duh / W[:, None] - (uh / (W * W))[:, None] * dW          # quotient rule
            G.append(np.einsum("qik,qkm,qm->qi", DF, gi, du))
        return np.concatenate(V), np.concatenate(G)

    def load_rational(self, fq):
        """b[node] = sum_q wdet_q f_q phi_node(xi_q) / W_h(xi_q)"""
        fq = np.asarray(fq, dtype=LD)
        b = np.zeros(self.nnodes, dtype=LD)
        for i, (g, PH, GR, aPH, aGR) in enumerate(self.elements):
            sl = slice(i * self.nqt, (i + 1) * self.nqt)
            np.add.at(b, g, PH @ (self.wdet[sl] * fq[sl] / (self._w[g] @ PH)))
        return b

    def sums_rational(self, u, e=None, ge=None):
        """(sum wdet (u - e)^2, sum wdet |grad u - ge|^2, sum wdet e^2) with u = u_h / W_h, and the SCALES the differences are
        judged by: (sum wdet (|u| + |e|)^2, sum wdet sum_i (|grad u|_i + |ge_i|)^2, sum wdet e^2)"""
        v, gr = self.eval_rational(u)
        e = np.zeros(self.npts, dtype=LD) if e is None else np.asarray(e, dtype=LD)
        ge = np.zeros((self.npts, self.nsd), dtype=LD) if ge is None else np.asarray(ge, dtype=LD)
        w = self.wdet
        s = (np.sum(w * (v - e) ** 2), np.sum(w * np.sum((gr - ge) ** 2, axis=1)), np.sum(w * e ** 2))
        m = (np.sum(w * (abs(v) + abs(e)) ** 2), np.sum(w * np.sum((abs(gr) + abs(ge)) ** 2, axis=1)), np.sum(w * e ** 2))
        return s, m


def solve_annulus_poisson(nel, nq=None, matrices=False):
    """The host flow of the rational Poisson problem on the quarter annulus (p = 2, homogeneous Dirichlet data, right-hand side
    ``postproc_reference.annulus_rhs`` at the points): returns (L2 error, H10 error) of u = u_h / W_h against
    ``annulus_exact``, same quadrature for the system and the norms, scipy direct solve.  ``matrices``: also the extracted
    stiffness and mass matrices on the free dofs and the right-hand side there."""
    import scipy.sparse.linalg as spl
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    s = O.BSpline([2, 2], [kv, kv])
    uks = [np.asarray(s1.uniqueKnots, dtype=np.float64) for s1 in s.splines]
    Mc = O.generate_M_tensor(s)
    cp = [np.asarray(Mc @ Pf[:, :, i].ravel(order="F")) for i in range(3)]
    pts = RationalPoints(uks, 2, cp, nq)
    x = np.asarray(pts.x, dtype=np.float64)
    Mr, Kr, _, b = rational_fe_system(uks, 2, cp, nq=nq, fq=R.annulus_rhs(x))
    ncp = Mc.shape[1]
    n1 = int(round(np.sqrt(ncp)))
    idx = np.arange(ncp).reshape(n1, n1, order="F")
    bd = np.unique(np.concatenate([idx[0], idx[-1], idx[:, 0], idx[:, -1]]))
    free = np.setdiff1d(np.arange(ncp), bd)
    K = (Mc.T @ Kr @ Mc).tocsr()
    U = np.zeros(ncp)
    Kf, bf = K[free][:, free].tocsc(), (Mc.T @ b)[free]
    U[free] = spl.spsolve(Kf, bf)
    (s0, s1, _), _ = pts.sums_rational(Mc @ U, R.annulus_exact(x), R.annulus_exact_grad(x))
    if matrices:
        return float(np.sqrt(s0)), float(np.sqrt(s1)), Kf, (Mc.T @ Mr @ Mc).tocsr()[free][:, free], bf
    return float(np.sqrt(s0)), float(np.sqrt(s1))
