"""Host reference of the quadrature-point kernels (csrc/tg_postproc.hip): a numpy element loop in ``longdouble`` with the
conventions of ``oracle.tigar_oracle.mapped_fe_system`` -- equispaced Lagrange nodes, Gauss-Legendre with nq points per
direction, direction 0 fastest, parametric gradients divided by the element sizes, weights times the element sizes.
Points are numbered element-major (elements and the points of an element lexicographic, direction 0 fastest).

Besides the values it computes the MAGNITUDES the rounding-error bounds of tests/test_gpu_postproc.py are stated in, by
first-order propagation: a nodal field at a point, sum_a u_a phi_a, has the magnitude sum_a |u_a phi_a|; a product a b of
two computed quantities with magnitudes ea, eb has |a| eb + ea |b| + |a b|; a quotient likewise.  A quantity computed in
floating point along a chain of at most c roundings then differs from the exact one by at most c eps magnitude, to first
order.  (Differences of neighbouring nodal values make the magnitudes of derivatives much larger than the derivatives on
small elements: that loss is real.)  The tables enter as |l| + DELTA |l'| and |l'| + DELTA |l''|: the Gauss abscissae of
the library are double-precision numbers (Newton iteration stopped at 1e-16 on [-1, 1]), so a table entry is the basis
function at a point up to DELTA = 4 eps away (the rounded nodes m / p of the factors t - m / p count into the same shift:
next to a node -- the Gauss point 0.33001 of nq = 4 and the node 1/3 of p = 3 -- a factor loses 40 eps of relative accuracy).
"""
import numpy as np

from oracle import tigar_oracle as O

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
DELTA = 4.0 * EPS


def gauss01(n):
    """Gauss-Legendre points / weights on [0, 1] in longdouble (numpy's double-precision points, Newton-refined)"""
    z = np.polynomial.legendre.leggauss(n)[0].astype(LD)
    for _ in range(3):
        p1, p2 = np.ones_like(z), np.zeros_like(z)
        for j in range(n):
            p1, p2 = ((2 * j + 1) * z * p1 - j * p2) / LD(j + 1), p1
        pp = n * (z * p1 - p2) / (z * z - 1)
        z = z - p1 / pp
    p1, p2 = np.ones_like(z), np.zeros_like(z)
    for j in range(n):
        p1, p2 = ((2 * j + 1) * z * p1 - j * p2) / LD(j + 1), p1
    pp = n * (z * p1 - p2) / (z * z - 1)
    return (z + 1) / 2, 1 / ((1 - z * z) * pp * pp)


def lagrange01(p, t):
    """l[a][q], l'[a][q], l''[a][q] of the equispaced Lagrange basis of degree p on [0, 1] at the points t (longdouble)"""
    nodes = np.arange(p + 1).astype(LD) / LD(p)
    out = np.zeros((3, p + 1, len(t)), dtype=LD)
    for a in range(p + 1):
        c = np.ones(1, dtype=LD)                      # coefficients, highest power first
        for m in range(p + 1):
            if m != a:
                c = np.convolve(c, np.array([1, -nodes[m]], dtype=LD)) / (nodes[a] - nodes[m])
        for k in range(3):
            v = np.zeros(len(t), dtype=LD)
            for coef in c:
                v = v * t + coef
            out[k, a] = v
            n = len(c) - 1
            c = c[:-1] * np.arange(n, 0, -1).astype(LD) if n > 0 else np.zeros(1, dtype=LD)
    return out[0], out[1], out[2]


def constants(d, p, nq, nsd, nelem=1, kappa=1.0):
    """Lengths of the longest chains of roundings in the kernels of csrc/tg_postproc.hip (the count is in the docstring of
    tests/test_gpu_postproc.py): the constants c of the bounds c eps magnitude.  ``kappa``: max wdet_mag / wdet, which
    turns the relative error of the weights into a multiple of the sums they weigh."""
    t = 6 * p + 4                                  # a table entry: p factors (t - m/p) / (a/p - m/p), p terms for l'
    cN = d * (t + p + 1)                           # a field at a point: d contractions of p + 1 fused multiply-adds
    cw, cg = cN + 16, cN + 24                      # DF 4, g nsd + 1 <= 4, det 7, sqrt 1 | inverse 4, two products d + 1 each
    tree = int(np.ceil(np.log2(max(nq ** d, 2)))) + (nelem + 255) // 256 + 8
    kw = float(kappa) * cw
    return {"val": cN, "x": cN + 2, "wdet": cw, "grad": cg, "load": cw + 1 + d * (t + nq) + 2 ** d,
            "err": (kw + 2 * cN + 4 + tree, kw + 2 * cg + nsd + 3 + tree, kw + 3 + tree)}


def _adj_det(g, eg):
    """adjugate and determinant of the symmetric d x d matrices g[q] with the magnitudes of both, given those of g"""
    d = g.shape[-1]
    adj, eadj = np.zeros_like(g), np.zeros_like(g)
    ag = abs(g)
    if d == 1:
        adj[:, 0, 0] = 1
        return adj, g[:, 0, 0].copy(), eadj, eg[:, 0, 0].copy()
    if d == 2:
        adj[:, 0, 0], adj[:, 1, 1], adj[:, 0, 1], adj[:, 1, 0] = g[:, 1, 1], g[:, 0, 0], -g[:, 0, 1], -g[:, 1, 0]
        eadj[:, 0, 0], eadj[:, 1, 1], eadj[:, 0, 1], eadj[:, 1, 0] = eg[:, 1, 1], eg[:, 0, 0], eg[:, 0, 1], eg[:, 1, 0]
        det = g[:, 0, 0] * g[:, 1, 1] - g[:, 0, 1] * g[:, 1, 0]
        edet = (ag[:, 1, 1] * eg[:, 0, 0] + ag[:, 0, 0] * eg[:, 1, 1] + ag[:, 0, 1] * eg[:, 1, 0] + ag[:, 1, 0] * eg[:, 0, 1]
                + ag[:, 0, 0] * ag[:, 1, 1] + ag[:, 0, 1] * ag[:, 1, 0])
        return adj, det, eadj, edet
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            c = [k for k in range(3) if k != j]
            adj[:, j, i] = (-1) ** (i + j) * (g[:, r[0], c[0]] * g[:, r[1], c[1]] - g[:, r[0], c[1]] * g[:, r[1], c[0]])
            eadj[:, j, i] = (ag[:, r[0], c[0]] * eg[:, r[1], c[1]] + eg[:, r[0], c[0]] * ag[:, r[1], c[1]]
                             + ag[:, r[0], c[1]] * eg[:, r[1], c[0]] + eg[:, r[0], c[1]] * ag[:, r[1], c[0]]
                             + ag[:, r[0], c[0]] * ag[:, r[1], c[1]] + ag[:, r[0], c[1]] * ag[:, r[1], c[0]])
    det = sum(g[:, 0, m] * adj[:, m, 0] for m in range(3))
    edet = sum(ag[:, 0, m] * eadj[:, m, 0] + eg[:, 0, m] * abs(adj[:, m, 0]) + ag[:, 0, m] * abs(adj[:, m, 0]) for m in range(3))
    return adj, det, eadj, edet


class Reference(object):
    """points, weights and the per-element tables of one patch; ``eval`` / ``load`` / ``sums`` on top of them"""

    def __init__(self, uks, p, cp, nq=None):
        self.d, self.p, self.nsd = len(uks), p, len(cp) - 1
        d, nsd = self.d, self.nsd
        self.nq = nq = p + 1 if nq is None else nq
        t, w = gauss01(nq)
        l, dl, d2l = lagrange01(p, t)
        ml, mdl = abs(l) + DELTA * abs(dl), abs(dl) + DELTA * abs(d2l)
        self.nel = nel = [len(u) - 1 for u in uks]
        self.n = n = [e * p + 1 for e in nel]
        p1 = p + 1
        self.nloc, self.nqt = p1 ** d, nq ** d
        loc = np.array(np.unravel_index(np.arange(self.nloc), (p1,) * d, order="F")).T
        qs = np.array(np.unravel_index(np.arange(self.nqt), (nq,) * d, order="F")).T
        cpa = [np.asarray(c, dtype=LD) for c in cp]
        self.elements = []                      # (global nodes, PH, GR, |PH|, |GR|) per element, in point order
        X, WD, XM, WM = [], [], [], []
        self._geo = []
        for e in np.ndindex(*nel[::-1]):
            el = e[::-1]
            h = [LD(uks[k][el[k] + 1]) - LD(uks[k][el[k]]) for k in range(d)]
            g = np.zeros(self.nloc, dtype=np.int64)
            stride = 1
            for k in range(d):
                g += stride * (el[k] * p + loc[:, k])
                stride *= n[k]
            PH, aPH = np.ones((self.nloc, self.nqt), dtype=LD), np.ones((self.nloc, self.nqt), dtype=LD)
            for k in range(d):
                PH = PH * l[loc[:, k]][:, qs[:, k]]
                aPH = aPH * ml[loc[:, k]][:, qs[:, k]]
            GR, aGR = np.zeros((self.nloc, self.nqt, d), dtype=LD), np.zeros((self.nloc, self.nqt, d), dtype=LD)
            for k in range(d):
                gk, agk = dl[loc[:, k]][:, qs[:, k]] / h[k], mdl[loc[:, k]][:, qs[:, k]] / h[k]
                for m in range(d):
                    if m != k:
                        gk, agk = gk * l[loc[:, m]][:, qs[:, m]], agk * ml[loc[:, m]][:, qs[:, m]]
                GR[:, :, k], aGR[:, :, k] = gk, agk
            wq = np.ones(self.nqt, dtype=LD)
            for k in range(d):
                wq = wq * w[qs[:, k]] * h[k]
            N = [cpa[c][g] @ PH for c in range(nsd + 1)]
            aN = [abs(cpa[c][g]) @ aPH for c in range(nsd + 1)]
            dN = [np.einsum("a,aqk->qk", cpa[c][g], GR) for c in range(nsd + 1)]
            adN = [np.einsum("a,aqk->qk", abs(cpa[c][g]), aGR) for c in range(nsd + 1)]
            W, aW = N[nsd], aN[nsd]
            DF = np.stack([(dN[i] * W[:, None] - N[i][:, None] * dN[nsd]) / (W * W)[:, None] for i in range(nsd)], axis=1)
            eDF = np.stack([(adN[i] * W[:, None] + abs(dN[i]) * aW[:, None] + aN[i][:, None] * abs(dN[nsd])
                             + abs(N[i])[:, None] * adN[nsd]) / (W * W)[:, None] for i in range(nsd)], axis=1) \
                + 2 * abs(DF) * (aW / W)[:, None, None]
            met = np.einsum("qik,qim->qkm", DF, DF)
            emet = np.einsum("qik,qim->qkm", eDF, abs(DF)) + np.einsum("qik,qim->qkm", abs(DF), eDF) \
                + np.einsum("qik,qim->qkm", abs(DF), abs(DF))
            adj, det, eadj, edet = _adj_det(met, emet)
            egi = eadj / abs(det)[:, None, None] + abs(adj) * (edet / det ** 2)[:, None, None]
            wd = wq * np.sqrt(abs(det))
            X.append(np.stack([N[i] / W for i in range(nsd)], axis=1))
            XM.append(np.stack([aN[i] / W + abs(N[i]) / W * (aW / W) for i in range(nsd)], axis=1))
            WD.append(wd)
            WM.append(wq * edet / (2 * np.sqrt(abs(det))) + wd)
            self.elements.append((g, PH, GR, aPH, aGR))
            self._geo.append((DF, eDF, adj / det[:, None, None], egi))
        self.x, self.x_mag = np.concatenate(X), np.concatenate(XM)
        self.wdet, self.wdet_mag = np.concatenate(WD), np.concatenate(WM)
        self.kappa = float(np.max(self.wdet_mag / self.wdet))
        self.npts = self.wdet.size
        self.nnodes = int(np.prod(n))

    def eval(self, u):
        """(values [npts], Cartesian gradient [npts, nsd], their magnitudes) of the nodal field u"""
        u = np.asarray(u, dtype=LD)
        V, G, VM, GM = [], [], [], []
        for (g, PH, GR, aPH, aGR), (DF, eDF, gi, egi) in zip(self.elements, self._geo):
            du, edu = np.einsum("a,aqk->qk", u[g], GR), np.einsum("a,aqk->qk", abs(u[g]), aGR)
            V.append(u[g] @ PH)
            VM.append(abs(u[g]) @ aPH)
            G.append(np.einsum("qik,qkm,qm->qi", DF, gi, du))
            GM.append(np.einsum("qik,qkm,qm->qi", eDF, abs(gi), abs(du)) + np.einsum("qik,qkm,qm->qi", abs(DF), egi, abs(du))
                      + np.einsum("qik,qkm,qm->qi", abs(DF), abs(gi), edu + abs(du)))
        return np.concatenate(V), np.concatenate(G), np.concatenate(VM), np.concatenate(GM)

    def plain_magnitude(self, u):
        """|u|_q = sum_a |u_a phi_a(xi_q)|"""
        u = np.asarray(u, dtype=LD)
        return np.concatenate([abs(u[g]) @ abs(PH) for (g, PH, GR, aPH, aGR) in self.elements])

    def load(self, fq):
        """(b[node] = sum_q wdet_q f_q phi_node(xi_q), its magnitude)"""
        fq = np.asarray(fq, dtype=LD)
        b, bm = np.zeros(self.nnodes, dtype=LD), np.zeros(self.nnodes, dtype=LD)
        for i, (g, PH, GR, aPH, aGR) in enumerate(self.elements):
            sl = slice(i * self.nqt, (i + 1) * self.nqt)
            np.add.at(b, g, PH @ (self.wdet[sl] * fq[sl]))
            np.add.at(bm, g, aPH @ (self.wdet_mag[sl] * abs(fq[sl])))
        return b, bm

    def sums(self, u=None, e=None, ge=None):
        """(sum wdet (u_h - e)^2, sum wdet |grad u_h - ge|^2, sum wdet e^2) and the magnitudes
        (sum wdet (|u|_q + |e_q|)^2, sum wdet sum_i (|grad u|_q,i + |ge_q,i|)^2, sum wdet e^2)"""
        zero = np.zeros(self.npts, dtype=LD)
        if u is not None:
            v, gr, _, gm = self.eval(u)
            vm = self.plain_magnitude(u)
        else:
            v, vm = zero, zero
            gr = gm = np.zeros((self.npts, self.nsd), dtype=LD)
        e = zero if e is None else np.asarray(e, dtype=LD)
        ge = np.zeros((self.npts, self.nsd), dtype=LD) if ge is None else np.asarray(ge, dtype=LD)
        w = self.wdet
        s = (np.sum(w * (v - e) ** 2), np.sum(w * np.sum((gr - ge) ** 2, axis=1)), np.sum(w * e ** 2))
        m = (np.sum(w * (vm + abs(e)) ** 2), np.sum(w * np.sum((gm + abs(ge)) ** 2, axis=1)), np.sum(w * e ** 2))
        return s, m


def oracle_load(uks, p, cp, fnodal, nq=None):
    return O.mapped_fe_system(uks, p, cp, nq=nq, fnodal=fnodal)[2]


def lagrange_nodes(uks, p):
    """coordinates of the Q_p nodes of the tensor grid, direction 0 fastest: list of d arrays"""
    ax = []
    for u in uks:
        u = np.asarray(u, dtype=np.float64)
        inner = u[:-1, None] + np.diff(u)[:, None] * (np.arange(1, p + 1) / float(p))[None, :]
        ax.append(np.concatenate([[u[0]], inner.ravel()]))
    return [g.ravel(order="F") for g in np.meshgrid(*ax, indexing="ij")]


def annulus_patch(nel):
    """(element vertices, homogeneous control functions on the FE nodes) of the quarter annulus, through the oracle"""
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    s = O.BSpline([2, 2], [kv, kv])
    uks = [np.asarray(sp1.uniqueKnots, dtype=np.float64) for sp1 in s.splines]
    Mc = O.generate_M_tensor(s)
    cp = [Mc @ Pf[:, :, i].ravel(order="F") for i in range(3)]
    return uks, cp


def volume_patch(p, nels):
    """the rational volume of geom_util.rational_volume, through the oracle"""
    from geom_util import rational_volume
    kvs, C = rational_volume(p, nels)
    s = O.BSpline([p] * 3, [list(k) for k in kvs])
    uks = [np.asarray(sp1.uniqueKnots, dtype=np.float64) for sp1 in s.splines]
    Mc = O.generate_M_tensor(s)
    return uks, [Mc @ C[..., i].ravel(order="F") for i in range(4)]


# ---- the Poisson problem on the quarter annulus of tests/test_gpu_assembly.py::test_poisson_on_nurbs_annulus_converges
def annulus_exact(x):
    r, th = np.hypot(x[:, 0], x[:, 1]), np.arctan2(x[:, 1], x[:, 0])
    return (r - 1.0) * (2.0 - r) * np.sin(2.0 * th)


def annulus_exact_grad(x):
    r, th = np.hypot(x[:, 0], x[:, 1]), np.arctan2(x[:, 1], x[:, 0])
    ur, ut = (3.0 - 2.0 * r) * np.sin(2.0 * th), 2.0 * (r - 1.0) * (2.0 - r) * np.cos(2.0 * th) / r
    return np.stack([ur * np.cos(th) - ut * np.sin(th), ur * np.sin(th) + ut * np.cos(th)], axis=1)


def annulus_rhs(x):   # -(u_rr + u_r/r + u_thth/r^2)
    r, th = np.hypot(x[:, 0], x[:, 1]), np.arctan2(x[:, 1], x[:, 0])
    return -(-2.0 + (3.0 - 2.0 * r) / r - 4.0 * (r - 1.0) * (2.0 - r) / r ** 2) * np.sin(2.0 * th)
