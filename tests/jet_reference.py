"""Host reference of the second-derivative point forms (csrc/tg_jet.hip, ``forms.JetCoefficientForm`` /
``VectorJetCoefficientForm`` / ``JetLoadForm`` / ``VectorJetLoadForm``, ``evaluateJetsAtQuadrature``):

    jet(f) = (f | f_,0 f_,1 | f_,00 f_,01 f_,11)      derivatives in the patch's parametric (knot) coordinates xi
    a(u, v) = sum_q wdet_q sum_ij jet(v_i)^T T_ij jet(u_j)          (u: column, v: row; dofs field after field)
    L(v)    = sum_q wdet_q sum_i s_i . jet(v_i)

Dense numpy loops per element and point.  The functions psi_a (phi_a, or phi_a / W_h with ``rational``), the geometry
x = N / W and their xi-derivatives are formed DIRECTLY: the 1-D Lagrange derivatives divided by the element sizes, and the
quotient rule applied to the functions themselves (psi W = phi differentiated once and twice).  No Q matrix, no transformed
coefficients, no sum factorisation.  d = 1, 2; nsd >= d.

``dtype``: longdouble (the reference proper) or float64 (the SAME computation in working precision: its distance from the
longdouble run is the yardstick of the GPU tests).
"""
import numpy as np

import postproc_reference as R

LD = np.longdouble
EPS = R.EPS
SLOTS = {1: ((0, 0),), 2: ((0, 0), (0, 1), (1, 1))}       # second derivatives, k <= m


def jet_size(d):
    return 1 + d + len(SLOTS[d])


def _quotient(f, W):
    """jet of f / W from the jets f, W [..., nJ] (any leading shape; W broadcast): psi W = f differentiated"""
    nJ = f.shape[-1]
    d = 1 if nJ == 3 else 2
    out = np.empty(np.broadcast(f, W).shape, dtype=f.dtype)
    w = W[..., 0]
    out[..., 0] = f[..., 0] / w
    for k in range(d):
        out[..., 1 + k] = (f[..., 1 + k] - out[..., 0] * W[..., 1 + k]) / w
    for s, (k, m) in enumerate(SLOTS[d]):
        out[..., 1 + d + s] = (f[..., 1 + d + s] - out[..., 1 + k] * W[..., 1 + m] - out[..., 1 + m] * W[..., 1 + k]
                               - out[..., 0] * W[..., 1 + d + s]) / w
    return out


class JetReference(object):
    def __init__(self, uks, p, cp, nq=None, rational=False, dtype=LD):
        self.d, self.p, self.nsd, self.dtype, self.rational = len(uks), p, len(cp) - 1, dtype, bool(rational)
        d, nsd = self.d, self.nsd
        if d not in (1, 2):
            raise ValueError("d = 1, 2")
        self.nJ = nJ = jet_size(d)
        self.nq = nq = p + 1 if nq is None else nq
        t, w = R.gauss01(nq)
        tabs = [a.astype(dtype) for a in R.lagrange01(p, t)]                 # l, l', l'' [a][q]
        w = w.astype(dtype)
        self.nel = nel = [len(u) - 1 for u in uks]
        self.n = n = [e * p + 1 for e in nel]
        p1 = p + 1
        self.nloc, self.nqt = p1 ** d, nq ** d
        loc = np.array(np.unravel_index(np.arange(self.nloc), (p1,) * d, order="F")).T
        qs = np.array(np.unravel_index(np.arange(self.nqt), (nq,) * d, order="F")).T
        cpa = [np.asarray(c).astype(dtype) for c in cp]
        self.nnodes = int(np.prod(n))
        self.elements = []                         # (global nodes, PSI [a, q, nJ]) per element, in point order
        X, WD, XJ = [], [], []
        for e in np.ndindex(*nel[::-1]):
            el = e[::-1]
            h = [dtype(uks[k][el[k] + 1]) - dtype(uks[k][el[k]]) for k in range(d)]
            g = np.zeros(self.nloc, dtype=np.int64)
            stride = 1
            for k in range(d):
                g += stride * (el[k] * p + loc[:, k])
                stride *= n[k]

            def deriv(orders):
                """prod_k l^(orders[k])_k / h_k^orders[k] for all (a, q)"""
                out = np.ones((self.nloc, self.nqt), dtype=dtype)
                for k in range(d):
                    out = out * tabs[orders[k]][loc[:, k]][:, qs[:, k]] / h[k] ** orders[k]
                return out
            PH = np.empty((self.nloc, self.nqt, nJ), dtype=dtype)
            PH[:, :, 0] = deriv([0] * d)
            for k in range(d):
                PH[:, :, 1 + k] = deriv([1 if m == k else 0 for m in range(d)])
            for s, (k, m) in enumerate(SLOTS[d]):
                PH[:, :, 1 + d + s] = deriv([(1 if r == k else 0) + (1 if r == m else 0) for r in range(d)])
            N = [np.einsum("a,aqj->qj", cpa[c][g], PH) for c in range(nsd + 1)]          # jets of the homogeneous functions
            xj = np.stack([_quotient(N[c], N[nsd]) for c in range(nsd)], axis=1)       # [q, nsd, nJ]
            DF = xj[:, :, 1:1 + d]
            met = np.einsum("qik,qim->qkm", DF, DF)
            det = met[:, 0, 0] if d == 1 else met[:, 0, 0] * met[:, 1, 1] - met[:, 0, 1] * met[:, 1, 0]
            wq = np.ones(self.nqt, dtype=dtype)
            for k in range(d):
                wq = wq * w[qs[:, k]] * h[k]
            PSI = _quotient(PH, N[nsd][None, :, :]) if self.rational else PH
            self.elements.append((g, PSI))
            X.append(xj[:, :, 0])
            XJ.append(xj)
            WD.append(wq * np.sqrt(abs(det)))
        self.x, self.wdet, self.xjet = np.concatenate(X), np.concatenate(WD), np.concatenate(XJ)
        self.npts = self.wdet.size

    def geometry_jets(self):
        """[npts, nsd, nJ]"""
        return self.xjet

    def jets(self, u):
        """[npts, nJ] of the nodal field u (rational: of u_h / W_h)"""
        u = np.asarray(u).astype(self.dtype)
        return np.concatenate([np.einsum("a,aqj->qj", u[g], PSI) for g, PSI in self.elements])

    def field_jets(self, u, nF):
        """[npts, nF, nJ] of nF fields, field after field"""
        u = np.asarray(u).astype(self.dtype).reshape(nF, self.nnodes)
        return np.stack([self.jets(ui) for ui in u], axis=1)

    def matrix(self, T):
        """dense [nF n, nF n] of T [npts, nF, nJ, nF, nJ] (or [npts, nJ, nJ], nF = 1)"""
        T = np.asarray(T).astype(self.dtype)
        if T.ndim == 3:
            T = T[:, None, :, None, :]
        nF, n = T.shape[1], self.nnodes
        K = np.zeros((nF, n, nF, n), dtype=self.dtype)
        for e, (g, PSI) in enumerate(self.elements):
            sl = slice(e * self.nqt, (e + 1) * self.nqt)
            Ke = np.einsum("q,aqA,qiAjB,bqB->iajb", self.wdet[sl], PSI, T[sl], PSI)
            K[np.ix_(range(nF), g, range(nF), g)] += Ke
        return K.reshape(nF * n, nF * n)

    def load(self, s):
        """[nF n] of s [npts, nF, nJ] (or [npts, nJ], nF = 1)"""
        s = np.asarray(s).astype(self.dtype)
        if s.ndim == 2:
            s = s[:, None, :]
        nF = s.shape[1]
        b = np.zeros((nF, self.nnodes), dtype=self.dtype)
        for e, (g, PSI) in enumerate(self.elements):
            sl = slice(e * self.nqt, (e + 1) * self.nqt)
            b[:, g] += np.einsum("q,aqA,qiA->ia", self.wdet[sl], PSI, s[sl])
        return b.ravel()


# ---- patches of the tests: element vertices and the homogeneous control functions on the Q_p nodes -----------------------------
def nonuniform_vertices(nels, p, seed=0):
    """non-uniform element vertices (the generator of tests/test_gpu_coef.py): S is no multiple of the identity"""
    d = len(nels)
    rng = np.random.default_rng(7 * d + p + seed)
    uks = []
    for k in range(d):
        steps = rng.uniform(0.6, 1.4, nels[k])
        uks.append(np.concatenate([[0.0], np.cumsum(steps) / np.sum(steps) * (1.0 + 0.5 * k)]))
    return uks


def polynomial_patch(nels, p, nsd, weighted=True):
    """a polynomial map of degree <= min(p, 2) per direction and a weight that varies by a third (``weighted``), given on the
    Q_p nodes; nsd > d: a curve / doubly curved surface in space"""
    uks = nonuniform_vertices(nels, p)
    X = R.lagrange_nodes(uks, p)
    d = len(nels)
    q = 2 if p >= 2 else 1
    wgt = 1.0 + (0.3 * X[0] * X[-1] + 0.1 * X[0] ** q if weighted else 0.0 * X[0])
    coords = [X[i] + 0.1 * X[(i + 1) % d] ** q for i in range(d)]
    for extra in range(d, nsd):
        coords.append(0.4 * X[0] ** q - 0.3 * X[-1] ** q + 0.2 * (extra - d + 1) * X[0] * X[-1] if d == 2 else
                      0.5 * X[0] ** q + (extra - d) * X[0])
    return uks, [c * wgt for c in coords] + [wgt]


def _arc_homogeneous(t):
    """the exact quarter circle of radius 1 as a rational quadratic in t in [0, 1]: (w x, w y, w)"""
    w = 1.0 / np.sqrt(2.0)
    b = np.stack([(1 - t) ** 2, 2 * t * (1 - t), t ** 2])
    return b[0] + b[1] * w, b[1] * w + b[2], b[0] + b[1] * w + b[2]       # control points (1,0), (1,1), (0,1), weights 1, w, 1


def annulus_patch(nels, p=2):
    """the exact quarter annulus 1 <= r <= 2 (rational; direction 0 radial, direction 1 the arc of
    geom_util.quarter_annulus) on non-uniform elements: its homogeneous coordinates are quadratics, which the Q_p nodal
    interpolation, p >= 2, reproduces"""
    assert p >= 2
    uks = nonuniform_vertices(nels, p)
    uks = [u / u[-1] for u in uks]
    X = R.lagrange_nodes(uks, p)
    wx, wy, w = _arc_homogeneous(X[1])
    r = 1.0 + X[0]
    return uks, [r * wx, r * wy, w]


def cylinder_patch(nels, p=2, length=1.5, radius=1.0):
    """the quarter-cylinder surface in space (rational): the arc times a line along z; direction 0 the arc, direction 1 z"""
    assert p >= 2
    uks = nonuniform_vertices(nels, p)
    uks = [u / u[-1] for u in uks]
    X = R.lagrange_nodes(uks, p)
    wx, wy, w = _arc_homogeneous(X[0])
    return uks, [radius * wx, radius * wy, w * length * X[1], w]
