"""Host reference of the volume forms with point coefficients (csrc/tg_coef.hip, the coefficient endings of
csrc/tg_postproc.hip):

    a(u, v) = int grad v . (A grad u) + (b . grad v) u + v (c . grad u) + m u v dx        (u: column, v: row)
    L(v)    = int s v + F . grad v dx

Dense loops per element and point, with the conventions of ``postproc_reference`` (equispaced Lagrange nodes,
Gauss-Legendre with nq points per direction, direction 0 fastest, points element-major, parametric gradients divided by
the element sizes).  At every point the functions psi (phi, or phi / W_h with ``rational``) and their CARTESIAN gradients
are formed directly, then the integrand as it is written above: no transformed tensor, no folding of beta, no sum
factorisation -- the kernels and the reference do not share the algebra.

``dtype``: longdouble (the reference proper) or float64 (the SAME computation in working precision, tables included:
its distance from the longdouble run is the yardstick of the GPU tests).  Also a host Newton flow with dense solves.
"""
import numpy as np

import postproc_reference as R

LD = np.longdouble
EPS = R.EPS


def tables(p, nq, dtype):
    """l[a][q], l'[a][q], w[q], the Gauss points: computed in ``dtype`` from Gauss points rounded to it"""
    t, w = R.gauss01(nq)
    t, w = t.astype(dtype), w.astype(dtype)
    nodes = np.arange(p + 1).astype(dtype) / dtype(p)
    l, dl = np.ones((p + 1, nq), dtype=dtype), np.zeros((p + 1, nq), dtype=dtype)
    for a in range(p + 1):
        others = [m for m in range(p + 1) if m != a]
        for m in others:
            l[a] = l[a] * (t - nodes[m]) / (nodes[a] - nodes[m])
        for m in others:
            term = np.full(nq, dtype(1) / (nodes[a] - nodes[m]), dtype=dtype)
            for r in others:
                if r != m:
                    term = term * (t - nodes[r]) / (nodes[a] - nodes[r])
            dl[a] = dl[a] + term
    return l, dl, w


def _inverse(g):
    """inverse and determinant of a d x d matrix, d <= 3, by cofactors (numpy.linalg has no longdouble)"""
    d = g.shape[0]
    if d == 1:
        return np.array([[1 / g[0, 0]]], dtype=g.dtype), g[0, 0]
    if d == 2:
        det = g[0, 0] * g[1, 1] - g[0, 1] * g[1, 0]
        return np.array([[g[1, 1], -g[0, 1]], [-g[1, 0], g[0, 0]]], dtype=g.dtype) / det, det
    adj = np.zeros((3, 3), dtype=g.dtype)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            c = [k for k in range(3) if k != j]
            adj[j, i] = (-1) ** (i + j) * (g[r[0], c[0]] * g[r[1], c[1]] - g[r[0], c[1]] * g[r[1], c[0]])
    det = g[0, 0] * adj[0, 0] + g[0, 1] * adj[1, 0] + g[0, 2] * adj[2, 0]
    return adj / det, det


class CoefReference(object):
    """per element and point: psi[a], its Cartesian gradient G[a][i] and the weight wdet; ``matrix``, ``load``, ``eval`` and
    the Newton flow on top of them"""

    def __init__(self, uks, p, cp, nq=None, rational=False, dtype=LD):
        self.d, self.p, self.nsd, self.dtype, self.rational = len(uks), p, len(cp) - 1, dtype, bool(rational)
        d, nsd = self.d, self.nsd
        self.nq = nq = p + 1 if nq is None else nq
        l, dl, w = tables(p, nq, dtype)
        nel = [len(u) - 1 for u in uks]
        n = [e * p + 1 for e in nel]
        p1 = p + 1
        self.nloc, self.nqt = p1 ** d, nq ** d
        loc = np.array(np.unravel_index(np.arange(self.nloc), (p1,) * d, order="F")).T
        qs = np.array(np.unravel_index(np.arange(self.nqt), (nq,) * d, order="F")).T
        cpa = [np.asarray(c, dtype=dtype) for c in cp]
        self.nnodes = int(np.prod(n))
        self.elements = []                      # (global nodes, PSI [q][a], G [q][a][i], wdet [q]) in point order
        X = []
        for e in np.ndindex(*nel[::-1]):
            el = e[::-1]
            h = [dtype(uks[k][el[k] + 1]) - dtype(uks[k][el[k]]) for k in range(d)]
            g = np.zeros(self.nloc, dtype=np.int64)
            stride = 1
            for k in range(d):
                g += stride * (el[k] * p + loc[:, k])
                stride *= n[k]
            cl = [c[g] for c in cpa]
            PSI = np.zeros((self.nqt, self.nloc), dtype=dtype)
            G = np.zeros((self.nqt, self.nloc, nsd), dtype=dtype)
            wd = np.zeros(self.nqt, dtype=dtype)
            x = np.zeros((self.nqt, nsd), dtype=dtype)
            for q in range(self.nqt):
                phi = np.ones(self.nloc, dtype=dtype)
                for k in range(d):
                    phi = phi * l[loc[:, k], qs[q, k]]
                gr = np.zeros((self.nloc, d), dtype=dtype)
                for k in range(d):
                    gk = dl[loc[:, k], qs[q, k]] / h[k]
                    for m in range(d):
                        if m != k:
                            gk = gk * l[loc[:, m], qs[q, m]]
                    gr[:, k] = gk
                N = np.array([c @ phi for c in cl], dtype=dtype)
                dN = np.array([c @ gr for c in cl], dtype=dtype)               # [c][k]
                W, dW = N[nsd], dN[nsd]
                DF = (dN[:nsd] * W - N[:nsd, None] * dW[None, :]) / (W * W)   # [i][k]
                gi, det = _inverse(DF.T @ DF)
                pinv = gi @ DF.T                                               # [k][i]
                wq = dtype(1)
                for k in range(d):
                    wq = wq * w[qs[q, k]] * h[k]
                wd[q] = wq * np.sqrt(abs(det))
                if self.rational:
                    psi = phi / W
                    gpar = gr / W - phi[:, None] * (dW / (W * W))[None, :]     # quotient rule, parametric
                else:
                    psi, gpar = phi, gr
                PSI[q], G[q] = psi, gpar @ pinv
                x[q] = N[:nsd] / W
            self.elements.append((g, PSI, G, wd))
            X.append(x)
        self.x = np.concatenate(X)
        self.npts = self.x.shape[0]

    # ---- point data: None, a constant (a number / nsd numbers), [npts] / [npts, nsd] / [npts, nsd, nsd]
    def _arr(self, v, shape):
        if v is None:
            return None
        v = np.asarray(v, dtype=self.dtype)
        return np.broadcast_to(v, (self.npts,) + shape) if (v.ndim == 0 or v.shape == shape) else v

    def matrix(self, A=None, b=None, c=None, m=None):
        """COO of the form: (sorted unique keys row * N + col, values)"""
        dt, nsd = self.dtype, self.nsd
        A = None if A is None else np.asarray(A, dtype=dt)
        if A is not None and A.ndim <= 1:                                      # isotropic
            A = np.broadcast_to(A, (self.npts,))[:, None, None] * np.eye(nsd, dtype=dt)[None]
        b, c, m = self._arr(b, (nsd,)), self._arr(c, (nsd,)), self._arr(m, ())
        keys, vals = [], []
        for i, (g, PSI, G, wd) in enumerate(self.elements):
            Ae = np.zeros((self.nloc, self.nloc), dtype=dt)
            for q in range(self.nqt):
                gq = i * self.nqt + q
                psi, Gq = PSI[q], G[q]
                t = np.zeros((self.nloc, self.nloc), dtype=dt)
                if A is not None:
                    t = t + Gq @ A[gq] @ Gq.T
                if b is not None:
                    t = t + np.outer(Gq @ b[gq], psi)
                if c is not None:
                    t = t + np.outer(psi, Gq @ c[gq])
                if m is not None:
                    t = t + m[gq] * np.outer(psi, psi)
                Ae = Ae + wd[q] * t
            keys.append((g[:, None] * self.nnodes + g[None, :]).ravel())
            vals.append(Ae.ravel())
        keys, vals = np.concatenate(keys), np.concatenate(vals)
        uk, inv = np.unique(keys, return_inverse=True)
        out = np.zeros(uk.size, dtype=dt)
        np.add.at(out, inv, vals)
        return uk, out

    def dense(self, *coefs):
        k, v = self.matrix(*coefs)
        D = np.zeros((self.nnodes, self.nnodes), dtype=self.dtype)
        D[k // self.nnodes, k % self.nnodes] = v
        return D

    def load(self, s=None, F=None):
        """b[node] = sum_q wdet_q (s_q psi_node + F_q . grad psi_node)"""
        s, F = self._arr(s, ()), self._arr(F, (self.nsd,))
        out = np.zeros(self.nnodes, dtype=self.dtype)
        for i, (g, PSI, G, wd) in enumerate(self.elements):
            be = np.zeros(self.nloc, dtype=self.dtype)
            for q in range(self.nqt):
                gq = i * self.nqt + q
                t = np.zeros(self.nloc, dtype=self.dtype)
                if s is not None:
                    t = t + s[gq] * PSI[q]
                if F is not None:
                    t = t + G[q] @ F[gq]
                be = be + wd[q] * t
            np.add.at(out, g, be)
        return out

    def eval(self, u):
        """(u at the points [npts], its Cartesian gradient [npts, nsd]) of the nodal values u (of u_h with ``rational``)"""
        u = np.asarray(u, dtype=self.dtype)
        V = np.concatenate([PSI @ u[g] for g, PSI, G, wd in self.elements])
        Gr = np.concatenate([np.einsum("qai,a->qi", G, u[g]) for g, PSI, G, wd in self.elements])
        return V, Gr

    def wdet(self):
        return np.concatenate([wd for g, PSI, G, wd in self.elements])

    def errors(self, u, exact, exact_grad):
        """(L2, H10) errors of u against the exact values / gradients at the points"""
        v, g = self.eval(u)
        w = self.wdet()
        return (float(np.sqrt(np.sum(w * (v - exact) ** 2))), float(np.sqrt(np.sum(w * np.sum((g - exact_grad) ** 2, axis=1)))))


def values_at(keys, vals, nnodes, rows, cols):
    """the reference values at the entries (rows, cols) of another pattern (0 where the reference has none), and whether
    every reference entry lies in that pattern"""
    want = rows.astype(np.int64) * nnodes + cols.astype(np.int64)
    pos = np.searchsorted(keys, want)
    pos[pos >= keys.size] = keys.size - 1
    hit = keys[pos] == want
    out = np.where(hit, vals[pos], vals.dtype.type(0))
    return out, bool(np.all(np.isin(keys[vals != 0], want)))


def newton(ref, Mc, free, residual, tangent, f=None, tol=1e-10, max_iters=25, U0=None):
    """The host Newton flow on the IGA dofs ``free`` (the others stay 0): M^T R, M^T J M dense in float64, with the control
    flow of ``solveNonlinearVariationalProblem`` -- stop when ||M^T R|| / (its first value) < tol.  ``Mc``: the extraction
    matrix (FE nodes x dofs); residual / tangent as for ``forms.QuasilinearResidual``; f: point values of the right-hand
    side.  Returns (dofs, history of the relative norms)."""
    Mc = np.asarray(Mc.todense() if hasattr(Mc, "todense") else Mc, dtype=np.float64)
    U = np.zeros(Mc.shape[1]) if U0 is None else np.array(U0, dtype=np.float64)
    x = ref.x.astype(np.float64)
    fixed = np.setdiff1d(np.arange(Mc.shape[1]), free)
    history, first = [], None
    for it in range(max_iters):
        uq, gq = ref.eval(Mc @ U)
        uq, gq = uq.astype(np.float64), gq.astype(np.float64)
        F, s = residual(x, uq, gq)
        if f is not None:
            s = (0.0 if s is None else s) - f
        Rv = Mc.T @ ref.load(s, F).astype(np.float64)
        Rv[fixed] = 0.0
        nrm = float(np.linalg.norm(Rv))
        first = nrm if first is None else first
        history.append(nrm / first)
        if history[-1] < tol:
            return U, history
        J = Mc.T @ ref.dense(*tangent(x, uq, gq)).astype(np.float64) @ Mc
        U[free] -= np.linalg.solve(J[np.ix_(free, free)], Rv[free])
    raise RuntimeError("the host Newton flow did not converge: %r" % (history,))
