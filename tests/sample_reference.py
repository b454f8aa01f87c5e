"""Host reference of the point kernels of csrc/tg_sample.hip in numpy ``longdouble``: evaluation at parametric points the
caller chooses and the closest-point iteration, with the magnitudes the rounding-error bounds of tests/test_gpu_sample.py are
stated in (first-order propagation, the conventions of tests/postproc_reference.py).

Evaluation: phi, phi / W_h, F, DF, g and the gradients are formed directly at every given xi -- the point's element by the
location rule (largest e <= nel - 1 with v[e] <= xi, exact comparisons), its own local coordinate t = (xi - v[e]) / h and its
own values of the 1-D Lagrange functions (product forms: the expanded polynomials of ``postproc_reference.lagrange01``
lose 1e-14 at p = 8); no table is shared between points.  Because the kernel's t carries the rounding
of (xi - v) / h, each 1-D value enters the magnitudes as |l| + delta |l'| (and |l'| + delta |l''|) with
delta = 4 eps (|xi_k| + |v_e|) / h_k, on top of the DELTA = 4 eps of the rounded nodes m / p.

``locate`` is the iteration of ``tg_point_locate`` as include/tigar_hip.h pins it, in longdouble (the slack of the decrease
test keeps the double-precision eps: it is part of the algorithm).

``lattice_reference`` is ``postproc_reference.Reference`` with the caller's abscissae in the place of the Gauss points.
"""
import numpy as np

import postproc_reference as R
from postproc_reference import lagrange01, annulus_patch, volume_patch, _adj_det   # noqa: F401

LD = np.longdouble
EPS = R.EPS
DELTA = R.DELTA
MAX_HALVINGS = 10
SINGULAR = 1e-20
SLACK = 32.0


def lagrange_products(p, t):
    """l[a][q], l'[a][q], l''[a][q] of the equispaced Lagrange basis at the points t in longdouble, by the PRODUCT forms
    (``postproc_reference.lagrange01`` expands the polynomials, which loses 1e-14 at p = 8: too much for a pointwise bound)"""
    t = np.asarray(t, dtype=LD)
    z = t * LD(p)                                         # integer nodes
    out = np.zeros((3, p + 1, len(t)), dtype=LD)
    f = [z - LD(m) for m in range(p + 1)]
    for a in range(p + 1):
        others = [m for m in range(p + 1) if m != a]
        den = LD(1)
        for m in others:
            den = den * LD(a - m)
        l, dl, d2l = np.ones(len(t), dtype=LD), np.zeros(len(t), dtype=LD), np.zeros(len(t), dtype=LD)
        for m in others:
            l = l * f[m]
            term = np.ones(len(t), dtype=LD)
            for r in others:
                if r != m:
                    term = term * f[r]
            dl = dl + term
            for r in others:
                if r == m:
                    continue
                term2 = np.ones(len(t), dtype=LD)
                for q in others:
                    if q != m and q != r:
                        term2 = term2 * f[q]
                d2l = d2l + term2
        out[0, a], out[1, a], out[2, a] = l / den, dl * LD(p) / den, d2l * LD(p) ** 2 / den
    return out[0], out[1], out[2]


def constants(d, p, nsd):
    """Lengths of the longest chains of roundings of k_point_eval (the count is in the docstring of tests/test_gpu_sample.py)"""
    t = 7 * p + 4
    cN = d * (t + p + 1)
    return {"val": cN, "x": cN + 2, "grad": cN + 24, "val_rational": cN + 2, "grad_rational": cN + 30}


def element_of(v, xi):
    """(inside, e) of the location rule for the coordinates xi along one direction with the vertices v"""
    v = np.asarray(v, dtype=np.float64)
    xi = np.asarray(xi, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (xi >= v[0]) & (xi <= v[-1])
    e = np.clip(np.searchsorted(v, np.where(inside, xi, v[0]), side="right") - 1, 0, len(v) - 2)
    return inside, e


class Patch(object):
    def __init__(self, uks, p, cp):
        self.uks = [np.asarray(u, dtype=np.float64) for u in uks]
        self.p, self.d, self.nsd = p, len(uks), len(cp) - 1
        self.cp = [np.asarray(c, dtype=LD) for c in cp]
        self.nel = [len(u) - 1 for u in self.uks]
        self.n = [e * p + 1 for e in self.nel]
        self.nnodes = int(np.prod(self.n))
        self.loc = np.array(np.unravel_index(np.arange((p + 1) ** self.d), (p + 1,) * self.d, order="F")).T

    def inside(self, xi):
        xi = np.asarray(xi, dtype=np.float64).reshape(-1, self.d)
        ok = np.ones(len(xi), dtype=bool)
        for k in range(self.d):
            ok &= element_of(self.uks[k], xi[:, k])[0]
        return ok

    def _basis(self, xi):
        """nodes [n, nloc], phi, its magnitude, grad_xi phi [n, nloc, d], its magnitude at the inside points xi [n, d]"""
        p, d = self.p, self.d
        n = len(xi)
        g = np.zeros((n, len(self.loc)), dtype=np.int64)
        PH, aPH = np.ones((n, len(self.loc)), dtype=LD), np.ones((n, len(self.loc)), dtype=LD)
        l1, m1, dl1, md1 = [], [], [], []
        stride = 1
        for k in range(d):
            v = self.uks[k]
            _, e = element_of(v, xi[:, k])
            h = LD(1) * v[e + 1] - v[e]
            t = (xi[:, k].astype(LD) - v[e]) / h
            l, dl, d2l = lagrange_products(p, t)                # [p + 1, n]: every point has its own column
            delta = DELTA + 4.0 * EPS * (abs(xi[:, k]) + abs(v[e])) / h.astype(np.float64)
            l1.append(l.T[:, self.loc[:, k]])
            m1.append((abs(l) + delta * abs(dl)).T[:, self.loc[:, k]])
            dl1.append((dl / h).T[:, self.loc[:, k]])
            md1.append(((abs(dl) + delta * abs(d2l)) / h).T[:, self.loc[:, k]])
            g += stride * (e[:, None] * p + self.loc[None, :, k])
            stride *= self.n[k]
        GR, aGR = np.zeros((n, len(self.loc), d), dtype=LD), np.zeros((n, len(self.loc), d), dtype=LD)
        for k in range(d):
            PH, aPH = PH * l1[k], aPH * m1[k]
            gk, agk = dl1[k], md1[k]
            for m in range(d):
                if m != k:
                    gk, agk = gk * l1[m], agk * m1[m]
            GR[:, :, k], aGR[:, :, k] = gk, agk
        return g, PH, aPH, GR, aGR

    def eval(self, xi, us=None, rational=False):
        """x, values [npts, nF] and Cartesian gradients [npts, nF, nsd] at xi [npts, d] with their magnitudes (``*_mag``);
        NaN at the points that are not inside (``inside``)"""
        xi = np.asarray(xi, dtype=np.float64).reshape(-1, self.d)
        d, nsd = self.d, self.nsd
        ok = self.inside(xi)
        nF = 0 if us is None else len(us)
        out = {"inside": ok}
        for name, shape in (("x", (nsd,)), ("val", (nF,)), ("grad", (nF, nsd))):
            out[name] = np.full((len(xi),) + shape, np.nan, dtype=LD)
            out[name + "_mag"] = np.full((len(xi),) + shape, np.nan, dtype=LD)
        if not ok.any():
            return out
        g, PH, aPH, GR, aGR = self._basis(xi[ok])
        N = [np.einsum("qa,qa->q", self.cp[c][g], PH) for c in range(nsd + 1)]
        aN = [np.einsum("qa,qa->q", abs(self.cp[c][g]), aPH) for c in range(nsd + 1)]
        dN = [np.einsum("qa,qak->qk", self.cp[c][g], GR) for c in range(nsd + 1)]
        adN = [np.einsum("qa,qak->qk", abs(self.cp[c][g]), aGR) for c in range(nsd + 1)]
        W, aW, dW, adW = N[nsd], aN[nsd], dN[nsd], adN[nsd]

        def quotient(Ni, aNi, dNi, adNi):
            """d (N / W): value and magnitude, the expression of the kernels"""
            D = (dNi * W[:, None] - Ni[:, None] * dW) / (W * W)[:, None]
            eD = (adNi * W[:, None] + abs(dNi) * aW[:, None] + aNi[:, None] * abs(dW) + abs(Ni)[:, None] * adW) / (W * W)[:, None] \
                + 2 * abs(D) * (aW / W)[:, None]
            return D, eD
        DFs = [quotient(N[i], aN[i], dN[i], adN[i]) for i in range(nsd)]
        DF, eDF = np.stack([a for a, _ in DFs], axis=1), np.stack([b for _, b in DFs], axis=1)
        met = np.einsum("qik,qim->qkm", DF, DF)
        emet = np.einsum("qik,qim->qkm", eDF, abs(DF)) + np.einsum("qik,qim->qkm", abs(DF), eDF) \
            + np.einsum("qik,qim->qkm", abs(DF), abs(DF))
        adj, det, eadj, edet = _adj_det(met, emet)
        gi = adj / det[:, None, None]
        egi = eadj / abs(det)[:, None, None] + abs(adj) * (edet / det ** 2)[:, None, None]
        out["x"][ok] = np.stack([N[i] / W for i in range(nsd)], axis=1)
        out["x_mag"][ok] = np.stack([aN[i] / W + abs(N[i]) / W * (aW / W) for i in range(nsd)], axis=1)
        out["DF"], out["gi"] = DF, gi
        for i in range(nF):
            u = np.asarray(us[i], dtype=LD)
            U, aU = np.einsum("qa,qa->q", u[g], PH), np.einsum("qa,qa->q", abs(u[g]), aPH)
            du, edu = np.einsum("qa,qak->qk", u[g], GR), np.einsum("qa,qak->qk", abs(u[g]), aGR)
            if rational:
                du, edu = quotient(U, aU, du, edu)
                U, aU = U / W, aU / W + abs(U) / W * (aW / W)
            out["val"][ok, i], out["val_mag"][ok, i] = U, aU
            out["grad"][ok, i] = np.einsum("qik,qkm,qm->qi", DF, gi, du)
            out["grad_mag"][ok, i] = np.einsum("qik,qkm,qm->qi", eDF, abs(gi), abs(du)) \
                + np.einsum("qik,qkm,qm->qi", abs(DF), egi, abs(du)) + np.einsum("qik,qkm,qm->qi", abs(DF), abs(gi), edu + abs(du))
        return out

    # ---- the closest-point iteration
    def _map(self, xi):
        """F [nsd] and d F / d xi [nsd, d] at one point of the box (longdouble)"""
        g, PH, _, GR, _ = self._basis_ld(xi)
        N = [self.cp[c][g] @ PH for c in range(self.nsd + 1)]
        dN = [self.cp[c][g] @ GR for c in range(self.nsd + 1)]
        W = N[self.nsd]
        X = np.array([N[i] / W for i in range(self.nsd)], dtype=LD)
        DF = np.array([(dN[i] * W - N[i] * dN[self.nsd]) / (W * W) for i in range(self.nsd)], dtype=LD)
        return X, DF

    def _basis_ld(self, xi):
        """nodes [nloc], phi [nloc], grad_xi phi [nloc, d] at one longdouble point"""
        p, d = self.p, self.d
        nodes = np.arange(p + 1).astype(LD) / LD(p)
        ls, dls, es = [], [], []
        for k in range(d):
            v = self.uks[k]
            e = int(np.clip(np.searchsorted(v.astype(LD), xi[k], side="right") - 1, 0, len(v) - 2))
            h = LD(v[e + 1]) - LD(v[e])
            t = (xi[k] - LD(v[e])) / h
            l, dl = np.ones(p + 1, dtype=LD), np.zeros(p + 1, dtype=LD)
            for a in range(p + 1):
                den = LD(1)
                for m in range(p + 1):
                    if m == a:
                        continue
                    den *= nodes[a] - nodes[m]
                    l[a] *= t - nodes[m]
                    term = LD(1)
                    for r in range(p + 1):
                        if r != a and r != m:
                            term *= t - nodes[r]
                    dl[a] += term
                l[a] /= den
                dl[a] /= den * h
            ls.append(l)
            dls.append(dl)
            es.append(e)
        g = np.zeros(len(self.loc), dtype=np.int64)
        stride = 1
        PH = np.ones(len(self.loc), dtype=LD)
        GR = np.ones((len(self.loc), d), dtype=LD)
        for k in range(d):
            g += stride * (es[k] * p + self.loc[:, k])
            stride *= self.n[k]
            PH = PH * ls[k][self.loc[:, k]]
            for m in range(d):
                GR[:, m] = GR[:, m] * (dls[k] if m == k else ls[k])[self.loc[:, k]]
        return g, PH, None, GR, None

    def seed_strides(self, max_seeds):
        stride, count = [1] * self.d, list(self.nel)
        while int(np.prod(count)) > max_seeds:
            k = int(np.argmax(count))                           # (the first of the largest)
            stride[k] += 1
            count[k] = -(-self.nel[k] // stride[k])
        return stride, count

    def seeds(self, max_seeds):
        """(parametric centres [ns, d], physical centres [ns, nsd]) of the seed elements, direction 0 fastest"""
        stride, count = self.seed_strides(max_seeds)
        ax = [0.5 * (self.uks[k][::stride[k]][:count[k]] + self.uks[k][1::stride[k]][:count[k]]) for k in range(self.d)]
        xi = np.stack([a.ravel(order="F") for a in np.meshgrid(*ax, indexing="ij")], axis=1)
        return xi, self.eval(xi)["x"]

    def _residual(self, x, X):
        r = x - X
        e = LD(SLACK * EPS) * (abs(x) + abs(X))
        return r, np.sum(r * r), np.sum(e * (2 * abs(r) + e))

    def locate_one(self, x, xi0, tol, max_iter):
        """(xi, distance, iterations, status, rho, rows): rho the ratio of the last two steps (0 with fewer than two), rows
        the row norms |(DF^T DF)^-1 DF^T|_k at xi (None when singular)"""
        d = self.d
        x = np.asarray(x, dtype=LD)
        if not (np.all(np.isfinite(x.astype(np.float64))) and np.all(np.isfinite(np.asarray(xi0, dtype=np.float64)))):
            return np.full(d, np.nan), np.nan, 0, 2, 0.0, None
        lo = np.array([u[0] for u in self.uks], dtype=LD)
        hi = np.array([u[-1] for u in self.uks], dtype=LD)
        rng = hi - lo
        xi = np.clip(np.asarray(xi0, dtype=LD), lo, hi)
        X, DF = self._map(xi)
        r, f, _ = self._residual(x, X)
        status, iters, steps = 1, 0, []
        for it in range(1, max_iter + 1):
            iters = it
            gh = (DF.T @ r) * rng
            held = ((xi <= lo) & (gh < 0)) | ((xi >= hi) & (gh > 0))
            free = ~held
            Gh = (DF.T @ DF) * np.outer(rng, rng)
            Gh[held, :] = 0
            Gh[:, held] = 0
            gmax = max([Gh[k, k] for k in range(d)])
            dx = np.zeros(d, dtype=LD)
            if free.any():
                for k in np.nonzero(held)[0]:
                    Gh[k, k] = gmax
                gh[held] = 0
                det = _det_ld(Gh)
                if not (det > LD(SINGULAR) * gmax ** d) or not np.isfinite(float(gmax)):
                    status = 3
                    break
                dx = _solve_ld(Gh, gh) * rng
            xt = np.clip(xi + dx, lo, hi)
            step = np.max(abs(xt - xi) / rng)
            steps.append(float(step))
            if step <= tol:
                xi = xt
                X, DF = self._map(xi)
                r, f, _ = self._residual(x, X)
                status = 0
                break
            lam, taken = LD(1), False
            for hv in range(MAX_HALVINGS + 1):
                Xt, DFt = self._map(xt)
                rt, ft, slack = self._residual(x, Xt)
                if ft <= f + slack:
                    taken = True
                    break
                lam = lam / 2
                xt = np.clip(xi + lam * dx, lo, hi)
            if not taken:
                break
            xi, X, DF, r, f = xt, Xt, DFt, rt, ft
        rho = steps[-1] / steps[-2] if len(steps) >= 2 and steps[-2] > 0 else 0.0
        rows = None
        if status != 3:
            try:
                A = np.linalg.pinv(DF.astype(np.float64))
                rows = np.sqrt(np.sum(A * A, axis=1))
            except np.linalg.LinAlgError:
                rows = None
        return xi, np.sqrt(f), iters, status, rho, rows

    def locate(self, x, guess=None, tol=1e-12, max_iter=50, max_seeds=32768):
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.nsd)
        if guess is None:
            sxi, sx = self.seeds(max_seeds)
            sx = sx.astype(np.float64)
        res = []
        for q in range(len(x)):
            if guess is not None:
                xi0 = np.asarray(guess, dtype=np.float64).reshape(-1, self.d)[q]
            elif np.all(np.isfinite(x[q])):
                d2 = np.zeros(len(sx))
                for c in range(self.nsd):
                    d2 = d2 + (x[q, c] - sx[:, c]) ** 2
                xi0 = sxi[int(np.argmin(d2))]                   # (argmin: the first of the smallest)
            else:
                xi0 = np.zeros(self.d)
            res.append(self.locate_one(x[q], xi0, tol, max_iter))
        return res


def _det_ld(G):
    if len(G) == 1:
        return G[0, 0]
    if len(G) == 2:
        return G[0, 0] * G[1, 1] - G[0, 1] * G[1, 0]
    return (G[0, 0] * (G[1, 1] * G[2, 2] - G[1, 2] * G[2, 1]) - G[0, 1] * (G[1, 0] * G[2, 2] - G[1, 2] * G[2, 0])
            + G[0, 2] * (G[1, 0] * G[2, 1] - G[1, 1] * G[2, 0]))


def _solve_ld(A, b):
    """A^-1 b for a small symmetric positive definite matrix in longdouble (Gaussian elimination without pivoting)"""
    A, b = A.copy(), b.copy()
    n = len(b)
    for i in range(n):
        for j in range(i + 1, n):
            f = A[j, i] / A[i, i]
            A[j, i:] -= f * A[i, i:]
            b[j] -= f * b[i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def lattice_reference(uks, p, cp, t):
    """``postproc_reference.Reference`` on the lattice of the abscissae t (the weights are 1: not an output of the lattice
    entry points)"""
    saved = R.gauss01
    R.gauss01 = lambda n: (np.asarray(t, dtype=LD), np.ones(n, dtype=LD))
    try:
        return R.Reference(uks, p, cp, len(t))
    finally:
        R.gauss01 = saved


def lattice_xi(uks, t):
    """the parametric coordinates [npts, d] of the lattice points, numbered as tg_lattice_points"""
    t = np.asarray(t, dtype=np.float64)
    ax = [(np.asarray(u)[:-1, None] + np.diff(u)[:, None] * t[None, :]) for u in uks]         # [nel_k, m]
    d, m = len(uks), len(t)
    nel = [len(u) - 1 for u in uks]
    out = []
    for e in np.ndindex(*nel[::-1]):
        el = e[::-1]
        for q in np.ndindex(*([m] * d)[::-1]):
            ql = q[::-1]
            out.append([ax[k][el[k], ql[k]] for k in range(d)])
    return np.array(out, dtype=np.float64).reshape(-1, d)
