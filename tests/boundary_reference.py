"""Host reference of the boundary kernels (csrc/tg_boundary.hip) in numpy longdouble.

Per boundary element and face Gauss point it forms phi, phi / W_h, F, DF, g, n, wsurf and d_n DIRECTLY by dense loops over
all (p+1)^d local functions: no sum factorisation, no use of the Kronecker delta of the normal direction, and d_n phi as the
Cartesian gradient DF g^-1 grad_xi phi dotted with the unit normal, not through the (g^-1 N).grad_xi shortcut of the kernel.
The surface weight is the square root of the determinant of the tangential block of the metric, which the kernel writes as
sqrt(det g (g^-1)_kk).  Coordinates of the reference element [0,1]^d, as in the kernel: no element size appears.

A face is (direction k, side s); its face elements are lexicographic in the remaining directions with the lower direction
fastest, the nq^(d-1) points of one likewise; node numbering of the tensor grid with direction 0 fastest.
"""
import numpy as np

from postproc_reference import LD, EPS, gauss01, lagrange01   # noqa: F401  (EPS is re-exported for the tests)


def _det_small(m):
    """determinant of a [.., k, k] array, k = 1, 2"""
    if m.shape[-1] == 1:
        return m[..., 0, 0]
    return m[..., 0, 0] * m[..., 1, 1] - m[..., 0, 1] * m[..., 1, 0]


def _inv(m):
    """inverse of [.., d, d] symmetric positive definite longdouble matrices by Gauss-Jordan (numpy.linalg has no longdouble)"""
    d = m.shape[-1]
    a = np.concatenate([m.copy(), np.broadcast_to(np.eye(d, dtype=LD), m.shape).copy()], axis=-1)
    for i in range(d):
        a[..., i, :] = a[..., i, :] / a[..., i, i][..., None]
        for j in range(d):
            if j != i:
                a[..., j, :] = a[..., j, :] - a[..., j, i][..., None] * a[..., i, :]
    return a[..., d:]


class FaceReference(object):
    def __init__(self, uks, p, cp, direction, side, nq=None):
        self.d, self.p, self.nsd = d, _, nsd = len(uks), p, len(cp) - 1
        self.k, self.side = k, side = int(direction), int(side)
        self.nq = nq = p + 1 if nq is None else nq
        t, w = gauss01(nq)
        end = np.array([LD(side)])
        l, dl, _ = lagrange01(p, t)
        le, dle, _ = lagrange01(p, end)
        self.nel = nel = [len(u) - 1 for u in uks]
        self.n = n = [e * p + 1 for e in nel]
        self.nnodes = int(np.prod(n))
        p1 = p + 1
        tang = [j for j in range(d) if j != k]
        self.nloc, self.nqf = p1 ** d, nq ** (d - 1)
        loc = np.array(np.unravel_index(np.arange(self.nloc), (p1,) * d, order="F")).T
        qs = np.array(np.unravel_index(np.arange(self.nqf), (nq,) * (d - 1), order="F")).T.reshape(self.nqf, d - 1)
        cpa = [np.asarray(c, dtype=LD) for c in cp]
        N_par = np.zeros(d, dtype=LD)
        N_par[k] = 2 * side - 1

        def tab(j, deriv):
            """[nloc, nqf]: l or l' of direction j at the face points"""
            if j == k:
                return np.repeat((dle if deriv else le)[loc[:, j]], self.nqf, axis=1)
            return (dl if deriv else l)[loc[:, j]][:, qs[:, tang.index(j)]]

        self.elements = []
        X, WS, NR, HN = [], [], [], []
        for e in np.ndindex(*[nel[j] for j in tang][::-1]):
            et = e[::-1]
            el = [0] * d
            el[k] = nel[k] - 1 if side else 0
            for j, v in zip(tang, et):
                el[j] = v
            g = np.zeros(self.nloc, dtype=np.int64)
            stride = 1
            for j in range(d):
                g += stride * (el[j] * p + loc[:, j])
                stride *= n[j]
            PH = np.ones((self.nloc, self.nqf), dtype=LD)
            for j in range(d):
                PH = PH * tab(j, False)
            GR = np.zeros((self.nloc, self.nqf, d), dtype=LD)
            for j in range(d):
                gj = tab(j, True)
                for m in range(d):
                    if m != j:
                        gj = gj * tab(m, False)
                GR[:, :, j] = gj
            wq = np.ones(self.nqf, dtype=LD)
            for i in range(d - 1):
                wq = wq * w[qs[:, i]]
            Nh = [cpa[c][g] @ PH for c in range(nsd + 1)]
            dNh = [np.einsum("a,aqk->qk", cpa[c][g], GR) for c in range(nsd + 1)]
            W, dW = Nh[nsd], dNh[nsd]
            DF = np.stack([(dNh[i] * W[:, None] - Nh[i][:, None] * dW) / (W * W)[:, None] for i in range(nsd)], axis=1)
            met = np.einsum("qik,qim->qkm", DF, DF)
            gi = _inv(met)
            v = np.einsum("qik,qkm,m->qi", DF, gi, N_par)            # DF g^-1 N
            nrm = v / np.sqrt(np.sum(v * v, axis=1))[:, None]
            mt = met[:, tang][:, :, tang]
            ws = wq * np.sqrt(_det_small(mt))
            # h_n: the distance between the faces xi_k = 0, 1 of the element measured along the normal -- 1 / |grad xi_k|,
            # grad xi_k = DF g^-1 e_k
            ek = np.zeros(d, dtype=LD)
            ek[k] = 1
            gx = np.einsum("qik,qkm,m->qi", DF, gi, ek)
            hn = 1 / np.sqrt(np.sum(gx * gx, axis=1))
            # plain and rational functions and their Cartesian gradients, then d_n = n . grad
            PS = PH / W[None, :]
            GRr = (GR * W[None, :, None] - PH[:, :, None] * dW[None, :, :]) / (W * W)[None, :, None]
            cg = np.einsum("qik,qkm,aqm->aqi", DF, gi, GR)
            cgr = np.einsum("qik,qkm,aqm->aqi", DF, gi, GRr)
            DN = np.einsum("aqi,qi->aq", cg, nrm)
            DNr = np.einsum("aqi,qi->aq", cgr, nrm)
            self.elements.append(dict(g=g, PH=PH, PS=PS, CG=cg, CGr=cgr, DN=DN, DNr=DNr))
            X.append(np.stack([Nh[i] / W for i in range(nsd)], axis=1))
            WS.append(ws)
            NR.append(nrm)
            HN.append(hn)
        self.x, self.wsurf, self.normal, self.hn = np.concatenate(X), np.concatenate(WS), np.concatenate(NR), np.concatenate(HN)
        self.npts = self.wsurf.size

    def eval(self, u, rational=False):
        """(values [npts], Cartesian gradient [npts, nsd], d_n u [npts]) of the nodal field u (u_h / W_h if rational)"""
        u = np.asarray(u, dtype=LD)
        V, G, D = [], [], []
        for E in self.elements:
            ue = u[E["g"]]
            V.append(ue @ (E["PS"] if rational else E["PH"]))
            G.append(np.einsum("a,aqi->qi", ue, E["CGr"] if rational else E["CG"]))
            D.append(ue @ (E["DNr"] if rational else E["DN"]))
        return np.concatenate(V), np.concatenate(G), np.concatenate(D)

    def load(self, fq=None, fnq=None, rational=False):
        """b[node] = sum_q wsurf_q (f_q phi_node + fn_q d_n phi_node)"""
        b = np.zeros(self.nnodes, dtype=LD)
        for i, E in enumerate(self.elements):
            sl = slice(i * self.nqf, (i + 1) * self.nqf)
            ws = self.wsurf[sl]
            if fq is not None:
                np.add.at(b, E["g"], (E["PS"] if rational else E["PH"]) @ (ws * np.asarray(fq, dtype=LD)[sl]))
            if fnq is not None:
                np.add.at(b, E["g"], (E["DNr"] if rational else E["DN"]) @ (ws * np.asarray(fnq, dtype=LD)[sl]))
        return b

    def matrix(self, a=None, b=None, c=None, rational=False):
        """dense A_ab = sum_q wsurf_q (a_q phi_a phi_b + b_q phi_a d_n phi_b + c_q d_n phi_a phi_b)"""
        A = np.zeros((self.nnodes, self.nnodes), dtype=LD)
        for i, E in enumerate(self.elements):
            sl = slice(i * self.nqf, (i + 1) * self.nqf)
            ws = self.wsurf[sl]
            PH, DN = (E["PS"], E["DNr"]) if rational else (E["PH"], E["DN"])
            Ae = np.zeros((self.nloc, self.nloc), dtype=LD)
            if a is not None:
                Ae += (PH * (ws * np.asarray(a, dtype=LD)[sl])) @ PH.T
            if b is not None:
                Ae += (PH * (ws * np.asarray(b, dtype=LD)[sl])) @ DN.T
            if c is not None:
                Ae += (DN * (ws * np.asarray(c, dtype=LD)[sl])) @ PH.T
            A[np.ix_(E["g"], E["g"])] += Ae
        return A


def all_faces(d):
    return [(k, s) for k in range(d) for s in (0, 1)]


def nitsche_gamma(ref, C):
    """gamma = C p^2 / h_n at the points of a face"""
    return LD(C) * ref.p ** 2 / ref.hn


# ---- polynomial (unit-weight, non-affine) maps with nsd = d: n wsurf is a polynomial on every face --------------------------
def _greville(p, kv):
    kv = np.asarray(kv, dtype=np.float64)
    return np.array([np.sum(kv[i + 1:i + p + 1]) / p for i in range(len(kv) - p - 1)])


def poly_patch_2d(nels):
    """(knot vectors, homogeneous control net [n0, n1, 3]) of a p = 2 B-spline map of the unit square, unit weights"""
    from oracle import tigar_oracle as O
    kvs = [np.asarray(O.uniform_knots(2, 0., 1., n), dtype=np.float64) for n in nels]
    g0, g1 = np.meshgrid(*[_greville(2, kv) for kv in kvs], indexing="ij")
    x = g0 + 0.2 * g1 ** 2 - 0.1 * g0 * g1
    y = g1 + 0.15 * g0 ** 2 + 0.1 * g0 * g1
    return kvs, np.stack([x, y, np.ones_like(x)], axis=-1)


def poly_patch_3d(nels):
    """(knot vectors, homogeneous control net [n0, n1, n2, 4]) of a trilinear skew map of the unit cube, degree-elevated to
    p = 2 (the B-splines reproduce a multilinear function from its values at the Greville points), unit weights"""
    from oracle import tigar_oracle as O
    kvs = [np.asarray(O.uniform_knots(2, 0., 1., n), dtype=np.float64) for n in nels]
    g0, g1, g2 = np.meshgrid(*[_greville(2, kv) for kv in kvs], indexing="ij")
    x = g0 + 0.2 * g1 * g2 + 0.1 * g0 * g1
    y = g1 + 0.15 * g0 * g2
    z = g2 * (1.0 + 0.2 * g0) + 0.1 * g0 * g1 * g2
    return kvs, np.stack([x, y, z, np.ones_like(x)], axis=-1)


def patch_from_net(p, kvs, C):
    """(element vertices, extraction matrix of the scalar space, control functions on the FE nodes) through the oracle"""
    from oracle import tigar_oracle as O
    s = O.BSpline([p] * len(kvs), [list(k) for k in kvs])
    uks = [np.asarray(s1.uniqueKnots, dtype=np.float64) for s1 in s.splines]
    Mc = O.generate_M_tensor(s)
    return uks, Mc, [np.asarray(Mc @ C[..., i].ravel(order="F")) for i in range(C.shape[-1])]


LIN_2D = (lambda x: 1.0 + 2.0 * x[:, 0] - x[:, 1], np.array([2.0, -1.0]))
LIN_3D = (lambda x: 0.5 - x[:, 0] + 2.0 * x[:, 1] + 0.75 * x[:, 2], np.array([-1.0, 2.0, 0.75]))


def patch_test_host(kvs, C, lin, alpha=2.0, nitsche_faces=None, penalty=10.0):
    """The host flow of the patch test on a polynomial map, p = 2, nq = 3, no zero dofs, solved in float64 by scipy's
    sparse LU: Laplace + Robin (alpha u v on every face, data grad l . n + alpha l), or -- with ``nitsche_faces`` -- the
    symmetric Nitsche terms with gamma = penalty p^2 / h_n and data l on those faces, Neumann data grad l . n on the
    others.  Returns max |u_h - l| over the FE nodes / max |l|."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    from oracle import tigar_oracle as O
    p, d = 2, len(kvs)
    l, gl = lin
    uks, Mc, cp = patch_from_net(p, kvs, C)
    A = O.mapped_fe_system(uks, p, cp)[1].toarray().astype(LD)
    b = np.zeros(A.shape[0], dtype=LD)
    for k, s in all_faces(d):
        ref = FaceReference(uks, p, cp, k, s)
        lq = np.asarray(l(ref.x.astype(np.float64)), dtype=LD)
        flux = ref.normal @ gl.astype(LD)
        if nitsche_faces is None:
            A += alpha * ref.matrix(a=np.ones(ref.npts))
            b += ref.load(flux + alpha * lq)
        elif (k, s) in nitsche_faces:
            gam = nitsche_gamma(ref, penalty)
            minus = -np.ones(ref.npts)
            A += ref.matrix(gam, minus, minus)
            b += ref.load(gam * lq, -lq)
        else:
            b += ref.load(flux)
    K = (Mc.T @ sp.csr_matrix(A.astype(np.float64)) @ Mc).tocsc()
    U = spl.spsolve(K, Mc.T @ b.astype(np.float64))
    xn = np.stack([cp[i] / cp[-1] for i in range(d)], axis=1)
    return float(np.max(np.abs(Mc @ U - l(xn))) / np.max(np.abs(l(xn))))


# ---- Poisson on the quarter annulus with Neumann data on the inner arc and a Robin condition on the outer one ---------------
ROBIN_ALPHA = 2.0


def robin_exact(x):
    """annulus_exact + 2 x y = ((r - 1)(2 - r) + r^2) sin 2 theta: zero on the straight edges, not on the arcs; the added
    term is harmonic, so that -lap u is still ``postproc_reference.annulus_rhs``"""
    import postproc_reference as R
    return R.annulus_exact(x) + 2.0 * x[:, 0] * x[:, 1]


def robin_exact_grad(x):
    import postproc_reference as R
    return R.annulus_exact_grad(x) + 2.0 * np.stack([x[:, 1], x[:, 0]], axis=1)


def neumann_data(x, n):
    return np.sum(robin_exact_grad(x) * n, axis=1)


def robin_data(x, n):
    return neumann_data(x, n) + ROBIN_ALPHA * robin_exact(x)


def solve_annulus_boundary(nel, nitsche=False, penalty=10.0):
    """The host flow on the quarter annulus (p = 2, nq = 3, rational functions): -lap u = f, d_n u = g_N on the inner arc
    (face (0, 0)), d_n u + alpha u = g_R on the outer arc (face (0, 1)), u = 0 on the straight edges -- through zero dofs,
    or with ``nitsche`` on the edge theta = 0 (face (1, 0)) through the symmetric Nitsche terms.  scipy's sparse LU in
    float64.  Returns a dict: the L2 and H10 errors of u_h / W_h, the flux sum_faces sum_q wsurf d_n u over the whole
    boundary, int f dx, the L2 norm and H10 seminorm of the exact solution, and the condition number of the system."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import postproc_reference as R
    import rational_reference as RR
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    uks, Mc, cp = patch_from_net(2, [kv, kv], Pf)
    pts = RR.RationalPoints(uks, 2, cp)
    x = np.asarray(pts.x, dtype=np.float64)
    fq = R.annulus_rhs(x)
    _, Kr, _, b = RR.rational_fe_system(uks, 2, cp, fq=fq)
    A = Kr.toarray().astype(LD)
    b = b.astype(LD)
    refs = dict(((k, s), FaceReference(uks, 2, cp, k, s)) for k, s in all_faces(2))
    xs = dict((f, np.asarray(r.x, dtype=np.float64)) for f, r in refs.items())
    ns = dict((f, np.asarray(r.normal, dtype=np.float64)) for f, r in refs.items())
    b += refs[(0, 0)].load(neumann_data(xs[(0, 0)], ns[(0, 0)]), rational=True)
    A += ROBIN_ALPHA * refs[(0, 1)].matrix(a=np.ones(refs[(0, 1)].npts), rational=True)
    b += refs[(0, 1)].load(robin_data(xs[(0, 1)], ns[(0, 1)]), rational=True)
    ncp = Mc.shape[1]
    n1 = int(round(np.sqrt(ncp)))
    idx = np.arange(ncp).reshape(n1, n1, order="F")
    if nitsche:
        r = refs[(1, 0)]
        gam, minus, g = nitsche_gamma(r, penalty), -np.ones(r.npts), np.asarray(robin_exact(xs[(1, 0)]), dtype=LD)
        A += r.matrix(gam, minus, minus, rational=True)
        b += r.load(gam * g, -g, rational=True)
        bd = idx[:, -1]
    else:
        bd = np.unique(np.concatenate([idx[:, 0], idx[:, -1]]))
    free = np.setdiff1d(np.arange(ncp), bd)
    K = (Mc.T @ sp.csr_matrix(A.astype(np.float64)) @ Mc).tocsr()
    Kf, bf = K[free][:, free].tocsc(), (Mc.T @ b.astype(np.float64))[free]
    U = np.zeros(ncp)
    U[free] = spl.spsolve(Kf, bf)
    u = Mc @ U
    e, ge = robin_exact(x), robin_exact_grad(x)
    (s0, s1, s2), _ = pts.sums_rational(u, e, ge)
    flux = sum(float(np.sum(r.wsurf * r.eval(u, rational=True)[2])) for r in refs.values())
    return dict(l2=float(np.sqrt(s0)), h10=float(np.sqrt(s1)), flux=flux, intf=float(np.sum(pts.wdet * fq)),
                unorm_l2=float(np.sqrt(s2)), unorm_h10=float(np.sqrt(np.sum(pts.wdet * np.sum(ge ** 2, axis=1)))),
                kappa=float(np.linalg.cond(Kf.toarray())))
