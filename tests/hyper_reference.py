"""Host reference of the vector point forms and of finite-strain elasticity on a mapped patch (csrc/tg_material.hip, the
block ending of k_postproc, ``forms.VectorCoefficientForm`` / ``VectorLoadForm`` / ``HyperelasticResidual``):

    a(u, v) = int d_K v_i A_iKjL d_L u_j + v_i M_ij u_j dx          (u: column, v: row; dofs field after field)
    R(v)    = int P(I + grad u) : grad v - f . v dx

Dense loops per element and point on top of ``coef_reference.CoefReference``, which forms the functions psi (phi, or
phi / W_h with ``rational``) and their CARTESIAN gradients directly at every point: every block is summed as it is written
above -- no tensor brought to the reference element, no folded beta, no sum factorisation.  The laws are the ``host``
methods of the materials of ``tigar_amd.forms`` (numpy, any float dtype), which tests/test_hyper_reference_host.py pins by
central differences of their own energy and stress.

``dtype``: longdouble (the reference proper) or float64 (the SAME computation in working precision: its distance from the
longdouble run is the yardstick of the GPU tests).  Also a dense Newton flow, and the two Newton problems of the tests.
"""
import numpy as np

from oracle import tigar_oracle as O
import coef_reference as CR

LD = np.longdouble
EPS = CR.EPS


class HyperReference(object):
    def __init__(self, uks, p, cp, nq=None, rational=False, dtype=LD):
        self.ref = CR.CoefReference(uks, p, cp, nq, rational=rational, dtype=dtype)
        self.dtype, self.nsd, self.nF, self.n, self.npts = dtype, self.ref.nsd, self.ref.nsd, self.ref.nnodes, self.ref.npts
        if self.ref.d != self.nsd:
            raise ValueError("nsd == d")
        self.x = self.ref.x

    def fields(self, u):
        return np.asarray(u, dtype=self.dtype).reshape(self.nF, self.n)

    def grad_u(self, u):
        """d u_i / d x_K at the points: [npts, nF, nsd]"""
        return np.stack([self.ref.eval(ui)[1] for ui in self.fields(u)], axis=1)

    def state(self, u, material):
        """(P [npts, nF, nsd], A [npts, nF, nsd, nF, nsd], psi [npts]) of the law at F = I + grad u"""
        F = self.grad_u(u) + np.eye(self.nsd, dtype=self.dtype)
        P, A, psi = material.host(F)
        assert P.dtype == self.dtype and A.dtype == self.dtype and psi.dtype == self.dtype
        return P, A, psi

    def load(self, f=None, flux=None):
        """b[i n + node] = sum_q wdet_q (f_i psi_node + flux_iK d_K psi_node): f [npts, nF], flux [npts, nF, nsd]"""
        return np.concatenate([self.ref.load(None if f is None else np.asarray(f, dtype=self.dtype)[:, i],
                                             None if flux is None else np.asarray(flux, dtype=self.dtype)[:, i, :])
                               for i in range(self.nF)])

    def residual(self, u, material, f=None):
        return self.load(None if f is None else -np.asarray(f, dtype=self.dtype), self.state(u, material)[0])

    def energy(self, u, material):
        return np.sum(self.ref.wdet() * self.state(u, material)[2])

    def blocks(self, A, M=None):
        """{(i, j): (keys row * n + col, values)} of the tangent A [npts, nF, nsd, nF, nsd] and the reaction M [npts, nF, nF]"""
        A = np.asarray(A, dtype=self.dtype)
        return {(i, j): self.ref.matrix(A[:, i, :, j, :], None, None, None if M is None else np.asarray(M, dtype=self.dtype)[:, i, j])
                for i in range(self.nF) for j in range(self.nF)}

    def dense(self, A, M=None):
        n, nF = self.n, self.nF
        D = np.zeros((nF * n, nF * n), dtype=self.dtype)
        for (i, j), (k, v) in self.blocks(A, M).items():
            D[i * n + k // n, j * n + k % n] = v
        return D

    def tangent(self, u, material):
        return self.dense(self.state(u, material)[1])


def random_F(n, count, seed):
    """F = Q1 diag(s) Q2 with proper rotations and singular values in [0.7, 1.44]: J = prod s in [0.34, 2.99] (inside the
    [0.3, 3] of the tests), |F^-1| <= 1 / 0.7"""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, n, n))
    for q in range(count):
        Q = []
        for _ in range(2):
            A, _ = np.linalg.qr(rng.standard_normal((n, n)))
            if np.linalg.det(A) < 0:
                A[:, 0] = -A[:, 0]
            Q.append(A)
        out[q] = Q[0] @ np.diag(rng.uniform(0.7, 1.44, n)) @ Q[1]
    return out


def derivative_bounds(lam, mu, f_norm, finv_norm, lnj):
    """(C3, C4): bounds of the third and fourth derivatives of the three energies as multilinear forms (Frobenius norms of the
    arguments), for states with |F|_2 <= f_norm, |F^-1|_2 <= finv_norm, |ln J| <= lnj.
    St. Venant-Kirchhoff: P = lambda/2 (|F|^2 - n) F + mu (F F^T F - F) is cubic, D^3 P[a, b, c] = lambda ((a.b) c + (a.c) b +
    (b.c) a) + mu (the six products a b^T c): C4 = 3 lambda + 6 mu, C3 = C4 |F|.
    Neo-Hookean: A = mu I (x) I + (mu - lambda ln J) G + lambda G' with G, G' products of two factors F^-1; each derivative of
    a factor F^-1 adds one more (and a sign), that of ln J one F^-1: C3 = |F^-1|^3 (2 mu + lambda (3 + 2 |ln J|)),
    C4 = |F^-1|^4 (6 mu + lambda (11 + 6 |ln J|)).  The linear law has none."""
    c3 = max((3 * lam + 6 * mu) * f_norm, finv_norm ** 3 * (2 * mu + lam * (3 + 2 * lnj)))
    c4 = max(3 * lam + 6 * mu, finv_norm ** 4 * (6 * mu + lam * (11 + 6 * lnj)))
    return c3, c4


def newton(ref, Mc, free, material, U0, f=None, tol=1e-9, max_iters=25):
    """The host Newton flow on the IGA dofs ``free`` (the others keep the data of ``U0``): M^T R, M^T K M dense in float64,
    no line search, with the control flow of ``solveNonlinearVariationalProblem`` -- stop when ||M^T R|| / (its first value)
    < tol.  ``Mc``: the extraction matrix (nF FE nodes x nF dofs, field after field).  Returns (dofs, relative norms)."""
    Mc = np.asarray(Mc.todense() if hasattr(Mc, "todense") else Mc, dtype=np.float64)
    U = np.array(U0, dtype=np.float64)
    fixed = np.setdiff1d(np.arange(Mc.shape[1]), free)
    history, first = [], None
    for it in range(max_iters):
        u = Mc @ U
        Rv = Mc.T @ ref.residual(u, material, f).astype(np.float64)
        Rv[fixed] = 0.0
        nrm = float(np.linalg.norm(Rv))
        first = nrm if first is None else first
        history.append(nrm / first)
        if history[-1] < tol:
            return U, history
        J = Mc.T @ ref.tangent(u, material).astype(np.float64) @ Mc
        U[free] -= np.linalg.solve(J[np.ix_(free, free)], Rv[free])
    raise RuntimeError("the host Newton flow did not converge: %r" % (history,))


# ---- the Newton problems of the tests: a face held, the opposite face moved (the data sit in the initial dofs) -----------------
LAM, MU = 2.0, 1.0
NEWTON_TOL = 1e-9


def _problem(degs, kvs, C, direction, move):
    """(element vertices, control functions on the FE nodes, extraction matrix for nF fields, initial dofs, free dofs, the
    dof indices of the two faces per field): the faces ``direction`` = 0 / 1 of the patch with the control net ``C`` (homogeneous),
    the first held, the second displaced by ``move`` -- for rational functions u = sum_a R_a d_a the dof of control point a
    is w_a d_a"""
    d = len(degs)
    s = O.BSpline(list(degs), [list(k) for k in kvs])
    uks = [np.asarray(s1.uniqueKnots, dtype=np.float64) for s1 in s.splines]
    M1 = O.generate_M_tensor(s)
    cp = [np.asarray(M1 @ C[..., i].ravel(order="F")) for i in range(d + 1)]
    Mc = O.generate_M_tensor(s, nfields=d)
    ncp = M1.shape[1]
    idx = np.arange(ncp).reshape(C.shape[:-1], order="F")
    lo, hi = np.take(idx, 0, axis=direction).ravel(), np.take(idx, -1, axis=direction).ravel()
    w = C[..., d].ravel(order="F")
    U0 = np.zeros(d * ncp)
    for f in range(d):
        U0[f * ncp + hi] = w[hi] * move[f]
    fixed = np.concatenate([f * ncp + np.concatenate([lo, hi]) for f in range(d)])
    return dict(uks=uks, cp=cp, Mc=Mc, U0=U0, free=np.setdiff1d(np.arange(d * ncp), fixed), lo=lo, hi=hi, ncp=ncp,
                w=w, move=np.asarray(move, dtype=np.float64), direction=direction)


def block_problem():
    """3-D, p = 2, 2 x 2 x 2 elements of the rational volume: face xi_0 = 0 held, face xi_0 = 1 moved"""
    from geom_util import rational_volume
    kvs, C = rational_volume(2, (2, 2, 2))
    out = _problem([2, 2, 2], kvs, C, 0, (0.2, 0.1, -0.05))
    out.update(p=2, kvs=kvs, C=C)
    return out


def annulus_problem():
    """2-D (plane strain), p = 2, 4 x 4 elements of the quarter annulus: edge theta = 0 held, edge theta = pi / 2 moved"""
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(4)
    out = _problem([2, 2], [kv, kv], Pf, 1, (-0.25, 0.15))
    out.update(p=2, kvs=[kv, kv], C=Pf)
    return out


_FLOWS = {}


def host_flow(name, material):
    """(problem, dofs, history) of the host flow in float64 for ``block`` / ``annulus``: computed once"""
    if name not in _FLOWS:
        pb = block_problem() if name == "block" else annulus_problem()
        ref = HyperReference(pb["uks"], pb["p"], pb["cp"], rational=True, dtype=np.float64)
        U, hist = newton(ref, pb["Mc"], pb["free"], material, pb["U0"], tol=NEWTON_TOL)
        _FLOWS[name] = (pb, U, hist)
    return _FLOWS[name]
