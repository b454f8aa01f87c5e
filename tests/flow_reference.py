"""Host reference of the first-order system forms, the element metric and the stabilised incompressible flow on a mapped
patch (the block ending of k_postproc with b and c per block, ``tg_quad_metric``, csrc/tg_flow.hip; ``forms.SystemCoefficientForm``
/ ``SystemLoadForm`` / ``SystemResidual`` / ``FlowResidual``):

    a(u, v) = sum_ij int d_K v_i A_iKjL d_L u_j + d_K v_i b_iKj u_j + v_i c_ijL d_L u_j + v_i m_ij u_j dx     (u: column, v: row)
    L(v)    = sum_i  int s_i v_i + F_iK d_K v_i dx                                    (dofs field after field)

On top of ``coef_reference.CoefReference``, which forms the functions psi (phi, or phi / W_h with ``rational``) and their
CARTESIAN gradients directly at every point of every element; every block is summed as it is written above, densely over
elements, points and local functions -- no tensor brought to the reference element, no folded beta, no sum factorisation.
The metric G is formed from the Jacobian of the map with respect to the knot coordinates and the element sizes, not from P.
The flow law is ``forms.IncompressibleFlow.host`` (numpy, any float dtype), which tests/test_flow_reference_host.py pins by
central differences of its own source and flux.

``dtype``: longdouble (the reference proper) or float64 (the SAME computation in working precision: its distance from the
longdouble run is the yardstick of the GPU tests).  Also a dense Newton flow, a time-stepping flow (generalized-alpha and
backward Euler, written out from the formulas) and the Taylor-Green problems of the tests.
"""
import math

import numpy as np

from oracle import tigar_oracle as O
import coef_reference as CR

LD = np.longdouble
EPS = CR.EPS


class SystemReference(object):
    def __init__(self, uks, p, cp, nF, nq=None, rational=False, dtype=LD):
        self.ref = CR.CoefReference(uks, p, cp, nq, rational=rational, dtype=dtype)
        self.dtype, self.nsd, self.d, self.nF, self.n, self.npts = dtype, self.ref.nsd, self.ref.d, int(nF), self.ref.nnodes, self.ref.npts
        self.x = self.ref.x
        el = self.ref.elements
        self.g = np.stack([e[0] for e in el])                  # [element][local node]
        self.PSI = np.stack([e[1] for e in el])                # [element][point][local node]
        self.GR = np.stack([e[2] for e in el])                 # [element][point][local node][Cartesian direction]
        self.wd = np.stack([e[3] for e in el])                 # [element][point]
        self.ne, self.nqt, self.nloc = self.PSI.shape

    def _pt(self, v, shape):
        """point data [npts] + shape (or one block) -> [element][point] + shape, None stays None"""
        if v is None:
            return None
        v = np.asarray(v, dtype=self.dtype)
        if v.shape == tuple(shape):
            v = np.broadcast_to(v, (self.npts,) + tuple(shape))
        assert v.shape == (self.npts,) + tuple(shape), (v.shape, shape)
        return v.reshape((self.ne, self.nqt) + tuple(shape))

    def element_matrices(self, A=None, b=None, c=None, M=None):
        """[element][i][a][j][b]: the integrand summed over the points of each element, term by term"""
        nF, nsd = self.nF, self.nsd
        A, b, c, M = (self._pt(A, (nF, nsd, nF, nsd)), self._pt(b, (nF, nsd, nF)), self._pt(c, (nF, nF, nsd)), self._pt(M, (nF, nF)))
        Ke = np.zeros((self.ne, nF, self.nloc, nF, self.nloc), dtype=self.dtype)
        w, P, G = self.wd, self.PSI, self.GR
        ne, nqt, nloc = self.ne, self.nqt, self.nloc

        def add(test, coef, trial):
            """Ke[e, i, a, j, b] += sum_q w test[e, q, a, (K)] coef[e, q, i, (K), j, (L)] trial[e, q, b, (L)]: the trial side first,
            then one product of [(i a), q (K)] with [q (K), (j b)] per element (numpy's own loops: no BLAS in longdouble)"""
            nK, nL = test.shape[3], trial.shape[3]
            right = np.einsum("eqiKjL,eqbL->eqKijb", coef, trial).reshape(ne, nqt * nK, nF, nF * nloc)
            left = (w[:, :, None, None] * test).transpose(0, 2, 1, 3).reshape(ne, nloc, nqt * nK)
            for i in range(nF):
                Ke[:, i] += np.matmul(left, right[:, :, i, :]).reshape(ne, nloc, nF, nloc)
        one = P[..., None]
        if A is not None:
            add(G, A, G)
        if b is not None:
            add(G, b[..., None], one)
        if c is not None:
            add(one, c[:, :, :, None, :, :], G)
        if M is not None:
            add(one, M[:, :, :, None, :, None], one)
        return Ke

    def coo(self, A=None, b=None, c=None, M=None):
        """(sorted unique keys row * (nF n) + col, values) of the nF n square matrix, rows and columns field-major"""
        nF, n = self.nF, self.n
        Ke = self.element_matrices(A, b, c, M)
        f = np.arange(nF, dtype=np.int64)
        rows = f[None, :, None] * n + self.g[:, None, :]                                            # [e][i][a]
        keys = (rows[:, :, :, None, None] * (nF * n) + rows[:, None, None, :, :]).ravel()
        uk, inv = np.unique(keys, return_inverse=True)
        out = np.zeros(uk.size, dtype=self.dtype)
        np.add.at(out, inv, Ke.ravel())
        return uk, out

    def dense(self, A=None, b=None, c=None, M=None):
        N = self.nF * self.n
        k, v = self.coo(A, b, c, M)
        D = np.zeros((N, N), dtype=self.dtype)
        D[k // N, k % N] = v
        return D

    def load(self, s=None, F=None):
        """b[i n + node] = sum_q wdet_q (s_i psi_node + F_iK d_K psi_node): s [npts, nF], F [npts, nF, nsd]"""
        nF, n = self.nF, self.n
        s, F = self._pt(s, (nF,)), self._pt(F, (nF, self.nsd))
        be = np.zeros((self.ne, nF, self.nloc), dtype=self.dtype)
        if s is not None:
            be = be + np.einsum("eq,eqi,eqa->eia", self.wd, s, self.PSI, optimize=True)
        if F is not None:
            be = be + np.einsum("eq,eqiK,eqaK->eia", self.wd, F, self.GR, optimize=True)
        out = np.zeros(nF * n, dtype=self.dtype)
        np.add.at(out, (np.arange(nF)[None, :, None] * n + self.g[:, None, :]).ravel(), be.ravel())
        return out

    def eval(self, u):
        """(U [npts, nF], grad U [npts, nF, nsd]) of the nodal values u (field after field)"""
        ul = np.asarray(u, dtype=self.dtype).reshape(self.nF, self.n)[:, self.g]                   # [i][e][a]
        U = np.einsum("eqa,iea->eqi", self.PSI, ul, optimize=True).reshape(self.npts, self.nF)
        G = np.einsum("eqaK,iea->eqiK", self.GR, ul, optimize=True).reshape(self.npts, self.nF, self.nsd)
        return U, G


def metric(uks, p, cp, nq=None, dtype=LD):
    """G [npts, nsd, nsd] = (d xi' / d x)^T (d xi' / d x) with xi' the coordinates of the BI-UNIT parent element: from the
    Jacobian J = d x / d xi (knot coordinates) of every point, its pseudo-inverse (J^T J)^-1 J^T, and d xi'_k / d xi_k = 2 / h_k"""
    d, nsd = len(uks), len(cp) - 1
    nq = p + 1 if nq is None else nq
    l, dl, w = CR.tables(p, nq, dtype)
    nel = [len(u) - 1 for u in uks]
    n = [e * p + 1 for e in nel]
    p1 = p + 1
    loc = np.array(np.unravel_index(np.arange(p1 ** d), (p1,) * d, order="F")).T
    qs = np.array(np.unravel_index(np.arange(nq ** d), (nq,) * d, order="F")).T
    cpa = [np.asarray(c, dtype=dtype) for c in cp]
    out = []
    for e in np.ndindex(*nel[::-1]):
        el = e[::-1]
        h = [dtype(uks[k][el[k] + 1]) - dtype(uks[k][el[k]]) for k in range(d)]
        g = np.zeros(p1 ** d, dtype=np.int64)
        stride = 1
        for k in range(d):
            g += stride * (el[k] * p + loc[:, k])
            stride *= n[k]
        cl = [c[g] for c in cpa]
        for q in range(nq ** d):
            phi = np.ones(p1 ** d, dtype=dtype)
            for k in range(d):
                phi = phi * l[loc[:, k], qs[q, k]]
            gr = np.zeros((p1 ** d, d), dtype=dtype)
            for k in range(d):
                gk = dl[loc[:, k], qs[q, k]] / h[k]
                for m in range(d):
                    if m != k:
                        gk = gk * l[loc[:, m], qs[q, m]]
                gr[:, k] = gk
            N = np.array([c @ phi for c in cl], dtype=dtype)
            dN = np.array([c @ gr for c in cl], dtype=dtype)
            W, dW = N[nsd], dN[nsd]
            J = (dN[:nsd] * W - N[:nsd, None] * dW[None, :]) / (W * W)             # d x_i / d xi_k
            gi, _ = CR._inverse(J.T @ J)
            dxi = (gi @ J.T) * (dtype(2) / np.array(h, dtype=dtype))[:, None]      # d xi'_k / d x_i
            out.append(dxi.T @ dxi)
    return np.array(out, dtype=dtype)


class FlowReference(SystemReference):
    """the stabilised flow on nF = nsd + 1 fields: the law at the points of ``eval`` and ``metric``, then the loads and blocks"""

    def __init__(self, uks, p, cp, nq=None, rational=False, dtype=LD):
        SystemReference.__init__(self, uks, p, cp, len(cp), nq, rational, dtype)
        assert self.nsd == self.d and self.nF == self.nsd + 1
        self.G = metric(uks, p, cp, nq, dtype)

    def state(self, u, law, c_a=0.0, a0=None, f=None, dt4=0.0):
        U, gU = self.eval(u)
        cast = lambda v: None if v is None else np.asarray(v, dtype=self.dtype)
        out = law.host(U, gU, self.G, c_a=c_a, a0=cast(a0), f=cast(f), dt4=dt4)
        assert all(o.dtype == self.dtype for o in out)
        return out

    def residual(self, u, law, **kw):
        s, F = self.state(u, law, **kw)[:2]
        return self.load(s, F)

    def tangent(self, u, law, **kw):
        return self.dense(*self.state(u, law, **kw)[2:6])


def _leibniz3(*factors):
    """bound of the third directional derivative of a product of functions, each given by the bounds (|f|, |f'|, |f''|, |f'''|)
    of its directional derivatives along unit directions: the multinomial sum of the product rule"""
    from itertools import product
    total = 0.0
    for orders in product(range(4), repeat=len(factors)):
        if sum(orders) == 3:
            term = 6.0
            for f, o in zip(factors, orders):
                term = term * f[o] / math.factorial(o)
            total = total + term
    return total


def derivative_bound(law, U, gradU, G, c_a=0.0, a0=None, f=None, dt4=0.0):
    """C3: a bound of |d^3 e [w, w, w]| over the entries e of (s, F) of ``IncompressibleFlow`` and the unit directions w of the
    state (u, grad u, p, grad p), over the given points.  s, the viscous flux and the pressure are polynomials of degree <= 2
    in the state: no third derivative.  The rest are products of
      T  = tau_M = Q^(-1/2), Q = 4/dt^2 + u.Gu + C_I nu^2 G:G.  Along a unit direction |Q'| = 2 |u.Gw| <= 2 sqrt(g Q) (Cauchy-
           Schwarz in the G inner product, u.Gu <= Q, g = |G|), |Q''| <= 2 g, Q''' = 0, so with a = sqrt(g) tau_M:
           |T'| <= T a, |T''| <= 4 T a^2, |T'''| <= 24 T a^3;
      T2 = tau_C = sqrt(Q) / tr G:  |T2'| <= sqrt(g) / tr G, |T2''| <= 2 g tau_M / tr G, |T2'''| <= 6 g^(3/2) tau_M^2 / tr G;
      X  = u_K (linear: |X'| <= 1),  Z = div u (linear: |Z'| <= sqrt(nsd)),
      Y  = r_i = rho (c_a u_i + a0_i - f_i + u_L d_L u_i) + d_i p (quadratic: |Y'| <= rho (|c_a| + |grad u| + |u|) + 1, |Y''| <= 2 rho)
    in F_iK = ... + T X Y + rho T2 Z d_iK and F_pK = T Y / rho: the product rule (``_leibniz3``) point by point, the largest taken."""
    U, gradU, G = [np.asarray(v, dtype=np.float64) for v in (U, gradU, G)]
    n = U.shape[1] - 1
    rho, mu = law.density, law.viscosity
    u, H = U[:, :n], gradU[:, :n, :]
    g = np.sqrt(np.einsum("qKL,qKL->q", G, G))
    Q = dt4 + np.einsum("qK,qKL,qL->q", u, G, u) + law.C_I * (mu / rho) ** 2 * g * g
    tau, trG = Q ** -0.5, np.einsum("qKK->q", G)
    a = np.sqrt(g) * tau
    un, Hn = np.sqrt(np.sum(u * u, axis=1)), np.sqrt(np.sum(H * H, axis=(1, 2)))
    r = np.asarray(law.host(U, gradU, G, c_a=c_a, a0=a0, f=f, dt4=dt4)[1], dtype=np.float64)[:, n, :] * (rho / tau)[:, None]
    zero = np.zeros_like(tau)
    T = (tau, tau * a, 4 * tau * a ** 2, 24 * tau * a ** 3)
    T2 = (np.sqrt(Q) / trG, np.sqrt(g) / trG, 2 * g * tau / trG, 6 * g ** 1.5 * tau ** 2 / trG)
    X = (un, 1.0 + zero, zero, zero)
    Z = (np.abs(np.einsum("qii->q", H)), math.sqrt(n) + zero, zero, zero)
    Y = (np.max(np.abs(r), axis=1), rho * (abs(c_a) + Hn + un) + 1.0, 2.0 * rho + zero, zero)
    return float(np.max(np.maximum(np.maximum(_leibniz3(T, X, Y), rho * _leibniz3(T2, Z)), _leibniz3(T, Y) / rho)))


def newton(ref, Mc, free, law, U0, f=None, tol=1e-9, max_iters=25, **kw):
    """The host Newton flow on the IGA dofs ``free`` (the others keep the data of ``U0``): M^T R, M^T K M dense in float64, no
    line search, the control flow of ``solveNonlinearVariationalProblem`` -- stop when ||M^T R|| / (its first value) < tol.
    ``Mc``: the extraction matrix (nF FE nodes x nF dofs, field after field).  Returns (dofs, relative norms)."""
    Mc = np.asarray(Mc.todense() if hasattr(Mc, "todense") else Mc, dtype=np.float64)
    U = np.array(U0, dtype=np.float64)
    fixed = np.setdiff1d(np.arange(Mc.shape[1]), free)
    history, first = [], None
    for it in range(max_iters):
        u = Mc @ U
        Rv = Mc.T @ ref.residual(u, law, f=f, **kw).astype(np.float64)
        Rv[fixed] = 0.0
        nrm = float(np.linalg.norm(Rv))
        first = nrm if first is None else first
        history.append(nrm / first)
        if history[-1] < tol:
            return U, history
        J = Mc.T @ ref.tangent(u, law, f=f, **kw).astype(np.float64) @ Mc
        U[free] -= np.linalg.solve(J[np.ix_(free, free)], Rv[free])
    raise RuntimeError("the host Newton flow did not converge: %r" % (history,))


def time_stepping(ref, Mc, free, law, U0, Udot0, dt, nsteps, scheme="generalized_alpha", rho_inf=0.5, f=None, tol=1e-9):
    """The host time-stepping flow in the IGA dofs: generalized-alpha for first-order systems (alpha_f = 1 / (1 + rho_inf),
    alpha_m = alpha_f (3 - rho_inf) / 2, gamma = 1/2 + alpha_m - alpha_f) or backward Euler, written out from the formulas: the
    law is read at x_alpha = alpha_f x + (1 - alpha_f) x_old with the acceleration xdot_alpha = alpha_m xdot + (1 - alpha_m)
    xdot_old, xdot = (x - x_old) / (gamma dt) + (1 - 1 / gamma) xdot_old, of the velocity fields; Newton on x from x_old with
    R / alpha_f and K(x_alpha), dense solves in float64.  Returns ([dofs after every step], [their rates], [Newton histories])."""
    Mc = np.asarray(Mc.todense() if hasattr(Mc, "todense") else Mc, dtype=np.float64)
    nsd = ref.nsd
    if scheme == "generalized_alpha":
        af = 1.0 / (1.0 + rho_inf)
        am = af * (1.5 - 0.5 * rho_inf)
        gam = 0.5 + am - af
    else:
        af = am = gam = 1.0
    fixed = np.setdiff1d(np.arange(Mc.shape[1]), free)
    Xo, Vo = np.array(U0, dtype=np.float64), np.array(Udot0, dtype=np.float64)
    states, rates, histories = [], [], []
    for step in range(nsteps):
        X = Xo.copy()
        history, first = [], None
        for it in range(25):
            Vn = (X - Xo) / (gam * dt) + (1.0 - 1.0 / gam) * Vo
            Xa, Va = af * X + (1.0 - af) * Xo, am * Vn + (1.0 - am) * Vo
            c_a = am / (gam * dt) / af                                   # d Va / d Xa
            a0 = ref.eval(Mc @ (Va - c_a * Xa))[0][:, :nsd]
            kw = dict(c_a=c_a, a0=a0, f=f, dt4=4.0 / dt ** 2)
            Rv = Mc.T @ ref.residual(Mc @ Xa, law, **kw).astype(np.float64) / af
            Rv[fixed] = 0.0
            nrm = float(np.linalg.norm(Rv))
            first = nrm if first is None else first
            history.append(nrm / first)
            if history[-1] < tol:
                break
            J = Mc.T @ ref.tangent(Mc @ Xa, law, **kw).astype(np.float64) @ Mc
            X[free] -= np.linalg.solve(J[np.ix_(free, free)], Rv[free])
        else:
            raise RuntimeError("the host time step did not converge: %r" % (history,))
        Vo = (X - Xo) / (gam * dt) + (1.0 - 1.0 / gam) * Vo
        Xo = X
        states.append(Xo.copy())
        rates.append(Vo.copy())
        histories.append(history)
    return states, rates, histories


# ---- the steady Taylor-Green vortex on the distorted square ---------------------------------------------------------------------
# The quadratic one-element square [-pi, pi]^2 whose interior control point is moved to (0.7, 0.3) pi, the control net of the
# reference's 2-D Taylor-Green demo: control points [i][j] (direction 0, direction 1) as (x, y) in units of pi, unit weights.
# As in the demo, parametric direction 0 runs along y and direction 1 along x.
TG_NET = [[(-1.0, -1.0), (0.0, -1.0), (1.0, -1.0)],
          [(-1.0, 0.0), (0.7, 0.3), (1.0, 0.0)],
          [(-1.0, 1.0), (0.0, 1.0), (1.0, 1.0)]]
TG_RHO, TG_MU = 1.0, 0.1
NEWTON_TOL = 1e-9


def tg_velocity(x, t=0.0):
    decay = math.exp(-2.0 * TG_MU / TG_RHO * t)
    return decay * np.stack([np.sin(x[:, 0]) * np.cos(x[:, 1]), -np.cos(x[:, 0]) * np.sin(x[:, 1])], axis=1)


def tg_force(x):
    """f = 2 nu u_exact per unit mass keeps the vortex steady"""
    return 2.0 * TG_MU / TG_RHO * tg_velocity(np.asarray(x, dtype=np.float64))


def taylor_green_problem(nel):
    """p = 2 on nel x nel elements: knot vectors, the refined control net (homogeneous), the FE patch, the extraction matrix of
    three fields, the free dofs: the normal velocity is zero on the four sides (on the sides of parametric direction k that is
    field 1 - k: direction 0 runs along y), the first pressure dof is pinned"""
    from geom_util import _refine_control_net
    p = 2
    coarse = O.BSpline1(p, [-1.0] * 3 + [1.0] * 3)
    kv = np.asarray(O.uniform_knots(p, -1.0, 1.0, nel), dtype=np.float64)
    fine = O.BSpline1(p, list(kv))
    Pw = np.ones((3, 3, 3))
    Pw[:, :, :2] = math.pi * np.asarray(TG_NET)
    Pr = np.stack([_refine_control_net(coarse, fine, Pw[:, j, :]) for j in range(3)], axis=1)
    C = np.stack([_refine_control_net(coarse, fine, Pr[i, :, :]) for i in range(Pr.shape[0])], axis=0)
    s = O.BSpline([p, p], [list(kv), list(kv)])
    uks = [np.asarray(s1.uniqueKnots, dtype=np.float64) for s1 in s.splines]
    M1 = O.generate_M_tensor(s)
    cp = [np.asarray(M1 @ C[..., i].ravel(order="F")) for i in range(3)]
    Mc = O.generate_M_tensor(s, nfields=3)
    ncp = M1.shape[1]
    idx = np.arange(ncp).reshape(C.shape[:-1], order="F")
    fixed = np.concatenate([np.concatenate([np.take(idx, 0, axis=k).ravel(), np.take(idx, -1, axis=k).ravel()]) + (1 - k) * ncp for k in range(2)]
                           + [np.array([2 * ncp])])
    return dict(p=p, nel=nel, kvs=[kv, kv], C=C, uks=uks, cp=cp, Mc=Mc, ncp=ncp, free=np.setdiff1d(np.arange(3 * ncp), fixed),
                U0=np.zeros(3 * ncp))


def velocity_errors(ref, u, t=0.0):
    """the L2 errors of the two velocity fields against the exact vortex, field by field, from the points of the reference"""
    U, _ = ref.eval(u)
    ex = tg_velocity(ref.x.astype(np.float64), t)
    w = ref.wd.ravel()
    return [float(np.sqrt(np.sum(w * (U[:, i] - ex[:, i]) ** 2))) for i in range(2)]


def tg_pressure(x, t=0.0):
    decay = math.exp(-4.0 * TG_MU / TG_RHO * t)
    return decay * 0.25 * TG_RHO * (np.cos(2.0 * x[:, 0]) + np.cos(2.0 * x[:, 1]))


def amplitude(ref, u):
    """int u_h . u_0 dx / int u_0 . u_0 dx with u_0 the vortex at t = 0: exp(-2 nu t) for the exact flow"""
    U, _ = ref.eval(u)
    ex = tg_velocity(ref.x.astype(np.float64))
    w = ref.wd.ravel().astype(np.float64)
    return float(np.sum(w * np.sum(U[:, :2].astype(np.float64) * ex, axis=1)) / np.sum(w * np.sum(ex * ex, axis=1)))


def host_projection(pb, values):
    """IGA dofs of the L2 projection of point values (one scalar field) in the rational space of the problem, on the host"""
    one = SystemReference(pb["uks"], pb["p"], pb["cp"], 1, rational=True, dtype=np.float64)
    M1 = np.asarray(pb["Mc"].todense() if hasattr(pb["Mc"], "todense") else pb["Mc"], dtype=np.float64)[:one.n, :pb["ncp"]]
    mass = M1.T @ one.dense(None, None, None, np.ones((1, 1))) @ M1
    return np.linalg.solve(mass, M1.T @ one.load(np.asarray(values, dtype=np.float64)[:, None]))


TG_DT = 0.125


def transient_taylor_green_data(U0=None):
    """(problem, law, initial dofs, initial rates, float64 reference) of the transient vortex on 8^2 elements: the initial dofs
    are the L2 projections of the exact fields (``U0``: projected elsewhere) with the constrained dofs set to zero, the
    rates those of the exact decay, -2 nu u and -4 nu p"""
    from tigar_amd import forms
    pb = taylor_green_problem(8)
    law = forms.IncompressibleFlow(TG_RHO, TG_MU)
    ref = FlowReference(pb["uks"], pb["p"], pb["cp"], rational=True, dtype=np.float64)
    ncp = pb["ncp"]
    if U0 is None:
        x = ref.x
        ex = tg_velocity(x)
        U0 = np.concatenate([host_projection(pb, ex[:, 0]), host_projection(pb, ex[:, 1]), host_projection(pb, tg_pressure(x))])
    U0 = np.array(U0, dtype=np.float64)
    U0[np.setdiff1d(np.arange(3 * ncp), pb["free"])] = 0.0
    V0 = -2.0 * TG_MU / TG_RHO * U0
    V0[2 * ncp:] *= 2.0
    return pb, law, U0, V0, ref


_FLOWS = {}


def host_taylor_green(nel, C_I=36.0):
    """(problem, law, dofs, history, velocity errors) of the steady host flow in float64 on nel x nel elements: computed once"""
    from tigar_amd import forms
    if (nel, C_I) not in _FLOWS:
        pb = taylor_green_problem(nel)
        law = forms.IncompressibleFlow(TG_RHO, TG_MU, C_I=C_I)
        ref = FlowReference(pb["uks"], pb["p"], pb["cp"], rational=True, dtype=np.float64)
        U, hist = newton(ref, pb["Mc"], pb["free"], law, pb["U0"], f=tg_force(ref.x), tol=NEWTON_TOL)
        Mc = np.asarray(pb["Mc"].todense() if hasattr(pb["Mc"], "todense") else pb["Mc"])
        _FLOWS[(nel, C_I)] = (pb, law, U, hist, velocity_errors(ref, Mc @ U))
    return _FLOWS[(nel, C_I)]
