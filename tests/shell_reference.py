"""Host reference of the Kirchhoff-Love shell (``forms.KirchhoffLoveSVK``, ``forms.ShellResidual``) on top of
``jet_reference.JetReference``: dense numpy loops per element and point, in longdouble or (``dtype``) in float64.

The energy density is written AS THE DEMO WRITES IT (demos/kl-shell-svk/dynamic-tspline.py:135-212 of the reference):
covariant basis from the parametric gradient, a_2 = unit(a_0 x a_1), curvature b = -a_alpha . d_beta a_2, strains brought to
the local Cartesian basis of a Gram-Schmidt orthonormalisation of the REFERENCE basis, Voigt notation and the plane-stress
matrix D.  That is a statement of psi independent of the curvilinear closed forms of ``KirchhoffLoveSVK.host`` (contravariant
metric, b_ab = x_,ab . a_3, C^abcd), which tests/test_jet_reference_host.py holds against it.

Residual and tangent are the jet load of s and the jet matrix of T of the law under test's ``host`` in the reference's dtype;
tests/test_jet_reference_host.py pins them by central differences of the demo's energy.  Also the dense Newton flow and the
problems of the GPU tests.
"""
import numpy as np

from oracle import tigar_oracle as O
import jet_reference as JR

LD = np.longdouble
EPS = JR.EPS


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return np.einsum("qc,qc->q", a, b)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[:, None]


def _shell_geometry(jet):
    """(a0, a1, a2, a [q,2,2], b [q,2,2]) of the demo's shellGeometry from the jet [npts, 3, 6] of the configuration"""
    a0, a1 = jet[:, :, 1], jet[:, :, 2]
    n = _cross(a0, a1)
    nn = np.sqrt(_dot(n, n))
    a2 = n / nn[:, None]
    second = {(0, 0): jet[:, :, 3], (0, 1): jet[:, :, 4], (1, 0): jet[:, :, 4], (1, 1): jet[:, :, 5]}
    a = np.stack([np.stack([_dot(a0, a0), _dot(a0, a1)], 1), np.stack([_dot(a1, a0), _dot(a1, a1)], 1)], 1)
    b = np.empty_like(a)
    for beta in range(2):
        dn = _cross(second[(0, beta)], a1) + _cross(a0, second[(1, beta)])          # d_beta (a0 x a1)
        da2 = (dn - a2 * _dot(a2, dn)[:, None]) / nn[:, None]                       # d_beta of the unit vector
        b[:, 0, beta], b[:, 1, beta] = -_dot(a0, da2), -_dot(a1, da2)
    return a0, a1, a2, a, b


def demo_energy(Xjet, ujet, E, nu, h):
    """psi per unit reference area, as the demo writes it; jets [npts, 3, 6] of one dtype"""
    dt = Xjet.dtype.type
    A0, A1, A2, A, B = _shell_geometry(Xjet)
    a0, a1, a2, a, b = _shell_geometry(Xjet + ujet)
    eps, kap = dt(0.5) * (a - A), B - b
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    ac = np.empty_like(A)
    ac[:, 0, 0], ac[:, 1, 1], ac[:, 0, 1], ac[:, 1, 0] = A[:, 1, 1] / det, A[:, 0, 0] / det, -A[:, 0, 1] / det, -A[:, 1, 0] / det
    a0c = ac[:, 0, 0, None] * A0 + ac[:, 0, 1, None] * A1
    a1c = ac[:, 1, 0, None] * A0 + ac[:, 1, 1, None] * A1
    e0 = _unit(A0)
    e1 = _unit(A1 - e0 * _dot(A1, e0)[:, None])
    ea = np.stack([np.stack([_dot(e0, a0c), _dot(e0, a1c)], 1), np.stack([_dot(e1, a0c), _dot(e1, a1c)], 1)], 1)

    def voigt_bar(T):
        Tb = np.einsum("qab,qbc,qdc->qad", ea, T, ea)
        return np.stack([Tb[:, 0, 0], Tb[:, 1, 1], dt(2) * Tb[:, 0, 1]], 1)
    c = dt(E) / (dt(1) - dt(nu) * dt(nu))
    D = np.zeros((3, 3), dtype=Xjet.dtype)
    D[0, 0] = D[1, 1] = c
    D[0, 1] = D[1, 0] = c * dt(nu)
    D[2, 2] = c * dt(0.5) * (dt(1) - dt(nu))
    ev, kv = voigt_bar(eps), voigt_bar(kap)
    nbar = dt(h) * np.einsum("ab,qb->qa", D, ev)
    mbar = dt(h) ** 3 * np.einsum("ab,qb->qa", D, kv) / dt(12)
    return dt(0.5) * (_dot(ev, nbar) + _dot(kv, mbar))


class ShellReference(object):
    def __init__(self, uks, p, cp, nq=None, rational=False, dtype=LD):
        self.ref = JR.JetReference(uks, p, cp, nq, rational=rational, dtype=dtype)
        if self.ref.d != 2 or self.ref.nsd != 3:
            raise ValueError("a surface in space")
        self.dtype, self.n, self.npts, self.nF = dtype, self.ref.nnodes, self.ref.npts, 3
        self.x = self.ref.x

    def jets(self, u):
        return self.ref.geometry_jets(), self.ref.field_jets(u, 3)

    def state(self, u, material):
        psi, s, T = material.host(*self.jets(u))
        assert psi.dtype == self.dtype and s.dtype == self.dtype and T.dtype == self.dtype
        return psi, s, T

    def energy(self, u, material):
        """sum wdet psi with the DEMO's psi"""
        X, U = self.jets(u)
        return np.sum(self.ref.wdet * demo_energy(X, U, material.E, material.nu, material.thickness))

    def law_energy(self, u, material):
        return np.sum(self.ref.wdet * self.state(u, material)[0])

    def magnitude(self, u, material):
        """(row sizes [3 n] = sum_q wdet sum_alpha s_mag |J^alpha psi_node|, sum_q wdet psi_mag): see ``magnitudes``"""
        X, U = self.jets(u)
        s, psi = magnitudes(X, U, material.E, material.nu, material.thickness)
        b = np.zeros((3, self.n), dtype=self.dtype)
        for e, (g, PSI) in enumerate(self.ref.elements):
            sl = slice(e * self.ref.nqt, (e + 1) * self.ref.nqt)
            b[:, g] += np.einsum("q,aqA,qiA->ia", self.ref.wdet[sl], abs(PSI), s[sl])
        return b.ravel(), np.sum(self.ref.wdet * psi)

    def body_load(self, f):
        """[3 n]: sum_q wdet f_i psi_node, f [npts, 3] or 3 numbers"""
        f = np.asarray(f).astype(self.dtype)
        s = np.zeros((self.npts, 3, self.ref.nJ), dtype=self.dtype)
        s[:, :, 0] = f
        return self.ref.load(s)

    def residual(self, u, material, f=None):
        s = self.state(u, material)[1]
        if f is not None:
            s = s.copy()
            s[:, :, 0] -= np.asarray(f).astype(self.dtype)
        return self.ref.load(s)

    def tangent(self, u, material):
        return self.ref.matrix(self.state(u, material)[2])


def magnitudes(Xjet, ujet, E, nu, h):
    """(s_mag [npts, 3, 6], psi_mag [npts]): the sizes of the terms that cancel in s and psi, by first-order propagation --
    eps_ab is a difference of a_ab and A_ab, kappa_ab of B_ab and b_ab, so they enter as (|a_ab| + |A_ab|) / 2 and
    |B_ab| + |b_ab|; every product takes the absolute values of its factors.  The yardstick of the rigid-motion test: a state
    without strain has s = 0 only up to rounding errors of this size."""
    dt = Xjet.dtype.type
    A0, A1, A2, A, B = _shell_geometry(Xjet)
    xj = Xjet + ujet
    a0, a1, a2, a, b = _shell_geometry(xj)
    em, km = dt(0.5) * (abs(a) + abs(A)), abs(B) + abs(b)
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    Ai = np.empty_like(A)
    Ai[:, 0, 0], Ai[:, 1, 1], Ai[:, 0, 1], Ai[:, 1, 0] = A[:, 1, 1] / det, A[:, 0, 0] / det, -A[:, 0, 1] / det, -A[:, 1, 0] / det
    Ai = abs(Ai)
    c = dt(E) / (dt(1) - dt(nu) * dt(nu))
    C = c * (dt(nu) * np.einsum("qab,qcd->qabcd", Ai, Ai) + dt(0.5) * (dt(1) - dt(nu)) *
             (np.einsum("qac,qbd->qabcd", Ai, Ai) + np.einsum("qad,qbc->qabcd", Ai, Ai)))
    nm, mm = dt(h) * np.einsum("qabcd,qcd->qab", C, em), dt(h) ** 3 / dt(12) * np.einsum("qabcd,qcd->qab", C, km)
    psi = dt(0.5) * (np.einsum("qab,qab->q", nm, em) + np.einsum("qab,qab->q", mm, km))
    deta = a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] * a[:, 1, 0]
    ai = np.empty_like(a)
    ai[:, 0, 0], ai[:, 1, 1], ai[:, 0, 1], ai[:, 1, 0] = a[:, 1, 1] / deta, a[:, 0, 0] / deta, -a[:, 0, 1] / deta, -a[:, 1, 0] / deta
    g = (a0, a1)
    gup = [abs(ai[:, k, 0, None] * a0) + abs(ai[:, k, 1, None] * a1) for k in range(2)]
    slot = {(0, 0): 3, (0, 1): 4, (1, 0): 4, (1, 1): 5}
    s = np.zeros_like(Xjet)
    for al in range(2):
        for be in range(2):
            s[:, :, 1 + al] += nm[:, al, be, None] * abs(g[be])
            s[:, :, slot[(al, be)]] += mm[:, al, be, None] * abs(a2)
            for k in range(2):
                gam = np.einsum("qc,qc->q", abs(xj[:, :, slot[(al, be)]]), gup[k])
                s[:, :, 1 + k] += (mm[:, al, be] * gam)[:, None] * abs(a2)
    return s, psi


def newton(ref, Mc, free, material, U0, f=None, tol=1e-9, max_iters=25):
    """The host Newton flow on the IGA dofs ``free``: M^T R, M^T K M dense in float64, no line search, with the control flow
    of ``solveNonlinearVariationalProblem`` -- stop when ||M^T R|| / (its first value) < tol.  Returns (dofs, relative norms)."""
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


# ---- surfaces as B-spline / NURBS control nets (what an ExtractedSpline is built from) ---------------------------------------
def _collocation(s1):
    n = s1.getNcp()
    N = np.zeros((n, n))
    g = np.array([s1.greville(i) for i in range(n)])
    for r, u in enumerate(g):
        N[r, s1.getNodes(u)] = s1.basisFuncs(s1.getKnotSpan(u), u)
    return g, N


def control_net(p, nels, homogeneous):
    """(knot vectors, control net [M, N, 4]) of the surface whose homogeneous coordinates ``homogeneous(t0, t1) -> 4 arrays``
    are polynomials of degree <= p per direction: interpolation at the Greville points, exact"""
    kvs = [np.asarray(O.uniform_knots(p, 0., 1., n), dtype=np.float64) for n in nels]
    g0, N0 = _collocation(O.BSpline1(p, list(kvs[0])))
    g1, N1 = _collocation(O.BSpline1(p, list(kvs[1])))
    T0, T1 = np.meshgrid(g0, g1, indexing="ij")
    F = np.stack(homogeneous(T0, T1), axis=-1)
    C = np.linalg.solve(N0, F.reshape(len(g0), -1)).reshape(F.shape)
    C = np.linalg.solve(N1, C.transpose(1, 0, 2).reshape(len(g1), -1)).reshape(len(g1), len(g0), 4).transpose(1, 0, 2)
    return kvs, C


def cylinder_homogeneous(length=1.5):
    def f(t0, t1):
        wx, wy, w = JR._arc_homogeneous(t0)
        return wx, wy, w * length * t1, w
    return f


def doubly_curved_homogeneous(t0, t1):
    return t0 + 0.1 * t1 ** 2, 1.2 * t1 + 0.1 * t0 ** 2, 0.4 * t0 ** 2 - 0.3 * t1 ** 2 + 0.2 * t0 * t1, np.ones_like(t0)


def plate_homogeneous(t0, t1):
    return t0, t1, np.zeros_like(t0), np.ones_like(t0)


def problem(p, nels, homogeneous, clamp=None, supported=False):
    """(element vertices, control functions on the FE nodes, extraction matrix for three fields, control net, free dofs):
    ``clamp`` = (direction, side, layers) fixes that many rows of control points of every field; ``supported``: one row on
    every edge"""
    kvs, C = control_net(p, nels, homogeneous)
    s = O.BSpline([p, p], [list(k) for k in kvs])
    uks = [np.asarray(s1.uniqueKnots, dtype=np.float64) for s1 in s.splines]
    M1 = O.generate_M_tensor(s)
    cp = [np.asarray(M1 @ C[..., i].ravel(order="F")) for i in range(4)]
    Mc = O.generate_M_tensor(s, nfields=3)
    ncp = M1.shape[1]
    idx = np.arange(ncp).reshape(C.shape[:-1], order="F")
    held = []
    if clamp is not None:
        direction, side, layers = clamp
        for layer in range(layers):
            held.append(np.take(idx, layer if side == 0 else -1 - layer, axis=direction).ravel())
    if supported:
        held += [idx[0, :], idx[-1, :], idx[:, 0], idx[:, -1]]
    held = np.unique(np.concatenate(held)) if held else np.zeros(0, dtype=np.int64)
    fixed = np.concatenate([f * ncp + held for f in range(3)])
    return dict(p=p, nels=tuple(nels), kvs=kvs, C=C, uks=uks, cp=cp, Mc=Mc, ncp=ncp, held=held, clamp=clamp, supported=supported,
                free=np.setdiff1d(np.arange(3 * ncp), fixed))


# ---- the Newton problem of the GPU tests: a clamped cylinder strip under a body force ------------------------------------------
E_MOD, NU, THICKNESS = 1.0e4, 0.3, 0.05
STRIP_LOAD = (-0.1, 0.0, 0.0)        # per unit reference area; chosen on the CPU so that the host flow takes at most 8 steps
NEWTON_TOL = 1e-9
_FLOWS = {}


def strip_problem(p):
    """quarter-cylinder strip, 4 x 4 elements, two rows of control points clamped on the straight edge z = 0"""
    return problem(p, (4, 4), cylinder_homogeneous(), clamp=(1, 0, 2))


def strip_flow(p, material):
    """(problem, dofs, history) of the host flow in float64: computed once per degree"""
    if p not in _FLOWS:
        pb = strip_problem(p)
        ref = ShellReference(pb["uks"], p, pb["cp"], rational=True, dtype=np.float64)
        U, hist = newton(ref, pb["Mc"], pb["free"], material, np.zeros(3 * pb["ncp"]), f=STRIP_LOAD, tol=NEWTON_TOL)
        _FLOWS[p] = (pb, U, hist)
    return _FLOWS[p]


# ---- plate bending: Navier's solution of the simply supported square under a sinusoidal load -----------------------------------
PLATE_E, PLATE_NU, PLATE_H = 1.0e6, 0.3, 0.1


def plate_load_amplitude():
    """q such that the exact centre deflection is 1e-4 h"""
    D = PLATE_E * PLATE_H ** 3 / (12.0 * (1.0 - PLATE_NU ** 2))
    return 1e-4 * PLATE_H * D * np.pi ** 4 * 4.0


def plate_exact_centre(q):
    D = PLATE_E * PLATE_H ** 3 / (12.0 * (1.0 - PLATE_NU ** 2))
    return q / (D * np.pi ** 4 * 4.0)          # a = b = 1: (a^-2 + b^-2)^2 = 4


def plate_problem(nel):
    return problem(3, (nel, nel), plate_homogeneous, supported=True)


def plate_force(x):
    """the load at the points x [npts, 3]"""
    q = plate_load_amplitude()
    f = np.zeros((x.shape[0], 3), dtype=x.dtype)
    f[:, 2] = q * np.sin(np.pi * x[:, 0]) * np.sin(np.pi * x[:, 1])
    return f


def centre_deflection(pb, U):
    """u_z at the centre of the plate (an element vertex for an even element count) from the dofs U"""
    u = np.asarray(pb["Mc"] @ U).ravel()
    n0 = pb["nels"][0] * pb["p"] + 1
    n = n0 * (pb["nels"][1] * pb["p"] + 1)
    c0, c1 = pb["nels"][0] // 2 * pb["p"], pb["nels"][1] // 2 * pb["p"]
    return float(u[2 * n + c0 + n0 * c1])
