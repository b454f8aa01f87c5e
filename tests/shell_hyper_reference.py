"""Host reference of the hyperelastic Kirchhoff-Love shell (``forms.KirchhoffLoveHyper``) and of the follower pressure
(``forms.ShellResidual(pressure=...)``) on top of tests/shell_reference.py: dense numpy per point, in longdouble or (``dtype``)
in float64.

The energy density is written AS THE DEMO WRITES IT (demos/kl-shell-hyper/kl-hyper.py:98-215 of the reference): the
parametric derivative of the unit normal formed directly, b = -a_alpha . d_beta a_3, the curvilinear basis G_b = A_b + xi d_b A_3,
Gram-Schmidt, ``tensorToCartesian`` with the inverse of the truncated metric, C_22 = 1 / det C_2D, the LITERAL multiplier term
-p (J - 1) with p = mu C_22, and the rule of ``getQuadRuleInterval``.  That is a statement of psi independent of the closed
forms of ``KirchhoffLoveHyper.host`` (Weingarten's formula, the triangular frame, the energy without the multiplier term,
the derivatives by the adjugate), which tests/test_shell_hyper_reference_host.py holds against it by central differences.

The pressure load and its tangent are written directly from -P sqrt(det a / det A) a_3 with the variations of sqrt(det a) and
of a_3 (not from the cross product x_,1 x x_,2 the package differentiates).  Also the dense load-stepped Newton flow of the
inflated square and the values chosen for it on the CPU.
"""
import numpy as np

import shell_reference as SR

LD = SR.LD
EPS = SR.EPS
_cross, _dot, _unit = SR._cross, SR._dot, SR._unit

# the Gauss rules on (-1, 1) in longdouble (numpy.polynomial.legendre.leggauss gives float64 only): closed forms
_S35, _S65 = np.sqrt(LD(3) / LD(5)), np.sqrt(LD(6) / LD(5))
_GAUSS = {
    1: ([LD(0)], [LD(2)]),
    2: ([-1 / np.sqrt(LD(3)), 1 / np.sqrt(LD(3))], [LD(1), LD(1)]),
    3: ([-_S35, LD(0), _S35], [LD(5) / 9, LD(8) / 9, LD(5) / 9]),
    4: ([-np.sqrt(LD(3) / 7 + LD(2) / 7 * _S65), -np.sqrt(LD(3) / 7 - LD(2) / 7 * _S65),
         np.sqrt(LD(3) / 7 - LD(2) / 7 * _S65), np.sqrt(LD(3) / 7 + LD(2) / 7 * _S65)],
        [(18 - np.sqrt(LD(30))) / 36, (18 + np.sqrt(LD(30))) / 36, (18 + np.sqrt(LD(30))) / 36, (18 - np.sqrt(LD(30))) / 36]),
}


def _midsurface(jet):
    """(a0, a1, a2, (d_0 a2, d_1 a2), a [q,2,2], b [q,2,2]) of the demo's midsurfaceGeometry from the jet [npts, 3, 6]"""
    a0, a1 = jet[:, :, 1], jet[:, :, 2]
    n = _cross(a0, a1)
    nn = np.sqrt(_dot(n, n))
    a2 = n / nn[:, None]
    second = {(0, 0): jet[:, :, 3], (0, 1): jet[:, :, 4], (1, 0): jet[:, :, 4], (1, 1): jet[:, :, 5]}
    a = np.stack([np.stack([_dot(a0, a0), _dot(a0, a1)], 1), np.stack([_dot(a1, a0), _dot(a1, a1)], 1)], 1)
    b = np.empty_like(a)
    da2 = []
    for beta in range(2):
        dn = _cross(second[(0, beta)], a1) + _cross(a0, second[(1, beta)])          # d_beta (a0 x a1)
        da2.append((dn - a2 * _dot(a2, dn)[:, None]) / nn[:, None])                 # d_beta of the unit vector
        b[:, 0, beta], b[:, 1, beta] = -_dot(a0, da2[beta]), -_dot(a1, da2[beta])
    return a0, a1, a2, da2, a, b


def _inv2(m):
    det = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]
    out = np.empty_like(m)
    out[:, 0, 0], out[:, 1, 1], out[:, 0, 1], out[:, 1, 0] = m[:, 1, 1] / det, m[:, 0, 0] / det, -m[:, 0, 1] / det, -m[:, 1, 0] / det
    return out, det


def _tensor_to_cartesian(T, a, a0, a1):
    ac, _ = _inv2(a)
    a0c = ac[:, 0, 0, None] * a0 + ac[:, 0, 1, None] * a1
    a1c = ac[:, 1, 0, None] * a0 + ac[:, 1, 1, None] * a1
    e0 = _unit(a0)
    e1 = _unit(a1 - e0 * _dot(a1, e0)[:, None])
    ea = np.stack([np.stack([_dot(e0, a0c), _dot(e0, a1c)], 1), np.stack([_dot(e1, a0c), _dot(e1, a1c)], 1)], 1)
    return np.einsum("qab,qbc,qdc->qad", ea, T, ea)


def demo_energy(Xjet, ujet, mu, h, n_thickness=4, details=None):
    """psi per unit reference area, as the demo writes it; jets [npts, 3, 6] of one dtype.  ``details``: a dict that receives
    the smallest det Gm and det C_2D met."""
    dt = Xjet.dtype.type
    A0, A1, A2, dA2, A, B = _midsurface(Xjet)
    a0, a1, a2, da2, a, b = _midsurface(Xjet + ujet)
    xs, ws = _GAUSS[n_thickness]
    mu = dt(mu)
    total = np.zeros(Xjet.shape[0], dtype=Xjet.dtype)
    for x, w in zip(xs, ws):
        xi2, wt = dt(h) * dt(float(x)) / dt(2), dt(h) * dt(float(w)) / dt(2)   # the demo's rule holds float64 constants
        G, g = A - dt(2) * xi2 * B, a - dt(2) * xi2 * b
        E_flat = dt(0.5) * (g - G)
        G0, G1 = A0 + xi2 * dA2[0], A1 + xi2 * dA2[1]
        E_2D = _tensor_to_cartesian(E_flat, G, G0, G1)
        C_2D = dt(2) * E_2D
        C_2D[:, 0, 0] += dt(1)
        C_2D[:, 1, 1] += dt(1)
        detC = C_2D[:, 0, 0] * C_2D[:, 1, 1] - C_2D[:, 0, 1] * C_2D[:, 1, 0]
        C22 = dt(1) / detC
        J = np.sqrt(detC * C22)
        psi_el = dt(0.5) * mu * (C_2D[:, 0, 0] + C_2D[:, 1, 1] + C22 - dt(3))
        p = mu * C22                                              # 2 (d psi_el / d C)_22 C_22
        total += wt * (psi_el - p * (J - dt(1)))
        if details is not None:
            detG = G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] * G[:, 1, 0]
            details["min_det_Gm"] = min(details.get("min_det_Gm", np.inf), float(np.min(detG)))
            details["min_det_C2D"] = min(details.get("min_det_C2D", np.inf), float(np.min(detC)))
    return total


def pressure_load(P, Xjet, ujet):
    """(s [npts, 3, 6], T [npts, 3, 6, 3, 6]) of dWext = -P sqrt(det a / det A) a_3 . v per unit reference area: the load in
    the value slot, and its derivative with d sqrt(det a) = sqrt(det a) a^c . dx_,c and d a_3 = -a^c (a_3 . dx_,c):
    d (sqrt(det a) a_3)_i / d x_j,c = sqrt(det a) (a_3i a^c_j - a^c_i a_3j)"""
    dt = Xjet.dtype.type
    _, _, _, _, A, _ = _midsurface(Xjet)
    a0, a1, a2, _, a, _ = _midsurface(Xjet + ujet)
    ai, deta = _inv2(a)
    _, detA = _inv2(A)
    ratio = np.sqrt(deta / detA)
    up = [ai[:, c, 0, None] * a0 + ai[:, c, 1, None] * a1 for c in range(2)]
    s = np.zeros(Xjet.shape, dtype=Xjet.dtype)
    T = np.zeros(Xjet.shape + (3, 6), dtype=Xjet.dtype)
    s[:, :, 0] = (-dt(P) * ratio)[:, None] * a2
    for c in range(2):
        T[:, :, 0, :, 1 + c] = (-dt(P) * ratio)[:, None, None] * (np.einsum("qi,qj->qij", a2, up[c]) - np.einsum("qi,qj->qij", up[c], a2))
    return s, T


class HyperShellReference(SR.ShellReference):
    """``ShellReference`` with a follower pressure ``P`` (None: none) in residual and tangent, and the demo's hyperelastic
    energy"""
    P = None

    def energy(self, u, material):
        X, U = self.jets(u)
        return np.sum(self.ref.wdet * demo_energy(X, U, material.mu, material.thickness, material.n_thickness))

    def residual(self, u, material, f=None):
        r = SR.ShellReference.residual(self, u, material, f)
        if self.P is not None:
            r = r + self.ref.load(pressure_load(self.P, *self.jets(u))[0])
        return r

    def tangent(self, u, material):
        K = SR.ShellReference.tangent(self, u, material)
        if self.P is not None:
            K = K + self.ref.matrix(pressure_load(self.P, *self.jets(u))[1])
        return K




def make_inadmissible(X, U, q, size=10.0):
    """adds ``size`` times the current normal to u_,00 at point q: b_00 = x_,00 . a_3 rises by ``size`` while the normal and the
    midsurface metric stay, so gm_00 = a_00 - 2 xi b_00 is negative at the thickness points xi > a_00 / (2 size), and
    det C_2D with it"""
    x1, x2 = X[q, :, 1] + U[q, :, 1], X[q, :, 2] + U[q, :, 2]
    n = np.cross(x1.astype(np.float64), x2.astype(np.float64))
    U[q, :, 3] += (size * n / np.linalg.norm(n)).astype(U.dtype)


# ---- the inflated square of the demo: [-1, 1]^2, two rows of control points clamped on every edge, follower pressure --------
MU, THICKNESS = 1.0e4, 0.03
# Chosen on the CPU with the host flow below (scanned: 4, 6, 8 elements per direction, first-step pressures 0.5 .. 2.5), so that
# each of the three equal load steps converges in at most 8 Newton steps at tolerance 1e-9 and the centre deflection after the
# last one is at least 3 h.  The first step, from the flat state, is the hard one: at the pressures that reach 3 h it takes 8 or
# 9 Newton steps, and no single (element count, pressure) met both conditions for both degrees -- so each degree has its own.
# The dense host flows take 2 s (p = 2) and 25 s (p = 3): their dofs and histories are recorded in
# tests/golden/shell_hyper_inflation.json (written by ``record_inflation``).
INFLATION = {2: dict(nel=4, pressure=3.9), 3: dict(nel=6, pressure=3.0)}
INFLATION_STEPS = 3
NEWTON_TOL = 1e-9
_FLOWS = {}


def square_homogeneous(t0, t1):
    return 2.0 * t0 - 1.0, 2.0 * t1 - 1.0, np.zeros_like(t0), np.ones_like(t0)


def inflation_problem(p):
    """the square with the chosen element count of degree p; ``free``: all dofs but two rows of control points on every edge"""
    nel = INFLATION[p]["nel"]
    pb = SR.problem(p, (nel, nel), square_homogeneous)
    n0, n1 = pb["C"].shape[:2]
    idx = np.arange(pb["ncp"]).reshape((n0, n1), order="F")
    inner = idx[2:-2, 2:-2].ravel()
    pb["free"] = np.sort(np.concatenate([f * pb["ncp"] + inner for f in range(3)]))
    return pb


def centre_deflection(pb, U):
    """u_z at the centre of the square from the dofs U"""
    return SR.centre_deflection(pb, U)


def inflation_flow(p, law, steps_run=INFLATION_STEPS, max_iters=25):
    """(problem, dofs after every load step run [steps_run, 3 ncp], Newton histories) of the dense host flow in float64: the
    pressure rises in INFLATION_STEPS equal steps, each solved by ``shell_reference.newton`` from the last state"""
    key = (p, steps_run, law.mu, law.thickness, law.n_thickness)
    if key not in _FLOWS:
        pb = inflation_problem(p)
        ref = HyperShellReference(pb["uks"], p, pb["cp"], dtype=np.float64)
        U = np.zeros(3 * pb["ncp"])
        states, histories = [], []
        for k in range(steps_run):
            ref.P = INFLATION[p]["pressure"] * (k + 1) / INFLATION_STEPS
            U, hist = SR.newton(ref, pb["Mc"], pb["free"], law, U, tol=NEWTON_TOL, max_iters=max_iters)
            states.append(U.copy())
            histories.append(hist)
        _FLOWS[key] = (pb, np.array(states), histories)
    return _FLOWS[key]


def record_inflation(law, path):
    """writes tests/golden/shell_hyper_inflation.json"""
    import json
    import time
    rec = dict(mu=law.mu, thickness=law.thickness, n_thickness=law.n_thickness, steps=INFLATION_STEPS, tolerance=NEWTON_TOL, flows={})
    for p in sorted(INFLATION):
        t0 = time.time()
        pb, states, hists = inflation_flow(p, law)
        rec["flows"][str(p)] = dict(nel=INFLATION[p]["nel"], pressure=INFLATION[p]["pressure"], seconds=round(time.time() - t0, 1),
                                    histories=[[float(v) for v in h] for h in hists],
                                    centre_deflection=[centre_deflection(pb, U) for U in states],
                                    dofs=[[float(v) for v in U] for U in states])
    with open(path, "w") as f:
        json.dump(rec, f, indent=0)
