"""The quasilinear model problem of the coefficient-form tests:

    -div(grad u / sqrt(1 + |grad u|^2)) + u^3 = f      on the quarter annulus 1 <= r <= 2, 0 <= theta <= pi / 2, u = 0 on all edges

with the manufactured solution u = (r - 1)(2 - r) sin 2 theta of ``postproc_reference.annulus_exact``, in the rational
space of degree 2.  ``residual`` / ``tangent`` are the callables ``forms.QuasilinearResidual`` takes; ``host_flow`` is the
Newton iteration of ``coef_reference.newton`` with dense solves.
"""
import numpy as np

from oracle import tigar_oracle as O
import postproc_reference as R
import coef_reference as CR

exact, exact_grad = R.annulus_exact, R.annulus_exact_grad


def rhs(x):
    """f = -div(grad u / s) + u^3 with s = sqrt(1 + |grad u|^2):  div(grad u / s) = lap u / s - (grad u . H grad u) / s^3, the
    Hessian H in the orthonormal polar frame"""
    r, th = np.hypot(x[:, 0], x[:, 1]), np.arctan2(x[:, 1], x[:, 0])
    a, a1, a2 = (r - 1.0) * (2.0 - r), 3.0 - 2.0 * r, -2.0
    s2, c2 = np.sin(2.0 * th), np.cos(2.0 * th)
    ur, ut = a1 * s2, 2.0 * a * c2                     # u_r, u_theta
    urr, urt, utt = a2 * s2, 2.0 * a1 * c2, -4.0 * a * s2
    gr, gt = ur, ut / r
    hrr, hrt, htt = urr, urt / r - ut / r ** 2, utt / r ** 2 + ur / r
    s = np.sqrt(1.0 + gr ** 2 + gt ** 2)
    lap = hrr + htt
    return -(lap / s - (gr * gr * hrr + 2.0 * gr * gt * hrt + gt * gt * htt) / s ** 3) + (a * s2) ** 3


def residual(x, u, g):
    s = np.sqrt(1.0 + np.sum(g * g, axis=1))
    return g / s[:, None], u ** 3


def tangent(x, u, g):
    s = np.sqrt(1.0 + np.sum(g * g, axis=1))
    A = np.eye(g.shape[1])[None] / s[:, None, None] - g[:, :, None] * g[:, None, :] / (s ** 3)[:, None, None]
    return A, None, None, 3.0 * u ** 2


def annulus(nel):
    """(knot vector, control net, oracle spline, element vertices, extraction matrix, control functions, free dofs)"""
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    s = O.BSpline([2, 2], [kv, kv])
    uks = [np.asarray(s1.uniqueKnots, dtype=np.float64) for s1 in s.splines]
    Mc = O.generate_M_tensor(s)
    cp = [np.asarray(Mc @ Pf[:, :, i].ravel(order="F")) for i in range(3)]
    ncp = Mc.shape[1]
    n1 = int(round(np.sqrt(ncp)))
    idx = np.arange(ncp).reshape(n1, n1, order="F")
    bd = np.unique(np.concatenate([idx[0], idx[-1], idx[:, 0], idx[:, -1]]))
    return kv, Pf, uks, Mc, cp, np.setdiff1d(np.arange(ncp), bd)


def host_flow(nel):
    """(dofs, history of the relative residual norms, (L2, H10) errors) of the host Newton flow, tolerance 1e-10"""
    kv, Pf, uks, Mc, cp, free = annulus(nel)
    ref = CR.CoefReference(uks, 2, cp, rational=True, dtype=np.float64)
    U, hist = CR.newton(ref, Mc, free, residual, tangent, f=rhs(ref.x), tol=1e-10)
    return U, hist, ref.errors(Mc @ U, exact(ref.x), exact_grad(ref.x))
