"""Plain reference of the fast diagonalization application (csrc/tg_fd.hip), for the kernel tests: the same operation
from the same Q, lam, dk, dm, coefficients and diag K the device is given, in any numpy float type (numpy.longdouble as
the reference proper, float64 for numpy's own rounding error), with the kernel's rules for its three decisions:

  * 1 / s with s = c_m + sum_k c_k lam_k[i_k] where s > floor, else 0; floor = 1e-13 (c_m + sum_k c_k max |lam_k|)
  * S = sqrt(dp / dg) where dg > 0 and dp > 0, else 1 (dg = K_ii, dp = P_ii from the 1-D diagonals)
  * off the box z_i = r_i / K_ii, r_i itself where K_ii == 0

Arrays of a block are indexed [i_{d-1}, ..., i_0] (direction 0 fastest, as the dofs are numbered); per-direction lists are
indexed by direction.  No fixtures here (like geom_util.py): a module the tests import."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53          # unit roundoff of float64


def modes(X, mats):
    """mats[k] acts on direction k: Y[.., i, ..] = sum_l mats[k][l][i] X[.., l, ..]"""
    d = X.ndim
    for k, A in enumerate(mats):
        X = np.moveaxis(np.tensordot(A.T, np.moveaxis(X, d - 1 - k, 0), axes=(1, 0)), 0, d - 1 - k)
    return X


def _along(v, k, d):
    sh = [1] * d
    sh[d - 1 - k] = -1
    return np.asarray(v).reshape(sh)


def floor_of(lams, coef):
    """the pseudo-inverse floor as tg_fd_set_coefficients forms it (float64); coef = (c_0, .., c_{d-1}, c_m)"""
    d = len(lams)
    top = float(coef[d])
    for k in range(d):
        top += float(coef[k]) * float(np.max(np.abs(lams[k])))
    return 1e-13 * top


def eig_sums(lams, coef, dt=LD):
    """s[i] = c_m + sum_k c_k lam_k[i_k]"""
    d = len(lams)
    s = np.full([len(l) for l in lams][::-1], dt(coef[d]), dtype=dt)
    for k in range(d):
        s = s + dt(coef[k]) * _along(np.asarray(lams[k]).astype(dt), k, d)
    return s


def fd_box(x, Qs, lams, coef, floor, dt=LD):
    """(Q x .. x Q) diag(1 / s, 0 where s <= floor) (Q^T x .. x Q^T) x on the box"""
    Qs = [np.asarray(q).astype(dt) for q in Qs]
    X = modes(np.asarray(x).astype(dt), Qs)
    s = eig_sums(lams, coef, dt)
    keep = s > dt(floor)
    X = np.where(keep, X / np.where(keep, s, dt(1)), dt(0))
    return modes(X, [q.T for q in Qs])


def diag_p(dk, dm, coef, dt=LD):
    """diag P on the box from the 1-D stiffness / mass diagonals"""
    d = len(dk)
    dk = [np.asarray(v).astype(dt) for v in dk]
    dm = [np.asarray(v).astype(dt) for v in dm]

    def term(a):
        out = np.ones([1] * d, dtype=dt)
        for k in range(d):
            out = out * _along(dk[k] if k == a else dm[k], k, d)
        return out
    dp = dt(coef[d]) * term(-1)
    for a in range(d):
        dp = dp + dt(coef[a]) * term(a)
    return dp


def box_slices(lo, hi):
    d = len(lo)
    return tuple(slice(int(lo[d - 1 - a]), int(hi[d - 1 - a])) for a in range(d))


def scaling_vector(dg, lo, hi, dk, dm, coef, scaling, dt=LD):
    """sv on the grid of one block (dg = diag K there, shape N[::-1]): S on the box, 1 / K_ii (1 where K_ii == 0) off it"""
    dg = np.asarray(dg)
    nz = dg != 0
    sv = np.where(nz, dt(1) / np.where(nz, dg, 1.0).astype(dt), dt(1))
    box = box_slices(lo, hi)
    if scaling:
        dgb = dg[box]
        dp = diag_p(dk, dm, coef, dt)
        ok = (dgb > 0) & (dp > 0)
        sv[box] = np.where(ok, np.sqrt(np.where(ok, dp, dt(1)) / np.where(ok, dgb, 1.0).astype(dt)), dt(1))
    else:
        sv[box] = dt(1)
    return sv


def fd_apply(r, dg, lo, hi, Qs, lams, dk, dm, coef, scaling, dt=LD):
    """z = S P^+ S r on the box, r / K_ii off it, for one block; r, dg, z of shape N[::-1]"""
    r = np.asarray(r).astype(dt)
    sv = scaling_vector(dg, lo, hi, dk, dm, coef, scaling, dt)
    box = box_slices(lo, hi)
    z = sv * r
    z[box] = sv[box] * fd_box(sv[box] * r[box], Qs, lams, coef, floor_of(lams, coef), dt)
    return z


def fd_absprod(r, dg, lo, hi, Qs, lams, dk, dm, coef, scaling):
    """the same chain on the box with |Q|, |1 / s|, |S|, |r| (float64: it scales a bound), shape nf[::-1]"""
    dt = np.float64
    box = box_slices(lo, hi)
    sv = np.abs(scaling_vector(dg, lo, hi, dk, dm, coef, scaling, dt)[box])
    aq = [np.abs(np.asarray(q, dtype=dt)) for q in Qs]
    X = modes(sv * np.abs(np.asarray(r, dtype=dt)[box]), aq)
    s = eig_sums(lams, coef, dt)
    keep = s > floor_of(lams, coef)
    X = np.where(keep, X / np.abs(np.where(keep, s, 1.0)), 0.0)
    return sv * modes(X, [q.T for q in aq])


def hard_bound(nfs, absprod):
    """first-order running-error bound of one application, elementwise: 2d chained dot products of the padded lengths,
    the division and the two scalings (s, dp and the square root formed in float64, a handful of roundings each, twice)"""
    nps = [(int(n) + 15) // 16 * 16 for n in nfs]
    return (2 * sum(nps) + 32) * U * absprod


def fit_sums(dg, lo, hi, dk, dm, dt=LD):
    """the four sums <diag K, t_a> over the box (a < d: stiffness in direction a, 0 for a >= d; 3: mass) and the same
    with |diag K t_a|"""
    d = len(dk)
    dgb = np.asarray(dg)[box_slices(lo, hi)].astype(dt)
    out, mag = np.zeros(4, dtype=dt), np.zeros(4, dtype=dt)
    for a in list(range(d)) + [3]:
        c = [0.0] * (d + 1)
        c[a if a < d else d] = 1.0
        t = dgb * diag_p(dk, dm, c, dt)
        out[a], mag[a] = t.sum(), np.abs(t).sum()
    return out, mag


def kron(mats):
    """Kronecker product with direction 0 fastest"""
    out = np.ones((1, 1))
    for m in mats[::-1]:
        out = np.kron(out, m)
    return out


def dense_p(Ks, Ms, coef):
    """P = sum_k c_k (M x .. K_k .. x M) + c_m (M x .. x M) from the 1-D matrices on the free box"""
    d = len(Ks)
    P = coef[d] * kron(Ms)
    for k in range(d):
        P = P + coef[k] * kron([Ks[j] if j == k else Ms[j] for j in range(d)])
    return P


def iga_1d(p, nel):
    """1-D B-spline stiffness / mass of the uniform open knot vector on [0, 1] with nel elements (nel + p functions):
    scipy's B-spline evaluation and p + 1 Gauss points per element"""
    from scipy.interpolate import BSpline
    t = np.r_[[0.0] * p, np.linspace(0.0, 1.0, nel + 1), [1.0] * p]
    n = nel + p
    xg, wg = np.polynomial.legendre.leggauss(p + 1)
    h = 1.0 / nel
    x = (t[p:p + nel, None] + 0.5 * (xg + 1.0) * h).ravel()
    w = np.tile(0.5 * h * wg, nel)
    N = BSpline.design_matrix(x, t, p).toarray()
    dN = np.stack([BSpline(t, np.eye(n)[i], p).derivative()(x) for i in range(n)], axis=1)
    return dN.T @ (w[:, None] * dN), N.T @ (w[:, None] * N)


def random_spd_pair(n, rng):
    """dense, sign-mixed SPD pencil: K = A A^T + n I, M = B B^T / n + I"""
    A, B = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    return A @ A.T + n * np.eye(n), B @ B.T / n + np.eye(n)


def eig_pencil(K1, M1):
    """Q, lam with Q^T M Q = I, Q^T K Q = lam; Q row-major Q[l][i] (column i the i-th vector)"""
    import scipy.linalg
    lam, Q = scipy.linalg.eigh(K1, M1)
    return np.ascontiguousarray(Q), lam
