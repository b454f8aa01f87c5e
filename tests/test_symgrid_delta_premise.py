"""The assumption the delta-coded values of the half-storage product rest on (csrc/tg_symgrid.hip): on a patch with
uniform knots the rows (i, j, k) and (i, j, k_ref) of K = M^T A M are equal up to rounding, and as 64-bit integers the two
doubles of a stored position differ by far less than an int16 holds.  Checked on the CPU with the oracle's own 1-D tables, K
formed as the Kronecker sum of the 1-D M1^T K1 M1 and M1^T M1 M1 -- should node placement or the 1-D tables ever change."""
import itertools

import numpy as np
import pytest

from oracle import tigar_oracle as O


def _one_d(p, nel):
    """dense K1 = M1^T K_fe M1 and S1 = M1^T M_fe M1 of the 1-D spline with nel uniform elements"""
    s1 = O.BSpline1(p, O.uniform_knots(p, 0., 1., nel))
    xs = O.fe_nodes_1d(s1)
    nodes, vals = O._eval_1d_table(s1, xs)
    M1 = np.zeros((len(xs), s1.getNcp()))
    for a in range(len(xs)):
        M1[a, nodes[a]] = vals[a]
    Mfe, Kfe = O.fe_1d_matrices(np.asarray(s1.uniqueKnots, dtype=float), p)
    return M1.T @ (Kfe @ M1), M1.T @ (Mfe @ M1)


@pytest.mark.parametrize("p,nel,measured", [(3, 256, 1276), (3, 100, 1106), (2, 128, 0)])
def test_rows_of_other_planes_are_within_int16_of_the_reference_plane(p, nel, measured):
    K1, S1 = _one_d(p, nel)
    n = K1.shape[0]
    kref = n // 2
    offs = [o for o in itertools.product(range(-p, p + 1), repeat=3) if o >= (0, 0, 0)]      # the stored half
    dz = np.array([o[0] for o in offs])
    dy = np.array([o[1] for o in offs])
    dx = np.array([o[2] for o in offs])
    planes = np.arange(2 * p, n - 2 * p)

    def rows(i, j, ks):
        """stored values of the rows (i, j, k), k in ks: S1z (x) S1y (x) K1x + S1z (x) K1y (x) S1x + K1z (x) S1y (x) S1x"""
        sx, kx, sy, ky = S1[i, i + dx], K1[i, i + dx], S1[j, j + dy], K1[j, j + dy]
        sz, kz = S1[ks[:, None], ks[:, None] + dz[None, :]], K1[ks[:, None], ks[:, None] + dz[None, :]]
        return sz * sy * kx + sz * ky * sx + kz * sy * sx

    rng = np.random.default_rng(p * 1000 + nel)
    worst = 0
    for _ in range(40):
        i, j = (int(v) for v in rng.integers(p, n - p, size=2))
        v = rows(i, j, planes).view(np.int64)
        t = rows(i, j, np.array([kref])).view(np.int64)
        worst = max(worst, int(np.abs(v - t).max()))
    print("p = %d, %d elements: largest integer distance to the reference plane %d (recorded: %d)" % (p, nel, worst, measured))
    assert worst < 2 ** 15
