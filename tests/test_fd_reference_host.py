"""CPU: the reference of the fast diagonalization kernel tests (tests/fd_reference.py) pinned against a dense solve with
the Kronecker P, and its float64 evaluation against its longdouble one."""
import numpy as np
import pytest

import fd_reference as R


def _case(name):
    rng = np.random.default_rng(11)
    if name == "2d":
        # B-spline pencils, p = 2 and 3; clamped on every side
        shape, lo, hi = [9, 8], [1, 1], [8, 7]
        mats = [R.iga_1d(2, 7), R.iga_1d(3, 5)]
        coef, scaling = [1.0, 2.0, 0.3], True
    else:
        # unequal sizes, direction 1 with lo = 0 (a face that is not clamped), direction 2 two layers deep
        shape, lo, hi = [8, 6, 9], [1, 0, 2], [7, 5, 7]
        mats = [R.iga_1d(2, 6), R.iga_1d(3, 3), R.random_spd_pair(9, rng)]
        coef, scaling = [1.0, 0.5, 2.0, 0.0], False
    d = len(shape)
    Ks = [mats[k][0][lo[k]:hi[k], lo[k]:hi[k]] for k in range(d)]
    Ms = [mats[k][1][lo[k]:hi[k], lo[k]:hi[k]] for k in range(d)]
    QL = [R.eig_pencil(Ks[k], Ms[k]) for k in range(d)]
    dk, dm = [np.diag(K).copy() for K in Ks], [np.diag(M).copy() for M in Ms]
    r = rng.standard_normal(shape[::-1])
    dg = rng.uniform(0.5, 2.0, size=shape[::-1])
    dg[R.box_slices(lo, hi)] *= R.diag_p(dk, dm, coef, np.float64)
    return dict(shape=shape, lo=lo, hi=hi, Ks=Ks, Ms=Ms, Qs=[q for q, _ in QL], lams=[l for _, l in QL], dk=dk, dm=dm,
                coef=coef, scaling=scaling, r=r, dg=dg)


@pytest.mark.parametrize("name", ["2d", "3d"])
def test_reference_matches_dense_solve(name):
    c = _case(name)
    args = (c["r"], c["dg"], c["lo"], c["hi"], c["Qs"], c["lams"], c["dk"], c["dm"], c["coef"], c["scaling"])
    zld = R.fd_apply(*args, dt=R.LD)
    z64 = R.fd_apply(*args, dt=np.float64)
    assert zld.dtype == R.LD and z64.dtype == np.float64
    box = R.box_slices(c["lo"], c["hi"])
    P = R.dense_p(c["Ks"], c["Ms"], c["coef"])
    dgb = c["dg"][box].ravel()
    S = np.sqrt(np.diag(P) / dgb) if c["scaling"] else np.ones(dgb.size)
    want = c["r"] / c["dg"]
    want[box] = (S * np.linalg.solve(P, S * c["r"][box].ravel())).reshape(want[box].shape)
    # (the relative norm tests/test_fast_diag_host.py::test_eig_reproduces_inverse asserts of the factored inverse)
    assert np.linalg.norm((zld - want).astype(np.float64)) <= 1e-11 * np.linalg.norm(want)
    assert np.linalg.norm((zld - z64).astype(np.float64)) <= 1e-13 * np.linalg.norm(z64)
    # the bound the GPU tests hold the kernel to holds for numpy's float64 evaluation with room to spare
    nfs = [h - l for l, h in zip(c["lo"], c["hi"])]
    bound = R.hard_bound(nfs, R.fd_absprod(*args))
    assert np.all(np.abs(z64[box] - zld[box]) <= bound)
    off = np.ones(zld.shape, dtype=bool)
    off[box] = False
    assert np.array_equal(z64[off], (1.0 / c["dg"] * c["r"])[off])


def test_reference_rules():
    """the three decisions of the kernel, on data where each branch is taken"""
    # pseudo-inverse: a pure Neumann box without a mass term has one eigenvalue sum at rounding level
    K1, M1 = R.iga_1d(2, 4)
    Q, lam = R.eig_pencil(K1, M1)
    coef = [1.0, 1.0, 0.0]
    floor = R.floor_of([lam, lam], coef)
    s = R.eig_sums([lam, lam], coef, np.float64)
    assert floor > 0 and np.sum(s <= floor) == 1 and np.all((s <= floor / 100) | (s >= 100 * floor))
    x = np.random.default_rng(2).standard_normal((6, 6))
    y = R.fd_box(x, [Q, Q], [lam, lam], coef, floor)
    # P^+ x has no component along the constant (the null vector of P): 1^T M y = 0 with M = M1 x M1
    ones = np.ones(6)
    assert abs(float(ones @ M1 @ y.astype(np.float64) @ M1 @ ones)) <= 1e-12 * np.linalg.norm(y.astype(np.float64))
    P = R.dense_p([K1, K1], [M1, M1], coef)
    res = P @ y.astype(np.float64).ravel() - x.ravel()
    # the residual is the part of x outside the range of P: a multiple of M 1
    m1 = np.kron(M1 @ ones, M1 @ ones)
    assert np.linalg.norm(res - (res @ m1) / (m1 @ m1) * m1) <= 1e-10 * np.linalg.norm(x)
    # S: 1 where diag K or diag P is not positive; off the box 1 / K_ii and 1 where K_ii == 0
    dg = np.array([[2.0, 0.0, -1.0, 4.0], [0.0, 8.0, -2.0, 0.5]])
    dk, dm = [np.array([1.0, 2.0]), np.array([3.0])], [np.array([0.5, 0.25]), np.array([2.0])]
    sv = R.scaling_vector(dg, [1, 0], [3, 1], dk, dm, [1.0, 1.0, 0.0], True, np.float64)
    dp = np.array([1.0 * 2.0 + 0.5 * 3.0, 2.0 * 2.0 + 0.25 * 3.0])
    assert np.array_equal(sv[0], [0.5, 1.0, 1.0, 0.25]) and np.array_equal(sv[1], [1.0, 0.125, -0.5, 2.0])
    assert np.array_equal(R.diag_p(dk, dm, [1.0, 1.0, 0.0], np.float64), dp.reshape(1, 2))
    sv = R.scaling_vector(np.abs(dg) + 1.0, [1, 0], [3, 1], dk, dm, [1.0, 1.0, 0.0], True, np.float64)
    assert np.allclose(sv[0, 1:3], np.sqrt(dp / np.array([1.0, 2.0])), rtol=1e-15)
    assert np.array_equal(R.scaling_vector(dg, [1, 0], [3, 1], dk, dm, [1.0, 1.0, 0.0], False, np.float64)[0], [0.5, 1, 1, 0.25])
    sums, mag = R.fit_sums(np.abs(dg) + 1.0, [1, 0], [3, 1], dk, dm)
    assert np.allclose(sums.astype(np.float64), [1.0 * 2.0 + 4.0 * 2.0, 0.5 * 3.0 + 2.0 * 0.25 * 3.0, 0.0, 1.0 + 2.0 * 0.5])
    assert np.array_equal(sums, mag)
