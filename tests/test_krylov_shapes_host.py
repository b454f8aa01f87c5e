"""The test-matrix family of tests/krylov_shapes.py on the host: every member lands on the register shape of the persistent
Krylov kernels it was made for, has its exact longest row, converges quickly in the oracle's CG and GMRES, and moves its exact
solution by far more than the tolerance of tests/test_gpu_krylov_shapes.py when ONE entry of ONE row is lost -- which is what
lets that tolerance see a row index that is off in one batch of the unrolled product."""
import numpy as np
import pytest

import krylov_shapes as S
from oracle import tigar_oracle as O

GPU_TOLERANCE = 1e-8            # max-norm error bound of the GPU tests, relative
NUM_CU = 256                    # MI355X
SEED = 20


def _cases():
    return [pytest.param(E, R, top, id="%d-%d-%s" % (E, R, "top" if top else "low")) for E, R in S.PS_SHAPES
            for top in (True, False)]


def test_expected_shape_restates_the_selection():
    # the natural number of workgroups: min(CUs, ceil(n / 16)); the second shape of a class from 16 R_prev * 256 rows up
    assert S.expected_shape(5000, 49, NUM_CU, S.PS_ROWS_MAX) == (2, 8, 256)
    assert S.expected_shape(16 * 4 * 256 + 1, 100, NUM_CU, S.PS_ROWS_MAX) == (4, 8, 256)
    assert S.expected_shape(16 * 48 * 256 + 1, 32, NUM_CU, S.PS_ROWS_MAX) == (1, 56, 256)
    assert S.expected_shape(16 * 56 * 256 + 1, 32, NUM_CU, S.PS_ROWS_MAX) is None
    assert S.expected_shape(40, 3, NUM_CU, S.PS_ROWS_MAX) == (1, 16, 3)
    # the cap lowers, never raises; 0 and negative values are no cap
    assert S.expected_shape(2686, 32, NUM_CU, S.PS_ROWS_MAX, cap=3) == (1, 56, 3)
    assert S.expected_shape(40, 3, NUM_CU, S.PS_ROWS_MAX, cap=100) == (1, 16, 3)
    assert S.expected_shape(5000, 49, NUM_CU, S.PS_ROWS_MAX, cap=0) == (2, 8, 256)
    assert S.expected_shape(5000, 49, NUM_CU, S.PS_ROWS_MAX, cap=-4) == (2, 8, 256)
    # refusals: rows per workgroup, longest row
    assert S.expected_shape(1026, 32, NUM_CU, S.PS_ROWS_MAX, cap=1) is None
    assert S.expected_shape(225 * 3, 32, NUM_CU, S.PG_ROWS, cap=3) is None
    assert S.expected_shape(5000, 161, NUM_CU, S.PS_ROWS_MAX) is None
    assert S.expected_shape(5000, 160, NUM_CU, S.PS_ROWS_MAX) == (5, 4, 256)
    assert S.expected_shape(5000, 0, NUM_CU, S.PS_ROWS_MAX) is None


@pytest.mark.parametrize("E,R,top", _cases())
def test_family_member_lands_on_its_shape_and_sees_a_lost_entry(E, R, top):
    G = 3
    for symmetric in (True, False):
        A, b, exact = S.reference(E, R, G, top, symmetric, SEED)
        n = A.shape[0]
        per = 16 * R if top else 16 * R - 1
        assert n % 2 == 0 and -(-n // G) == per and n - (G - 1) * per < per          # a short last block
        assert n <= 2686
        assert A.has_sorted_indices and np.all(np.diff(A.indptr) >= 1)
        assert S.longest_row(A) == (32 * E if top else 32 * (E - 1) + 1)
        assert S.expected_shape(n, S.longest_row(A), NUM_CU, S.PS_ROWS_MAX, cap=G) == (E, R, G)
        assert np.all(np.diff(A.indptr)[:3] == S.longest_row(A))                      # rows 0, 1, 2 are full
        if E > 1 or top:
            assert np.diff(A.indptr).min() < S.longest_row(A)                        # ragged
            # columns span the whole matrix: row 0 reaches into every workgroup's block
            assert len(set(A.indices[A.indptr[0]:A.indptr[1]] // per)) == G
        if symmetric:
            assert (A != A.T).nnz == 0
        else:
            assert E == 1 and not top or (A != A.T).nnz > 0
        dinv = S.jacobi_dinv(A)
        bnorm = np.linalg.norm(dinv * b)
        if symmetric:
            x, its, res = O.cg_jacobi(A, b, rtol=1e-10, atol=1e-300, maxit=40)
        else:
            x, its, res = O.gmres_jacobi(A, b, rtol=1e-10, atol=1e-300, maxit=40, restart=30)
        assert its <= 40 and res <= 1e-10 * bnorm, (its, res / bnorm)
        assert np.max(np.abs(x - exact)) <= 1e-8 * np.max(np.abs(exact))
        # ONE entry of row 0 lost: the exact solution moves by >= 1e3 tolerances.  To first order x_0 moves by a_0j x_j / a_00,
        # and a standard normal a_0j (or an x_j) can be as small as one likes -- no tolerance sees the loss of an entry that
        # contributes nothing --, so the entry taken away is a TYPICAL one: the median of |a_0j x_j| over the row.
        if A.indptr[1] - A.indptr[0] > 1:
            a, e = A.indptr[0], A.indptr[1]
            offd = np.flatnonzero(A.indices[a:e] != 0)
            weight = np.abs(A.data[a:e][offd] * exact[A.indices[a:e][offd]])
            which = int(np.argsort(weight, kind="stable")[offd.size // 2])
            moved = S.direct_solve(S.without_entry(A, 0, which), b)
            shift = np.max(np.abs(moved - exact)) / np.max(np.abs(exact))
            assert shift >= 1e3 * GPU_TOLERANCE, shift
        else:
            assert E == 1 and not top                 # (the diagonal member: nothing to lose but the diagonal itself)


@pytest.mark.parametrize("E,R", [(2, 8), (5, 11)])
def test_dead_diagonals_keep_the_family_solvable(E, R):
    A, b, exact = S.reference(E, R, 3, True, False, SEED)
    D, bd, exact_d = S.reference(E, R, 3, True, False, SEED, dead=True)
    n = A.shape[0]
    assert np.array_equal(b, bd)
    assert D.nnz == A.nnz - 2 and S.longest_row(D) == S.longest_row(A)
    assert np.array_equal(np.flatnonzero(D.diagonal() == 0.0), [0, 5, n // 2, n - 1])
    assert S.expected_shape(n, S.longest_row(D), NUM_CU, S.PG_ROWS, cap=3) == (E, R, 3)
    x, its, res = O.gmres_jacobi(D, b, rtol=1e-10, atol=1e-300, maxit=40, restart=30)
    assert its <= 40 and res <= 1e-10 * np.linalg.norm(S.jacobi_dinv(D) * b)
    # (error <= condition number x residual: the condition numbers are 4e2 and 5e3, see tests/test_gpu_krylov_shapes.py)
    assert np.max(np.abs(x - exact_d)) <= 1e4 * 1e-10 * np.max(np.abs(exact_d))
