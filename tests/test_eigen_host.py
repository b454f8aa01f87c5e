"""CPU: the host pieces of the block LOBPCG eigensolver (tigar_amd/eigen.py) on small numpy pencils -- the Rayleigh-Ritz
and basis-selection step, the restart without P, and merging the eigenpairs of decoupled rows into the sorted spectrum."""
import numpy as np
import pytest
import scipy.linalg as sl

from tigar_amd import eigen as E


def _pencil(n, seed):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, n))
    A = Q @ Q.T + n * np.eye(n)
    R = rng.standard_normal((n, n))
    B = R @ R.T / n + np.eye(n)
    return A, B


def test_svqb_orthonormalizes_and_drops_dependent_directions():
    rng = np.random.default_rng(0)
    _, B = _pencil(30, 1)
    W = rng.standard_normal((30, 6))
    W[:, 5] = W[:, 0] - 2.0 * W[:, 3]           # dependent
    T = E.svqb(W.T @ B @ W)
    assert T.shape == (6, 5)
    V = W @ T
    assert np.abs(V.T @ B @ V - np.eye(5)).max() < 1e-12
    assert E.svqb(np.zeros((3, 3))).shape == (3, 0)


def test_cholesky_qr_factor():
    _, B = _pencil(8, 2)
    R = E.cholesky_qr_factor(B)
    assert np.allclose(R.T @ R, B, rtol=1e-14, atol=1e-13)
    assert E.cholesky_qr_factor(-B) is None
    assert E.cholesky_qr_factor(np.full((2, 2), np.nan)) is None


def test_rayleigh_ritz_and_basis_selection_step():
    """one step on a basis [X, W, P] of a dense pencil: the Ritz values bound the true ones from above, the Ritz
    coefficients are GB-orthonormal and the new P is GB-orthonormal and GB-orthogonal to the new X"""
    n, m = 40, 4
    A, B = _pencil(n, 3)
    rng = np.random.default_rng(4)
    S = rng.standard_normal((n, 3 * m))
    S = S @ E.svqb(S.T @ B @ S)                 # B-orthonormal basis
    GA, GB = S.T @ A @ S, S.T @ B @ S
    active = [0, 2, 3]
    theta, C, Z, restarted = E.rr_step(GA, GB, m, m, m, active)
    assert not restarted
    true = sl.eigh(A, B, eigvals_only=True)[:m]
    assert np.all(theta >= true - 1e-10 * np.abs(true))
    assert np.allclose(theta, sl.eigh(GA, GB, eigvals_only=True)[:m], rtol=1e-12)
    assert np.abs(C.T @ GB @ C - np.eye(m)).max() < 1e-12
    assert Z.shape == (3 * m, len(active))
    assert np.abs(Z.T @ GB @ Z - np.eye(len(active))).max() < 1e-10
    assert np.abs(C.T @ GB @ Z).max() < 1e-10
    # Z has no X part before the orthogonalization against C: its span lies in the W, P rows plus the span of C
    Zraw = C[:, active].copy()
    Zraw[:m] = 0.0
    proj = Zraw - C @ (C.T @ GB @ Zraw)
    assert np.linalg.matrix_rank(np.hstack([proj, Z]), tol=1e-8) == len(active)


def test_restart_without_p_when_the_gram_matrix_is_singular():
    n, m = 30, 3
    A, B = _pencil(n, 5)
    rng = np.random.default_rng(6)
    X = rng.standard_normal((n, m))
    X = X @ E.svqb(X.T @ B @ X)
    W = rng.standard_normal((n, m))
    W = W @ E.svqb(W.T @ B @ W)
    P = X[:, :2].copy()                         # P inside span X: GB singular
    S = np.hstack([X, W, P])
    GA, GB = S.T @ A @ S, S.T @ B @ S
    with pytest.raises(np.linalg.LinAlgError):
        E.rayleigh_ritz(GA, GB, m)
    theta, C, Z, restarted = E.rr_step(GA, GB, m, m, m, [0, 1, 2])
    assert restarted and C.shape == (2 * m, m) and Z.shape[0] == 2 * m
    S2 = np.hstack([X, W])
    assert np.allclose(theta, sl.eigh(S2.T @ A @ S2, S2.T @ B @ S2, eigvals_only=True)[:m], rtol=1e-12)
    with pytest.raises(np.linalg.LinAlgError):       # without P there is nothing to drop
        E.rr_step(GA[:2 * m, :2 * m] * 0 - np.eye(2 * m), -np.eye(2 * m), m, m, m, [0])


def test_merge_decoupled_pairs():
    free = [12.36, 485.5, 3806.5]
    # demo: diag = 1 / DOLFIN_EPS in A, 1 in B -> far above the requested modes
    pen = 1.0 / 3.0e-16
    got = E.merge_decoupled(free, [pen, pen], 3)
    assert [s for _, s, _ in got] == ["free"] * 3 and [v for v, _, _ in got] == free
    # diag = 1 in both: lambda = 1 first, with the multiplicity of the zero dofs
    got = E.merge_decoupled(free, [1.0, 1.0], 3)
    assert got == [(1.0, "decoupled", 0), (1.0, "decoupled", 1), (12.36, "free", 0)]
    # ties keep the free pair first; interleaving is by value
    got = E.merge_decoupled([1.0, 5.0], [0.5, 1.0, 7.0], 5)
    assert got == [(0.5, "decoupled", 0), (1.0, "free", 0), (1.0, "decoupled", 1), (5.0, "free", 1),
                   (7.0, "decoupled", 2)]


def test_default_block_size():
    assert E.default_block_size(5, 10000) == 7
    assert E.default_block_size(11, 10000) == 16
    assert E.default_block_size(48, 10 ** 6) == 64
    assert E.default_block_size(10, 40) == 13          # (40 - 1) // 3
    assert E.default_block_size(10, 20) == 10          # never below the pairs requested (refused later)


def test_refusals_before_any_device_work():
    class Two:
        size = 2
    with pytest.raises(NotImplementedError):
        E.SLEPcEigenSolver(np.eye(4), comm=Two())
    with pytest.raises(ValueError, match="not square"):
        E.SLEPcEigenSolver(np.ones((3, 4)))
