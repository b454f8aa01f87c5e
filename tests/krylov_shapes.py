"""Test matrices that land on a chosen register shape of the persistent Krylov kernels (csrc/tg_krylov_small.hip), plain
numpy / scipy.

A shape is (E, R): E entries per lane and row, R rows per group of 32 lanes.  ``ps_shape`` picks it from the longest row
(E = ceil(maxlen / 32)) and from per = ceil(n / G) rows per workgroup (the first R of the class with per <= 16 R); with
TIGAR_KSP_PERSISTENT_WGS the number of workgroups G is capped, so a few hundred to a few thousand rows reach every R.

The family is circulant in its pattern -- entries at (i, (i +- o) mod n) for random offsets o --, so the columns of every row
span the whole matrix (every product gathers from every workgroup), ragged (pairs are dropped at random: row lengths differ
from row to row), with the longest row exactly at the upper (``top``: 32 E) or the lower (32 (E - 1) + 1) end of the class,
and diagonally dominant with a diagonal that varies from row to row (condition number of order 10, a Jacobi scaling that is
not a multiple of the identity)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

# PS_SHAPES of csrc/tg_krylov_small.hip, in its order
PS_SHAPES = ((1, 16), (1, 32), (1, 48), (1, 56),
             (2, 8), (2, 16), (2, 24), (2, 28),
             (3, 6), (3, 12), (3, 17), (3, 18),
             (4, 4), (4, 8), (4, 12), (4, 14),
             (5, 4), (5, 8), (5, 11), (5, 13))
PS_GROUPS = 16          # groups of 32 lanes per workgroup: one row each at a time
PS_MAXG = 512           # workgroups at most
PS_ROWS_MAX = 1024      # rows per workgroup at most (CG, Chebyshev-CG, BiCGStab)
PG_ROWS = 224           # rows per workgroup at most (GMRES: the basis in LDS)
PG_M = 30               # GMRES restart at most
MAXLEN = 160            # longest row at most


def lds_layers(E, R):
    """layers of K that GMRES and BiCGStab keep in LDS (ps_el)"""
    return 1 if E == 5 and R >= 11 else 0


def previous_rows(E, R):
    """R of the shape before (E, R) in its class, 0 for the first"""
    rs = [r for e, r in PS_SHAPES if e == E]
    at = rs.index(R)
    return rs[at - 1] if at else 0


def expected_shape(n, maxlen, num_cu, rows_max, cap=None):
    """``ps_shape`` restated: (E, R, G) or None when the persistent loop does not take the system"""
    if maxlen < 1 or maxlen > MAXLEN:
        return None
    epr = (maxlen + 31) // 32
    G = min(num_cu, PS_MAXG)
    G = min(G, max(1, -(-n // PS_GROUPS)))
    if cap is not None and cap >= 1:
        G = min(G, cap)
    per = -(-n // G)
    if per > rows_max:
        return None
    for e, r in PS_SHAPES:
        if e == epr and per <= r * PS_GROUPS:
            return (e, r, G)
    return None


def family_size(R, G, top, per=None):
    """rows of the member: ceil(n / G) == per, the last workgroup holds a short block, n even (the offset n / 2 exists)"""
    if per is None:
        per = 16 * R if top else 16 * R - 1
    n = per * G - (G - 1)
    return n + (n & 1)


def shape_system(E, R, G, top, symmetric, seed, per=None, n=None):
    """Sorted CSR matrix that ``ps_shape`` maps to (E, R) under the cap G (``n`` overrides the size of the family: the caller
    answers for the shape then; an odd n has no offset n / 2, so ``top`` needs an even one).  The pattern depends on
    (E, R, G, top, seed, per, n) only: the symmetric and the non-symmetric member share it."""
    if n is None:
        n = family_size(R, G, top, per)
    assert not (top and n & 1), "the self-mirrored offset n / 2 needs an even n"
    rng = np.random.default_rng(seed)
    h = 16 * E - 1 if top else 16 * (E - 1)
    offs = rng.choice(np.arange(1, (n + 1) // 2), size=h, replace=False)
    I = np.tile(np.arange(n), h)
    J = (I + np.repeat(offs, n)) % n
    if top:
        I = np.concatenate([I, np.arange(n // 2)])
        J = np.concatenate([J, np.arange(n // 2) + n // 2])
    keep = (rng.random(I.size) < 0.6) | (I < 3) | (J < 3)
    I, J = I[keep], J[keep]
    v = rng.standard_normal(I.size)
    vt = v if symmetric else rng.standard_normal(I.size)
    off = sp.coo_matrix((np.concatenate([v, vt]), (np.concatenate([I, J]), np.concatenate([J, I]))), shape=(n, n)).tocsr()
    rowsum = np.asarray(abs(off).sum(axis=1)).ravel()
    u = rng.random(n)
    diag = (1.2 + u) * rowsum + 1.0
    # (a row without neighbours -- every row of the diagonal member E = 1, not top -- gets 1 + U instead of 1: the member is not
    #  the identity, so rows that are mixed up show there as well)
    diag[rowsum == 0.0] += u[rowsum == 0.0]
    A = (off + sp.diags(diag)).tocsr()
    A.sort_indices()
    return A


def longest_row(A):
    return int(np.diff(A.indptr).max())


def with_dead_diagonals(A):
    """The diagonal of rows 0, 5, n / 2 and n - 1 set to zero: rows 0 and n / 2 keep it as a stored 0.0, rows 5 and n - 1
    lose it from the pattern (PCJACOBI uses 1 for both)."""
    n = A.shape[0]
    data = A.data.copy()
    drop = np.zeros(A.nnz, dtype=bool)
    for i in (0, 5, n // 2, n - 1):
        a, e = A.indptr[i], A.indptr[i + 1]
        at = a + np.flatnonzero(A.indices[a:e] == i)
        assert at.size == 1
        if i in (0, n // 2):
            data[at] = 0.0
        else:
            drop[at] = True
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    B = sp.csr_matrix((data[~drop], (rows[~drop], A.indices[~drop])), shape=A.shape)     # (stored zeros stay stored)
    B.sort_indices()
    for i in (0, n // 2):
        a, e = B.indptr[i], B.indptr[i + 1]
        assert i in B.indices[a:e] and B[i, i] == 0.0
    for i in (5, n - 1):
        assert i not in B.indices[B.indptr[i]:B.indptr[i + 1]]
    return B


def without_entry(A, row, which):
    """A with the ``which``-th off-diagonal entry of ``row`` removed from the pattern"""
    a, e = A.indptr[row], A.indptr[row + 1]
    offd = [q for q in range(a, e) if A.indices[q] != row]
    q = offd[which]
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = np.ones(A.nnz, dtype=bool)
    keep[q] = False
    B = sp.csr_matrix((A.data[keep], (rows[keep], A.indices[keep])), shape=A.shape)
    B.sort_indices()
    return B


def direct_solve(A, b):
    """scipy's sparse LU in double (the pattern of the family is symmetric: minimum degree on A^T + A fills half as much as
    the default column ordering on random columns)"""
    return sla.spsolve(sp.csc_matrix(A), b, permc_spec="MMD_AT_PLUS_A")


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(E, R, G, top, symmetric, seed, per=None, n=None, dead=False):
    """(A, b, exact) of one member, computed once and shared (read-only): b standard normal, exact = spsolve(A, b) in double"""
    A = shape_system(E, R, G, top, symmetric, seed, per=per, n=n)
    if dead:
        A = with_dead_diagonals(A)
    b = np.random.default_rng(seed + 7919).standard_normal(A.shape[0])
    exact = direct_solve(A, b)
    for a in (A.data, A.indices, A.indptr):
        a.setflags(write=False)
    return A, _frozen(b), _frozen(exact)


def jacobi_dinv(A, jacobi=True):
    """PCJACOBI: the inverse diagonal, 1 where the diagonal is zero or absent (and everywhere without Jacobi)"""
    dinv = np.ones(A.shape[0])
    if jacobi:
        d = A.diagonal()
        nz = d != 0.0
        dinv[nz] = 1.0 / d[nz]
    return dinv


def true_residual(A, b, x, dinv):
    """||D^-1 (b - A x)|| and ||D^-1 b||, formed in np.longdouble from the CSR arrays"""
    L = np.longdouble
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    Ax = np.zeros(A.shape[0], dtype=L)
    np.add.at(Ax, rows, A.data.astype(L) * x.astype(L)[A.indices])
    r = dinv.astype(L) * (b.astype(L) - Ax)
    return float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum((dinv.astype(L) * b.astype(L)) ** 2)))
