"""numpy / scipy reference of the FE-order kernels (tigar_amd/csrc/tg_feorder.hip), for the tests only: recognising node
coordinates as a permutation of a tensor node grid, the symmetric permutation of a CSR matrix and of a vector.  The product
has no CPU path; this file is what its kernels are compared with."""
import numpy as np
import scipy.sparse as sp


class Declined(ValueError):
    """the coordinates are not a permutation of the node grid; ``reason`` is one of "wrong row count", "off the grid",
    "node of another field", "two rows on one node"; ``row`` the first offending row (None for the row count)"""

    def __init__(self, reason, row=None):
        ValueError.__init__(self, "%s (row %s)" % (reason, row))
        self.reason, self.row = reason, row


def _nearest(axis, x):
    """index of the node of the ascending ``axis`` nearest to every x, and the distance"""
    axis = np.asarray(axis, dtype=np.float64)
    hi = np.clip(np.searchsorted(axis, x, side="left"), 0, len(axis) - 1)
    lo = np.clip(hi - 1, 0, len(axis) - 1)
    dh, dl = np.abs(axis[hi] - x), np.abs(axis[lo] - x)
    take_lo = dl < dh
    return np.where(take_lo, lo, hi), np.where(take_lo, dl, dh)


def _on_grid(axes, x, tol):
    """lexicographic index (direction 0 fastest) of every row of x on the grid of ``axes``, -1 where it is off the grid;
    and the largest distance over the directions"""
    lex = np.zeros(x.shape[0], dtype=np.int64)
    ok = np.ones(x.shape[0], dtype=bool)
    snap = np.zeros(x.shape[0])
    stride = 1
    for k, a in enumerate(axes):
        a = np.asarray(a, dtype=np.float64)
        h = np.min(np.diff(a)) if len(a) > 1 else 1.0
        idx, dist = _nearest(a, x[:, k])
        ok &= dist <= tol * h
        snap = np.maximum(snap, dist)
        lex += stride * idx
        stride *= len(a)
    return np.where(ok, lex, -1), snap


def locate(field_axes, x, fields=None, tol=1e-6):
    """(grid_of_fe, fe_of_grid, max_snap) of the rows with node coordinates ``x`` [nrows x d] on the space whose field f lives
    on the tensor grid ``field_axes[f]``; ``fields``: field of every row.  Raises ``Declined``."""
    nf, d = len(field_axes), len(field_axes[0])
    x = np.asarray(x, dtype=np.float64).reshape(-1, d)
    sizes = [int(np.prod([len(a) for a in fa])) for fa in field_axes]
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    if x.shape[0] != n:
        raise Declined("wrong row count")
    f = np.zeros(n, dtype=np.int64) if fields is None else np.asarray(fields, dtype=np.int64)
    g = np.full(n, -1, dtype=np.int64)
    snap = np.zeros(n)
    bad = []                                       # (row, reason)
    for q in range(nf):
        rows = np.nonzero(f == q)[0]
        lex, s = _on_grid(field_axes[q], x[rows], tol)
        g[rows] = np.where(lex >= 0, off[q] + lex, -1)
        snap[rows] = np.where(lex >= 0, s, 0.0)
        for r in rows[lex < 0]:
            other = any(p != q and _on_grid(field_axes[p], x[r:r + 1], tol)[0][0] >= 0 for p in range(nf))
            bad.append((int(r), "node of another field" if other else "off the grid"))
    fe_of_grid = np.full(n, n, dtype=np.int64)
    valid = np.nonzero(g >= 0)[0]
    np.minimum.at(fe_of_grid, g[valid], valid)     # the smallest row that names a node claims it
    for r in valid[fe_of_grid[g[valid]] != valid]:
        # a duplicate; when the same node of a field with the same grid has no row, the label is what is wrong
        q = int(np.searchsorted(off, g[r], side="right") - 1)
        lex = g[r] - off[q]
        relabel = any(p != q and all(np.array_equal(a, b) for a, b in zip(field_axes[p], field_axes[q])) and
                      len(field_axes[p]) == len(field_axes[q]) and fe_of_grid[off[p] + lex] == n for p in range(nf))
        bad.append((int(r), "node of another field" if relabel else "two rows on one node"))
    if bad:
        row, reason = min(bad)
        raise Declined(reason, row)
    return g.astype(np.int32), fe_of_grid.astype(np.int32), float(snap.max()) if n else 0.0


def permute_sym(A, grid_of_fe):
    """B[g(i), g(j)] = A[i, j] as canonical CSR, values untouched"""
    A = sp.csr_matrix(A)
    g = np.asarray(grid_of_fe, dtype=np.int64)
    inv = np.empty_like(g)
    inv[g] = np.arange(len(g))
    B = A[inv][:, inv].tocsr()
    B.sort_indices()
    return B


def vec_to_grid(x, grid_of_fe):
    y = np.empty_like(np.asarray(x, dtype=np.float64))
    y[np.asarray(grid_of_fe, dtype=np.int64)] = x
    return y


def vec_to_caller(x, grid_of_fe):
    return np.asarray(x, dtype=np.float64)[np.asarray(grid_of_fe, dtype=np.int64)]
