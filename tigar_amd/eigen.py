"""
Block LOBPCG for the smallest eigenpairs of a symmetric-definite pencil A x = lambda B x (Knyazev 2001), with the basis
selection of Hetmaniuk & Lehoucq (2006): the search directions W are B-orthogonalized against X and P and orthonormalized
on their own, and P is built from the W and P parts of the Ritz vectors, made B-orthogonal to the new X in coefficient
space.  Converged vectors are locked softly (they stay in X for the Rayleigh-Ritz step; their W and P columns are dropped).

Every vector of length n stays on the device inside the loop (csrc/tg_eig.hip: SpMM, Gram, combine, residual); the host
sees the Gram matrices and solves the <= 3m x 3m projected pencil with ``scipy.linalg.eigh``.

Rows whose only non-zero is the diagonal, in A and in B (the zero dofs of ``extractMatrix`` / ``assembleMatrix``: row and
column zeroed, ``diag`` on the diagonal), are found once per solve.  The block starts at zero on them and both A x and the
preconditioners keep it zero there, so the iteration runs in the free subspace; their eigenpairs are exact
(lambda = A_ii / B_ii, x = e_i / sqrt(B_ii)) and are merged into the sorted result, as SLEPc reports them for the same
pencil.  This also keeps a penalty diagonal (1 / DOLFIN_EPS) out of the Gram matrices.

``SLEPcEigenSolver`` is the look-alike of dolfin's class (demos/euler-bernoulli-beam/modal-analysis.py).
"""
import time

import numpy as np
import scipy.linalg

from . import device as _dev
from .device import DeviceBlock, DeviceCSR, DeviceVector

MAX_PAIRS = 48           # most pairs one solve computes (the block of 3m directions must fit the 64-wide kernels)
DEFAULT_PAIRS = 6        # solve() without a count (the modal-analysis demo reads five)
SYMMETRY_TOL = 1e-10     # max |A - A^T| relative to the largest off-diagonal |A_ij|
SVQB_TOL = 1e-12         # directions whose B-norm falls below this (relative) after scaling are dropped
# A pair also counts as converged when |A x - lambda B x| <= ROUNDING_FLOOR eps |A| |x| (|A| = the largest row sum of |a_ij|
# over the free rows): the rounding of the product A x alone leaves a residual of that size, so a tolerance below it cannot
# be met in double precision by any method (the first cantilever mode of the modal-analysis demo: lambda_max / lambda_1 ~
# 6e9, the exact dense eigenvector's relative residual is 1.4e-7).
ROUNDING_FLOOR = 4.0


# ------------------------------------------------------------------------------------------------- host pieces
def svqb(G, tol=SVQB_TOL):
    """T with T^T G T = I for a symmetric positive semi-definite Gram matrix G (Stathopoulos & Wu 2002): columns scaled to
    unit norm first, directions with eigenvalues below ``tol`` times the largest dropped.  Returns a k x k' matrix, k' <= k
    (k' = 0 when nothing is left)."""
    G = 0.5 * (G + G.T)
    k = G.shape[0]
    if k == 0:
        return np.zeros((0, 0))
    d = np.diag(G).copy()
    if not np.all(np.isfinite(G)):
        return np.zeros((k, 0))
    good = d > 0
    dinv = np.zeros(k)
    dinv[good] = 1.0 / np.sqrt(d[good])
    Gs = dinv[:, None] * G * dinv[None, :]
    s, V = np.linalg.eigh(Gs)
    smax = s[-1] if s.size else 0.0
    keep = s > tol * max(smax, 0.0)
    if smax <= 0.0 or not keep.any():
        return np.zeros((k, 0))
    return dinv[:, None] * (V[:, keep] / np.sqrt(s[keep])[None, :])


def cholesky_qr_factor(G):
    """upper triangular R with G = R^T R, or None when G is not (numerically) positive definite"""
    G = 0.5 * (G + G.T)
    if not np.all(np.isfinite(G)):
        return None
    try:
        return scipy.linalg.cholesky(G, lower=False)
    except np.linalg.LinAlgError:
        return None


def rayleigh_ritz(GA, GB, m):
    """the m smallest eigenpairs of the projected pencil GA c = theta GB c: (theta, C) with C^T GB C = I.  Raises
    ``numpy.linalg.LinAlgError`` when GB is not positive definite."""
    GA = 0.5 * (GA + GA.T)
    GB = 0.5 * (GB + GB.T)
    m = min(m, GA.shape[0])
    theta, C = scipy.linalg.eigh(GA, GB, subset_by_index=[0, m - 1])
    return theta, C


def p_coefficients(C, GB, m, active):
    """Hetmaniuk & Lehoucq's P: coefficients (rows: the basis [X, W, P]) of the W and P parts of the active Ritz vectors,
    B-orthogonalized against all Ritz vectors C and orthonormalized (in the metric GB).  Returns a matrix of at most
    len(active) columns (none when the directions are dependent)."""
    Z = C[:, active].copy()
    Z[:m, :] = 0.0
    Z = Z - C @ (C.T @ (GB @ Z))
    T = svqb(Z.T @ GB @ Z)
    return Z @ T


def rr_step(GA, GB, m, nx, nw, active):
    """One Rayleigh-Ritz step on the basis [X (nx), W (nw), P (rest)]: (theta, C, Z, restarted).  When GB is not positive
    definite with P the step is redone without P (restarted = True; C and Z then have nx + nw rows).  Z = the coefficients
    of the next P (``p_coefficients``)."""
    restarted = False
    try:
        theta, C = rayleigh_ritz(GA, GB, m)
    except np.linalg.LinAlgError:
        if GA.shape[0] == nx + nw:
            raise
        k = nx + nw
        GA, GB = GA[:k, :k], GB[:k, :k]
        theta, C = rayleigh_ritz(GA, GB, m)
        restarted = True
    Z = p_coefficients(C, GB, nx, active)
    return theta, C, Z, restarted


def merge_decoupled(lam_free, lam_dec, count):
    """the ``count`` smallest of the free Ritz values and the exact eigenvalues of the decoupled rows, ascending:
    list of (lambda, source, index) with source "free" (column of X) or "decoupled" (index into lam_dec).  Ties keep the
    free pairs first."""
    lam_free = np.asarray(lam_free, dtype=np.float64)
    lam_dec = np.asarray(lam_dec, dtype=np.float64)
    allv = np.concatenate([lam_free, lam_dec])
    order = np.argsort(allv, kind="stable")[:count]
    nf = lam_free.size
    return [(float(allv[o]), "free", int(o)) if o < nf else (float(allv[o]), "decoupled", int(o - nf)) for o in order]


def default_block_size(nev, nfree):
    """nev + max(2, nev // 2) guard vectors, at most 64 and at most (nfree - 1) // 3 (so that 3m < free rows), never below
    nev"""
    m = min(_dev.BLOCK_MAX, nev + max(2, nev // 2))
    return max(nev, min(m, (nfree - 1) // 3))


# ------------------------------------------------------------------------------------------------- device solve
class _Timer(object):
    def __init__(self):
        self.t = {"spmm": 0.0, "gram": 0.0, "combine": 0.0, "residual": 0.0, "preconditioner": 0.0, "rayleigh_ritz": 0.0}

    def run(self, key, fn, *args, sync=True):
        t0 = time.perf_counter()
        out = fn(*args)
        if sync:
            _dev.sync()
        self.t[key] += time.perf_counter() - t0
        return out


def _combine(tm, terms, n, k):
    Y = DeviceBlock(n, k, zero=False)
    tm.run("combine", _dev.block_combine, terms, Y)
    return Y


def _gram_blocks(tm, left, right):
    """[[left_a^T right_b]] for lists of DeviceBlocks, upper triangle computed, lower mirrored (symmetric pencils)"""
    sizes = [b.k for b in left]
    off = np.concatenate([[0], np.cumsum(sizes)])
    G = np.zeros((off[-1], off[-1]))
    for a in range(len(left)):
        for b in range(a, len(left)):
            g = tm.run("gram", _dev.block_gram, left[a], right[b], sync=False)
            G[off[a]:off[a + 1], off[b]:off[b + 1]] = g
            if b != a:
                G[off[b]:off[b + 1], off[a]:off[a + 1]] = g.T
    return G


def lobpcg(A, B, nev, m, tol, maxit, precond, mask, dinv, X0, fd=None, timer=None, anorm=0.0):
    """Block LOBPCG on the device.  A, B: DeviceCSR; X0: DeviceBlock (n x m, zero on the masked rows); precond "none",
    "jacobi" (dinv = D^-1 as a DeviceVector) or "fast_diagonalization" (``fd``); anorm: the largest row sum of |A| on the
    free rows (the rounding floor, ROUNDING_FLOOR).  Returns a dict with X, lam, residuals (relative: |r| / (|lambda|
    |B x|)), floors (the rounding floor in the same measure), iterations, converged (of the first nev), restarts."""
    tm = timer or _Timer()
    n = X0.n
    Im = np.eye(m)
    # B-orthonormal start: Cholesky QR of X0^T B X0
    BX = tm.run("spmm", B.mult_block, X0)
    Rf = cholesky_qr_factor(tm.run("gram", _dev.block_gram, X0, BX, sync=False))
    if Rf is None:
        raise RuntimeError("SLEPcEigenSolver: B is not positive definite on the free rows (the Cholesky factorization of "
                           "X^T B X of the start block failed)")
    Ri = scipy.linalg.solve_triangular(Rf, Im, lower=False)
    X = _combine(tm, [(X0, Ri)], n, m)
    BX = _combine(tm, [(BX, Ri)], n, m)
    AX = tm.run("spmm", A.mult_block, X)
    GA = _gram_blocks(tm, [X], [AX])
    GB = _gram_blocks(tm, [X], [BX])
    t0 = time.perf_counter()
    lam, C = rayleigh_ritz(GA, GB, m)
    tm.t["rayleigh_ritz"] += time.perf_counter() - t0
    X, AX, BX = (_combine(tm, [(Y, C)], n, m) for Y in (X, AX, BX))
    P = AP = BP = None
    R = DeviceBlock(n, m, zero=False)
    Wfull = DeviceBlock(n, m, zero=False) if precond == "jacobi" else None
    rv = zv = None
    if precond == "fast_diagonalization":
        rv, zv = DeviceVector(n, zero=False), DeviceVector(n, zero=False)
    res = np.full(m, np.inf)
    restarts = 0
    it = 0
    stalled = False
    fresh = False           # AX and BX were just recomputed from X (not carried through the combines)
    while True:
        rn2, bn2 = tm.run("residual", _dev.block_residual, AX, BX, lam, R, Wfull, mask, dinv, sync=False)
        xn = np.sqrt(np.maximum(np.diag(tm.run("gram", _dev.block_gram, X, X, sync=False)), 0.0))
        denom = np.abs(lam) * np.sqrt(np.maximum(bn2, 0.0))
        rn = np.sqrt(np.maximum(rn2, 0.0))
        ok = denom > 0
        res = np.where(ok, rn / np.where(ok, denom, 1.0), np.inf)
        res[rn == 0.0] = 0.0
        floor = np.where(ok, ROUNDING_FLOOR * np.finfo(np.float64).eps * anorm * xn / np.where(ok, denom, 1.0), 0.0)
        conv = res <= np.maximum(tol, floor)
        if conv[:nev].all() and not fresh:
            # confirm on products taken afresh: the AX, BX the combines carry drift by rounding from A X, B X
            AX = tm.run("spmm", A.mult_block, X)
            BX = tm.run("spmm", B.mult_block, X)
            fresh = True
            continue
        if conv[:nev].all() or it >= maxit or stalled:
            break
        it += 1
        fresh = False
        active = [j for j in range(m) if not conv[j]]
        na = len(active)
        Sel = Im[:, active]
        if precond == "fast_diagonalization":
            t0 = time.perf_counter()
            Wa = DeviceBlock(n, na, zero=False)
            for jj, j in enumerate(active):
                R.get_column(j, rv)
                fd.apply(rv, zv)
                Wa.set_column(jj, zv)
            _dev.sync()
            tm.t["preconditioner"] += time.perf_counter() - t0
        else:
            Wa = _combine(tm, [(Wfull if precond == "jacobi" else R, Sel)], n, na)
        BWa = tm.run("spmm", B.mult_block, Wa)
        # B-orthogonal to X and P, then orthonormal on its own (SVQB: dependent directions dropped)
        c1 = tm.run("gram", _dev.block_gram, X, BWa, sync=False)
        terms, bterms = [(Wa, np.eye(na)), (X, -c1)], [(BWa, np.eye(na)), (BX, -c1)]
        if P is not None:
            c2 = tm.run("gram", _dev.block_gram, P, BWa, sync=False)
            terms.append((P, -c2))
            bterms.append((BP, -c2))
        W1, BW1 = _combine(tm, terms, n, na), _combine(tm, bterms, n, na)
        T = svqb(tm.run("gram", _dev.block_gram, W1, BW1, sync=False))
        nw = T.shape[1]
        if nw == 0:
            stalled = True          # (every residual direction lies in span [X, P]: nothing left to add)
            continue
        W, BW = _combine(tm, [(W1, T)], n, nw), _combine(tm, [(BW1, T)], n, nw)
        AW = tm.run("spmm", A.mult_block, W)
        basis, abasis, bbasis = [X, W], [AX, AW], [BX, BW]
        if P is not None:
            basis, abasis, bbasis = basis + [P], abasis + [AP], bbasis + [BP]
        GA = _gram_blocks(tm, basis, abasis)
        GB = _gram_blocks(tm, basis, bbasis)
        t0 = time.perf_counter()
        try:
            lam, C, Z, restarted = rr_step(GA, GB, m, m, nw, active)
        except np.linalg.LinAlgError:
            tm.t["rayleigh_ritz"] += time.perf_counter() - t0
            stalled = True
            continue
        tm.t["rayleigh_ritz"] += time.perf_counter() - t0
        if restarted:
            restarts += 1
            basis, abasis, bbasis = basis[:2], abasis[:2], bbasis[:2]
        off = np.concatenate([[0], np.cumsum([b.k for b in basis])])

        def parts(Cm, blocks):
            return [(blk, Cm[off[i]:off[i + 1], :]) for i, blk in enumerate(blocks)]
        X, AX, BX = (_combine(tm, parts(C, bl), n, m) for bl in (basis, abasis, bbasis))
        if Z.shape[1]:
            P, AP, BP = (_combine(tm, parts(Z, bl), n, Z.shape[1]) for bl in (basis, abasis, bbasis))
        else:
            P = AP = BP = None
    return {"X": X, "BX": BX, "lam": np.asarray(lam), "residuals": res, "floors": floor, "iterations": it,
            "converged": int(np.count_nonzero(conv[:nev])), "restarts": restarts, "timer": tm}


# ------------------------------------------------------------------------------------------------- public interface
class SLEPcEigenSolver(object):
    """Look-alike of dolfin's ``SLEPcEigenSolver(A, B)`` for the smallest eigenpairs of a symmetric-definite pencil
    A x = lambda B x (B = None: the standard problem), by block LOBPCG on the GPU (tigar_amd/eigen.py,
    csrc/tg_eig.hip).  ``A`` / ``B``: DeviceCSR (as ``assembleMatrix`` returns them) or scipy matrices.

    parameters: "spectrum" ("smallest magnitude" or "smallest real": both mean the smallest eigenvalues of the definite
    pencil), "tolerance" (1e-8: |A x - lambda B x| <= tol |lambda| |B x|, or the rounding floor of A x where that
    is larger, ROUNDING_FLOOR), "maximum_iterations" (1000),
    "error_on_nonconvergence" (True), and, not dolfin's, "preconditioner" ("jacobi" = diag A, default; "none";
    "fast_diagonalization" for an A that carries ``tensor_structure``), "block_size" (None = nev + max(2, nev // 2), at
    most 64 and below a third of the free rows) and "seed" (0: the start block; same inputs and seed, same bits).

    ``solve(n=None)`` computes the n smallest pairs (None: 6); ``get_eigenpair(i)`` returns (lambda, 0.0, x, 0-vector) with
    x a DeviceVector of IGA dofs, x^T B x = 1, its entry of largest magnitude positive.  ``last`` reports iterations,
    residuals, the preconditioner and the seconds spent per phase.  Refused: non-square or mismatched matrices, A or B not
    symmetric, B not positive definite on the free rows, more than 48 pairs or a block of 3m >= the free rows (ValueError
    / RuntimeError), several ranks or a row-block matrix (NotImplementedError)."""

    def __init__(self, A, B=None, comm=None):
        size = getattr(comm, "size", 1) if comm is not None else 1
        size = size() if callable(size) else size
        if comm is not None and hasattr(comm, "Get_size"):
            size = comm.Get_size()
        if size > 1:
            raise NotImplementedError("SLEPcEigenSolver: several ranks are not supported (the block kernels run on one "
                                      "GPU; solve on a single rank)")
        self.A = self._matrix(A, "A")
        self.B = self._matrix(B, "B") if B is not None else None
        if self.B is not None and self.B.shape != self.A.shape:
            raise ValueError("SLEPcEigenSolver: A is %d x %d, B is %d x %d" % (self.A.shape + self.B.shape))
        self.parameters = {"spectrum": "smallest magnitude", "tolerance": 1e-8, "maximum_iterations": 1000,
                           "error_on_nonconvergence": True, "preconditioner": "jacobi", "block_size": None, "seed": 0}
        self.last = None
        self._pairs = []
        self._n = self.A.shape[0]
        self._checked = False

    @staticmethod
    def _matrix(M, name):
        if isinstance(M, DeviceCSR):
            nr, nc = M.shape
            if nr < nc:
                raise NotImplementedError("SLEPcEigenSolver: %s is a row block (%d of %d rows: a z-slab of a matrix spread "
                                          "over several ranks); only single-rank matrices are supported" % (name, nr, nc))
            if nr != nc:
                raise ValueError("SLEPcEigenSolver: %s is not square (%d x %d)" % (name, nr, nc))
            if M.is_loose():
                M = M.compact()
            return M
        shape = getattr(M, "shape", None)
        if shape is None or len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("SLEPcEigenSolver: %s is not square (shape %s)" % (name, shape))
        return DeviceCSR.from_scipy(M)

    def _check_symmetric(self):
        for name, M in (("A", self.A), ("B", self.B)):
            if M is None or getattr(M, "symmetric_by_construction", False):
                continue
            had_t = M._T is not None
            defect, scale = _dev.csr_sym_defect(M)
            if not had_t:
                M._T = None             # (the transpose served the check only)
            if not defect <= SYMMETRY_TOL * scale:
                raise ValueError("SLEPcEigenSolver: %s is not symmetric (max |%s - %s^T| = %.3e against a largest "
                                 "off-diagonal entry of %.3e); only symmetric-definite pencils are supported"
                                 % (name, name, name, defect, scale))

    def solve(self, n=None):
        nev = DEFAULT_PAIRS if n is None else int(n)
        prm = self.parameters
        if prm["spectrum"] not in ("smallest magnitude", "smallest real"):
            raise ValueError("SLEPcEigenSolver: spectrum %r is not supported (\"smallest magnitude\" or \"smallest real\": "
                             "the smallest eigenvalues of the definite pencil)" % (prm["spectrum"],))
        precond = prm["preconditioner"]
        if precond not in ("jacobi", "none", "fast_diagonalization"):
            raise ValueError("SLEPcEigenSolver: unknown preconditioner %r (jacobi, none, fast_diagonalization)" % (precond,))
        if nev < 1 or nev > MAX_PAIRS:
            raise ValueError("SLEPcEigenSolver: %d pairs requested; at most %d pairs per solve (and there is no CPU "
                             "fallback)" % (nev, MAX_PAIRS))
        fd = None
        if precond == "fast_diagonalization":
            from .fastdiag import FastDiagonalization
            fd = FastDiagonalization(self.A)           # (ValueError with its reason when A has no tensor structure)
        if not self._checked:
            self._check_symmetric()
            self._checked = True
        A, nrow = self.A, self._n
        B = self.B
        if B is None:
            import scipy.sparse as sp
            B = DeviceCSR.from_scipy(sp.identity(nrow, format="csr"))
        t_all = time.perf_counter()
        mark, da, db, ndec, anorm = _dev.csr_decoupled_rows(A, self.B)
        mk = mark.get_local() != 0.0
        dA = da.get_local()
        dB = db.get_local() if db is not None else np.ones(nrow)
        nfree = nrow - int(ndec)
        dec = np.nonzero(mk)[0]
        if np.any(dB[dec] <= 0.0):
            raise RuntimeError("SLEPcEigenSolver: B is not positive definite (a decoupled row has B_ii <= 0)")
        m = prm["block_size"]
        m = default_block_size(nev, nfree) if m is None else int(m)
        if m < nev or m > _dev.BLOCK_MAX:
            raise ValueError("SLEPcEigenSolver: block size %d for %d pairs (must lie in [%d, %d])"
                             % (m, nev, nev, _dev.BLOCK_MAX))
        if 3 * m >= nfree:
            raise ValueError("SLEPcEigenSolver: %d pairs need a block of %d vectors, and 3 x %d >= %d free rows (the "
                             "limit: 3 x block size < free rows; there is no CPU fallback)" % (nev, m, m, nfree))
        # deterministic start block, zero on the decoupled rows
        rng = np.random.default_rng(int(prm["seed"]))
        X0h = rng.standard_normal((nrow, m))
        X0h[mk, :] = 0.0
        X0 = DeviceBlock(nrow, m, data=X0h)
        dinv = None
        if precond == "jacobi":
            dv = np.zeros(nrow)
            free = ~mk
            dv[free] = np.where(dA[free] != 0.0, 1.0 / np.where(dA[free] != 0.0, dA[free], 1.0), 1.0)
            dinv = DeviceVector(data=dv)
        out = lobpcg(A, B, nev, m, float(prm["tolerance"]), int(prm["maximum_iterations"]), precond, mark, dinv, X0, fd=fd,
                     anorm=anorm)
        tm = out["timer"]
        conv = out["converged"]
        if conv < nev and prm["error_on_nonconvergence"]:
            raise RuntimeError("SLEPcEigenSolver: %d of %d eigenpairs converged after %d iterations (tolerance %.1e, "
                               "largest relative residual %.3e)" % (conv, nev, out["iterations"], prm["tolerance"],
                                                                     float(np.max(out["residuals"][:nev]))))
        # B-normalized, sign-fixed eigenvectors (one download of the block, after the loop)
        X = out["X"]
        gd = np.diag(_dev.block_gram(X, out["BX"]))
        Xh = X.to_numpy()
        big = np.argmax(np.abs(Xh), axis=0)
        sgn = np.where(Xh[big, np.arange(m)] < 0.0, -1.0, 1.0)
        X = _combine(tm, [(X, np.diag(sgn / np.sqrt(gd)))], nrow, m)
        lam_dec = dA[dec] / dB[dec]
        self._pairs = merge_decoupled(out["lam"][:nev], lam_dec, nev)
        self._X, self._dec, self._dB = X, dec, dB[dec]
        res, flo = out["residuals"], out["floors"]
        self.last = {"iterations": out["iterations"], "block_size": m, "preconditioner": precond,
                     "residuals": [float(res[i]) if s == "free" else 0.0 for (_, s, i) in self._pairs],
                     "rounding_floors": [float(flo[i]) if s == "free" else 0.0 for (_, s, i) in self._pairs],
                     "converged": conv + sum(1 for (_, s, _i) in self._pairs if s == "decoupled"),
                     "decoupled_rows": int(ndec), "free_rows": nfree, "restarts": out["restarts"],
                     "seconds": dict(tm.t, total=time.perf_counter() - t_all)}
        self._nconv = min(nev, sum(1 for (_, s, i) in self._pairs
                                   if s == "decoupled" or res[i] <= max(prm["tolerance"], flo[i])))
        return self._nconv

    def get_number_converged(self):
        return self._nconv if self.last is not None else 0

    def get_eigenvalue(self, i):
        lam, _, _ = self._pairs[i]
        return (lam, 0.0)

    def get_eigenpair(self, i):
        lam, src, j = self._pairs[i]
        if src == "free":
            rx = self._X.get_column(j)
        else:
            e = np.zeros(self._n)
            e[self._dec[j]] = 1.0 / np.sqrt(self._dB[j])
            rx = DeviceVector(data=e)
        return (lam, 0.0, rx, DeviceVector(self._n))
