"""What runs for ``linearSolver=None``: the limits of the banded direct solvers and the order in which the default
solver tries them.  Pure Python (no device layer): ``default_plan`` can be read and tested without a GPU."""

GIB = 2 ** 30

# ---- the banded LU (csrc/tg_lu.hip) as the default solver's first choice
LU_MAX_BAND_BYTES = 8 * GIB          # band storage (dgbtrf's layout) the default solver accepts for an LU
LU_MAX_MADDS = 4e12                  # multiply-adds of the factorisation it accepts
LU_MAX_ROWS = 400000                 # rows: above, neither the LU nor a host ordering is offered
RCM_MAX_NNZ = 2e8                    # stored entries up to which K is downloaded and ordered on the host
# ---- the banded Cholesky factorisation (csrc/tg_chol.hip) beyond those limits
CHOL_MAX_BAND_BYTES = 96 * GIB       # its band storage (the lower half only)
CHOL_MAX_MADDS = 4e13                # n kl^2
CHOL_MAX_KL = 16000                  # half-bandwidth
CHOL_FIRST_BAND_FRACTION = 4         # 4 kl < n: banded as numbered (one field), Cholesky goes before any ordering
# ---- PETScLUSolver on its own
LU_SOLVER_MAX_BAND_BYTES = 16 * GIB  # default of parameters["max_band_bytes"]
AUTO_REORDER_MIN_BAND_BYTES = 2 ** 28    # reorder="auto" orders only bands above this size ...
AUTO_REORDER_BAND_FRACTION = 8           # ... that are wider than n / 8 (kl + ku)


def lu_band_bytes(n, kl, ku):
    """bytes of the LU's band storage: 2 kl + ku + 1 rows of n doubles (kl of them for the fill of the interchanges)"""
    return 8 * n * (2 * kl + ku + 1)


def lu_madds(n, kl, ku):
    """multiply-adds of the banded LU with partial pivoting"""
    return 2.0 * n * kl * (kl + ku)


def chol_band_bytes(n, kl):
    return 8 * n * (kl + 1)


def lu_fits(n, kl, ku):
    """within the default solver's budget for an LU in this numbering"""
    return lu_band_bytes(n, kl, ku) <= LU_MAX_BAND_BYTES and lu_madds(n, kl, ku) <= LU_MAX_MADDS and n <= LU_MAX_ROWS


def auto_reorders(n, kl, ku):
    """PETScLUSolver's reorder="auto": is an ordering worth its download"""
    return lu_band_bytes(n, kl, ku) > AUTO_REORDER_MIN_BAND_BYTES and (kl + ku) > n // AUTO_REORDER_BAND_FRACTION


def default_plan(n, nnz, kl, ku, comm_set=False, default_solver=None, lu_cholesky=None):
    """The attempts of the default solver in order, from "cholesky", "rcm", "lu", "krylov"; each runs only if those
    before it declined.  ``default_solver`` / ``lu_cholesky``: the values of TIGAR_DEFAULT_SOLVER / TIGAR_LU_CHOLESKY
    (None: unset).  "cholesky" declines what is not symmetric positive definite; "rcm" orders the pattern and solves by LU
    if the reordered band is within the LU's budget; "lu" (as numbered, PETScLUSolver's own reorder="auto") and "krylov"
    never decline."""
    if comm_set or default_solver == "krylov":
        return ("krylov",)
    if lu_fits(n, kl, ku):
        return ("lu",)
    chol = kl == ku and chol_band_bytes(n, kl) <= CHOL_MAX_BAND_BYTES and float(n) * kl * kl <= CHOL_MAX_MADDS \
        and kl <= CHOL_MAX_KL and lu_cholesky != "0"
    # a band as numbered (kl well below n: one field) goes to Cholesky at once; a field-major system of several fields
    # (kl ~ n (nF-1)/nF) has its reordered band evaluated first (a download of K and a host ordering: 0.2-0.45 s for
    # 15-34 M entries, which the single-field solves paid for nothing)
    chol_first = chol and CHOL_FIRST_BAND_FRACTION * kl < n
    plan = []
    if chol_first:
        plan.append("cholesky")
    if n <= LU_MAX_ROWS and nnz <= RCM_MAX_NNZ:
        plan.append("rcm")
    if default_solver == "lu":
        return tuple(plan) + ("lu",)
    if chol and not chol_first:
        plan.append("cholesky")
    return tuple(plan) + ("krylov",)
