"""The default solver's decision table (tigar_amd/direct_plan.py) against the sequences recorded from the solver it
replaces, and ``_DefaultSolver.solve`` as a loop over that table, with the device layer stubbed: no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph

from tigar_amd import direct_plan as P

# n, nnz, kl, ku, r (half-bandwidth after the "ordering"), environment, communicator set,
# what ran at the parent commit, the plan
ROWS = [
    (67600, 5.5e6, 1044, 1044, 10, {}, False, "lu(auto)", ("lu",)),
    (5000, 1e5, 40, 17, 10, {}, False, "lu(auto)", ("lu",)),
    (125000, 1.6e7, 5102, 5102, 10, {}, False, "cholesky, rcm, lu(reorder)", ("cholesky", "rcm", "krylov")),
    (125000, 1.6e7, 5102, 5102, 2990, {}, False, "cholesky, rcm, krylov", ("cholesky", "rcm", "krylov")),
    (125000, 1.6e7, 5102, 5000, 2990, {}, False, "rcm, krylov", ("rcm", "krylov")),
    (125000, 1.6e7, 5102, 5102, 2990, {"TIGAR_LU_CHOLESKY": "0"}, False, "rcm, krylov", ("rcm", "krylov")),
    (44652, 3e6, 29768, 29768, 10, {}, False, "rcm, lu(reorder)", ("rcm", "krylov")),
    (180000, 5e6, 46500, 46500, 2990, {}, False, "rcm, krylov", ("rcm", "krylov")),
    (60000, 5e6, 15500, 15500, 10, {}, False, "rcm, lu(reorder)", ("rcm", "cholesky", "krylov")),
    (60000, 5e6, 15500, 15500, 5990, {}, False, "rcm, cholesky, krylov", ("rcm", "cholesky", "krylov")),
    (60000, 5e6, 15500, 15500, 5990, {"TIGAR_LU_CHOLESKY": "0"}, False, "rcm, krylov", ("rcm", "krylov")),
    (60000, 5e6, 15500, 15500, 5990, {"TIGAR_DEFAULT_SOLVER": "lu"}, False, "rcm, lu(auto)", ("rcm", "lu")),
    (500000, 6e7, 6000, 6000, 10, {}, False, "cholesky, krylov", ("cholesky", "krylov")),
    (500000, 6e7, 6000, 6000, 10, {"TIGAR_DEFAULT_SOLVER": "lu"}, False, "cholesky, lu(auto)", ("cholesky", "lu")),
    (500000, 6e7, 6000, 5000, 10, {"TIGAR_DEFAULT_SOLVER": "lu"}, False, "lu(auto)", ("lu",)),
    (300000, 3e8, 9000, 9000, 10, {}, False, "cholesky, krylov", ("cholesky", "krylov")),
    (400001, 4e6, 10, 10, 10, {}, False, "cholesky, krylov", ("cholesky", "krylov")),     # (not offered to the LU)
    (67600, 5.5e6, 1044, 1044, 10, {"TIGAR_DEFAULT_SOLVER": "krylov"}, False, "krylov", ("krylov",)),
    (67600, 5.5e6, 1044, 1044, 10, {}, True, "krylov", ("krylov",)),
]
# the Cholesky factorisation accepts the system: nothing after it runs
ROWS_CHOLESKY_SOLVES = [
    (125000, 1.6e7, 5102, 5102, 10, {}, False, "cholesky", None),
    (60000, 5e6, 15500, 15500, 5990, {}, False, "rcm, cholesky", None),
]


def _walk(plan, n, r):
    """what runs of a plan when Cholesky declines and the ordering gives half-bandwidths r"""
    ran = []
    for attempt in plan:
        if attempt == "rcm":
            ran.append("rcm")
            if not P.lu_fits(n, r, r):
                continue
            attempt = "lu(reorder)"
        ran.append("lu(auto)" if attempt == "lu" else attempt)
        if attempt != "cholesky":
            break
    return ", ".join(ran)


def test_plan_reproduces_the_recorded_sequences():
    for (n, nnz, kl, ku, r, env, comm, ran, plan) in ROWS:
        got = P.default_plan(n, nnz, kl, ku, comm, env.get("TIGAR_DEFAULT_SOLVER"), env.get("TIGAR_LU_CHOLESKY"))
        assert got == plan, (n, kl, ku, env, got)
        assert _walk(got, n, r) == ran, (n, kl, ku, r, env)
    # the formulas the limits are stated in
    assert P.lu_band_bytes(67600, 1044, 1044) == 8 * 67600 * (3 * 1044 + 1)
    assert P.lu_madds(5000, 40, 17) == 2.0 * 5000 * 40 * 57
    assert P.lu_fits(400000, 10, 10) and not P.lu_fits(400001, 10, 10)
    assert P.LU_MAX_BAND_BYTES == 8 * 2 ** 30 and P.LU_SOLVER_MAX_BAND_BYTES == 16 * 2 ** 30


class _FakeK(object):
    def __init__(self, n, nnz, r):
        self.shape, self.nnz, self.r, self.downloads = (n, n), int(nnz), r, 0

    def to_scipy(self):
        self.downloads += 1
        m = max(3000, self.r + 1)
        S = sp.identity(m, format="lil")
        S[self.r, 0] = S[0, self.r] = 1.0
        return S.tocsr()


def trace_default_solver(monkeypatch, row, cholesky_solves=False):
    """(what ran, the fake matrix, the orderings the LU solver was handed) of one ``_DefaultSolver.solve``"""
    from tigar_amd import common as tc
    n, nnz, kl, ku, r, env, comm = row[:7]
    log, handed = [], []
    for name in ("TIGAR_DEFAULT_SOLVER", "TIGAR_LU_CHOLESKY"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    monkeypatch.setattr(tc, "_as_device_csr", lambda A: A)
    monkeypatch.setattr(tc, "_as_device_vector", lambda v: v)
    monkeypatch.setattr(tc._dev, "lu_band_info", lambda A: (kl, ku, 8 * n * (2 * kl + ku + 1)))

    def chol_solve(A, b, x):
        log.append("cholesky")
        return cholesky_solves

    def lu_solve(self, A, x, b, _ordering=None):
        log.append("lu(reorder)" if self.parameters["reorder"] is True else "lu(auto)")
        handed.append(_ordering)
        self.last = {"info": 0, "kl": 1, "ku": 1, "band_bytes": 24 * n, "reordered": False, "factorisation": "lu"}
        return 1

    def krylov_solve(self, A, x, b):
        log.append("krylov")
        self.last = {"iterations": 3, "status": 0}
        return 3

    def rcm(pattern, symmetric_mode=False):
        log.append("rcm")
        return np.arange(pattern.shape[0])

    monkeypatch.setattr(tc._dev, "chol_solve", chol_solve)
    monkeypatch.setattr(tc.PETScLUSolver, "solve", lu_solve)
    monkeypatch.setattr(tc.PETScKrylovSolver, "solve", krylov_solve)
    monkeypatch.setattr(scipy.sparse.csgraph, "reverse_cuthill_mckee", rcm)
    K = _FakeK(n, nnz, r)
    d = tc._default_linear_solver()
    d.comm = object() if comm else None
    ret = d.solve(K, object(), object())
    return ", ".join(log), K, handed, d, ret


def test_default_solver_walks_its_plan():
    for cholesky_solves, rows in ((False, ROWS), (True, ROWS_CHOLESKY_SOLVES)):
        for row in rows:
            with pytest.MonkeyPatch.context() as mp:
                ran, K, handed, d, ret = trace_default_solver(mp, row, cholesky_solves)
            n, kl, ku = row[0], row[2], row[3]
            assert ran == row[7], (row[:7], ran)
            # one download and one ordering at most, and the LU solver gets them
            assert K.downloads == ran.count("rcm") <= 1
            if "rcm" in ran and "lu" in ran:
                assert handed[0] is not None and handed[0][2] == (row[4], row[4])
            if ran.endswith("krylov"):
                assert d.last == {"iterations": 3, "status": 0, "solver": "gmres"} and ret == 3
            elif ran.endswith("cholesky"):
                assert d.last == {"solver": "lu", "factorisation": "cholesky", "info": 0, "kl": kl, "ku": ku,
                                  "band_bytes": 8 * n * (kl + 1), "reordered": False} and ret == 1
            else:
                assert d.last == {"info": 0, "kl": 1, "ku": 1, "band_bytes": 24 * n, "reordered": False,
                                  "factorisation": "lu", "solver": "lu"} and ret == 1
