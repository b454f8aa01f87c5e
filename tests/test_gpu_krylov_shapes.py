"""-m gpu: every register shape of the persistent Krylov kernels (csrc/tg_krylov_small.hip: CG, GMRES(m), BiCGStab and
Chebyshev-CG, each compiled for the 20 (entries per lane and row, rows per group of lanes) shapes of PS_SHAPES) on the matrix
family of tests/krylov_shapes.py.  TIGAR_KSP_PERSISTENT_WGS caps the number of workgroups, so systems of 188 .. 2 686 rows
reach the shapes that 16 000 .. 230 000 rows take on the whole chip: the short last batch of the unrolled product, local rows
g + 16 ri up to ri = 55, the layer of K in LDS at ri > 0.  The family has rows of exactly 32 E and 32 (E - 1) + 1 entries, ragged
rows, and columns anywhere in the matrix (every product gathers from every workgroup).

Every solve is checked against scipy's sparse direct solve in double (max-norm error <= 1e-8 relative at rtol 1e-12 and a
condition number of order 10 -- rounding gives about 1e-11, measured 4e-12 at most; ONE lost entry of typical size moves the
exact solution by >= 1e-5, see tests/test_krylov_shapes_host.py), against the residual formed on the host in long double, against the iteration counts of the
oracle's textbook loops, for bit-reproducibility, and -- from the trace line and the profile counter -- for the shape that ran."""
import functools
import re

import numpy as np
import pytest

import krylov_shapes as S
from oracle import tigar_oracle as O

pytestmark = pytest.mark.gpu

SEED = 20                       # (tests/test_krylov_shapes_host.py checks the members of this seed)
TOL = 1e-8                      # max-norm error against spsolve, relative
RTOL, ATOL, MAXIT = 1e-12, 1e-300, 500
PERSISTENT_SLOT = 6             # profile counter of the persistent kernels
NAMES = {("cg", "jacobi"): "CG", ("cg", "none"): "CG", ("cg", "chebyshev"): "Chebyshev-CG", ("gmres", "jacobi"): "GMRES",
         ("bicgstab", "jacobi"): "BiCGStab"}
TRACE = re.compile(r"\[trace\] persistent (\S+): (\d+) its in \S+ ms \((\d+) workgroups, (\d+) entries per lane and row, "
                   r"(\d+) rows per group of\s+lanes, (\d+) layers of K in LDS\)")


def _dev():
    from tigar_amd import device
    return device


@functools.lru_cache(maxsize=None)
def _oracle_cg(key, jacobi, maxit=MAXIT):
    A, b, _ = S.reference(*key)
    x, its, _ = O.cg_jacobi(A, b, rtol=RTOL, atol=ATOL, maxit=maxit, jacobi=jacobi)
    x.setflags(write=False)
    return x, its


@functools.lru_cache(maxsize=None)
def _oracle_gmres(key, restart=30, maxit=MAXIT):
    A, b, _ = S.reference(*key)
    x, its, _ = O.gmres_jacobi(A, b, rtol=RTOL, atol=ATOL, maxit=maxit, restart=restart)
    x.setflags(write=False)
    return x, its


class _Result(object):
    pass


class _Bench(object):
    """One system on the device under one cap of the workgroup count; ``solve`` runs it and reads what ran from the trace line
    and the counter; failed checks are collected (``fail``) and raised together by ``done``: one run shows all of them."""

    def __init__(self, monkeypatch, capfd, A, b, exact, cap, shape):
        self.mp, self.capfd = monkeypatch, capfd
        self.A, self.b, self.exact, self.cap = A, b, exact, cap
        self.E, self.R = shape
        self.Ad = _dev().DeviceCSR.from_scipy(A)
        self.failures = []

    def fail(self, what, *figures):
        self.failures.append("%s %r" % (what, figures))

    def solve(self, method, pc, restart=30, persistent=True, guess=None, maxit=MAXIT, b=None):
        dev = _dev()
        self.mp.setenv("TIGAR_KSP_PERSISTENT", "1" if persistent else "0")
        if self.cap is None:
            self.mp.delenv("TIGAR_KSP_PERSISTENT_WGS", raising=False)
        else:
            self.mp.setenv("TIGAR_KSP_PERSISTENT_WGS", str(self.cap))
        self.mp.setenv("TIGAR_TRACE", "1")
        n = self.A.shape[0]
        x = dev.DeviceVector(n) if guess is None else dev.DeviceVector(data=np.array(guess))
        bd = dev.DeviceVector(data=np.array(self.b if b is None else b))
        self.capfd.readouterr()
        before = dev.prof_get(PERSISTENT_SLOT)[1]
        r = _Result()
        r.its, r.res, r.status = dev.krylov_solve(self.Ad, bd, x, method, pc, RTOL, ATOL, maxit, restart,
                                                  nonzero_initial_guess=guess is not None)
        r.ran = dev.prof_get(PERSISTENT_SLOT)[1] - before
        r.trace = [(m[0],) + tuple(int(q) for q in m[1:]) for m in TRACE.findall(self.capfd.readouterr().err)]
        r.x = x.get_local()
        r.method, r.pc, r.tag = method, pc, "%s/%s/%d" % (method, pc, restart)
        return r

    def took(self, r, G, layers=0):
        """the persistent kernel ran, on (G workgroups, E, R, layers)"""
        want = [(NAMES[(r.method, r.pc)], r.its, G, self.E, self.R, layers)]
        if r.ran != 1 or r.trace != want:
            self.fail(r.tag + ": persistent kernel / shape", r.ran, r.trace, want)

    def refused(self, r):
        """the multi-kernel loop ran instead: the counter stays, no trace line"""
        if r.ran != 0 or r.trace:
            self.fail(r.tag + ": expected the multi-kernel loop", r.ran, r.trace)

    def right(self, r, tol=TOL, residual=None):
        """status 0, the error against the direct solve, and (CG, GMRES) the reported norm against the true preconditioned
        residual of the returned iterate"""
        if r.status != 0:
            self.fail(r.tag + ": status", r.status, r.its)
        err = np.max(np.abs(r.x - self.exact)) / np.max(np.abs(self.exact))
        if not err <= tol:
            self.fail(r.tag + ": error against spsolve", err, tol)
        if residual is None:
            residual = r.method in ("cg", "gmres") and r.pc != "chebyshev"
        if residual:
            true, bnorm = S.true_residual(self.A, self.b, r.x, S.jacobi_dinv(self.A, r.pc == "jacobi"))
            if not abs(true - r.res) <= 1e-6 * max(true, r.res) + 1e-3 * RTOL * bnorm:
                self.fail(r.tag + ": reported norm against the true residual", true, r.res, bnorm)

    def same_again(self, r, **kw):
        r2 = self.solve(r.method, r.pc, **kw)
        if r2.its != r.its or not np.array_equal(r2.x.view(np.int64), r.x.view(np.int64)):
            self.fail(r.tag + ": second run differs", r.its, r2.its, float(np.max(np.abs(r2.x - r.x))))

    def count(self, r, its, slack=1):
        if not abs(r.its - its) <= slack:
            self.fail(r.tag + ": iterations", r.its, its, slack)

    def done(self):
        assert not self.failures, "\n".join(self.failures)


def _gmres_per(E, R, top):
    """rows per workgroup of the member GMRES runs on, and whether the kernel takes it: the family's own where the basis
    fits (<= 224 rows), 224 where that still selects the shape (more than 16 R_prev), else the family's own -- refused"""
    per = 16 * R if top else 16 * R - 1
    if per <= S.PG_ROWS:
        return None, True
    if S.PG_ROWS > 16 * S.previous_rows(E, R):
        return S.PG_ROWS, True
    return None, False


def _sweep_cases():
    return [pytest.param(E, R, top, id="%d-%d-%s" % (E, R, "top" if top else "low")) for E, R in S.PS_SHAPES
            for top in (True, False)]


@pytest.mark.parametrize("E,R,top", _sweep_cases())
def test_every_register_shape_of_the_four_persistent_solvers(E, R, top, monkeypatch, capfd):
    """(a) CG with Jacobi, CG without, Chebyshev-CG of degree 4 on the symmetric member; GMRES(30) and BiCGStab with Jacobi on
    the non-symmetric one; three workgroups.  GMRES holds its basis in LDS and takes at most 224 rows per workgroup: where the
    family's member has more, it is REFUSED there (the multi-kernel loop answers), and where 224 rows still select the shape --
    (1,16), (2,16), (3,17) -- GMRES runs on a member of 224 rows per workgroup as well."""
    G = 3
    skey, nkey = (E, R, G, top, True, SEED), (E, R, G, top, False, SEED)
    sym = _Bench(monkeypatch, capfd, *S.reference(*skey), cap=G, shape=(E, R))
    for pc, jacobi in (("jacobi", True), ("none", False)):
        r = sym.solve("cg", pc)
        sym.took(r, G)
        sym.right(r)
        sym.count(r, _oracle_cg(skey, jacobi)[1])
        sym.same_again(r)
    r = sym.solve("cg", "chebyshev", restart=4)
    sym.took(r, G)
    sym.right(r)
    sym.count(r, sym.solve("cg", "chebyshev", restart=4, persistent=False).its)
    sym.same_again(r, restart=4)

    non = _Bench(monkeypatch, capfd, *S.reference(*nkey), cap=G, shape=(E, R))
    r = non.solve("bicgstab", "jacobi")
    non.took(r, G, S.lds_layers(E, R))
    non.right(r)
    i0 = non.solve("bicgstab", "jacobi", persistent=False).its
    non.count(r, i0, 0.35 * i0 + 10)
    non.same_again(r)

    per, taken = _gmres_per(E, R, top)
    r = non.solve("gmres", "jacobi")
    if per is None and taken:
        non.took(r, G, S.lds_layers(E, R))
    else:
        non.refused(r)
    non.right(r)
    non.count(r, _oracle_gmres(nkey)[1])
    non.same_again(r)
    benches = [sym, non]
    if per is not None:
        gkey = nkey + (per,)
        g224 = _Bench(monkeypatch, capfd, *S.reference(*gkey), cap=G, shape=(E, R))
        assert S.expected_shape(g224.A.shape[0], S.longest_row(g224.A), 256, S.PG_ROWS, G) == (E, R, G)
        r = g224.solve("gmres", "jacobi")
        g224.took(r, G, S.lds_layers(E, R))
        g224.right(r)
        g224.count(r, _oracle_gmres(gkey)[1])
        g224.same_again(r)
        benches.append(g224)

    # GMRES(5) on the top member: the restart does happen (the cycle closes, x and the gather vector are formed anew)
    tper, ttaken = _gmres_per(E, R, True)
    tkey = (E, R, G, True, False, SEED) + ((tper,) if tper is not None else ())
    topm = _Bench(monkeypatch, capfd, *S.reference(*tkey), cap=G, shape=(E, R))
    r = topm.solve("gmres", "jacobi", restart=5)
    if ttaken:
        topm.took(r, G, S.lds_layers(E, R))
    else:
        topm.refused(r)
    topm.right(r)
    if not r.its > 5:
        topm.fail("gmres(5): no restart happened", r.its)
    benches.append(topm)
    assert not sum((q.failures for q in benches), []), "\n".join(sum((q.failures for q in benches), []))


def _edge_cases():
    # (cap, n, top): 16 rows per workgroup -- one row per group of lanes -- at 16, 17 and 33 workgroups (a full first-level
    # group of the barrier, a group of one, a third group), and n = 529 under the cap 33: 17 rows per workgroup, 32 workgroups
    # own rows, the last owner two of them, one workgroup none (an odd n has no offset n / 2: the low member).  Rows of 33 .. 64
    # entries do not fit a matrix of 16 or 32 rows, so the one-workgroup barrier (cap 1) and the half-filled group (cap 2) run on
    # the family's own sizes for (2,8): 128 rows per workgroup.
    return [pytest.param(1, S.family_size(8, 1, True), True, id="1"), pytest.param(2, S.family_size(8, 2, True), True, id="2"),
            pytest.param(16, 256, True, id="16"), pytest.param(17, 272, True, id="17"), pytest.param(33, 528, True, id="33"),
            pytest.param(33, 529, False, id="33-one-idle")]


@pytest.mark.parametrize("cap,n,top", _edge_cases())
def test_barrier_and_block_edges(cap, n, top, monkeypatch, capfd):
    """(b) the two-level barrier at 1, 2, 16, 17 and 33 workgroups, and a workgroup without rows, on shape (2,8)"""
    E, R = 2, 8
    benches = []
    for symmetric, method in ((True, "cg"), (False, "bicgstab")):
        key = (E, R, cap, top, symmetric, SEED, None, n)
        A, b, exact = S.reference(*key)
        assert A.shape[0] == n and S.expected_shape(n, S.longest_row(A), 256, S.PS_ROWS_MAX, cap) == (E, R, cap)
        if n == 529:
            per = -(-n // cap)
            assert per == 17 and -(-n // per) == 32 and n - 31 * per == 2
        q = _Bench(monkeypatch, capfd, A, b, exact, cap=cap, shape=(E, R))
        r = q.solve(method, "jacobi")
        q.took(r, cap)
        q.right(r)
        if method == "cg":
            q.count(r, _oracle_cg(key, True)[1])
        else:
            i0 = q.solve(method, "jacobi", persistent=False).its
            q.count(r, i0, 0.35 * i0 + 10)
        q.same_again(r)
        benches.append(q)
    assert not sum((q.failures for q in benches), []), "\n".join(sum((q.failures for q in benches), []))


@pytest.mark.parametrize("E,R", [(1, 56), (5, 13)])
@pytest.mark.parametrize("method", ["cg", "gmres"])
def test_start_vector_and_limits_at_a_large_shape(method, E, R, monkeypatch, capfd):
    """(c) a start from the solution, from a perturbed solution, the iteration limit against the oracle's iterate, b = 0.
    (GMRES at (1,56) has 896 rows per workgroup: refused, the multi-kernel loop answers the same questions.)"""
    G = 3
    key = (E, R, G, True, method == "cg", SEED)
    q = _Bench(monkeypatch, capfd, *S.reference(*key), cap=G, shape=(E, R))
    taken = method == "cg" or _gmres_per(E, R, True) == (None, True)
    layers = S.lds_layers(E, R) if method == "gmres" else 0

    def ran(r):
        q.took(r, G, layers) if taken else q.refused(r)

    r = q.solve(method, "jacobi")
    ran(r)
    q.right(r)
    rg = q.solve(method, "jacobi", guess=r.x)
    ran(rg)
    if not (rg.its <= 1 and rg.status == 0):
        q.fail("start from the solution", rg.its, rg.status)
    rp = q.solve(method, "jacobi", guess=r.x * (1.0 + 1e-3 * np.cos(np.arange(r.x.size))))
    ran(rp)
    q.right(rp)
    # the iteration limit: the oracle's iterate after 3 iterations (1e-10: the project's bound for CG's limit comparison)
    rm = q.solve(method, "jacobi", maxit=3)
    ran(rm)
    xo, io = _oracle_cg(key, True, 3) if method == "cg" else _oracle_gmres(key, 30, 3)
    assert io == 3
    if not (rm.its == 3 and rm.status != 0):
        q.fail("iteration limit", rm.its, rm.status)
    d = np.max(np.abs(rm.x - xo)) / np.max(np.abs(xo))
    if not d <= 1e-10:
        q.fail("iterate at the limit against the oracle's", d)
    rz = q.solve(method, "jacobi", b=np.zeros(q.A.shape[0]))
    ran(rz)
    if not (rz.its == 0 and not rz.x.any()):
        q.fail("b = 0", rz.its, float(np.max(np.abs(rz.x))))
    q.done()


@pytest.mark.parametrize("E,R", [(2, 8), (5, 11)])
def test_dead_diagonals(E, R, monkeypatch, capfd):
    """(d) a stored zero and an absent diagonal entry both count as 1 in the Jacobi scaling (rows 0 and n / 2 stored, rows 5 and
    n - 1 absent; the last one in the short block of the last workgroup)"""
    G = 3
    key = (E, R, G, True, False, SEED, None, None, True)
    A, b, exact = S.reference(*key)
    # the error bound of (a) is for a condition number of order 10; it is widened by the ratio of the condition numbers
    # (np.linalg.cond, 2-norm): (2,8) 3.7 -> 1.2e3, (5,11) 3.3 -> 3.4e3, ratios 3.4e2 and 1.0e3
    healthy = S.reference(E, R, G, True, False, SEED)[0]
    ratio = np.linalg.cond(A.toarray()) / np.linalg.cond(healthy.toarray())
    assert 1.0 <= ratio <= 2e3
    q = _Bench(monkeypatch, capfd, A, b, exact, cap=G, shape=(E, R))
    r = q.solve("gmres", "jacobi")
    q.took(r, G, S.lds_layers(E, R))
    q.right(r, tol=TOL * ratio, residual=False)
    q.count(r, _oracle_gmres(key)[1])
    r = q.solve("bicgstab", "jacobi")
    q.took(r, G, S.lds_layers(E, R))
    q.right(r, tol=TOL * ratio)
    q.done()


@pytest.mark.parametrize("cap", [None, "0", "-3", "1000", "x", "5"])
def test_the_cap_only_lowers_the_workgroup_count(cap, monkeypatch, capfd):
    """TIGAR_KSP_PERSISTENT_WGS unset, below 1, not a number or above min(CUs, ceil(n / 16)): the selection without a cap"""
    E, R = 2, 8
    A, b, exact = S.reference(E, R, 3, True, True, SEED)
    n = A.shape[0]
    natural = S.expected_shape(n, S.longest_row(A), _dev().device_info()["num_cu"], S.PS_ROWS_MAX)
    assert natural == (E, R, min(_dev().device_info()["num_cu"], -(-n // 16)))
    q = _Bench(monkeypatch, capfd, A, b, exact, cap=cap, shape=(E, R))
    r = q.solve("cg", "jacobi")
    q.took(r, min(natural[2], 5) if cap == "5" else natural[2])
    q.right(r)
    q.done()


def test_refusals_fall_back_to_the_multi_kernel_loop(monkeypatch, capfd):
    """(e) more than 1 024 rows per workgroup, a row of 161 entries, a restart beyond 30: the counter stays and the answer is
    right"""
    benches = []
    # one workgroup of 1 026 rows
    key = (1, 56, 1, True, True, SEED, None, 1026)
    A, b, exact = S.reference(*key)
    assert S.expected_shape(1026, S.longest_row(A), 256, S.PS_ROWS_MAX, 1) is None
    q = _Bench(monkeypatch, capfd, A, b, exact, cap=1, shape=(1, 56))
    for method in ("cg", "bicgstab"):
        r = q.solve(method, "jacobi")
        q.refused(r)
        q.right(r)
    benches.append(q)
    # one row of the (5,4) member widened from 160 to 161 entries
    A, b, _ = S.reference(5, 4, 3, True, False, SEED)
    A = A.tolil(copy=True)
    free = np.setdiff1d(np.arange(A.shape[0]), A.rows[0])
    A[0, free[:1]] = 1e-3
    A = A.tocsr()
    A.sort_indices()
    assert S.longest_row(A) == 161 and S.expected_shape(A.shape[0], 161, 256, S.PS_ROWS_MAX, 3) is None
    q = _Bench(monkeypatch, capfd, A, b, S.direct_solve(A, b), cap=3, shape=(5, 4))
    for method in ("gmres", "bicgstab"):
        r = q.solve(method, "jacobi")
        q.refused(r)
        q.right(r)
    benches.append(q)
    # GMRES(31): the basis of the kernel holds 30 vectors
    q = _Bench(monkeypatch, capfd, *S.reference(2, 8, 3, True, False, SEED), cap=3, shape=(2, 8))
    r = q.solve("gmres", "jacobi", restart=31)
    q.refused(r)
    q.right(r)
    r = q.solve("gmres", "jacobi", restart=30)
    q.took(r, 3)
    benches.append(q)
    assert not sum((q.failures for q in benches), []), "\n".join(sum((q.failures for q in benches), []))
