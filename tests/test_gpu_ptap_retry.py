"""-m gpu: the grow-and-retry protocol of the bump-allocating PtAP passes (csrc/tg_bump.h) on inputs BUILT to overflow what the
symbolic passes size from a sample of rows -- the random matrices of tests/test_gpu_fuzz.py may or may not get there.  Every
test reads the trace of the helper (``TIGAR_TRACE=1``: one line per attempt and site) and asserts that the site it is about
did retry; K against scipy's M^T A M (pattern and values, 1e-12 of the largest entry as tests/fuzz/fuzz_kernels.py), a second
product on the same plan, and the number of live pool blocks before and after.

Attempts of these inputs on the code before the helper existed (its own debug lines, MI355X), which the helper repeats:
wave kernels with columns 1 and 3 of M filled in 160 rows: stage M^T (A M) 5 attempts (status 1, 1, 1, 4, 0); filled in all
rows: stage M^T (A M) 6 attempts, status 1 each, then the workgroup kernel; 300 extra entries in row 1 of A: stage A M
6 attempts (1, 1, 1, 1, 4, 0).  The workgroup kernel had no such line: from the formulas of tg_ptap_symbolic / tg_ptap_numeric the
dense columns 1 and 3 make it overflow the result table (64 slots from a sample maximum of 9) and the capacity (20 357
against 22 492 entries), hence at least two retries."""
import gc
import re

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

HASH, WAVE1, WAVE2, CELLS = "workgroup kernel", "wave kernels, A M", "wave kernels, Mt (A M)", "cell-block gather"
LINE = re.compile(r"\[tigar\] ptap temporary \((.+?)\): attempt (\d+) status (\d+) used (\d+) capacity (\d+) tables (\d+) / (\d+) -> (.+)")


def attempts(err, site):
    """[(attempt, status, verdict)] of the site's lines in a captured stderr"""
    return [(int(m.group(2)), int(m.group(3)), m.group(8)) for m in LINE.finditer(err) if m.group(1) == site]


def retries(err, site):
    return sum(1 for a in attempts(err, site) if a[2] == "retry")


def live_blocks(dev):
    gc.collect()
    dev.sync()
    return dev.pool_stats()[2]


def tridiagonal(n, rng, extra_row1=0):
    """A: tridiagonal, optionally with `extra_row1` more entries in row 1"""
    r = np.concatenate([np.arange(n), np.arange(1, n), np.arange(n - 1)])
    c = np.concatenate([np.arange(n), np.arange(n - 1), np.arange(1, n)])
    if extra_row1:
        r = np.concatenate([r, np.full(extra_row1, 1)])
        c = np.concatenate([c, 10 + np.arange(extra_row1)])
    A = sp.csr_matrix((rng.standard_normal(r.size), (r, c)), shape=(n, n))
    A.sort_indices()
    return A


def banded_m(n, rng, dense_rows=0):
    """M: columns {i-1, i, i+1} of row i (clipped), plus columns 1 and 3 in the rows [0, dense_rows)"""
    r = np.concatenate([np.arange(n), np.arange(1, n), np.arange(n - 1)] + [np.arange(dense_rows)] * 2)
    c = np.concatenate([np.arange(n), np.arange(n - 1), np.arange(1, n), np.full(dense_rows, 1), np.full(dense_rows, 3)])
    P = sp.csr_matrix((np.ones(r.size), (r, c)), shape=(n, n))          # (duplicates merge)
    P.sum_duplicates()
    P.sort_indices()
    P.data = rng.standard_normal(P.nnz)
    return P


def reference(M, A, zd, diag):
    K = (M.T @ A @ M).tolil()
    for i in zd:
        K[i, :] = 0.0
        K[:, i] = 0.0
        K[i, i] = diag                        # (the diagonal is structural in every K of this file)
    ones = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    S = (ones(M).T @ ones(A) @ ones(M)).tocsr()
    S.sort_indices()
    return K.tocsr(), S


def product_twice(dev, A, M, zd, diag, capfd, bitwise):
    """K of a fresh plan against scipy, the second product on the plan, the pool; returns the trace"""
    before = live_blocks(dev)
    capfd.readouterr()
    Ad, Md = dev.DeviceCSR.from_scipy(A), dev.DeviceCSR.from_scipy(M)
    MT = Md.transpose()
    plan = dev.ptap_symbolic(Ad, Md, MT)
    Kd = dev.ptap_numeric(plan, Ad, Md, MT, zd if zd else None, diag)
    err = capfd.readouterr().err
    K = Kd.to_scipy().tocsr()
    K.sort_indices()
    Ko, S = reference(M, A, zd, diag)
    assert np.array_equal(K.indptr, S.indptr) and np.array_equal(K.indices, S.indices)
    assert abs(K - Ko).max() <= 1e-12 * abs(Ko).max()
    K2 = dev.ptap_numeric(plan, Ad, Md, MT, zd if zd else None, diag).to_scipy().tocsr()
    K2.sort_indices()
    assert np.array_equal(K2.indptr, K.indptr) and np.array_equal(K2.indices, K.indices)
    if bitwise:
        assert np.array_equal(K2.data.view(np.int64), K.data.view(np.int64))
    else:                                      # (the wave kernels add floating-point numbers in the order of arrival)
        assert abs(K2 - K).max() <= 1e-13 * abs(K).max()
    err2 = capfd.readouterr().err
    assert not attempts(err2, HASH) and not attempts(err2, WAVE2)         # rows of K placed by the plan: no temporary
    del Ad, Md, MT, plan, Kd
    assert live_blocks(dev) == before
    return err, K


@pytest.fixture
def dev(monkeypatch):
    from tigar_amd import device
    device.device_info()
    monkeypatch.setenv("TIGAR_TRACE", "1")
    return device


@pytest.mark.parametrize("zd,diag", [((), 1.0), ((5, 1200), 2.5)])
def test_hash_kernel_grows_table_and_capacity(dev, monkeypatch, capfd, zd, diag):
    """the probe samples the K rows 0, 4, 8, ...: rows 1 and 3 (2048 entries each) are unseen, the result table (64 slots from
    a sample maximum of 9) and the capacity (20 357 against 22 492 entries) both overflow"""
    monkeypatch.setenv("TIGAR_PTAP_WAVE", "0")
    n = 2048
    rng = np.random.default_rng(1)
    A, M = tridiagonal(n, rng), banded_m(n, rng, dense_rows=n)
    err, K = product_twice(dev, A, M, list(zd), diag, capfd, bitwise=True)
    assert K.nnz == 22492
    got = attempts(err, HASH)
    print(got)
    assert retries(err, HASH) >= 2 and got[-1][2] == "done"
    assert {2, 4} <= {a[1] for a in got}                      # the result table and the capacity
    assert not attempts(err, WAVE1) and not attempts(err, WAVE2)


def test_wave_stage_2_grows_and_succeeds(dev, monkeypatch, capfd):
    """columns 1 and 3 of M filled in the rows 0 .. 159: the K rows 1 and 3 hold a few hundred entries against a stride and a
    table sized from about 9"""
    monkeypatch.setenv("TIGAR_PTAP_WAVE", "1")
    n = 2048
    rng = np.random.default_rng(2)
    A, M = tridiagonal(n, rng), banded_m(n, rng, dense_rows=160)
    err, K = product_twice(dev, A, M, [], 1.0, capfd, bitwise=False)
    got = attempts(err, WAVE2)
    print(got)
    assert retries(err, WAVE2) >= 1 and got[-1][2] == "done"
    assert [a[1] for a in got] == [1, 1, 1, 4, 0]             # as before the helper (module docstring)
    assert not attempts(err, HASH)                            # no decline


def test_wave_kernels_decline_and_the_hash_kernel_takes_over(dev, monkeypatch, capfd):
    """a row of 2048 entries cannot fit a table of 2048 slots within six doublings: 100, then K from the workgroup kernel"""
    monkeypatch.setenv("TIGAR_PTAP_WAVE", "1")
    n = 2048
    rng = np.random.default_rng(1)
    A, M = tridiagonal(n, rng), banded_m(n, rng, dense_rows=n)
    err, K = product_twice(dev, A, M, [], 1.0, capfd, bitwise=True)
    got = attempts(err, WAVE2)
    print(got, attempts(err, HASH))
    assert [a[1] for a in got] == [1] * 6 and all(a[2] == "retry" for a in got)      # as before the helper
    assert attempts(err, HASH)[-1][2] == "done" and retries(err, HASH) >= 2


def test_wave_stage_1_grows(dev, monkeypatch, capfd):
    """n = 8192: the plan samples every second row of A, and row 1 holds 300 entries more than the others"""
    monkeypatch.setenv("TIGAR_PTAP_WAVE", "1")
    n = 8192
    rng = np.random.default_rng(4)
    A, M = tridiagonal(n, rng, extra_row1=300), banded_m(n, rng)
    err, K = product_twice(dev, A, M, [], 1.0, capfd, bitwise=False)
    got = attempts(err, WAVE1)
    print(got)
    assert retries(err, WAVE1) >= 1 and got[-1][2] == "done"
    assert [a[1] for a in got] == [1, 1, 1, 1, 4, 0]          # as before the helper (module docstring)


def test_cell_block_gather_with_one_function_in_many_cells(dev, capfd):
    """the smallest case of tests/test_gpu_cellptap.py plus one function that every cell lists.  The plan of the cell-block
    product takes the longest row of K from ALL rows (tigar_amd/cellptap.py: klen.max()), not from a sample, so the stride of
    the temporary fits at the first attempt: correctness, one block, and the pool are what is asserted; against the general
    kernels."""
    from test_gpu_cellptap import _cells
    from tigar_amd.cellptap import CellBlockPtAP
    ncell, b, ncp = 64, 4, 40
    rng = np.random.default_rng(ncell + b)
    M, A = _cells(rng, ncell, b, ncp, 1, 8)
    M = M.tolil()
    M[np.arange(0, ncell * b, b), ncp - 1] = rng.standard_normal(ncell)        # function ncp - 1: in every cell
    M = M.tocsr()
    M.sort_indices()
    before = live_blocks(dev)
    capfd.readouterr()
    Md, Ad = dev.DeviceCSR.from_scipy(M), dev.DeviceCSR.from_scipy(A)
    plan = CellBlockPtAP(Md, b)
    zd = np.array([2, 17], dtype=np.int32)
    K = plan.ptap(Ad, zd, 2.5).to_scipy().tocsr()
    err = capfd.readouterr().err
    got = attempts(err, CELLS)
    print(got)
    assert len(got) >= 1 and got[-1][2] == "done" and all(a[1] in (0, 1, 4) for a in got)
    MT = Md.transpose()
    Kg = dev.ptap_numeric(dev.ptap_symbolic(Ad, Md, MT), Ad, Md, MT, zd, 2.5).to_scipy().tocsr()
    K.sort_indices(), Kg.sort_indices()
    assert np.array_equal(K.indptr, Kg.indptr) and np.array_equal(K.indices, Kg.indices)
    assert abs(K - Kg).max() <= 1e-12 * abs(Kg).max()
    assert K[ncp - 1].nnz == ncp                               # the row of the function every cell lists is full
    K2 = plan.ptap(Ad, zd, 2.5).to_scipy().tocsr()
    assert np.array_equal(K2.indices, K.indices) and np.array_equal(K2.data.view(np.int64), K.data.view(np.int64))
    del Md, Ad, MT, plan
    assert live_blocks(dev) == before


def kron_case(d, p, nel):
    """a Kronecker-form extraction, random values on the element-coupling pattern (direction 0 fastest), M as one matrix;
    `nel`: elements per direction, one number for all or one per direction"""
    from tigar_amd import BSplines as B
    from tigar_amd.kronptap import KronExtraction
    nels = [nel] * d if np.isscalar(nel) else list(nel)
    basis = B.ExplicitBSplineControlMesh([p] * d, [B.uniformKnots(p, 0., 1., n) for n in nels]).getScalarSpline()
    kx = KronExtraction(basis, basis.generateMesh(degree=p))
    pats = []
    for k in range(d):
        P1 = sp.lil_matrix((kx.nfe[k], kx.nfe[k]))
        for e in range(nels[k]):
            P1[p * e:p * e + p + 1, p * e:p * e + p + 1] = 1.0
        pats.append(P1.tocsr())
    A, Mo = pats[0], sp.csr_matrix(kx.M1[0])
    for k in range(1, d):
        A, Mo = sp.kron(pats[k], A).tocsr(), sp.kron(sp.csr_matrix(kx.M1[k]), Mo).tocsr()
    A.sort_indices()
    A.data = np.random.default_rng(d).standard_normal(A.nnz)
    return kx, A, Mo


def kron_chain(dev, kx, Ad, zd, diag, loose, builder, groups=None):
    """direction after direction (or group of directions after group) through ``ptap_kron``; `loose`: intermediate stages
    handed over as loose rows, `builder`: the last stage appended to a builder (else a matrix of its own)"""
    d = kx.d
    groups = groups or [[k] for k in range(d)]
    cur, done = Ad, set()
    for gi, group in enumerate(groups):
        last = gi == len(groups) - 1
        dims, fac = kx.dims(done), [kx.M1[j] if j in group else None for j in range(d)]
        done = done | set(group)
        n_out = int(np.prod(kx.dims(done)))
        if last and builder:
            bld = dev.CSRBuilder(n_out, n_out, 1)
            assert dev.ptap_kron(cur, 0, dims, fac, 0, n_out, zd, diag, append_to=bld) is True
            cur = bld.finish()
        elif last:
            cur = dev.ptap_kron(cur, 0, dims, fac, 0, n_out, zd, diag)
        else:
            cur = dev.ptap_kron(cur, 0, dims, fac, 0, n_out, intermediate=loose)
            assert cur.is_loose() == loose
    K = cur.to_scipy().tocsr()
    K.sort_indices()
    return K


@pytest.mark.parametrize("d,p,nel", [(2, 2, 12), (3, 2, 6)])
def test_box_and_line_stages_by_all_three_endings(dev, capfd, d, p, nel):
    """the stages of a Kronecker-form product through ``ptap_kron``: intermediate stages handed over as loose rows and the last
    one as a matrix of its own, the last one appended to a builder, and every stage as a matrix of its own -- the same K bit
    for bit, and scipy's.  Whether a stage retries depends on what the capacity cache has seen before: no line may report
    an error status."""
    kx, A, Mo = kron_case(d, p, nel)
    zd = np.array([0, 7], dtype=np.int32)
    before = live_blocks(dev)
    capfd.readouterr()
    Ad = dev.DeviceCSR.from_scipy(A)
    K_own, K_loose, K_builder = (kron_chain(dev, kx, Ad, zd, 2.5, *how) for how in ((False, False), (True, False), (True, True)))
    err = capfd.readouterr().err
    got = attempts(err, "box stage") + attempts(err, "line stage")
    print(got)
    assert len(got) >= 3 * d and all(a[1] in (0, 3) for a in got)        # 3: the temporary was too small (TG_BOX_CAP)
    assert sum(1 for a in got if a[2] == "done") == 3 * d
    for Kx in (K_loose, K_builder):
        assert np.array_equal(Kx.indptr, K_own.indptr) and np.array_equal(Kx.indices, K_own.indices)
        assert np.array_equal(Kx.data.view(np.int64), K_own.data.view(np.int64))
    Ko, S = reference(Mo, A, list(zd), 2.5)
    assert np.array_equal(K_own.indptr, S.indptr) and np.array_equal(K_own.indices, S.indices)
    assert abs(K_own - Ko).max() <= 1e-12 * abs(Ko).max()
    del Ad
    assert live_blocks(dev) == before
