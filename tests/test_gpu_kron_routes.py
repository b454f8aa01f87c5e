"""-m gpu: the host driver of the Kronecker-stage PtAP (csrc/tg_ptap_box.hip: tg_kron_* stages, the table g_kron_routes) row by
row.  Every case is one chain of stages through ``dev.ptap_kron`` against scipy's M^T A M: the pattern equal to the structural
product, the values within 1e-12 of the largest entry (the bound of tests/test_gpu_ptap_retry.py), the pool level.  Which row
of the table a stage took is read from the trace (``TIGAR_TRACE=1``: "[tigar] kron stage: <row>") and asserted.

Rows: all eight (variant, a, u) combinations of ``k_ptap_line`` and both workgroup sizes of ``k_ptap_box``.  The hi flag follows
from the 24-bit magic numbers of the sizes (tg_magic24, one flag per divisor: the quotient needs the high half of the product
from bound * divisor >= 2^32 on; the template takes hi=1 when BOTH divisors carry it, about n0 * n1 >= 2^16), so the small
shapes here reach the hi=0 row of every pair, with both quotients from the low word.  The hi=1 rows, the hi=0 row with one
flag set (its 64-bit shift) and the sizes for which no 24-bit magic number exists are run by tests/test_gpu_kron_stage.py,
which tests the kernels one stage at a time; the union of the rows asserted by name in the two files is the whole table
(tests/test_kron_stage_reference_host.py).
Variant <20,10> holds boxes of up to 20 nodes along the contracted direction: p = 2 and 3 (p^2 + 3 p - 1 = 9 and 17 nodes);
p = 4 with 5 or 6 elements (21 or 25 nodes) takes <32,16>.

Endings: one line case and one box case as a matrix of its own, as loose rows and appended to a builder, bit for bit equal.
The ladder of tg_ptap_kron_any: a stacked view into the box kernel (compacted, then as usual) and a support list longer than
TG_BOX_MAXLIST (declined on the host); the sampled reach is covered by tests/test_gpu_api.py."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_ptap_retry import attempts, kron_case, kron_chain, live_blocks, reference, tridiagonal

pytestmark = pytest.mark.gpu

ROUTE = re.compile(r"\[tigar\] kron stage: (\S+)")
LINE0, NT64 = {"TIGAR_PTAP_LINE": "0"}, {"TIGAR_PTAP_LINE": "0", "TIGAR_BOX_NT": "64"}
# (d, p, elements, direction groups, switches, the rows its stages take in order)
CASES = [
    (1, 3, 6, None, {}, ["k_ptap_line<20,10,0,-1,hi=0>"]),
    (2, 2, 4, None, {}, ["k_ptap_line<20,10,0,1,hi=0>", "k_ptap_line<20,10,1,0,hi=0>"]),
    (3, 2, 3, None, {}, ["k_ptap_line<20,10,0,1,hi=0>", "k_ptap_line<20,10,1,0,hi=0>", "k_ptap_line<20,10,2,0,hi=0>"]),
    (1, 4, 6, None, {}, ["k_ptap_line<32,16,0,-1,hi=0>"]),
    (2, 4, 5, None, {}, ["k_ptap_line<32,16,0,1,hi=0>", "k_ptap_line<32,16,1,0,hi=0>"]),
    (3, 4, (1, 1, 5), None, {}, ["k_ptap_line<20,10,0,1,hi=0>", "k_ptap_line<20,10,1,0,hi=0>", "k_ptap_line<32,16,2,0,hi=0>"]),
    (2, 3, 4, None, LINE0, ["k_ptap_box<256>", "k_ptap_box<256>"]),
    (2, 2, 5, None, NT64, ["k_ptap_box<64>", "k_ptap_box<64>"]),
    (3, 2, 3, [[0, 1], [2]], {}, ["k_ptap_box<256>", "k_ptap_line<20,10,2,0,hi=0>"]),
    (3, 3, 2, [[0, 1], [2]], NT64, ["k_ptap_box<64>", "k_ptap_box<64>"]),
]
ENDINGS = ((False, False), (True, False), (True, True))       # (loose intermediates, builder) of kron_chain
ZD, DIAG = np.array([0, 3], dtype=np.int32), 2.5


@pytest.fixture
def dev(monkeypatch):
    from tigar_amd import device
    device.device_info()
    monkeypatch.setenv("TIGAR_TRACE", "1")
    return device


def check_against_scipy(K, Mo, A):
    Ko, S = reference(Mo, A, list(ZD), DIAG)
    assert np.array_equal(K.indptr, S.indptr) and np.array_equal(K.indices, S.indices)
    assert abs(K - Ko).max() <= 1e-12 * abs(Ko).max()


def test_the_cases_name_every_line_combination_and_both_box_sizes():
    rows = {r for c in CASES for r in c[5]}
    want = {"k_ptap_line<%s,%d,%d,hi=0>" % (v, a, u) for v in ("20,10", "32,16") for a, u in ((0, 1), (1, 0), (2, 0), (0, -1))}
    assert rows == want | {"k_ptap_box<256>", "k_ptap_box<64>"}


@pytest.mark.parametrize("d,p,nel,groups,env,rows", CASES)
def test_stage_takes_its_row_and_equals_scipy(dev, monkeypatch, capfd, d, p, nel, groups, env, rows):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    kx, A, Mo = kron_case(d, p, nel)
    before = live_blocks(dev)
    capfd.readouterr()
    Ad = dev.DeviceCSR.from_scipy(A)
    K = kron_chain(dev, kx, Ad, ZD, DIAG, True, False, groups)
    err = capfd.readouterr().err
    print(ROUTE.findall(err))
    assert ROUTE.findall(err) == rows
    check_against_scipy(K, Mo, A)
    del Ad
    assert live_blocks(dev) == before


@pytest.mark.parametrize("d,p,nel,groups,env,rows", [CASES[2], CASES[6]])
def test_line_and_box_case_by_all_three_endings(dev, monkeypatch, capfd, d, p, nel, groups, env, rows):
    """a matrix of its own after every stage, loose intermediates, the last stage appended to a builder: the same K bit for bit"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    kx, A, Mo = kron_case(d, p, nel)
    before = live_blocks(dev)
    capfd.readouterr()
    Ad = dev.DeviceCSR.from_scipy(A)
    K_own, K_loose, K_builder = (kron_chain(dev, kx, Ad, ZD, DIAG, *how, groups) for how in ENDINGS)
    err = capfd.readouterr().err
    assert ROUTE.findall(err) == rows * 3
    got = attempts(err, "box stage") + attempts(err, "line stage")
    assert all(a[1] in (0, 3) for a in got) and sum(1 for a in got if a[2] == "done") == 3 * len(rows)
    for Kx in (K_loose, K_builder):
        assert np.array_equal(Kx.indptr, K_own.indptr) and np.array_equal(Kx.indices, K_own.indices)
        assert np.array_equal(Kx.data.view(np.int64), K_own.data.view(np.int64))
    check_against_scipy(K_own, Mo, A)
    del Ad
    assert live_blocks(dev) == before


def test_stacked_view_into_the_box_kernel_is_compacted(dev, monkeypatch, capfd):
    """the box kernel reads columns and values through one row start, a stacked view has two: the driver answers "needs
    compaction" to itself, compacts once and runs the stage on the copy -- the result of the stage fed the stacked copy"""
    kx, A, Mo = kron_case(3, 2, 3)
    before = live_blocks(dev)
    Ad = dev.DeviceCSR.from_scipy(A)
    plane = kx.ncp[0] * kx.nfe[1]
    n_x, half = plane * kx.nfe[2], (kx.nfe[2] // 2) * plane
    dims, fac = kx.dims(set()), [kx.M1[0], None, None]
    lo = dev.ptap_kron(Ad, 0, dims, fac, 0, half, intermediate=True)
    hi = dev.ptap_kron(Ad, 0, dims, fac, half, n_x, intermediate=True)
    view, copy = dev.csr_vstack_view([lo, hi]), dev.csr_vstack([lo, hi])
    assert view.is_loose() and copy.is_loose()
    monkeypatch.setenv("TIGAR_PTAP_LINE", "0")
    dims_y, fac_y, n_y = kx.dims({0}), [None, kx.M1[1], None], kx.ncp[0] * kx.ncp[1] * kx.nfe[2]
    capfd.readouterr()
    y_view = dev.ptap_kron(view, 0, dims_y, fac_y, 0, n_y).to_scipy()
    err = capfd.readouterr().err
    assert ROUTE.findall(err) == ["k_ptap_box<256>"]                        # no kernel before the compaction, one after it
    assert [a[2] for a in attempts(err, "box stage")][-1] == "done" and not attempts(err, "line stage")
    y_copy = dev.ptap_kron(copy, 0, dims_y, fac_y, 0, n_y).to_scipy()
    assert np.array_equal(y_view.indptr, y_copy.indptr) and np.array_equal(y_view.indices, y_copy.indices)
    assert abs(y_view - y_copy).max() <= 1e-13 * abs(y_copy).max()            # the bound of test_loose_row_stage_results
    Mxy = sp.kron(sp.identity(kx.nfe[2]), sp.kron(sp.csr_matrix(kx.M1[1]), sp.csr_matrix(kx.M1[0]))).tocsr()
    Yo = (Mxy.T @ A @ Mxy).tocsr()
    assert abs(y_view - Yo).max() <= 1e-12 * abs(Yo).max()
    del Ad, lo, hi, view, copy
    assert live_blocks(dev) == before


def test_support_list_too_long_declines_on_the_host(dev, capfd):
    """d = 1, a 128 x 4 factor whose column 1 is full: a support list of 128 entries against TG_BOX_MAXLIST = 96.  Declined
    (None) as a matrix of its own and with a builder, before any product kernel; nothing reaches the builder, the pool is level"""
    n, m = 128, 4
    rng = np.random.default_rng(5)
    F = sp.lil_matrix((n, m))
    F[np.arange(n), np.arange(n) // 32] = 1.0
    F[:, 1] = 1.0
    F = F.tocsr()
    F.data = rng.standard_normal(F.nnz)
    A = tridiagonal(n, rng)
    Ko = (F.T @ A @ F).tocsr()
    Ko.sort_indices()
    before = live_blocks(dev)
    capfd.readouterr()
    Ad = dev.DeviceCSR.from_scipy(A)
    assert dev.ptap_kron(Ad, 0, [n], [F], 0, m) is None
    bld = dev.CSRBuilder(m, m, 1)
    assert dev.ptap_kron(Ad, 0, [n], [F], 0, m, append_to=bld) is None
    err = capfd.readouterr().err
    assert not ROUTE.findall(err) and not attempts(err, "box stage") and not attempts(err, "line stage")
    bld.append(dev.DeviceCSR.from_scipy(Ko))             # all m rows still fit: the builder's row count did not move
    Kb = bld.finish().to_scipy()
    assert Kb.shape == (m, m) and np.array_equal(Kb.indptr, Ko.indptr) and np.array_equal(Kb.data, Ko.data)
    del Ad, bld
    assert live_blocks(dev) == before
