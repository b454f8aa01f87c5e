"""-m gpu: the wave-per-row PtAP kernels (tigar_amd/csrc/tg_ptap_wave.hip: k_gw, gw_row, gw_accum, gw_insert_new) at every lane
group and edge, through ``device.ptap_symbolic`` / ``device.ptap_numeric`` with ``TIGAR_PTAP_WAVE=1``.

References, bounds and operand builders: tests/ptap_wave_reference.py (the derivation of the per-entry bound is there; the
premises of the operands are asserted without a GPU in tests/test_ptap_wave_reference_host.py).  Two checks only: bit
equality with the exact reference, and |K_ij - ref_ij| <= 1.05 (T_ij + 2) 2^-53 mag_ij against numpy.longdouble.

Every product asserts its route first: the ``TIGAR_TRACE`` lines of the sites ``wave kernels, A M`` and ``wave kernels,
Mt (A M)`` end in ``done`` and no ``workgroup kernel`` line appears; the instantiation (table sizes, lane groups) is read
from the ``[gw]`` line of ``TIGAR_PTAP_WAVE_DEBUG``.  The tile hints are the one switch the trace does not show.  Lines
that begin with ``[ptap-wave]`` report what was seen (instantiations, ratio to the bound, repeatability of the bits)."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import ptap_wave_reference as R

pytestmark = pytest.mark.gpu

HASH, WAVE1, WAVE2 = "workgroup kernel", "wave kernels, A M", "wave kernels, Mt (A M)"
LINE = re.compile(r"\[tigar\] ptap temporary \((.+?)\): attempt (\d+) status (\d+) used (\d+) capacity (\d+) tables (\d+) / (\d+) -> (.+)")
GW = re.compile(r"\[gw\] max_am (\d+) mean_am ([\d.]+) max_k (\d+) mean_k ([\d.]+) ts (\d+) / (\d+) lg (\d+) / (\d+)")
SWITCHES = ["TIGAR_PTAP_WAVE_" + s for s in ("LG1", "LG2", "RPW1", "RPW2", "TILE1", "TILE2", "STRIDED", "LOADINV")]


def attempts(err, site):
    """[dict(status, used, tables, verdict)] of the site's lines in a captured stderr"""
    return [dict(status=int(m.group(3)), used=int(m.group(4)), tables=int(m.group(6)), verdict=m.group(8))
            for m in LINE.finditer(err) if m.group(1) == site]


def instantiation(err):
    """(ts_am, ts_k, lg_m, lg_am) of the plan"""
    got = GW.findall(err)
    assert len(got) == 1, err
    return tuple(int(x) for x in got[0][4:])


def assert_wave_route(err, placed=False):
    a1, a2 = attempts(err, WAVE1), attempts(err, WAVE2)
    assert not attempts(err, HASH), err
    assert a1 and a1[-1]["verdict"] == "done", err
    if placed:
        assert not a2, err                           # rows of K placed by the plan: no temporary
    else:
        assert a2 and a2[-1]["verdict"] == "done", err
    return a1, a2


def as_sorted(Kd):
    K = Kd.to_scipy().tocsr()
    K.sort_indices()
    return K


def same_bits(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64).view(np.int64), np.asarray(y, dtype=np.float64).view(np.int64))


def assert_exact(K, S, data):
    assert np.array_equal(K.indptr, S.indptr) and np.array_equal(K.indices, S.indices)
    assert same_bits(K.data, data)


def product(dev, capfd, M, A, zd=None, diag=1.0, rows=(0, 0, 0), MT=None, placed=True):
    """a fresh plan and its product through the public route; returns (K, err, (ts_am, ts_k, lg_m, lg_am), K of a second
    product on the plan -- rows placed directly -- or None).  `rows`, `MT`: first rows of the blocks of A, M and M^T, and
    the block of M^T"""
    capfd.readouterr()
    Ad, Md = dev.DeviceCSR.from_scipy(A), dev.DeviceCSR.from_scipy(M)
    MT = Md.transpose() if MT is None else MT
    plan = dev.ptap_symbolic(Ad, Md, MT, *rows)
    assert isinstance(plan, dev.PtAPPlan)
    K = as_sorted(dev.ptap_numeric(plan, Ad, Md, MT, zd, diag))
    err = capfd.readouterr().err
    assert_wave_route(err)
    K2 = None
    if placed:
        K2 = as_sorted(dev.ptap_numeric(plan, Ad, Md, MT, zd, diag))
        assert_wave_route(capfd.readouterr().err, placed=True)
    return K, err, instantiation(err), K2


@pytest.fixture
def dev(monkeypatch):
    from tigar_amd import device
    device.device_info()
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("TIGAR_TRACE", "1")
    monkeypatch.setenv("TIGAR_PTAP_WAVE", "1")
    monkeypatch.setenv("TIGAR_PTAP_WAVE_DEBUG", "1")
    return device


@pytest.fixture
def report():
    """lines for the log, printed when the test is over (``product`` empties what was captured before it)"""
    lines = []
    yield lambda text: lines.append("[ptap-wave] " + text)
    print("\n".join(lines))


def force_lg(monkeypatch, lg1, lg2):
    monkeypatch.setenv("TIGAR_PTAP_WAVE_LG1", str(lg1))
    monkeypatch.setenv("TIGAR_PTAP_WAVE_LG2", str(lg2))


# ---- the references, computed once
@pytest.fixture(scope="module")
def lane_exact():
    M, A, info = R.lane_group_operands(R.exact_value_source(1))
    S, data = R.exact_reference(M, A)
    zd = R.lane_group_zero_dofs(S, info)
    return dict(M=M, A=A, S=S, data=data, zd=zd, data_zd=R.exact_reference(M, A, zd, 2.5)[1])


@pytest.fixture(scope="module")
def lane_float():
    M, A, _ = R.lane_group_operands(R.normal_values(2), row_scale=R.decade_row_scale)
    S, ref, bound = R.float_reference(M, A)
    return dict(M=M, A=A, S=S, ref=ref, bound=bound)


def assert_bound(K, F):
    assert np.array_equal(K.indptr, F["S"].indptr) and np.array_equal(K.indices, F["S"].indices)
    ratio = R.bound_ratio(K.data, F["ref"], F["bound"])
    assert ratio <= 1.0, ratio
    return ratio


# ---- 1. every lane group, both stages
@pytest.mark.parametrize("lg2", R.LANE_GROUPS)
@pytest.mark.parametrize("lg1", R.LANE_GROUPS)
def test_every_lane_group(dev, report, monkeypatch, capfd, lane_exact, lane_float, lg1, lg2):
    """operand rows of 0, 1, G - 1, G, G + 1, 2 G + 1, 64, 65, 129 entries and outer rows of 0, 1, U NG - 1, U NG, U NG + 1, 63,
    64, 65, 130 in both stages: the exact set bit for bit (fresh plan and placed rows), the same with dofs to zero, the
    floating set inside the per-entry bound"""
    force_lg(monkeypatch, lg1, lg2)
    E, F = lane_exact, lane_float
    K, err, inst, K2 = product(dev, capfd, E["M"], E["A"])
    assert inst[2:] == (lg1, lg2)
    assert_exact(K, E["S"], E["data"])
    assert_exact(K2, E["S"], E["data"])
    K, err, inst, K2 = product(dev, capfd, E["M"], E["A"], E["zd"], 2.5)
    assert inst[2:] == (lg1, lg2)
    assert_exact(K, E["S"], E["data_zd"])
    assert_exact(K2, E["S"], E["data_zd"])
    K, err, inst, K2 = product(dev, capfd, F["M"], F["A"])
    assert inst[2:] == (lg1, lg2)
    ratio = max(assert_bound(K, F), assert_bound(K2, F))
    Kb, _, _, Kb2 = product(dev, capfd, F["M"], F["A"])
    repeat = same_bits(K.data, Kb.data) and same_bits(K.data, K2.data) and same_bits(K.data, Kb2.data)
    report("lane groups %d / %d: tables %d / %d, ratio to the bound %.3f, bits repeat %s" % (lg1, lg2, inst[0], inst[1], ratio, repeat))
    if lg1 == 6 and lg2 == 6:
        assert repeat


# ---- 2. the rule itself
@pytest.mark.parametrize("L,lg", [(8, 3), (12, 4), (24, 5), (48, 6), (100, 6)])
def test_the_rule_chooses_the_lane_group(dev, report, capfd, L, lg):
    M, A = R.uniform_operands(L, R.exact_value_source(L))
    K, err, inst, K2 = product(dev, capfd, M, A)
    report("rows of %d entries: tables %d / %d, lane groups %d / %d" % ((L,) + inst))
    assert inst[2:] == (lg, lg)
    S, data = R.exact_reference(M, A)
    assert_exact(K, S, data)
    assert_exact(K2, S, data)


# ---- 3. scheduling switches change nothing
def switched(monkeypatch, settings):
    for name in ("RPW1", "RPW2", "TILE1", "TILE2", "STRIDED"):
        monkeypatch.delenv("TIGAR_PTAP_WAVE_" + name, raising=False)
    for name, value in settings.items():
        monkeypatch.setenv("TIGAR_PTAP_WAVE_" + name, str(value))


@pytest.mark.parametrize("rpw", [1, 3, 8])
def test_rows_per_wave_and_row_counts(dev, monkeypatch, capfd, rpw):
    """1, 3, 4, 5 and 4 rpw k -+ 1 rows (k = 2) in both stages: the last workgroup, the last wave and the last row of a wave
    are partly empty.  Exact set bit for bit; floating set with 64-lane groups: the bits of the unswitched run"""
    force_lg(monkeypatch, 6, 6)
    for n in (1, 3, 4, 5, 8 * rpw - 1, 8 * rpw + 1):
        M, A = R.random_operands(n, R.exact_value_source(n), n)
        S, data = R.exact_reference(M, A)
        Mf, Af = R.random_operands(n, R.normal_values(n), n)
        F = dict(zip(("S", "ref", "bound"), R.float_reference(Mf, Af)))
        switched(monkeypatch, {})
        K0 = product(dev, capfd, Mf, Af)[0]
        assert_bound(K0, F)
        for r1, r2 in ((rpw, rpw), (rpw, 2), (8, rpw)):
            switched(monkeypatch, dict(RPW1=r1, RPW2=r2))
            K, err, inst, K2 = product(dev, capfd, M, A)
            assert_exact(K, S, data)
            assert_exact(K2, S, data)
            K, err, inst, K2 = product(dev, capfd, Mf, Af)
            assert inst[2:] == (6, 6)
            assert same_bits(K.data, K0.data) and same_bits(K2.data, K0.data)


def test_rows_per_wave_on_the_lane_group_set(dev, report, monkeypatch, capfd, lane_exact, lane_float):
    """RPW1, RPW2 in {1, 3, 8} on the ragged set (the rule itself drops the stride there: `used` is not 0); with 64-lane groups
    the bits of the floating set are those of the unswitched run, with the groups the rule chooses only the bound holds"""
    E, F = lane_exact, lane_float
    for lgs in ((6, 6), None):
        if lgs:
            force_lg(monkeypatch, *lgs)
        else:
            monkeypatch.delenv("TIGAR_PTAP_WAVE_LG1")
            monkeypatch.delenv("TIGAR_PTAP_WAVE_LG2")
        switched(monkeypatch, {})
        K0, err, inst0, _ = product(dev, capfd, F["M"], F["A"])
        a1, a2 = assert_wave_route(err)
        assert a1[-1]["used"] > 0 and a2[-1]["used"] > 0              # rows at the cursor
        ratio, differed = assert_bound(K0, F), False
        for r1, r2 in ((1, 1), (3, 3), (8, 8), (1, 8), (3, 1)):
            switched(monkeypatch, dict(RPW1=r1, RPW2=r2))
            K, err, inst, K2 = product(dev, capfd, E["M"], E["A"])
            assert_exact(K, E["S"], E["data"])
            assert_exact(K2, E["S"], E["data"])
            K, err, inst, K2 = product(dev, capfd, F["M"], F["A"])
            assert inst == inst0
            ratio = max(ratio, assert_bound(K, F), assert_bound(K2, F))
            same = same_bits(K.data, K0.data) and same_bits(K2.data, K0.data)
            differed = differed or not same
            if lgs:
                assert same
        report("rows per wave, lane groups %d / %d: ratio to the bound %.3f, bits differed %s" % (inst0[2], inst0[3], ratio, differed))


@pytest.mark.parametrize("hint", ["5,7,2,3,2", "5,7,9,9,9"])
def test_tile_ordered_rows(dev, report, monkeypatch, capfd, hint):
    """5 x 7 x 3 rows in both stages, tiles that neither divide the lattice nor fit inside it"""
    n = 105
    M, A = R.random_operands(n, R.exact_value_source(n), n, per_row=9)
    S, data = R.exact_reference(M, A)
    Mf, Af = R.random_operands(n, R.normal_values(n), n, per_row=9)
    F = dict(zip(("S", "ref", "bound"), R.float_reference(Mf, Af)))
    for lgs in ((6, 6), (3, 4)):
        force_lg(monkeypatch, *lgs)
        switched(monkeypatch, {})
        K0 = product(dev, capfd, Mf, Af)[0]
        ratio, differed = assert_bound(K0, F), False
        for which in (("TILE1",), ("TILE2",), ("TILE1", "TILE2")):
            switched(monkeypatch, {w: hint for w in which})
            K, err, inst, K2 = product(dev, capfd, M, A)
            assert_exact(K, S, data)
            assert_exact(K2, S, data)
            K, err, inst, K2 = product(dev, capfd, Mf, Af)
            assert inst[2:] == lgs
            ratio = max(ratio, assert_bound(K, F), assert_bound(K2, F))
            same = same_bits(K.data, K0.data) and same_bits(K2.data, K0.data)
            differed = differed or not same
            if lgs == (6, 6):
                assert same
        report("tiles %s, lane groups %d / %d: ratio to the bound %.3f, bits differed %s" % ((hint,) + lgs + (ratio, differed)))


def test_strided_and_cursor_placement(dev, report, monkeypatch, capfd):
    """rows of 24 entries: the rule keeps the stride (`used` is 0 exactly when rows are strided), TIGAR_PTAP_WAVE_STRIDED=0
    sends them to the cursor"""
    M, A = R.uniform_operands(24, R.exact_value_source(24))
    S, data = R.exact_reference(M, A)
    Mf, Af = R.uniform_operands(24, R.normal_values(24))
    Af = (sp.diags(R.decade_row_scale(np.random.default_rng(24), Af.shape[0])) @ Af).tocsr()
    F = dict(zip(("S", "ref", "bound"), R.float_reference(Mf, Af)))
    for lgs in ((6, 6), None):
        if lgs:
            force_lg(monkeypatch, *lgs)
        else:
            monkeypatch.delenv("TIGAR_PTAP_WAVE_LG1")
            monkeypatch.delenv("TIGAR_PTAP_WAVE_LG2")
        got = {}
        for strided in (True, False):
            switched(monkeypatch, {} if strided else dict(STRIDED=0))
            K, err, inst, K2 = product(dev, capfd, M, A)
            a1, a2 = assert_wave_route(err)
            assert (a1[-1]["used"] == 0) == strided and (a2[-1]["used"] == 0) == strided
            assert_exact(K, S, data)
            assert_exact(K2, S, data)
            K, err, inst, K2 = product(dev, capfd, Mf, Af)
            a1, a2 = assert_wave_route(err)
            assert (a1[-1]["used"] == 0) == strided and (a2[-1]["used"] == 0) == strided
            ratio = max(assert_bound(K, F), assert_bound(K2, F))
            got[strided] = (K.data, K2.data)
        same = all(same_bits(x, got[True][0]) for x in got[True] + got[False])
        report("strided / cursor, lane groups %d / %d: ratio to the bound %.3f, bits differed %s" % (inst[2], inst[3], ratio, not same))
        if lgs:
            assert same
        else:
            assert inst[2:] == (5, 5)


# ---- 4. the re-hash
@pytest.mark.parametrize("lg", R.LANE_GROUPS)
def test_seeded_rehash_of_one_row(dev, monkeypatch, capfd, lg):
    """a row of A M and a row of K with three columns that share both slots under the plain mix: no placement at attempt 0,
    one at attempt 1, tables unchanged -- only the seeded path can have produced the exact K"""
    force_lg(monkeypatch, lg, lg)
    M, A, row = R.rehash_operands(R.exact_value_source(7), "a")
    S, data = R.exact_reference(M, A)
    K, err, inst, K2 = product(dev, capfd, M, A)
    a1, a2 = assert_wave_route(err)
    assert [a["status"] for a in a1] == [0] and [a["status"] for a in a2] == [0]
    assert a1[0]["tables"] == inst[0] == 64 and a2[0]["tables"] == inst[1] == 64
    S_, AM = R.structural(M, A)
    for pattern, ts in ((AM, a1[0]["tables"]), (S_, a2[0]["tables"])):
        rows = R.rows_of(pattern)
        assert not R.placeable(rows[row], 0, ts) and R.placeable(rows[row], 1, ts)
        assert all(R.placeable(c, 0, ts) for i, c in enumerate(rows) if i != row)
    assert_exact(K, S, data)
    assert_exact(K2, S, data)


@pytest.mark.parametrize("lg", [3, 6])
def test_row_that_no_seed_settles_grows_the_table(dev, monkeypatch, capfd, lg):
    """twelve keys, one triple per hashing of the attempts 0 ... 3 at 64 slots: status 1, a retry at 128 slots, exact K.  (A wrong
    restatement of the hashing in the helper would let the row settle at once.)"""
    force_lg(monkeypatch, lg, lg)
    M, A, row = R.rehash_operands(R.exact_value_source(8), "b")
    S, data = R.exact_reference(M, A)
    K, err, inst, K2 = product(dev, capfd, M, A)
    a1, a2 = assert_wave_route(err)
    assert inst[:2] == (64, 64)
    for a in (a1, a2):
        assert [(x["status"], x["tables"], x["verdict"]) for x in a] == [(1, 64, "retry"), (0, 128, "done")]
    assert_exact(K, S, data)
    assert_exact(K2, S, data)


# ---- 5. row blocks
def test_row_blocks(dev, monkeypatch, capfd):
    """the rows [100, 180) of K from row blocks of A, M and M^T with non-zero first rows, as the streamed engines form them and
    as SplitPtAPPlan hands them on; dofs to zero inside and outside the block"""
    M, A = R.banded_operands(R.exact_value_source(5))
    d0, d1 = 100, 180
    (a0, a1), (m0, m1) = R.block_rows(M, A, d0, d1)
    assert min(a0, m0) > 0
    zd = [50, 120, 179, 200]
    S, _ = R.structural(M, A)
    Sb = S[d0:d1].tocsr()
    assert np.array_equal(Sb.indices, S.indices[S.indptr[d0]:S.indptr[d1]])
    MTd = dev.DeviceCSR.from_scipy(M.T.tocsr()[d0:d1])
    for lgs in ((3, 3), (6, 6)):
        force_lg(monkeypatch, *lgs)
        for dofs in (None, zd):
            whole = R.exact_reference(M, A, dofs, 2.5)[1][S.indptr[d0]:S.indptr[d1]]
            K, err, inst, K2 = product(dev, capfd, M[m0:m1], A[a0:a1], dofs, 2.5, rows=(a0, m0, d0), MT=MTd)
            assert inst[2:] == lgs
            assert_exact(K, Sb, whole)
            assert_exact(K2, Sb, whole)
    # the split plan's partial products on the same blocks (no dofs: it zeroes after the sum)
    capfd.readouterr()
    Ad, Md = dev.DeviceCSR.from_scipy(A[a0:a1]), dev.DeviceCSR.from_scipy(M[m0:m1])
    plan = dev.SplitPtAPPlan(Ad, Md, MTd, a0, m0, d0)
    K = as_sorted(dev.ptap_numeric(plan, Ad, Md, MTd))
    err = capfd.readouterr().err
    assert_wave_route(err)
    assert all(a["verdict"] in ("done", "retry") for a in attempts(err, WAVE1) + attempts(err, WAVE2))
    assert sum(1 for a in attempts(err, WAVE1) if a["verdict"] == "done") == len(plan.parts) >= 4
    assert_exact(K, Sb, R.exact_reference(M, A)[1][S.indptr[d0]:S.indptr[d1]])


# ---- 6. statuses, not faults
def _uncovered(values, offender):
    """8192 FE rows, 8000 dofs; the block of M holds its first 8000 rows, to which every row of A refers but (with `offender`)
    row 4097, which refers to row 8100: an odd row, which the plan's sample of every second row misses"""
    n, nc = 8192, 8000
    r = np.arange(n)
    M = R.csr_with(r, r % nc, (n, nc), values)
    c = r % nc
    rows = np.concatenate([r, r[c > 0], r[c < nc - 1]])
    cols = np.concatenate([c, c[c > 0] - 1, c[c < nc - 1] + 1])
    if offender:
        rows, cols = np.append(rows, 4097), np.append(cols, 8100)
    return M, R.csr_with(rows, cols, (n, n), values)


@pytest.mark.parametrize("stage", [1, 2])
def test_uncovered_row_is_a_status(dev, capfd, stage):
    """the kernel bounds-checks the operand row and reports status 3: TigarHipError from the numeric product (the symbolic
    pass's samples miss the row), no matrix, no fallback.  Stage 1: row 4097 of A refers to a row behind the block of M, in
    its LAST entry.  Stage 2: the block of A ends one row early, row 191 of M^T refers to that row in its second entry (the
    K rows sampled are the multiples of 15).  The flag is raised by the lane that read the entry, not by lane 0: a kernel
    that reports lane 0's flag only returned a K without the entry here"""
    M, A = _uncovered(R.exact_value_source(9), False)
    MTd = dev.DeviceCSR.from_scipy(M.T.tocsr())
    Mb = M[:8000]
    S, data = R.exact_reference(M, A)                       # (A refers to the first 8000 rows only: the block's product is K)
    K, err, inst, K2 = product(dev, capfd, Mb, A, MT=MTd)
    assert_exact(K, S, data)
    if stage == 1:
        A = _uncovered(R.exact_value_source(9), True)[1]
        assert A[4097].indices[-1] == 8100 and A[4097].nnz == 4
    else:
        A = A[:8191]
        assert list(M.T.tocsr()[191].indices) == [191, 8191]
    Ad, Md = dev.DeviceCSR.from_scipy(A), dev.DeviceCSR.from_scipy(Mb)
    capfd.readouterr()
    plan = dev.ptap_symbolic(Ad, Md, MTd, 0, 0, 0)
    assert isinstance(plan, dev.PtAPPlan)
    with pytest.raises(dev.TigarHipError, match="does not cover"):
        dev.ptap_numeric(plan, Ad, Md, MTd)
    err = capfd.readouterr().err
    a1, a2 = attempts(err, WAVE1), attempts(err, WAVE2)
    assert not attempts(err, HASH)
    if stage == 1:
        assert [(a["status"], a["verdict"]) for a in a1] == [(3, "gave up")] and not a2
    else:
        assert a1[-1]["verdict"] == "done" and [(a["status"], a["verdict"]) for a in a2] == [(3, "gave up")]


def test_plan_reused_on_another_pattern(dev, report, capfd):
    """M diagonal, so K has the pattern of A.  One more entry in A: the 'no longer match' error (or the correct K), never another
    K.  One entry moved within its row, every row length kept: the correct K on the new pattern"""
    n = 600
    values = R.exact_value_source(10)
    M, A = R.identity_like(n, values), R.tridiagonal_with_row(n, values, 300, [299, 300, 301])
    K, err, inst, K2 = product(dev, capfd, M, A)
    S, data = R.exact_reference(M, A)
    assert_exact(K2, S, data)
    Ad, Md = dev.DeviceCSR.from_scipy(A), dev.DeviceCSR.from_scipy(M)
    MT = Md.transpose()
    plan = dev.ptap_symbolic(Ad, Md, MT)
    assert_exact(as_sorted(dev.ptap_numeric(plan, Ad, Md, MT)), S, data)
    # moved: (300, 301) -> (300, 310)
    A3 = R.tridiagonal_with_row(n, R.exact_value_source(11), 300, [299, 300, 310])
    S3, data3 = R.exact_reference(M, A3)
    assert np.array_equal(S3.indptr, S.indptr) and not np.array_equal(S3.indices, S.indices)
    capfd.readouterr()
    K3 = as_sorted(dev.ptap_numeric(plan, dev.DeviceCSR.from_scipy(A3), Md, MT))
    assert_wave_route(capfd.readouterr().err, placed=True)
    assert_exact(K3, S3, data3)
    # one more: (300, 10)
    A4 = R.tridiagonal_with_row(n, R.exact_value_source(12), 300, [10, 299, 300, 310])
    S4, data4 = R.exact_reference(M, A4)
    capfd.readouterr()
    try:
        K4 = as_sorted(dev.ptap_numeric(plan, dev.DeviceCSR.from_scipy(A4), Md, MT))
    except dev.TigarHipError as e:
        report("one more entry in A: %s" % e)
        assert "no longer match" in str(e)
    else:
        report("one more entry in A: a layer planned again, K correct")
        assert_exact(K4, S4, data4)
    assert not attempts(capfd.readouterr().err, HASH)
