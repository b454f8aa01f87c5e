"""-m gpu: the kernels of the Kronecker-stage PtAP (tigar_amd/csrc/tg_ptap_box.hip: k_ptap_line, k_ptap_box, k_box_reach,
k_box_row_absmax) at their decode, run and box edges, ONE stage at a time through ``device.ptap_kron`` against
(x)F_k^T A (x)F_k built with scipy.sparse.kron.

References, bounds, operand builders and the restated host logic: tests/kron_stage_reference.py (the derivations of the
per-entry bounds are there; the premises of the operands and the route every case claims are asserted without a GPU in
tests/test_kron_stage_reference_host.py).  Two checks only: bit equality of pattern and values with the exact reference, and
|K_ij - ref_ij| <= bound_ij against numpy.longdouble.  Every case asserts its route first, from the ``TIGAR_TRACE`` lines
``kron stage: <row of g_kron_routes>`` and, for line stages, ``kron line runs: u= mlen= ...``; a declined stage returns None,
writes nothing and leaves the pool level.  Lines that begin with ``[kron-stage]`` report the measured ratio to the bound.

The run-loop cases keep their runs long at a few thousand rows with ``TIGAR_LINE_MIN_WAVES=1``; one case of 600 x 600 nodes
reaches runs of 20 rows at the default threshold."""
import functools
import re

import numpy as np
import pytest
import scipy.sparse as sp

import kron_stage_reference as R
import ptap_wave_reference as W
from test_gpu_ptap_retry import attempts, live_blocks

pytestmark = pytest.mark.gpu

ROUTE = re.compile(r"\[tigar\] kron stage: (\S+)")
RUNS = re.compile(r"\[tigar\] kron line runs: u=(-?\d+) mlen=(\d+) nchunk=(\d+) nx=(\d+) grab=(\d+)")
SWITCHES = ["TIGAR_LINE_RUN", "TIGAR_LINE_MIN_WAVES", "TIGAR_LINE_GRAB", "TIGAR_PTAP_LINE", "TIGAR_BOX_NT", "TIGAR_BOX_G1",
            "TIGAR_BOX_SLOWDECODE", "TIGAR_PTAP_ACCUM", "TIGAR_BOX_REACH_STRIDE", "TIGAR_BOX_EXACT_REACH", "TIGAR_PTAP_PROBE",
            "TIGAR_BOX_PROF", "TIGAR_PTAP_NOLOOSE"]
DIAG = 2.5


@pytest.fixture
def dev(monkeypatch):
    from tigar_amd import device
    device.device_info()
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("TIGAR_TRACE", "1")
    return device


@pytest.fixture
def report():
    lines = []
    yield lambda text: lines.append("[kron-stage] " + text)
    print("\n".join(lines))


def total_rows(c):
    return int(np.prod(R.nout_of(c)))


def zero_dofs(c):
    n = total_rows(c)
    return [0, min(3, n - 1), n // 2, n - 1]


def as_sorted(Kd):
    K = Kd.to_scipy().tocsr()
    K.sort_indices()
    return K


def same_bits(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64).view(np.int64), np.asarray(y, dtype=np.float64).view(np.int64))


def product(dev, capfd, c, rows=None, cur=None, zd=None, diag=1.0):
    """one stage through ptap_kron: (K as sorted scipy CSR or None when declined, the trace).  `rows`: the block of output
    rows; `cur`: the block of rows of A that is handed over"""
    A = c["A"]
    r0, r1 = cur or (0, A.shape[0])
    o0, o1 = rows or (0, total_rows(c))
    Ad = dev.DeviceCSR.from_scipy(A[r0:r1] if cur else A)
    capfd.readouterr()
    Kd = dev.ptap_kron(Ad, r0, c["dims"], c["factors"], o0, o1, zd, diag)
    err = capfd.readouterr().err
    K = None if Kd is None else as_sorted(Kd)
    del Ad, Kd
    return K, err


def assert_exact(K, S, data, rows=None):
    o0, o1 = rows or (0, S.shape[0])
    indptr, indices, values = R.rows_of_block(S, data, o0, o1)
    assert K.shape == (o1 - o0, S.shape[1])
    assert np.array_equal(K.indptr, indptr) and np.array_equal(K.indices, indices)
    assert same_bits(K.data, values)


def assert_bound(K, ref):
    S, val, bound, _ = ref
    assert np.array_equal(K.indptr, S.indptr) and np.array_equal(K.indices, S.indices)
    ratio = W.bound_ratio(K.data, val, bound)
    assert ratio <= 1.0, ratio
    return ratio


def runs_of(err):
    got = RUNS.findall(err)
    assert got, err
    return [dict(zip(("u", "mlen", "nchunk", "nx", "grab"), map(int, g))) for g in got]


def no_error_status(err):
    got = attempts(err, "box stage") + attempts(err, "line stage")
    assert got and all(a[1] in (0, 3) for a in got) and got[-1][2] == "done", err       # (3: the temporary grew, retried)


@functools.lru_cache(maxsize=None)
def exact_of(build, *args):
    c = build(*args)
    return c, R.exact_reference(c["dims"], c["factors"], c["A"])


@functools.lru_cache(maxsize=None)
def exact_zd_of(build, *args):
    c = build(*args)
    return R.exact_reference(c["dims"], c["factors"], c["A"], zero_dofs(c), DIAG)[1]


# ---- 1. decode classes
@pytest.mark.parametrize("name", list(R.DECODE_CASES))
def test_decode_class(dev, capfd, name):
    """exact operands on a 9- / 27-point A in every decode class: lo, mixed (the hi=0 instantiation through its 64-bit shift),
    hi (all eight hi=1 rows of g_kron_routes by name) and no24 (the second magic number does not exist: a one-direction stage
    on the box kernel).  The route first, then bit equality; dofs to zero in one case per class"""
    c, (S, data) = exact_of(R.decode_case, name)
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == [c["route"]]
    no_error_status(err)
    assert_exact(K, S, data)
    if name in ("lo-2d", "mixed-01", "hi-01-v1", "no24-256"):
        K, err = product(dev, capfd, c, zd=zero_dofs(c), diag=DIAG)
        assert ROUTE.findall(err) == [c["route"]]
        assert_exact(K, S, exact_zd_of(R.decode_case, name))
    del K
    assert live_blocks(dev) == before


# ---- 2. the run loop of the line kernel
@pytest.mark.parametrize("line_run", R.LINE_RUNS)
@pytest.mark.parametrize("which", ["u1", "u0", "u0-3d"])
def test_run_lengths_and_row_blocks(dev, monkeypatch, capfd, which, line_run):
    """runs of 1 ... 64 rows along directions 1 and 0 (2-D and across the lines of 3 planes), spans that are no multiple of the
    run, box extents that change from step to step; 100 is clamped to 64.  The whole product and blocks of rows that begin and
    end inside a run, a line and a plane -- the same bits as those rows of the whole product"""
    monkeypatch.setenv("TIGAR_LINE_MIN_WAVES", "1")
    monkeypatch.setenv("TIGAR_LINE_RUN", str(line_run))
    c, (S, data) = exact_of(R.run_case, which)
    nout = R.nout_of(c)
    before = live_blocks(dev)
    for rows in [(0, total_rows(c))] + R.RUN_BLOCKS[which]:
        K, err = product(dev, capfd, c, rows=rows)
        assert ROUTE.findall(err) == [R.RUN_ROUTES[which]]
        Q, (got,) = R.line_runs(nout, c["u"], rows[0], rows[1], line_run, 1), runs_of(err)
        assert (got["u"], got["mlen"], got["nchunk"], got["nx"]) == (c["u"], Q["mlen"], Q["nchunk"], Q["nx"])
        assert got["mlen"] <= 64 and (line_run > nout[c["u"]] or got["mlen"] == min(line_run, 64))
        no_error_status(err)
        assert_exact(K, S, data, rows)
    if line_run == 20:
        K, err = product(dev, capfd, c, zd=zero_dofs(c), diag=DIAG)
        assert_exact(K, S, exact_zd_of(R.run_case, which))
    del K
    assert live_blocks(dev) == before


@pytest.mark.parametrize("which", ["none", "none-3d"])
def test_stages_without_a_run_direction(dev, monkeypatch, capfd, which):
    monkeypatch.setenv("TIGAR_LINE_MIN_WAVES", "1")
    monkeypatch.setenv("TIGAR_LINE_RUN", "64")
    c, (S, data) = exact_of(R.run_case, which)
    before = live_blocks(dev)
    for rows in [(0, total_rows(c))] + R.RUN_BLOCKS[which]:
        K, err = product(dev, capfd, c, rows=rows)
        assert ROUTE.findall(err) == [R.RUN_ROUTES[which]] and runs_of(err)[0]["u"] == -1
        assert_exact(K, S, data, rows)
    del K
    assert live_blocks(dev) == before


@pytest.mark.parametrize("probe", ["0", "1"])
def test_row_block_of_the_operand_and_its_halo(dev, monkeypatch, capfd, probe):
    """cur_row0 > 0: the rows of A that the output block refers to and no more -- the bits of the whole product; one row less
    at the front is the error "slab halo too small", from the probe and (with the capacity of the run before in the cache) from
    the kernel itself, never a wrong result"""
    monkeypatch.setenv("TIGAR_LINE_MIN_WAVES", "1")
    monkeypatch.setenv("TIGAR_PTAP_PROBE", probe)
    c, (S, data) = exact_of(R.run_case, "u1")
    rows, cur = (36, 566), (27 * 3, 27 * 48)             # output (0, 3) ... (1, 47) of 12 x 70; the lines 3 ... 47 of A
    before = live_blocks(dev)
    K, err = product(dev, capfd, c, rows=rows, cur=cur)
    assert ROUTE.findall(err) == [R.RUN_ROUTES["u1"]] and runs_of(err)[0]["mlen"] == 20
    assert_exact(K, S, data, rows)
    del K
    with pytest.raises(Exception, match="slab halo too small"):
        product(dev, capfd, c, rows=rows, cur=(cur[0] + 1, cur[1]))
    assert live_blocks(dev) == before


@pytest.mark.parametrize("run", ["20", "64"])
def test_line_grab_changes_no_bit(dev, monkeypatch, capfd, run):
    """output entries a wave reserves at a time: 1 (every row reserves for itself), 64 and the default -- the look-ahead
    reservation across the rows of a run on rows of 0 ... 505 entries"""
    monkeypatch.setenv("TIGAR_LINE_MIN_WAVES", "1")
    monkeypatch.setenv("TIGAR_LINE_RUN", run)
    c, (S, data) = exact_of(R.operand_row_case)
    before = live_blocks(dev)
    for grab in ("1", "64", None):
        if grab is None:
            monkeypatch.delenv("TIGAR_LINE_GRAB")
        else:
            monkeypatch.setenv("TIGAR_LINE_GRAB", grab)
        K, err = product(dev, capfd, c)
        assert ROUTE.findall(err) == [R.LINE % (R.V1, 0, 1, 0)]
        assert runs_of(err)[0]["grab"] == int(grab or 8192) and runs_of(err)[0]["mlen"] == int(run)
        no_error_status(err)
        assert_exact(K, S, data)
    del K
    assert live_blocks(dev) == before


def test_runs_of_20_rows_at_the_default_threshold(dev, capfd):
    """600 x 600 nodes, no switch: 18 000 runs of 20 rows are more than 64 waves per CU, the halving loop leaves them alone"""
    c, (S, data) = exact_of(R.default_threshold_case)
    want = R.line_runs(R.nout_of(c), 1, 0, total_rows(c), 20, max(1, dev.device_info()["num_cu"] * 64))
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == [R.LINE % (R.V1, 0, 1, 1)]
    got = runs_of(err)[0]
    assert got["mlen"] == want["mlen"] == 20 and got["nchunk"] == 30 and got["nx"] == 600
    no_error_status(err)
    assert_exact(K, S, data)
    del K
    assert live_blocks(dev) == before


# ---- 3. operand rows and items of the line kernel
@pytest.mark.parametrize("zeros", [False, True])
def test_operand_rows_items_and_box_lines(dev, monkeypatch, capfd, zeros):
    """operand rows of 0 ... 257 entries against the 64-entry passes, 3 ... 12 items per output row against the batches of 4,
    boxes of 63, 64, 65 lines and contracted boxes of 63, 64, 65 slots; `zeros`: a tenth of the entries of A stored as +-0.0
    (entries of the pattern with value +0.0)"""
    monkeypatch.setenv("TIGAR_LINE_MIN_WAVES", "1")
    c, (S, data) = exact_of(R.operand_row_case, 5, zeros)
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == [R.LINE % (R.V1, 0, 1, 0)] and runs_of(err)[0]["mlen"] == 20
    assert_exact(K, S, data)
    K, err = product(dev, capfd, c, zd=zero_dofs(c), diag=DIAG)
    assert_exact(K, S, exact_zd_of(R.operand_row_case, 5, zeros))
    del K
    assert live_blocks(dev) == before


def test_support_lists_of_0_1_31_32_entries(dev, monkeypatch, capfd):
    """an all-zero column of F: an empty output row in every step of its runs; the longest list a line stage can have"""
    monkeypatch.setenv("TIGAR_LINE_MIN_WAVES", "1")
    c, (S, data) = exact_of(R.list_case)
    empty = c["columns"][0]
    assert all(S.indptr[empty + 10 * y] == S.indptr[empty + 10 * y + 1] for y in range(9))
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == [R.LINE % (R.V2, 0, 1, 0)] and runs_of(err)[0]["mlen"] == 9
    assert_exact(K, S, data)
    del K
    assert live_blocks(dev) == before


@functools.lru_cache(maxsize=None)
def floating_line(which):
    c = R.floating(R.run_case("u1") if which == "u1" else R.operand_row_case(), 31, W.decade_row_scale)
    return c, R.float_reference(c["dims"], c["factors"], c["A"])


@pytest.mark.parametrize("which", ["u1", "oprows"])
@pytest.mark.parametrize("line_run", ["1", "20", "64"])
def test_line_kernel_inside_its_bound(dev, report, monkeypatch, capfd, which, line_run):
    """normal values, rows of A scaled by 10^-6 ... 10^6: |K_ij - ref_ij| <= 1.05 (T_ij + 2) 2^-53 mag_ij"""
    monkeypatch.setenv("TIGAR_LINE_MIN_WAVES", "1")
    monkeypatch.setenv("TIGAR_LINE_RUN", line_run)
    c, ref = floating_line(which)
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == [R.LINE % (R.V1, 0, 1, 0)] and runs_of(err)[0]["mlen"] == int(line_run)
    report("line kernel, %s, runs of %s: ratio to the bound %.3f" % (which, line_run, assert_bound(K, ref)))
    del K
    assert live_blocks(dev) == before


# ---- 4. variant and size edges
@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_variant_and_size_edges(dev, capfd, name):
    """either side of maxB 20 | 21 and 32 | 33, Dmax 10 | 11 and 16 | 17, D == Ba, lists of 65, 96 | 97 entries, Dmax 48 | 49, the 60 KiB
    of the line kernel's box and the 150 KiB of the box kernel's: the kernel the limit says, bit for bit -- or declined:
    None, nothing in a builder, the pool level"""
    c, (S, data) = exact_of(R.edge_case, name)
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    if c["route"] is None or c.get("declines_in_kernel"):
        assert K is None
        assert ROUTE.findall(err) == ([c["route"]] if c.get("declines_in_kernel") else [])
        n = total_rows(c)
        Ad, bld = dev.DeviceCSR.from_scipy(c["A"]), dev.CSRBuilder(n, n, 1)
        assert dev.ptap_kron(Ad, 0, c["dims"], c["factors"], 0, n, append_to=bld) is None
        Kd = dev.DeviceCSR.from_scipy(sp.csr_matrix((data, S.indices, S.indptr), shape=S.shape))
        bld.append(Kd)                                      # all n rows still fit: the builder's row count did not move
        Kb = as_sorted(bld.finish())
        assert_exact(Kb, S, data)
        del Ad, bld, Kd, Kb
    else:
        assert ROUTE.findall(err) == [c["route"]]
        no_error_status(err)
        assert_exact(K, S, data)
    del K
    capfd.readouterr()
    assert live_blocks(dev) == before


# ---- 5. the box kernel
ACCUM = ["", "int", "float"]


def set_accum(monkeypatch, accum):
    if accum:
        monkeypatch.setenv("TIGAR_PTAP_ACCUM", accum)
    else:
        monkeypatch.delenv("TIGAR_PTAP_ACCUM", raising=False)


@pytest.mark.parametrize("nt", ["256", "64"])
@pytest.mark.parametrize("ncon", [1, 2, 3])
def test_box_kernel_one_two_three_directions(dev, monkeypatch, capfd, ncon, nt):
    """27-point A on 11 x 9 x 7 nodes, the first one, two, three directions contracted in one stage, both workgroup sizes; the
    exact set gives the same bits whatever the accumulation (unset, integer grid, floating point), also with dofs to zero"""
    monkeypatch.setenv("TIGAR_PTAP_LINE", "0")
    monkeypatch.setenv("TIGAR_BOX_NT", nt)
    c, (S, data) = exact_of(R.box_case, ncon)
    before = live_blocks(dev)
    for accum in ACCUM:
        set_accum(monkeypatch, accum)
        K, err = product(dev, capfd, c)
        assert ROUTE.findall(err) == ["k_ptap_box<%s>" % nt]
        no_error_status(err)
        assert_exact(K, S, data)
        K, err = product(dev, capfd, c, zd=zero_dofs(c), diag=DIAG)
        assert_exact(K, S, exact_zd_of(R.box_case, ncon))
        rows = (S.shape[0] // 3, S.shape[0] - 2)
        K, err = product(dev, capfd, c, rows=rows)
        assert_exact(K, S, data, rows)
    del K
    assert live_blocks(dev) == before


@pytest.mark.parametrize("nt", ["256", "64"])
def test_box_kernel_operand_rows_around_the_workgroup_size(dev, monkeypatch, capfd, nt):
    """output rows of 63, 64, 65 and 255, 256, 258 operand rows (the product of two list lengths): the staging of the operand-row
    descriptors in chunks of NT"""
    monkeypatch.setenv("TIGAR_BOX_NT", nt)
    c, (S, data) = exact_of(R.ncombo_case)
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == ["k_ptap_box<%s>" % nt]
    assert_exact(K, S, data)
    del K
    assert live_blocks(dev) == before


@pytest.mark.parametrize("g1", ["1", "4", "64"])
def test_box_kernel_lanes_per_operand_row(dev, monkeypatch, capfd, g1):
    """TIGAR_BOX_G1 lanes walk an operand row TG_BOX_UNROLL = 4 entries each at a time: rows of 3, 4, 5, 15, 16, 17, 255, 256, 257
    entries (and the others of the operand-row case, stored zeros included) around g1 * 4"""
    monkeypatch.setenv("TIGAR_PTAP_LINE", "0")
    monkeypatch.setenv("TIGAR_BOX_G1", g1)
    c, (S, data) = exact_of(R.operand_row_case, 5, True)
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == ["k_ptap_box<256>"]
    assert_exact(K, S, data)
    del K
    assert live_blocks(dev) == before


def test_box_kernel_second_buffer_larger_than_the_first(dev, capfd):
    """cap1 > cap: every node carries two functions, the box grows in the contraction"""
    c, (S, data) = exact_of(R.repeated_knot_case)
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == [c["route"]]
    assert_exact(K, S, data)
    K, err = product(dev, capfd, c, zd=zero_dofs(c), diag=DIAG)
    assert_exact(K, S, exact_zd_of(R.repeated_knot_case))
    del K
    assert live_blocks(dev) == before


def test_slow_decode_sends_a_line_stage_to_the_box_kernel(dev, monkeypatch, capfd):
    monkeypatch.setenv("TIGAR_BOX_SLOWDECODE", "1")
    c, (S, data) = exact_of(R.run_case, "u1")
    before = live_blocks(dev)
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == ["k_ptap_box<256>"]
    assert_exact(K, S, data)
    del K
    assert live_blocks(dev) == before


def test_stacked_view_into_the_box_kernel(dev, monkeypatch, capfd):
    """two loose-row halves of a first stage (line kernel, cut inside a line) as a stacked view: compacted once, then the box
    kernel -- the bits of the two-direction product"""
    both, first, second = R.view_case()
    S, data = R.exact_reference(both["dims"], both["factors"], both["A"])
    dims, F0, F1 = first["dims"], first["factors"][0], second[1]
    m0, n1 = F0.shape[1], dims[1]
    half = m0 * (n1 // 2) + 5
    before = live_blocks(dev)
    Ad = dev.DeviceCSR.from_scipy(first["A"])
    capfd.readouterr()
    lo = dev.ptap_kron(Ad, 0, dims, [F0, None], 0, half, intermediate=True)
    hi = dev.ptap_kron(Ad, 0, dims, [F0, None], half, m0 * n1, intermediate=True)
    assert ROUTE.findall(capfd.readouterr().err) == [R.RUN_ROUTES["u1"]] * 2
    view = dev.csr_vstack_view([lo, hi])
    assert view.is_loose()
    monkeypatch.setenv("TIGAR_PTAP_LINE", "0")
    K = as_sorted(dev.ptap_kron(view, 0, [m0, n1], second, 0, m0 * F1.shape[1]))
    err = capfd.readouterr().err
    assert ROUTE.findall(err) == ["k_ptap_box<256>"]                        # no kernel before the compaction, one after it
    assert_exact(K, S, data)
    del Ad, lo, hi, view, K
    assert live_blocks(dev) == before


@functools.lru_cache(maxsize=None)
def floating_box(ncon, step, accum):
    c = R.box_case(ncon, W.normal_values(50 + ncon), rows=R.two_scales(step))
    return c, R.float_reference(c["dims"], c["factors"], c["A"], kernel="box", accum=accum)


@pytest.mark.parametrize("step", [0, 1])
@pytest.mark.parametrize("ncon", [1, 2, 3])
def test_box_kernel_inside_the_bound_of_its_accumulation(dev, report, monkeypatch, capfd, ncon, step):
    """normal values, the largest entries of the operand rows at ratio exactly 2^16 (step 0: unset accumulates on the integer
    grid) and at the next double above it (step 1: unset accumulates in floating point).  Each mode against its own bound;
    the integer grid repeats its bits, and unset equals the mode tg_fix_choose takes"""
    monkeypatch.setenv("TIGAR_PTAP_LINE", "0")
    before = live_blocks(dev)
    got = {}
    for accum in ACCUM:
        set_accum(monkeypatch, accum)
        c, ref = floating_box(ncon, step, accum)
        K, err = product(dev, capfd, c)
        assert ROUTE.findall(err) == ["k_ptap_box<256>"]
        report("box kernel, %d directions, scales at 2^16 + %d ulp, accumulation %r: ratio to the bound %.3f"
               % (ncon, step, accum or "unset", assert_bound(K, ref)))
        got[accum] = K.data
        if accum == "int":
            K2, err = product(dev, capfd, c)
            assert same_bits(K.data, K2.data)
    if step == 0:
        assert same_bits(got[""], got["int"])
    del K, K2
    assert live_blocks(dev) == before


@pytest.mark.parametrize("line", ["1", "0"])
def test_sampled_reach_that_misses_an_entry_is_repeated_exactly(dev, monkeypatch, capfd, line):
    """k_box_reach on every 7th row misses a long-range entry: the kernel (line and box) flags the entry outside its box, the
    stage is run again with the exact reach -- the bits of the exact-reach run"""
    monkeypatch.setenv("TIGAR_PTAP_LINE", line)
    monkeypatch.setenv("TIGAR_LINE_MIN_WAVES", "1")
    c, (S, data) = exact_of(R.reach_stride_case)
    route = R.RUN_ROUTES["u1"] if line == "1" else "k_ptap_box<256>"
    before = live_blocks(dev)
    K0, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == [route]
    monkeypatch.setenv("TIGAR_BOX_REACH_STRIDE", str(c["stride"]))
    K, err = product(dev, capfd, c)
    assert ROUTE.findall(err) == [route, route]                 # sampled, then exact
    assert np.array_equal(K.indptr, K0.indptr) and np.array_equal(K.indices, K0.indices) and same_bits(K.data, K0.data)
    assert_exact(K, S, data)
    del K, K0
    assert live_blocks(dev) == before
