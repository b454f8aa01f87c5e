"""The CPU helper of the Kronecker-stage PtAP tests (tests/kron_stage_reference.py) and the premises of the inputs it builds:
what tests/test_gpu_kron_stage.py takes for granted about its operands, and the route every case claims, is asserted here
without a GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import kron_stage_reference as R
import ptap_wave_reference as W

NUM_CU = 256
TABLE = {R.LINE % (v, a, u, hi) for v in (R.V1, R.V2) for a, u in R.LINE_PAIRS for hi in (0, 1)} | {"k_ptap_box<256>", "k_ptap_box<64>"}


def geometry(c, **kw):
    return R.stage_geometry(c["dims"], c["factors"], c["A"], **kw)


# ---- decode
def test_decode_classes_of_the_index_spaces():
    for shape in [(129, 129, 1), (200, 200, 1)]:
        assert R.decode_class(*shape) == "lo", shape
    for shape in [(255, 255, 1), (127, 127, 9), (129, 129, 5)]:
        assert R.decode_class(*shape) == "mixed", shape
    for shape in [(257, 257, 1), (512, 128, 1), (257, 257, 7), (46341, 1, 1), (769, 769, 17)]:
        assert R.decode_class(*shape) == "hi", shape
    for shape in R.NO24_SHAPES:                            # the second magic number is not found: n0 <= 256 with a long n1
        a, b = R.decode_magics(*shape)
        assert a is not None and b is None and R.decode_class(*shape) == "no24", shape
    assert R.magic24(0, 10) is None and R.magic24(3, (1 << 24) + 1) is None
    assert R.magic24(1, 1) == (1, 0, 0)


@pytest.mark.parametrize("name", list(R.DECODE_CASES))
def test_decode_case_is_of_its_class_and_decodes_every_offset(name):
    """the class and the route the case claims; magic24 / decode24 against integer division at EVERY offset below the bound
    (what the kernel computes for the columns of a box is right before a GPU is asked)"""
    c = R.decode_case(name)
    G = geometry(c)
    assert (G["decode"], G["route"]) == (c["decode"], c["route"])
    n0, n1, B2 = G["nin"][0], G["nin"][1], G["maxB"][2]
    assert R.decode_class(n0, n1, B2) == c["decode"]
    if c["decode"] == "no24":
        assert not G["fast24"] and G["variant"] == 0
        return
    bam, dmt = R.LINE_VARIANTS[G["variant"]]
    assert all(D <= Ba <= bam and D <= dmt for Ba, D in R.line_box_shapes(G, c["factors"][G["a"]]))
    a, b = R.decode_magics(n0, n1, B2)
    assert (a[2], b[2]) == {"lo": (0, 0), "mixed": (1, 0), "hi": (1, 1)}[c["decode"]]
    n01 = n0 * n1
    e = np.arange(n01 * B2, dtype=np.int64)
    x2, x1, x0 = R.decode24(e, n0, n1, B2)
    assert np.array_equal(x2, e // n01) and np.array_equal(x1, (e % n01) // n0) and np.array_equal(x0, e % n0)


def test_every_line_case_decodes_every_offset():
    """the same for the small stages of the other groups (all of class lo but the default-threshold case)"""
    cases = [R.run_case(w) for w in R.RUN_BLOCKS] + [R.default_threshold_case(), R.operand_row_case(), R.list_case(), R.reach_stride_case()]
    cases += [R.edge_case(n) for n in R.EDGE_CASES]
    for c in cases:
        G = geometry(c)
        if not G["variant"]:
            continue
        bam, dmt = R.LINE_VARIANTS[G["variant"]]
        if not c.get("declines_in_kernel"):              # no box that the kernel would decline
            assert all(D <= Ba <= bam and D <= dmt for Ba, D in R.line_box_shapes(G, c["factors"][G["a"]]))
        n0, n1, B2 = G["nin"][0], G["nin"][1], G["maxB"][2]
        e = np.arange(n0 * n1 * B2, dtype=np.int64)
        x2, x1, x0 = R.decode24(e, n0, n1, B2)
        assert np.array_equal(x2, e // (n0 * n1)) and np.array_equal(x1, (e % (n0 * n1)) // n0) and np.array_equal(x0, e % n0)


def test_float_divmod_is_exact():
    """for all s < 2^16 and every divisor a box extent of the cases can be (1 ... 1400 covers the largest, 1316), and at the
    limits the kernel's comment states: s < 2^16 with s B < 2^21"""
    s = np.arange(1 << 16, dtype=np.int64)
    for B in range(1, 1401):
        q, r = R.float_divmod(s, B)
        assert np.array_equal(q, s // B) and np.array_equal(r, s % B), B
    for B in (1, 2, 31, 32, 33):
        top = np.arange(max(0, (1 << 21) // B - 70000), min(1 << 16, (1 << 21) // B), dtype=np.int64)
        q, r = R.float_divmod(top, B)
        assert np.array_equal(q, top // B)


# ---- runs
def covers(nout, u, r0, r1, line_run, min_waves):
    waves = R.run_rows(nout, u, r0, r1, line_run, min_waves)
    rows = sorted(r for w in waves for r in w)
    assert rows == list(range(r0, r1)), (nout, u, r0, r1, line_run, min_waves)
    Q = R.line_runs(nout, u, r0, r1, line_run, min_waves)
    assert all(len(w) <= max(Q["mlen"], 1) <= 64 for w in waves)
    return Q


def test_every_requested_row_is_written_by_exactly_one_wave():
    rng = np.random.default_rng(0)
    shapes = {1: [(7, 9, 1), (5, 4, 3), (1, 6, 2)], 0: [(9, 7, 1), (4, 5, 3), (6, 1, 2)], 2: [(3, 4, 9)], -1: [(11, 1, 1), (5, 1, 4)]}
    for u, nouts in shapes.items():
        for nout in nouts:
            total = nout[0] * nout[1] * nout[2]
            blocks = [(0, total), (0, 1), (total - 1, total), (total // 2, total // 2 + 1)]
            blocks += [tuple(sorted(rng.integers(0, total + 1, size=2))) for _ in range(12)]
            for r0, r1 in blocks:
                if r1 <= r0:
                    continue
                for line_run in list(range(1, 65)) + [100]:
                    for min_waves in (1, NUM_CU * 64):
                        covers(nout, u, int(r0), int(r1), line_run, min_waves)


def test_run_lengths_of_the_run_cases():
    want = {"u1": [1, 2, 3, 20, 63, 64, 64], "u0": [1, 2, 3, 20, 63, 64, 64], "u0-3d": [1, 2, 3, 20, 23, 23, 23]}
    for which, mlens in want.items():
        c = R.run_case(which)
        nout = R.nout_of(c)
        total = nout[0] * nout[1] * nout[2]
        for line_run, mlen in zip(R.LINE_RUNS, mlens):
            assert covers(nout, c["u"], 0, total, line_run, 1)["mlen"] == mlen
            for r0, r1 in R.RUN_BLOCKS[which]:
                covers(nout, c["u"], r0, r1, line_run, 1)
        span = nout[c["u"]]
        assert span % 20 and span % 63 and span % 64 or which == "u0-3d"
        assert covers(nout, c["u"], 0, total, 20, NUM_CU * 64)["mlen"] == 1          # what the suite saw before the switch
    c = R.default_threshold_case()
    Q = covers(R.nout_of(c), 1, 0, 360000, 20, NUM_CU * 64)
    assert Q["mlen"] == 20 and Q["nwaves"] == 18000 >= NUM_CU * 64


# ---- builders: routes and shapes
def test_run_cases_take_their_routes_and_their_extents_change_along_the_run():
    for which, route in R.RUN_ROUTES.items():
        c = R.run_case(which)
        G = geometry(c)
        assert G["route"] == route and G["u"] == c["u"]
        if c["u"] >= 0:
            ext = G["bhi"][c["u"]] - G["blo"][c["u"]] + 1
            assert len(set(ext[1:-1])) > 1                         # interior steps with different box extents
    G = geometry(R.run_case("u1"))
    assert len(set(G["bhi"][0] - G["blo"][0] + 1)) > 2                 # the wide window at one coordinate
    G = geometry(R.default_threshold_case())
    assert G["route"] == R.LINE % (R.V1, 0, 1, 1) and G["maxB"][0] == G["Dmax"][0] == 3


def test_operand_row_case_delivers_its_lengths():
    for zeros in (False, True):
        c = R.operand_row_case(zeros=zeros)
        G = geometry(c)
        assert G["route"] == R.LINE % (R.V1, 0, 1, 0)
        cnt = np.diff(c["A"].indptr)
        for L, row in c["designated"].items():
            assert cnt[row] == L
        shapes = R.line_row_shapes(G, c["factors"][0], c["A"], range(12 * 120))
        assert {l for s in shapes for l in s["operand_rows"]} >= set(R.OPERAND_ROWS)
        assert {s["items"] for s in shapes} >= set(R.ITEM_COUNTS)
        assert {s["len"] for s in shapes} == {3, 4, 5}
        assert {s["nlines"] for s in shapes} >= set(R.LINES_AND_SLOTS) and {s["nY"] for s in shapes} >= set(R.LINES_AND_SLOTS)
        assert all(s["D"] <= s["Ba"] for s in shapes)
    z = c["A"].data[c["A"].data == 0]
    assert np.signbit(z).any() and not np.signbit(z).all() and z.size > 1000
    assert geometry(c, line=False)["route"] == "k_ptap_box<256>"
    assert {3, 4, 5, 15, 16, 17, 255, 256, 257} <= set(cnt)            # around g1 * TG_BOX_UNROLL for g1 = 1, 4, 64


def test_list_case_delivers_its_lists():
    c = R.list_case()
    G = geometry(c)
    assert G["route"] == R.LINE % (R.V2, 0, 1, 0) and G["maxB"][0] == 32 and G["cstr"][0] == 32
    assert G["nout"][:2] == [10, 9]
    lens = np.diff(G["FT"][0].indptr)
    for L, col in c["columns"].items():
        assert lens[col] == L
    assert set(R.LIST_LENGTHS) <= set(lens)
    # one entry more is a box of 33 nodes: no line stage has a longer list
    src = W.exact_value_source(1)
    spans = [(50, 33) if sp_ == (50, 32) else sp_ for sp_ in R.LIST_SPANS]
    wider = R.stage((91, 9), 0, R.span_factor(spans, src), c["A"])
    assert geometry(wider)["route"] == "k_ptap_box<256>"


@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_edge_case_sits_on_its_edge(name):
    c = R.edge_case(name)
    G = geometry(c)
    assert G["route"] == c["route"] and G["declined"] == (c["route"] is None)
    if "maxB" in c:
        assert G["maxB"][0] == c["maxB"]
    if "Dmax" in c:
        assert G["Dmax"][0] == c["Dmax"]
    if "boxmax" in c:
        assert G["boxmax"] == c["boxmax"]
    if name == "D>Ba in one box":
        shapes = R.line_row_shapes(G, c["factors"][0], c["A"], range(G["nout"][0] * G["nout"][1]))
        bad = [s for s in shapes if s["D"] > s["Ba"]]
        assert G["Dmax"][0] <= G["maxB"][0] and bad and all((s["Ba"], s["D"]) == (1, 4) for s in bad)
    if name == "line LDS 60 KiB":
        assert G["line_lds"] <= 60 * 1024 < geometry(R.edge_case("line LDS above 60 KiB"))["line_lds"]
    if name == "box LDS 150 KiB":
        assert G["lds"] <= 150 * 1024 < geometry(R.edge_case("box LDS above 150 KiB"))["lds"]
    if name == "list 96":
        assert G["maxlen"][0] == R.TG_BOX_MAXLIST
    if name == "Dmax 48":
        assert G["Dmax"][0] == R.TG_BOX_MAXD


def test_the_line_limit_on_the_box_is_its_lds():
    """the driver's ``boxmax <= 2^16`` cannot be the edge between line and box kernel: 60 KiB of LDS hold 7464 slots"""
    assert (7464 + 20 * 10 + 10) * 8 <= 60 * 1024 < (7472 + 20 * 10 + 10) * 8


def test_box_cases_take_the_box_kernels():
    for c in (1, 2, 3):
        for nt in (256, 64):
            assert geometry(R.box_case(c), line=False, nt=nt)["route"] == "k_ptap_box<%d>" % nt
    c = R.ncombo_case()
    for nt in (256, 64):
        G = geometry(c, nt=nt)
        assert G["route"] == "k_ptap_box<%d>" % nt
    l0, l1 = np.diff(G["FT"][0].indptr), np.diff(G["FT"][1].indptr)
    for n, row in c["rows"].items():
        assert l0[row % 12] * l1[row // 12] == n
    c = R.repeated_knot_case()
    G = geometry(c)
    assert G["route"] == "k_ptap_box<256>" and G["Dmax"][0] > G["maxB"][0] and G["cap1"] >= 6 * 3 > G["boxmax"]
    assert geometry(R.run_case("u1"), slowdecode=True)["route"] == "k_ptap_box<256>"
    both, first, second = R.view_case()
    assert geometry(first)["route"] == R.RUN_ROUTES["u1"] and second[0] is None and second[1].shape == (70, 34)
    assert all(D <= Ba for Ba, D in R.line_box_shapes(geometry(first), first["factors"][0]))
    R.exact_reference(both["dims"], both["factors"], both["A"])
    c = R.reach_stride_case()
    sampled, exact = geometry(c, stride=c["stride"]), geometry(c)
    assert sampled["maxB"][0] < exact["maxB"][0] and sampled["route"] == exact["route"] == R.RUN_ROUTES["u1"]


def test_two_scales_sit_on_the_switch_of_tg_fix_choose():
    for c in (1, 2, 3):
        for step, all_float in ((0, False), (1, True)):
            cs = R.box_case(c, W.normal_values(40 + c), rows=R.two_scales(step))
            fp = R.box_row_is_float(R.projector(cs["dims"], cs["factors"]), cs["A"], "")
            assert fp.all() if all_float else not fp.any()


def test_the_union_of_asserted_routes_is_the_whole_table():
    import test_gpu_kron_routes as K
    assert R.claimed_routes() | {r for c in K.CASES for r in c[5]} == TABLE
    assert {n for n in R.claimed_routes() if "hi=1" in n} == {n for n in TABLE if "hi=1" in n}


# ---- references
def exact_cases():
    yield from (R.decode_case(n) for n in R.DECODE_CASES)
    yield from (R.run_case(w) for w in R.RUN_BLOCKS)
    yield from (R.default_threshold_case(), R.operand_row_case(), R.operand_row_case(zeros=True), R.list_case(), R.ncombo_case(),
                R.repeated_knot_case(), R.reach_stride_case())
    yield from (R.edge_case(n) for n in R.EDGE_CASES)
    yield from (R.box_case(c) for c in (1, 2, 3))


def test_exact_budget_holds_for_every_exact_case():
    for c in exact_cases():
        S, data = R.exact_reference(c["dims"], c["factors"], c["A"])           # (asserts the budget)
        assert data.shape == (S.nnz,) and not np.signbit(data[data == 0]).any()


def test_exact_reference_counts_stored_zeros_and_keeps_cancelled_entries():
    F = sp.csr_matrix(np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 2.0]]))
    A = sp.csr_matrix((np.array([1.0, -1.0, -0.0, 0.5]), np.array([0, 1, 2, 2]), np.array([0, 2, 3, 4])), shape=(3, 3))
    assert A.nnz == 4
    S, data = R.exact_reference([3], [F], A)
    assert S.toarray().tolist() == [[2.0, 1.0], [0.0, 1.0]]               # (0, 0) cancels and stays; (0, 1) is the stored -0.0
    assert data.tolist() == [0.0, 0.0, 2.0] and not np.signbit(data).any()
    S, data = R.exact_reference([3], [F], A, [0], 2.5)
    assert data.tolist() == [2.5, 0.0, 2.0]


def test_bounds_stand_2_to_the_10_above_the_reference_error():
    c = R.run_case("u1")
    A = sp.csr_matrix(c["A"], copy=True)
    A.data = W.normal_values(3)(A.nnz)
    S, ref, bound, own = R.float_reference(c["dims"], c["factors"], sp.diags(W.decade_row_scale(np.random.default_rng(1), A.shape[0])) @ A)
    assert np.all(bound >= 2.0 ** 10 * own) and np.all(own > 0)
    for k in (1, 2, 3):
        cs = R.box_case(k, W.normal_values(k), rows=R.two_scales(1))
        for accum in ("", "int", "float"):
            S, ref, bound, own = R.float_reference(cs["dims"], cs["factors"], cs["A"], kernel="box", accum=accum)
            assert np.all(bound >= 2.0 ** 10 * own) and np.all(own > 0)
    # the reference against the exact one on exact operands: within its own bound
    c = R.box_case(2)
    S, data = R.exact_reference(c["dims"], c["factors"], c["A"], [0, 5], 2.5)
    S2, ref, bound, own = R.float_reference(c["dims"], c["factors"], c["A"], [0, 5], 2.5, kernel="box")
    assert np.array_equal(S.indices, S2.indices) and np.all(abs(ref - data) <= own)
