"""Seeded random patches through generateM / extractMatrix / extractVector / solveLinearSystem against the oracle
(`tests/fuzz/fuzz_parity.py`: dimension, degrees per direction, element counts, periodic directions, repeated and non-uniform
knots, several fields, boundary dofs, FE matrices on and off the element-coupling pattern), once per set of environment
switches so that every family of kernels sees them (tIGAr/common.py:1516-1578, 1142-1204, 1236-1263)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env, tool="fuzz_parity.py"):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz", tool)] + args, env=e, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stdout[-2000:]
    return r.returncode, json.loads(lines[-1]), [l for l in lines[:-1]]


@pytest.mark.parametrize("seed,env", [
    (101, {}),
    (102, {"TIGAR_POOL_POISON": "1"}),
    (103, {"TIGAR_IMPLICIT_M": "1"}),
    (104, {"TIGAR_PTAP_TENSOR": "0"}),
    (105, {"TIGAR_PTAP_TENSOR": "0", "TIGAR_PTAP_FACTORED": "0"}),
    (106, {"TIGAR_PTAP_TENSOR": "0", "TIGAR_PTAP_FACTORED": "0", "TIGAR_PTAP_WAVE": "1"}),
    (107, {"TIGAR_KSP_PERSISTENT": "1"}),
    (108, {"TIGAR_PTAP_UNWRAP": "0"}),
    (109, {"TIGAR_EXTRACT_KRON": "0"}),
    (110, {"TIGAR_FUZZ_ROUNDTRIP": "1"}),        # through writeExtraction / ExtractedSpline(dirname): a stored M without structure
    (111, {"TIGAR_PTAP_TENSOR": "0", "TIGAR_PTAP_FACTORED": "0", "TIGAR_PTAP_ELEMENTS": "2"}),   # element-split cell products
    # round 6: the element chunks of the streamed engine (implicit M, two element layers per chunk), and the element split on its
    # alternative kernels (multi-way merge for the row patterns, vector-unit cell products, node -> cells as lists)
    (112, {"TIGAR_PTAP_TENSOR": "0", "TIGAR_PTAP_FACTORED": "0", "TIGAR_PTAP_ELEMENTS": "2", "TIGAR_IMPLICIT_M": "1",
           "TIGAR_ELEM_LAYERS": "2"}),
    (113, {"TIGAR_PTAP_TENSOR": "0", "TIGAR_PTAP_FACTORED": "0", "TIGAR_PTAP_ELEMENTS": "2", "TIGAR_EL_MERGE": "1",
           "TIGAR_EL_VALU": "1", "TIGAR_EL_LISTS": "1"}),
])
def test_random_patches_match_the_oracle(seed, env):
    rc, summary, failures = _run(["--seed", str(seed), "--cases", "80"], env)
    assert rc == 0 and summary["failed"] == 0, "\n".join(failures)[:4000]
    if not env:
        assert summary["cases_on_the_tensor_walks"] > 0


def test_hand_added_couplings_that_end_inside_an_element_of_a_repeated_knot_direction():
    """found by the random run: the line kernel of the sum-factorised stages stores a contracted line over the head of its
    own line of the box, which needs (functions reachable from the box) <= (nodes of the box) per OUTPUT ROW; the host
    compared the maxima only.  A coupling added by hand can end a box inside an element, and with repeated knots that
    element brings more functions than the box has nodes of it: such rows are declined now (general kernels)."""
    force = json.dumps({"matrix": "random_extra", "nfields": 1})
    for first in (1, 185, 197, 291):
        rc, summary, failures = _run(["--seed", "5", "--first", str(first), "--cases", "1", "--force", force], {})
        assert rc == 0 and summary["failed"] == 0, "\n".join(failures)[:4000]


def test_hand_added_couplings_on_patches_with_repeated_knots():
    """found by the random runs of round 6 (seeds 6901 / 51 and 6902 / 291; present since round 3): ONE coupling added by hand to
    a block of a 3-D p = 3 patch with repeated knots came out with rows of K short by their last entries (16 rows with wrong
    values, 57 entries missing) from the box kernel of the direction-by-direction product.  Cause: a window of nodes that ends
    inside an element of a C^0 direction reaches more functions than it has nodes, so the box after the contraction is LARGER
    than before it, and the "touched" flags of the second LDS buffer were carved for the smaller one -- the flags of the
    tail fell off the end of the LDS allocation (csrc/tg_ptap_box.hip, ``cap1 > cap``).  Fixed there; the cases stay."""
    cases = [{"d": 3, "ps": [3, 3, 3], "kinds": ["drop", "drop", "nonuniform"], "nels": [7, 2, 3], "drops": [2, 1, 0], "nfields": 2,
              "knot_seed": 885604054, "bc": "none", "diag": 1000.0, "matrix": "random_extra", "val_seed": 919211811,
              "apply_bcs": True},
             {"d": 3, "ps": [3, 3, 3], "kinds": ["uniform", "nonuniform", "drop"], "nels": [5, 4, 6], "drops": [0, 0, 2], "nfields": 2,
              "knot_seed": 307650820, "bc": "sides2", "diag": 1000.0, "matrix": "random_extra", "val_seed": 681249583,
              "apply_bcs": True}]
    for case in cases:
        for env in ({}, {"TIGAR_IMPLICIT_M": "1"}):
            rc, summary, failures = _run(["--case", json.dumps(case)], env)
            assert rc == 0 and summary["failed"] == 0, "\n".join(failures)[:4000]


@pytest.mark.parametrize("seed,env", [(201, {}), (202, {"TIGAR_PTAP_WAVE": "1"}), (203, {"TIGAR_PTAP_ACCUM": "int"}),
                                      (204, {"TIGAR_POOL_POISON": "1", "TIGAR_KSP_PERSISTENT": "1"}),
                                      (205, {"TIGAR_KSP_PERSISTENT": "1", "TIGAR_KSP_PERSISTENT_WGS": "2"})])
def test_random_sparse_matrices_through_the_kernels(seed, env):
    """`tests/fuzz/fuzz_kernels.py`: matrices of any shape and row-length profile (empty, one row, empty rows, a few rows that fill
    the matrix) through SpMV / M^T b / transpose / add / selections / the general PtAP (structural pattern, values,
    MatZeroRowsColumns, the same bits twice) / the Krylov solvers, against scipy"""
    rc, summary, failures = _run(["--seed", str(seed), "--cases", "25"], env, tool="fuzz_kernels.py")
    assert rc == 0 and summary["failed"] == 0, "\n".join(failures)[:4000]


def test_sequences_of_different_matrices_through_one_spline():
    """`tests/fuzz/fuzz_sequences.py`: eight FE matrices in a row through ONE ExtractedSpline per random patch (Laplace, random
    values, three matrices with the same number of hand-added couplings at different places, Laplace again, mass, the first
    again) -- cached symbolic products, tensor plans, fold plans must never serve a matrix they were not made for; pattern
    (the structural product, also for the hand-added couplings) and values against the oracle.  Found this way: a field block
    that holds only hand-added couplings came back on the full tensor pattern with stored zeros."""
    rc, summary, failures = _run(["--seed", "3", "--cases", "70"], {}, tool="fuzz_sequences.py")
    assert rc == 0 and summary["failed"] == 0, "\n".join(failures)[:4000]


def test_sequences_of_different_matrices_through_the_streamed_field_engine():
    """the same tool with the operator kept implicit: patches with two fields go through the streamed field engine, whose
    blocks off the diagonal hold NOTHING but the three hand-added couplings -- anywhere on the patch.  Until the entries of
    such a block were counted the engine looked at three node planes of it and dropped the block when the couplings sat
    elsewhere; the summary says how many cases put them there."""
    rc, summary, failures = _run(["--seed", "3", "--cases", "12", "--max-dofs", "4000"], {"TIGAR_IMPLICIT_M": "1"},
                                 tool="fuzz_sequences.py")
    assert rc == 0 and summary["failed"] == 0, "\n".join(failures)[:4000]
    assert summary["streamed_couplings_off_the_probed_planes"] >= 3, summary


def test_random_mapped_patches_through_the_assembly():
    """`tests/fuzz/fuzz_assembly.py`: 80 random mapped patches (1-3 parametric in 1-3 physical dimensions, degrees 1-4, rational
    and perturbed maps, non-uniform elements, p+1 / p+2 Gauss points) through the element kernels of csrc/tg_assemble.hip:
    mass, Laplace(-Beltrami), nodal load, and -- where nsd == d -- field blocks of the elasticity form and the biharmonic form
    (round 6), each against its element-loop oracle"""
    rc, summary, failures = _run(["80"], {}, tool="fuzz_assembly.py")
    assert rc == 0 and summary["failed"] == 0, "\n".join(failures)[:4000]


def test_random_spd_band_systems_through_the_direct_solve():
    """`tests/fuzz/fuzz_direct.py` (round 6): random SPD band systems -- sizes the blocks of 32 never divide, half-widths 1 .. 1300,
    bands with holes, 2 .. 64 sweep workgroups or one -- against LAPACK's banded Cholesky, and matrices that are not SPD handed on
    to the LU; once more with the allocator handing out NaNs"""
    for env in ({}, {"TIGAR_POOL_POISON": "1"}):
        rc, summary, failures = _run(["--seed", "11", "--cases", "40"], env, tool="fuzz_direct.py")
        assert rc == 0 and summary["failed"] == 0, "\n".join(failures)[:4000]
