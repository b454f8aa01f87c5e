"""CPU: the partition of FE planes into classes with bit-identical rows of the last-direction Kronecker factor
(tt_plane_classes in tigar_amd/csrc/tg_tensor_body.h, host build: tests/emu/plane_classes_emu.cpp) -- the x and y passes
of the tensor-pattern PtAP contract one plane per class.  Checked against a plain Python grouping of the rows by
(length, bytes of every term)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tigar_amd.forms import fe_matrices_1d

HERE = os.path.dirname(os.path.abspath(__file__))
c_f64p, c_i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def emu():
    build = os.path.join(HERE, "emu", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libplane_classes_emu.so")
    src = os.path.join(HERE, "emu", "plane_classes_emu.cpp")
    hdr = os.path.join(HERE, "..", "tigar_amd", "csrc", "tg_tensor_body.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", src, "-o", so])
    lib = C.CDLL(so)
    lib.emu_plane_classes.restype = C.c_int
    lib.emu_plane_classes.argtypes = [C.c_int, C.c_int64, c_f64p, c_i32p, C.c_int, C.c_int, c_i32p]
    return lib


def _factor_terms(p, nel, nterms=3):
    """(rps, [values of term 0, 1, ...]) of the last-direction factor of LaplaceForm on nel uniform elements of [0, 1]:
    mass, mass, stiffness (one term: mass; two: mass, stiffness)"""
    h = 1.0 / float(nel)
    Mm, Km = fe_matrices_1d([0.0 + float(i) * h for i in range(nel + 1)], p)
    assert np.array_equal(Mm.indptr, Km.indptr) and np.array_equal(Mm.indices, Km.indices)
    terms = {1: [Mm], 2: [Mm, Km], 3: [Mm, Mm, Km]}[nterms]
    return Mm.indptr.astype(np.int32), [np.array(t.data, dtype=np.float64) for t in terms]


def _partition(emu, rps, terms, z0=0, z1=None):
    z1 = len(rps) - 1 if z1 is None else z1
    val = np.ascontiguousarray(np.concatenate(terms))
    rep = np.full(z1 - z0, -7, dtype=np.int32)
    n = emu.emu_plane_classes(len(terms), int(rps[-1]), val.ctypes.data_as(c_f64p), rps.ctypes.data_as(c_i32p),
                              z0, z1, rep.ctypes.data_as(c_i32p))
    return n, rep


def _python_partition(rps, terms, z0=0, z1=None):
    z1 = len(rps) - 1 if z1 is None else z1
    first, rep = {}, []
    for q in range(z0, z1):
        key = (int(rps[q + 1] - rps[q]),) + tuple(t[rps[q]:rps[q + 1]].tobytes() for t in terms)
        rep.append(first.setdefault(key, q))
    return len(first), np.array(rep, dtype=np.int32)


@pytest.mark.parametrize("p,nel,nclasses", [(3, 8, 5), (2, 6, 11), (3, 10, 16), (4, 16, 6)])
def test_partition_of_the_laplace_factors_is_the_grouping_by_length_and_bytes(emu, p, nel, nclasses):
    rps, terms = _factor_terms(p, nel)
    n, rep = _partition(emu, rps, terms)
    n_py, rep_py = _python_partition(rps, terms)
    assert n == n_py and np.array_equal(rep, rep_py)
    assert n == len(set(rep.tolist())) == nclasses
    # a representative is the lowest plane of its class and represents itself
    assert np.all(rep <= np.arange(len(rep))) and np.all(rep[rep] == rep)


@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_one_two_and_three_terms(emu, nterms):
    rps, terms = _factor_terms(3, 8, nterms)
    n, rep = _partition(emu, rps, terms)
    n_py, rep_py = _python_partition(rps, terms)
    assert n == n_py == 5 and np.array_equal(rep, rep_py)
    # a difference in the LAST term alone separates two planes
    q = 10                                                      # an interior node of element 3
    terms[-1] = terms[-1].copy()
    terms[-1][rps[q] + 1] = np.nextafter(terms[-1][rps[q] + 1], np.inf)
    n2, rep2 = _partition(emu, rps, terms)
    assert n2 == 6 and rep2[q] == q and np.array_equal(np.delete(rep2, q), np.delete(rep, q))


def test_a_row_moved_by_one_ulp_in_one_term_leaves_its_class(emu):
    rps, terms = _factor_terms(3, 8)
    _, rep = _partition(emu, rps, terms)
    for q, term in ((9, 0), (11, 1), (13, 2)):                  # a vertex and two interior nodes, one term each
        assert rep[q] != q                                      # shares a lower plane's blocks before the change
        moved = [t.copy() for t in terms]
        j = rps[q] + 2
        moved[term][j] = np.nextafter(moved[term][j], -np.inf)
        n, rep_m = _partition(emu, rps, moved)
        assert n == 6 and rep_m[q] == q
        assert np.array_equal(np.delete(rep_m, q), np.delete(rep, q))
        assert np.array_equal(rep_m, _python_partition(rps, moved)[1])


def test_negative_zero_is_not_merged_with_zero_and_equal_nans_are(emu):
    rps, terms = _factor_terms(2, 6, 1)
    rps = rps.copy()
    val = np.zeros_like(terms[0])                               # every row zero: classes by length only
    n, rep = _partition(emu, rps, [val])
    assert n == 2
    q = 5                                                       # an interior node (length p + 1), not the lowest of its class
    assert rep[q] != q
    val[rps[q] + 1] = -0.0
    assert val[rps[q] + 1] == 0.0
    n, rep = _partition(emu, rps, [val])
    assert n == 3 and rep[q] == q
    # two rows with the same NaN payload at the same place are one class
    val[rps[q] + 1] = 0.0
    nan = np.frombuffer(np.uint64(0x7ff8000000000abc).tobytes(), dtype=np.float64)[0]
    val[rps[3] + 2] = nan
    val[rps[7] + 2] = nan
    n, rep = _partition(emu, rps, [val])
    assert n == 3 and rep[7] == 3 and rep[3] == 3 and rep[q] != q


def test_a_range_inside_the_grid_picks_its_representatives_inside_the_range(emu):
    rps, terms = _factor_terms(3, 8)
    nfe = len(rps) - 1
    for z0, z1 in ((7, 19), (10, 11), (4, nfe), (12, 14)):
        n, rep = _partition(emu, rps, terms, z0, z1)
        n_py, rep_py = _python_partition(rps, terms, z0, z1)
        assert n == n_py and np.array_equal(rep, rep_py)
        assert rep.min() >= z0 and rep.max() < z1
        assert np.all(rep <= np.arange(z0, z1)) and np.all(rep[rep - z0] == rep)
    # planes 7..18 of p = 3: vertices 9, 12, 15, 18 and the two kinds of interior node
    n, rep = _partition(emu, rps, terms, 7, 19)
    assert n == 3 and sorted(set(rep.tolist())) == [7, 8, 9]
