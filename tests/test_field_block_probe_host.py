"""CPU: which field blocks of an FE matrix the streamed / distributed field engines treat as "not coupled"
(``dist._block_is_empty``, asked by ``FieldSlabPath.assemble_matrix`` and ``FieldListSlabPath.assemble_matrix`` before they
form M_f^T A_fg M_g).  ``extractMatrix`` promises M^T A M for ANY assembled A (tIGAr/common.py:1194-1200): a block that holds
one entry -- a constraint, a penalty or a contact term between two fields on a few nodes -- is coupled, wherever the entry
sits.  Only producers that declare "structurally empty or populated on every node plane" (the blocks of an assembled form)
are judged by three planes, and those must not be asked for more."""
import numpy as np
import pytest
import scipy.sparse as sp

from tigar_amd import dist


def _layout(p, nel_z, plane_fe, plane_dofs):
    """slab arithmetic of the last direction: open uniform knots, CG degree-p nodes"""
    knots = np.concatenate([np.zeros(p), np.linspace(0.0, 1.0, nel_z + 1), np.ones(p)])
    nodes = np.linspace(0.0, 1.0, p * nel_z + 1)
    return dist.ZSlabLayout(knots, p, nodes, p, plane_dofs, plane_fe)


# (name, plane_fe, node planes, layout): 3-D p = 2 on 3 x 3 x 8 elements, 2-D p = 3 on 4 x 9 elements
GRIDS = [("3d", 49, 17, _layout(2, 8, 49, 25)), ("2d", 13, 28, _layout(3, 9, 13, 7))]


def _row_ranges(lay):
    """FE rows of the whole patch, and of rank 1 of 2 (``SlabHotPath.mine["a_rows"]``)"""
    whole = lay.slab(0, lay.ncp)["a_rows"]
    k0, k1 = dist.split_range(lay.ncp, 2)[1]
    return [("whole", whole), ("rank1of2", lay.slab(k0, k1)["a_rows"])]


CASES = [(name, pf, nz, who, ar) for name, pf, nz, lay in GRIDS for who, ar in _row_ranges(lay)]
IDS = ["%s-%s" % (c[0], c[3]) for c in CASES]


class Producer(object):
    """``a_block`` over a scipy block (0, 1) of one field's rows x one field's columns; every other block is empty"""

    def __init__(self, B01):
        self.B, self.asked = sp.csr_matrix(B01), []

    def __call__(self, f, g, r0, r1):
        self.asked.append((int(r0), int(r1)))
        if (f, g) == (0, 1):
            return self.B[int(r0):int(r1)]
        return sp.csr_matrix((int(r1) - int(r0), self.B.shape[1]))


def _one_entry(n, pf, k, col_plane):
    """one entry of block (0, 1): a node in the middle of plane k coupled to one of plane ``col_plane``"""
    return sp.csr_matrix(([1.5], ([k * pf + pf // 2], [col_plane * pf + pf // 3])), shape=(n, n))


def _explicit(B01, mode):
    """the producer as ``ExtractedSpline._block_producer`` makes it for an explicit two-field matrix (counted on the host),
    or one that declares nothing"""
    P = Producer(B01)
    if mode == "counted":
        from tigar_amd.common import ExtractedSpline
        n = B01.shape[0]
        A = sp.bmat([[sp.identity(n), B01], [None, sp.identity(n)]], format="csr")
        P.is_empty = ExtractedSpline._explicit_block_is_empty(A, n)
    return P


def test_rank_one_of_two_is_inside_the_patch():
    # (the cases below mean something only if rank 1's rows are a proper part of the planes)
    for name, pf, nz, who, ar in CASES:
        assert ar[0] % pf == 0 and ar[1] % pf == 0
        if who == "whole":
            assert (ar[0], ar[1]) == (0, nz * pf)
        else:
            assert 0 < ar[0] < ar[1] == nz * pf and (ar[1] - ar[0]) // pf >= 5


@pytest.mark.parametrize("mode", ["undeclared", "counted"])
@pytest.mark.parametrize("name,pf,nz,who,ar", CASES, ids=IDS)
def test_one_entry_on_any_plane_is_a_coupling(name, pf, nz, who, ar, mode):
    n = nz * pf
    for k in range(ar[0] // pf, ar[1] // pf):
        for col_plane in (k, (k + nz // 2) % nz):
            P = _explicit(_one_entry(n, pf, k, col_plane), mode)
            assert not dist._block_is_empty(P, 0, 1, ar, pf, None), "entry on plane %d reported as no coupling" % k
            assert dist._block_is_empty(P, 1, 0, ar, pf, None)
    # an entry on the rows of the OTHER rank is no coupling on these
    if ar[0] > 0:
        P = _explicit(_one_entry(n, pf, ar[0] // pf - 1, 0), mode)
        assert dist._block_is_empty(P, 0, 1, ar, pf, None)


@pytest.mark.parametrize("mode", ["undeclared", "counted"])
@pytest.mark.parametrize("name,pf,nz,who,ar", CASES, ids=IDS)
def test_a_block_without_entries_is_empty(name, pf, nz, who, ar, mode):
    n = nz * pf
    P = _explicit(sp.csr_matrix((n, n)), mode)
    assert dist._block_is_empty(P, 0, 1, ar, pf, None)
    if mode == "undeclared":
        # nothing declared: every row of the rank was looked at, once, in pieces
        assert P.asked[0][0] == ar[0] and P.asked[-1][1] == ar[1]
        assert all(a[1] == b[0] for a, b in zip(P.asked, P.asked[1:]))
    else:
        assert P.asked == []                     # (counted where the matrix is: nothing cut out for the question)


@pytest.mark.parametrize("name,pf,nz,who,ar", CASES, ids=IDS)
def test_a_producer_that_returns_none_is_empty(name, pf, nz, who, ar):
    for declare in (False, True):
        asked = []

        def none(f, g, r0, r1):
            asked.append((r0, r1))
            return None
        if declare:
            dist.populates_every_plane(none)
        assert dist._block_is_empty(none, 0, 1, ar, pf, None)
        assert len(asked) == 1
    assert dist._block_is_empty(lambda f, g, r0, r1: None, 0, 1, (ar[0], ar[0]), pf, None)       # (a rank without rows)


@pytest.mark.parametrize("name,pf,nz,who,ar", CASES, ids=IDS)
def test_a_block_with_a_kronecker_factor_is_asked_for_one_row(name, pf, nz, who, ar):
    n = nz * pf
    P = Producer(sp.csr_matrix((n, n)))           # (no entry in that row: the factor decides, not the row)
    assert not dist._block_is_empty(P, 0, 1, ar, pf, object())
    assert P.asked == [(ar[0], ar[0] + 1)]
    asked = []

    def none(f, g, r0, r1):
        asked.append((r0, r1))
        return None
    assert dist._block_is_empty(none, 0, 1, ar, pf, object())
    assert asked == [(ar[0], ar[0] + 1)]


@pytest.mark.parametrize("p,nels", [(2, [3, 3, 8]), (3, [4, 9]), (1, [5]), (2, [1, 2, 1])])
def test_entry_count_of_the_element_coupling_pattern(p, nels):
    """what the one pass over element chunks compares the rows of a block with before it writes K on the pattern of the
    cells: the count of the whole element-coupling pattern, here against the assembled Laplace matrix of the oracle"""
    from oracle import tigar_oracle as O
    so = O.BSpline([p] * len(nels), [O.uniform_knots(p, 0., 1., n) for n in nels])
    A = O.poisson_fe_system(so, degree=p)[0].tocsr()
    shape = [p * n + 1 for n in nels]
    pf = int(np.prod(shape[:-1]))
    for za, zb in [(0, shape[-1]), (0, 1), (1, shape[-1] - 1), (shape[-1] - 1, shape[-1]), (2, 2)]:
        if 0 <= za <= zb <= shape[-1]:
            assert dist.element_pattern_nnz(shape, p, za, zb) == A[za * pf:zb * pf].nnz, (za, zb)


@pytest.mark.parametrize("name,pf,nz,who,ar", CASES, ids=IDS)
def test_a_form_driven_producer_is_asked_for_three_planes_at_most(name, pf, nz, who, ar):
    """the blocks of an assembled form: structurally empty or populated on every plane, and declared so -- the question
    costs three planes of assembly, never the rank's whole row block"""
    n = nz * pf
    full = sp.csr_matrix(np.ones((n, 1))) @ sp.csr_matrix(np.ones((1, 3)))
    full = sp.hstack([full, sp.csr_matrix((n, n - 3))], format="csr")
    for B, want in ((full, False), (sp.csr_matrix((n, n)), True)):
        P = dist.populates_every_plane(Producer(B))
        assert dist._block_is_empty(P, 0, 1, ar, pf, None) is want
        assert 1 <= len(P.asked) <= 3
        assert all(ar[0] <= a < b <= ar[1] and b - a <= pf and a % pf == 0 for a, b in P.asked)
        assert sum(b - a for a, b in P.asked) <= 3 * pf
        if want:
            # first, middle and last plane of the rows
            np_ = (ar[1] - ar[0]) // pf
            assert [a for a, _ in P.asked] == [ar[0], ar[0] + (np_ // 2) * pf, ar[1] - pf]
