"""Fields coupled on a FEW nodes through the streamed field engines (TIGAR_IMPLICIT_M=1: ``dist.FieldSlabPath`` for several
fields on one basis, ``dist.FieldListSlabPath`` for fields on different bases).  ``extractMatrix(A)`` is M^T A M for ANY
assembled A (tIGAr/common.py:1194-1200) -- also when a block A_fg holds one entry, or the rows of two node planes: a
constraint, a penalty or a contact term added by hand.  The engines form the product block by block and skip the blocks
they judge empty; that judgement is what these cases are about (``dist._block_is_empty``: until now three node planes of the
rows were looked at, for explicit matrices too).

Reference: plain scipy in float64 on the same inputs (``oracle.extract_matrix``), rows and columns renumbered by
``localDofIndices()``; pattern identical, values to 1e-12 of the largest entry (the project's bound for this product).
Every case first shows on the host that K without the off-diagonal blocks is further away than 1e-6: a dropped block
cannot pass.

Also here: ``dist._ChunkRows`` (the carried rows of the element chunks) with chunks that overlap, and in the wrong order."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import tigar_oracle as O  # noqa: E402

KINDS = ["a", "b", "c", "d", "e", "f"]
_REF = {}


def _reference(space, kind):
    """(A, Ko, Ko without the couplings, zero dofs) in the reference numbering; computed once per case, on the resident path's
    inputs (the FE matrix is assembled by the forms, M comes from the oracle -- for the RT space, whose M the oracle's tensor
    routine does not make, from the resident spline, which the kernel tests pin to the oracle bit for bit)"""
    if (space, kind) not in _REF:
        import gpu_rank_worker_fields as W
        from tigar_amd import common as tc
        assert os.environ.get("TIGAR_IMPLICIT_M") is None
        gen, spline, A, A0 = W.coupled_space(space, kind, tc.selfcomm)
        assert not getattr(gen.M, "is_implicit", False)
        if space == "rt3d":
            Mo = gen.M.to_scipy().tocsr()
        else:
            d, p, nels = (3, 2, [3, 3, 8]) if space == "eq3d" else (2, 3, [4, 9])
            Mo = O.generate_M_tensor(O.BSpline([p] * d, [O.uniform_knots(p, 0., 1., n) for n in nels]), nfields=2)
        zd = [int(i) for i in spline.zeroDofs]
        assert len(zd) > 0
        Ko, K0 = (O.extract_matrix(Mo, X, zd, diag=1.5).tocsr() for X in (A, A0))
        _REF[(space, kind)] = (A, Ko, K0, zd)
    return _REF[(space, kind)]


def _check(space, kind, monkeypatch, env=None, after=None):
    import gpu_rank_worker_fields as W
    from tigar_amd import common as tc, device as dev
    A, Ko, K0, zd = _reference(space, kind)
    scale = abs(Ko).max()
    sep = abs(Ko - K0).max() / scale
    print("%s %s: %d entries in the couplings, K without them differs by %.3e" % (space, kind, A.nnz - _diag_nnz(A, space), sep))
    if kind != "f":
        assert sep > 1e-6, "the case cannot tell a dropped block: %g" % sep
    monkeypatch.setenv("TIGAR_IMPLICIT_M", "1")
    for k_, v_ in (env or {}).items():
        monkeypatch.setenv(k_, v_)
    gen, spline, A2, _ = W.coupled_space(space, kind, tc.selfcomm)
    assert getattr(gen.M, "is_implicit", False) and gen.M.nfields == (3 if space == "rt3d" else 2)
    assert (A2 != A).nnz == 0 and [int(i) for i in spline.zeroDofs] == zd
    idx = np.asarray(spline.localDofIndices(), dtype=np.int64)
    assert np.array_equal(np.sort(idx), np.arange(Ko.shape[0])) and not np.array_equal(idx, np.arange(Ko.shape[0]))
    Kr = Ko[idx][:, idx].tocsr()
    Kr.sort_indices()
    for how, A_in in (("scipy", A), ("DeviceCSR", dev.DeviceCSR.from_scipy(A))):
        dev.prof_reset()
        K = spline.extractMatrix(A_in, diag=1.5).to_scipy().tocsr()
        K.sort_indices()
        assert K.shape == Kr.shape
        err = abs(K - Kr).max() / scale
        print("  %s: nnz %d (reference %d), error %.3e" % (how, K.nnz, Kr.nnz, err))
        assert np.array_equal(K.indptr, Kr.indptr) and np.array_equal(K.indices, Kr.indices), \
            "%s: pattern of K (nnz %d, reference %d)" % (how, K.nnz, Kr.nnz)
        assert err <= 1e-12, "%s: values of K: %g" % (how, err)
        if after is not None:
            after(spline, dev)


def _diag_nnz(A, space):
    nF = 3 if space == "rt3d" else 2
    n = A.shape[0] // nF
    return sum(A[f * n:(f + 1) * n, f * n:(f + 1) * n].nnz for f in range(nF))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("space", ["eq3d", "eq2d", "rt3d"])
def test_fields_coupled_on_a_few_nodes(space, kind, monkeypatch):
    """a to d: couplings off the first, the middle and the last node plane (lost until the emptiness of a block of an
    explicit matrix was counted); e: on those planes only (the control, right before too); f: no couplings"""
    _check(space, kind, monkeypatch)


@pytest.mark.parametrize("kind", ["b", "c"])
def test_fields_coupled_on_a_few_nodes_in_sub_slabs_of_two_planes(kind, monkeypatch):
    def streamed(spline, dev):
        assert len(spline._slab_path().scalar.sub_slabs()) >= 3
    _check("eq3d", kind, monkeypatch, {"TIGAR_SUB_PLANES": "2"}, streamed)


@pytest.mark.parametrize("kind", ["b", "c"])
def test_fields_coupled_on_a_few_nodes_in_one_pass_over_element_chunks(kind, monkeypatch):
    """nothing assumed about M or A (no tensor passes, no Kronecker factors): ONE pass over chunks of two element layers is
    offered all coupled blocks -- four in case c, three in case b: the couplings are among them, not dropped.  The pass
    writes K on the pattern of the cells, the structural product only for a block that holds the whole element-coupling
    pattern: it declines these (until it compared the entry counts, case c came back with 23826 stored zeros), the
    diagonal blocks go through chunks of their own and the couplings through the row-wise stages."""
    from tigar_amd import dist
    calls, added = [], []
    inner, inner_add = dist.SlabHotPath.assemble_blocks_by_elements, dist._ChunkRows.add_chunk

    def spy(self, producers, timers=None):
        del added[:]
        out = inner(self, producers, timers)
        calls.append((len(producers), out is not None, len(added)))
        return out

    def spy_add(self, Kc, d0, d1, done_row):
        added.append((d0, d1))
        return inner_add(self, Kc, d0, d1, done_row)
    monkeypatch.setattr(dist.SlabHotPath, "assemble_blocks_by_elements", spy)
    monkeypatch.setattr(dist._ChunkRows, "add_chunk", spy_add)

    seen = []

    def chunked(spline, dev):
        # (producers, result, chunks added) of every pass: ONE pass is offered all coupled blocks and declines in its first
        # chunk, at the first block that is not the whole pattern; then block by block -- the diagonal blocks in four chunks of two element layers,
        # the couplings declined again and formed by the row-wise stages
        few = (1, False, 0)
        want = [(4, False, 1), (1, True, 4), few, few, (1, True, 4)] if kind == "c" else [(3, False, 1), (1, True, 4), few, (1, True, 4)]
        assert [c[:len(w)] for c, w in zip(calls, want)] == want and len(calls) == len(want), calls
        seen.append(len(calls))
        del calls[:]
    _check("eq3d", kind, monkeypatch, {"TIGAR_PTAP_TENSOR": "0", "TIGAR_PTAP_FACTORED": "0", "TIGAR_PTAP_ELEMENTS": "2",
                                       "TIGAR_ELEM_LAYERS": "2"}, chunked)
    assert len(seen) == 2                        # (once for the scipy matrix, once for the DeviceCSR)


# ---- the carried rows of the element chunks ---------------------------------------------------------------------------
def _chunk(rng, d0, d1, ncols):
    Kc = sp.random(d1 - d0, ncols, density=0.3, random_state=rng, format="csr")
    Kc.data = rng.uniform(1.0, 2.0, Kc.nnz)
    return Kc


def test_overlapping_chunks_in_order_add_up():
    """rows [0, 14) of a rank from three chunks that overlap by the rows the next chunk still adds to (dof planes of 2 rows):
    the sum of the chunks, pattern and values, against scipy"""
    from tigar_amd import device as dev, dist
    rng = np.random.default_rng(17)
    ncols, g0, g1 = 9, 0, 14
    chunks = [(0, 6, 4), (4, 11, 8), (8, 14, 14)]            # (d0, d1, rows below this are final after the chunk)
    acc = dist._ChunkRows(dev, g0, g1, ncols, 2)
    want = sp.csr_matrix((g1 - g0, ncols))
    for d0, d1, done in chunks:
        Kc = _chunk(rng, d0, d1, ncols)
        want = want + sp.vstack([sp.csr_matrix((d0, ncols)), Kc, sp.csr_matrix((g1 - d1, ncols))]).tocsr()
        acc.add_chunk(dev.DeviceCSR.from_scipy(Kc), d0, d1, done)
    K = acc.finish().to_scipy().tocsr()
    K.sort_indices()
    want.sort_indices()
    assert K.shape == want.shape
    assert np.array_equal(K.indptr, want.indptr) and np.array_equal(K.indices, want.indices)
    assert abs(K - want).max() <= 4e-16 * abs(want).max()      # (one addition per entry)


def test_a_chunk_that_starts_below_the_carried_rows_is_an_error():
    """the rows [d0, pend0) of such a chunk were dropped without a word: rows 2 .. 4 here, final after the first chunk"""
    from tigar_amd import device as dev, dist
    rng = np.random.default_rng(18)
    ncols = 9
    acc = dist._ChunkRows(dev, 0, 14, ncols, 2)
    acc.add_chunk(dev.DeviceCSR.from_scipy(_chunk(rng, 0, 8, ncols)), 0, 8, 4)
    with pytest.raises(RuntimeError, match=r"rows 2 \.\. 4 of a chunk arrive after the rows below 4 were final"):
        acc.add_chunk(dev.DeviceCSR.from_scipy(_chunk(rng, 2, 10, ncols)), 2, 10, 8)
