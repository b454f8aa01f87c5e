"""The CPU helper of the wave-per-row PtAP tests (tests/ptap_wave_reference.py) and the premises of the inputs it builds: what
tests/test_gpu_ptap_wave.py takes for granted about its operands is asserted here, without a GPU."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import ptap_wave_reference as R


def test_unmix_inverts_mix():
    rng = np.random.default_rng(0)
    sample = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1] + [int(x) for x in rng.integers(0, 2 ** 32, size=2000)]
    for x in sample:
        assert R.gw_unmix(R.gw_mix(x)) == x
    assert len({R.gw_mix(x) for x in range(5000)}) == 5000
    assert R.gw_mix(817077582) == R.U32          # the one column whose mixed key is the empty marker (out of the tests' reach)


def test_seed_sequence_and_slots():
    s1 = 0x9E3779B9
    s2 = (s1 * 0x2545F491 + 0x9E3779B9) & R.U32
    s3 = (s2 * 0x2545F491 + 0x9E3779B9) & R.U32
    assert [R.gw_seed(a) for a in range(4)] == [0, s1, s2, s3] and len({0, s1, s2, s3}) == 4
    assert R.gw_reseed(R.gw_mix(3), s1) != R.gw_mix(3)
    for ts in (64, 128, 1024):
        for c in (0, 3, 4000, 2 ** 31 - 1):
            for attempt in range(4):
                s1, s2 = R.gw_slots(c, attempt, ts)
                assert 0 <= s1 < ts // 2 <= s2 < ts
    assert [R.gw_lg_group(m) for m in (1, 8, 10.6, 10.7, 12, 24, 42.6, 42.7, 48, 100, 1000)] == [3, 3, 3, 4, 4, 5, 5, 6, 6, 6, 6]
    assert [R.gw_table_size(n) for n in (0, 12, 24, 25, 300)] == [64, 64, 64, 128, 1024]


# ---- the tile-ordered row schedule
HINTS = [((5, 7, 3), (2, 3, 2)), ((5, 7, 3), (9, 9, 9))]          # the hints of the GPU test: tiles neither divide nor fit


def test_tile_row_is_a_bijection():
    tiles = np.array(list(itertools.product(range(1, 8), repeat=3)), dtype=np.int64)
    t0, t1, t2 = (tiles[:, k:k + 1] for k in range(3))
    for n in itertools.product(range(1, 7), repeat=3):
        total = n[0] * n[1] * n[2]
        rows = R.gw_tile_row(np.arange(total, dtype=np.int64)[None, :], n[0], n[1], n[2], t0, t1, t2)
        assert np.array_equal(np.sort(rows, axis=1), np.broadcast_to(np.arange(total), rows.shape)), n
    for n, t in HINTS:
        total = n[0] * n[1] * n[2]
        rows = [int(R.gw_tile_row(i, *n, *t)) for i in range(total)]
        assert sorted(rows) == list(range(total)), (n, t)


def test_tile_row_keeps_tiles_together():
    """not only a bijection: the first t0 t1 t2 indices are the points of the first tile"""
    n, t = (6, 5, 4), (2, 3, 2)
    first = {R.gw_tile_row(i, *n, *t) for i in range(12)}
    assert first == {x + n[0] * (y + n[1] * z) for x in range(2) for y in range(3) for z in range(2)}


# ---- placeable
def _brute(columns, attempt, ts):
    slots = [R.gw_slots(c, attempt, ts) for c in columns]
    return any(len(set(pick)) == len(pick) for pick in itertools.product(*slots))


def test_placeable_against_brute_force():
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(1500):
        k = int(rng.integers(1, 7))
        cols = [int(c) for c in rng.choice(40, size=k, replace=False)]
        attempt = int(rng.integers(0, 4))
        got = R.placeable(cols, attempt, 8)
        assert got == (_brute(cols, attempt, 8) and k <= 4), (cols, attempt)
        seen.add((got, k <= 4))
    assert {(True, True), (False, True), (False, False)} <= seen      # both answers occur among the sets that fit


# ---- the committed key lists of the re-hash cases
def test_rehash_triple_and_row_premises():
    t = R.REHASH_TRIPLE
    assert len({R.gw_slots(c, 0, 64) for c in t}) == 1
    assert not R.placeable(t, 0, 64) and R.placeable(t, 1, 64)
    # the 12-key row re-derived: for every attempt a, the three smallest columns that share both slots with column a
    derived = []
    for a in range(4):
        want = R.gw_slots(a, a, 64)
        derived += [c for c in range(4000) if R.gw_slots(c, a, 64) == want][:3]
    assert derived == R.REHASH_ROW
    for a in range(4):
        assert not R.placeable(R.REHASH_ROW, a, 64)
    assert R.placeable(R.REHASH_ROW, 0, 128)


@pytest.mark.parametrize("which", ["a", "b"])
def test_rehash_operands_premises(which):
    M, A, row = R.rehash_operands(R.exact_value_source(7), which)
    S, AM = R.structural(M, A)
    assert np.array_equal(S.indices, A.indices) and np.array_equal(AM.indices, A.indices)      # M is diagonal
    longest = int(np.diff(A.indptr).max())
    ts = R.gw_table_size(longest)
    assert ts == 64
    assert A.shape[0] > 64                                             # more than one workgroup in either stage
    for i, cols in enumerate(R.rows_of(A)):
        if i != row:
            assert R.placeable(cols, 0, 64) and R.placeable(cols, 0, 128)
    cols = R.rows_of(A)[row]
    if which == "a":
        assert not R.placeable(cols, 0, 64) and R.placeable(cols, 1, 64)
    else:
        assert not any(R.placeable(cols, a, 64) for a in range(4)) and R.placeable(cols, 0, 128)


# ---- the operand sets
def test_lane_group_operands_have_the_prescribed_lengths():
    inner, outer = R.lane_group_lengths()
    for G in (8, 16, 32, 64):
        assert {0, 1, G - 1, G, G + 1, 2 * G + 1, 64, 65, 129} <= set(inner)
        for U in R.GW_U:
            n = U * (64 // G)
            assert {0, 1, n - 1, n, n + 1, 63, 64, 65, 130} <= set(outer)
    M, A, info = R.lane_group_operands(R.exact_value_source(1))
    S, AM = R.structural(M, A)
    lm, la, lam = np.diff(M.indptr), np.diff(A.indptr), np.diff(AM.indptr)
    lc = np.diff(M.T.tocsr().indptr)
    assert [lm[info["m_rows"][L]] for L in inner] == inner
    assert [lam[info["am_rows"][L]] for L in inner] == inner
    assert [lc[info["m_cols"][L]] for L in outer] == outer
    assert la[0] == 0 and all(la[r] == L for L, r in info["a_rows"].items()) and set(info["a_rows"]) == set(outer) - {0, 1}
    # every designated row of A M is an operand row of the second stage: its FE row has entries in M
    assert all(lm[r] > 0 for r in info["am_rows"].values())
    # the empty row of M is referred to by rows of A, the empty row of A M by columns of M
    assert (A.tocsc()[:, info["m_rows"][0]]).nnz >= 2
    i = info["no_diagonal_dof"]
    assert S[i].nnz > 0 and S[i, i] == 0
    # ragged: the rule drops the stride in both stages
    lk = np.diff(S.indptr)
    assert not R.gw_strided(lam.max(), lam.mean()) and not R.gw_strided(lk.max(), lk.mean())
    assert R.gw_table_size(lam.max()) <= 2048 and R.gw_table_size(lk.max()) <= 2048
    # the floating set has the same structure
    Mf, Af, _ = R.lane_group_operands(R.normal_values(2), row_scale=R.decade_row_scale)
    assert np.array_equal(Mf.indices, M.indices) and np.array_equal(Af.indices, A.indices)
    scale = abs(Af).max(axis=1).toarray().ravel()
    assert scale[scale > 0].max() / scale[scale > 0].min() > 1e9


@pytest.mark.parametrize("L,lg", [(8, 3), (12, 4), (24, 5), (48, 6), (100, 6)])
def test_uniform_operands(L, lg):
    M, A = R.uniform_operands(L, R.exact_value_source(L))
    S, AM = R.structural(M, A)
    assert set(np.diff(M.indptr)) == {L} and set(np.diff(AM.indptr)) == {L}
    assert R.gw_lg_group(L) == lg
    lk = np.diff(S.indptr)
    assert R.gw_strided(L, L) and R.gw_strided(lk.max(), lk.mean())      # the rule keeps the stride in both stages


def test_exact_reference_is_exact_in_any_order():
    M, A, info = R.lane_group_operands(R.exact_value_source(1))
    S, data = R.exact_reference(M, A)
    K = (M.T.tocsr() @ (A @ M)).tocsr()
    assert np.array_equal(R._on_pattern(S, K), data)
    K2 = ((M.T.tocsr() @ A) @ M).tocsr()
    assert np.array_equal(R._on_pattern(S, K2), data)
    with pytest.raises(AssertionError):
        R.exact_reference(M * 2.0 ** 20, A)                              # the budget is asserted


def test_zero_dofs_of_the_reference():
    M, A, info = R.lane_group_operands(R.exact_value_source(1))
    nd = info["no_diagonal_dof"]
    S, _ = R.structural(M, A)
    zd = R.lane_group_zero_dofs(S, info)
    assert len(set(zd)) == 3 and zd[2] == nd
    S, data = R.exact_reference(M, A, zd, 2.5)
    K = sp.csr_matrix((data, S.indices, S.indptr), shape=S.shape)
    assert S[zd[0], zd[0]] > 0 and K[zd[0], zd[0]] == 2.5 and K[zd[1], zd[1]] == 2.5
    assert S[zd[0]].nnz > 1 and S[zd[1]].nnz > 1
    for i in zd:
        assert abs(K[i]).sum() == (2.5 if i != nd else 0.0) and abs(K[:, i]).sum() == (2.5 if i != nd else 0.0)
    _, plain = R.exact_reference(M, A)
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    untouched = ~np.isin(rows, zd) & ~np.isin(S.indices, zd)
    assert np.array_equal(plain[untouched], data[untouched])


def test_float_bound_holds_for_scipy_and_catches_a_dropped_term():
    M, A = R.random_operands(60, R.normal_values(4), 4)
    A = (sp.diags(R.decade_row_scale(np.random.default_rng(4), 60)) @ A).tocsr()
    S, ref, bound = R.float_reference(M, A)
    K = R._on_pattern(S, (M.T.tocsr() @ (A @ M)).tocsr())
    assert R.bound_ratio(K, ref, bound) <= 1.0
    # the smallest triple term of an entry with several terms, dropped: far outside the bound, inside 1e-12 max|K|
    Md, Ad = M.toarray(), A.toarray()
    i, j = np.unravel_index(np.argmax(S.toarray()), S.shape)
    terms = [Md[r, i] * Ad[r, s] * Md[s, j] for r in range(60) for s in range(60) if Md[r, i] and Ad[r, s] and Md[s, j]]
    assert len(terms) == S[i, j] >= 2
    small = min(terms, key=abs)
    at = S.indptr[i] + list(S.indices[S.indptr[i]:S.indptr[i + 1]]).index(j)
    K2 = K.copy()
    K2[at] -= small
    assert R.bound_ratio(K2, ref, bound) > 1.0


def test_block_rows_cover_what_they_refer_to():
    M, A = R.banded_operands(R.exact_value_source(5))
    (a0, a1), (m0, m1) = R.block_rows(M, A, 100, 180)
    assert 0 < a0 < a1 < 400 and 0 < m0 < m1 < 400
    MT = M.T.tocsr()[100:180]
    assert MT.indices.min() >= a0 and MT.indices.max() < a1
    assert A[a0:a1].indices.min() >= m0 and A[a0:a1].indices.max() < m1
    S, data = R.exact_reference(M, A)
    # the rows of the block's product are the rows of the whole product
    Kb = (MT[:, a0:a1] @ A[a0:a1][:, m0:m1] @ M[m0:m1]).tocsr()
    K = sp.csr_matrix((data, S.indices, S.indptr), shape=S.shape)
    assert abs(Kb - K[100:180]).max() == 0
