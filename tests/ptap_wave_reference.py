"""CPU side of tests/test_gpu_ptap_wave.py: references, operand builders and a plain-Python restatement of the table logic
of the wave-per-row PtAP kernels (tigar_amd/csrc/tg_ptap_wave.hip).  Nothing here needs a GPU;
tests/test_ptap_wave_reference_host.py checks this file and the premises of the inputs it builds.

Exact reference
    Operands whose values are small integers times a power of two (``exact_values``: an integer in [-4, 4] \\ {0} times
    2^e, e in [-3, 3]).  Scaled by 2^3 they are integers, K scaled by 2^9 is the int64 product of scipy.  ``exact_reference``
    asserts the budget  max_ij (|M|^T |A| |M|)_ij < 2^53  in units of the smallest term (2^-9): every partial sum of every
    entry, in any order, is then an integer below 2^53 in those units, i.e. a double -- no addition rounds, whatever the
    order, and the device result has to equal the reference bit for bit.  The pattern is the structural product
    ones(M)^T ones(A) ones(M); entries that cancel to zero are stored (as +0.0).

Floating reference and its bound
    ``float_reference``: numpy.longdouble on dense copies.  The kernels form an entry of K as two nested recursive sums in
    double precision (u = 2^-53, no FMA: a product is rounded, then added by an LDS atomic):

        stage 1   B_rj = sum_s  fl(A_rs M_sj)         n1(r, j) terms:  one rounding per product, n1 - 1 per sum
        stage 2   K_ij = sum_r  fl(M_ri B_rj)         n2(i, j) terms:  one rounding per product, n2 - 1 per sum

    (the first addition is 0 + x, exact).  Whatever the order of a sum, a term of it passes through at most n roundings
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), so every triple term M_ri A_rs M_sj of K_ij carries
    a factor prod (1 + d_k), |d_k| <= u, of at most  max_r n1(r, j) + n2(i, j)  factors, and

        |K_ij - exact_ij|  <=  ((1 + u)^q - 1) mag_ij ,     q = max_r n1 + n2 ,     mag = |M|^T |A| |M| .

    T_ij, the number of triple terms of the entry, is sum_r n1(r, j) >= max_r n1 + (n2 - 1), hence q <= T_ij + 1 <= T_ij + 2, and
    (1 + u)^q - 1 <= 1.05 q u for q u < 0.09.  The bound of the tests is therefore

        |K_ij - ref_ij|  <=  1.05 (T_ij + 2) 2^-53 mag_ij ,

    T_ij read from the structural product (its value IS the count).  The reference's own error, (T + 2) 2^-64 mag, is 2^-11 of
    that.  Derived, not measured.

Table logic
    ``gw_mix`` ... ``gw_tile_row`` follow the functions of the same names.  ``placeable`` answers whether a set of columns
    has a cuckoo placement at all: a key is an edge between its two slots, and a placement exists iff no connected component
    of that graph has more edges than vertices (and the keys fit the ts / 2 accumulators).  That does not depend on the
    order of insertion, so the premises of the re-hash cases can be checked here.
"""
import numpy as np
import scipy.sparse as sp

U32 = 0xFFFFFFFF
GW_U = (4, 8)                     # operand rows in flight per lane group, stage 1 / stage 2
LANE_GROUPS = (3, 4, 5, 6)
REHASH_ROW = [0, 1101, 1367, 1, 2171, 2267, 2, 9, 701, 3, 8, 1494]      # one triple per hashing at 64 slots (attempts 0-3)
REHASH_TRIPLE = [3, 6, 12]                                              # share both slots under the plain mix at 64 slots


# ---------------------------------------------------------------------------------------------- table logic
def gw_mix(key):
    m = (key * 0x9E3779B1) & U32
    m ^= m >> 15
    m = (m * 0x85EBCA77) & U32
    m ^= m >> 13
    return m


def gw_unmix(m):
    m ^= m >> 13
    m ^= m >> 26
    m = (m * 0xB6C92F47) & U32
    m ^= m >> 15
    m ^= m >> 30
    return (m * 0x0E8B2F51) & U32


def gw_reseed(m, seed):
    m = ((m ^ seed) * 0xC2B2AE35) & U32
    return m ^ (m >> 16)


def gw_seed(attempt):
    """seed of the `attempt`-th try of a row by a wave that has not re-hashed before (attempt 0: the plain mix)"""
    seed = 0
    for _ in range(attempt):
        seed = (seed * 0x2545F491 + 0x9E3779B9) & U32
    return seed


def gw_s1(m, lgh):
    return m >> (32 - lgh)


def gw_s2(m, lgh, half):
    return half + ((m >> (32 - 2 * lgh)) & (half - 1))


def lg2(v):
    l = 0
    while (1 << l) < v:
        l += 1
    return l


def gw_slots(column, attempt, ts):
    """the two slots of a column in a table of ts slots at the given attempt"""
    half, lgh = ts >> 1, lg2(ts) - 1
    m = gw_mix(int(column))
    if attempt:
        m = gw_reseed(m, gw_seed(attempt))
    return gw_s1(m, lgh), gw_s2(m, lgh, half)


def placeable(columns, attempt, ts):
    """True iff the columns have a cuckoo placement in a table of ts slots at the given attempt (module docstring)"""
    columns = [int(c) for c in columns]
    assert len(set(columns)) == len(columns)
    if len(columns) > ts >> 1:
        return False
    parent = list(range(ts))
    edges = [0] * ts

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    pairs = [gw_slots(c, attempt, ts) for c in columns]
    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    size = [0] * ts
    for s in range(ts):
        size[find(s)] += 1
    for a, _ in pairs:
        edges[find(a)] += 1
    return all(edges[r] <= size[r] for r in range(ts))


def gw_lg_group(mean):
    g = 8
    while g < 64 and g < 0.75 * mean:
        g <<= 1
    return lg2(g)


def gw_table_size(longest, load_inv=2.5):
    """slots the plan gives a wave's table for rows of at most `longest` keys"""
    v, p = int(longest * load_inv) + 4, 1
    while p < v:
        p <<= 1
    return max(64, p)


def gw_strided(longest, mean):
    """the rule by which the rows of a temporary go to a fixed stride (no cursor)"""
    return longest <= 2.0 * mean + 32.0


def gw_tile_row(idx, n0, n1, n2, t0, t1, t2):
    """index in tile-major order -> row; integers or integer arrays that broadcast"""
    slab = t2 * n0 * n1
    tz = idx // slab
    rem = idx - tz * slab
    h = np.minimum(t2, n2 - tz * t2)
    strip = t1 * n0 * h
    ty = rem // strip
    rem -= ty * strip
    w1 = np.minimum(t1, n1 - ty * t1)
    blk = t0 * w1 * h
    tx = rem // blk
    rem -= tx * blk
    w0 = np.minimum(t0, n0 - tx * t0)
    lz = rem // (w0 * w1)
    rem -= lz * w0 * w1
    ly = rem // w0
    lx = rem - ly * w0
    return (tx * t0 + lx) + n0 * ((ty * t1 + ly) + n1 * (tz * t2 + lz))


# ---------------------------------------------------------------------------------------------- references
def ones(X):
    X = sp.csr_matrix(X)
    return sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)


def structural(M, A):
    """S = ones(M)^T ones(A) ones(M), sorted CSR: the pattern of K; S_ij = T_ij, the number of triple terms of the entry.
    Also the pattern of A M (rows of the intermediate)"""
    AM = (ones(A) @ ones(M)).tocsr()
    S = (ones(M).T.tocsr() @ AM).tocsr()
    S.sort_indices()
    AM.sort_indices()
    return S, AM


def _on_pattern(S, X):
    """the values of X on the (sorted) pattern of S, 0 where X has no entry; X's entries lie inside the pattern"""
    X = sp.csr_matrix(X)
    X.sum_duplicates()
    X.sort_indices()
    nc = S.shape[1]
    ks = np.repeat(np.arange(S.shape[0], dtype=np.int64), np.diff(S.indptr)) * nc + S.indices
    kx = np.repeat(np.arange(X.shape[0], dtype=np.int64), np.diff(X.indptr)) * nc + X.indices
    at = np.searchsorted(ks, kx)
    assert np.array_equal(ks[at], kx)
    out = np.zeros(S.nnz, dtype=X.dtype)
    out[at] = X.data
    return out


def apply_zero_dofs(S, data, zero_dofs, diag, row0=0):
    """MatZeroRowsColumns on the entries of the pattern S (rows row0 ... of K): rows and columns of the dofs to zero, `diag`
    on the diagonal WHERE THE PATTERN HAS ONE"""
    data = np.array(data, copy=True)
    if zero_dofs is None or len(zero_dofs) == 0:
        return data
    mask = np.zeros(S.shape[1], dtype=bool)
    mask[np.asarray(zero_dofs)] = True
    rows = np.repeat(np.arange(S.shape[0], dtype=np.int64), np.diff(S.indptr)) + row0
    hit = mask[rows] | mask[S.indices]
    data[hit] = 0
    data[hit & mask[rows] & (rows == S.indices)] = diag
    return data


EXACT_SHIFT = 3                   # values are integers times 2^-3


def exact_values(rng, n):
    return rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], size=n) * np.exp2(rng.integers(-EXACT_SHIFT, EXACT_SHIFT + 1, size=n))


def exact_reference(M, A, zero_dofs=None, diag=1.0):
    """(S, data): the pattern of K and its values as float64, exact (module docstring)"""
    S, _ = structural(M, A)
    sc = 2.0 ** EXACT_SHIFT
    Mi, Ai = sp.csr_matrix(M) * sc, sp.csr_matrix(A) * sc
    for X in (Mi, Ai):
        assert np.array_equal(X.data, np.rint(X.data)) and np.all(X.data != 0)
    Mi, Ai = Mi.astype(np.int64), Ai.astype(np.int64)
    budget = (abs(Mi).T.tocsr() @ abs(Ai) @ abs(Mi))
    assert budget.nnz == 0 or int(budget.max()) < 2 ** 53, "exact operands: an entry of K leaves the integers of a double"
    Ki = _on_pattern(S, (Mi.T.tocsr() @ Ai @ Mi).tocsr())
    data = Ki.astype(np.float64) * 2.0 ** (-3 * EXACT_SHIFT)
    return S, apply_zero_dofs(S, data, zero_dofs, diag)


def float_reference(M, A, zero_dofs=None, diag=1.0):
    """(S, ref, bound) on the pattern S: K in numpy.longdouble (dense copies) and the per-entry bound of the module docstring,
    0 at the entries that the dofs to zero set (those are exact)"""
    S, _ = structural(M, A)
    Md, Ad = sp.csr_matrix(M).toarray().astype(np.longdouble), sp.csr_matrix(A).toarray().astype(np.longdouble)
    Kd = Md.T @ (Ad @ Md)
    mag = abs(Md).T @ (abs(Ad) @ abs(Md))
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    ref, mg = Kd[rows, S.indices], mag[rows, S.indices]
    bound = np.longdouble(1.05) * (S.data.astype(np.longdouble) + 2) * np.longdouble(2.0) ** -53 * mg
    if zero_dofs is not None and len(zero_dofs):
        keep = apply_zero_dofs(S, np.ones(S.nnz), zero_dofs, 7.0) == 1.0
        ref = np.where(keep, ref, apply_zero_dofs(S, np.zeros(S.nnz), zero_dofs, diag).astype(np.longdouble))
        bound = np.where(keep, bound, np.longdouble(0))
    return S, ref, bound


def bound_ratio(data, ref, bound):
    """largest |K - ref| / bound over the entries (entries with bound 0 have to be equal)"""
    err = abs(data.astype(np.longdouble) - ref)
    assert np.all(err[bound == 0] == 0)
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------- operand builders
def csr_with(rows, cols, shape, values):
    """sorted CSR with the given entries (no duplicates among them) and values drawn by `values(n)`"""
    P = sp.csr_matrix((np.ones(len(rows)), (np.asarray(rows), np.asarray(cols))), shape=shape)
    assert P.nnz == len(rows), "duplicate entries"
    P.sort_indices()
    P.data = values(P.nnz)
    return P


def lane_group_lengths():
    """(operand row lengths, outer row lengths) that the lane-group cases ask for, over ALL lane groups G = 8 ... 64 and both
    stages: 0, 1, G - 1, G, G + 1, 2 G + 1, 64, 65, 129 and 0, 1, U NG - 1, U NG, U NG + 1, 63, 64, 65, 130 (NG = 64 / G)"""
    inner, outer = {0, 1, 64, 65, 129}, {0, 1, 63, 64, 65, 130}
    for lg in LANE_GROUPS:
        G = 1 << lg
        inner |= {G - 1, G, G + 1, 2 * G + 1}
        for U in GW_U:
            outer |= {U * (64 // G) - 1, U * (64 // G), U * (64 // G) + 1}
    return sorted(inner), sorted(outer)


def lane_group_operands(values, seed=11, nfe=400, ncp=300, row_scale=None):
    """One operand set for every lane group (``lane_group_lengths``).  Returns (M, A, info).

    M (nfe x ncp):  the first rows are the DESIGNATED rows, one per operand row length, with their entries in the columns that
    are not designated; the first columns are the DESIGNATED columns, one per outer row length, with their entries in the
    rows that are not designated; every other row has three entries more in the other columns.
    A (nfe x nfe):  behind the designated rows of M, one row of one entry per designated row of M (so that A M has a row of
    each operand row length, and M^T reaches it), then one row per outer row length with random columns (the longest lists
    every designated row of M), the rest random rows of 2 ... 12 entries.  No row of A holds its own diagonal.
    info: the designated rows / columns and the dof of the one-entry column (its row of K has no diagonal)."""
    rng = np.random.default_rng(seed)
    inner, outer = lane_group_lengths()
    nr, nc = len(inner), len(outer)
    free_rows, free_cols = np.arange(nr, nfe), np.arange(nc, ncp)
    r, c = [], []
    for i, L in enumerate(inner):                                   # designated rows
        r += [i] * L
        c += list(rng.choice(free_cols, size=L, replace=False))
    single = nr + inner.index(1)                                    # the row of A with one entry, at the M row of one entry
    for j, L in enumerate(outer):                                   # designated columns
        rows = [single] if L == 1 else list(rng.choice(free_rows, size=L, replace=False))
        r += rows
        c += [j] * L
    for i in free_rows:
        r += [i] * 3
        c += list(rng.choice(free_cols, size=3, replace=False))
    M = csr_with(r, c, (nfe, ncp), values)
    r, c = [], []
    for i in range(nr):                                             # rows nr ... 2 nr - 1: one entry, at designated row i of M
        r.append(nr + i)
        c.append(i)
    outer_rows = {}
    row = 2 * nr
    for L in outer:
        if L in (0, 1):                                             # (row 0 of A is empty; the rows above have one entry)
            continue
        others = np.array([x for x in range(nfe) if x != row])
        if L >= nr + 1:
            rest = np.array([x for x in others if x >= nr])
            cols = list(range(nr)) + list(rng.choice(rest, size=L - nr, replace=False))
        else:
            cols = list(rng.choice(others, size=L, replace=False))
        r += [row] * L
        c += cols
        outer_rows[L] = row
        row += 1
    for i in range(row, nfe):
        L = int(rng.integers(2, 13))
        others = np.array([x for x in range(nfe) if x != i])
        r += [i] * L
        c += list(rng.choice(others, size=L, replace=False))
    for i in range(1, nr):                                          # rows 1 ... nr - 1: short random rows (row 0 stays empty)
        others = np.array([x for x in range(nfe) if x != i])
        r += [i] * 2
        c += list(rng.choice(others, size=2, replace=False))
    A = csr_with(r, c, (nfe, nfe), values)
    if row_scale is not None:
        A = sp.diags(row_scale(rng, nfe)) @ A
        A = A.tocsr()
        A.sort_indices()
    info = dict(inner=inner, outer=outer, m_rows=dict(zip(inner, range(nr))), m_cols=dict(zip(outer, range(nc))),
                am_rows=dict(zip(inner, range(nr, 2 * nr))), a_rows=outer_rows, no_diagonal_dof=outer.index(1))
    return M, A, info


def lane_group_zero_dofs(S, info):
    """dofs to zero for the lane-group set: the first and the last dof whose row of K has a diagonal, and the dof whose row
    has none"""
    d = S.diagonal()
    with_diag = np.nonzero(d > 0)[0]
    return [int(with_diag[0]), int(with_diag[-1]), info["no_diagonal_dof"]]


def normal_values(seed):
    rng = np.random.default_rng(seed)
    return lambda n: rng.standard_normal(n)


def exact_value_source(seed):
    rng = np.random.default_rng(seed)
    return lambda n: exact_values(rng, n)


def decade_row_scale(rng, n):
    """10^k, k in [-6, 6], per row"""
    return 10.0 ** rng.integers(-6, 7, size=n)


def uniform_operands(L, values, nfe=402, ncp=300):
    """every row of M and of A M has exactly L entries: the rows 3 g, 3 g + 1, 3 g + 2 of M share one column list, and a row of
    A refers to one to three rows of its own group"""
    assert nfe % 3 == 0 and L <= ncp
    r, c = [], []
    for s in range(nfe):
        g = s // 3
        r += [s] * L
        c += list((7 * g + np.arange(L)) % ncp)
    M = csr_with(r, c, (nfe, ncp), values)
    r, c = [], []
    for s in range(nfe):
        g = s // 3
        for t in range(1 + s % 3):
            r.append(s)
            c.append(3 * g + (s + t) % 3)
    return M, csr_with(r, c, (nfe, nfe), values)


def random_operands(n, values, seed, per_row=6):
    """square operands of n rows with up to `per_row` random entries per row (the scheduling cases: only the row count matters)"""
    rng = np.random.default_rng(seed)

    def pattern():
        r, c = [], []
        for i in range(n):
            L = min(n, int(rng.integers(1, per_row + 1)))
            r += [i] * L
            c += list(rng.choice(n, size=L, replace=False))
        return r, c
    return csr_with(*pattern(), (n, n), values), csr_with(*pattern(), (n, n), values)


def banded_operands(values, seed=5, nfe=400, ncp=300):
    """M: row r holds 4 columns around r ncp / nfe; A: row r holds the columns r - 3 ... r + 3 except r - 1 (clipped).  Row
    blocks of the product need only a halo of rows"""
    r, c = [], []
    for i in range(nfe):
        c0 = min(max(i * ncp // nfe - 1, 0), ncp - 4)
        r += [i] * 4
        c += list(range(c0, c0 + 4))
    M = csr_with(r, c, (nfe, ncp), values)
    r, c = [], []
    for i in range(nfe):
        cols = [x for x in range(i - 3, i + 4) if 0 <= x < nfe and x != i - 1]
        r += [i] * len(cols)
        c += cols
    return M, csr_with(r, c, (nfe, nfe), values)


def block_rows(M, A, d0, d1):
    """the row blocks of a product of the dofs [d0, d1), as the streamed engines form them: the rows of M^T of the dofs, the
    rows of A that they refer to, the rows of M that those refer to.  Returns ((a0, a1), (m0, m1))"""
    MT = sp.csr_matrix(M).T.tocsr()[d0:d1]
    a0, a1 = int(MT.indices.min()), int(MT.indices.max()) + 1
    Ab = sp.csr_matrix(A)[a0:a1]
    return (a0, a1), (int(Ab.indices.min()), int(Ab.indices.max()) + 1)


def identity_like(n, values):
    return csr_with(np.arange(n), np.arange(n), (n, n), values)


def tridiagonal_with_row(n, values, row, columns):
    """tridiagonal A of n rows whose row `row` holds `columns` instead"""
    r = np.concatenate([np.arange(n), np.arange(1, n), np.arange(n - 1)])
    c = np.concatenate([np.arange(n), np.arange(n - 1), np.arange(1, n)])
    keep = r != row
    r, c = list(r[keep]), list(c[keep])
    r += [row] * len(columns)
    c += list(columns)
    return csr_with(r, c, (n, n), values)


def rehash_operands(values, which):
    """(M, A, row): M diagonal, A tridiagonal but for one row.  'a': the row holds REHASH_TRIPLE and its own neighbourhood
    (600 rows); 'b': the row is REHASH_ROW (2304 rows).  With M diagonal, A M and K have the pattern of A: the row is the
    designated row of both stages, alone in its workgroup"""
    if which == "a":
        n, row = 600, 300
        cols = REHASH_TRIPLE + [299, 300, 301]
    else:
        n, row = 2304, 1000
        cols = list(REHASH_ROW)
    return identity_like(n, values), tridiagonal_with_row(n, values, row, cols), row


def rows_of(S):
    S = sp.csr_matrix(S)
    return [S.indices[S.indptr[i]:S.indptr[i + 1]] for i in range(S.shape[0])]
