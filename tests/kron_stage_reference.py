"""CPU side of tests/test_gpu_kron_stage.py: references, operand builders and a plain-Python restatement of the host logic of
the Kronecker-stage PtAP (tigar_amd/csrc/tg_ptap_box.hip).  Nothing here needs a GPU;
tests/test_kron_stage_reference_host.py checks this file and the premises of the inputs it builds.

A stage is  K = P^T A P,  P = F_2 (x) F_1 (x) F_0  (direction 0 fastest; F_k the identity where a direction is not contracted),
A an arbitrary sparse matrix on the input index space n_0 x n_1 x n_2.

Restated host logic
    ``magic24`` follows ``tg_magic24`` line by line; ``decode24`` the column decode of ``k_ptap_line`` (operands masked to 24
    bits as v_mul_u32_u24 / v_mul_hi_u32_u24 do, the high word of the 48-bit product when both divisors carry the hi flag,
    else the 64-bit product shifted by sh or sh + 32); ``float_divmod`` the single-precision quotients of the contraction and
    the write loop; ``line_runs`` / ``run_rows`` the runs of ``tg_kron_line_runs`` and the first / last cut of the kernel;
    ``stage_geometry`` the stages operands -> boxes -> LDS layout -> kernel choice of the driver, so that the row of
    ``g_kron_routes`` a case claims is known before a GPU is asked.

    A consequence that the geometry shows: the line kernels need ``maxB[a] <= 32``, and a support list lies inside its box,
    so a line stage never has a list of more than 32 entries.  The guard ``cstr <= 64`` of the driver and the ``len <= 64``
    of the kernel cannot be approached from the line side; lists of 33 and more entries belong to the box kernel.

Exact reference
    Operands whose values are small integers times a power of two (``exact_values`` of tests/ptap_wave_reference.py: an
    integer in [-4, 4] \\ {0} times 2^e, e in [-3, 3]; a stored +-0.0 in A is an entry of value 0).  With c contracted
    directions the entries of P scaled by 2^(3 c) and those of A scaled by 2^3 are integers, K scaled by 2^(3 (2 c + 1)) is the
    int64 product of scipy.  ``exact_reference`` asserts  max_ij (|P|^T |A| |P|)_ij < 2^53  in those units: every partial sum of
    every entry, in any order and any association, is then an integer below 2^53, i.e. a double, and so is every
    intermediate of the box kernel's integer grid (its grid step 2^(exponent(b1) - 61) divides the unit as long as
    b1 < 2^(61 - 3 (2 c + 1)), which the budget implies).  No operation rounds and the device has to return the reference bit
    for bit.  The pattern is ones(P)^T ones(A) ones(P); entries that cancel are stored as +0.0 (a sum that cancels is +0.0 in
    round-to-nearest, and the first addition to an untouched slot, -0.0 + x, gives +0.0 for x = +-0.0 through fma(w, v, 0.0)).

Floating reference and the bound of the line kernel
    ``float_reference``: numpy.longdouble, summed term by term over the stored entries.  The line kernel forms an entry as

        scatter       X_s  = sum_r fl(w_r A_rs)            fma(w, v, 0.0): one rounding per product; the n1(s) products of a
                                                           slot are added by LDS atomics: n1 - 1 roundings in some order
        contraction   K_ij = sum_x F_xi X_x                an FMA chain over the line of the box: one rounding per step whose
                                                           operand is touched and whose weight is structural (the other steps
                                                           add +-0.0), n2(i, j) such steps

    so every triple term F_ri A_rs F_sj of K_ij passes through at most  q = max_x n1(x) + n2  roundings (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2: whatever the order).  T_ij, the number of triple terms, is
    sum_x n1(x) >= max_x n1 + (n2 - 1), so q <= T_ij + 1, and with (1 + u)^q - 1 <= 1.05 q u for q u < 0.09 the bound of the
    wave-per-row kernels carries over unchanged:

        |K_ij - ref_ij|  <=  1.05 (T_ij + 2) 2^-53 mag_ij ,      mag = |P|^T |A| |P| ,

    T_ij read from the structural product.  The reference's own error is (T + 2) 2^-64 mag, 2^-11 of it.

The bounds of the box kernel (c contracted directions)
    ``TIGAR_PTAP_ACCUM=float``.  The weight of an operand row is the product of its c list weights (c - 1 roundings); the
    scatter rounds the product w v and every one of the n1 - 1 additions of a slot; contraction k rounds a product and an
    addition per step (one rounding where the compiler fuses them), at most n2_k + 1 roundings on the way of a term.  The
    terms of an entry form a tree of nested sums, T_ij >= n1 + sum_k (n2_k - 1), so a triple term passes through at most
    q = (c - 1) + n1 + sum_k (n2_k + 1) <= T_ij + 3 c  roundings:

        |K_ij - ref_ij|  <=  1.05 (T_ij + 3 c) 2^-53 mag_ij .

    The integer grid (``int``, and unset while the operand rows of the output row are of one scale: largest entries within
    2^16 of each other, ``box_row_is_float``).  tg_fix rounds every scatter term fl(w v) of output row i to the grid
    2^(exponent(b1_i) - 61) <= b1_i 2^-61,  b1_i = sum_r |P_ri| max_s |A_rs|  -- half a step each, an ABSOLUTE error relative to
    the bound of the row, not to mag_ij -- and adds the integers exactly; the way back rounds once.  The n1(i, s) roundings
    of slot s reach K_ij through the contraction weights, so with the count matrix N = ones(P)^T ones(A)

        |K_ij - ref_ij|  <=  1.05 (T_ij + 3 c) 2^-53 mag_ij  +  1.05 * 2^-62 b1_i (N |P|)_ij

    (the relative part as above: c - 1 for the weight, one for w v, one for the way back in place of the n1 - 1 additions;
    the factor 1.05 of the second part covers the roundings of the contractions on the carried error and those of b1 itself).
    Derived, not measured.
"""
import numpy as np
import scipy.sparse as sp

import ptap_wave_reference as W

M24 = (1 << 24) - 1
TG_BOX_MAXLIST, TG_BOX_MAXD = 96, 48
LINE_VARIANTS = {1: (20, 10), 2: (32, 16)}
LINE_PAIRS = ((0, 1), (1, 0), (2, 0), (0, -1))


# ---------------------------------------------------------------------------------------------- decode
def magic24(dsr, bound):
    """(m, sh, hi) or None: tg_magic24"""
    if dsr == 0 or bound > (1 << 24):
        return None
    k = 0
    while (1 << k) < bound * dsr:
        k += 1
    for p in range(2):
        kk = k if p == 0 else max(k, 32)
        if kk > 47:
            return None
        mm = ((1 << kk) + dsr - 1) // dsr
        if mm >= (1 << 24):
            continue
        if p == 0 and (kk >= 32 or bound * mm >= (1 << 32)):
            continue
        j = np.arange((bound + dsr - 1) // dsr, dtype=object) if bound * mm >= (1 << 62) else np.arange((bound + dsr - 1) // dsr, dtype=np.int64)
        e1 = j * dsr
        ok = bool(np.all((e1 * mm) >> kk == j)) and bool(np.all(((e1[1:] - 1) * mm) >> kk == j[1:] - 1))
        if ok and bound > 0:
            ok = ((bound - 1) * mm) >> kk == (bound - 1) // dsr
        if not ok:
            continue
        return mm, (kk - 32 if kk >= 32 else kk), (1 if kk >= 32 else 0)
    return None


def decode_magics(nin0, nin1, maxB2):
    """(magic of e / (n0 n1) for e < n0 n1 maxB2, magic of r / n0 for r < n0 n1), either None when not found; the conditions of
    tg_kron_lds_layout on the sizes included"""
    n01 = nin0 * nin1
    if not (n01 < (1 << 23) and n01 * maxB2 <= (1 << 24)):
        return None, None
    return magic24(n01, n01 * maxB2), magic24(nin0, n01)


def decode_class(nin0, nin1, maxB2):
    """'lo': both quotients from the low word; 'mixed': one divisor carries the hi flag, the hi=0 instantiation shifts the
    64-bit product by sh + 32; 'hi': both do, the hi=1 instantiations; 'no24': no 24-bit decode, the stage goes to the box kernel"""
    a, b = decode_magics(nin0, nin1, maxB2)
    if a is None or b is None:
        return "no24"
    return {0: "lo", 1: "mixed", 2: "hi"}[a[2] + b[2]]


def _div24(e, magic, HI):
    m, sh, hi = magic
    e = np.asarray(e, dtype=np.uint64) & np.uint64(M24)
    prod = e * np.uint64(m & M24)                                   # 48 bits
    if HI:
        return (prod >> np.uint64(32)) >> np.uint64(sh)             # v_mul_hi_u32_u24, then the shift
    return (prod >> np.uint64(sh + 32 if hi else sh)) & np.uint64(0xFFFFFFFF)      # (hi << 32 | lo) >> total shift, to 32 bits


def decode24(e, nin0, nin1, maxB2):
    """(x2, x1, x0) of the offsets e as ``add`` of k_ptap_line computes them; arrays of int64"""
    a, b = decode_magics(nin0, nin1, maxB2)
    HI = bool(a[2] and b[2])
    e = np.asarray(e, dtype=np.int64)
    x2 = _div24(e, a, HI).astype(np.int64)
    rem = e - x2 * (nin0 * nin1)                                    # v_mad_i32_i24: all three within 24 bits here
    x1 = _div24(rem, b, HI).astype(np.int64)
    return x2, x1, rem - x1 * nin0


def float_divmod(s, B):
    """(s / B, s % B) as the kernel's  (int)(((float)s + 0.5f) * (1.0f / (float)B))"""
    s = np.asarray(s, dtype=np.int64)
    inv = np.float32(1.0) / np.float32(B)
    q = ((s.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)
    return q, s - q * B


# ---------------------------------------------------------------------------------------------- runs
def line_runs(nout, u, out_row0, out_row1, line_run=20, min_waves=1):
    """dict(mlen, ulo, uhi, x0, nx, nchunk, nwaves) of tg_kron_line_runs; `nout` = (m0, m1, m2).  u < 0: one row per wave"""
    m0, m1 = nout[0], nout[1]
    m01 = m0 * m1
    if u < 0:
        return dict(mlen=0, ulo=0, uhi=0, x0=0, nx=0, nchunk=0, nwaves=out_row1 - out_row0)
    ra, rb = out_row0, out_row1 - 1
    if u == 2:
        ulo, uhi, x0, nx = ra // m01, rb // m01, 0, m01
    elif u == 1:
        ulo, uhi, x0, nx = 0, m1 - 1, m0 * (ra // m01), m0 * (rb // m01 - ra // m01 + 1)
    else:
        ulo, uhi, x0 = 0, m0 - 1, ra // m0
        nx = rb // m0 - x0 + 1
    span = uhi - ulo + 1
    T = min(min(64, max(1, line_run)), span)
    cdiv = lambda a, b: (a + b - 1) // b
    while T > 1 and nx * cdiv(span, T) < min_waves:
        T = (T + 1) // 2
    return dict(mlen=T, ulo=ulo, uhi=uhi, x0=x0, nx=nx, nchunk=cdiv(span, T), nwaves=nx * cdiv(span, T))


def run_rows(nout, u, out_row0, out_row1, line_run=20, min_waves=1):
    """for every wave, the output rows it writes (the first / last cut of k_ptap_line)"""
    Q = line_runs(nout, u, out_row0, out_row1, line_run, min_waves)
    if u < 0:
        return [[r] for r in range(out_row0, out_row1)]
    m0, m1 = nout[0], nout[1]
    m01 = m0 * m1
    waves = []
    for b in range(Q["nx"] * Q["nchunk"]):
        c = b // Q["nx"]
        x = Q["x0"] + (b - c * Q["nx"])
        iu0 = Q["ulo"] + c * Q["mlen"]
        last = min(Q["mlen"], Q["uhi"] + 1 - iu0)
        if u == 0:
            I, rstep = [iu0, x % m1, x // m1], 1
        elif u == 1:
            I, rstep = [x % m0, iu0, x // m0], m0
        else:
            I, rstep = [x % m0, x // m0, iu0], m01
        R0 = I[0] + m0 * I[1] + m01 * I[2]
        first = 0
        if R0 < out_row0:
            first = (out_row0 - R0 + rstep - 1) // rstep
        if R0 + (last - 1) * rstep >= out_row1:
            last = (out_row1 - 1 - R0) // rstep + 1 if R0 < out_row1 else 0
        waves.append([R0 + t * rstep for t in range(first, last)])
    return waves


# ---------------------------------------------------------------------------------------------- the host driver
def _lists(F):
    FT = sp.csr_matrix(F).T.tocsr()
    FT.sort_indices()
    return FT


def reach(dims, A, cur_row0=0, stride=1):
    """(lmax, rmax) per direction and coordinate: k_box_reach over every `stride`-th row of the block"""
    n = list(dims) + [1] * (3 - len(dims))
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
    keep = rows % stride == 0
    g, s = rows[keep] + cur_row0, A.indices[keep].astype(np.int64)
    L, R = [], []
    for k in range(3):
        div = int(np.prod(n[:k]))
        rk, sk = (g // div) % n[k], (s // div) % n[k]
        l, r = np.zeros(n[k], dtype=np.int64), np.zeros(n[k], dtype=np.int64)
        np.maximum.at(l, rk, rk - sk)
        np.maximum.at(r, rk, sk - rk)
        L.append(l)
        R.append(r)
    return L, R


def dmax(F, B):
    """tg_kron_dmax: most output indices reachable from a window of B input indices (first column of the first non-empty
    row, last column of the last one)"""
    F = sp.csr_matrix(F)
    F.sort_indices()
    n = F.shape[0]
    ne = np.diff(F.indptr) > 0
    first = np.where(ne, F.indices[np.minimum(F.indptr[:-1], max(F.nnz - 1, 0))], 0) if F.nnz else np.zeros(n, dtype=np.int64)
    last = np.where(ne, F.indices[np.maximum(F.indptr[1:] - 1, 0)], 0) if F.nnz else np.zeros(n, dtype=np.int64)
    idx = np.arange(n)
    nxt = np.where(ne, idx, n)                    # first non-empty row at or after a
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]
    prv = np.maximum.accumulate(np.where(ne, idx, -1))
    D = 1
    for a0 in range(n):
        a1 = min(n, a0 + B) - 1
        lo, hi = nxt[a0], prv[a1]
        if lo <= a1 and hi >= a0 and last[hi] >= first[lo]:
            D = max(D, int(last[hi] - first[lo] + 1))
    return D


def box_lds(cap, cap1, ctab, nlist, nt):
    b = (cap + cap1) * 8 + nt * 16 + nlist * 8 + ctab * 8
    b += nt * 4 + 128 + nlist * 4 + 3 * TG_BOX_MAXD * 4 + ctab * 4
    return b + cap * 2 + 64


def stage_geometry(dims, factors, A, cur_row0=0, stride=1, nt=256, line=True, slowdecode=False):
    """The plan of one stage as tg_kron_operands ... tg_kron_choose make it: dict(nin, nout, blo, bhi, maxB, boxmax, Dmax, cstr,
    maxlen, lds, declined, fast24, decode, variant, a, u, hi, route).  `route` is the name the trace prints, None when the
    stage is declined on the host"""
    d = len(dims)
    nin = list(dims) + [1] * (3 - d)
    fac = list(factors) + [None] * (3 - d)
    con = [f is not None for f in fac]
    nout = [sp.csr_matrix(fac[k]).shape[1] if con[k] else nin[k] for k in range(3)]
    FT = [_lists(fac[k]) if con[k] else None for k in range(3)]
    L, R = reach(dims, A, cur_row0, stride)
    blo, bhi, maxB, maxlen, cstr, Dm = [], [], [1, 1, 1], [1, 1, 1], [0, 0, 0], [1, 1, 1]
    for k in range(3):
        lo, hi = np.zeros(nout[k], dtype=np.int64), np.zeros(nout[k], dtype=np.int64)
        if con[k]:
            for i in range(nout[k]):
                a = FT[k].indices[FT[k].indptr[i]:FT[k].indptr[i + 1]].astype(np.int64)
                if a.size:
                    lo[i], hi[i] = (a - L[k][a]).min(), (a + R[k][a]).max()
                    maxlen[k] = max(maxlen[k], int(a[-1] - a[0] + 1))
            cstr[k] = max(1, int(np.diff(FT[k].indptr).max()))
        else:
            i = np.arange(nout[k])
            lo, hi = i - L[k], i + R[k]
        lo, hi = np.maximum(lo, 0), np.minimum(hi, nin[k] - 1)
        blo.append(lo)
        bhi.append(hi)
        maxB[k] = max(1, int((hi - lo + 1).max()))
    boxmax = maxB[0] * maxB[1] * maxB[2]
    cap = (min(boxmax, 1 << 20) + 7) & ~7
    ctab = nlist = 0
    maxl = 1
    for k in range(3):
        if con[k]:
            Dm[k] = dmax(fac[k], maxB[k])
            maxl = max(maxl, maxlen[k])
            ctab += Dm[k] * cstr[k]
            nlist += cstr[k]
    ctab, nlist = (ctab + 7) & ~7, (nlist + 7) & ~7
    ext, sz = list(maxB), []
    for k in range(d):
        if con[k]:
            ext[k] = Dm[k]
            sz.append(ext[0] * ext[1] * ext[2])
    c1need = max([8] + sz[0::2])
    cap = max([cap] + sz[1::2])
    cap1 = (c1need + 7) & ~7
    cap = max(cap, cap1)
    need = sum(Dm[k] for k in range(d) if con[k])
    ntk = 256 if need > nt else nt
    lds = box_lds(cap, cap1, ctab, nlist, ntk)
    G = dict(nin=nin, nout=nout, blo=blo, bhi=bhi, maxB=maxB, boxmax=boxmax, Dmax=Dm, cstr=cstr, maxlen=maxlen, lds=lds, cap=cap,
             cap1=cap1, FT=FT, con=con, d=d, variant=0, a=-1, u=-1, hi=0, route=None, nt=ntk)
    G["declined"] = boxmax > (1 << 20) or lds > 150 * 1024 or maxl > TG_BOX_MAXLIST or max(Dm) > TG_BOX_MAXD
    if G["declined"]:
        return G
    ma, mb = (None, None) if slowdecode or not maxB[0] * maxB[1] < (1 << 23) else decode_magics(nin[0], nin[1], maxB[2])
    G["fast24"] = ma is not None and mb is not None
    G["decode"] = "slow" if slowdecode else decode_class(nin[0], nin[1], maxB[2])
    ks = [k for k in range(d) if con[k]]
    if len(ks) == 1 and line and cstr[ks[0]] <= 64 and boxmax <= (1 << 16) and G["fast24"]:
        a = ks[0]
        variant = 1 if maxB[a] <= 20 and Dm[a] <= 10 else 2 if maxB[a] <= 32 and Dm[a] <= 16 else 0
        if Dm[a] > maxB[a]:
            variant = 0
        bam, dmt = LINE_VARIANTS[1] if variant == 1 else LINE_VARIANTS[2]
        G["line_lds"] = (((boxmax + 7) & ~7) + bam * dmt + dmt) * 8
        if G["line_lds"] > 60 * 1024:
            variant = 0
        u = -1
        for k in range(d):
            if not con[k] and nout[k] > 1:
                u = k
                break
        if not ((a == 0 and u == 1) or (a >= 1 and u == 0)):
            u = -1
        if u < 0 and a != 0:
            variant = 0
        G.update(variant=variant, a=a, u=u)
    if G["variant"]:
        G["hi"] = 1 if ma[2] and mb[2] else 0
        G["route"] = "k_ptap_line<%d,%d,%d,%d,hi=%d>" % (LINE_VARIANTS[G["variant"]] + (G["a"], G["u"], G["hi"]))
    else:
        G["route"] = "k_ptap_box<%d>" % ntk
    return G


def line_row_shapes(G, fac_a, A, rows, cur_row0=0):
    """what k_ptap_line sees at the output rows `rows` of a line stage: [dict(len, Ba, D, nlines, nY, items, operand_rows)],
    items = (operand row, 64-entry pass) pairs of the stream, operand_rows = the entry counts of the operand rows"""
    a, nin, nout = G["a"], G["nin"], G["nout"]
    F = sp.csr_matrix(fac_a)
    F.sort_indices()
    FT = G["FT"][a]
    A = sp.csr_matrix(A)
    cnt = np.diff(A.indptr)
    out = []
    for Rr in rows:
        I = [Rr % nout[0], (Rr // nout[0]) % nout[1], Rr // (nout[0] * nout[1])]
        B = [int(G["bhi"][k][I[k]] - G["blo"][k][I[k]] + 1) for k in range(3)]
        boa = int(G["blo"][a][I[a]])
        sub = F[boa:boa + B[a]]
        D = int(sub.indices.max() - sub.indices.min() + 1) if sub.nnz else 0
        la = FT.indices[FT.indptr[I[a]]:FT.indptr[I[a] + 1]]
        lens = []
        for s in la:
            r = list(I)
            r[a] = int(s)
            lens.append(int(cnt[r[0] + nin[0] * r[1] + nin[0] * nin[1] * r[2] - cur_row0]))
        nlines = B[0] * B[1] * B[2] // B[a]
        out.append(dict(len=len(la), Ba=B[a], D=D, nlines=nlines, nY=nlines * D, operand_rows=lens,
                        items=sum(max(1, -(-l // 64)) for l in lens)))
    return out


# ---------------------------------------------------------------------------------------------- operand builders
def banded_factor(m, L, s, values, lengths=None, drop=None):
    """F (n x m), n = s (m - 1) + L: column j holds the rows s j ... s j + L - 1 (`lengths[j]` rows instead where given: 0 is an
    all-zero column; a longer one widens the window at that coordinate only); `drop`: (row, column) pairs taken out again"""
    lengths = dict(lengths or {})
    n = s * (m - 1) + L
    r, c = [], []
    for j in range(m):
        Lj = lengths.get(j, L)
        rows = [x for x in range(s * j, s * j + Lj) if x < n]
        r += rows
        c += [j] * len(rows)
    if drop:
        gone = set(drop)
        keep = [i for i in range(len(r)) if (r[i], c[i]) not in gone]
        r, c = [r[i] for i in keep], [c[i] for i in keep]
    return W.csr_with(r, c, (n, m), values)


def band_pattern(n, left, right=None):
    """1-D pattern: row i holds the columns i - left(i) ... i + right(i) (clipped); numbers or functions of i"""
    right = left if right is None else right
    fl = left if callable(left) else (lambda i: left)
    fr = right if callable(right) else (lambda i: right)
    r, c = [], []
    for i in range(n):
        cols = range(max(0, i - fl(i)), min(n - 1, i + fr(i)) + 1)
        r += [i] * len(cols)
        c += list(cols)
    return sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))


def stencil(dims, reaches, values):
    """A on the tensor index space with the box stencil of the per-direction reaches (numbers, functions of the coordinate or
    (left, right) pairs): 9-point / 27-point for reach 1"""
    P = None
    for n, rch in zip(dims, reaches):
        Pk = band_pattern(n, *rch) if isinstance(rch, tuple) else band_pattern(n, rch)
        P = Pk if P is None else sp.kron(Pk, P, format="csr")
    P = sp.csr_matrix(P)
    P.sort_indices()
    P.data = values(P.nnz)
    return P


def with_rows(A, rows, values):
    """A with the rows {row: columns} replaced"""
    A = sp.csr_matrix(A).tolil()
    for row, cols in rows.items():
        A.rows[row] = sorted(int(c) for c in cols)
        A.data[row] = [1.0] * len(cols)
    A = A.tocsr()
    A.sort_indices()
    A.data = values(A.nnz)
    return A


def neighbourhood(dims, node, reaches, count, rng):
    """`count` columns out of the box node +- reaches (clipped), the node itself first"""
    n = list(dims)
    axes = [np.arange(max(0, x - r), min(nk - 1, x + r) + 1) for x, r, nk in zip(node, reaches, n)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(n))
    strides = np.cumprod([1] + n[:-1])
    cols = grid @ strides
    assert count <= cols.size
    return list(rng.choice(cols, size=count, replace=False))


def signed_zeros(A, rng, share=0.1):
    """a share of A's entries set to +0.0 / -0.0, stored"""
    A = sp.csr_matrix(A, copy=True)
    hit = rng.random(A.nnz) < share
    A.data[hit] = np.where(rng.random(int(hit.sum())) < 0.5, 0.0, -0.0)
    return A


# ---------------------------------------------------------------------------------------------- references
def projector(dims, factors):
    P = None
    for n, F in zip(dims, factors):
        Fk = sp.identity(n, format="csr") if F is None else sp.csr_matrix(F)
        P = Fk if P is None else sp.kron(Fk, P, format="csr")
    return sp.csr_matrix(P)


def structural(P, A):
    S = (W.ones(P).T.tocsr() @ (W.ones(A) @ W.ones(P))).tocsr()
    S.sort_indices()
    return S


def exact_reference(dims, factors, A, zero_dofs=None, diag=1.0):
    """(S, data): the pattern of the stage's result and its values as float64, exact (module docstring); A is the whole
    operand, rows of a block are cut from the result with ``rows_of_block``"""
    c = sum(1 for F in factors if F is not None)
    P = projector(dims, factors)
    S = structural(P, A)
    Pi, Ai = P * 2.0 ** (W.EXACT_SHIFT * c), sp.csr_matrix(A) * 2.0 ** W.EXACT_SHIFT
    for X in (Pi, Ai):
        assert np.array_equal(X.data, np.rint(X.data))
    assert np.all(Pi.data != 0)
    Pi = sp.csr_matrix((Pi.data.astype(np.int64), Pi.indices, Pi.indptr), shape=Pi.shape)
    Ai = sp.csr_matrix((Ai.data.astype(np.int64), Ai.indices, Ai.indptr), shape=Ai.shape)       # (stored zeros stay entries)
    budget = abs(Pi).T.tocsr() @ (abs(Ai) @ abs(Pi))
    assert budget.nnz == 0 or int(budget.max()) < 2 ** 53, "exact operands: an entry of K leaves the integers of a double"
    Ki = W._on_pattern(S, (Pi.T.tocsr() @ (Ai @ Pi)).tocsr())
    data = Ki.astype(np.float64) * 2.0 ** (-W.EXACT_SHIFT * (2 * c + 1))
    return S, W.apply_zero_dofs(S, data, zero_dofs, diag)


def rows_of_block(S, data, r0, r1):
    """(indptr, indices, data) of the rows [r0, r1) of a result"""
    p0, p1 = S.indptr[r0], S.indptr[r1]
    return S.indptr[r0:r1 + 1] - p0, S.indices[p0:p1], data[p0:p1]


def box_row_is_float(P, A, accum):
    """per output row: does the box kernel accumulate it in floating point (tg_fix_choose)?  accum: '' | 'int' | 'float'"""
    P, A = sp.csc_matrix(P), sp.csr_matrix(A)
    if accum == "float":
        return np.ones(P.shape[1], dtype=bool)
    if accum == "int":
        return np.zeros(P.shape[1], dtype=bool)
    rowmax = np.zeros(A.shape[0])
    np.maximum.at(rowmax, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), abs(A.data))
    fp = np.zeros(P.shape[1], dtype=bool)
    for i in range(P.shape[1]):
        sl = slice(P.indptr[i], P.indptr[i + 1])
        rm = rowmax[P.indices[sl]][(P.data[sl] != 0)]
        rm = rm[rm != 0]
        fp[i] = rm.size > 0 and rm.max() > 65536.0 * rm.min()
    return fp


def ld_matmul(X, Y, yvals=None):
    """X Y in numpy.longdouble, term by term over the stored entries: (product pattern as sorted CSR of ones, values on it).
    Y: a CSR matrix, or a pattern with longdouble values `yvals` on it (the result of an earlier call)"""
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    X.sort_indices()
    Y.sort_indices()
    yv = (Y.data if yvals is None else yvals).astype(np.longdouble)
    xr = np.repeat(np.arange(X.shape[0], dtype=np.int64), np.diff(X.indptr))
    cnt = np.diff(Y.indptr)[X.indices]
    start = Y.indptr[X.indices]
    which = np.repeat(np.arange(X.nnz), cnt)                              # the entry of X of every term
    at = np.arange(which.size) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(start, cnt)
    key = xr[which] * Y.shape[1] + Y.indices[at]
    keys, inv = np.unique(key, return_inverse=True)
    vals = np.zeros(keys.size, dtype=np.longdouble)
    np.add.at(vals, inv, X.data.astype(np.longdouble)[which] * yv[at])
    r, c = keys // Y.shape[1], keys % Y.shape[1]
    Z = sp.csr_matrix((np.ones(keys.size), (r, c)), shape=(X.shape[0], Y.shape[1]))
    Z.sort_indices()
    assert Z.nnz == keys.size
    return Z, vals


def _ld_on_pattern(S, Z, vals):
    """longdouble values of (Z, vals) on the pattern S (Z's pattern lies inside it)"""
    nc = S.shape[1]
    ks = np.repeat(np.arange(S.shape[0], dtype=np.int64), np.diff(S.indptr)) * nc + S.indices
    kz = np.repeat(np.arange(Z.shape[0], dtype=np.int64), np.diff(Z.indptr)) * nc + Z.indices
    at = np.searchsorted(ks, kz)
    assert np.array_equal(ks[at], kz)
    out = np.zeros(S.nnz, dtype=np.longdouble)
    out[at] = vals
    return out


def float_reference(dims, factors, A, zero_dofs=None, diag=1.0, kernel="line", accum=""):
    """(S, ref, bound, own): numpy.longdouble, term by term over the stored entries, the per-entry bound of the module docstring (`kernel`: 'line' or
    'box', the latter with the setting `accum` of TIGAR_PTAP_ACCUM) and the bound of the reference's own error"""
    c = sum(1 for F in factors if F is not None)
    P = projector(dims, factors)
    A = sp.csr_matrix(A)
    S = structural(P, A)
    PT = P.T.tocsr()
    ref = _ld_on_pattern(S, *ld_matmul(PT, *ld_matmul(A, P)))
    mg = _ld_on_pattern(S, *ld_matmul(abs(PT), *ld_matmul(abs(A), abs(P))))
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    T = S.data.astype(np.longdouble)
    q = (T + 3 * c) if kernel == "box" else (T + 2)
    bound = np.longdouble(1.05) * q * np.longdouble(2.0) ** -53 * mg
    if kernel == "box":
        # the integer grid: every scatter term of row i is rounded to a grid of at most b1_i 2^-61, b1_i = sum_r |P_ri| rowmax_r
        # (half a step each), and the n1(i, s) roundings of slot s reach K_ij through the weights |P_sj|
        rowmax = np.zeros(A.shape[0])
        np.maximum.at(rowmax, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), abs(A.data))
        b1 = (abs(PT) @ rowmax).astype(np.longdouble) * (1 + np.longdouble(2.0) ** -40)
        carried = W._on_pattern(S, ((W.ones(P).T.tocsr() @ W.ones(A)) @ abs(P)).tocsr()).astype(np.longdouble) * (1 + np.longdouble(2.0) ** -40)
        grid = np.longdouble(1.05) * np.longdouble(2.0) ** -62 * b1[rows] * carried
        bound = bound + np.where(box_row_is_float(P, A, accum)[rows], np.longdouble(0), grid)
    own = (T + 2) * np.longdouble(2.0) ** -64 * mg
    if zero_dofs is not None and len(zero_dofs):
        keep = W.apply_zero_dofs(S, np.ones(S.nnz), zero_dofs, 7.0) == 1.0
        ref = np.where(keep, ref, W.apply_zero_dofs(S, np.zeros(S.nnz), zero_dofs, diag).astype(np.longdouble))
        bound, own = np.where(keep, bound, np.longdouble(0)), np.where(keep, own, np.longdouble(0))
    return S, ref, bound, own


# ---------------------------------------------------------------------------------------------- the cases of the GPU file
def fit_factor(n, L0, s, values, **kw):
    """banded factor with exactly n rows: stride s, the shortest list length L >= L0 that fits"""
    L = L0
    while (n - L) % s:
        L += 1
    return banded_factor((n - L) // s + 1, L, s, values, **kw)


def stage(dims, a, factor, A, **more):
    fac = [None] * len(dims)
    if isinstance(a, int):
        fac[a] = factor
    else:
        for k, F in zip(a, factor):
            fac[k] = F
    return dict(dims=list(dims), factors=fac, A=A, **more)


LINE = "k_ptap_line<%s,%d,%d,hi=%d>"
V1, V2 = "20,10", "32,16"
# name: (input index space, contracted direction, (L0, stride) of the factor, rows of A kept along direction 1 or None,
#        decode class, route)
DECODE_CASES = {
    "lo-2d": ((129, 129), 0, (5, 2), None, "lo", LINE % (V1, 0, 1, 0)),
    "lo-3d": ((17, 9, 45), 2, (21, 4), None, "lo", LINE % (V2, 2, 0, 0)),
    "mixed-01": ((255, 255), 0, (5, 2), None, "mixed", LINE % (V1, 0, 1, 0)),
    "mixed-10": ((255, 255), 1, (21, 4), None, "mixed", LINE % (V2, 1, 0, 0)),
    "mixed-20": ((127, 127, 9), 2, (5, 2), 24, "mixed", LINE % (V1, 2, 0, 0)),
    "mixed-0n": ((40001, 1, 5), 0, (5, 2), None, "mixed", LINE % (V1, 0, -1, 0)),
    "hi-01-v1": ((257, 257), 0, (5, 2), None, "hi", LINE % (V1, 0, 1, 1)),
    "hi-10-v2": ((257, 257), 1, (21, 4), None, "hi", LINE % (V2, 1, 0, 1)),
    "hi-01-v2": ((512, 128), 0, (20, 4), None, "hi", LINE % (V2, 0, 1, 1)),
    "hi-10-v1": ((512, 128), 1, (4, 2), None, "hi", LINE % (V1, 1, 0, 1)),
    "hi-0n-v1": ((46341,), 0, (5, 2), None, "hi", LINE % (V1, 0, -1, 1)),
    "hi-0n-v2": ((46341,), 0, (21, 4), None, "hi", LINE % (V2, 0, -1, 1)),
    "hi-20-v1": ((257, 257, 3), 2, (3, 1), 12, "hi", LINE % (V1, 2, 0, 1)),
    "hi-20-v2": ((257, 257, 25), 2, (21, 4), 6, "hi", LINE % (V2, 2, 0, 1)),
    "no24-256": ((256, 256), 0, (4, 2), None, "no24", "k_ptap_box<256>"),
    "no24-128x512": ((128, 512), 0, (4, 2), None, "no24", "k_ptap_box<256>"),
}
NO24_SHAPES = [(256, 256, 1), (128, 512, 1), (33, 2049, 1), (255, 257, 1)]


def decode_case(name):
    dims, a, (L0, s), keep1, cls, route = DECODE_CASES[name]
    src = W.exact_value_source(sum(map(ord, name)))
    F = fit_factor(dims[a], L0, s, src)
    reaches = [1] * len(dims)
    if keep1 is not None:                                # rows of A only in the first lines: the class needs the index space, not the rows
        reaches[1] = (lambda i: 1 if i < keep1 else -1, lambda i: 1 if i < keep1 else -1)
    return stage(dims, a, F, stencil(dims, reaches, src), decode=cls, route=route)


# ---- the run loop: small stages whose runs are kept long by TIGAR_LINE_MIN_WAVES=1
def run_case(which, seed=3):
    """'u1': 2-D, a = 0, runs along direction 1 (70 rows: no multiple of 20, 63 or 64; the reach along the run is 1 but for
    the last 10 rows, where it is 4 to the left and 2 to the right, so the box extents change from step to step; column 4 of
    the factor has a window of 9 rows instead of 5).  'u0': the same transposed, a = 1.  'u0-3d': a = 2, runs along direction 0
    over 3 planes.  'none': 1-D.  'none-3d': a = 0 with a single line per plane (n1 = 1): no run direction either"""
    src = W.exact_value_source(seed)
    wide = dict(lengths={4: 9})
    along = (lambda i: 1 if i < 60 else 4, lambda i: 1 if i < 60 else 2)
    if which == "u1":
        return stage((27, 70), 0, banded_factor(12, 5, 2, src, **wide), stencil((27, 70), [1, along], src), u=1)
    if which == "u0":
        return stage((70, 27), 1, banded_factor(12, 5, 2, src, **wide), stencil((70, 27), [along, 1], src), u=0)
    if which == "u0-3d":
        return stage((23, 5, 11), 2, banded_factor(4, 5, 2, src), stencil((23, 5, 11), [along_short, 1, 1], src), u=0)
    if which == "none":
        return stage((131,), 0, banded_factor(64, 5, 2, src, **wide), stencil((131,), [2], src), u=-1)
    if which == "none-3d":
        return stage((27, 1, 6), 0, banded_factor(12, 5, 2, src), stencil((27, 1, 6), [1, 0, 1], src), u=-1)
    raise KeyError(which)


def along_short(i):
    return 1 if i < 18 else 3


def default_threshold_case():
    """600 x 600 input nodes, 9-point A, a = 0 with a diagonal factor (D == Ba == 3): 600 cross-section lines x 30 chunks of 20
    rows are more than the 64 waves per CU of a 256-CU part, so the runs keep their 20 rows without the switch"""
    src = W.exact_value_source(17)
    return stage((600, 600), 0, banded_factor(600, 1, 1, src), stencil((600, 600), [1, 1], src), u=1)


# ---- operand rows, items, lists and box lines of the line kernel
OPERAND_ROWS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 128, 129, 255, 256, 257]
ITEM_COUNTS = [3, 4, 5, 8, 9]
LINES_AND_SLOTS = [63, 64, 65]


def operand_row_case(seed=5, zeros=False):
    """2-D (27 x 120), a = 0, runs along direction 1.  The factor: 12 columns of 5 rows at stride 2, column 0 with 3 and column 1
    with 4.  A: the 9-point stencil, with designated rows of OPERAND_ROWS entries out of the neighbourhood +-1 x +-50 of their
    node (two of them in one support list, so that item counts of 8 and 9 occur), and rows whose reach along direction 1 gives
    their line boxes of exactly 63, 64, 65 lines, and of 21, 16 / 32 and 13 lines, which with D = 3, 4 / 2 and 5 functions are 63, 64
    and 65 slots of the contracted box.  `zeros`: a tenth of the entries stored as +0.0 / -0.0"""
    rng = np.random.default_rng(seed)
    src = W.exact_value_source(seed)
    dims = (27, 120)
    F = banded_factor(12, 5, 2, src, lengths={0: 3, 1: 4})
    A = stencil(dims, [1, 1], src)
    rows = {}
    node = lambda x, y: x + dims[0] * y
    spots = [(9 + (k % 2) * 2, 52 + k // 2) for k in range(len(OPERAND_ROWS))]        # x = 9 and 11 share the lists of columns 4, 5
    for L, (x, y) in zip(OPERAND_ROWS, spots):
        rows[node(x, y)] = neighbourhood(dims, (x, y), (1, 50), L, rng) if L else []
    for y, (l, r) in {40: (31, 31), 42: (31, 32), 44: (32, 32), 12: (10, 10), 10: (7, 8), 14: (6, 6), 36: (15, 16)}.items():
        for x in (0, 2, 13):
            rows[node(x, y)] = [node(x, y - l), node(x, y), node(x, y + r)]
    A = with_rows(A, rows, src)
    if zeros:
        A = signed_zeros(A, rng)
    return stage(dims, 0, F, A, u=1, designated={L: node(*xy) for L, xy in zip(OPERAND_ROWS, spots)})


LIST_LENGTHS = [0, 1, 31, 32]


def span_factor(spans, values):
    """F whose column j holds the rows start ... start + length - 1 of spans[j]"""
    r = [x for start, length in spans for x in range(start, start + length)]
    c = [j for j, (start, length) in enumerate(spans) for _ in range(length)]
    return W.csr_with(r, c, (max(start + length for start, length in spans), len(spans)), values)


LIST_SPANS = [(0, 5), (4, 5), (8, 0), (9, 1), (10, 5), (14, 5), (19, 31), (50, 32), (82, 5), (86, 5)]


def list_case(seed=7):
    """2-D (91 x 9), a = 0: columns of 5 rows that share one row with their neighbour, but column 2 with none (an empty output
    row in every run step of its line), column 3 with 1, column 6 with 31 and column 7 with 32 rows -- the longest list a line
    stage can have.  A couples along direction 1 only, so the boxes are the windows.  (The long columns stand beside the short
    ones, not across them: a box of 5 nodes inside a column of 32 would see the hull of all the columns that cross it, more
    functions than it has nodes, and the kernel declines such a stage.)"""
    src = W.exact_value_source(seed)
    F = span_factor(LIST_SPANS, src)
    return stage((91, 9), 0, F, stencil((91, 9), [0, 1], src), u=1, columns={0: 2, 1: 3, 31: 6, 32: 7})


def line_box_shapes(G, fac_a):
    """[(Ba, D)] per output coordinate along the contracted direction: the box and the hull of the functions it reaches"""
    a = G["a"]
    F = sp.csr_matrix(fac_a)
    F.sort_indices()
    out = []
    for i in range(G["nout"][a]):
        lo, hi = int(G["blo"][a][i]), int(G["bhi"][a][i])
        sub = F[lo:hi + 1]
        out.append((hi - lo + 1, int(sub.indices.max() - sub.indices.min() + 1) if sub.nnz else 0))
    return out


# ---- variant and size edges: name -> (stage, expected route or None for a decline on the host, maxB[a], Dmax[a])
def uniform_line(L, s, m=24, reach=0, n1=6, seed=9):
    src = W.exact_value_source(seed + L + s)
    n0 = s * (m - 1) + L
    return stage((n0, n1), 0, banded_factor(m, L, s, src), stencil((n0, n1), [reach, 1], src), u=1)


def edge_case(name):
    src = W.exact_value_source(sum(map(ord, name)))
    if name in EDGE_UNIFORM:
        (L, s), route, maxB, D = EDGE_UNIFORM[name]
        return dict(uniform_line(L, s), route=route, maxB=maxB, Dmax=D)
    if name == "D==Ba":                                   # a diagonal factor, reach 2: every box has 5 nodes and reaches 5 functions
        return dict(stage((40, 6), 0, banded_factor(40, 1, 1, src), stencil((40, 6), [2, 1], src)), route=LINE % (V1, 0, 1, 0),
                    maxB=5, Dmax=5)
    if name == "D>Ba in one box":
        # a C^0 joint: column 10 holds node 20 alone, and a coupling added by hand gives that node function 11 as well (it
        # carries 8 ... 11).  A does not couple across the joint, so the box of output 10 is the node itself and reaches
        # four functions: the maxima the host compares (8 nodes, 7 functions) do not show it, the kernel declines at that row
        F = banded_factor(20, 5, 2, src, lengths={10: 1}).tolil()
        F[20, 11] = 1.0
        F = sp.csr_matrix(F)
        F.sort_indices()
        F.data = src(F.nnz)
        cut = (lambda i: 0 if i == 20 else 1 if i != 21 else 0, lambda i: 0 if i == 20 else 1 if i != 19 else 0)
        return dict(stage((43, 6), 0, F, stencil((43, 6), [cut, 1], src)), route=LINE % (V1, 0, 1, 0), declines_in_kernel=True)
    if name in ("list 65", "list 96", "list 97"):
        L = int(name.split()[1])                          # one column with L rows; the others 5 at stride 4
        F = banded_factor(40, 5, 4, src, lengths={6: L})
        return dict(stage((161, 4), 0, F, stencil((161, 4), [0, 1], src)), route=None if L > TG_BOX_MAXLIST else "k_ptap_box<256>",
                    maxB=L)
    if name in ("Dmax 48", "Dmax 49"):                    # 1-D, 5 rows per column at stride 1: a box of B nodes reaches B + 4 functions
        r = (19, 20) if name == "Dmax 48" else (20, 20)
        return dict(stage((124,), 0, banded_factor(120, 5, 1, src), stencil((124,), [r], src)),
                    route="k_ptap_box<256>" if name == "Dmax 48" else None, Dmax=int(name.split()[1]))
    if name in ("line LDS 60 KiB", "line LDS above 60 KiB", "box LDS 150 KiB", "box LDS above 150 KiB"):
        # boxes of 8 x B1 nodes: one row per line that reaches far along direction 1
        B1 = {"line LDS 60 KiB": 933, "line LDS above 60 KiB": 934, "box LDS 150 KiB": BOX_B1_FITS, "box LDS above 150 KiB": BOX_B1_FITS + 1}[name]
        n1 = B1 + 40
        dims = (12, n1)
        A = stencil(dims, [1, 1], src)
        y = n1 // 2
        l, r = (B1 - 1) // 2, B1 - 1 - (B1 - 1) // 2
        A = with_rows(A, {x + 12 * y: [x + 12 * (y - l), x + 12 * y, x + 12 * (y + r)] for x in range(12)}, src)
        route = {"line LDS 60 KiB": LINE % (V1, 0, 1, 0), "line LDS above 60 KiB": "k_ptap_box<256>", "box LDS 150 KiB": "k_ptap_box<256>",
                 "box LDS above 150 KiB": None}[name]
        return dict(stage(dims, 0, banded_factor(4, 6, 2, src), A), route=route, boxmax=8 * B1)
    raise KeyError(name)


BOX_B1_FITS = 1315        # the largest B1 whose box of 8 x B1 nodes (and 4 x B1 after the contraction) fits in 150 KiB (box_lds)
EDGE_UNIFORM = {          # (L, stride) of a uniform factor, reach 0: the box is the window
    "maxB 20": ((20, 4), LINE % (V1, 0, 1, 0), 20, 10),
    "maxB 21": ((21, 4), LINE % (V2, 0, 1, 0), 21, 11),
    "maxB 32": ((32, 8), LINE % (V2, 0, 1, 0), 32, 8),
    "maxB 33": ((33, 8), "k_ptap_box<256>", 33, 9),
    "Dmax 10": ((20, 4), LINE % (V1, 0, 1, 0), 20, 10),
    "Dmax 11": ((16, 3), LINE % (V2, 0, 1, 0), 16, 11),
    "Dmax 16": ((31, 4), LINE % (V2, 0, 1, 0), 31, 16),
    "Dmax 17": ((25, 3), "k_ptap_box<256>", 25, 17),
}
EDGE_CASES = list(EDGE_UNIFORM) + ["D==Ba", "D>Ba in one box", "list 65", "list 96", "list 97", "Dmax 48", "Dmax 49",
                                   "line LDS 60 KiB", "line LDS above 60 KiB", "box LDS 150 KiB", "box LDS above 150 KiB"]


# ---- the box kernel
BOX_DIMS = (11, 9, 7)


def box_factors(src):
    return [banded_factor(4, 5, 2, src), banded_factor(3, 5, 2, src), banded_factor(2, 5, 2, src)]


def box_case(c, values=None, seed=21, rows=None):
    """3-D (11 x 9 x 7), 27-point A, the first c directions contracted at once.  `rows`: a function (A) -> A applied to the
    operand (row scales)"""
    src = values or W.exact_value_source(seed + c)
    fac = box_factors(src)
    A = stencil(BOX_DIMS, [1, 1, 1], src)
    if rows is not None:
        A = rows(A)
    return stage(BOX_DIMS, list(range(c)), fac[:c], A)


def two_scales(step):
    """rows of A normalised to a largest entry of exactly 1, every other row times 2^16 (1 + step 2^-52): at step 0 the largest
    entries of the operand rows of an output row differ by exactly 2^16 (one scale: the integer grid), at step 1 by the next
    double above it (tg_fix_choose goes to floating point)"""
    def rows(A):
        A = sp.csr_matrix(A, copy=True)
        r = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        big = np.zeros(A.shape[0])
        np.maximum.at(big, r, abs(A.data))
        A.data = A.data / big[r]
        assert np.all(np.maximum.reduceat(abs(A.data), A.indptr[:-1]) == 1.0)
        A.data = A.data * np.where(r % 2 == 1, 65536.0 * (1.0 + step * 2.0 ** -52), 1.0)
        return A
    return rows


NCOMBO = {63: (7, 9), 64: (8, 8), 65: (5, 13), 255: (15, 17), 256: (16, 16), 258: (6, 43)}


def ncombo_case(seed=23):
    """2-D (25 x 61), both directions contracted: the columns 0 ... 5 of the two factors have the list lengths of NCOMBO, so the
    output rows (j, j) have 63, 64, 65, 255, 256 and 258 operand rows: NT - 1, NT, NT + 1 for the workgroup of 64 and NT - 1, NT,
    NT + 2 for that of 256 (257 is prime and would need one list of 257 entries, beyond TG_BOX_MAXLIST)"""
    src = W.exact_value_source(seed)
    pairs = list(NCOMBO.values())
    F0 = banded_factor(12, 3, 2, src, lengths={j: p[0] for j, p in enumerate(pairs)})
    F1 = banded_factor(30, 3, 2, src, lengths={j: p[1] for j, p in enumerate(pairs)})
    return stage((25, 61), [0, 1], [F0, F1], stencil((25, 61), [1, 1], src), rows={n: j + 12 * j for j, n in enumerate(NCOMBO)})


def view_case(seed=29):
    """2-D (27 x 70), both directions: the factor and A of the run case 'u1' and a second factor of 34 columns.  (stage, the
    first stage alone, the second stage on its result)"""
    c = run_case("u1", seed)
    F0, F1 = c["factors"][0], banded_factor(34, 4, 2, W.exact_value_source(seed + 1))
    both = stage((27, 70), [0, 1], [F0, F1], c["A"])
    first = stage((27, 70), 0, F0, c["A"])
    return both, first, [None, F1]


def repeated_knot_case(seed=25):
    """every node carries two functions of its own (a direction of C^-1 pieces): a box of 3 nodes reaches 6 functions, the
    buffer after the contraction (cap1) is larger than the one before it (cap)"""
    src = W.exact_value_source(seed)
    n = 20
    F = W.csr_with(np.repeat(np.arange(n), 2), np.arange(2 * n), (n, 2 * n), src)
    return stage((n, 5), 0, F, stencil((n, 5), [1, 1], src), route="k_ptap_box<256>")


def reach_stride_case(seed=27, stride=7):
    """the run case 'u1' with one entry far along direction 0 in a row that the sampled reach scan (every 7th row) skips"""
    c = run_case("u1", seed)
    row = 13 + 27 * 30
    assert row % stride
    cols = list(c["A"][row].indices) + [row + 9]
    src = W.exact_value_source(seed + 1)
    return dict(c, A=with_rows(c["A"], {row: cols}, src), stride=stride, row=row)


# ---- what the GPU file runs, for the host test to check without a GPU
LINE_RUNS = [1, 2, 3, 20, 63, 64, 100]                    # TIGAR_LINE_RUN; 100 is clamped to 64
RUN_BLOCKS = {            # output row blocks: one row; first and last row inside a run, a line, a plane
    "u1": [(5, 6), (41, 566)], "u0": [(70, 71), (173, 671)], "u0-3d": [(130, 131), (168, 379)], "none": [(10, 50)], "none-3d": [(7, 61)]}
RUN_ROUTES = {"u1": LINE % (V1, 0, 1, 0), "u0": LINE % (V1, 1, 0, 0), "u0-3d": LINE % (V1, 2, 0, 0), "none": LINE % (V2, 0, -1, 0),
              "none-3d": LINE % (V1, 0, -1, 0)}


def nout_of(c):
    return [c["dims"][k] if F is None else F.shape[1] for k, F in enumerate(c["factors"])] + [1] * (3 - len(c["dims"]))


def claimed_routes():
    """every row of g_kron_routes that a case of tests/test_gpu_kron_stage.py asserts by name"""
    names = {v[5] for v in DECODE_CASES.values()} | set(RUN_ROUTES.values()) | {"k_ptap_box<64>", "k_ptap_box<256>"}
    return names | {v[1] for v in EDGE_UNIFORM.values()}


def floating(c, seed, row_scale=None):
    """the case with normal values on the same patterns; `row_scale(rng, n)`: a scale per row of A"""
    vals = W.normal_values(seed)
    fac = []
    for F in c["factors"]:
        if F is not None:
            F = sp.csr_matrix(F, copy=True)
            F.data = vals(F.nnz)
        fac.append(F)
    A = sp.csr_matrix(c["A"], copy=True)
    A.data = vals(A.nnz)
    if row_scale is not None:
        scale = row_scale(np.random.default_rng(seed), A.shape[0])
        A.data = A.data * np.repeat(scale, np.diff(A.indptr))
    return dict(c, factors=fac, A=A)
