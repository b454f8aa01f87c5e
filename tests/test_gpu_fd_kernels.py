"""GPU: the kernels of csrc/tg_fd.hip (k_fd_mode<0..3>, k_fd_outside, k_fd_diag, k_fd_fit, k_fd_scale) driven through
tigar_amd.device.DeviceFD with no spline, against the longdouble reference of tests/fd_reference.py evaluated from the
same Q, lam, dk, dm, coefficients and diag K: at exact tiles and chunks, degenerate directions, padded sizes that differ per
direction, partial last chunks and row tiles, boxes with free faces, several blocks in one workspace, the pseudo-inverse
branch, the fitted sums and the refusals.

Two checks per application (u = 2^-53):

1. elementwise, derived: |z_gpu - z_ld| <= (2 sum_k np_k + 32) u absprod, absprod the same chain with |Q|, |1/s|, |S|, |r|.
2. normwise, measured: ||z_gpu - z_ld|| / ||z_ld|| on the box over the same figure of numpy's float64 evaluation of the
   reference (never under u: a result merely rounded to float64 is that far off) is at most RATIO_BOUND.

RATIO_BOUND is 4 times the largest ratio seen on an MI355X, rounded up to a power of two.  Largest ratio per shape over the
coefficient sets, scalings and layouts, in that run (kernel error / numpy error):

    (16, 16, 16) 1.01   (64, 64) 1.02       (32, 64, 16) 1.01   (1, 1, 1) 0.85      (2, 1, 3) 1.35
    (1, 200) 2.22       (200, 1) 2.04       (17, 33, 65) 1.02   (5, 40, 70) and its five other orders 1.00 to 1.01
    (70, 40) 1.00       (40, 70) 1.03       (129, 64) 1.00      (64, 129) 1.01      (3, 200) 1.43
    (100, 90, 80) 1.00  (144, 144, 20) 1.00 three blocks (70, 40, 5) 1.01, (5, 8, 3) 1.03, (33, 17, 65) 1.01
    Neumann (22, 22, 22) 1.02               diagonal defects (17, 6, 9) 1.06

The kernel's relative error was 9e-17 to 7.8e-16, numpy's 1e-17 to 7.8e-16; the largest ratio 2.22 gives 4 x 2.22 = 8.9,
rounded up 16.  In check 1 the worst entry of the same run used 1e-2 of the bound at (2, 1, 3), 1e-6 at (144, 144, 20).
The module takes 9 s on that machine (the longdouble references of (100, 90, 80) and (144, 144, 20) most of it), so each
coefficient set evaluates its own reference.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import fd_reference as R

pytestmark = pytest.mark.gpu

RATIO_BOUND = 16.0

# free sizes per direction; the id says what the shape is there for
SHAPES = [
    ("exact-tiles-16-16-16", (16, 16, 16)),
    ("exact-tiles-64-64", (64, 64)),
    ("exact-tiles-32-64-16", (32, 64, 16)),
    ("degenerate-1-1-1", (1, 1, 1)),
    ("degenerate-2-1-3", (2, 1, 3)),
    ("degenerate-1-200-quarter-c-tile", (1, 200)),
    ("degenerate-200-1-quarter-c-tile", (200, 1)),
    ("np-32-48-80-partial-chunk-partial-row-tile", (17, 33, 65)),
    ("np-16-48-80-order-012", (5, 40, 70)),
    ("np-16-48-80-order-021", (5, 70, 40)),
    ("np-16-48-80-order-102", (40, 5, 70)),
    ("np-16-48-80-order-120", (40, 70, 5)),
    ("np-16-48-80-order-201", (70, 5, 40)),
    ("np-16-48-80-order-210", (70, 40, 5)),
    ("2d-C-48", (70, 40)),
    ("2d-C-80", (40, 70)),
    ("2d-C-64-three-row-tiles", (129, 64)),
    ("2d-C-144", (64, 129)),
    ("2d-C-208", (3, 200)),
    ("five-chunks-two-row-tiles-100-90-80", (100, 90, 80)),
    ("bench-np-144-144-thin-third", (144, 144, 20)),
]
# also run with lo = 0 on some sides and two layers on others, so that N, lo and nf all differ per direction
MIXED = {(16, 16, 16), (2, 1, 3), (1, 200), (17, 33, 65), (5, 40, 70), (70, 5, 40), (70, 40), (64, 129)}
# real B-spline pencils (p = 2, 3, 4 per direction) instead of random SPD pairs
BSPLINE = {(17, 33, 65), (100, 90, 80)}

# (scaling, (c_0, c_1, c_2, c_m)); c_2 is dropped in 2-D
CONFIGS = [
    ("diagonal-mass", True, (1.0, 2.5, 0.5, 0.3)),
    ("none-nomass", False, (0.7, 1.0, 1.3, 0.0)),
    ("diagonal-c1-zero", True, (1.0, 0.0, 2.0, 0.5)),
    ("none-c0-zero-nomass", False, (0.0, 1.5, 1.0, 0.0)),
]


def _layout(nf, mixed):
    """grid shape N, lo, hi per direction"""
    d = len(nf)
    if not mixed:
        return [n + 2 for n in nf], [1] * d, [n + 1 for n in nf]
    pads = [(0, 2), (2, 0), (2, 2)] if d == 3 else [(0, 2), (2, 1)]
    return [n + a + b for n, (a, b) in zip(nf, pads)], [a for a, _ in pads], [n + a for n, (a, _) in zip(nf, pads)]


class _Block(object):
    """host data of one block: grid, box, the 1-D pencils' Q, lam and diagonals"""

    def __init__(self, shape, lo, hi, rng, bspline=None):
        """bspline: degrees per direction of real B-spline pencils on the grid, None for random SPD pairs"""
        self.shape, self.lo, self.hi = list(shape), list(lo), list(hi)
        self.d = len(shape)
        self.nf = [h - l for l, h in zip(lo, hi)]
        self.Qs, self.lams, self.dk, self.dm = [], [], [], []
        for k in range(self.d):
            if bspline:
                p = bspline[k]
                K1, M1 = R.iga_1d(p, shape[k] - p)
                K1, M1 = K1[lo[k]:hi[k], lo[k]:hi[k]], M1[lo[k]:hi[k], lo[k]:hi[k]]
            else:
                K1, M1 = R.random_spd_pair(self.nf[k], rng)
            Q, lam = R.eig_pencil(K1, M1)
            self.Qs.append(Q)
            self.lams.append(lam)
            self.dk.append(np.diag(K1).copy())
            self.dm.append(np.diag(M1).copy())
        self.size = int(np.prod(shape))
        # diag K: diag P (all coefficients 1) times a factor in [0.5, 2] on the box, positive values off it
        self.dg = rng.uniform(0.5, 2.0, size=shape[::-1])
        self.dg[R.box_slices(lo, hi)] *= R.diag_p(self.dk, self.dm, [1.0] * (self.d + 1), np.float64)

    def coef(self, c4):
        return [c4[k] for k in range(self.d)] + [c4[3]]

    def args(self, r, dg, c4, scaling):
        return (r, dg, self.lo, self.hi, self.Qs, self.lams, self.dk, self.dm, self.coef(c4), scaling)


def _csr(dg, rng, drop=()):
    """a matrix whose diagonal is dg (the rows listed in ``drop`` store none) with two off-diagonal entries in most rows"""
    n = dg.size
    keep = np.ones(n, dtype=bool)
    keep[list(drop)] = False
    i = np.arange(n)
    rows = np.concatenate([i[keep], i[:-1], i[3:]])
    cols = np.concatenate([i[keep], i[1:], i[:-3]])
    vals = np.concatenate([dg[keep], rng.standard_normal(max(n - 1, 0) + max(n - 3, 0))])
    M = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    assert M.nnz == rows.size                      # (zeros on the diagonal stay stored)
    return M


class _Case(object):
    """blocks at consecutive offsets, the device object fitted to a synthetic K, one residual"""

    def __init__(self, blocks, rng, dg=None, drop=()):
        from tigar_amd.device import DeviceCSR, DeviceFD
        self.blocks = blocks
        self.offsets = np.concatenate([[0], np.cumsum([b.size for b in blocks])]).astype(np.int64)
        self.n = int(self.offsets[-1])
        self.dg = np.concatenate([b.dg.ravel() for b in blocks]) if dg is None else dg
        self.r = rng.standard_normal(self.n)
        self.K = DeviceCSR.from_scipy(_csr(self.dg, rng, drop))
        self.fd = DeviceFD(self.n)
        for b, off in zip(blocks, self.offsets):
            self.fd.add_block(int(off), b.shape, b.lo, b.hi, b.Qs, b.lams, b.dk, b.dm)
        self.sums = self.fd.fit(self.K, len(blocks))

    def part(self, v, i):
        b = self.blocks[i]
        return v[self.offsets[i]:self.offsets[i + 1]].reshape(b.shape[::-1])

    def apply(self, c4, scaling):
        """two applications into NaN-filled vectors: bits equal, every entry finite"""
        from tigar_amd.device import DeviceVector
        self.fd.set_coefficients(np.tile(np.asarray(c4, dtype=np.float64), len(self.blocks)), scaling)
        rv = DeviceVector(data=self.r)
        out = []
        for _ in range(2):
            z = DeviceVector(data=np.full(self.n, np.nan))
            self.fd.apply(rv, z)
            out.append(z.get_local())
        assert np.array_equal(out[0].view(np.int64), out[1].view(np.int64)), "two applications differ in bits"
        assert np.all(np.isfinite(out[0])), "%d entries were not written" % np.sum(~np.isfinite(out[0]))
        return out[0]


def _assert_floor_clear(b, c4):
    """a condition on the inputs: no eigenvalue sum within a factor 100 of the floor, so that the branch taken does not
    hang on a rounding"""
    s = R.eig_sums(b.lams, b.coef(c4), np.float64)
    floor = R.floor_of(b.lams, b.coef(c4))
    assert floor > 0 and np.all((s <= floor / 100) | (s >= 100 * floor)), "test data: an eigenvalue sum near the floor"
    return int(np.sum(s <= floor))


def _check_block(case, i, z, c4, scaling, label):
    """the two checks and the off-box entries of block i of one application; returns the ratio of check 2"""
    b = case.blocks[i]
    zb, r, dg = case.part(z, i), case.part(case.r, i), case.part(case.dg, i)
    box = R.box_slices(b.lo, b.hi)
    zld = R.fd_apply(*b.args(r, dg, c4, scaling), dt=R.LD)
    z64 = R.fd_apply(*b.args(r, dg, c4, scaling), dt=np.float64)
    bound = R.hard_bound(b.nf, R.fd_absprod(*b.args(r, dg, c4, scaling)))
    err = np.abs(zb[box].astype(R.LD) - zld[box])
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0)))
    nrm = float(np.linalg.norm(zld[box].astype(np.float64)))
    e_gpu = float(np.linalg.norm(err.astype(np.float64))) / nrm
    e_np = float(np.linalg.norm((z64[box] - zld[box]).astype(np.float64))) / nrm
    ratio = e_gpu / max(e_np, R.U)
    print("FD %s block %d nf %s: worst err / hard bound %.3g, rel err kernel %.3g numpy %.3g ratio %.3g"
          % (label, i, tuple(b.nf), worst, e_gpu, e_np, ratio))
    assert np.all(err <= bound), "%d entries beyond the running-error bound, worst %.3g times it" % (np.sum(err > bound), worst)
    assert ratio <= RATIO_BOUND, "normwise error %.3g is %.3g times numpy's %.3g" % (e_gpu, ratio, e_np)
    off = np.ones(zb.shape, dtype=bool)
    off[box] = False
    with np.errstate(divide="ignore"):
        want = np.where(dg != 0, (1.0 / dg) * r, r)[off]
    assert np.all(np.abs(zb[off] - want) <= 2 * np.spacing(np.abs(want))), "off the box: more than 2 ulp from r / K_ii"
    return ratio


_cache = {}


def _shape_case(nf, mixed):
    """one case alive at a time (the coefficient sets of a shape run back to back)"""
    key = (nf, mixed)
    if key not in _cache:
        _cache.clear()
        rng = np.random.default_rng(1000 + 7 * sum(n * 31 ** k for k, n in enumerate(nf)) + int(mixed))
        shape, lo, hi = _layout(nf, mixed)
        _cache[key] = _Case([_Block(shape, lo, hi, rng, bspline=(2, 3, 4) if nf in BSPLINE else None)], rng)
    return _cache[key]


_APPLY = [pytest.param(nf, mixed, cfg, id="%s-%s-%s" % (name, "mixed-faces" if mixed else "clamped", cfg[0]))
          for name, nf in SHAPES for mixed in ((False, True) if nf in MIXED else (False,)) for cfg in CONFIGS]


@pytest.mark.parametrize("nf,mixed,cfg", _APPLY)
def test_apply_matches_reference(nf, mixed, cfg):
    _, scaling, c4 = cfg
    case = _shape_case(nf, mixed)
    assert _assert_floor_clear(case.blocks[0], c4) == 0
    z = case.apply(c4, scaling)
    _check_block(case, 0, z, c4, scaling, "%s %s %s" % (nf, "mixed" if mixed else "clamped", cfg[0]))


def _three_blocks(order, rng_seed=77):
    """three boxes of different size in one grid shape, at offsets f N0 N1 N2"""
    shape = [72, 42, 67]
    boxes = [((70, 40, 5), (1, 1, 3)), ((5, 8, 3), (0, 30, 60)), ((33, 17, 65), (2, 0, 1))]
    blocks = []
    for j in order:
        nf, lo = boxes[j]
        blocks.append(_Block(shape, lo, [l + n for l, n in zip(lo, nf)], np.random.default_rng(rng_seed + j)))
    return blocks


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)], ids=["largest-first", "reversed"])
def test_several_blocks_share_the_workspaces(order):
    """w0 / w1 are sized by the largest block and never cleared: each block's result must be what that block gives alone"""
    rng = np.random.default_rng(5)
    case = _Case(_three_blocks(order), rng)
    scaling, c4 = True, (1.0, 2.5, 0.5, 0.3)
    z = case.apply(c4, scaling)
    for i, b in enumerate(case.blocks):
        assert _assert_floor_clear(b, c4) == 0
        _check_block(case, i, z, c4, scaling, "blocks %s" % (order,))
        alone = _Case([b], rng, dg=case.part(case.dg, i).ravel().copy())
        alone.r = case.part(case.r, i).ravel().copy()
        za = alone.apply(c4, scaling)
        assert np.array_equal(za.view(np.int64), case.part(z, i).ravel().view(np.int64)), \
            "block %d of %s differs from the same block alone" % (i, order)


@pytest.mark.parametrize("scaling", [True, False], ids=["diagonal", "none"])
def test_pseudo_inverse_neumann_box(scaling):
    """B-spline box (20^3 elements, p = 2) with no clamped face and no mass term: the constant mode's eigenvalue sum is at
    rounding level (1e-12), under the floor (2.6e-9), and is dropped; the next sum is 9.87"""
    rng = np.random.default_rng(9)
    N = [22, 22, 22]
    case = _Case([_Block(N, [0, 0, 0], N, rng, bspline=(2, 2, 2))], rng)
    c4 = (1.0, 1.0, 1.0, 0.0)
    assert _assert_floor_clear(case.blocks[0], c4) == 1
    s = np.sort(R.eig_sums(case.blocks[0].lams, c4, np.float64).ravel())
    assert abs(s[0]) < 1e-10 and 9.8 < s[1] < 9.9 and 2e-9 < R.floor_of(case.blocks[0].lams, c4) < 3e-9
    z = case.apply(c4, scaling)
    _check_block(case, 0, z, c4, scaling, "neumann scaling %s" % scaling)


def test_diagonal_defects():
    """rows of K with no diagonal entry, a stored zero and a negative diagonal, each on and off the box: k_fd_diag gives
    0 for the absent ones, S is 1 where K_ii <= 0, z_i = r_i off the box where K_ii == 0"""
    rng = np.random.default_rng(21)
    shape, lo, hi = _layout((17, 6, 9), True)
    b = _Block(shape, lo, hi, rng)
    idx = np.arange(b.size).reshape(shape[::-1])
    inside = idx[R.box_slices(lo, hi)].ravel()
    outside = np.setdiff1d(idx.ravel(), inside)
    pick = lambda a: [int(v) for v in rng.choice(a, size=6, replace=False)]
    pin, pout = pick(inside), pick(outside)
    dg = b.dg.ravel().copy()
    absent = pin[0:2] + pout[0:2]
    dg[absent] = 0.0
    dg[pin[2:4] + pout[2:4]] = 0.0                 # stored zeros
    dg[pin[4:6] + pout[4:6]] *= -1.0
    b.dg = dg.reshape(shape[::-1])
    case = _Case([b], rng, drop=absent)
    want, mag = R.fit_sums(b.dg, lo, hi, b.dk, b.dm)
    assert np.all(np.abs(case.sums[0].astype(R.LD) - want) <= (len(inside) + 16) * R.U * mag)
    for _, scaling, c4 in CONFIGS[:2]:
        z = case.apply(c4, scaling)
        _check_block(case, 0, z, c4, scaling, "defects scaling %s" % scaling)
        flat = z.ravel()
        assert np.array_equal(flat[pout[0:4]], case.r[pout[0:4]])


def _check_fit(case):
    for i, b in enumerate(case.blocks):
        want, mag = R.fit_sums(case.part(case.dg, i), b.lo, b.hi, b.dk, b.dm)
        nbox = int(np.prod(b.nf))
        err = np.abs(case.sums[i].astype(R.LD) - want)
        print("FD fit block %d nf %s: err / bound %s" % (i, tuple(b.nf), np.asarray(
            err / np.where(mag > 0, (nbox + 16) * R.U * mag, 1), dtype=np.float64)))
        assert np.all(err <= (nbox + 16) * R.U * mag), (case.sums[i], want)
        assert np.all(want[:b.d] > 0) and want[3] > 0 and (b.d == 3 or case.sums[i][2] == 0.0)


def test_fit_sums_several_blocks():
    _check_fit(_Case(_three_blocks((0, 1, 2)), np.random.default_rng(6)))


def test_fit_sums_grid_stride():
    """720 000 box entries: more than the 512 x 256 threads of k_fd_fit, so its grid-stride loop runs several times"""
    _check_fit(_shape_case((100, 90, 80), False))
    _check_fit(_shape_case((129, 64), False))


def test_fit_recorded_diagonal_matches_extracted():
    """tg_fd_fit copies the diagonal that the tensor PtAP recorded with K, or extracts it (k_fd_diag) from a matrix that
    has none recorded: the same sums to the bit, and both the longdouble sums"""
    import tigar_amd as t
    from tigar_amd import BSplines as B
    from tigar_amd.device import DeviceCSR, DeviceFD
    from tigar_amd.forms import LaplaceForm
    p, nels = 2, (9, 6, 4)
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * 3, [B.uniformKnots(p, 0.0, 1.0, n) for n in nels]))
    sc = gen.getScalarSpline(0)
    for direction in range(3):
        for side in (0, 1):
            gen.addZeroDofs(0, sc.getSideDofs(direction, side))
    K = t.ExtractedSpline(gen, 2 * p).assembleMatrix(LaplaceForm())
    # (the diagonal is not observable from here: that K came out of the tensor PtAP, which records it, is)
    assert getattr(K, "tensor_structure", None) is not None
    shape = [n + p for n in nels]
    assert K.shape[0] == int(np.prod(shape))
    Ks = K.to_scipy()
    rng = np.random.default_rng(4)
    b = _Block(shape, [1, 0, 2], [shape[0] - 1, shape[1], shape[2]], rng)
    sums = []
    for M in (K, DeviceCSR.from_scipy(Ks)):
        fd = DeviceFD(K.shape[0])
        fd.add_block(0, b.shape, b.lo, b.hi, b.Qs, b.lams, b.dk, b.dm)
        sums.append(fd.fit(M, 1)[0])
    assert np.array_equal(sums[0].view(np.int64), sums[1].view(np.int64)), sums
    want, mag = R.fit_sums(Ks.diagonal().reshape(shape[::-1]), b.lo, b.hi, b.dk, b.dm)
    assert np.all(np.abs(sums[0].astype(R.LD) - want) <= (int(np.prod(b.nf)) + 16) * R.U * mag)


def test_refusals():
    """each refusal returns before anything is launched"""
    from tigar_amd._lib import TigarHipError
    from tigar_amd.device import DeviceFD, DeviceVector
    rng = np.random.default_rng(8)

    def add(fd, shape, lo, hi, offset=0):
        nf = [max(h - l, 1) for l, h in zip(lo, hi)]
        fd.add_block(offset, shape, lo, hi, [np.eye(n) for n in nf], [np.ones(n) for n in nf], [np.ones(n) for n in nf],
                     [np.ones(n) for n in nf])

    fd = DeviceFD(1000)
    with pytest.raises(TigarHipError, match="d must be 2 or 3"):
        add(fd, [10], [1], [9])
    with pytest.raises(TigarHipError, match="d must be 2 or 3"):
        add(fd, [5, 5, 5, 5], [1] * 4, [4] * 4)
    with pytest.raises(TigarHipError, match="empty or out-of-range box"):
        add(fd, [10, 10, 10], [1, 4, 1], [9, 4, 9])
    with pytest.raises(TigarHipError, match="empty or out-of-range box"):
        add(fd, [10, 10, 10], [1, 1, 1], [9, 11, 9])
    with pytest.raises(TigarHipError, match="empty or out-of-range box"):
        add(fd, [10, 10], [-1, 1], [9, 9])
    with pytest.raises(TigarHipError, match="outside the matrix"):
        add(fd, [10, 10, 10], [1, 1, 1], [9, 9, 9], offset=1)
    with pytest.raises(TigarHipError, match="outside the matrix"):
        add(fd, [10, 10], [1, 1], [9, 9], offset=-1)
    add(fd, [10, 10, 10], [1, 1, 1], [9, 9, 9])
    r, z = DeviceVector(data=np.ones(1000)), DeviceVector(1000)
    with pytest.raises(TigarHipError, match="tg_fd_fit \\(diagonal of K\\) must come first"):
        fd.set_coefficients([1.0, 1.0, 1.0, 0.0], True)
    with pytest.raises(TigarHipError, match="must come first"):
        fd.apply(r, z)
    case = _Case([_Block([10, 9, 8], [1, 1, 1], [9, 8, 7], rng)], rng)
    rv, zv = DeviceVector(data=case.r), DeviceVector(case.n)
    with pytest.raises(TigarHipError, match="tg_fd_set_coefficients must come first"):
        case.fd.apply(rv, zv)                      # fitted, no coefficients yet
    with pytest.raises(TigarHipError, match="vector length"):
        case.fd.apply(rv, DeviceVector(case.n + 1))
    for bad in ([1.0, -1.0, 1.0, 0.0], [1.0, 1.0, 1.0, -0.5], [float("nan"), 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, float("nan")]):
        with pytest.raises(TigarHipError, match="negative or NaN coefficient"):
            case.fd.set_coefficients(bad, True)
    with pytest.raises(TigarHipError, match="every coefficient is zero"):
        case.fd.set_coefficients([0.0, 0.0, 0.0, 0.0], False)
    case.fd.set_coefficients([1.0, 1.0, 1.0, 0.0], False)
    with pytest.raises(TigarHipError, match="r and z must be different vectors"):
        case.fd.apply(rv, rv)
    case.fd.apply(rv, zv)
    good = zv.get_local()
    # a refused set of coefficients stores nothing (the good ones ahead of the bad one neither): the last good set applies
    for bad in ([2.0, 3.0, -1.0, 0.0], [2.0, 3.0, 4.0, float("nan")]):
        with pytest.raises(TigarHipError, match="negative or NaN coefficient"):
            case.fd.set_coefficients(bad, True)
        zv = DeviceVector(data=np.full(case.n, np.nan))
        case.fd.apply(rv, zv)
        assert np.array_equal(zv.get_local().view(np.int64), good.view(np.int64))
