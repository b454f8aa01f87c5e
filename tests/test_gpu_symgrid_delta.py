"""-m gpu: the delta-coded values of the half-storage product (csrc/tg_symgrid.hip, TIGAR_SYMGRID_DELTA): the stored half of
K as int16 distances -- in 64-bit integer arithmetic -- from the fp64 blocks of one reference plane, restored bit for bit in
the product.  Everything is compared EXACTLY (``view(np.int64)``) with the plain plan (TIGAR_SYMGRID_DELTA=0): products on
compressible matrices (whole and as z slabs, several chunkings), the edges of the fit rule, a pool that overflows, matrices
the coding does not suit, and a CG solve through the API."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from tigar_amd import device
    device.device_info()          # raises loudly if the library / GPU is missing
    return device


def _upper_offsets(reach):
    """(dz, dy, dx) of the stored half: the diagonal and what follows it in a row"""
    return [o for o in itertools.product(range(-reach, reach + 1), repeat=3) if o >= (0, 0, 0)]


def _move(values, ulps):
    return (np.asarray(values, dtype=np.float64).view(np.int64) + np.asarray(ulps, dtype=np.int64)).view(np.float64)


def _repeated_stencil(rng, shape, reach, ulps=3000, scale_planes=(), factor=1.5):
    """ONE random symmetric stencil repeated over the (n0, n1, n2) grid (x fastest), every stored value moved by a random
    number of ulps in +-ulps (upper triangle, mirrored: K stays symmetric), truncated at the faces.  The upper entries of
    the rows in ``scale_planes`` are multiplied by ``factor`` (those planes then differ from every other by far more than
    an int16 of ulps).  Returns (A, base) with base[(dz, dy, dx)] the stencil."""
    n0, n1, n2 = shape
    n = n0 * n1 * n2
    idx = np.arange(n).reshape(n2, n1, n0)
    zpl = np.repeat(np.arange(n2), n0 * n1)
    rows, cols, vals = [], [], []
    base = {}
    for off in _upper_offsets(reach):
        b = rng.standard_normal()
        base[off] = b
        src = tuple(slice(max(0, -o), s - max(0, o)) for o, s in zip(off, (n2, n1, n0)))
        dst = tuple(slice(max(0, o), s - max(0, -o)) for o, s in zip(off, (n2, n1, n0)))
        r, c = idx[src].ravel(), idx[dst].ravel()
        v = _move(np.full(r.size, b), rng.integers(-ulps, ulps + 1, size=r.size))
        if len(scale_planes):
            v = np.where(np.isin(zpl[r], scale_planes), v * factor, v)
        rows.append(r), cols.append(c), vals.append(v)
        if off != (0, 0, 0):
            rows.append(c), cols.append(r), vals.append(v)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A, base


def _product(dev, A, x, monkeypatch, delta, row0=0):
    """(y, info) of the half-storage product with the delta coding on / off; explicit zeros of A are kept"""
    monkeypatch.setenv("TIGAR_SYMGRID_DELTA", "1" if delta else "0")
    y, info = dev.DeviceCSR.from_scipy(A).mult_symgrid(dev.DeviceVector(data=x), row0=row0)
    monkeypatch.delenv("TIGAR_SYMGRID_DELTA")
    return (None if y is None else y.get_local()), info


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def _interior_parts(info, planes, n2g, reach):
    """parts of the planes that are at least 2 reach from either z face of the grid (every plane holds as many parts)"""
    inner = sum(1 for z in planes if 2 * reach <= z < n2g - 2 * reach)
    return info["parts"] // len(planes) * inner


@pytest.mark.parametrize("shape,reach,chunks", [((41, 33, 29), 3, "0"), ((41, 33, 29), 3, "1"), ((41, 33, 29), 3, "4"),
                                                ((25, 17, 20), 2, "0"), ((49, 35, 23), 2, "3"), ((16, 50, 21), 1, "2"),
                                                ((73, 18, 30), 1, "5"), ((47, 45, 37), 3, "6")])
def test_compressible_matrix_same_bits_as_the_plain_plan(dev, shape, reach, chunks, monkeypatch):
    rng = np.random.default_rng(sum(shape) * 7 + reach)
    A, _ = _repeated_stencil(rng, shape, reach)
    assert abs(A - A.T).max() == 0.0
    x = rng.standard_normal(A.shape[0])
    monkeypatch.setenv("TIGAR_SYMGRID_CHUNKS", chunks)
    y1, info = _product(dev, A, x, monkeypatch, True)
    y0, info0 = _product(dev, A, x, monkeypatch, False)
    assert info is not None and info0 is not None, "a symmetric box stencil was declined"
    assert info["compressed"] and not info0["compressed"] and info0["compressed_share"] == 0
    inner = _interior_parts(info, range(shape[2]), shape[2], reach)
    print("shape %s reach %d: %d of %d parts compressed (interior planes: %d), largest fitting distance %d, reference plane %d"
          % (shape, reach, info["parts_compressed"], info["parts"], inner, info["max_fit_distance"], info["reference_plane"]))
    assert inner > 0 and info["parts_compressed"] > 0.8 * inner
    assert info["reference_plane"] == shape[2] // 2
    assert _same_bits(y1, y0)
    ref, scale = A @ x, np.abs(A) @ np.abs(x)
    assert np.max(np.abs(y1 - ref) / scale) < 1e-14
    # the accounting: value_bytes stays the fp64 half-storage figure, the HBM figure is smaller
    npos = ((2 * reach + 1) ** 3 + 1) // 2
    assert info["value_bytes"] == info0["value_bytes"] == A.shape[0] * ((npos + 1) // 2) * 16
    assert info0["hbm_value_bytes"] == info0["value_bytes"]
    assert info["hbm_value_bytes"] == info["value_bytes"] // 4 + info["pool_bytes"] + info["template_bytes"]


@pytest.mark.parametrize("shape,reach,cuts", [((20, 18, 40), 2, (0, 13, 27, 40)), ((26, 17, 48), 3, (0, 15, 31, 48)),
                                              ((16, 33, 24), 1, (0, 8, 16, 24))])
def test_compressible_z_slabs_same_bits_as_the_plain_plan(dev, shape, reach, cuts, monkeypatch):
    """several ranks: every slab (row0 > 0 for all but the first) takes its own reference plane -- the plane of the slab
    nearest the middle of the grid"""
    rng = np.random.default_rng(sum(shape) * reach)
    A, _ = _repeated_stencil(rng, shape, reach)
    x = rng.standard_normal(A.shape[0])
    n01, n2g = shape[0] * shape[1], shape[2]
    ref_all, scale = A @ x, np.abs(A) @ np.abs(x)
    for z0, z1 in zip(cuts[:-1], cuts[1:]):
        r0, r1 = z0 * n01, z1 * n01
        B = A[r0:r1].tocsr()
        B.sort_indices()
        y1, info = _product(dev, B, x, monkeypatch, True, row0=r0)
        y0, info0 = _product(dev, B, x, monkeypatch, False, row0=r0)
        assert info is not None and info0 is not None, (z0, z1)
        assert info["compressed"], (z0, z1)
        assert info["reference_plane"] == min(max(n2g // 2, z0), z1 - 1), (z0, z1)
        inner = _interior_parts(info, range(z0, z1), n2g, reach)
        print("slab %d..%d: %d of %d parts compressed (interior planes: %d)" % (z0, z1, info["parts_compressed"], info["parts"], inner))
        assert inner > 0 and info["parts_compressed"] > 0.8 * inner, (z0, z1)
        assert _same_bits(y1, y0), (z0, z1)
        assert np.max(np.abs(y1 - ref_all[r0:r1]) / scale[r0:r1]) < 1e-14, (z0, z1)


# ---- the edges of the fit rule: d = int64(v) - int64(t) in two's complement fits iff -32768 <= d <= 32767
_EDGE_SHAPE, _EDGE_REACH = (26, 18, 30), 2


def _set_sym(A, i, j, v):
    """A[i, j] = A[j, i] = v in place (the entries exist: the pattern, explicit zeros included, stays what it is)"""
    for r, c in ((i, j), (j, i)):
        lo, hi = A.indptr[r], A.indptr[r + 1]
        k = lo + int(np.searchsorted(A.indices[lo:hi], c))
        assert A.indices[k] == c
        A.data[k] = v


def _get(A, i, j):
    lo, hi = A.indptr[i], A.indptr[i + 1]
    k = lo + int(np.searchsorted(A.indices[lo:hi], j))
    assert A.indices[k] == j
    return A.data[k]


def _edge_cases():
    # (name, value as a function of the reference plane's value t, template value forced to (None: left), fits)
    mv = lambda k: (lambda t: float(_move(t, k)))
    return [("plus_32767", mv(32767), None, True), ("minus_32768", mv(-32768), None, True),
            ("plus_32768", mv(32768), None, False), ("minus_32769", mv(-32769), None, False),
            ("sign_flip", lambda t: -t, None, False),
            ("zero_vs_nonzero", lambda t: 0.0, None, False), ("negzero_vs_nonzero", lambda t: -0.0, None, False),
            ("zero_vs_zero", lambda t: 0.0, 0.0, True), ("negzero_vs_zero", lambda t: -0.0, 0.0, False),
            ("subnormal_vs_nonzero", lambda t: 3e-320, None, False), ("subnormal_vs_zero", lambda t: 3e-320, 0.0, True),
            ("subnormal_vs_subnormal_far", lambda t: 5e-324 * 40000, 5e-324, False)]


@pytest.mark.parametrize("case", range(len(_edge_cases()) + 1))
def test_edges_of_the_fit_rule(dev, case, monkeypatch):
    """single entries of a plane other than the reference plane set to exact distances from the reference plane's value
    (and to signs, zeros and subnormals): the product equals the plain plan's bit for bit, and exactly the parts that hold
    a distance beyond int16 leave the compressed set.  The last case applies all of them at once."""
    rng = np.random.default_rng(77)
    A, _ = _repeated_stencil(rng, _EDGE_SHAPE, _EDGE_REACH)
    n0, n1, n2 = _EDGE_SHAPE
    x = rng.standard_normal(A.shape[0])
    _, info_base = _product(dev, A, x, monkeypatch, True)
    assert info_base["compressed"]
    zref = info_base["reference_plane"]
    assert zref == n2 // 2
    cases = _edge_cases()
    todo = list(range(len(cases))) if case == len(cases) else [case]
    misfits = 0
    for q in todo:
        name, fv, tforce, fits = cases[q]
        # every case in a plane of its own (below the reference plane, whole boxes), at another (ix, iy)
        zt = 1 + q
        assert zt + 1 < zref
        ix, iy = 3 + (q * 5) % (n0 - 8), 2 + (q * 3) % (n1 - 6)
        off = (1, (q % 3) - 1, (q % 5) - 2) if q % 2 else (0, 1, (q % 5) - 2)
        row = lambda z: (z * n1 + iy) * n0 + ix
        shift = (off[0] * n1 + off[1]) * n0 + off[2]
        if tforce is not None:
            _set_sym(A, row(zref), row(zref) + shift, tforce)
            # (the other planes now differ from the template at this place: they are put at the template's value as well,
            #  so that the only part whose fit is in question is the one aimed at)
            for z in range(n2 - off[0]):
                if z != zref:
                    _set_sym(A, row(z), row(z) + shift, tforce)
        t = _get(A, row(zref), row(zref) + shift)
        _set_sym(A, row(zt), row(zt) + shift, fv(t))
        misfits += 0 if fits else 1
    assert abs(A - A.T).max() == 0.0
    y1, info = _product(dev, A, x, monkeypatch, True)
    y0, info0 = _product(dev, A, x, monkeypatch, False)
    assert info is not None and info["compressed"] and not info0["compressed"]
    assert _same_bits(y1, y0)
    assert info["parts_compressed"] == info_base["parts_compressed"] - misfits, (info["parts_compressed"], info_base["parts_compressed"])
    ref, scale = A @ x, np.abs(A) @ np.abs(x)
    assert np.max(np.abs(y1 - ref) / scale) < 1e-14


def test_pool_overflow_and_unsuitable_matrices_keep_the_plain_plan(dev, monkeypatch):
    rng = np.random.default_rng(5)
    shape, reach = (30, 22, 24), 2
    n2 = shape[2]
    # the reference plane and the one next to it alike (the probe passes), 16 of 24 planes (the two truncated ones at the top included) unlike them: more parts misfit
    # than the pool (a quarter of the parts) holds
    far = [z for z in range(n2) if z % 2 == 1 and z not in (n2 // 2, n2 // 2 + 1)] + [0, 2, 4, 6]
    A, _ = _repeated_stencil(rng, shape, reach, scale_planes=far)
    assert abs(A - A.T).max() == 0.0
    x = rng.standard_normal(A.shape[0])
    y1, info = _product(dev, A, x, monkeypatch, True)
    y0, info0 = _product(dev, A, x, monkeypatch, False)
    assert info is not None and not info["compressed"] and info["compressed_share"] == 0
    assert info["value_bytes"] == info0["value_bytes"] == info["hbm_value_bytes"]
    assert _same_bits(y1, y0)
    ref, scale = A @ x, np.abs(A) @ np.abs(x)
    assert np.max(np.abs(y1 - ref) / scale) < 1e-14
    # fewer misfitting planes than the pool holds: coded, the misfits in the pool
    A2, _ = _repeated_stencil(rng, shape, reach, scale_planes=[1, 5, 20])
    y1, info = _product(dev, A2, x, monkeypatch, True)
    y0, _ = _product(dev, A2, x, monkeypatch, False)
    assert info["compressed"] and info["pool_bytes"] > 0 and _same_bits(y1, y0)
    assert info["parts"] - info["parts_compressed"] <= info["pool_capacity_parts"]
    # values without any likeness between the planes: not attempted
    R, _ = _repeated_stencil(rng, shape, reach)
    R.data[:] = rng.standard_normal(R.nnz)
    R = ((R + R.T) * 0.5).tocsr()
    R.sort_indices()
    y1, info = _product(dev, R, x, monkeypatch, True)
    y0, _ = _product(dev, R, x, monkeypatch, False)
    assert info is not None and not info["compressed"] and info["compressed_share"] == 0
    assert _same_bits(y1, y0)


def test_cg_solve_through_the_api_same_bits_with_and_without_the_coding(dev, monkeypatch):
    """a uniform p = 3 patch: ``solveLinearSystem`` with the coding on and off -- the same iteration count, the same U bit for
    bit; the plan of this K is delta-coded (its share is recorded, not bounded: it is a property of the spline K)"""
    import tigar_amd as t
    from tigar_amd import BSplines as B, forms as F
    p, nel = 3, (20, 20, 60)
    kv = [B.uniformKnots(p, 0., 1., n) for n in nel]
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * 3, kv))
    s0 = gen.getScalarSpline(0)
    for direction in range(3):
        for side in (0, 1):
            gen.addZeroDofs(0, s0.getSideDofs(direction, side))
    spline = t.ExtractedSpline(gen, 2 * p)
    K = spline.assembleMatrix(F.LaplaceForm())
    rhs = spline.assembleVector(F.SeparableLoadForm([lambda x: np.sin(np.pi * x)] * 3, scale=3 * np.pi ** 2))
    monkeypatch.setenv("TIGAR_SPMV_SYM", "2")
    monkeypatch.setenv("TIGAR_KSP_PERSISTENT", "0")
    monkeypatch.setenv("TIGAR_SYMGRID_DELTA", "1")
    _, info = K.mult_symgrid()
    assert info is not None and info["compressed"]
    print("spline K, p = 3, %s elements: compressed share %.4f (%d of %d parts), largest fitting distance %d"
          % (nel, info["compressed_share"], info["parts_compressed"], info["parts"], info["max_fit_distance"]))
    assert info["compressed_share"] > 0
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("TIGAR_SYMGRID_DELTA", mode)
        solver = t.PETScKrylovSolver("cg", "jacobi")
        solver.parameters["relative_tolerance"] = 1e-9
        spline.setSolverOptions(linearSolver=solver)
        c0 = dev.prof_get(7)[1]
        U = spline.solveLinearSystem(K, rhs, t.Function(spline.V))
        assert dev.prof_get(7)[1] - c0 == 1          # (the half-storage copy multiplied)
        assert solver.last["status"] == 0
        out[mode] = (solver.last["iterations"], U.get_local().copy())
    assert out["1"][0] == out["0"][0]
    assert _same_bits(out["1"][1], out["0"][1])
