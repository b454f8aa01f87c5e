"""-m gpu: how the scalar half-storage product (csrc/tg_symgrid.hip) fills the chip.  One wave per workgroup, the two window
rings in static LDS: the LDS of a workgroup decides how many of the four SIMDs of a CU hold a wave, and the number of z chunks
decides how full the last round of waves is.  Guarded here: at least four workgroups per CU for every radius and plan kind
(``device.symgrid_occupancy``), the products at the edges of the patch size, the chunk chooser against its own cost model,
and a CG solve through the API."""
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


def _box_stencil(rng, shape, reach):
    """random symmetric box-stencil matrix on an (n0, n1, n2) grid (x fastest), truncated at the boundary, general CSR"""
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape[::-1])
    rows, cols = [], []
    for off in itertools.product(*[range(-reach, reach + 1)] * 3):
        src = [slice(max(0, -o), s - max(0, o)) for o, s in zip(off[::-1], shape[::-1])]
        dst = [slice(max(0, o), s - max(0, -o)) for o, s in zip(off[::-1], shape[::-1])]
        rows.append(idx[tuple(src)].ravel())
        cols.append(idx[tuple(dst)].ravel())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sp.csr_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(n, n))
    A = (A + A.T).tocsr()
    A.sort_indices()
    return A


def _repeated_stencil(rng, shape, reach, ulps=3000):
    """ONE random symmetric stencil repeated over the grid, every stored value moved by a random number of ulps in +-ulps
    (upper triangle, mirrored): the planes are alike up to rounding, which is what the delta coding takes"""
    n0, n1, n2 = shape
    n = n0 * n1 * n2
    idx = np.arange(n).reshape(n2, n1, n0)
    rows, cols, vals = [], [], []
    for off in (o for o in itertools.product(range(-reach, reach + 1), repeat=3) if o >= (0, 0, 0)):
        b = rng.standard_normal()
        src = tuple(slice(max(0, -o), s - max(0, o)) for o, s in zip(off, (n2, n1, n0)))
        dst = tuple(slice(max(0, o), s - max(0, -o)) for o, s in zip(off, (n2, n1, n0)))
        r, c = idx[src].ravel(), idx[dst].ravel()
        v = (np.full(r.size, b).view(np.int64) + rng.integers(-ulps, ulps + 1, size=r.size)).view(np.float64)
        rows.append(r), cols.append(c), vals.append(v)
        if off != (0, 0, 0):
            rows.append(c), cols.append(r), vals.append(v)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def _product(dev, dA, dx, monkeypatch, delta):
    monkeypatch.setenv("TIGAR_SYMGRID_DELTA", "1" if delta else "0")
    y, info = dA.mult_symgrid(dx)
    monkeypatch.delenv("TIGAR_SYMGRID_DELTA")
    assert info is not None, "a symmetric box stencil was declined"
    return y.get_local(), info


@pytest.mark.parametrize("coded", [True, False])
@pytest.mark.parametrize("reach", [1, 2, 3])
def test_every_simd_of_a_cu_holds_a_wave(dev, reach, coded):
    """the regression guard: a few hundred bytes of LDS more in the product kernel cost a SIMD of every CU"""
    occ = dev.symgrid_occupancy(reach, coded)
    print("radius %d, %s plan: %d workgroups per CU, %d B of static LDS, %d places on %d CUs, patches of %d x %d"
          % (reach, "coded" if coded else "plain", occ["workgroups_per_cu"], occ["lds_bytes"], occ["places"], occ["num_cu"],
             occ["patch"][0], occ["patch"][1]))
    assert occ["workgroups_per_cu"] >= 4
    assert occ["num_cu"] == dev.device_info()["num_cu"]
    assert occ["places"] == occ["workgroups_per_cu"] * occ["num_cu"]
    assert 0 < occ["lds_bytes"] <= 160 * 1024 // 4


def _edge_grids(dev, reach):
    px, py = dev.symgrid_occupancy(reach)["patch"]
    return px, py, (px - 1, px, px + 1, 2 * px + 1), (16, py + 1, 2 * py + 1), (2 * reach + 2, 13, 29)


@pytest.mark.parametrize("k1", [0, 1, 2])
@pytest.mark.parametrize("k0", [0, 1, 2, 3])
@pytest.mark.parametrize("reach", [1, 2, 3])
def test_products_at_the_edges_of_the_patch_size(dev, reach, k0, k1, monkeypatch):
    """n0 in {PX - 1, PX, PX + 1, 2 PX + 1}, n1 in {16, PY + 1, 2 PY + 1}, n2 in {2 P + 2, 13, 29}: a patch of exactly one
    sub-step, of one row more than whole sub-steps, a last sub-step of a single row.  A random matrix (the plain plan) and
    one whose planes are alike (the coded plan) against scipy -- |y - A x| <= 1e-14 |A| |x| --, the coded product against the
    plain one and every product against its second run bit for bit."""
    px, py, n0s, n1s, n2s = _edge_grids(dev, reach)
    n0, n1 = n0s[k0], n1s[k1]
    assert n0 >= 16 and n1 >= 16
    for n2 in n2s:
        shape = (n0, n1, n2)
        rng = np.random.default_rng(1000 * reach + 100 * k0 + 10 * k1 + n2)
        x = rng.standard_normal(n0 * n1 * n2)
        dx = dev.DeviceVector(data=x)
        # the plain plan on a random matrix
        A = _box_stencil(rng, shape, reach)
        dA = dev.DeviceCSR.from_scipy(A)
        y, info = dA.mult_symgrid(dx)
        assert info is not None, ("declined", shape)
        ref, scale = A @ x, np.abs(A) @ np.abs(x)
        err = np.max(np.abs(y.get_local() - ref) / scale)
        y2, _ = dA.mult_symgrid(dx)
        # the coded plan on planes that are alike
        R = _repeated_stencil(rng, shape, reach)
        dR = dev.DeviceCSR.from_scipy(R)
        y1, info1 = _product(dev, dR, dx, monkeypatch, True)
        y0, info0 = _product(dev, dR, dx, monkeypatch, False)
        y1b, _ = _product(dev, dR, dx, monkeypatch, True)
        refr, scaler = R @ x, np.abs(R) @ np.abs(x)
        err1 = np.max(np.abs(y1 - refr) / scaler)
        print("radius %d grid %s (patch %d x %d): plain %.2e, coded %.2e of |A||x|, coded plan: %s, %d chunks"
              % (reach, shape, px, py, err, err1, info1["compressed"], info1["chunks"]))
        assert err < 1e-14, shape
        assert _same_bits(y.get_local(), y2.get_local()), shape
        assert not info0["compressed"]
        if n2 == 29:          # (fewer planes: the truncated rows at the z faces are more than the pool of misfits holds)
            assert info1["compressed"], shape
        assert err1 < 1e-14, shape
        assert _same_bits(y1, y0), shape
        assert _same_bits(y1, y1b), shape
        if n2 == 29:          # the coded kernel with chunks of unequal length (14 + 15; 9 + 10 + 10 planes)
            for k in (2, 3):
                monkeypatch.setenv("TIGAR_SYMGRID_CHUNKS", str(k))
                yk1, infok = _product(dev, dR, dx, monkeypatch, True)
                yk0, _ = _product(dev, dR, dx, monkeypatch, False)
                monkeypatch.delenv("TIGAR_SYMGRID_CHUNKS")
                assert infok["compressed"] and infok["chunks"] == k, (shape, k)
                assert np.max(np.abs(yk1 - refr) / scaler) < 1e-14, (shape, k)
                assert _same_bits(yk1, yk0), (shape, k)


_CHUNK_START = 0.5          # planes a chunk pays for its start (csrc/tg_symgrid.hip, SG_CHUNK_START)


def _model_cost(npatch, c, n2, places):
    """the cost model of the chunk chooser, restated: rounds of waves x planes a wave walks (its chunk and its start)"""
    return -(-npatch * c // places) * (n2 / c + _CHUNK_START)


@pytest.mark.parametrize("grid", [(259, 259, 259), (259, 259, 67), (259, 259, 35), (64, 64, 64)])
@pytest.mark.parametrize("coded", [True, False])
@pytest.mark.parametrize("reach", [1, 2, 3])
def test_chunk_chooser_minimises_its_model(dev, reach, coded, grid, monkeypatch):
    """each plan kind against the model with its OWN places (the two kernels need not hold as many waves)"""
    monkeypatch.delenv("TIGAR_SYMGRID_CHUNKS", raising=False)
    n0, n1, n2 = grid
    occ = dev.symgrid_occupancy(reach, coded, grid)
    px, py = occ["patch"]
    npatch = -(-n0 // px) * -(-n1 // py)
    cmax = max(1, n2 // max(reach, 4))
    costs = {c: _model_cost(npatch, c, n2, occ["places"]) for c in range(1, cmax + 1)}
    chosen = occ["chunks"]
    print("radius %d (%s) grid %s: %d patches on %d places, %d chunks (cost %.2f; least %.2f)"
          % (reach, "coded" if coded else "plain", grid, npatch, occ["places"], chosen, costs[chosen], min(costs.values())))
    assert 1 <= chosen <= cmax
    assert costs[chosen] <= min(costs.values()) + 1e-9


@pytest.mark.parametrize("reach,grid", [(3, (64, 64, 64)), (2, (40, 33, 67)), (1, (64, 48, 35))])
def _builder_kind(dev, reach, delta):
    """(workgroups per CU, plan kind) the builder plans with: the plain kernel's figure, or -- the coding is tried first and
    may be declined -- the fewer of the two"""
    plain = dev.symgrid_occupancy(reach, False)["workgroups_per_cu"]
    coded = dev.symgrid_occupancy(reach, True)["workgroups_per_cu"]
    return (coded, True) if delta and coded <= plain else (plain, False)


def _check_last_plan(dev, reach, delta, chunks):
    """the places the BUILDER used for the plan built last (not the export's own product) = the occupancy query x CUs"""
    per_cu, _ = _builder_kind(dev, reach, delta)
    last = dev.symgrid_last_plan()
    assert last is not None and last["reach"] == reach and last["chunks"] == chunks
    assert last["workgroups_per_cu"] == per_cu and per_cu >= 4
    assert last["places"] == per_cu * dev.device_info()["num_cu"]


@pytest.mark.parametrize("reach,grid", [(3, (64, 64, 64)), (2, (40, 33, 67)), (1, (64, 48, 35))])
def test_chosen_chunks_are_those_of_the_plan_and_the_override_stands(dev, reach, grid, monkeypatch):
    """the plan that is built has the chunks the chooser names and was planned for workgroups per CU x CUs places (no
    matrix of 259^3 rows for that: the builder calls the same chooser at every size, and reports the places it handed it),
    and TIGAR_SYMGRID_CHUNKS = k forces k, capped at n2 / max(P, 4)"""
    monkeypatch.delenv("TIGAR_SYMGRID_CHUNKS", raising=False)
    rng = np.random.default_rng(reach + sum(grid))
    A = _repeated_stencil(rng, grid, reach)
    x = rng.standard_normal(A.shape[0])
    dA, dx = dev.DeviceCSR.from_scipy(A), dev.DeviceVector(data=x)
    ref, scale = A @ x, np.abs(A) @ np.abs(x)
    for delta in (True, False):
        y, info = _product(dev, dA, dx, monkeypatch, delta)
        assert info["compressed"] == delta
        assert info["chunks"] == dev.symgrid_occupancy(reach, _builder_kind(dev, reach, delta)[1], grid)["chunks"]
        _check_last_plan(dev, reach, delta, info["chunks"])
        assert np.max(np.abs(y - ref) / scale) < 1e-14
    cmax = grid[2] // max(reach, 4)
    for k in (1, 3, cmax, cmax + 5):
        monkeypatch.setenv("TIGAR_SYMGRID_CHUNKS", str(k))
        assert dev.symgrid_occupancy(reach, True, grid)["chunks"] == min(k, cmax)
        y, info = _product(dev, dA, dx, monkeypatch, True)
        assert info["chunks"] == min(k, cmax)
        assert np.max(np.abs(y - ref) / scale) < 1e-14


def test_cg_solve_through_the_api(dev, monkeypatch):
    """p = 3 on 20 x 20 x 40 elements (a small patch on which the solve takes the half-storage copy, with enough planes that
    those at the z faces -- which are unlike the reference plane -- fit the pool, so that the plan IS coded): converges to
    rtol, the same iteration count and the same U bit for bit with the coding on and off"""
    import tigar_amd as t
    from tigar_amd import BSplines as B, forms as F
    p, nel, rtol = 3, (20, 20, 40), 1e-9
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
    Ks, b = K.to_scipy(), rhs.get_local()
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("TIGAR_SYMGRID_DELTA", mode)
        solver = t.PETScKrylovSolver("cg", "jacobi")
        solver.parameters["relative_tolerance"] = rtol
        spline.setSolverOptions(linearSolver=solver)
        c0 = dev.prof_get(7)[1]
        U = spline.solveLinearSystem(K, rhs, t.Function(spline.V))
        assert dev.prof_get(7)[1] - c0 == 1          # (the half-storage copy multiplied)
        assert solver.last["status"] == 0
        # (the solver's own plan: built for the places the occupancy query gives, with the chunks the chooser names)
        n0, n1, n2 = (n + p for n in nel)
        _check_last_plan(dev, p, mode == "1",
                         dev.symgrid_occupancy(p, _builder_kind(dev, p, mode == "1")[1], (n0, n1, n2))["chunks"])
        out[mode] = (solver.last["iterations"], U.get_local().copy())
    its, U1 = out["1"]
    # the solver stops at ||B r_k|| <= rtol ||B b|| (B = 1 / diag K) on the residual of its recurrence; the residual
    # computed from U differs from that one by the rounding of ~its products, orders below rtol: a factor 2 covers it
    d = Ks.diagonal()
    res = np.linalg.norm((b - Ks @ U1) / d) / np.linalg.norm(b / d)
    print("p = 3, %s elements: %d iterations, preconditioned relative residual %.3e" % (nel, its, res))
    assert res < 2 * rtol
    assert out["0"][0] == its
    assert _same_bits(U1, out["0"][1])
