"""GPU: time integration (tigar_amd/timeIntegration.py, csrc/tg_timeint.hip) -- the three kernels against numpy / scipy data
in longdouble with bounds from the arithmetic they do, the integrators against their own expressions, and the driver
``LinearTransientProblem`` against the dense longdouble recurrence of tests/timeint_reference.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import timeint_reference as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
LD = R.LD
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 100003]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dv(a):
    from tigar_amd.device import DeviceVector
    return DeviceVector(data=np.asarray(a, dtype=np.float64))


def _spline(d, p, nels):
    """one clamped tensor-product patch on the unit box"""
    import tigar_amd as t
    from tigar_amd import BSplines as B
    kv = [B.uniformKnots(p, 0.0, 1.0, n) for n in nels]
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * d, kv))
    sc = gen.getScalarSpline(0)
    for direction in range(d):
        for side in (0, 1):
            gen.addZeroDofs(0, sc.getSideDofs(direction, side))
    return t.ExtractedSpline(gen, 2 * p)


# ---- 1. tg_vec_lincomb ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_vec_lincomb(n, k):
    from tigar_amd import device as dev
    rng = np.random.default_rng(100 * k + n % 97)
    vs = [rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4) for _ in range(k)]
    coef = rng.standard_normal(k) * 3.0
    want = sum(LD(c) * v.astype(LD) for c, v in zip(coef, vs))
    bound = k * EPS * sum(np.abs(c * v) for c, v in zip(coef, vs))
    first = None
    for where in ("fresh", "first", "last"):
        dvs = [_dv(v) for v in vs]
        out = {"fresh": dev.DeviceVector(n), "first": dvs[0], "last": dvs[-1]}[where]
        got = dev.vec_lincomb(out, coef, dvs).get_local()
        assert np.all(np.abs(got - want) <= bound), "out = %s" % where
        for j, v in enumerate(dvs):                          # the other inputs are untouched
            if v is not out:
                assert np.array_equal(_bits(v.get_local()), _bits(vs[j]))
        if first is None:
            first = got
            again = dev.vec_lincomb(dev.DeviceVector(n), coef, dvs).get_local()
            assert np.array_equal(_bits(again), _bits(first)), "two runs differ in bits"
        else:
            assert np.array_equal(_bits(got), _bits(first)), "aliasing the output changed the bits"


def test_vec_lincomb_refusals():
    from tigar_amd import device as dev
    from tigar_amd._lib import TigarHipError
    out = dev.DeviceVector(5)
    vs = [dev.DeviceVector(5) for _ in range(9)]
    with pytest.raises(TigarHipError):
        dev.vec_lincomb(out, [], [])
    with pytest.raises(TigarHipError):
        dev.vec_lincomb(out, np.ones(9), vs)
    with pytest.raises(TigarHipError):
        dev.vec_lincomb(out, [1.0, 2.0], [vs[0], dev.DeviceVector(6)])
    dev.vec_lincomb(out, np.ones(8), vs[:8])                 # (the library is usable after a refusal)


def test_linear_combination_evaluate_chunks():
    """more than 8 terms: chunks of 8, then 7 with the accumulator; the output may be one of the late terms"""
    from tigar_amd.timeIntegration import LinearCombination as LC
    rng = np.random.default_rng(11)
    n, k = 1001, 19
    vs = [rng.standard_normal(n) for _ in range(k)]
    coef = rng.standard_normal(k)
    want = sum(LD(c) * v.astype(LD) for c, v in zip(coef, vs))
    bound = (k + 3) * EPS * sum(np.abs(c * v) for c, v in zip(coef, vs))
    dvs = [_dv(v) for v in vs]
    e = LC(list(zip(coef, dvs)))
    assert np.all(np.abs(e.evaluate().get_local() - want) <= bound)
    out = e.evaluate(out=dvs[12])
    assert out is dvs[12] and np.all(np.abs(out.get_local() - want) <= bound)


# ---- 2. tg_state_advance ----------------------------------------------------------------------------------------------
def _advance_reference(c, x, xo, vo, ao):
    """(v, a, bound_v, bound_a, mag_v, mag_a) in longdouble: the values, the elementwise bounds of the kernel's arithmetic
    (4 eps sum |terms| for v; |c4| times that plus 3 eps sum |terms of a| for a) and the sums of the magnitudes of the terms
    (for a: with v expanded into its own terms)"""
    c = [LD(v) for v in c]
    tv = [c[0] * x.astype(LD), c[1] * xo.astype(LD), c[2] * vo.astype(LD)] + ([c[3] * ao.astype(LD)] if ao is not None else [])
    v = sum(tv)
    mv = sum(np.abs(t) for t in tv).astype(np.float64)
    bv = 4 * EPS * mv
    if ao is None:
        return v, None, bv, None, mv, None
    ta = [c[4] * v, c[5] * vo.astype(LD), c[6] * ao.astype(LD)]
    ba = float(abs(c[4])) * bv + 3 * EPS * sum(np.abs(t) for t in ta).astype(np.float64)
    ma = float(abs(c[4])) * mv + (np.abs(ta[1]) + np.abs(ta[2])).astype(np.float64)
    return v, sum(ta), bv, ba, mv, ma


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_state_advance(n, order):
    from tigar_amd import device as dev
    rng = np.random.default_rng(7 * n % 1000 + order)
    x, xo, vo, ao = (rng.standard_normal(n) * s for s in (1.0, 1.0, 30.0, 900.0))
    c = rng.standard_normal(7) * np.array([50.0, 50.0, 1.0, 0.01, 40.0, 40.0, 1.0])
    dx, dxo, dvo, dao = _dv(x), _dv(xo), _dv(vo), _dv(ao)
    dev.state_advance(c, dx, dxo, dvo, dao if order == 2 else None)
    v, a, bv, ba, _, _ = _advance_reference(c, x, xo, vo, ao if order == 2 else None)
    assert np.array_equal(_bits(dx.get_local()), _bits(x)), "x was written"
    assert np.array_equal(_bits(dxo.get_local()), _bits(x)), "x_old is not x bit for bit"
    assert np.all(np.abs(dvo.get_local() - v) <= bv)
    if order == 2:
        assert np.all(np.abs(dao.get_local() - a) <= ba)
    else:
        assert np.array_equal(_bits(dao.get_local()), _bits(ao)), "order 1 touched the acceleration"


def test_state_advance_refusals():
    from tigar_amd import device as dev
    from tigar_amd._lib import TigarHipError, lib
    a, b, c, d = (dev.DeviceVector(9) for _ in range(4))
    cs = np.ones(7)
    for args in ((a, a, c, d), (a, b, a, d), (a, b, c, a), (a, b, b, d), (a, b, c, b), (a, b, c, c), (a, b, b, None), (a, a, c, None)):
        with pytest.raises(TigarHipError):
            dev.state_advance(cs, *args)
    with pytest.raises(TigarHipError):
        dev.state_advance(cs, a, b, c, dev.DeviceVector(8))
    L = lib()
    cp = cs.ctypes.data_as(C.POINTER(C.c_double))
    assert L.tg_state_advance(3, cp, a._h, b._h, c._h, d._h) == 2
    assert L.tg_state_advance(2, cp, a._h, b._h, c._h, None) == 2
    assert L.tg_state_advance(1, cp, a._h, b._h, c._h, d._h) == 2
    dev.state_advance(cs, a, b, c, d)


# ---- 3. tg_spmv_pair --------------------------------------------------------------------------------------------------
def _pair_reference(A, B, xa, xb, y0):
    """(y0 - A xa - B xb in longdouble, the bound per row) for scipy CSR matrices on one pattern"""
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    ta = A.data.astype(LD) * xa[A.indices].astype(LD)
    tb = B.data.astype(LD) * xb[B.indices].astype(LD)
    s = np.zeros(n, dtype=LD)
    np.add.at(s, rows, ta + tb)
    mag = np.zeros(n, dtype=np.float64)
    np.add.at(mag, rows, (np.abs(ta) + np.abs(tb)).astype(np.float64))
    y0v = np.zeros(n) if y0 is None else y0
    length = np.diff(A.indptr)
    return y0v.astype(LD) - s, (2 * length + 3) * EPS * (np.abs(y0v) + mag)


def _check_pair(dA, dB, seed=0):
    """all three ways of passing y0 on one pair of device matrices"""
    from tigar_amd import device as dev
    A, B = dA.to_scipy(), dB.to_scipy()
    nr, nc = A.shape
    rng = np.random.default_rng(seed)
    xa, xb, y0 = rng.standard_normal(nc), rng.standard_normal(nc), rng.standard_normal(nr)
    pair = dev.CSRPair(dA, dB)
    dxa, dxb = _dv(xa), _dv(xb)
    want, bound = _pair_reference(A, B, xa, xb, y0)
    y = _dv(np.full(nr, 7.0))
    assert pair.mult(dxa, dxb, y0=_dv(y0), y=y) is y
    got = y.get_local()
    assert np.all(np.abs(got - want) <= bound), "y0 given: worst excess %g" % np.max(np.abs(got - want) - bound)
    alias = _dv(y0)
    pair.mult(dxa, dxb, y0=alias, y=alias)
    assert np.array_equal(_bits(alias.get_local()), _bits(got)), "y aliasing y0 changed the result"
    want0, bound0 = _pair_reference(A, B, xa, xb, None)
    got0 = pair.mult(dxa, dxb).get_local()
    assert np.all(np.abs(got0 - want0) <= bound0), "y0 null"
    assert np.array_equal(_bits(dxa.get_local()), _bits(xa)) and np.array_equal(_bits(dxb.get_local()), _bits(xb))
    return got


def _same_pattern(A, seed):
    B = sp.csr_matrix(A).copy()
    B.data = np.random.default_rng(seed).standard_normal(B.nnz)
    return B


def _long_rows(lengths, ncols=5000, seed=3):
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    indices = np.concatenate([np.sort(rng.choice(ncols, size=l, replace=False)) for l in lengths]).astype(np.int32)
    return sp.csr_matrix((rng.standard_normal(indices.size), indices, indptr), shape=(len(lengths), ncols))


def test_spmv_pair_stiffness_and_mass():
    from tigar_amd import forms as F
    spline = _spline(3, 3, (4, 4, 4))
    K, M = spline.assembleMatrix(F.LaplaceForm()), spline.assembleMatrix(F.MassForm())
    assert K.shape == (343, 343)
    _check_pair(M, K, seed=1)


def test_spmv_pair_random_with_empty_rows():
    from tigar_amd.device import DeviceCSR
    A = sp.random(300, 300, density=0.05, random_state=4, format="lil")
    for r in (0, 17, 18, 19, 150, 299):
        A[r, :] = 0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    assert A.indptr[1] == 0 and A.indptr[-1] == A.indptr[-2] and A.nnz > 3000
    _check_pair(DeviceCSR.from_scipy(A), DeviceCSR.from_scipy(_same_pattern(A, 5)), seed=2)


def test_spmv_pair_tiny_and_empty():
    from tigar_amd.device import DeviceCSR
    one = sp.csr_matrix(np.array([[2.5]]))
    _check_pair(DeviceCSR.from_scipy(one), DeviceCSR.from_scipy(sp.csr_matrix(np.array([[-4.0]]))))
    _check_pair(DeviceCSR.from_scipy(one), DeviceCSR.from_scipy(one))
    empty = sp.csr_matrix((5, 5))
    _check_pair(DeviceCSR.from_scipy(empty), DeviceCSR.from_scipy(empty))


@pytest.mark.parametrize("lengths", [(2048, 2049, 4096, 0, 1, 7), (2048, 2049, 4096, 0, 1, 4097)],
                         ids=["stream_plan_edges", "wave_per_row"])
def test_spmv_pair_long_rows(lengths):
    """rows of 2048, 2049 and 4096 entries: the edges at which the row-block plan doubles its stage; one of 4097: no stage
    holds it and the plan goes to a wave per row"""
    from tigar_amd.device import DeviceCSR
    A = _long_rows(lengths)
    _check_pair(DeviceCSR.from_scipy(A), DeviceCSR.from_scipy(_same_pattern(A, 8)), seed=6)


def test_spmv_pair_refusals():
    from tigar_amd import device as dev
    from tigar_amd._lib import TigarHipError, handle, lib
    A = sp.csr_matrix(np.array([[1.0, 2.0, 0.0], [0.0, 3.0, 0.0], [4.0, 0.0, 5.0]]))
    B = sp.csr_matrix(np.array([[1.0, 2.0, 0.0], [0.0, 3.0, 0.0], [0.0, 4.0, 5.0]]))         # same nnz, one other column
    assert A.nnz == B.nnz and np.array_equal(A.indptr, B.indptr)
    dA, dB = dev.DeviceCSR.from_scipy(A), dev.DeviceCSR.from_scipy(B)
    h = handle()
    assert lib().tg_csr_pair_create(dA._h, dB._h, C.byref(h)) == 2
    assert b"do not share one sparsity pattern" in lib().tg_last_error()
    with pytest.raises(ValueError, match="do not share one sparsity pattern"):
        dev.CSRPair(dA, dB)
    Bp = sp.csr_matrix(np.array([[1.0, 0.0, 0.0], [2.0, 3.0, 0.0], [4.0, 0.0, 5.0]]))         # same columns, other row pointer
    with pytest.raises(ValueError):
        dev.CSRPair(dA, dev.DeviceCSR.from_scipy(Bp))
    with pytest.raises(ValueError):
        dev.CSRPair(dA, dev.DeviceCSR.from_scipy(sp.csr_matrix(np.eye(3))))
    pair = dev.CSRPair(dA, dev.DeviceCSR.from_scipy(_same_pattern(A, 1)))
    x, y = dev.DeviceVector(3), dev.DeviceVector(3)
    for args in ((y, x, None, y), (x, y, None, y), (dev.DeviceVector(4), x, None, y), (x, x, dev.DeviceVector(2), y)):
        with pytest.raises(TigarHipError):
            pair.mult(args[0], args[1], y0=args[2], y=args[3])
    pair.mult(x, x, y0=y, y=y)


# ---- 4. integrators ---------------------------------------------------------------------------------------------------
class _Space(object):
    def __init__(self, n):
        self.n = n

    def dim(self):
        return self.n


def _expanded_bound(expr, values):
    """6 eps sum |c_i w_i| of an expression: up to 4 fused terms and the rounding of its merged coefficients"""
    return 6 * EPS * sum(np.abs(c * values[id(v)]) for c, v in expr.terms)


@pytest.mark.parametrize("order,as_functions", [(2, False), (2, True), (1, False)])
def test_generalized_alpha_advance(order, as_functions):
    import tigar_amd as t
    from tigar_amd import timeIntegration as TI
    n = 1003
    rng = np.random.default_rng(order)
    host = [rng.standard_normal(n) * s for s in (1.0, 1.0, 20.0, 400.0)][:order + 2]
    vecs = [_dv(h) for h in host]
    objs = [t.Function(_Space(n), vector=v) for v in vecs] if as_functions else vecs
    it = TI.GeneralizedAlphaIntegrator(0.5, 0.01, objs[0], objs[1:], t=1.0)
    values = {id(o): h for o, h in zip(objs, host)}
    pred = it.sameVelocityPredictor()
    want_pred = sum(LD(c) * values[id(v)].astype(LD) for c, v in pred.terms)
    assert len(pred.terms) == order + (order == 2)
    assert np.all(np.abs(pred.evaluate().get_local() - want_pred) <= _expanded_bound(pred, values))
    ev, eva = it.xdot(), (it.xddot() if order == 2 else None)
    v_before = ev.evaluate().get_local()
    a_before = eva.evaluate().get_local() if order == 2 else None
    c = list(it._xdot_coefficients()) + (list(it._xddot_coefficients()) if order == 2 else [0.0] * 3)
    v, _, bv, ba, _, ma = _advance_reference(c, host[0], host[1], host[2], host[3] if order == 2 else None)
    it.advance()
    assert it.t == 1.0 + 0.01 + 0.01
    assert np.array_equal(_bits(vecs[1].get_local()), _bits(host[0]))
    # xdot() holds the kernel's own four coefficients on four distinct vectors, and tg_vec_lincomb runs the same c0 v0 + fma
    # chain as tg_state_advance: the velocity is the same bits (well inside bv, the bound of test_state_advance)
    assert np.array_equal(_bits(vecs[2].get_local()), _bits(v_before))
    assert np.all(np.abs(vecs[2].get_local() - v) <= bv)
    if order == 2:
        # xddot() is another computation: c4 is multiplied into xdot()'s coefficients and the terms on xdot_old and
        # xddot_old are merged, so each coefficient carries up to two roundings (a product, a sum) and the four terms are
        # fused in one chain: 6 eps on the expanded magnitudes for evaluate(), on top of ba for the kernel
        assert np.all(np.abs(vecs[3].get_local() - a_before) <= ba + 6 * EPS * ma)


@pytest.mark.parametrize("order", [1, 2])
def test_backward_euler_advance(order):
    from tigar_amd import timeIntegration as TI
    n = 515
    rng = np.random.default_rng(20 + order)
    host = [rng.standard_normal(n) for _ in range(order + 1)]
    vecs = [_dv(h) for h in host]
    it = TI.BackwardEulerIntegrator(0.125, vecs[0], vecs[1:], t=0.5)
    v_before = it.xdot().evaluate().get_local()
    assert np.all(np.abs(v_before - (host[0] - host[1]) / 0.125) <= 4 * EPS * (np.abs(host[0]) + np.abs(host[1])) / 0.125)
    it.advance()
    assert it.t == 0.75
    assert np.array_equal(_bits(vecs[1].get_local()), _bits(host[0]))
    if order == 2:
        assert np.array_equal(_bits(vecs[2].get_local()), _bits(v_before))      # (8 x and 8 x_old: the same two products)


# ---- 5. - 8. the driver -----------------------------------------------------------------------------------------------
def _dense(Mdev):
    return Mdev.to_scipy().toarray()


def _state(spline, seed, scale=1.0):
    """a smooth-ish random state that vanishes on the zero dofs"""
    n = spline.M.shape[1]
    v = np.random.default_rng(seed).standard_normal(n) * scale
    v[np.asarray(spline.zeroDofs, dtype=np.int64)] = 0.0
    return v


def _keff_coefficients(order, scheme, rho, dt, damping):
    """(c_K, c_M) in closed form"""
    a_M, a_K = damping if damping is not None else (0.0, 0.0)
    if scheme == "backward_euler":
        return (1.0 + a_K / dt, 1.0 / dt ** 2 + a_M / dt) if order == 2 else (1.0, 1.0 / dt)
    am, af, gamma, beta = R.parameters(rho, order)
    if order == 1:
        return af, am / (gamma * dt)
    c_v, c_a = gamma / (beta * dt), 1.0 / (beta * dt * dt)
    return af * (1.0 + c_v * a_K), am * c_a + af * c_v * a_M


def _trajectory(prob, steps, zero):
    xs = [prob.x.get_local()]
    its = []
    for _ in range(steps):
        prob.step()
        xs.append(prob.x.get_local())
        its.append(prob.last["iterations"])
        assert np.all(xs[-1][zero] == 0.0), "the state is not exactly 0 on the zero dofs"
        if prob.xdot is not None:
            assert np.all(prob.xdot.get_local()[zero] == 0.0)
    return xs, its


def _deviation(xs, ref):
    top = max(float(np.linalg.norm(r)) for r in ref)
    return max(float(np.linalg.norm(a.astype(LD) - r)) for a, r in zip(xs, ref)) / top


def _jacobi(rtol):
    import tigar_amd as t
    s = t.PETScKrylovSolver("cg", "jacobi")
    s.parameters["relative_tolerance"] = rtol
    return s


def _scaled_condition(A):
    d = 1.0 / np.sqrt(np.diag(A))
    return np.linalg.cond(d[:, None] * A * d[None, :])


@pytest.mark.parametrize("fused", [True, False], ids=["pair_product", "two_products"])
def test_driver_right_hand_side_both_ways(fused):
    """``LinearTransientProblem.FUSED_RHS`` chooses between ``tg_spmv_pair`` and two ``tg_spmv`` with two axpy for
    rhs = f - M w_M - K w_K; whichever is the default, both stay correct.  The bound per row is the one of the pair product:
    the composition rounds each product of length len to len eps of its magnitudes and adds two roundings for the two
    subtractions, (len + 2) eps, which the pair's (2 len + 3) eps covers.  The zero dofs of the result are exactly 0."""
    from tigar_amd import forms as F, timeIntegration as TI
    spline = _spline(2, 3, (6, 6))
    spline.setSolverOptions(linearSolver=None)
    prob = TI.LinearTransientProblem(spline, stiffness=F.LaplaceForm(), mass=F.MassForm(), order=2, RHO_INF=0.5, DELTA_T=0.01)
    prob.FUSED_RHS = fused
    n = prob.n
    rng = np.random.default_rng(11)
    wM, wK, f = rng.standard_normal(n), rng.standard_normal(n) * 3.0, rng.standard_normal(n)
    prob._wM[:] = _dv(wM)
    prob._wK[:] = _dv(wK)
    zero = np.asarray(spline.zeroDofs, dtype=np.int64)
    for y0 in (f, None):
        want, bound = _pair_reference(prob.Mm.to_scipy(), prob.K.to_scipy(), wM, wK, y0)
        prob._residual(None if y0 is None else _dv(y0))
        got = prob._rhs.get_local()
        assert np.all(got[zero] == 0.0)
        free = np.setdiff1d(np.arange(n), zero)
        assert np.all(np.abs(got[free] - want[free]) <= bound[free])


def test_driver_wave_2d_against_longdouble():
    """Order 2, generalized-alpha, Rayleigh damping, time-dependent load, 10 steps on a 2-D p = 2 patch of 8 x 8 elements
    (100 dofs), against the dense longdouble recurrence.  B = steps * cond2(K_eff) * 32 eps for the direct solve (a
    backward-stable solve errs by cond * eps times a small polynomial in n per step, 32 being the allowance for it at
    <= 100 unknowns; a scheme with RHO_INF <= 1 does not amplify earlier errors), the float64 numpy recurrence is held to
    B / 8; Jacobi-CG at rtol = 1e-12 (a test on the preconditioned residual relative to ||B b||) to
    steps * cond2(D^-1/2 K_eff D^-1/2) * 4 rtol.
    The deviations are printed before they are asserted (``pytest -s``).  Measured on the MI355X: direct solve 1.80e-14
    against B = 2.31e-10 (float64 numpy recurrence 2.0e-16; xdot 3.9e-14, xddot 4.2e-14 relative at the last step); Jacobi-CG
    2.50e-11 against 1.68e-09, 40-41 iterations per step."""
    from tigar_amd import forms as F, timeIntegration as TI
    spline = _spline(2, 2, (8, 8))
    rho, dt, steps, damping = 0.5, 0.01, 10, (0.1, 0.01)
    shape = lambda s: np.sin(np.pi * s)
    amplitude = lambda t: 1.0 + np.sin(5.0 * t)
    load = lambda t: F.SeparableLoadForm([shape, shape], scale=amplitude(t))
    x0, v0 = _state(spline, 1), _state(spline, 2, 5.0)
    zero = np.asarray(spline.zeroDofs, dtype=np.int64)

    def problem(solver):
        spline.setSolverOptions(linearSolver=solver)
        return TI.LinearTransientProblem(spline, stiffness=F.LaplaceForm(), mass=F.MassForm(), order=2, RHO_INF=rho, DELTA_T=dt,
                                         damping=damping, load=load, x0=_dv(x0), xdot0=_dv(v0), t=0.25)

    prob = problem(None)
    K, M = _dense(prob.K), _dense(prob.Mm)
    assert K.shape == (100, 100)
    f1 = spline.assembleVector(F.SeparableLoadForm([shape, shape], scale=1.0)).get_local()
    c_K, c_M = _keff_coefficients(2, "generalized_alpha", rho, dt, damping)
    assert np.isclose(prob.c_K, c_K, rtol=1e-14) and np.isclose(prob.c_M, c_M, rtol=1e-14)
    Keff = c_K * K + c_M * M
    assert np.allclose(_dense(prob.K_eff), Keff, rtol=1e-14, atol=0)
    kw = dict(order=2, rho_inf=rho, damping=damping, load=lambda t: amplitude(t) * f1, x0=x0, v0=v0, t0=0.25)
    ref = R.integrate(K, M, dt, steps, dtype=LD, **kw)
    B = steps * np.linalg.cond(Keff) * 32 * EPS
    host = _deviation(R.integrate(K, M, dt, steps, dtype=np.float64, **kw)["x"], ref["x"])
    print("direct: bound %.3e, float64 recurrence %.3e" % (B, host))
    assert host <= B / 8
    xs, _ = _trajectory(prob, steps, zero)
    got = _deviation(xs, ref["x"])
    print("direct: device %.3e" % got)
    assert got <= B
    assert np.isclose(prob.t, 0.25 + steps * dt) and prob.steps_done == steps
    assert set(prob.last) == {"iterations", "rhs_seconds", "solve_seconds", "advance_seconds"}
    err_v = np.linalg.norm(prob.xdot.get_local() - ref["v"][-1].astype(np.float64)) / np.linalg.norm(ref["v"][-1].astype(np.float64))
    err_a = np.linalg.norm(prob.xddot.get_local() - ref["a"][-1].astype(np.float64)) / np.linalg.norm(ref["a"][-1].astype(np.float64))
    print("direct: xdot %.3e xddot %.3e" % (err_v, err_a))
    u = prob.prolong().vector().get_local()
    assert np.allclose(u, spline.M.to_scipy() @ xs[-1], rtol=0, atol=1e-13 * np.max(np.abs(u)))
    e = R.energy(K, M, ref["x"][-1].astype(np.float64), ref["v"][-1].astype(np.float64))
    assert np.isclose(prob.energy(), e, rtol=1e-9)

    rtol = 1e-12
    solver = _jacobi(rtol)
    probj = problem(solver)
    Bj = steps * _scaled_condition(Keff) * 4 * rtol
    xsj, its = _trajectory(probj, steps, zero)
    gotj = _deviation(xsj, ref["x"])
    print("Jacobi-CG: bound %.3e, device %.3e, iterations %s" % (Bj, gotj, its))
    assert gotj <= Bj
    assert solver.parameters["nonzero_initial_guess"] is False, "the caller's setting was not restored"
    assert min(its) >= 1


@pytest.mark.parametrize("scheme", ["generalized_alpha", "backward_euler"])
def test_driver_heat_3d_against_longdouble(scheme):
    """Order 1 on a 3-D p = 3 patch of 4^3 elements (343 dofs), 6 steps, same comparison and bound as the order-2 test;
    the initial velocity of the generalized-alpha run is given to both sides"""
    from tigar_amd import forms as F, timeIntegration as TI
    spline = _spline(3, 3, (4, 4, 4))
    spline.setSolverOptions(linearSolver=None)
    rho, dt, steps = 0.5, 0.002, 6
    shape = lambda s: np.sin(np.pi * s)
    amplitude = lambda t: np.cos(40.0 * t)
    load = lambda t: F.SeparableLoadForm([shape] * 3, scale=amplitude(t))
    x0 = _state(spline, 3)
    zero = np.asarray(spline.zeroDofs, dtype=np.int64)
    Kd, Md = spline.assembleMatrix(F.LaplaceForm()), spline.assembleMatrix(F.MassForm())
    K, M = _dense(Kd), _dense(Md)
    f1 = spline.assembleVector(F.SeparableLoadForm([shape] * 3, scale=1.0)).get_local()
    v0 = None
    if scheme == "generalized_alpha":
        v0 = np.linalg.solve(M, amplitude(0.0) * f1 - K @ x0)
        v0[zero] = 0.0
    prob = TI.LinearTransientProblem(spline, stiffness=F.LaplaceForm(), mass=F.MassForm(), order=1, scheme=scheme, RHO_INF=rho,
                                     DELTA_T=dt, load=load, x0=_dv(x0), xdot0=None if v0 is None else _dv(v0))
    c_K, c_M = _keff_coefficients(1, scheme, rho, dt, None)
    assert np.isclose(prob.c_K, c_K, rtol=1e-14) and np.isclose(prob.c_M, c_M, rtol=1e-14)
    Keff = c_K * K + c_M * M
    kw = dict(order=1, scheme=scheme, rho_inf=rho, load=lambda t: amplitude(t) * f1, x0=x0, v0=v0)
    ref = R.integrate(K, M, dt, steps, dtype=LD, **kw)
    B = steps * np.linalg.cond(Keff) * 32 * EPS
    host = _deviation(R.integrate(K, M, dt, steps, dtype=np.float64, **kw)["x"], ref["x"])
    print("%s: bound %.3e, float64 recurrence %.3e" % (scheme, B, host))
    assert host <= B / 8
    xs, _ = _trajectory(prob, steps, zero)
    got = _deviation(xs, ref["x"])
    print("%s: device %.3e" % (scheme, got))
    assert got <= B
    assert (prob.xdot is None) == (scheme == "backward_euler") and prob.xddot is None


def test_driver_midpoint_conserves_energy():
    """RHO_INF = 1, no damping, no load: the energy is conserved in exact arithmetic; 50 steps with the default direct solver
    on a 2-D p = 3 patch of 6 x 6 elements drift by at most 50 * cond2(K_eff) * 32 eps relative (the float64 recurrence: an
    eighth of that)"""
    from tigar_amd import forms as F, timeIntegration as TI
    spline = _spline(2, 3, (6, 6))
    spline.setSolverOptions(linearSolver=None)
    dt, steps = 0.02, 50
    x0, v0 = _state(spline, 4), _state(spline, 5, 10.0)
    prob = TI.LinearTransientProblem(spline, stiffness=F.LaplaceForm(), mass=F.MassForm(), order=2, RHO_INF=1.0, DELTA_T=dt,
                                     x0=_dv(x0), xdot0=_dv(v0))
    K, M = _dense(prob.K), _dense(prob.Mm)
    c_K, c_M = _keff_coefficients(2, "generalized_alpha", 1.0, dt, None)
    bound = steps * np.linalg.cond(c_K * K + c_M * M) * 32 * EPS
    ref = R.integrate(K, M, dt, steps, order=2, rho_inf=1.0, x0=x0, v0=v0)
    eh = np.array([R.energy(K, M, x, v) for x, v in zip(ref["x"], ref["v"])])
    host = np.max(np.abs(eh - eh[0])) / eh[0]
    assert host <= bound / 8
    e = [prob.energy()]
    for _ in range(steps):
        prob.step()
        e.append(prob.energy())
    e = np.array(e)
    assert np.isclose(e[0], eh[0], rtol=1e-12)
    drift = np.max(np.abs(e - e[0])) / e[0]
    print("energy drift: bound %.3e, float64 recurrence %.3e, device %.3e" % (bound, host, drift))
    assert drift <= bound


def test_driver_fast_diagonalization():
    """unmapped 3-D p = 2 patch of 6^3 elements: K_eff = c_K K + c_M M keeps the tensor structure of K and M, so FD-CG takes it;
    5 steps agree with Jacobi-CG within the sum of the direct and the Jacobi bound of the order-2 test, in no more
    iterations"""
    import tigar_amd as t
    from tigar_amd import forms as F, timeIntegration as TI
    spline = _spline(3, 2, (6, 6, 6))
    rho, dt, steps, rtol = 0.5, 0.01, 5, 1e-12
    x0, v0 = _state(spline, 6), _state(spline, 7, 3.0)
    zero = np.asarray(spline.zeroDofs, dtype=np.int64)

    def run(solver):
        solver.parameters["relative_tolerance"] = rtol
        spline.setSolverOptions(linearSolver=solver)
        prob = TI.LinearTransientProblem(spline, stiffness=F.LaplaceForm(), mass=F.MassForm(), order=2, RHO_INF=rho, DELTA_T=dt,
                                         x0=_dv(x0), xdot0=_dv(v0))
        return prob, _trajectory(prob, steps, zero)

    pj, (xj, itj) = run(t.PETScKrylovSolver("cg", "jacobi"))
    fd = t.PETScKrylovSolver("cg", "fast_diagonalization")
    pf, (xf, itf) = run(fd)
    assert getattr(pf.K_eff, "tensor_structure", None) is not None
    assert getattr(pf.K_eff, "symmetric_by_construction", False) is True
    assert fd.last["preconditioner"] == "fast_diagonalization"
    Keff = _dense(pf.K_eff)
    bound = steps * np.linalg.cond(Keff) * 32 * EPS + steps * _scaled_condition(Keff) * 4 * rtol
    top = max(np.linalg.norm(x) for x in xj)
    dev = max(np.linalg.norm(a - b) for a, b in zip(xf, xj)) / top
    print("FD-CG vs Jacobi-CG: bound %.3e, deviation %.3e, iterations %s vs %s" % (bound, dev, itf, itj))
    assert dev <= bound
    assert all(a <= b for a, b in zip(itf, itj))
    assert pf.last["iterations"] <= pj.last["iterations"]


def test_combine_hands_structure_on():
    from tigar_amd import forms as F
    from tigar_amd.device import DeviceCSR
    spline = _spline(2, 2, (5, 4))
    K, M = spline.assembleMatrix(F.LaplaceForm()), spline.assembleMatrix(F.MassForm())
    assert K.tensor_structure is not M.tensor_structure
    C1 = K.combine(2.0, M, 3.0)
    assert C1.tensor_structure is K.tensor_structure and C1.symmetric_by_construction is True
    plain = DeviceCSR.from_scipy(M.to_scipy())
    C2 = K.combine(2.0, plain, 3.0)
    assert getattr(C2, "tensor_structure", None) is None and not getattr(C2, "symmetric_by_construction", False)
    w = _dv(np.ones(K.shape[0]))
    C3 = K.combine(1.0, M, 1.0, w)                       # a column scaling: neither symmetric nor a Kronecker sum
    assert getattr(C3, "tensor_structure", None) is None and not getattr(C3, "symmetric_by_construction", False)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------
def test_driver_refusals():
    from tigar_amd import forms as F, timeIntegration as TI
    spline = _spline(2, 2, (4, 4))
    kw = dict(stiffness=F.LaplaceForm(), mass=F.MassForm())
    for bad in (dict(RHO_INF=1.5, DELTA_T=0.1), dict(RHO_INF=-0.1, DELTA_T=0.1), dict(DELTA_T=0.0), dict(DELTA_T=-1.0),
                dict(DELTA_T=0.1, order=3), dict(DELTA_T=0.1, scheme="newmark"), dict(DELTA_T=0.1, order=1, damping=(1.0, 0.0)),
                dict(DELTA_T=0.1, x0=_dv(np.zeros(3)))):
        with pytest.raises(ValueError):
            TI.LinearTransientProblem(spline, **dict(kw, **bad))
    nfe = spline.M.shape[0]
    corner = sp.csr_matrix(([1.0], ([0], [0])), shape=(nfe, nfe))          # an FE matrix with another pattern than the mass
    with pytest.raises(ValueError):
        TI.LinearTransientProblem(spline, stiffness=F.LaplaceForm(), mass=corner, DELTA_T=0.1)

    class Several(object):
        def _distributed(self):
            return True

        def _caller_ordered(self):
            return False

    class CallerOrdered(object):
        def _distributed(self):
            return False

        def _caller_ordered(self):
            return True

    class RowBlocks(object):
        zeroDofs = np.zeros(0, dtype=np.int32)

        def _distributed(self):
            return False

        def _caller_ordered(self):
            return False

        def assembleMatrix(self, form):
            return [object()]

    for stub in (Several(), CallerOrdered(), RowBlocks()):
        with pytest.raises(NotImplementedError):
            TI.LinearTransientProblem(stub, DELTA_T=0.1, **kw)
    TI.LinearTransientProblem(spline, DELTA_T=0.1, **kw).step(2)
