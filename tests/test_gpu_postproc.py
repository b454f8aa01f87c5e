"""GPU: quadrature-point kernels (csrc/tg_postproc.hip) against the longdouble reference of tests/postproc_reference.py,
and what is built on them: QuadratureLoadForm, ExtractedSpline.project / projectDofs / errorNorm / integrate /
evaluateAtQuadrature, callables as initial data of LinearTransientProblem.

Elementwise bounds c eps magnitude.  The magnitudes come from the reference (first-order propagation: a nodal field at a
point has the magnitude sum_a |u_a phi_a|, a product |a| eb + ea |b| + |a b|, see its docstring); the constants c count the
longest chain of roundings of the kernel (``postproc_reference.constants``):

  table entry        t = 6 p + 4     l: p factors (x - m/p) / (a/p - m/p) of 5 roundings, one product each; l': p such terms
                                     and their sum
  field at a point   cN = d (t + p + 1)   per direction one table factor and p + 1 fused multiply-adds
  x = N_i / W        cN + 2          a quotient of two fields
  wdet               cN + 16         DF = (dN W - N dW) / W^2: 4, g = DF^T DF: nsd + 1 <= 4, determinant: 7, square root,
                                     d weights and their product: 1 + 3
  gradient           cN + 24         DF and g as above (8), the inverse: 3 + 4 + 1, g^-1 grad_xi u and DF times it: d + 1 each
  load               (cN + 16) + 1 + d (t + nq) + 2^d   wdet f, then per direction a table factor and nq fused multiply-adds
                                     back to the nodes, then the sum over the 2^d elements around a node
  error sums         kappa (cN + 16) + (2 cN + 4 | 2 (cN + 24) + nsd + 3 | 3) + tree    the three sums; kappa = max wdet_mag /
                                     wdet turns the relative error of the weights into a multiple of the sums, tree =
                                     log2(nq^d) + ceil(nelem / 256) + 8 is the depth of the fixed summation order

Normwise: max |error| / max |reference| of every vector output stays below NORMWISE_FIELDS eps and the relative error of the
three sums with random u below NORMWISE_SUMS eps: 8 x the largest ratios observed on the MI355X against the longdouble
reference over all cases, 150.86 eps (the gradient at p = 8, nq = 4 in 2-D, where the equispaced basis is badly conditioned;
wdet 123.19 and the load 126.92 there; at p <= 5 the largest is 56.48, the gradient at p = 5, nq = 6) and 210.15 eps (sum 0 at
p = 8; at p <= 5 the largest is 18.95, sum 1 at p = 4, nq = 10).
"""
import numpy as np
import pytest

from oracle import tigar_oracle as O
import postproc_reference as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
NORMWISE_FIELDS = 1207.0     # 8 x 150.86 eps observed
NORMWISE_SUMS = 1681.0       # 8 x 210.15 eps observed


@pytest.fixture(scope="module")
def T():
    import tigar_amd
    from tigar_amd import BSplines, forms, device, NURBS
    device.device_info()

    class NS:
        pass
    ns = NS()
    ns.t, ns.B, ns.F, ns.dev, ns.N = tigar_amd, BSplines, forms, device, NURBS
    return ns


def _smooth_patch(nels, p, seed, nsd=None, uniform=False):
    """non-uniform element vertices and a smooth non-affine rational map given on the Q_p nodes"""
    d = len(nels)
    rng = np.random.default_rng(seed)
    uks = []
    for k in range(d):
        if uniform or nels[k] == 1:
            uks.append(np.linspace(0.0, 1.0 + 0.5 * k, nels[k] + 1))
        else:
            steps = rng.uniform(0.5, 1.5, nels[k])
            uks.append(np.concatenate([[0.0], np.cumsum(steps) / np.sum(steps) * (1.0 + 0.5 * k)]))
    X = R.lagrange_nodes(uks, p)
    wgt = 1.0 + 0.2 * X[0] * X[-1]
    coords = [X[i] + 0.1 * X[(i + 1) % d] ** 2 for i in range(d)]
    if nsd is not None and nsd > d:
        coords.append(X[0] ** 2 + X[-1])
    return uks, [c * wgt for c in coords] + [wgt]


def _surface_patch():
    """the surface of test_surface_and_volume_maps_match_oracle: z = x^2 + y over [0, 1] x [0, 2], 4 x 3 elements, p = 2"""
    uks = [np.linspace(0.0, 1.0, 5), np.linspace(0.0, 2.0, 4)]
    X = R.lagrange_nodes(uks, 2)
    return uks, [X[0], X[1], X[0] ** 2 + X[1], np.ones_like(X[0])]


CASES = {
    "1d_p3_5": lambda: (3, None) + _smooth_patch((5,), 3, 1),
    "2d_p2_5x4": lambda: (2, None) + _smooth_patch((5, 4), 2, 2),
    "2d_p2_6x5_full_and_partial_group": lambda: (2, None) + _smooth_patch((6, 5), 2, 3),
    "2d_p5_2x2_nq6": lambda: (5, 6) + _smooth_patch((2, 2), 5, 4),
    "2d_p2_single_element": lambda: (2, None) + _smooth_patch((1, 1), 2, 5),
    "3d_p2_3x2x4": lambda: (2, None) + _smooth_patch((3, 2, 4), 2, 6),
    "3d_p3_2x3x2_wave_per_element": lambda: (3, 4) + _smooth_patch((2, 3, 2), 3, 7),
    "2d_p2_3x4_nq4": lambda: (2, 4) + _smooth_patch((3, 4), 2, 8),
    "3d_p2_2x2x3_nq4": lambda: (2, 4) + _smooth_patch((2, 2, 3), 2, 9),
    "2d_p3_3x2_nq2_fewer_points_than_nodes": lambda: (3, 2) + _smooth_patch((3, 2), 3, 15),
    "2d_p2_3x3_nq1": lambda: (2, 1) + _smooth_patch((3, 3), 2, 16),
    "2d_p8_2x1_nq4": lambda: (8, 4) + _smooth_patch((2, 1), 8, 17),
    "3d_p3_2x2x2_nq3": lambda: (3, 3) + _smooth_patch((2, 2, 2), 3, 18),
    "3d_p2_3x2x2_nq2": lambda: (2, 2) + _smooth_patch((3, 2, 2), 2, 19),
    "3d_p4_1x2x1_nq4": lambda: (4, 4) + _smooth_patch((1, 2, 1), 4, 20),
    "3d_p4_1x1x2_nq10_more_than_64KiB_of_LDS": lambda: (4, 10) + _smooth_patch((1, 1, 2), 4, 21),
    "surface_in_3d": lambda: (2, None) + _surface_patch(),
    "quarter_annulus_5": lambda: (2, None) + R.annulus_patch(5),
    "rational_volume_p2_2x3x2": lambda: (2, None) + R.volume_patch(2, (2, 3, 2)),
}
_REF = {}


def _case(name):
    """(p, nq, vertices, control functions, reference, inputs): computed once per case and shared"""
    if name not in _REF:
        p, nq, uks, cp = CASES[name]()
        ref = R.Reference(uks, p, cp, nq)
        rng = np.random.default_rng(len(name))
        xq = ref.x.astype(np.float64)
        smooth = np.sin(2.0 * xq[:, 0]) + 0.5 * xq[:, -1] ** 2
        gsm = np.zeros_like(xq)
        gsm[:, 0] += 2.0 * np.cos(2.0 * xq[:, 0])
        gsm[:, -1] += xq[:, -1]
        Xn = np.stack([np.asarray(cp[i]) / np.asarray(cp[-1]) for i in range(ref.nsd)], axis=1)
        _REF[name] = dict(p=p, nq=nq, uks=uks, cp=cp, ref=ref, u=rng.standard_normal(ref.nnodes), fq=rng.standard_normal(ref.npts),
                          e=smooth, ge=gsm, u_interp=np.sin(2.0 * Xn[:, 0]) + 0.5 * Xn[:, -1] ** 2,
                          c=R.constants(ref.d, p, ref.nq, ref.nsd, int(np.prod(ref.nel)), ref.kappa))
    return _REF[name]


def _dcp(T, c):
    return [T.dev.DeviceVector(data=v) for v in c["cp"]]


def _normwise(name, what, err, scale):
    ratio = float(np.max(np.abs(err)) / np.max(np.abs(scale))) / EPS
    print("normwise %-40s %-8s %.2f eps" % (name, what, ratio))
    assert ratio <= (NORMWISE_SUMS if what.startswith("sum") else NORMWISE_FIELDS), (name, what, ratio)


@pytest.mark.parametrize("name", sorted(CASES))
def test_quad_points(T, name):
    c = _case(name)
    ref = c["ref"]
    x, w = T.dev.quad_points(c["uks"], c["p"], _dcp(T, c), nq=c["nq"])
    x = x.get_local().reshape(ref.nsd, ref.npts).T
    w = w.get_local()
    ex, ew = np.abs(x - ref.x).astype(np.float64), np.abs(w - ref.wdet).astype(np.float64)
    print("points %s: x %.2f of the bound, wdet %.2f" % (name, float(np.max(ex / (c["c"]["x"] * EPS * ref.x_mag))),
                                                         float(np.max(ew / (c["c"]["wdet"] * EPS * ref.wdet_mag)))))
    assert np.all(ex <= c["c"]["x"] * EPS * ref.x_mag)
    assert np.all(ew <= c["c"]["wdet"] * EPS * ref.wdet_mag)
    _normwise(name, "x", ex, ref.x)
    _normwise(name, "wdet", ew, ref.wdet)


@pytest.mark.parametrize("name", sorted(CASES))
def test_quad_eval(T, name):
    c = _case(name)
    ref = c["ref"]
    v, g, vm, gm = ref.eval(c["u"])
    du = T.dev.DeviceVector(data=c["u"])
    val, grad = T.dev.quad_eval(c["uks"], c["p"], _dcp(T, c), du, grad=True, nq=c["nq"])
    only = T.dev.quad_eval(c["uks"], c["p"], _dcp(T, c), du, nq=c["nq"]).get_local()
    val, grad = val.get_local(), grad.get_local().reshape(ref.nsd, ref.npts).T
    assert np.array_equal(only.view(np.int64), val.view(np.int64))           # the values do not depend on with_grad
    ev, eg = np.abs(val - v).astype(np.float64), np.abs(grad - g).astype(np.float64)
    print("eval %s: values %.2f of the bound, gradient %.2f" % (name, float(np.max(ev / (c["c"]["val"] * EPS * vm))),
                                                                 float(np.max(eg / (c["c"]["grad"] * EPS * gm)))))
    assert np.all(ev <= c["c"]["val"] * EPS * vm)
    assert np.all(eg <= c["c"]["grad"] * EPS * gm)
    _normwise(name, "val", ev, v)
    _normwise(name, "grad", eg, g)


@pytest.mark.parametrize("name", sorted(CASES))
def test_quad_load(T, name):
    c = _case(name)
    ref = c["ref"]
    b, bm = ref.load(c["fq"])
    out = T.dev.quad_load(c["uks"], c["p"], _dcp(T, c), T.dev.DeviceVector(data=c["fq"]), nq=c["nq"]).get_local()
    eb = np.abs(out - b).astype(np.float64)
    print("load %s: %.2f of the bound" % (name, float(np.max(eb / (c["c"]["load"] * EPS * bm)))))
    assert np.all(eb <= c["c"]["load"] * EPS * bm)
    _normwise(name, "load", eb, b)


@pytest.mark.parametrize("setting", ["random_u", "interpolant_of_e"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_quad_error(T, name, setting):
    """the three sums within c eps sum wdet (|u|_q + |e_q|)^2 (and its analogue for the gradients): with u random, where the
    sums are O(1), and with u the nodal interpolant of e, where they are small and the same ABSOLUTE bound applies"""
    c = _case(name)
    ref = c["ref"]
    u = c["u"] if setting == "random_u" else c["u_interp"]
    s, m = ref.sums(u, c["e"], c["ge"])
    dv = T.dev.DeviceVector
    ge = dv(data=np.ascontiguousarray(c["ge"].T).ravel())
    got = T.dev.quad_error(c["uks"], c["p"], _dcp(T, c), dv(data=u), dv(data=c["e"]), ge, nq=c["nq"])
    for t in range(3):
        err = abs(float(got[t] - s[t]))
        bound = c["c"]["err"][t] * EPS * float(m[t])
        print("error %s %s term %d: %.3e (reference %.3e), error %.2e, bound %.2e" % (name, setting, t, got[t], float(s[t]), err, bound))
        assert err <= bound
        if setting == "random_u":
            _normwise(name, "sum%d" % t, np.array([err]), np.array([float(s[t])]))
    if setting == "interpolant_of_e":
        assert got[0] < 1e-2 * got[2]                 # (the sums ARE small here, whatever the number of points)
    # null operands: e^2 alone, u^2 alone
    only_e = T.dev.quad_error(c["uks"], c["p"], _dcp(T, c), None, dv(data=c["e"]), None, nq=c["nq"])
    assert only_e[1] == 0.0 and only_e[0] == only_e[2] and abs(only_e[2] - float(s[2])) <= c["c"]["err"][2] * EPS * float(m[2])
    only_u = T.dev.quad_error(c["uks"], c["p"], _dcp(T, c), dv(data=u), None, None, nq=c["nq"])
    su, mu = ref.sums(u)
    assert only_u[2] == 0.0 and abs(only_u[0] - float(su[0])) <= c["c"]["err"][0] * EPS * float(mu[0])


@pytest.mark.parametrize("name", sorted(n for n in CASES if "more_than_64KiB" not in n))
def test_load_of_the_evaluated_interpolant_equals_the_nodal_load(T, name):
    """independent cross-check: quad_load(quad_eval(f)) is the load of the nodal interpolant, which tg_assemble_mapped_load
    computes with the plain kernels of the parent commit (which refuse the one shape whose element data exceed 64 KiB of
    LDS: no partner there)"""
    c = _case(name)
    dcp = _dcp(T, c)
    fn = T.dev.DeviceVector(data=c["u_interp"])
    a = T.dev.quad_load(c["uks"], c["p"], dcp, T.dev.quad_eval(c["uks"], c["p"], dcp, fn, nq=c["nq"]), nq=c["nq"]).get_local()
    b = T.dev.assemble_mapped_load(c["uks"], c["p"], dcp, fn, nq=c["nq"]).get_local()
    assert np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(b))


@pytest.mark.parametrize("p,nels", [(2, (6, 5)), (2, (9, 7, 8)), (3, (37, 24))])
def test_sums_and_load_are_bit_reproducible(T, p, nels):
    uks, cp = _smooth_patch(nels, p, 11)
    dcp = [T.dev.DeviceVector(data=v) for v in cp]
    rng = np.random.default_rng(12)
    npts = T.dev.quad_count(uks, p + 1)
    u, e = T.dev.DeviceVector(data=rng.standard_normal(cp[0].size)), T.dev.DeviceVector(data=rng.standard_normal(npts))
    ge = T.dev.DeviceVector(data=rng.standard_normal(len(nels) * npts))
    runs = [(T.dev.quad_error(uks, p, dcp, u, e, ge), T.dev.quad_load(uks, p, dcp, e).get_local()) for _ in range(3)]
    for s, b in runs[1:]:
        assert s == runs[0][0]
        assert np.array_equal(b.view(np.int64), runs[0][1].view(np.int64))


def test_limits_are_errors_with_a_message(T):
    uks, cp = _smooth_patch((2, 2), 2, 13)
    dcp = [T.dev.DeviceVector(data=v) for v in cp]
    max_loc, max_q1 = T.dev.assemble_limits()
    assert (max_loc, max_q1) == (128, 10)                # (TG_ASM_MAXLOC, TG_ASM_MAXQ1 of csrc/tg_asm_shared.h)
    with pytest.raises(T.dev.TigarHipError, match="Gauss points"):
        T.dev.quad_points(uks, 2, dcp, nq=max_q1 + 1)
    uks3, cp3 = _smooth_patch((1, 1, 1), 5, 14)
    with pytest.raises(T.dev.TigarHipError, match="local nodes"):
        T.dev.quad_points(uks3, 5, [T.dev.DeviceVector(data=v) for v in cp3])
    with pytest.raises(T.dev.TigarHipError):
        T.dev.quad_load(uks, 2, dcp, T.dev.DeviceVector(7))
    a = T.dev.DeviceVector(data=np.array([1.0, -6.0, 0.5]))
    b = T.dev.DeviceVector(data=np.array([4.0, 3.0, 0.25]))
    assert np.array_equal(a.pointwise_divide(b).get_local(), np.array([0.25, -2.0, 2.0]))
    with pytest.raises(T.dev.TigarHipError):
        a.pointwise_divide(T.dev.DeviceVector(4))


# ---- projection ------------------------------------------------------------------------------------------------------------
def _zero_all_sides(gen, d):
    sp0 = gen.getScalarSpline(0)
    for direction in range(d):
        for side in (0, 1):
            gen.addZeroDofs(0, sp0.getSideDofs(direction, side))


def _projection_spline(T, kind, clamp, rtol=1e-12):
    """(spline, oracle extraction operator, element vertices, p, host control functions)"""
    t, B = T.t, T.B
    if kind == "2d":
        p, kvs = 2, [B.uniformKnots(2, 0.0, 1.0, 6), B.uniformKnots(2, 0.0, 1.5, 5)]
        gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2, 2], kvs))
    elif kind == "annulus":
        from geom_util import quarter_annulus
        kv, Pf = quarter_annulus(5)
        p, kvs = 2, [kv, kv]
        gen = t.EqualOrderSpline(1, T.N.NURBSControlMesh([2, 2], kvs, Pf))
    else:
        p, kvs = 2, [B.uniformKnots(2, 0.0, 1.0, n) for n in (3, 2, 4)]
        gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2] * 3, kvs))
    d = len(kvs)
    if clamp:
        _zero_all_sides(gen, d)
    spline = t.ExtractedSpline(gen, 2 * p)
    solver = t.PETScKrylovSolver("cg", "jacobi")
    solver.parameters["relative_tolerance"] = rtol
    spline.setSolverOptions(linearSolver=solver)
    Mo = O.generate_M_tensor(O.BSpline([p] * d, [list(k) for k in kvs]))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k], dtype=np.float64) for k in range(d)]
    cp = [f.vector().get_local() for f in gen.cpFuncs]
    return spline, Mo, uks, p, cp


@pytest.mark.parametrize("applyBCs", [False, True])
@pytest.mark.parametrize("kind", ["2d", "annulus", "3d"])
def test_consistent_projection_reproduces_a_function_of_the_space(T, kind, applyBCs):
    """random IGA dofs U0, u0 = M U0 handed over as a Function: projectDofs returns U0 within kappa (rtol + 64 eps) |U0|_inf,
    kappa the condition number of the reference mass K; the mass K is assembled once"""
    rtol = 1e-12
    spline, Mo, uks, p, cp = _projection_spline(T, kind, applyBCs, rtol)
    zd = [int(i) for i in spline.zeroDofs]
    rng = np.random.default_rng(21)
    U0 = rng.standard_normal(Mo.shape[1])
    if applyBCs:
        U0[zd] = 0.0
    u0 = T.t.Function(spline.V)
    u0.vector().set_local(Mo @ U0)
    Km = O.extract_matrix(Mo, O.mapped_fe_system(uks, p, cp)[0], zd if applyBCs else None, applyBCs=applyBCs)
    kappa = np.linalg.cond(Km.toarray())
    U = spline.projectDofs(u0, applyBCs=applyBCs).get_local()
    err = np.max(np.abs(U - U0))
    print("projection %s applyBCs=%s: error %.2e, kappa %.1f, bound %.2e" % (kind, applyBCs, err, kappa,
                                                                            kappa * (rtol + 64 * EPS) * np.max(np.abs(U0))))
    assert err <= kappa * (rtol + 64 * EPS) * np.max(np.abs(U0))
    if applyBCs:
        assert np.all(U[zd] == 0.0)
    assert spline.__dict__["_projection_mass_builds"] == 1
    key = (applyBCs, p + 1, np.asarray(spline.zeroDofs).tobytes() if applyBCs else b"")
    K1 = spline.__dict__["_projection_mass"][key]
    U2 = spline.projectDofs(u0, applyBCs=applyBCs).get_local()
    assert spline.__dict__["_projection_mass_builds"] == 1 and spline.__dict__["_projection_mass"][key] is K1
    assert np.array_equal(U2.view(np.int64), U.view(np.int64))
    # project() is M U
    uf = spline.project(u0, applyBCs=applyBCs).vector().get_local()
    assert np.max(np.abs(uf - Mo @ U)) <= 64 * EPS * np.max(np.abs(Mo @ U))
    assert spline.__dict__["_projection_mass_builds"] == 1


@pytest.mark.parametrize("kind", ["2d", "annulus", "3d"])
def test_lumped_projection(T, kind):
    spline, Mo, uks, p, cp = _projection_spline(T, kind, True)
    zd = np.array([int(i) for i in spline.zeroDofs])
    free = np.setdiff1d(np.arange(Mo.shape[1]), zd)
    # a constant, by partition of unity
    U = spline.projectDofs(3.7, lumpMass=True).get_local()
    assert np.max(np.abs(U - 3.7)) <= 64 * EPS * 3.7
    U = spline.projectDofs(3.7, lumpMass=True, applyBCs=True).get_local()
    assert np.all(U[zd] == 0.0) and np.max(np.abs(U[free] - 3.7)) <= 64 * EPS * 3.7
    assert "_projection_mass" not in spline.__dict__                         # no matrix
    # a smooth function against the host formula M^T b ./ M^T 1 from the reference's loads
    f = lambda x: np.sin(2.0 * x[:, 0]) + 0.5 * x[:, -1] ** 2
    ref = R.Reference(uks, p, cp)
    b = ref.load(f(ref.x.astype(np.float64)))[0].astype(np.float64)
    one = ref.load(np.ones(ref.npts))[0].astype(np.float64)
    want = (Mo.T @ b) / (Mo.T @ one)
    U = spline.projectDofs(f, lumpMass=True).get_local()
    assert np.max(np.abs(U - want)) <= 1e-12 * np.max(np.abs(want))
    # the measure: integrate(1) is the sum of the weights
    assert abs(spline.integrate(1.0) - float(np.sum(ref.wdet))) <= 1e-13 * float(np.sum(ref.wdet))
    assert abs(spline.integrate(f) - float(np.sum(ref.wdet * f(ref.x.astype(np.float64))))) <= 1e-12


def test_quadrature_points_and_evaluation_on_the_spline(T):
    spline, Mo, uks, p, cp = _projection_spline(T, "annulus", False)
    ref = R.Reference(uks, p, cp)
    pts = spline.quadraturePoints()
    assert pts is spline.quadraturePoints() and pts is spline.quadraturePoints(nq=3) and pts is not spline.quadraturePoints(nq=4)
    assert (pts.nq, pts.npts) == (3, ref.npts) and pts.x.shape == (ref.npts, 2)
    assert np.max(np.abs(pts.x - ref.x.astype(np.float64))) <= 1e-14
    assert np.max(np.abs(pts.weights.get_local() - ref.wdet.astype(np.float64))) <= 1e-14
    u = T.t.Function(spline.V)
    u.vector().set_local(Mo @ np.random.default_rng(3).standard_normal(Mo.shape[1]))
    v, g, _, _ = ref.eval(u.vector().get_local())
    val, comps = spline.evaluateAtQuadrature(u, grad=True)
    assert len(comps) == 2 and np.max(np.abs(val.get_local() - v.astype(np.float64))) <= 1e-13
    for i in range(2):
        assert np.max(np.abs(comps[i].get_local() - g[:, i].astype(np.float64))) <= 1e-11
    assert np.array_equal(spline.evaluateAtQuadrature(u).get_local(), val.get_local())
    # a load given by point values, by a callable and by a Function of the space
    F = T.F
    f = lambda x: np.cos(x[:, 0]) * x[:, 1]
    b_ref = ref.load(f(ref.x.astype(np.float64)))[0].astype(np.float64)
    for arg in (f, f(pts.x), T.dev.DeviceVector(data=f(pts.x))):
        b = F.QuadratureLoadForm(arg, spline).assemble_vector(spline.V).get_local()
        assert np.max(np.abs(b - b_ref)) <= 1e-13 * np.max(np.abs(b_ref))
    b = F.QuadratureLoadForm(u, spline).assemble_vector(spline.V).get_local()
    assert np.max(np.abs(b - ref.load(v)[0].astype(np.float64))) <= 1e-13 * np.max(np.abs(b))
    # error norms against the reference's sums
    (s0, s1, s2), _ = ref.sums(u.vector().get_local(), R.annulus_exact(ref.x.astype(np.float64)),
                               R.annulus_exact_grad(ref.x.astype(np.float64)))
    l2 = spline.errorNorm(u, R.annulus_exact, "L2")
    h10 = spline.errorNorm(u, R.annulus_exact, "H10", exact_grad=R.annulus_exact_grad)
    h1 = spline.errorNorm(u, R.annulus_exact, "H1", exact_grad=R.annulus_exact_grad)
    assert abs(l2 - float(np.sqrt(s0))) <= 1e-12 * l2 and abs(h10 - float(np.sqrt(s1))) <= 1e-12 * h10
    assert abs(h1 - float(np.sqrt(s0 + s1))) <= 1e-12 * h1
    rel = spline.errorNorm(u, R.annulus_exact, "L2", relative=True)
    assert abs(rel - float(np.sqrt(s0 / s2))) <= 1e-12 * rel


@pytest.mark.parametrize("projection", ["direct", "jacobi_cg"])
def test_nonzero_dirichlet_data_exact_case(T, projection):
    """demos/poisson/poisson-nonzero-bc.py: u = 1 + x + x y^2 lies in the space (unmapped, p = 2, 4 x 3 elements, all faces
    clamped), f = -lap u = -2 x is reproduced by its nodal interpolant.  Projection -> lifting g -> one Newton step of the
    linear residual (Jacobi-CG at rtol) -> the exact solution.

    "direct": the projection through the direct solver; the L2 error (relative) and the H10 error (absolute and relative)
    stay below kappa_K (rtol + 64 eps), kappa_K the condition number of the host stiffness K.

    "jacobi_cg": the flow as the demo runs it, the projection through the spline's Jacobi-CG at rtol as well.  Then the
    lifting carries the error of the mass solve into the solution as boundary data, which kappa_K knows nothing of
    (measured: H10 error 1.6e-11 relative against kappa_K (rtol + 64 eps) = 4.6e-12, L2 error 9.6e-13).  Derived bound: CG
    stops at |D^-1 r| <= rtol |D^-1 b|, so the dofs of the projection are off by at most
        delta = kappa_M (rtol + 64 eps) |U_g|_2,   kappa_M = cond(D^-1 K_mass);
    the solution then differs from the exact one by the discrete-harmonic extension E of that boundary perturbation,
    |E|_H10^2 = d^T S d <= lambda_max(K_bb) delta^2 (S the Schur complement of the free dofs, S <= K_bb) and
    |E|_L2 <= sqrt(lambda_max(M)) (1 + |K_ff^-1 K_fb|_2) delta, plus the part of the solve itself, kappa_K (rtol + 64 eps)
    times the norm of u."""
    t, B, F = T.t, T.B, T.F
    rtol = 1e-12
    kvs = [B.uniformKnots(2, 0.0, 1.0, 4), B.uniformKnots(2, 0.0, 1.0, 3)]
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2, 2], kvs))
    _zero_all_sides(gen, 2)
    spline = t.ExtractedSpline(gen, 4)
    solver = t.PETScKrylovSolver("cg", "jacobi")
    solver.parameters["relative_tolerance"] = rtol
    spline.setSolverOptions(relativeTolerance=1e-9, linearSolver=solver)
    exact = lambda x: 1.0 + x[:, 0] + x[:, 0] * x[:, 1] ** 2
    exact_grad = lambda x: np.stack([1.0 + x[:, 1] ** 2, 2.0 * x[:, 0] * x[:, 1]], axis=1)
    Ug = spline.projectDofs(exact, linearSolver=t.PETScLUSolver() if projection == "direct" else None).get_local()
    lift = np.zeros_like(Ug)
    zd = np.array([int(i) for i in spline.zeroDofs])
    lift[zd] = Ug[zd]                                   # the free dofs zeroed: the lifting
    u = t.Function(spline.V)
    spline.M.mult(T.dev.DeviceVector(data=lift), u.vector())
    X = gen.cpFuncs[0].vector().get_local()
    zero = lambda v: T.dev.DeviceVector(v.size())
    res = F.SemilinearResidual(u, -2.0 * X, zero, zero)
    hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u)
    assert len(hist) == 2
    # the host matrices at this size
    s = O.BSpline([2, 2], [list(k) for k in kvs])
    Mo = O.generate_M_tensor(s)
    A = O.poisson_fe_system(s)[0]
    kappa = np.linalg.cond(O.extract_matrix(Mo, A, [int(i) for i in zd]).toarray())
    tol = kappa * (rtol + 64 * EPS)
    l2_rel = spline.errorNorm(u, exact, "L2", relative=True)
    h10_rel = spline.errorNorm(u, exact, "H10", exact_grad=exact_grad, relative=True)
    l2, h10 = spline.errorNorm(u, exact, "L2"), spline.errorNorm(u, exact, "H10", exact_grad=exact_grad)
    print("non-zero Dirichlet data (%s): L2 %.2e (relative %.2e), H10 %.2e (relative %.2e), kappa_K (rtol + 64 eps) = %.2e "
          "(kappa_K %.1f)" % (projection, l2, l2_rel, h10, h10_rel, tol, kappa))
    if projection == "direct":
        assert l2_rel <= tol and h10 <= tol and h10_rel <= tol
        return
    cp = [f.vector().get_local() for f in gen.cpFuncs]
    g = gen.V.grids[0]
    Mfe = O.mapped_fe_system([np.asarray(g.vertices[k], dtype=np.float64) for k in range(2)], 2, cp)[0]
    Kf, Mf = (Mo.T @ A @ Mo).toarray(), (Mo.T @ Mfe @ Mo).toarray()
    fr = np.setdiff1d(np.arange(Kf.shape[0]), zd)
    delta = np.linalg.cond(Mf / np.diag(Mf)[:, None]) * (rtol + 64 * EPS) * np.linalg.norm(Ug)
    ext = np.linalg.norm(np.linalg.solve(Kf[np.ix_(fr, fr)], Kf[np.ix_(fr, zd)]), 2)
    zero_fn = t.Function(spline.V)
    norm_l2, norm_h10 = spline.errorNorm(zero_fn, exact, "L2"), spline.errorNorm(zero_fn, exact, "H10", exact_grad=exact_grad)
    bound_h10 = np.sqrt(np.linalg.eigvalsh(Kf[np.ix_(zd, zd)]).max()) * delta + tol * norm_h10
    bound_l2 = np.sqrt(np.linalg.eigvalsh(Mf).max()) * (1.0 + ext) * delta + tol * norm_l2
    print("    derived bounds: L2 %.2e, H10 %.2e" % (bound_l2, bound_h10))
    assert l2 <= bound_l2 and h10 <= bound_h10


def test_error_norms_converge_on_the_annulus(T):
    """the annulus Poisson problem of test_poisson_on_nurbs_annulus_converges at nel = 4, 8, 16: the L2 error drops per
    halving by at least 2^p (one order under the asymptotic 2^(p+1): nel = 4 is pre-asymptotic), the H10 error by at least
    2^(p-1).  The host reference's own flow (oracle matrices, direct solve: tests/test_postproc_reference_host.py) gives
    the ratios 10.08, 8.55 (L2) and 4.46, 4.11 (H10)."""
    from geom_util import quarter_annulus
    t, F = T.t, T.F
    errs = []
    for nel in (4, 8, 16):
        kv, Pf = quarter_annulus(nel)
        gen = t.EqualOrderSpline(1, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf))
        _zero_all_sides(gen, 2)
        spline = t.ExtractedSpline(gen, 4)
        solver = t.PETScKrylovSolver("cg", "jacobi")
        solver.parameters["relative_tolerance"] = 1e-12
        spline.setSolverOptions(linearSolver=solver)
        u = t.Function(spline.V)
        spline.solveLinearVariationalProblem(F.Equation(F.LaplaceForm(geometry=gen), F.NodalLoadForm(R.annulus_rhs, gen)), u)
        errs.append((spline.errorNorm(u, R.annulus_exact, "L2"),
                     spline.errorNorm(u, R.annulus_exact, "H10", exact_grad=R.annulus_exact_grad)))
    print("annulus: L2 %s ratios %.2f %.2f; H10 %s ratios %.2f %.2f" % (
        [e[0] for e in errs], errs[0][0] / errs[1][0], errs[1][0] / errs[2][0],
        [e[1] for e in errs], errs[0][1] / errs[1][1], errs[1][1] / errs[2][1]))
    for a, b in zip(errs[:-1], errs[1:]):
        assert a[0] / b[0] >= 4.0 and a[1] / b[1] >= 2.0


def test_transient_problem_takes_a_callable_as_initial_data(T):
    from tigar_amd import timeIntegration as TI
    t, B, F = T.t, T.B, T.F
    kv = [B.uniformKnots(2, 0.0, 1.0, 4) for _ in range(3)]
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2] * 3, kv))
    _zero_all_sides(gen, 3)
    spline = t.ExtractedSpline(gen, 4)
    x0 = lambda x: np.sin(np.pi * x[:, 0]) * np.sin(np.pi * x[:, 1]) * x[:, 2] * (1.0 - x[:, 2])
    v0 = lambda x: x[:, 0] * (1.0 - x[:, 0]) * np.sin(np.pi * x[:, 1]) * np.sin(2.0 * np.pi * x[:, 2])
    out = []
    for given in (True, False):
        a, b = (x0, v0) if given else (spline.projectDofs(x0, applyBCs=True), spline.projectDofs(v0, applyBCs=True))
        prob = TI.LinearTransientProblem(spline, stiffness=F.LaplaceForm(), mass=F.MassForm(), order=2, RHO_INF=0.5,
                                         DELTA_T=0.01, x0=a, xdot0=b)
        prob.step(3)
        out.append((prob.x.get_local(), prob.xdot.get_local()))
    assert np.any(out[0][0] != 0.0)
    assert np.array_equal(out[0][0].view(np.int64), out[1][0].view(np.int64))
    assert np.array_equal(out[0][1].view(np.int64), out[1][1].view(np.int64))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(T, monkeypatch):
    t, B, F = T.t, T.B, T.F
    spline, Mo, uks, p, cp = _projection_spline(T, "annulus", True)
    npts = spline.quadraturePoints().npts
    one = lambda x: np.ones(x.shape[0])
    # ValueError
    with pytest.raises(ValueError, match="point values"):
        spline.integrate(T.dev.DeviceVector(npts + 1))
    with pytest.raises(ValueError, match="shape"):
        spline.projectDofs(np.ones(npts - 1))
    with pytest.raises(ValueError, match="shape"):
        spline.projectDofs(lambda x: np.ones((x.shape[0], 2)))
    with pytest.raises(ValueError, match="shape"):
        spline.errorNorm(t.Function(spline.V), one, "H10", exact_grad=lambda x: np.ones(x.shape[0]))
    with pytest.raises(ValueError, match="kind"):
        spline.errorNorm(t.Function(spline.V), one, "H2")
    for kind in ("H1", "H10"):
        with pytest.raises(ValueError, match="exact_grad"):
            spline.errorNorm(t.Function(spline.V), one, kind)
    for nq in (0, T.dev.assemble_limits()[1] + 1):
        with pytest.raises(ValueError, match="nq"):
            spline.quadraturePoints(nq=nq)
        with pytest.raises(ValueError, match="nq"):
            spline.projectDofs(one, nq=nq)
    # NotImplementedError
    with pytest.raises(NotImplementedError, match="weights"):
        spline.project(one, rationalize=True)
    plane = spline.V.grids[0].shape()[0]
    with pytest.raises(NotImplementedError, match="row blocks"):
        F.QuadratureLoadForm(one, spline).assemble_vector(spline.V, 0, plane)
    # (unit weights: both values of rationalize mean the same thing)
    flat, _, _, _, _ = _projection_spline(T, "2d", False)
    a = flat.project(one, rationalize=True).vector().get_local()
    assert np.array_equal(a, flat.project(one, rationalize=False).vector().get_local())
    with monkeypatch.context() as m:
        m.setattr(spline, "_distributed", lambda: True)
        with pytest.raises(NotImplementedError, match="ranks"):
            spline.projectDofs(one)
        with pytest.raises(NotImplementedError, match="ranks"):
            spline.errorNorm(t.Function(spline.V), one)
    with monkeypatch.context() as m:
        m.setattr(spline, "_caller_ordered", lambda: True)
        for call in (lambda: spline.projectDofs(one), lambda: spline.quadraturePoints(), lambda: spline.integrate(1.0)):
            with pytest.raises(NotImplementedError, match="feOrder"):
                call()
    with monkeypatch.context() as m:
        m.setenv("TIGAR_IMPLICIT_M", "1")
        kv = [B.uniformKnots(2, 0.0, 1.0, 3)] * 3
        gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2] * 3, kv))
        streamed = t.ExtractedSpline(gen, 4)
        assert streamed._implicit()
        with pytest.raises(NotImplementedError, match="streamed"):
            streamed.projectDofs(one)
    kv2 = [B.uniformKnots(2, 0.0, 1.0, 3)] * 2
    cm = B.ExplicitBSplineControlMesh([2, 2], kv2)
    two = t.ExtractedSpline(t.EqualOrderSpline(2, cm), 4)
    with pytest.raises(NotImplementedError, match="nFields"):
        two.projectDofs(one)
    lst = t.ExtractedSpline(t.FieldListSpline(cm, [B.BSpline([2, 2], kv2)]), 4)
    with pytest.raises(NotImplementedError, match="FieldListSpline"):
        lst.projectDofs(one)
    # compatible, multi-patch and T-spline spaces
    import os
    from tigar_amd.compatibleSplines import BSplineCompat
    from tigar_amd.RhinoTSplines import RhinoTSplineControlMesh
    patches = [B.BSpline([2, 2], [B.uniformKnots(2, 0., 3., 3), B.uniformKnots(2, 0., 1., 2)]),
               B.BSpline([2, 2], [B.uniformKnots(2, -1., 1., 2), B.uniformKnots(2, 0., 2., 3)])]
    mb = B.MultiBSpline(patches)

    class TwoPatches(t.AbstractControlMesh):
        def getScalarSpline(self):
            return mb

        def getNsd(self):
            return 2

        def getHomogeneousCoordinate(self, node, direction):
            if direction == 2:
                return 1.0
            patch = 0 if node < mb.doffsets[1] else 1
            local = node - mb.doffsets[patch]
            n0 = patches[patch].splines[0].getNcp()
            idx = (local % n0, local // n0)
            return patches[patch].splines[direction].greville(idx[direction]) + (2.0 * patch if direction == 0 else 0.0)
    others = {"compatible": t.ExtractedSpline(BSplineCompat(cm, "RT", [1, 1]), 4),
              "multi-patch": t.ExtractedSpline(t.EqualOrderSpline(1, TwoPatches()), 4),
              "T-spline": t.ExtractedSpline(t.EqualOrderSpline(1, RhinoTSplineControlMesh(
                  os.path.join(os.path.dirname(__file__), "golden", "tspline_bicubic_patch.iga"))), 4)}
    for name, sp_ in others.items():
        with pytest.raises(NotImplementedError):
            sp_.projectDofs(one)
        with pytest.raises(NotImplementedError):
            sp_.errorNorm(t.Function(sp_.V), one)
        with pytest.raises(NotImplementedError):
            sp_.quadraturePoints()
    kvd = [0, 0, 0, 0.5, 0.5, 0.5, 1, 1, 1]
    dg = t.ExtractedSpline(t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2, 2], [kvd, kvd])), 4)
    with pytest.raises(NotImplementedError, match="DG"):
        dg.errorNorm(t.Function(dg.V), one)
