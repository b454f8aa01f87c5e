"""GPU: second-derivative point forms -- ``tg_quad_jet`` / ``tg_quad_geometry_jet`` / ``tg_jet_transform`` /
``tg_jet_load_transform`` / ``tg_assemble_jet_blocks`` / ``tg_quad_load_jet`` (csrc/tg_jet.hip) and what is built on them:
``evaluateJetsAtQuadrature``, ``geometryJetsAtQuadrature``, ``forms.JetCoefficientForm`` / ``VectorJetCoefficientForm`` /
``JetLoadForm`` / ``VectorJetLoadForm``.

Reference: tests/jet_reference.py, which forms phi (or phi / W_h), x = N / W and their parametric derivatives directly at
every point -- the 1-D Lagrange derivatives divided by the element sizes, the quotient rule applied to the functions
themselves -- and sums the integrand as written: no Q matrix, no transformed data.  Point data are RANDOM per point, so that
any mis-numbering of points, slots or blocks shows; T is not symmetric.  Element vertices are non-uniform: S is no multiple of
the identity.

Tolerance: normwise, max |error| / max |reference| against the longdouble run.  The bound of a case is 8 x the error of the
float64 run of the same reference for that case (computed here, on the CPU: no figure of the code under test), and never
below 32 eps -- the rule of tests/test_gpu_coef.py.  ``-s`` prints error, float64 error and bound of every case; the largest
error / bound (printed when the module's fixture is torn down) measured on the MI355X is in the README section "Second-derivative point forms".
"""
import os

import numpy as np
import pytest

import jet_reference as JR
import shell_reference as SR

pytestmark = pytest.mark.gpu

EPS = JR.EPS
FLOOR = 32 * EPS
LD = JR.LD


@pytest.fixture(scope="module")
def T():
    import tigar_amd
    from tigar_amd import BSplines, forms, device, NURBS
    device.device_info()

    class NS:
        pass
    ns = NS()
    ns.t, ns.B, ns.F, ns.dev, ns.N = tigar_amd, BSplines, forms, device, NURBS
    yield ns
    # the figure for the README: every ``_hold`` has asserted its own case, this only reports the largest of those that ran
    print("\nlargest error / bound over the cases of this file that ran: %.3f" % WORST["ratio"])


# name -> (p, nq, element vertices, control functions on the Q_p nodes)
CASES = {
    # d = 1: a curve in the plane and one in space, p = 2 and 3, 1 and 5 elements
    "curve2_p2_1": lambda: (2, None) + JR.polynomial_patch((1,), 2, 2),
    "curve2_p3_5": lambda: (3, None) + JR.polynomial_patch((5,), 3, 2),
    "curve3_p3_1": lambda: (3, 2) + JR.polynomial_patch((1,), 3, 3),
    "curve3_p2_5": lambda: (2, 4) + JR.polynomial_patch((5,), 2, 3),
    # d = 2, patches: 1 x 1 (three empty colours), 1 x 3, 3 x 2, 5 x 4, and 17 x 3 = 51 elements, more than a workgroup of
    # k_jet_points takes (max(1, 256 / nq^2) of them): 28 at nq = 3 -- two workgroups, the last with 23 -- and 16 at nq = 4 -- four
    # workgroups, the last with 3.  (Every other patch of this file runs in one workgroup.)
    "plane_p2_1x1": lambda: (2, None) + JR.polynomial_patch((1, 1), 2, 2),
    "plane_p2_1x3": lambda: (2, None) + JR.polynomial_patch((1, 3), 2, 2),
    "plane_p2_3x2": lambda: (2, None) + JR.polynomial_patch((3, 2), 2, 2),
    "plane_p2_5x4": lambda: (2, None) + JR.polynomial_patch((5, 4), 2, 2),
    "plane_p2_17x3": lambda: (2, None) + JR.polynomial_patch((17, 3), 2, 2),
    "plane_p2_17x3_nq4": lambda: (2, 4) + JR.polynomial_patch((17, 3), 2, 2),
    # degrees and points: p = 1..4; nq = 1, nq != p + 1, nq = p + 1, nq = 10 (one or two elements)
    "plane_p1_3x2_nq1": lambda: (1, 1) + JR.polynomial_patch((3, 2), 1, 2),
    "plane_p1_2x3": lambda: (1, None) + JR.polynomial_patch((2, 3), 1, 2),
    "plane_p3_2x3_nq2": lambda: (3, 2) + JR.polynomial_patch((2, 3), 3, 2),
    "plane_p3_3x2": lambda: (3, None) + JR.polynomial_patch((3, 2), 3, 2),
    "plane_p3_2x1_nq10": lambda: (3, 10) + JR.polynomial_patch((2, 1), 3, 2),
    "plane_p4_2x2": lambda: (4, None) + JR.polynomial_patch((2, 2), 4, 2),
    "plane_p4_1x1_nq10": lambda: (4, 10) + JR.polynomial_patch((1, 1), 4, 2),
    "plane_p4_2x1_nq1": lambda: (4, 1) + JR.polynomial_patch((2, 1), 4, 2),
    # geometries: the quarter annulus (rational), the quarter-cylinder surface in space (rational), a doubly curved polynomial
    # surface in space
    "annulus_p2_3x2": lambda: (2, None) + JR.annulus_patch((3, 2), 2),
    "annulus_p3_2x3_nq3": lambda: (3, 3) + JR.annulus_patch((2, 3), 3),
    "cylinder_p2_3x2": lambda: (2, None) + JR.cylinder_patch((3, 2), 2),
    "cylinder_p3_2x3": lambda: (3, None) + JR.cylinder_patch((2, 3), 3),
    "curved_p2_3x2": lambda: (2, None) + JR.polynomial_patch((3, 2), 2, 3),
    "curved_p3_2x2_nq5": lambda: (3, 5) + JR.polynomial_patch((2, 2), 3, 3),
}
NAMES = sorted(CASES)
_REF = {}
WORST = {"ratio": 0.0}


def _case(name):
    """patch, random point data and the reference objects per space (longdouble, float64): built once"""
    if name not in _REF:
        p, nq, uks, cp = CASES[name]()
        cp = [np.asarray(c, dtype=np.float64) for c in cp]
        c = dict(p=p, nq=nq, uks=uks, cp=cp, refs={})
        for rat in (False, True):
            c["refs"][rat] = (JR.JetReference(uks, p, cp, nq, rational=rat), JR.JetReference(uks, p, cp, nq, rational=rat, dtype=np.float64))
        ref = c["refs"][False][0]
        rng = np.random.default_rng(sum(map(ord, name)))
        npts, nJ = ref.npts, ref.nJ
        c.update(npts=npts, nJ=nJ, nsd=ref.nsd, d=ref.d, n=ref.nnodes, u=rng.standard_normal(ref.nnodes),
                 T1=rng.standard_normal((npts, nJ, nJ)), T3=rng.standard_normal((npts, 3, nJ, 3, nJ)),
                 s1=rng.standard_normal((npts, nJ)), s3=rng.standard_normal((npts, 3, nJ)))
        _REF[name] = c
    return _REF[name]


def _dcp(T, c):
    return [T.dev.DeviceVector(data=v) for v in c["cp"]]


def _blocks(T, Tq):
    """[npts, nF, nJ, nF, nJ] (or [npts, nJ, nJ]) -> the block layout on the device"""
    Tq = np.asarray(Tq, dtype=np.float64)
    if Tq.ndim == 3:
        Tq = Tq[:, None, :, None, :]
    return T.dev.DeviceVector(data=np.ascontiguousarray(Tq.transpose(1, 3, 2, 4, 0)).ravel())


def _fields(T, s):
    s = np.asarray(s, dtype=np.float64)
    if s.ndim == 2:
        s = s[:, None, :]
    return T.dev.DeviceVector(data=np.ascontiguousarray(s.transpose(1, 2, 0)).ravel())


def _hold(label, got, want, w64):
    """normwise error of ``got`` against the longdouble ``want``; the bound from the float64 run ``w64``"""
    want = np.asarray(want)
    scale = float(np.max(np.abs(want)))
    e64 = float(np.max(np.abs(np.asarray(w64).astype(LD) - want))) / scale
    bound = max(8.0 * e64, FLOOR)
    err = float(np.max(np.abs(np.asarray(got).astype(LD) - want))) / scale
    WORST["ratio"] = max(WORST["ratio"], err / bound)
    print("%-58s error %.2e  float64 reference %.2e  bound %.2e" % (label, err, e64, bound))
    assert err <= bound, (label, err, bound)


def _hold_jets(label, got, want, w64, d):
    """``_hold`` per derivative order (arrays [..., nJ]): the second derivatives scale with 1 / h^2 and would hide the error of
    the values and of the first derivatives in one norm over the whole jet"""
    for order, sl in (("values", slice(0, 1)), ("first derivatives", slice(1, 1 + d)), ("second derivatives", slice(1 + d, None))):
        _hold("%s, %s" % (label, order), np.asarray(got)[..., sl], np.asarray(want)[..., sl], np.asarray(w64)[..., sl])


def _gpu_matrix(T, c, dcp, Tq, nF, rational):
    coef = T.dev.jet_transform(c["uks"], c["p"], dcp, _blocks(T, Tq), nF * nF, nq=c["nq"], rational=rational)
    return T.dev.assemble_jet_blocks(c["uks"], c["p"], dcp, coef, nF, nq=c["nq"])


def _gpu_load(T, c, dcp, s, nF, rational):
    st = T.dev.jet_load_transform(c["uks"], c["p"], dcp, _fields(T, s), nF, nq=c["nq"], rational=rational)
    return T.dev.quad_load_jet(c["uks"], c["p"], dcp, st, nF, nq=c["nq"])


@pytest.mark.parametrize("name", NAMES)
def test_jets_of_a_field_and_of_the_geometry(T, name):
    c = _case(name)
    dcp, nJ, npts = _dcp(T, c), c["nJ"], c["npts"]
    u = T.dev.DeviceVector(data=c["u"])
    for rat in (False, True):
        ref, r64 = c["refs"][rat]
        got = T.dev.quad_jet(c["uks"], c["p"], dcp, u, nq=c["nq"], rational=rat).get_local().reshape(nJ, npts).T
        _hold_jets("%s jets rational=%d" % (name, rat), got, ref.jets(c["u"]), r64.jets(c["u"]), c["d"])
    ref, r64 = c["refs"][False]
    got = T.dev.quad_geometry_jet(c["uks"], c["p"], dcp, nq=c["nq"]).get_local().reshape(c["nsd"], nJ, npts).transpose(2, 0, 1)
    _hold_jets("%s geometry jets" % name, got, ref.geometry_jets(), r64.geometry_jets(), c["d"])


@pytest.mark.parametrize("name", NAMES)
def test_matrix_of_random_point_data(T, name):
    """nF = 1 and the nine blocks of nF = 3, T random and not symmetric, plain and rational"""
    c = _case(name)
    dcp = _dcp(T, c)
    for rat in (False, True):
        ref, r64 = c["refs"][rat]
        for nF, Tq in ((1, c["T1"]), (3, c["T3"])):
            K = _gpu_matrix(T, c, dcp, Tq, nF, rat).to_scipy()
            assert K.shape == (nF * c["n"], nF * c["n"])
            _hold("%s matrix nF=%d rational=%d" % (name, nF, rat), K.toarray(), ref.matrix(Tq), r64.matrix(Tq))


@pytest.mark.parametrize("name", NAMES)
def test_load_of_random_point_data(T, name):
    c = _case(name)
    dcp = _dcp(T, c)
    for rat in (False, True):
        ref, r64 = c["refs"][rat]
        for nF, s in ((1, c["s1"]), (3, c["s3"])):
            b = _gpu_load(T, c, dcp, s, nF, rat).get_local()
            _hold("%s load nF=%d rational=%d" % (name, nF, rat), b, ref.load(s), r64.load(s))


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_nine_blocks_are_nine_single_blocks_and_runs_repeat(T, name):
    """``tg_jet_transform`` with nblk = 9 equals nine calls with nblk = 1 bit for bit (the geometry of a point is formed once, the
    arithmetic of a block does not change); two runs of every entry point give the same bits"""
    c = _case(name)
    dcp, nJ, npts = _dcp(T, c), c["nJ"], c["npts"]
    each = nJ * nJ * npts
    u = T.dev.DeviceVector(data=c["u"])
    for rat in (False, True):
        Tb = _blocks(T, c["T3"])
        nine = T.dev.jet_transform(c["uks"], c["p"], dcp, Tb, 9, nq=c["nq"], rational=rat).get_local()
        host = Tb.get_local()
        for b in range(9):
            one = T.dev.jet_transform(c["uks"], c["p"], dcp, T.dev.DeviceVector(data=host[b * each:(b + 1) * each]), 1, nq=c["nq"], rational=rat)
            assert np.array_equal(_bits(one.get_local()), _bits(nine[b * each:(b + 1) * each])), (name, rat, b)
        runs = []
        for _ in range(2):
            K = _gpu_matrix(T, c, dcp, c["T3"], 3, rat).to_scipy()
            runs.append([T.dev.quad_jet(c["uks"], c["p"], dcp, u, nq=c["nq"], rational=rat).get_local(),
                         T.dev.quad_geometry_jet(c["uks"], c["p"], dcp, nq=c["nq"]).get_local(),
                         T.dev.jet_transform(c["uks"], c["p"], dcp, Tb, 9, nq=c["nq"], rational=rat).get_local(),
                         T.dev.jet_load_transform(c["uks"], c["p"], dcp, _fields(T, c["s3"]), 3, nq=c["nq"], rational=rat).get_local(),
                         K.data, K.indices.astype(np.float64), _gpu_load(T, c, dcp, c["s3"], 3, rat).get_local()])
        for a, b in zip(*runs):
            assert np.array_equal(_bits(a), _bits(b))


# ---- cross-checks against existing code --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plane_p2_3x2", "annulus_p2_3x2", "cylinder_p3_2x3", "curved_p2_3x2", "curve3_p2_5"])
def test_value_and_gradient_slots_are_the_mass_and_laplace_forms(T, name):
    """T with only the (0, 0) entry set is the mass form; first-derivative entries g^-1 (the metric of the geometry jets,
    inverted on the host) are the Laplace form: the jet matrix and the mapped forms are both held to the reference's bound"""
    c = _case(name)
    dcp, nJ, npts, d = _dcp(T, c), c["nJ"], c["npts"], c["d"]
    gj = T.dev.quad_geometry_jet(c["uks"], c["p"], dcp, nq=c["nq"]).get_local().reshape(c["nsd"], nJ, npts).transpose(2, 0, 1)
    DF = gj[:, :, 1:1 + d]
    gi = np.linalg.inv(np.einsum("qik,qim->qkm", DF, DF))
    Tm, Tl = np.zeros((npts, nJ, nJ)), np.zeros((npts, nJ, nJ))
    Tm[:, 0, 0] = 1.0
    Tl[:, 1:1 + d, 1:1 + d] = gi
    for rat in (False, True):
        ref, r64 = c["refs"][rat]
        for form, Tq in (("mass", Tm), ("laplace", Tl)):
            K = _gpu_matrix(T, c, dcp, Tq, 1, rat).to_scipy().toarray()
            A = T.dev.assemble_mapped_matrix(c["uks"], c["p"], dcp, form, nq=c["nq"], rational=rat).to_scipy().toarray()
            want, w64 = ref.matrix(Tq), r64.matrix(Tq)
            _hold("%s %s rational=%d: jet matrix" % (name, form, rat), K, want, w64)
            _hold("%s %s rational=%d: mapped form" % (name, form, rat), A, want, w64)


def test_second_derivative_slots_are_the_biharmonic_form(T):
    """unmapped patch, uniform knots: entries 1 at every (kk, mm) pair of second-derivative slots is int lap u lap v, the
    Kronecker-sum ``BiharmonicForm()``; through ``forms.JetCoefficientForm`` on a generator"""
    p = 3
    kvs = [T.B.uniformKnots(p, 0.0, 1.0, 3), T.B.uniformKnots(p, 0.0, 2.0, 2)]
    gen = T.t.EqualOrderSpline(1, T.B.ExplicitBSplineControlMesh([p, p], kvs))
    Tq = np.zeros((6, 6))
    for a in (3, 5):
        for b in (3, 5):
            Tq[a, b] = 1.0
    form = T.F.JetCoefficientForm(gen, Tq)
    assert form.symmetric is True
    K = form.assemble_matrix(gen.V).to_scipy().toarray()
    A = T.F.BiharmonicForm().assemble_matrix(gen.V).to_scipy().toarray()
    g = gen.V.grids[0]
    uks, cp = [np.asarray(v) for v in g.vertices], [f.vector().get_local() for f in gen.cpFuncs]
    ref, r64 = JR.JetReference(uks, p, cp), JR.JetReference(uks, p, cp, dtype=np.float64)
    Tp = np.tile(Tq, (ref.npts, 1, 1))
    _hold("biharmonic: jet matrix", K, ref.matrix(Tp), r64.matrix(Tp))
    _hold("biharmonic: Kronecker form", A, ref.matrix(Tp), r64.matrix(Tp))


@pytest.mark.parametrize("name", ["annulus_p3_2x3_nq3", "curved_p2_3x2"])
def test_load_of_T_jet_u_is_the_matrix_applied_to_u(T, name):
    c = _case(name)
    dcp, nJ, npts = _dcp(T, c), c["nJ"], c["npts"]
    u = T.dev.DeviceVector(data=c["u"])
    for rat in (False, True):
        ref, r64 = c["refs"][rat]
        J = T.dev.quad_jet(c["uks"], c["p"], dcp, u, nq=c["nq"], rational=rat).get_local().reshape(nJ, npts).T
        b = _gpu_load(T, c, dcp, np.einsum("qab,qb->qa", c["T1"], J), 1, rat).get_local()
        Ku = _gpu_matrix(T, c, dcp, c["T1"], 1, rat).to_scipy() @ c["u"]
        want, w64 = ref.matrix(c["T1"]) @ c["u"].astype(LD), r64.matrix(c["T1"]) @ c["u"]
        _hold("%s load of T jet(u) rational=%d" % (name, rat), b, want, w64)
        _hold("%s K u rational=%d" % (name, rat), Ku, want, w64)


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def _surface_spline(T, p, nels, homogeneous, nF):
    kvs, C = SR.control_net(p, nels, homogeneous)
    gen = T.t.EqualOrderSpline(nF, T.N.NURBSControlMesh([p, p], kvs, C))
    return kvs, C, gen


def test_spline_methods_and_forms_in_a_linear_problem(T):
    """``evaluateJetsAtQuadrature`` / ``geometryJetsAtQuadrature`` on an ExtractedSpline of the cylinder surface (three fields: a
    list), and a(u, v) = sum_q wdet (jet v)^T T (jet u) = L(v) with random symmetric positive point data solved through
    ``Sum``, ``Equation`` and ``solveLinearVariationalProblem`` against the dense host solve of the reference's matrices"""
    p = 2
    kvs, C, gen = _surface_spline(T, p, (3, 2), SR.cylinder_homogeneous(), 3)
    spline = T.t.ExtractedSpline(gen, 2 * p)
    pb = SR.problem(p, (3, 2), SR.cylinder_homogeneous())
    ref, r64 = (JR.JetReference(pb["uks"], p, pb["cp"], rational=True, dtype=dt) for dt in (LD, np.float64))
    n, npts = ref.nnodes, ref.npts
    rng = np.random.default_rng(11)
    un = rng.standard_normal(3 * n)
    u = T.t.Function(spline.V)
    u.vector().set_local(un)
    jets = spline.evaluateJetsAtQuadrature(u, rational=True)
    assert isinstance(jets, list) and len(jets) == 3
    got = np.stack([j.get_local().reshape(6, npts).T for j in jets], axis=1)
    _hold_jets("spline: jets of three fields", got, ref.field_jets(un, 3), r64.field_jets(un, 3), 2)
    gj = spline.geometryJetsAtQuadrature().get_local().reshape(3, 6, npts).transpose(2, 0, 1)
    _hold_jets("spline: geometry jets", gj, ref.geometry_jets(), r64.geometry_jets(), 2)
    # a symmetric positive definite problem: T = B^T B + a mass term per field
    Bq = rng.standard_normal((npts, 18, 18))
    Tq = np.einsum("qki,qkj->qij", Bq, Bq) * 1e-3
    Tq = (0.5 * (Tq + Tq.transpose(0, 2, 1))).reshape(npts, 3, 6, 3, 6)          # (symmetric in its bits)
    Tm = np.zeros((3, 6, 3, 6))
    for i in range(3):
        Tm[i, 0, i, 0] = 1.0
    s = rng.standard_normal((npts, 3, 6))
    lhs = T.F.Sum(T.F.VectorJetCoefficientForm(spline, Tq, rational=True), (2.0, T.F.VectorJetCoefficientForm(spline, Tm, rational=True)))
    assert lhs.symmetric is True
    w = T.t.Function(spline.V)
    spline.setSolverOptions(linearSolver=T.t.PETScLUSolver())
    U = spline.solveLinearVariationalProblem(T.F.Equation(lhs, T.F.VectorJetLoadForm(s, spline, rational=True)), w)
    Mc = np.asarray(pb["Mc"].todense())
    Tt = Tq + 2.0 * Tm[None]
    want = None
    for r in (ref, r64):
        K, b = Mc.T.astype(r.dtype) @ r.matrix(Tt) @ Mc.astype(r.dtype), Mc.T.astype(r.dtype) @ r.load(s)
        sol = np.linalg.solve(K.astype(np.float64), b.astype(np.float64))
        if r is ref:                                  # one step of refinement in longdouble
            sol = sol.astype(LD) + np.linalg.solve(K.astype(np.float64), (b - K @ sol.astype(LD)).astype(np.float64)).astype(LD)
            want = sol
        else:
            w64 = sol
    _hold("spline: solution of the linear problem", U.get_local(), want, w64)
    # blocks
    form = T.F.VectorJetCoefficientForm(spline, Tq, rational=True)
    K12 = form.assemble_block(spline.V, 1, 2).to_scipy().toarray()
    _hold("spline: block (1, 2)", K12, ref.matrix(Tq)[n:2 * n, 2 * n:], r64.matrix(Tq)[n:2 * n, 2 * n:])
    assert T.F.VectorJetCoefficientForm(spline, rng.standard_normal((npts, 3, 6, 3, 6))).symmetric is False


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _calls(F, np_):
    return (lambda s: F.VectorJetCoefficientForm(s, lambda x: np_.zeros((x.shape[0], len(s.V.grids), 6, len(s.V.grids), 6))).assemble_matrix(s.V),
            lambda s: F.VectorJetLoadForm(lambda x: np_.zeros((x.shape[0], len(s.V.grids), 6)), s).assemble_vector(s.V),
            lambda s: s.evaluateJetsAtQuadrature(np_.zeros(s.V.dim())), lambda s: s.geometryJetsAtQuadrature())


@pytest.fixture(scope="module")
def surface(T):
    kvs, C, gen = _surface_spline(T, 2, (3, 2), SR.doubly_curved_homogeneous, 3)
    return T.t.ExtractedSpline(gen, 4)


@pytest.mark.parametrize("what,word", [("_distributed", "ranks"), ("_implicit", "row blocks"), ("_caller_ordered", "feOrder")])
def test_refuses_ranks_streaming_and_caller_order(T, surface, monkeypatch, what, word):
    monkeypatch.setattr(surface, what, lambda: True)
    for call in _calls(T.F, np):
        with pytest.raises(NotImplementedError, match=word):
            call(surface)


def test_refuses_row_blocks(T, surface):
    V, n = surface.V, surface.V.grids[0].num_nodes()
    Tq, s = np.zeros((3, 6, 3, 6)), np.zeros((3, 6))
    for call in (lambda: T.F.VectorJetCoefficientForm(surface, Tq).assemble_matrix(V, 0, n), lambda: T.F.VectorJetCoefficientForm(surface, Tq).assemble_block(V, 0, 1, 0, 3),
                 lambda: T.F.VectorJetLoadForm(s, surface).assemble_vector(V, n, 3 * n)):
        with pytest.raises(NotImplementedError, match="row blocks"):
            call()


def test_refuses_three_parametric_directions(T):
    kv = [T.B.uniformKnots(2, 0.0, 1.0, 2)] * 3
    vol = T.t.ExtractedSpline(T.t.EqualOrderSpline(1, T.B.ExplicitBSplineControlMesh([2, 2, 2], kv)), 4)
    for call in _calls(T.F, np):
        with pytest.raises(NotImplementedError, match="d = 3"):
            call(vol)
    g = vol.V.grids[0]
    uks, dcp = [np.asarray(v) for v in g.vertices], [f.vector() for f in vol.cpFuncs]
    with pytest.raises(NotImplementedError, match="d = 3"):
        T.dev.quad_geometry_jet(uks, 2, dcp)


def test_refuses_field_list_spaces(T):
    B, t = T.B, T.t
    kv2 = [B.uniformKnots(2, 0.0, 1.0, 3)] * 2
    cm = B.ExplicitBSplineControlMesh([2, 2], kv2)
    lst = t.ExtractedSpline(t.FieldListSpline(cm, [B.BSpline([2, 2], kv2), B.BSpline([3, 3], [B.uniformKnots(3, 0.0, 1.0, 3)] * 2)]), 4)
    for call in _calls(T.F, np):
        with pytest.raises(NotImplementedError, match="FieldListSpline"):
            call(lst)


def test_refuses_compatible_spaces(T):
    from tigar_amd.compatibleSplines import BSplineCompat
    cm = T.B.ExplicitBSplineControlMesh([2, 2], [T.B.uniformKnots(2, 0.0, 1.0, 3)] * 2)
    s = T.t.ExtractedSpline(BSplineCompat(cm, "RT", [1, 1]), 4)
    for call in _calls(T.F, np):
        with pytest.raises(NotImplementedError, match="not supported"):
            call(s)


def test_refuses_dg_spaces(T):
    kvd = [0, 0, 0, 0.5, 0.5, 0.5, 1, 1, 1]
    dg = T.t.ExtractedSpline(T.t.EqualOrderSpline(2, T.B.ExplicitBSplineControlMesh([2, 2], [kvd, kvd])), 4)
    for call in _calls(T.F, np):
        with pytest.raises(NotImplementedError, match="DG"):
            call(dg)


def test_refuses_several_patches(T):
    B, t = T.B, T.t
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
    s = t.ExtractedSpline(t.EqualOrderSpline(2, TwoPatches()), 4)
    for call in _calls(T.F, np):
        with pytest.raises(NotImplementedError, match="not supported"):
            call(s)


def test_refuses_t_splines(T):
    from tigar_amd.RhinoTSplines import RhinoTSplineControlMesh
    s = T.t.ExtractedSpline(T.t.EqualOrderSpline(2, RhinoTSplineControlMesh(
        os.path.join(os.path.dirname(__file__), "golden", "tspline_bicubic_patch.iga"))), 4)
    for call in _calls(T.F, np):
        with pytest.raises(NotImplementedError, match="not supported"):
            call(s)


def test_bad_arguments(T, surface):
    F, V = T.F, surface.V
    npts = surface.geometryJetsAtQuadrature().size() // 18
    for make in (lambda: F.VectorJetCoefficientForm(None, np.zeros((3, 6, 3, 6))), lambda: F.JetLoadForm(np.zeros(6), None)):
        with pytest.raises(ValueError, match="geometry"):
            make()
    for bad in (np.zeros((npts, 3, 6, 3)), np.zeros((npts + 1, 3, 6, 3, 6)), T.dev.DeviceVector(324 * npts + 1)):
        with pytest.raises(ValueError, match="shape|values"):
            F.VectorJetCoefficientForm(surface, bad).assemble_matrix(V)
    for bad in (np.zeros((npts, 3, 5)), T.dev.DeviceVector(npts)):
        with pytest.raises(ValueError, match="shape|values"):
            F.VectorJetLoadForm(bad, surface).assemble_vector(V)
    with pytest.raises(ValueError, match="block"):
        F.VectorJetCoefficientForm(surface, np.zeros((3, 6, 3, 6))).assemble_block(V, 0, 3)
    with pytest.raises(NotImplementedError, match="nFields"):
        F.JetCoefficientForm(surface, np.zeros((6, 6))).assemble_matrix(V)
    with pytest.raises(ValueError, match="nodal values"):
        surface.evaluateJetsAtQuadrature(np.zeros(5))
    # the C entries check their arguments themselves
    g = V.grids[0]
    uks, dcp = [np.asarray(v) for v in g.vertices], [f.vector() for f in surface.cpFuncs]
    with pytest.raises(T.dev.TigarHipError):
        T.dev.jet_transform(uks, 2, dcp, T.dev.DeviceVector(36 * npts - 1), 1)
    with pytest.raises(T.dev.TigarHipError):
        T.dev.assemble_jet_blocks(uks, 2, dcp, T.dev.DeviceVector(36 * npts), 3)
    with pytest.raises(T.dev.TigarHipError):
        T.dev.quad_load_jet(uks, 2, dcp, T.dev.DeviceVector(6 * npts), 3)
