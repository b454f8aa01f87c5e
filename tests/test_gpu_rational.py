"""GPU: rational (NURBS) trial and test functions, ``rational=True`` -- the element kernels of csrc/tg_assemble.hip and the
point kernel of csrc/tg_postproc.hip against the host reference of tests/rational_reference.py (which forms phi / W_h and
its gradient directly, not through the transformed coefficient tensor of the kernels), and what is built on them: the
forms, errorNorm / projectDofs / project / evaluateAtQuadrature / rationalize, the Krylov and the streamed path on the
rational K.

Matrices are held to 1e-12 max|A| and loads to 1e-13 max|b|, the tolerances tests/test_gpu_assembly.py applies to the
un-rationalised kernels.  Point fields and sums are held NORMWISE against the longdouble reference, max |error| / max
|reference| (fields) and |error| / scale (sums: the scale is sum wdet (|u| + |e|)^2 and its analogue for the gradients):
the bounds are 4 x the largest figures observed on the MI355X over the cases of this file, which leaves room for another
order of the reductions --

    fields  FIELDS_MEASURED = 38.5 eps   the gradient of a SMOOTH field of the space, w l(x) with l linear, on the quarter
                                         annulus of 5 x 5 elements (test_linear_functions_through_the_api; 9.62 on 3 x 3
                                         elements): it is small against the nodal differences it is formed from,
                                         (grad u_h W - u_h grad W) / W^2 cancels.  Random nodal fields, whose gradients are as
                                         large as their differences: load 4.53 (annulus, nq = 3), gradient 3.87, values 1.24
    sums    SUMS_MEASURED   = 4.42 eps   sum 2 on the rational volume; sum 1 3.13, sum 0 2.32 there

The rational errorNorm of a linear function (test_linear_functions_through_the_api) is held to the measured figure itself,
FIELDS_MEASURED eps times the H1 norm of the function; observed 6.60 eps |l|_H1.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from oracle import tigar_oracle as O
import postproc_reference as R
import rational_reference as RR

pytestmark = pytest.mark.gpu

EPS = R.EPS
FIELDS_MEASURED, SUMS_MEASURED = 38.5, 4.42
NORMWISE_FIELDS = 4 * FIELDS_MEASURED
NORMWISE_SUMS = 4 * SUMS_MEASURED
LAM, MU = 1.3, 0.7


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


# ---- patches -----------------------------------------------------------------------------------------------------------------
def _annulus_nodes(nels):
    """the exact quarter annulus on a mesh of nels[0] x nels[1] elements: its homogeneous coordinates are quadratics in the
    parameters, which the Q_2 nodal interpolation on any mesh reproduces -- the one-element control functions evaluated at
    the nodes of the finer mesh"""
    uks1, cp1 = R.annulus_patch(1)
    uks = [np.linspace(0.0, 1.0, n + 1) for n in nels]
    X = R.lagrange_nodes(uks, 2)
    l = lambda t: np.stack([2.0 * (t - 0.5) * (t - 1.0), -4.0 * t * (t - 1.0), 2.0 * t * (t - 0.5)])      # nodes 0, 1/2, 1
    L0, L1 = l(X[0]), l(X[1])
    cp = [np.einsum("an,bn,ab->n", L0, L1, np.asarray(c).reshape(3, 3, order="F")) for c in cp1]
    return uks, cp


def _weighted_nodes(nels, p, nsd=None):
    """non-uniform element vertices, a smooth non-affine map and a weight that varies by a third, given on the Q_p nodes"""
    d = len(nels)
    rng = np.random.default_rng(7 * d + p)
    uks = []
    for k in range(d):
        steps = rng.uniform(0.6, 1.4, nels[k])
        uks.append(np.concatenate([[0.0], np.cumsum(steps) / np.sum(steps) * (1.0 + 0.5 * k)]))
    X = R.lagrange_nodes(uks, p)
    wgt = 1.0 + 0.3 * X[0] * X[-1] + 0.1 * X[0] ** 2
    coords = [X[i] + 0.1 * X[(i + 1) % d] ** 2 for i in range(d)]
    if nsd is not None and nsd > d:
        coords.append(X[0] ** 2 + X[-1])
    return uks, [c * wgt for c in coords] + [wgt]


PLAIN = {
    "1d_p3_3": lambda: (3, None) + _weighted_nodes((3,), 3),
    "annulus_3x2_nq3": lambda: (2, 3) + _annulus_nodes((3, 2)),
    "annulus_3x2_nq4": lambda: (2, 4) + _annulus_nodes((3, 2)),
    "surface_in_3d_p2_2x2": lambda: (2, None) + _weighted_nodes((2, 2), 2, nsd=3),
    "volume_p1_2x2x2": lambda: (1, None) + R.volume_patch(1, (2, 2, 2)),
    "volume_p4_1x2x1": lambda: (4, None) + R.volume_patch(4, (1, 2, 1)),
    # nq = 9 in 3-D: the un-rationalised forms fill the 64 KiB a launch gets by itself (p = 4: 64 472 B), the rational
    # stiffness and elasticity need beta on top and ask for more
    "volume_p1_1x1x1_nq9": lambda: (1, 9) + R.volume_patch(1, (1, 1, 1)),
    "volume_p4_1x1x1_nq9": lambda: (4, 9) + R.volume_patch(4, (1, 1, 1)),
}
SUMFAC = {
    # three pieces of the walk with a partial one, an odd number of lines (a wave holds one line of two), two z layers
    "volume_p2_5x3x2": (2, (5, 3, 2), {"TIGAR_ASM_CHUNK": "2"}),
    # a full group of four elements and a partial one, a workgroup per group
    "volume_p3_6x2x2": (3, (6, 2, 2), {"TIGAR_ASM_QUAD_CHUNK": "1"}),
    # ... and the default pieces: the workgroup loops over its groups
    "volume_p3_6x2x2_default_pieces": (3, (6, 2, 2), {}),
}
_REF = {}


def _host(name, p, nq, uks, cp):
    """reference matrices and loads of one patch: computed once and shared"""
    if name not in _REF:
        cp = [np.asarray(c, dtype=np.float64) for c in cp]
        x = RR.physical_nodes(cp)
        fn = np.sin(2.0 * x[:, 0]) + 0.5 * x[:, -1] ** 2
        M, K, b, _ = RR.rational_fe_system(uks, p, cp, nq=nq, fnodal=fn)
        E = RR.rational_elasticity_fe_system(uks, p, cp, LAM, MU, nq=nq) if len(cp) - 1 == len(uks) else None
        _REF[name] = dict(p=p, nq=nq, uks=uks, cp=cp, fn=fn, M=M, K=K, b=b, E=E)
    return _REF[name]


def _plain_case(name):
    if name not in _REF:
        _host(name, *PLAIN[name]())
    return _REF[name]


def _sumfac_case(name):
    if name not in _REF:
        p, nels, _ = SUMFAC[name]
        uks, cp = R.volume_patch(p, nels)
        _host(name, p, None, uks, cp)
    return _REF[name]


def _dcp(T, c):
    return [T.dev.DeviceVector(data=v) for v in c["cp"]]


def _close(A, Ao, scale=None, tol=1e-12):
    A = A.to_scipy() if hasattr(A, "to_scipy") else A
    assert A.shape == Ao.shape
    assert abs(A - Ao).max() <= tol * (abs(Ao).max() if scale is None else scale)
    assert A.nnz >= Ao.nnz


def _assemble_all(T, c, dcp=None):
    dcp = _dcp(T, c) if dcp is None else dcp
    a = (c["uks"], c["p"], dcp)
    M = T.dev.assemble_mapped_matrix(*a, "mass", nq=c["nq"], rational=True)
    K = T.dev.assemble_mapped_matrix(*a, "laplace", nq=c["nq"], rational=True)
    b = T.dev.assemble_mapped_load(*a, T.dev.DeviceVector(data=c["fn"]), nq=c["nq"], rational=True)
    return M, K, b


# ---- the plain element kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_plain_kernel_matches_the_reference(T, name):
    c = _plain_case(name)
    assert np.ptp(c["cp"][-1]) > 0.05                                   # the weights do vary
    M, K, b = _assemble_all(T, c)
    _close(M, c["M"])
    _close(K, c["K"])
    assert np.max(np.abs(b.get_local() - c["b"])) <= 1e-13 * np.max(np.abs(c["b"]))
    # the rational space is another one: the un-rationalised matrix is far from this one
    Ku = T.dev.assemble_mapped_matrix(c["uks"], c["p"], _dcp(T, c), "laplace", nq=c["nq"]).to_scipy()
    assert abs(Ku - c["K"]).max() > 1e-3 * abs(c["K"]).max()
    if c["E"] is not None:
        d, N = len(c["uks"]), c["M"].shape[0]
        for i in range(d):
            for j in range(d):
                B = T.dev.assemble_mapped_elasticity_block(c["uks"], c["p"], _dcp(T, c), i, j, LAM, MU, nq=c["nq"], rational=True)
                _close(B, c["E"][i * N:(i + 1) * N, j * N:(j + 1) * N], scale=abs(c["E"]).max())
    else:
        with pytest.raises(T.dev.TigarHipError):
            T.dev.assemble_mapped_elasticity_block(c["uks"], c["p"], _dcp(T, c), 0, 1, LAM, MU, rational=True)


def test_no_rational_biharmonic_form(T):
    c = _plain_case("annulus_3x2_nq3")
    with pytest.raises(ValueError):
        T.dev.assemble_mapped_matrix(c["uks"], c["p"], _dcp(T, c), "biharmonic", rational=True)


# ---- the sum-factorised path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SUMFAC))
def test_sum_factorised_path(T, name, monkeypatch, capfd):
    c = _sumfac_case(name)
    p, nels, env = SUMFAC[name]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    dcp = _dcp(T, c)
    monkeypatch.setenv("TIGAR_ASM_TIME", "1")
    capfd.readouterr()
    M, K, b = _assemble_all(T, c, dcp)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[tg_assemble]")]
    monkeypatch.delenv("TIGAR_ASM_TIME")
    assert len(lines) == 3 and all("rational" in ln and "sum-factorised" in ln for ln in lines), lines
    _close(M, c["M"])
    _close(K, c["K"])
    M, K, b = M.to_scipy(), K.to_scipy(), b.get_local()
    assert np.max(np.abs(b - c["b"])) <= 1e-13 * np.max(np.abs(c["b"]))
    # two runs give the same bits
    M2, K2, b2 = _assemble_all(T, c, dcp)
    for a, a2 in ((M.data, M2.to_scipy().data), (K.data, K2.to_scipy().data), (b, b2.get_local())):
        assert np.array_equal(a.view(np.int64), a2.view(np.int64))
    # the row blocks of single node planes, from windows of the control functions, are the rows of the whole matrix
    n0, n1, n2 = [e * p + 1 for e in nels]
    plane = n0 * n1
    parts = {"mass": [], "laplace": [], "load": []}
    for z in range(n2):
        e0 = z // p - 1 if (z > 0 and z % p == 0) else z // p
        e1 = min(nels[2], z // p + 1)
        fa, fb = e0 * p, e1 * p + 1
        win = [T.dev.DeviceVector(data=v[fa * plane:fb * plane]) for v in c["cp"]]
        rows = dict(row0=z * plane, row1=(z + 1) * plane, cp_node0=fa * plane, rational=True)
        for f in ("mass", "laplace"):
            parts[f].append(T.dev.assemble_mapped_matrix(c["uks"], p, win, f, **rows).to_scipy())
        parts["load"].append(T.dev.assemble_mapped_load(c["uks"], p, win, T.dev.DeviceVector(data=c["fn"][fa * plane:fb * plane]),
                                                        **rows).get_local())
    for f, whole in (("mass", M), ("laplace", K)):
        S = sps.vstack(parts[f]).tocsr()
        assert np.array_equal(S.indptr, whole.indptr) and np.array_equal(S.indices, whole.indices)
        assert np.array_equal(S.data.view(np.int64), whole.data.view(np.int64))
    assert np.array_equal(np.concatenate(parts["load"]).view(np.int64), b.view(np.int64))
    # the plain kernel gives the same values
    monkeypatch.setenv("TIGAR_ASM_LEGACY", "1")
    monkeypatch.setenv("TIGAR_ASM_TIME", "1")
    capfd.readouterr()
    Ml, Kl, bl = _assemble_all(T, c, dcp)
    assert "plain" in capfd.readouterr().err
    monkeypatch.delenv("TIGAR_ASM_LEGACY")
    monkeypatch.delenv("TIGAR_ASM_TIME")
    for a, al in ((M, Ml.to_scipy()), (K, Kl.to_scipy())):
        assert np.array_equal(a.indptr, al.indptr) and np.array_equal(a.indices, al.indices)
        assert abs(a - al).max() <= 1e-12 * abs(al).max()
    assert np.max(np.abs(b - bl.get_local())) <= 1e-12 * np.max(np.abs(b))


# ---- identities on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["annulus_3x2_nq3", "volume_p4_1x2x1", "volume_p2_5x3x2", "volume_p3_6x2x2_default_pieces"])
def test_stiffness_annihilates_the_weights(T, name):
    c = _plain_case(name) if name in PLAIN else _sumfac_case(name)
    K = T.dev.assemble_mapped_matrix(c["uks"], c["p"], _dcp(T, c), "laplace", nq=c["nq"], rational=True)
    kw = K.mult(T.dev.DeviceVector(data=c["cp"][-1])).get_local()
    assert np.max(np.abs(kw)) <= 1e-12 * abs(c["K"]).max()


@pytest.mark.parametrize("d,p,nels", [(1, 3, (3,)), (2, 2, (3, 2)), (3, 2, (3, 2, 2)), (3, 3, (5, 2, 1)), (3, 1, (2, 2, 2))])
def test_unit_weights_give_the_unrationalised_forms(T, d, p, nels):
    B, t, dev = T.B, T.t, T.dev
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * d, [B.uniformKnots(p, 0.0, 1.0 + 0.5 * k, nels[k]) for k in range(d)]))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k]) for k in range(d)]
    X = [gen.cpFuncs[i].vector().get_local() for i in range(d)]
    cp = [X[i] + 0.1 * X[(i + 1) % d] ** 2 for i in range(d)] + [np.ones_like(X[0])]      # a non-affine map, unit weights
    dcp = [dev.DeviceVector(data=v) for v in cp]
    rng = np.random.default_rng(3)
    fn = dev.DeviceVector(data=rng.standard_normal(cp[0].size))
    for form in ("mass", "laplace"):
        A0 = dev.assemble_mapped_matrix(uks, p, dcp, form).to_scipy()
        A1 = dev.assemble_mapped_matrix(uks, p, dcp, form, rational=True).to_scipy()
        assert np.array_equal(A0.indices, A1.indices) and abs(A0 - A1).max() <= 1e-12 * abs(A0).max()
    if d > 1:
        E0 = dev.assemble_mapped_elasticity_block(uks, p, dcp, 0, d - 1, LAM, MU).to_scipy()
        E1 = dev.assemble_mapped_elasticity_block(uks, p, dcp, 0, d - 1, LAM, MU, rational=True).to_scipy()
        assert abs(E0 - E1).max() <= 1e-12 * abs(E0).max()
    b0, b1 = [dev.assemble_mapped_load(uks, p, dcp, fn, rational=r).get_local() for r in (False, True)]
    assert np.max(np.abs(b0 - b1)) <= 1e-12 * np.max(np.abs(b0))
    v0, g0 = dev.quad_eval(uks, p, dcp, fn, grad=True)
    v1, g1 = dev.quad_eval(uks, p, dcp, fn, grad=True, rational=True)
    assert np.max(np.abs(v0.get_local() - v1.get_local())) <= 1e-12 * np.max(np.abs(v0.get_local()))
    assert np.max(np.abs(g0.get_local() - g1.get_local())) <= 1e-12 * np.max(np.abs(g0.get_local()))
    l0, l1 = [dev.quad_load(uks, p, dcp, v0, rational=r).get_local() for r in (False, True)]
    assert np.max(np.abs(l0 - l1)) <= 1e-12 * np.max(np.abs(l0))
    s0, s1 = [dev.quad_error(uks, p, dcp, fn, v0, g0, rational=r) for r in (False, True)]
    assert all(abs(a - b_) <= 1e-12 * max(abs(a), 1.0) for a, b_ in zip(s0, s1))
    # through the forms: the same keyword
    F = T.F
    K0 = F.LaplaceForm(geometry=gen).assemble_matrix(gen.V).to_scipy()
    K1 = F.LaplaceForm(geometry=gen, rational=True).assemble_matrix(gen.V).to_scipy()
    assert abs(K0 - K1).max() <= 1e-12 * abs(K0).max()


# ---- the point kernel --------------------------------------------------------------------------------------------------------
POINTS = {
    "annulus_nq3": lambda: (2, 3) + R.annulus_patch(3),
    "annulus_nq5": lambda: (2, 5) + R.annulus_patch(3),
    "volume_p2_2x1x2": lambda: (2, None) + R.volume_patch(2, (2, 1, 2)),
}
_PTS = {}


def _points_case(name):
    if name not in _PTS:
        p, nq, uks, cp = POINTS[name]()
        cp = [np.asarray(v, dtype=np.float64) for v in cp]
        ref = RR.RationalPoints(uks, p, cp, nq)
        rng = np.random.default_rng(len(name))
        xq = ref.x.astype(np.float64)
        e = np.sin(2.0 * xq[:, 0]) + 0.5 * xq[:, -1] ** 2
        ge = np.zeros_like(xq)
        ge[:, 0] += 2.0 * np.cos(2.0 * xq[:, 0])
        ge[:, -1] += xq[:, -1]
        xn = RR.physical_nodes(cp)
        lin = cp[-1] * (1.0 + xn @ np.array([2.0, -1.0, 0.5])[:xn.shape[1]])      # w l(x): a linear function in the rational space
        _PTS[name] = dict(p=p, nq=nq, uks=uks, cp=cp, ref=ref, u=rng.standard_normal(ref.nnodes), fq=rng.standard_normal(ref.npts),
                          e=e, ge=ge, fn=np.sin(2.0 * xn[:, 0]) + 0.5 * xn[:, -1] ** 2, lin=lin)
    return _PTS[name]


def _normwise(name, what, err, scale, bound):
    ratio = float(np.max(np.abs(err)) / np.max(np.abs(scale))) / EPS
    print("rational normwise %-20s %-6s %.2f eps" % (name, what, ratio))
    assert ratio <= bound, (name, what, ratio)


@pytest.mark.parametrize("name", sorted(POINTS))
def test_point_kernel_matches_the_reference(T, name):
    c = _points_case(name)
    ref, dv = c["ref"], T.dev.DeviceVector
    a = (c["uks"], c["p"], _dcp(T, c))
    v, g = ref.eval_rational(c["u"])
    val, grad = T.dev.quad_eval(*a, dv(data=c["u"]), grad=True, nq=c["nq"], rational=True)
    only = T.dev.quad_eval(*a, dv(data=c["u"]), nq=c["nq"], rational=True).get_local()
    val, grad = val.get_local(), grad.get_local().reshape(ref.nsd, ref.npts).T
    assert np.array_equal(only.view(np.int64), val.view(np.int64))
    _normwise(name, "val", (val - v).astype(np.float64), v, NORMWISE_FIELDS)
    _normwise(name, "grad", (grad - g).astype(np.float64), g, NORMWISE_FIELDS)
    # a smooth field of the space: its gradient is small against the nodal differences it is formed from
    vl, gl = ref.eval_rational(c["lin"])
    val_l, grad_l = T.dev.quad_eval(*a, dv(data=c["lin"]), grad=True, nq=c["nq"], rational=True)
    _normwise(name, "val_l", (val_l.get_local() - vl).astype(np.float64), vl, NORMWISE_FIELDS)
    _normwise(name, "grad_l", (grad_l.get_local().reshape(ref.nsd, ref.npts).T - gl).astype(np.float64), gl, NORMWISE_FIELDS)
    b = ref.load_rational(c["fq"])
    out = T.dev.quad_load(*a, dv(data=c["fq"]), nq=c["nq"], rational=True).get_local()
    _normwise(name, "load", (out - b).astype(np.float64), b, NORMWISE_FIELDS)
    s, m = ref.sums_rational(c["u"], c["e"], c["ge"])
    ge = dv(data=np.ascontiguousarray(c["ge"].T).ravel())
    got = T.dev.quad_error(*a, dv(data=c["u"]), dv(data=c["e"]), ge, nq=c["nq"], rational=True)
    for t in range(3):
        _normwise(name, "sum%d" % t, np.array([float(got[t] - s[t])]), np.array([float(m[t])]), NORMWISE_SUMS)
    # the flag does something on these patches
    plain = T.dev.quad_eval(*a, dv(data=c["u"]), nq=c["nq"]).get_local()
    assert np.max(np.abs(plain - val)) > 1e-3 * np.max(np.abs(val))
    # the load of the point values of a nodal interpolant is the rational nodal load of that function
    fn = dv(data=c["fn"])
    la = T.dev.quad_load(*a, T.dev.quad_eval(*a, fn, nq=c["nq"]), nq=c["nq"], rational=True).get_local()
    lb = T.dev.assemble_mapped_load(*a, fn, nq=c["nq"], rational=True).get_local()
    assert np.max(np.abs(la - lb)) <= 1e-13 * np.max(np.abs(lb))


# ---- through the API ---------------------------------------------------------------------------------------------------------
def _annulus_spline(T, nel, clamp, rtol=1e-12):
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    gen = T.t.EqualOrderSpline(1, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf))
    if clamp:
        sp0 = gen.getScalarSpline(0)
        for direction in (0, 1):
            for side in (0, 1):
                gen.addZeroDofs(0, sp0.getSideDofs(direction, side))
    spline = T.t.ExtractedSpline(gen, 4)
    solver = T.t.PETScKrylovSolver("cg", "jacobi")
    solver.parameters["relative_tolerance"] = rtol
    spline.setSolverOptions(linearSolver=solver)
    return gen, spline, kv, Pf


def test_linear_functions_through_the_api(T):
    """U_i = w_i l(P_i) is l(x) in the rational space: error at rounding level with rational=True, visible without; the
    rational projection of l returns these dofs; rationalize is the nodal quotient; rationalize=True of project still
    refuses non-unit weights"""
    gen, spline, kv, Pf = _annulus_spline(T, 5, False)
    w = Pf[:, :, 2].ravel(order="F")
    X, Y = Pf[:, :, 0].ravel(order="F") / w, Pf[:, :, 1].ravel(order="F") / w
    U0 = w * (1.0 + 2.0 * X - Y)
    lin = lambda x: 1.0 + 2.0 * x[:, 0] - x[:, 1]
    glin = lambda x: np.tile(np.array([2.0, -1.0]), (x.shape[0], 1))
    u = T.t.Function(spline.V)
    spline.M.mult(T.dev.DeviceVector(data=U0), u.vector())
    pts = spline.quadraturePoints()
    s = T.dev.quad_error(pts.verts, pts.p, pts.cp, None, pts.values(lin), pts.vector_values(glin), nq=pts.nq)
    norm_l = float(np.sqrt(s[1] + s[2]))                                                   # the H1 norm of l
    err = spline.errorNorm(u, lin, "H1", exact_grad=glin, rational=True)
    print("rational errorNorm of a linear function: %.3e = %.2f eps |l|_H1" % (err, err / (EPS * norm_l)))
    assert err <= FIELDS_MEASURED * EPS * norm_l
    assert spline.errorNorm(u, lin, "H1", exact_grad=glin, rational=False) > 1e-3
    # projection in the rational space (consistent: the function is in the space)
    rtol = 1e-12
    Mo = O.generate_M_tensor(O.BSpline([2, 2], [kv, kv]))
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k], dtype=np.float64) for k in range(2)]
    cp = [f.vector().get_local() for f in gen.cpFuncs]
    Km = O.extract_matrix(Mo, RR.rational_fe_system(uks, 2, cp)[0], None, applyBCs=False)
    kappa = np.linalg.cond(Km.toarray())
    U = spline.projectDofs(lin, rational=True).get_local()
    print("rational projection: error %.2e, kappa %.1f" % (np.max(np.abs(U - U0)), kappa))
    assert np.max(np.abs(U - U0)) <= kappa * (rtol + 64 * EPS) * np.max(np.abs(U0))
    assert spline.__dict__["_projection_mass_builds"] == 1
    Uu = spline.projectDofs(lin).get_local()                                               # another space, another matrix
    assert spline.__dict__["_projection_mass_builds"] == 2 and np.max(np.abs(Uu - U0)) > 1e-3
    uf = spline.project(lin, rational=True, rationalize=False).vector().get_local()
    assert np.max(np.abs(uf - Mo @ U)) <= 64 * EPS * np.max(np.abs(Mo @ U))
    assert spline.__dict__["_projection_mass_builds"] == 2
    # the nodal quotient: l at the nodes
    q = spline.rationalize(u).vector().get_local()
    xn = RR.physical_nodes(cp)
    assert np.max(np.abs(q - lin(xn))) <= 64 * EPS * np.max(np.abs(lin(xn)))
    # values at the points through the spline
    val, comps = spline.evaluateAtQuadrature(u, grad=True, rational=True)
    ev = np.max(np.abs(val.get_local() - lin(pts.x))) / np.max(np.abs(lin(pts.x))) / EPS
    eg = max(np.max(np.abs(comps[0].get_local() - 2.0)), np.max(np.abs(comps[1].get_local() + 1.0))) / 2.0 / EPS
    print("rational evaluateAtQuadrature of a linear function: values %.2f eps, gradient %.2f eps normwise" % (ev, eg))
    assert ev <= NORMWISE_FIELDS and eg <= NORMWISE_FIELDS
    one = lambda x: np.ones(x.shape[0])
    with pytest.raises(NotImplementedError):
        spline.project(one, rationalize=True)
    with pytest.raises(NotImplementedError):
        spline.project(one, rationalize=True, rational=True)


def test_rational_needs_a_geometry(T):
    F = T.F
    for make in (lambda: F.LaplaceForm(rational=True), lambda: F.MassForm(rational=True),
                 lambda: F.ElasticityForm(rational=True), lambda: F.NodalLoadForm(1.0, None, rational=True),
                 lambda: F.QuadratureLoadForm(1.0, None, rational=True)):
        with pytest.raises(ValueError):
            make()
    for form in (F.LaplaceForm(), F.MassForm(), F.ElasticityForm()):
        assert form.symmetric and form.rational is False
    with pytest.raises(TypeError):
        F.BiharmonicForm(rational=True)


def test_elasticity_form_holds_the_rigid_motions(T):
    """the assembled rational ElasticityForm on the annulus annihilates w r(x) for the three rigid motions r, which the
    un-rationalised one does not (it holds no rotation)"""
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(3)
    gen = T.t.EqualOrderSpline(2, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf))
    cp = [f.vector().get_local() for f in gen.cpFuncs]
    x, w = RR.physical_nodes(cp), cp[-1]
    A = T.F.ElasticityForm(LAM, MU, geometry=gen, rational=True).assemble_matrix(gen.V)
    Au = T.F.ElasticityForm(LAM, MU, geometry=gen).assemble_matrix(gen.V)
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k], dtype=np.float64) for k in range(2)]
    Eo = RR.rational_elasticity_fe_system(uks, 2, cp, LAM, MU)
    _close(A, Eo)
    amax = abs(Eo).max()
    for r in (np.stack([np.ones_like(w), 0 * w]), np.stack([0 * w, np.ones_like(w)]), np.stack([-x[:, 1], x[:, 0]])):
        v = T.dev.DeviceVector(data=(w[None, :] * r).ravel())
        assert np.max(np.abs(A.mult(v).get_local())) <= 1e-12 * amax
    assert np.max(np.abs(Au.mult(v).get_local())) > 1e-4 * amax


def test_poisson_on_the_annulus_in_the_rational_space(T):
    """demos/poisson/poisson-nurbs.py as the reference writes it -- rational trial and test functions, the error of
    rationalize(u) -- at nel = 4, 8, 16, against the host flow of tests/rational_reference.py (same quadrature, direct
    solve).  The two flows differ by the solve: CG stops at |r| <= rtol |b| (rtol = 1e-12), so that the error norms differ
    by at most |K^-1 r|: sqrt(lambda_max(M)) rtol |b| / lambda_min(K) in L2 and rtol |b| / sqrt(lambda_min(K)) in H10 (K,
    M: the extracted rational stiffness and mass matrices on the free dofs), times 10 for the preconditioned norm the
    solver may measure its residual in, plus 1e-12 of the norm for the rounding of the sums."""
    F = T.F
    rtol = 1e-12
    errs = []
    for nel in (4, 8, 16):
        gen, spline, kv, Pf = _annulus_spline(T, nel, True, rtol)
        u = T.t.Function(spline.V)
        spline.solveLinearVariationalProblem(
            F.Equation(F.LaplaceForm(geometry=gen, rational=True), F.QuadratureLoadForm(R.annulus_rhs, gen, rational=True)), u)
        l2 = spline.errorNorm(u, R.annulus_exact, "L2", rational=True)
        h10 = spline.errorNorm(u, R.annulus_exact, "H10", exact_grad=R.annulus_exact_grad, rational=True)
        hl2, hh10, Kf, Mf, bf = RR.solve_annulus_poisson(nel, matrices=True)
        lmin = float(np.linalg.eigvalsh(Kf.toarray()).min())
        mmax = float(np.linalg.eigvalsh(Mf.toarray()).max())
        nb = float(np.linalg.norm(bf))
        tol_l2 = 10.0 * np.sqrt(mmax) * rtol * nb / lmin + 1e-12 * hl2
        tol_h10 = 10.0 * rtol * nb / np.sqrt(lmin) + 1e-12 * hh10
        print("rational annulus nel %2d: L2 %.6e (host %.6e, tolerance %.1e)  H10 %.6e (host %.6e, tolerance %.1e)"
              % (nel, l2, hl2, tol_l2, h10, hh10, tol_h10))
        assert abs(l2 - hl2) <= tol_l2 and abs(h10 - hh10) <= tol_h10
        errs.append((l2, h10))
    for a, b in zip(errs[:-1], errs[1:]):
        assert a[0] / b[0] >= 7.0 and a[1] / b[1] >= 3.5


# ---- downstream paths on the rational K --------------------------------------------------------------------------------------
def _volume_generator(T, p, nels):
    from geom_util import rational_volume
    from tigar_amd import common as tc
    kvs, C = rational_volume(p, nels)
    gen = T.t.EqualOrderSpline(tc.selfcomm, 1, T.N.NURBSControlMesh([p] * 3, kvs, C))
    sp0 = gen.getScalarSpline(0)
    for direction in range(3):
        for side in (0, 1):
            gen.addZeroDofs(0, sp0.getSideDofs(direction, side))
    return gen, kvs


def _host_extracted(gen, kvs, p, load, diag=1.0):
    g = gen.V.grids[0]
    uks = [np.asarray(g.vertices[k]) for k in range(3)]
    cp = [f.vector().get_local() for f in gen.cpFuncs]
    _, Ko, bo, _ = RR.rational_fe_system(uks, p, cp, fnodal=load(RR.physical_nodes(cp)))
    Mo = O.generate_M_tensor(O.BSpline([p] * 3, [list(k) for k in kvs]))
    zd = [int(i) for i in gen.zeroDofsArray()]
    return O.extract_matrix(Mo, Ko, zd, diag=diag), O.extract_vector(Mo, bo, zd), zd


def test_fast_diagonalization_on_the_rational_stiffness(T):
    """one CG solve preconditioned by fast diagonalization on the rational K of a NURBS volume, against the host flow (the
    tolerances of tests/test_gpu_fast_diag.py::test_mapped_poisson: rtol 1e-10, the solutions within 1e-7)"""
    import scipy.sparse.linalg as spl
    p, nels = 2, (5, 4, 4)
    gen, kvs = _volume_generator(T, p, nels)
    spline = T.t.ExtractedSpline(gen, 2 * p)
    load = lambda x: 1.0 + x[:, 0] * x[:, 2]
    K = spline.assembleMatrix(T.F.LaplaceForm(geometry=gen, rational=True))
    b = spline.assembleVector(T.F.NodalLoadForm(load, gen, rational=True))
    solver = T.t.PETScKrylovSolver("cg", "fast_diagonalization")
    solver.parameters["relative_tolerance"] = 1e-10
    spline.setSolverOptions(linearSolver=solver)
    U = spline.solveLinearSystem(K, b, T.t.Function(spline.V)).get_local()
    assert solver.last["preconditioner"] == "fast_diagonalization"
    print("fast diagonalization on the rational K, %s elements p = %d: %d iterations" % (nels, p, solver.last["iterations"]))
    Kr, br, zd = _host_extracted(gen, kvs, p, load)
    Ur = spl.spsolve(Kr.tocsc(), br)
    assert np.linalg.norm(U - Ur) <= 1e-7 * np.linalg.norm(Ur)


def test_rational_forms_streamed_through_the_slab_engine(T, monkeypatch):
    """the rational forms hand out row blocks like their twins: operator implicit, patch streamed in sub-slabs of dof planes
    (set up as tests/test_gpu_assembly.py::test_mapped_forms_streamed_through_the_slab_engine, same tolerances)"""
    monkeypatch.setenv("TIGAR_IMPLICIT_M", "1")
    monkeypatch.setenv("TIGAR_SUB_PLANES", "3")
    p, nels = 2, (4, 3, 6)
    gen, kvs = _volume_generator(T, p, nels)
    assert getattr(gen.M, "is_implicit", False)
    spline = T.t.ExtractedSpline(gen, 2 * p, comm=gen.comm)
    load = lambda x: np.sin(x[:, 0]) + x[:, 1] * x[:, 2]
    T.dev.prof_reset()
    K = spline.assembleMatrix(T.F.LaplaceForm(geometry=gen, rational=True), diag=2.0).to_scipy()
    walks, certified = T.dev.prof_get(5)[1], T.dev.prof_get(3)[1]
    b = spline.assembleVector(T.F.NodalLoadForm(load, gen, rational=True)).get_local()
    Kr, br, zd = _host_extracted(gen, kvs, p, load, diag=2.0)
    assert np.array_equal(K.indptr, Kr.indptr) and np.array_equal(K.indices, Kr.indices)
    assert abs(K - Kr).max() <= 1e-12 * abs(Kr).max()
    assert np.max(np.abs(b - br)) <= 1e-12 * np.max(np.abs(br))
    assert walks > 0 and certified > 0


def test_transient_problem_projects_in_the_rational_space(T):
    from tigar_amd import timeIntegration as TI
    gen, spline, kv, Pf = _annulus_spline(T, 4, True)
    F = T.F
    x0 = lambda x: R.annulus_exact(x)
    forms = dict(stiffness=F.LaplaceForm(geometry=gen, rational=True), mass=F.MassForm(geometry=gen, rational=True))
    prob = TI.LinearTransientProblem(spline, order=1, RHO_INF=0.5, DELTA_T=0.01, x0=x0, rational=True, **forms)
    want = spline.projectDofs(x0, applyBCs=True, rational=True).get_local()
    assert np.array_equal(prob.x.get_local().view(np.int64), want.view(np.int64))
    other = TI.LinearTransientProblem(spline, order=1, RHO_INF=0.5, DELTA_T=0.01, x0=x0, **forms)
    assert np.max(np.abs(other.x.get_local() - want)) > 1e-4 * np.max(np.abs(want))
