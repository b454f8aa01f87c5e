"""GPU: the boundary kernels (csrc/tg_boundary.hip) against the longdouble reference of tests/boundary_reference.py, exact
identities, and what is built on them: FacePoints, BoundaryLoadForm, BoundaryMassForm, NitscheForm, Sum,
ExtractedSpline.boundaryPoints / evaluateAtBoundary / integrateBoundary / boundaryFlux.

Normwise bounds: max |error| / max |reference| of every output stays below 4 x the largest ratio observed on the MI355X
against the longdouble reference over all cases, faces and variants of this file (``MEASURED``, in units of eps; the margin
of the postproc and rational tests, it covers the change of summation order between builds).  Every test prints its
figures before it asserts.
"""
import numpy as np
import pytest

import postproc_reference as R
import boundary_reference as BR

pytestmark = pytest.mark.gpu

EPS = BR.EPS
LD = BR.LD
# largest normwise errors observed on the MI355X over the cases, faces and variants of this file, in eps
MEASURED = {
    "x": 2.07, "wsurf": 10.85, "normal": 23.52, "h_normal": 28.68,         # tg_face_points
    "values": 4.55, "gradient": 23.72, "d_n": 24.08,                       # tg_face_eval (random nodal values)
    "load": 20.52, "matrix": 38.55, "matrix_add": 3.61,                    # tg_face_load, tg_face_matrix, tg_face_matrix_add
    "normal_exact": 12.25, "area": 3.33,                                   # against closed forms
    "closed": 0.45, "moment": 1.27,                                        # sum wsurf n, sum wsurf x . n, relative to sum wsurf
}
MARGIN = 4.0


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


def _hold(what, figures):
    """figures: the normwise ratios (in eps) of one quantity over the faces and variants of a test"""
    worst = max(figures)
    bound = MARGIN * max(MEASURED[what], 1.0)         # (a figure below one rounding is luck of the values: no bound below 4 eps)
    print("normwise %-12s %.2f eps (bound %.2f)" % (what, worst, bound))
    assert worst <= bound, (what, worst)


def _nw(got, ref, scale=None):
    ref = np.asarray(ref, dtype=LD)
    scale = np.max(np.abs(ref)) if scale is None else scale
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref)) / scale) / EPS


def _smooth_patch(nels, p, seed, nsd=None):
    """non-uniform element vertices and a smooth non-affine rational map given on the Q_p nodes"""
    d = len(nels)
    rng = np.random.default_rng(seed)
    uks = []
    for k in range(d):
        steps = rng.uniform(0.5, 1.5, nels[k])
        uks.append(np.concatenate([[0.0], np.cumsum(steps) / np.sum(steps) * (1.0 + 0.5 * k)]))
    X = R.lagrange_nodes(uks, p)
    wgt = 1.0 + 0.2 * X[0] * X[-1]
    coords = [X[i] + 0.1 * X[(i + 1) % d] ** 2 for i in range(d)]
    if nsd is not None and nsd > d:
        coords.append(X[0] ** 2 + X[-1])
    return uks, [c * wgt for c in coords] + [wgt]


def _lifted_annulus():
    """the quarter annulus as a rational surface in space: z = x y"""
    uks, cp = R.annulus_patch(4)
    return uks, [cp[0], cp[1], cp[0] * cp[1] / cp[2], cp[2]]


def _cylinder_shell():
    from geom_util import quarter_cylinder_shell
    kvs, C = quarter_cylinder_shell(2, 3)
    uks, _, cp = BR.patch_from_net(2, kvs, C)
    return uks, cp


# name -> (p, nq, vertices, control functions).  Every face of every case is run: both sides, nel = 1 normally and
# tangentially, odd and even tangential counts (colours and the tail colour), more face elements than a workgroup takes
# with a partial last group, nq = 1, nq != p + 1, the largest nq, nsd > d, B-spline and NURBS control meshes.
CASES = {
    "2d_p1_2x27_nq10_two_groups_largest_nq": lambda: (1, 10) + _smooth_patch((2, 27), 1, 1),
    "2d_p2_5x4": lambda: (2, None) + _smooth_patch((5, 4), 2, 2),
    "2d_p3_3x1_nq2_one_element_across": lambda: (3, 2) + _smooth_patch((3, 1), 3, 3),
    "2d_p4_1x3_nq1": lambda: (4, 1) + _smooth_patch((1, 3), 4, 4),
    "3d_p1_2x3x2_nq2": lambda: (1, 2) + _smooth_patch((2, 3, 2), 1, 5),
    "3d_p2_2x5x4_nq4_two_groups": lambda: (2, 4) + _smooth_patch((2, 5, 4), 2, 6),
    "3d_p3_2x3x1_nq3": lambda: (3, 3) + _smooth_patch((2, 3, 1), 3, 7),
    "3d_p4_1x2x1_nq5": lambda: (4, 5) + _smooth_patch((1, 2, 1), 4, 8),
    "3d_p2_1x2x2_nq10_largest_nq": lambda: (2, 10) + _smooth_patch((1, 2, 2), 2, 9),
    "surface_in_3d_p2_4x3": lambda: (2, None) + _smooth_patch((4, 3), 2, 10, nsd=3),
    "quarter_annulus_5": lambda: (2, None) + R.annulus_patch(5),
    "lifted_annulus_in_3d": lambda: (2, None) + _lifted_annulus(),
    "rational_volume_p2_2x3x2": lambda: (2, None) + R.volume_patch(2, (2, 3, 2)),
    "quarter_cylinder_shell_2x2x3": lambda: (2, None) + _cylinder_shell(),
}
_REF = {}


def _case(name):
    """(p, nq, vertices, control functions, a reference and inputs per face): computed once per case and shared"""
    if name not in _REF:
        p, nq, uks, cp = CASES[name]()
        faces = {}
        for k, s in BR.all_faces(len(uks)):
            ref = BR.FaceReference(uks, p, cp, k, s, nq)
            rng = np.random.default_rng(100 * k + s + len(name))
            faces[(k, s)] = dict(ref=ref, u=rng.standard_normal(ref.nnodes), a=rng.standard_normal(ref.npts),
                                 b=rng.standard_normal(ref.npts), c=rng.standard_normal(ref.npts))
        _REF[name] = dict(p=p, nq=nq, uks=uks, cp=cp, faces=faces)
    return _REF[name]


def _dcp(T, c):
    return [T.dev.DeviceVector(data=v) for v in c["cp"]]


def _dv(T, v):
    return T.dev.DeviceVector(data=np.asarray(v, dtype=np.float64)) if v is not None else None


# ---- 1. kernels against the longdouble reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_face_points(T, name):
    c = _case(name)
    dcp = _dcp(T, c)
    fig = dict(x=[], wsurf=[], normal=[], h_normal=[])
    for (k, s), f in c["faces"].items():
        ref = f["ref"]
        x, w, nr, hn = T.dev.face_points(c["uks"], c["p"], dcp, k, s, c["nq"])
        assert w.size() == ref.npts == T.dev.face_count(c["uks"], k, ref.nq)
        fig["x"].append(_nw(x.get_local().reshape(ref.nsd, ref.npts).T, ref.x))
        fig["wsurf"].append(_nw(w.get_local(), ref.wsurf))
        fig["normal"].append(_nw(nr.get_local().reshape(ref.nsd, ref.npts).T, ref.normal))
        fig["h_normal"].append(_nw(hn.get_local(), ref.hn))
    for what, v in fig.items():
        _hold(what, v)


def test_face_points_outputs_may_be_null(T):
    import ctypes as C
    from tigar_amd import _lib
    c = _case("2d_p2_5x4")
    dcp = _dcp(T, c)
    ref = c["faces"][(1, 1)]["ref"]
    pt, keep = T.dev._patch(c["uks"], c["p"], dcp, ref.nq)
    w = T.dev.DeviceVector(ref.npts, zero=False)
    _lib.check(_lib.lib().tg_face_points(C.byref(pt), 1, 1, None, w._h, None, None), "tg_face_points")
    assert np.array_equal(w.get_local(), T.dev.face_points(c["uks"], c["p"], dcp, 1, 1, ref.nq)[1].get_local())


@pytest.mark.parametrize("name", sorted(CASES))
def test_face_eval(T, name):
    c = _case(name)
    dcp = _dcp(T, c)
    fig = dict(values=[], gradient=[], d_n=[])
    for (k, s), f in c["faces"].items():
        ref = f["ref"]
        for rat in (False, True):
            val, g, dn = T.dev.face_eval(c["uks"], c["p"], dcp, k, s, _dv(T, f["u"]), True, True, c["nq"], rat)
            rv, rg, rd = ref.eval(f["u"], rat)
            fig["values"].append(_nw(val.get_local(), rv))
            fig["gradient"].append(_nw(g.get_local().reshape(ref.nsd, ref.npts).T, rg))
            fig["d_n"].append(_nw(dn.get_local(), rd))
        only = T.dev.face_eval(c["uks"], c["p"], dcp, k, s, _dv(T, f["u"]), nq=c["nq"])
        assert only[1] is None and only[2] is None and np.array_equal(only[0].get_local(), T.dev.face_eval(
            c["uks"], c["p"], dcp, k, s, _dv(T, f["u"]), True, True, c["nq"])[0].get_local())
    for what, v in fig.items():
        _hold(what, v)


@pytest.mark.parametrize("name", sorted(CASES))
def test_face_load(T, name):
    """f_q only, fn_q only, both; the call adds into its output"""
    c = _case(name)
    dcp = _dcp(T, c)
    fig = []
    for (k, s), f in c["faces"].items():
        ref = f["ref"]
        for rat in (False, True):
            for a, b in ((f["a"], None), (None, f["b"]), (f["a"], f["b"])):
                out = T.dev.DeviceVector(ref.nnodes)
                T.dev.face_load(c["uks"], c["p"], dcp, k, s, _dv(T, a), _dv(T, b), out, c["nq"], rat)
                fig.append(_nw(out.get_local(), ref.load(a, b, rat)))
        start = np.random.default_rng(5).standard_normal(ref.nnodes)
        out = _dv(T, start)
        T.dev.face_load(c["uks"], c["p"], dcp, k, s, _dv(T, f["a"]), None, out, c["nq"])
        exp = start.astype(LD) + ref.load(f["a"])
        assert _nw(out.get_local(), exp) <= MARGIN * MEASURED["load"] + 1.0
    _hold("load", fig)


@pytest.mark.parametrize("name", sorted(CASES))
def test_face_matrix(T, name):
    """each coefficient array alone and all three; only the rows of the boundary layer are non-empty, and the pattern is
    the element coupling restricted to that layer"""
    c = _case(name)
    dcp = _dcp(T, c)
    fig = []
    for (k, s), f in c["faces"].items():
        ref = f["ref"]
        for rat in (False, True):
            for a, b, cc in ((f["a"], None, None), (None, f["b"], None), (None, None, f["c"]), (f["a"], f["b"], f["c"])):
                A = T.dev.face_matrix(c["uks"], c["p"], dcp, k, s, _dv(T, a), _dv(T, b), _dv(T, cc), c["nq"], rat).to_scipy()
                fig.append(_nw(A.toarray(), ref.matrix(a, b, cc, rat)))
        layer = np.zeros(ref.nnodes, dtype=bool)
        pattern = np.zeros((ref.nnodes, ref.nnodes), dtype=bool)
        for E in ref.elements:
            layer[E["g"]] = True
            pattern[np.ix_(E["g"], E["g"])] = True
        assert A.shape == (ref.nnodes, ref.nnodes) and np.array_equal(np.diff(A.indptr) > 0, layer)
        stored = np.zeros_like(pattern)
        stored[np.repeat(np.arange(ref.nnodes), np.diff(A.indptr)), A.indices] = True
        assert np.array_equal(stored, pattern) and A.has_sorted_indices
    _hold("matrix", fig)


ADD_CASES = ["2d_p2_5x4", "2d_p3_3x1_nq2_one_element_across", "3d_p1_2x3x2_nq2", "quarter_annulus_5", "rational_volume_p2_2x3x2"]


@pytest.mark.parametrize("name", ADD_CASES)
def test_face_matrix_add(T, name):
    """every face added in place, with a factor, into the mapped Laplace matrix: A + scale * face, on A's pattern"""
    c = _case(name)
    dcp = _dcp(T, c)
    scale = -0.75
    for rat in (False, True):
        A = T.dev.assemble_mapped_matrix(c["uks"], c["p"], dcp, "laplace", rational=rat)
        S0 = A.to_scipy()
        exp, mag = S0.toarray().astype(LD), np.abs(S0.toarray()).astype(LD)
        for (k, s), f in c["faces"].items():
            assert T.dev.face_matrix_add(A, c["uks"], c["p"], dcp, k, s, _dv(T, f["a"]), _dv(T, f["b"]), _dv(T, f["c"]),
                                         scale=scale, nq=c["nq"], rational=rat)
            exp += scale * f["ref"].matrix(f["a"], f["b"], f["c"], rat)
        S1 = A.to_scipy()
        assert np.array_equal(S1.indptr, S0.indptr) and np.array_equal(S1.indices, S0.indices)
        _hold("matrix_add", [_nw(S1.toarray(), exp)])


def test_face_matrix_add_refuses_a_pattern_without_the_entries(T):
    """the error return, with the matrix unchanged: a diagonal matrix, and the matrix of the opposite face"""
    import scipy.sparse as sp
    c = _case("2d_p2_5x4")
    dcp = _dcp(T, c)
    f = c["faces"][(0, 0)]
    n = f["ref"].nnodes
    D = T.dev.DeviceCSR.from_scipy(sp.diags(np.arange(1.0, n + 1.0)).tocsr())
    other = T.dev.face_matrix(c["uks"], c["p"], dcp, 0, 1, _dv(T, c["faces"][(0, 1)]["a"]), None, None, c["nq"])
    for M in (D, other):
        before = M.to_scipy()
        assert T.dev.face_matrix_add(M, c["uks"], c["p"], dcp, 0, 0, _dv(T, f["a"]), _dv(T, f["b"]), None, nq=c["nq"]) is False
        after = M.to_scipy()
        assert np.array_equal(before.data, after.data) and np.array_equal(before.indices, after.indices)
    with pytest.raises(T.dev.TigarHipError, match="lacks entries"):
        import ctypes as C
        from tigar_amd import _lib
        pt, keep = T.dev._patch(c["uks"], c["p"], dcp, f["ref"].nq)
        aq = _dv(T, f["a"])
        _lib.check(_lib.lib().tg_face_matrix_add(C.byref(pt), 0, 0, aq._h, None, None, 1.0, D._h), "tg_face_matrix_add")
    # the matrix of the face itself holds them
    own = T.dev.face_matrix(c["uks"], c["p"], dcp, 0, 0, _dv(T, f["a"]), None, None, c["nq"])
    assert T.dev.face_matrix_add(own, c["uks"], c["p"], dcp, 0, 0, _dv(T, f["a"]), None, None, nq=c["nq"]) is True


# ---- 2. exact geometry ----------------------------------------------------------------------------------------------------------
def test_exact_normals_on_the_annulus(T):
    c = _case("quarter_annulus_5")
    dcp = _dcp(T, c)
    fig = []
    for k, s in BR.all_faces(2):
        x, w, nr, hn = T.dev.face_points(c["uks"], 2, dcp, k, s)
        x, nr = x.get_local().reshape(2, -1).T, nr.get_local().reshape(2, -1).T
        exact = (2 * s - 1) * x / np.hypot(x[:, 0], x[:, 1])[:, None] if k == 0 else \
            np.tile([0.0, -1.0] if s == 0 else [-1.0, 0.0], (x.shape[0], 1))
        fig.append(_nw(nr, exact, 1.0))
    _hold("normal_exact", fig)


def test_exact_faces_of_the_box(T):
    """n = +- e_k and sum wsurf = the face area on the box [0, 1] x [0, 1.5] x [0, 2], and on the rectangle"""
    fign, figa = [], []
    for nels in ((3, 2), (2, 3, 2)):
        d = len(nels)
        uks = [np.linspace(0.0, 1.0 + 0.5 * k, n + 1) for k, n in enumerate(nels)]
        X = R.lagrange_nodes(uks, 2)
        dcp = [T.dev.DeviceVector(data=v) for v in X + [np.ones_like(X[0])]]
        for k, s in BR.all_faces(d):
            x, w, nr, hn = T.dev.face_points(uks, 2, dcp, k, s)
            e = np.zeros(d)
            e[k] = 2 * s - 1
            area = float(np.prod([1.0 + 0.5 * j for j in range(d) if j != k]))
            fign.append(_nw(nr.get_local().reshape(d, -1).T, np.tile(e, (w.size(), 1)), 1.0))
            figa.append(abs(float(np.sum(w.get_local().astype(LD))) - area) / area / EPS)
    _hold("normal_exact", fign)
    _hold("area", figa)


# ---- 3. closed surface and divergence theorem --------------------------------------------------------------------------------
POLY = {"2d": lambda: BR.poly_patch_2d((3, 2)), "3d": lambda: BR.poly_patch_3d((2, 1, 3))}


@pytest.mark.parametrize("which", sorted(POLY))
def test_closed_surface_and_divergence_theorem(T, which):
    """Polynomial maps with unit weights, p = 2, nq = 3: per face element n wsurf is a polynomial of degree <= 1 (2-D) /
    (1, 1) (3-D, trilinear map) and x . n wsurf of degree <= 3 / (2, 2); the volume weight det DF has degree <= (3, 3) /
    (2, 2, 2): a 3-point rule integrates degree 5 exactly.  So sum wsurf n = 0 and sum wsurf x . n = d sum wdet."""
    kvs, C = POLY[which]()
    d = len(kvs)
    uks, _, cp = BR.patch_from_net(2, kvs, C)
    dcp = [T.dev.DeviceVector(data=v) for v in cp]
    closed, moment, area = np.zeros(d, dtype=LD), LD(0), LD(0)
    for k, s in BR.all_faces(d):
        x, w, nr, hn = T.dev.face_points(uks, 2, dcp, k, s, 3)
        x, nr, w = x.get_local().reshape(d, -1).T.astype(LD), nr.get_local().reshape(d, -1).T.astype(LD), w.get_local().astype(LD)
        closed += w @ nr
        moment += np.sum(w * np.sum(x * nr, axis=1))
        area += w.sum()
    vol = np.sum(T.dev.quad_points(uks, 2, dcp, 3)[1].get_local().astype(LD))
    _hold("closed", [float(np.max(np.abs(closed)) / area) / EPS])
    _hold("moment", [float(abs(moment - d * vol) / area) / EPS])


# ---- 4. same bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d_p2_5x4", "3d_p2_2x5x4_nq4_two_groups", "rational_volume_p2_2x3x2"])
def test_two_runs_give_the_same_bits(T, name):
    c = _case(name)
    dcp = _dcp(T, c)

    def run(k, s, f, rat):
        n = f["ref"].nnodes
        out = [v.get_local() for v in T.dev.face_points(c["uks"], c["p"], dcp, k, s, c["nq"])]
        out += [v.get_local() for v in T.dev.face_eval(c["uks"], c["p"], dcp, k, s, _dv(T, f["u"]), True, True, c["nq"], rat)]
        out.append(T.dev.face_load(c["uks"], c["p"], dcp, k, s, _dv(T, f["a"]), _dv(T, f["b"]), T.dev.DeviceVector(n), c["nq"],
                                   rat).get_local())
        out.append(T.dev.face_matrix(c["uks"], c["p"], dcp, k, s, _dv(T, f["a"]), _dv(T, f["b"]), _dv(T, f["c"]), c["nq"],
                                     rat).to_scipy().data)
        A = T.dev.assemble_mapped_matrix(c["uks"], c["p"], dcp, "mass")
        assert T.dev.face_matrix_add(A, c["uks"], c["p"], dcp, k, s, _dv(T, f["a"]), _dv(T, f["b"]), _dv(T, f["c"]), 0.5, c["nq"], rat)
        out.append(A.to_scipy().data)
        return out
    for (k, s), f in c["faces"].items():
        for rat in (False, True):
            for one, two in zip(run(k, s, f, rat), run(k, s, f, rat)):
                assert np.array_equal(one, two)


# ---- through the API -----------------------------------------------------------------------------------------------------------
def _poly_spline(T, which, nfields=1):
    kvs, C = POLY[which]()
    gen = T.t.EqualOrderSpline(nfields, T.N.NURBSControlMesh([2] * len(kvs), kvs, C))
    return gen, T.t.ExtractedSpline(gen, 4), kvs, C


def _annulus_spline(T, nel, zero_faces, nfields=1):
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    gen = T.t.EqualOrderSpline(nfields, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf))
    sp0 = gen.getScalarSpline(0)
    for direction, side in zero_faces:
        gen.addZeroDofs(0, sp0.getSideDofs(direction, side))
    return gen, T.t.ExtractedSpline(gen, 4)


def _nodes(gen):
    cp = [f.vector().get_local() for f in gen.cpFuncs]
    return np.stack([cp[i] / cp[-1] for i in range(len(cp) - 1)], axis=1), cp


def test_sum_adds_face_terms_in_place(T):
    """Sum(volume, face terms): the face terms go into the volume matrix in place, and the result is the one through
    DeviceCSR.add to the rounding of one addition per entry and term"""
    F = T.F
    gen, spline, kvs, C = _poly_spline(T, "2d")
    lap = F.LaplaceForm(geometry=gen)
    mass = F.BoundaryMassForm(lambda x: 1.0 + x[:, 0], gen, [(0, 0), (1, 1)])
    nit = F.NitscheForm(gen, [(0, 1)], 10.0)
    total = F.Sum(lap, (2.0, mass), nit)
    assert total.symmetric
    K = total.assemble_matrix(gen.V)
    assert total.in_place == 2
    parts = [lap.assemble_matrix(gen.V), mass.assemble_matrix(gen.V), nit.assemble_matrix(gen.V)]
    viaadd = parts[0].add(parts[1].combine(2.0, parts[1], 0.0)).add(parts[2])
    S, Sa = K.to_scipy(), viaadd.to_scipy()
    assert np.array_equal(S.indptr, parts[0].to_scipy().indptr)          # the pattern of the volume term
    mag = abs(parts[0].to_scipy()).toarray() + 2.0 * abs(parts[1].to_scipy()).toarray() + abs(parts[2].to_scipy()).toarray()
    assert np.all(np.abs(S.toarray() - Sa.toarray()) <= 3.0 * EPS * mag)
    assert np.array_equal(S.data, total.assemble_matrix(gen.V).to_scipy().data)
    # a first term whose pattern lacks the entries: the union pattern through DeviceCSR.add
    both = F.Sum(mass, nit)
    Kb = both.assemble_matrix(gen.V).to_scipy()
    assert both.in_place == 0
    assert np.max(np.abs(Kb.toarray() - parts[1].to_scipy().toarray() - parts[2].to_scipy().toarray())) <= 3.0 * EPS * np.max(mag)
    # vectors
    b = F.Sum(F.BoundaryLoadForm(1.0, gen, [(0, 0)]), (0.5, nit.load(2.0))).assemble_vector(gen.V).get_local()
    exp = F.BoundaryLoadForm(1.0, gen, [(0, 0)]).assemble_vector(gen.V).get_local() + 0.5 * nit.load(2.0).assemble_vector(gen.V).get_local()
    assert np.max(np.abs(b - exp)) <= 4.0 * EPS * np.max(np.abs(exp))


# ---- 5. patch test ---------------------------------------------------------------------------------------------------------------
NITSCHE_FACES = {"2d": [(0, 0), (1, 1)], "3d": [(0, 1), (2, 0)]}


@pytest.mark.parametrize("which", sorted(POLY))
@pytest.mark.parametrize("kind", ["robin", "nitsche"])
def test_patch_test(T, which, kind):
    """Laplace + Robin on every face (data grad l . n + alpha l), and Laplace + symmetric Nitsche terms on two faces with
    Neumann data on the rest, for a linear l on a polynomial map without zero dofs, through solveLinearVariationalProblem
    with the default direct solver: the solution is l at the FE nodes, to 4 x the error of the host flow
    (boundary_reference.patch_test_host: the same matrices in longdouble, solved in float64).  On the MI355X, in eps of
    max |l| (host flow in brackets): 2-D Robin 2.11 (3.86), Nitsche 2.81 (4.21); 3-D Robin 10.49 (5.90), Nitsche 6.56 (9.84)."""
    F = T.F
    gen, spline, kvs, C = _poly_spline(T, which)
    d = len(kvs)
    l, gl = BR.LIN_2D if d == 2 else BR.LIN_3D
    alpha = 2.0
    flux = lambda x, n: n @ gl
    if kind == "robin":
        lhs = F.Sum(F.LaplaceForm(geometry=gen), F.BoundaryMassForm(alpha, gen))
        rhs = F.BoundaryLoadForm(lambda x, n: n @ gl + alpha * l(x), gen)
        host = BR.patch_test_host(kvs, C, (l, gl), alpha)
    else:
        nf = NITSCHE_FACES[which]
        nit = F.NitscheForm(gen, nf, 10.0)
        lhs = F.Sum(F.LaplaceForm(geometry=gen), nit)
        rhs = F.Sum(nit.load(l), F.BoundaryLoadForm(flux, gen, [f for f in BR.all_faces(d) if f not in nf]))
        host = BR.patch_test_host(kvs, C, (l, gl), nitsche_faces=nf, penalty=10.0)
    u = T.t.Function(spline.V)
    spline.solveLinearVariationalProblem(F.Equation(lhs, rhs), u)
    xn, _ = _nodes(gen)
    err = float(np.max(np.abs(u.vector().get_local() - l(xn))) / np.max(np.abs(l(xn))))
    print("patch test %s %s: error %.3e = %.2f eps, host flow %.3e = %.2f eps" % (which, kind, err, err / EPS, host, host / EPS))
    assert err <= 4.0 * host


# ---- 6. convergence on the quarter annulus -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nitsche", [False, True])
def test_annulus_with_neumann_and_robin_data(T, nitsche):
    """-lap u = f on the quarter annulus in the rational space, p = 2, nel = 4, 8, 16: Neumann data on the inner arc, a
    Robin condition on the outer one, u = 0 on the straight edges through zero dofs -- or, ``nitsche``, on the edge
    theta = 0 through the symmetric NitscheForm.  errorNorm equals the host flow of boundary_reference (same quadrature,
    scipy's LU).  The two flows differ by the rounding of the direct solves: a relative error of at most 64 eps kappa(K) of
    the solution (kappa: the 2-norm condition number of the system, computed by the host flow), which changes an error
    norm by at most that multiple of the norm of the solution; plus 1e-12 of the error norm for the rounding of the sums.
    boundaryFlux over the whole boundary equals - int f dx to the discretisation error the host flow shows."""
    F = T.F
    errs = []
    for nel in (4, 8, 16):
        gen, spline = _annulus_spline(T, nel, [(1, 1)] if nitsche else [(1, 0), (1, 1)])
        lhs = [F.LaplaceForm(geometry=gen, rational=True), (BR.ROBIN_ALPHA, F.BoundaryMassForm(1.0, gen, [(0, 1)], rational=True))]
        rhs = [F.QuadratureLoadForm(R.annulus_rhs, gen, rational=True),
               F.BoundaryLoadForm([BR.neumann_data, BR.robin_data], gen, [(0, 0), (0, 1)], rational=True)]
        if nitsche:
            nit = F.NitscheForm(gen, [(1, 0)], 10.0, rational=True)
            lhs.append(nit)
            rhs.append(nit.load(BR.robin_exact))
        u = T.t.Function(spline.V)
        spline.solveLinearVariationalProblem(F.Equation(F.Sum(*lhs), F.Sum(*rhs)), u)
        l2 = spline.errorNorm(u, BR.robin_exact, "L2", rational=True)
        h10 = spline.errorNorm(u, BR.robin_exact, "H10", exact_grad=BR.robin_exact_grad, rational=True)
        flux = spline.boundaryFlux(u, rational=True)
        H = BR.solve_annulus_boundary(nel, nitsche)
        rel = 64.0 * EPS * H["kappa"]
        tol_l2, tol_h10 = rel * H["unorm_l2"] + 1e-12 * H["l2"], rel * H["unorm_h10"] + 1e-12 * H["h10"]
        print("annulus nitsche=%s nel %2d: L2 %.6e (host %.6e, tolerance %.1e)  H10 %.6e (host %.6e, tolerance %.1e)  "
              "flux %.9f (host %.9f, -int f %.9f)" % (nitsche, nel, l2, H["l2"], tol_l2, h10, H["h10"], tol_h10, flux, H["flux"],
                                                     -H["intf"]))
        assert abs(l2 - H["l2"]) <= tol_l2 and abs(h10 - H["h10"]) <= tol_h10
        assert abs(flux + H["intf"]) <= abs(H["flux"] + H["intf"]) + rel * abs(H["intf"]) * 10.0
        assert abs(spline.integrate(R.annulus_rhs) - H["intf"]) <= 64 * EPS * abs(H["intf"])
        errs.append((l2, h10))
    for a, b in zip(errs[:-1], errs[1:]):
        assert a[0] / b[0] >= 7.0 and a[1] / b[1] >= 3.5


# ---- 7. traction -----------------------------------------------------------------------------------------------------------------
def test_pressure_on_the_inner_arc_of_the_annulus(T):
    """ElasticityForm's space on the annulus under BoundaryLoadForm.pressure on the inner arc: the assembled load is the
    reference's load of -p n_c per component"""
    F = T.F
    gen, spline = _annulus_spline(T, 5, [], nfields=2)
    p0 = 3.0
    F.ElasticityForm(1.0, 1.0, geometry=gen, rational=True)._grid(gen.V)          # the space that form requires
    b = F.BoundaryLoadForm.pressure(p0, gen, [(0, 0)], rational=True).assemble_vector(gen.V).get_local()
    c = _case("quarter_annulus_5")
    ref = c["faces"][(0, 0)]["ref"]
    assert b.size == 2 * ref.nnodes
    fig = [_nw(b[i * ref.nnodes:(i + 1) * ref.nnodes], ref.load(-p0 * ref.normal[:, i], rational=True)) for i in range(2)]
    _hold("load", fig)
    # a pressure given as a function of the points, on two faces
    pf = lambda x: 1.0 + x[:, 0]
    b2 = F.BoundaryLoadForm.pressure(pf, gen, [(0, 0), (1, 1)], rational=True).assemble_vector(gen.V).get_local()
    exp = np.zeros((2, ref.nnodes), dtype=LD)
    for f in ((0, 0), (1, 1)):
        r = c["faces"][f]["ref"]
        for i in range(2):
            exp[i] += r.load(-pf(np.asarray(r.x, dtype=np.float64)) * r.normal[:, i], rational=True)
    _hold("load", [_nw(b2[i * ref.nnodes:(i + 1) * ref.nnodes], exp[i]) for i in range(2)])


@pytest.mark.parametrize("which", sorted(POLY))
def test_constant_pressure_on_a_closed_boundary_has_no_resultant(T, which):
    """the sum of the load over all nodes per component is -p sum wsurf n_c = 0 (the functions sum to one): check 3 through
    the load ending"""
    gen, spline, kvs, C = _poly_spline(T, which, nfields=len(POLY[which]()[0]))
    d = len(kvs)
    b = T.F.BoundaryLoadForm.pressure(1.0, gen).assemble_vector(gen.V).get_local().reshape(d, -1).astype(LD)
    area = sum(float(np.sum(T.F.face_points(gen, gen.V, k, s).weights.get_local())) for k, s in BR.all_faces(d))
    _hold("closed", [float(np.max(np.abs(b.sum(axis=1))) / area) / EPS])


# ---- points and integrals through the spline ------------------------------------------------------------------------------------
def test_boundary_points_and_integrals_through_the_spline(T):
    gen, spline = _annulus_spline(T, 5, [])
    c = _case("quarter_annulus_5")
    pts = spline.boundaryPoints(0, 1)
    ref = c["faces"][(0, 1)]["ref"]
    assert pts is spline.boundaryPoints(0, 1) and pts is not spline.boundaryPoints(0, 1, nq=4) and pts.npts == ref.npts
    assert pts.x.shape == (ref.npts, 2) and pts.n.shape == (ref.npts, 2) and pts.nq == 3
    assert pts.x_device.size() == pts.normals.size() == 2 * ref.npts and pts.h_normal.size() == ref.npts
    _hold("x", [_nw(pts.x, ref.x)])
    _hold("wsurf", [_nw(pts.weights.get_local(), ref.wsurf)])
    assert np.array_equal(pts.values(2.0).get_local(), np.full(ref.npts, 2.0))
    assert pts.vector_values(lambda x: 2.0 * x).size() == 2 * ref.npts
    # the length of the boundary, an integrand of (x, n), point values per face
    length = spline.integrateBoundary(1.0)
    assert abs(length - (1.5 * np.pi + 2.0)) <= 1e-7
    got = spline.integrateBoundary(lambda x, n: np.sum(x * n, axis=1))          # 2 |Omega| = 2 (pi 4 / 4 - pi / 4)
    assert abs(got - 1.5 * np.pi) <= 1e-7
    vals = [np.ones(spline.boundaryPoints(k, s).npts) for k, s in BR.all_faces(2)]
    assert abs(spline.integrateBoundary(vals) - length) <= 8 * EPS * length
    assert abs(spline.integrateBoundary(1.0, faces=(0, 0)) - np.pi / 2) <= 1e-8
    # a linear function of the rational space: values, gradient and d_n at the points
    xn, cp = _nodes(gen)
    lin = lambda x: 1.0 + 2.0 * x[:, 0] - x[:, 1]
    u = T.t.Function(spline.V)
    u.vector()[:] = cp[-1] * lin(xn)
    val, comps, dn = spline.evaluateAtBoundary(u, 0, 1, grad=True, normal_derivative=True, rational=True)
    assert _nw(val.get_local(), lin(pts.x)) <= MARGIN * MEASURED["gradient"]          # (the largest figure of the fields)
    assert max(np.max(np.abs(comps[0].get_local() - 2.0)), np.max(np.abs(comps[1].get_local() + 1.0))) <= 1e-12
    assert np.max(np.abs(dn.get_local() - pts.n @ np.array([2.0, -1.0]))) <= 1e-12
    assert abs(spline.integrateBoundary(u, faces=[(0, 1)]) - pts.weights.inner(pts.values(u))) == 0.0
    assert abs(spline.boundaryFlux(u, rational=True)) <= 1e-7                  # a harmonic function (quadrature error of the arcs)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(T, monkeypatch):
    t, F, B = T.t, T.F, T.B
    gen, spline = _annulus_spline(T, 3, [])
    V = gen.V
    n = V.dim()
    one = lambda x: np.ones(x.shape[0])
    load, mass, nit = F.BoundaryLoadForm(1.0, gen), F.BoundaryMassForm(1.0, gen), F.NitscheForm(gen, [(0, 0)], 10.0)
    # row blocks: several ranks, streamed operands
    for call in (lambda: load.assemble_vector(V, 0, n // 2), lambda: mass.assemble_matrix(V, 0, n // 2),
                 lambda: nit.assemble_matrix(V, n // 2, n), lambda: nit.load(1.0).assemble_vector(V, 0, n // 2),
                 lambda: F.Sum(F.LaplaceForm(geometry=gen), mass).assemble_matrix(V, 0, n // 2)):
        with pytest.raises(NotImplementedError):
            call()
    with monkeypatch.context() as m:
        m.setattr(spline, "_distributed", lambda: True)
        with pytest.raises(NotImplementedError, match="ranks"):
            spline.boundaryPoints(0, 0)
    with monkeypatch.context() as m:
        m.setattr(spline, "_caller_ordered", lambda: True)
        for call in (lambda: spline.boundaryPoints(0, 0), lambda: spline.integrateBoundary(1.0),
                     lambda: spline.boundaryFlux(t.Function(spline.V)), lambda: spline.evaluateAtBoundary(t.Function(spline.V), 0, 0)):
            with pytest.raises(NotImplementedError, match="feOrder"):
                call()
    # faces
    for bad in ((2, 0), (0, 2), (-1, 1)):
        with pytest.raises(ValueError):
            spline.boundaryPoints(*bad)
        with pytest.raises(ValueError):
            F.BoundaryLoadForm(1.0, gen, [bad]).assemble_vector(V)
        with pytest.raises(ValueError):
            F.BoundaryMassForm(1.0, gen, [bad]).assemble_matrix(V)
    kvp = [B.uniformKnots(2, 0.0, 1.0, 4), B.uniformKnots(2, 0.0, 1.0, 4, periodic=True)]
    per = t.ExtractedSpline(t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2, 2], kvp)), 4)
    with pytest.raises(ValueError, match="periodic"):
        per.boundaryPoints(1, 0)
    with pytest.raises(ValueError, match="periodic"):
        per.integrateBoundary(1.0, faces=[(0, 0), (1, 1)])
    assert per.integrateBoundary(1.0) == per.integrateBoundary(1.0, faces=[(0, 0), (0, 1)])      # faces=None: those that are a boundary
    # point counts and shapes
    npts = spline.boundaryPoints(0, 0).npts
    with pytest.raises(ValueError):
        spline.integrateBoundary(np.ones(npts + 1), faces=(0, 0))
    with pytest.raises(ValueError):
        spline.integrateBoundary([np.ones(npts)])                               # one entry for four faces
    with pytest.raises(ValueError):
        F.BoundaryLoadForm(lambda x: np.ones((x.shape[0], 2)), gen, [(0, 0)]).assemble_vector(V)
    with pytest.raises(ValueError):
        F.BoundaryMassForm(T.dev.DeviceVector(npts + 1), gen, [(0, 0)]).assemble_matrix(V)
    with pytest.raises(ValueError):
        spline.evaluateAtBoundary(T.dev.DeviceVector(n + 1), 0, 0)
    pts = spline.boundaryPoints(0, 0)
    with pytest.raises(T.dev.TigarHipError):
        T.dev.face_load(pts.verts, 2, pts.cp, 0, 0, T.dev.DeviceVector(npts + 1), None, T.dev.DeviceVector(n))
    # nq
    most = T.dev.assemble_limits()[1]
    for bad in (0, most + 1, 2.5):
        with pytest.raises(ValueError):
            spline.boundaryPoints(0, 0, nq=bad)
    with pytest.raises(ValueError):
        F.BoundaryLoadForm(1.0, gen, nq=most + 1).assemble_vector(V)
    # geometry=None
    for make in (lambda: F.BoundaryLoadForm(1.0, None), lambda: F.BoundaryMassForm(1.0, None), lambda: F.NitscheForm(None, None, 1.0)):
        with pytest.raises(ValueError, match="geometry"):
            make()
    # spaces
    kv2 = [B.uniformKnots(2, 0.0, 1.0, 3)] * 2
    cm = B.ExplicitBSplineControlMesh([2, 2], kv2)
    two = t.ExtractedSpline(t.EqualOrderSpline(2, cm), 4)
    with pytest.raises(NotImplementedError, match="nFields"):
        two.boundaryPoints(0, 0)
    lst = t.ExtractedSpline(t.FieldListSpline(cm, [B.BSpline([2, 2], kv2)]), 4)
    with pytest.raises(NotImplementedError, match="FieldListSpline"):
        lst.boundaryPoints(0, 0)
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
            sp_.boundaryPoints(0, 0)
        with pytest.raises(NotImplementedError):
            sp_.integrateBoundary(1.0)
        with pytest.raises(NotImplementedError):
            F.BoundaryLoadForm(1.0, sp_).assemble_vector(sp_.V)
        with pytest.raises(NotImplementedError):
            F.BoundaryMassForm(1.0, sp_).assemble_matrix(sp_.V)
    kvd = [0, 0, 0, 0.5, 0.5, 0.5, 1, 1, 1]
    dg = t.ExtractedSpline(t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2, 2], [kvd, kvd])), 4)
    with pytest.raises(NotImplementedError):
        dg.boundaryPoints(0, 0)
    with pytest.raises(NotImplementedError):
        F.NitscheForm(dg, [(0, 0)], 1.0).assemble_matrix(dg.V)
