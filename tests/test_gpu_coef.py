"""GPU: volume forms with point coefficients -- ``tg_coef_transform`` / ``tg_flux_transform`` / ``tg_quad_load_flux`` (endings
of k_postproc), ``tg_assemble_coef_matrix`` (csrc/tg_coef.hip) and what is built on them: ``forms.CoefficientForm``, the
``flux`` of ``forms.QuadratureLoadForm``, ``forms.QuasilinearResidual`` under ``solveNonlinearVariationalProblem``.

Reference: tests/coef_reference.py, which forms phi (or phi / W_h) and its Cartesian gradient at every point and sums the
integrand as written -- no transformed tensor, no folded beta, no sum factorisation.  Coefficients are RANDOM per point, so
that any mis-numbering of the points shows; the diffusion tensor is not symmetric.

Tolerance: normwise, max |error| / max |reference| against the longdouble run.  The bound of a case is 8 x the error of the
float64 run of the same reference for that case (computed here, on the CPU: no figure of the code under test), and never
below 32 eps.  The factor allows for the transformed tensors and another order of the sums.

Measured on the MI355X (``-s`` prints every figure): the largest error / bound over the cases of this file is in the
README section "Point-coefficient forms".
"""
import numpy as np
import pytest

from oracle import tigar_oracle as O
import postproc_reference as R
import coef_reference as CR
import coef_problem as P

pytestmark = pytest.mark.gpu

EPS = R.EPS
FLOOR = 32 * EPS


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
def _weighted_nodes(nels, p, nsd=None):
    """non-uniform element vertices, a smooth non-affine map and a weight that varies by a third, given on the Q_p nodes;
    nsd > d: a curve or surface in space"""
    d = len(nels)
    rng = np.random.default_rng(7 * d + p)
    uks = []
    for k in range(d):
        steps = rng.uniform(0.6, 1.4, nels[k])
        uks.append(np.concatenate([[0.0], np.cumsum(steps) / np.sum(steps) * (1.0 + 0.5 * k)]))
    X = R.lagrange_nodes(uks, p)
    wgt = 1.0 + 0.3 * X[0] * X[-1] + 0.1 * X[0] ** 2
    coords = [X[i] + 0.1 * X[(i + 1) % d] ** 2 for i in range(d)]
    for extra in range(d, nsd if nsd is not None else d):
        coords.append(X[0] ** 2 + (extra - d + 1) * X[-1])
    return uks, [c * wgt for c in coords] + [wgt]


# name -> (p, nq, element vertices, control functions); ``full``: every term alone (else the sum of all four only)
CASES = {
    "1d_p1_4_nq1": lambda: (1, 1) + _weighted_nodes((4,), 1),
    "1d_p3_3": lambda: (3, None) + _weighted_nodes((3,), 3),
    "curve_in_3d_p2_3_nq4": lambda: (2, 4) + _weighted_nodes((3,), 2, nsd=3),
    "2d_p4_2x3_nq3": lambda: (4, 3) + _weighted_nodes((2, 3), 4),
    "annulus_3x2": lambda: (2, None) + _annulus_nodes((3, 2)),
    "annulus_3x2_nq4": lambda: (2, 4) + _annulus_nodes((3, 2)),
    "surface_in_3d_p2_2x2": lambda: (2, None) + _weighted_nodes((2, 2), 2, nsd=3),
    "surface_in_3d_p3_2x1_nq1": lambda: (3, 1) + _weighted_nodes((2, 1), 3, nsd=3),
    "volume_p1_2x2x2": lambda: (1, None) + R.volume_patch(1, (2, 2, 2)),
    "volume_p2_3x2x3_nq2": lambda: (2, 2) + R.volume_patch(2, (3, 2, 3)),
    "volume_p4_1x2x1": lambda: (4, None) + R.volume_patch(4, (1, 2, 1)),
    # nq = 10 in 3-D: the element's point data (16 x 1000 doubles) and the slots of the flux load need more LDS than a
    # launch gets without asking
    "volume_p1_1x1x1_nq10": lambda: (1, 10) + R.volume_patch(1, (1, 1, 1)),
    "volume_p4_1x1x1_nq10": lambda: (4, 10) + R.volume_patch(4, (1, 1, 1)),
}
ALL_TERMS_ONLY = {"volume_p4_1x2x1", "volume_p4_1x1x1_nq10", "volume_p2_3x2x3_nq2"}
# the sum-factorised route (3-D, nsd = 3, nq = p + 1, p = 2, 3): one element, even and odd counts with more than one colour,
# lines longer than a piece, and the default pieces (16 elements at p = 2, 8 groups of four at p = 3) with a seam
HOT = {
    "volume_p2_1x1x1": (2, (1, 1, 1)), "volume_p2_2x3x2": (2, (2, 3, 2)), "volume_p2_3x2x3": (2, (3, 2, 3)),
    "volume_p2_5x3x2": (2, (5, 3, 2)), "volume_p2_17x1x2": (2, (17, 1, 2)),
    "volume_p3_1x1x1": (3, (1, 1, 1)), "volume_p3_2x3x2": (3, (2, 3, 2)), "volume_p3_3x2x3": (3, (3, 2, 3)),
    "volume_p3_6x2x2": (3, (6, 2, 2)), "volume_p3_33x2x1": (3, (33, 2, 1)),
}
ROUTES = {"default": {}, "short_pieces": {"TIGAR_ASM_CHUNK": "2", "TIGAR_ASM_QUAD_CHUNK": "1"}, "legacy": {"TIGAR_ASM_LEGACY": "1"}}
EVERY_TERM = {"volume_p2_2x3x2", "volume_p3_2x3x2"}


def _annulus_nodes(nels):
    """the exact quarter annulus on nels[0] x nels[1] elements: its homogeneous coordinates are quadratics in the parameters,
    which the Q_2 nodal interpolation on any mesh reproduces"""
    uks1, cp1 = R.annulus_patch(1)
    uks = [np.linspace(0.0, 1.0, n + 1) for n in nels]
    X = R.lagrange_nodes(uks, 2)
    l = lambda t: np.stack([2.0 * (t - 0.5) * (t - 1.0), -4.0 * t * (t - 1.0), 2.0 * t * (t - 0.5)])
    L0, L1 = l(X[0]), l(X[1])
    return uks, [np.einsum("an,bn,ab->n", L0, L1, np.asarray(c).reshape(3, 3, order="F")) for c in cp1]


_REF = {}


def _case(name):
    """patch, random point coefficients and the two reference objects per space (longdouble, float64): built once"""
    if name not in _REF:
        if name in HOT:
            p, nq = HOT[name][0], None
            uks, cp = R.volume_patch(*HOT[name])
        else:
            p, nq, uks, cp = CASES[name]()
        cp = [np.asarray(c, dtype=np.float64) for c in cp]
        c = dict(p=p, nq=nq, uks=uks, cp=cp, refs={})
        for rat in (False, True):
            c["refs"][rat] = (CR.CoefReference(uks, p, cp, nq, rational=rat), CR.CoefReference(uks, p, cp, nq, rational=rat, dtype=np.float64))
        ref = c["refs"][False][0]
        rng = np.random.default_rng(sum(map(ord, name)))
        npts, nsd = ref.npts, ref.nsd
        c.update(npts=npts, nsd=nsd, nnodes=ref.nnodes,
                 a=rng.uniform(0.5, 1.5, npts), A=rng.standard_normal((npts, nsd, nsd)), b=rng.standard_normal((npts, nsd)),
                 c=rng.standard_normal((npts, nsd)), m=rng.standard_normal(npts), s=rng.standard_normal(npts),
                 Fv=rng.standard_normal((npts, nsd)))
        _REF[name] = c
    return _REF[name]


def _dcp(T, c):
    return [T.dev.DeviceVector(data=v) for v in c["cp"]]


def _dv(T, v):
    """host point data -> DeviceVector, component-major"""
    if v is None:
        return None
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 3:
        v = v.transpose(1, 2, 0)
    elif v.ndim == 2:
        v = v.T
    return T.dev.DeviceVector(data=np.ascontiguousarray(v).ravel())


def _terms(c, full):
    every = {"all": (c["A"], c["b"], c["c"], c["m"])}
    if full:
        every.update({"isotropic": (c["a"], None, None, None), "tensor": (c["A"], None, None, None),
                      "b": (None, c["b"], None, None), "c": (None, None, c["c"], None), "m": (None, None, None, c["m"])})
    return every


_WANT = {}


def _bound(ref, ref64, what, *args, key=None):
    """(reference values in longdouble, their scale, the bound 8 x float64 error, floor 32 eps); ``key``: computed once"""
    if key is not None and key in _WANT:
        return _WANT[key]
    out = _bound_of(ref, ref64, what, *args)
    if key is not None:
        _WANT[key] = out
    return out


def _bound_of(ref, ref64, what, *args):
    want, w64 = getattr(ref, what)(*args), getattr(ref64, what)(*args)
    if what == "matrix":
        assert np.array_equal(want[0], w64[0])
        keys, want, w64 = want[0], want[1], w64[1]
    else:
        keys = None
    scale = float(np.max(np.abs(want)))
    e64 = float(np.max(np.abs(w64.astype(CR.LD) - want))) / scale
    return keys, want, scale, max(8.0 * e64, FLOOR), e64


def _gpu_matrix(T, c, dcp, coefs, rational):
    A, b, cc, m = coefs
    coef = T.dev.coef_transform(c["uks"], c["p"], dcp, _dv(T, A), _dv(T, b), _dv(T, cc), _dv(T, m), nq=c["nq"], rational=rational)
    return T.dev.assemble_coef_matrix(c["uks"], c["p"], dcp, coef, nq=c["nq"])


def _check_matrix(T, name, tag, c, dcp, coefs, rational, key=None):
    ref, ref64 = c["refs"][rational]
    keys, want, scale, bound, e64 = _bound(ref, ref64, "matrix", *coefs, key=key or (name, tag, rational))
    G = _gpu_matrix(T, c, dcp, coefs, rational).to_scipy()
    assert G.shape == (c["nnodes"], c["nnodes"])
    rows = np.repeat(np.arange(G.shape[0]), np.diff(G.indptr))
    at, inside = CR.values_at(keys, want, c["nnodes"], rows, G.indices)
    assert inside, "an entry of the reference lies outside the pattern"
    err = float(np.max(np.abs(G.data.astype(CR.LD) - at))) / scale
    print("matrix %-34s %-9s %s: error %7.2f eps, float64 reference %6.2f eps, bound %7.2f eps"
          % (name, tag, "rational" if rational else "plain   ", err / EPS, e64 / EPS, bound / EPS))
    assert err <= bound
    # the same bits in a second run
    G2 = _gpu_matrix(T, c, dcp, coefs, rational).to_scipy()
    assert np.array_equal(G.data.view(np.int64), G2.data.view(np.int64))
    return G


def _check_load(T, name, tag, c, dcp, s, F, rational):
    ref, ref64 = c["refs"][rational]
    _, want, scale, bound, e64 = _bound(ref, ref64, "load", s, F)
    run = lambda: T.dev.quad_load_flux(c["uks"], c["p"], dcp, _dv(T, s), _dv(T, F), nq=c["nq"], rational=rational).get_local()
    b = run()
    err = float(np.max(np.abs(b.astype(CR.LD) - want))) / scale
    print("load   %-26s %-9s %s: error %7.2f eps, float64 reference %6.2f eps, bound %7.2f eps"
          % (name, tag, "rational" if rational else "plain   ", err / EPS, e64 / EPS, bound / EPS))
    assert err <= bound
    assert np.array_equal(b.view(np.int64), run().view(np.int64))
    # the transform alone: the same data on the reference element, twice the same bits
    t1 = T.dev.flux_transform(c["uks"], c["p"], dcp, _dv(T, s), _dv(T, F), nq=c["nq"], rational=rational).get_local()
    t2 = T.dev.flux_transform(c["uks"], c["p"], dcp, _dv(T, s), _dv(T, F), nq=c["nq"], rational=rational).get_local()
    assert t1.size == (len(c["uks"]) + 1) * c["npts"] and np.array_equal(t1.view(np.int64), t2.view(np.int64))


# ---- the kernels against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rational", [False, True])
@pytest.mark.parametrize("name", sorted(CASES) + ["volume_p2_2x3x2", "volume_p3_2x3x2"])
def test_matrix_and_load_match_the_reference(T, name, rational):
    c = _case(name)
    if rational:
        assert np.ptp(c["cp"][-1]) > 0.05                               # the weights do vary
    dcp = _dcp(T, c)
    for tag, coefs in sorted(_terms(c, name not in ALL_TERMS_ONLY).items()):
        _check_matrix(T, name, tag, c, dcp, coefs, rational)        # (the HOT names: whichever route is the default)
    for tag, (s, F) in (("s", (c["s"], None)), ("F", (None, c["Fv"])), ("s+F", (c["s"], c["Fv"]))):
        _check_load(T, name, tag, c, dcp, s, F, rational)


def _route_cases():
    out = []
    for name in sorted(HOT):
        for route in ("default", "legacy"):
            out.append((name, route))
        if HOT[name][1][0] > 2:                 # (p = 2: more than one piece of 2 elements; p = 3: the kernel that does not loop)
            out.append((name, "short_pieces"))
    return out


@pytest.mark.parametrize("name,route", _route_cases())
def test_sum_factorised_route_and_plain_kernel(T, name, route, monkeypatch, capfd):
    """3-D, nq = p + 1, p = 2, 3: the matrix comes from the sum-factorised kernels (p = 2 the walk along direction 0, p = 3
    the groups of four), with TIGAR_ASM_CHUNK / TIGAR_ASM_QUAD_CHUNK cutting the lines into short pieces, and from the plain
    kernel under TIGAR_ASM_LEGACY -- the library's timing line names the route -- and each holds the reference bound"""
    c = _case(name)
    dcp = _dcp(T, c)
    for k_, v_ in ROUTES[route].items():
        monkeypatch.setenv(k_, v_)
    monkeypatch.setenv("TIGAR_ASM_TIME", "1")
    capfd.readouterr()
    _gpu_matrix(T, c, dcp, (c["A"], c["b"], c["c"], c["m"]), True)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[tg_assemble]")]
    monkeypatch.delenv("TIGAR_ASM_TIME")
    assert len(lines) == 1 and ("(plain)" if route == "legacy" else "point coefficients") in lines[0], lines
    assert ("sum-factorised" in lines[0]) == (route != "legacy"), lines
    for rational in (True, False):
        for tag, coefs in sorted(_terms(c, name in EVERY_TERM).items()):
            _check_matrix(T, name + ":" + route, tag, c, dcp, coefs, rational, key=(name, tag, rational))


def test_an_absent_term_is_a_zero_term(T):
    c = _case("annulus_3x2")
    dcp = _dcp(T, c)
    zero_v, zero_s = np.zeros((c["npts"], c["nsd"])), np.zeros(c["npts"])
    for rational in (False, True):
        a = _gpu_matrix(T, c, dcp, (c["A"], None, None, c["m"]), rational).to_scipy()
        b = _gpu_matrix(T, c, dcp, (c["A"], zero_v, zero_v, c["m"]), rational).to_scipy()
        assert np.array_equal(a.data.view(np.int64), b.data.view(np.int64))
        l1 = T.dev.quad_load_flux(c["uks"], c["p"], dcp, None, _dv(T, c["Fv"]), nq=c["nq"], rational=rational).get_local()
        l2 = T.dev.quad_load_flux(c["uks"], c["p"], dcp, _dv(T, zero_s), _dv(T, c["Fv"]), nq=c["nq"], rational=rational).get_local()
        assert np.array_equal(l1.view(np.int64), l2.view(np.int64))


def test_source_load_is_the_point_load(T):
    """tg_quad_load_flux with s alone is tg_quad_load"""
    for name in ("annulus_3x2_nq4", "volume_p2_2x3x2"):
        c = _case(name)
        dcp = _dcp(T, c)
        for rational in (False, True):
            a = T.dev.quad_load_flux(c["uks"], c["p"], dcp, _dv(T, c["s"]), None, nq=c["nq"], rational=rational).get_local()
            b = T.dev.quad_load(c["uks"], c["p"], dcp, _dv(T, c["s"]), nq=c["nq"], rational=rational).get_local()
            assert np.max(np.abs(a - b)) <= FLOOR * np.max(np.abs(b))


# ---- cross checks through the forms ------------------------------------------------------------------------------------------
def _annulus_spline(T, nel, clamp=True):
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    gen = T.t.EqualOrderSpline(1, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf))
    if clamp:
        sp0 = gen.getScalarSpline(0)
        for direction in (0, 1):
            for side in (0, 1):
                gen.addZeroDofs(0, sp0.getSideDofs(direction, side))
    return gen, T.t.ExtractedSpline(gen, 4)


def _volume_spline(T, p, nels):
    from geom_util import rational_volume
    kvs, C = rational_volume(p, nels)
    gen = T.t.EqualOrderSpline(1, T.N.NURBSControlMesh([p] * 3, kvs, C))
    sp0 = gen.getScalarSpline(0)
    for direction in range(3):
        for side in (0, 1):
            gen.addZeroDofs(0, sp0.getSideDofs(direction, side))
    return gen, T.t.ExtractedSpline(gen, 2 * p)


def _patch_of(spline):
    g = spline.V.grids[0]
    return ([np.asarray(g.vertices[k], dtype=np.float64) for k in range(g.dim())], int(g.degree),
            [f.vector().get_local() for f in spline.cpFuncs])


@pytest.mark.parametrize("kind", ["annulus", "volume"])
@pytest.mark.parametrize("rational", [False, True])
def test_unit_coefficients_are_the_laplace_and_mass_forms(T, kind, rational):
    gen, spline = _annulus_spline(T, 3) if kind == "annulus" else _volume_spline(T, 2, (2, 3, 2))
    uks, p, cp = _patch_of(spline)
    ref, ref64 = CR.CoefReference(uks, p, cp, rational=rational), CR.CoefReference(uks, p, cp, rational=rational, dtype=np.float64)
    F = T.F
    for coefs, mine, twin in (((1.0, None, None, None), F.CoefficientForm(spline, diffusion=1, rational=rational),
                               F.LaplaceForm(geometry=spline, rational=rational)),
                              ((None, None, None, 1.0), F.CoefficientForm(spline, reaction=1, rational=rational),
                               F.MassForm(geometry=spline, rational=rational))):
        _, _, _, bound, _ = _bound(ref, ref64, "matrix", *coefs)
        A, B = mine.assemble_matrix(spline.V).to_scipy(), twin.assemble_matrix(spline.V).to_scipy()
        assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
        err = np.max(np.abs(A.data - B.data)) / np.max(np.abs(B.data))
        print("CoefficientForm against %s, %s %s: %.2f eps, bound %.2f eps"
              % (type(twin).__name__, kind, "rational" if rational else "plain", err / EPS, bound / EPS))
        assert err <= bound
        assert mine.symmetric is True


def test_flux_load_of_a_diffusive_flux_is_the_matrix_times_u(T):
    """tg_quad_load_flux with F = A grad u at the points against CoefficientForm(A) u"""
    for kind, rational in (("annulus", True), ("volume", False)):
        gen, spline = _annulus_spline(T, 4) if kind == "annulus" else _volume_spline(T, 2, (2, 2, 3))
        pts = spline.quadraturePoints()
        rng = np.random.default_rng(11)
        A = rng.standard_normal((pts.npts, pts.nsd, pts.nsd))
        u = T.t.Function(spline.V)
        u.vector().set_local(rng.standard_normal(spline.V.dim()))
        val, comps = spline.evaluateAtQuadrature(u, grad=True, rational=rational)
        g = np.stack([cmp.get_local() for cmp in comps], axis=1)
        flux = np.einsum("qij,qj->qi", A, g)
        load = T.F.QuadratureLoadForm(None, spline, rational=rational, flux=flux).assemble_vector(spline.V).get_local()
        Au = T.F.CoefficientForm(spline, diffusion=A, rational=rational).assemble_matrix(spline.V).mult(u.vector()).get_local()
        # both sides sum the same products in another order: rows of up to (2p + 1)^d entries of size |A_ab u_b|
        Aabs = abs(T.F.CoefficientForm(spline, diffusion=A, rational=rational).assemble_matrix(spline.V).to_scipy())
        scale = np.max(Aabs @ np.abs(u.vector().get_local()))
        err = np.max(np.abs(load - Au)) / scale
        print("flux load against matrix times u, %s: %.2f eps of the row sums of |A| |u|" % (kind, err / EPS))
        assert err <= 64 * EPS


def test_quadrature_load_form_without_flux_is_unchanged(T):
    gen, spline = _annulus_spline(T, 3)
    f = lambda x: np.cos(x[:, 0]) * x[:, 1]
    a = T.F.QuadratureLoadForm(f, spline).assemble_vector(spline.V).get_local()
    pts = spline.quadraturePoints()
    b = T.dev.quad_load(pts.verts, pts.p, pts.cp, pts.values(f), nq=pts.nq).get_local()
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_symmetric_only_when_the_inputs_prove_it(T):
    gen, spline = _annulus_spline(T, 2)
    F = T.F
    pts = spline.quadraturePoints()
    rng = np.random.default_rng(2)
    S = rng.standard_normal((pts.npts, 2, 2))
    S = S + S.transpose(0, 2, 1)
    N = S.copy()
    N[0, 0, 1] = np.nextafter(N[0, 1, 0], np.inf)                   # differs from its transpose in the last bit of one entry
    b = rng.standard_normal((pts.npts, 2))
    yes = [F.CoefficientForm(spline, diffusion=2.0), F.CoefficientForm(spline, diffusion=lambda x: 1.0 + x[:, 0] ** 2),
           F.CoefficientForm(spline, diffusion=S, reaction=3.0), F.CoefficientForm(spline, reaction=lambda x: x[:, 1]),
           F.CoefficientForm(spline, diffusion=S, flux_velocity=b, velocity=b.copy())]
    no = [F.CoefficientForm(spline, diffusion=N), F.CoefficientForm(spline, diffusion=S, flux_velocity=b),
          F.CoefficientForm(spline, velocity=b), F.CoefficientForm(spline, flux_velocity=b, velocity=np.nextafter(b, np.inf)),
          F.CoefficientForm(spline, diffusion=T.dev.DeviceVector(data=np.ascontiguousarray(N.transpose(1, 2, 0)).ravel()))]
    assert [f.symmetric for f in yes] == [True] * len(yes)
    assert [f.symmetric for f in no] == [False] * len(no)
    # ... and the matrices agree with the claim
    for f in (yes[2], yes[4]):
        A = f.assemble_matrix(spline.V).to_scipy()
        assert abs(A - A.T).max() <= 64 * EPS * abs(A).max()
    A = no[1].assemble_matrix(spline.V).to_scipy()
    assert abs(A - A.T).max() > 1e-3 * abs(A).max()
    assert T.F.Sum(yes[0], yes[2]).symmetric is True and T.F.Sum(yes[0], no[1]).symmetric is False


def test_certificate_and_ptap_route_of_the_laplace_twin(T):
    """the matrix of a CoefficientForm comes on the element-coupling pattern with its certificate: the extraction takes the
    route it takes for LaplaceForm(geometry=...) -- same counters of certified patterns and tensor line walks, same K
    pattern -- and a constant diffusion gives the twin's K"""
    gen, spline = _volume_spline(T, 2, (4, 3, 3))
    counters = lambda: (T.dev.prof_get(3)[1], T.dev.prof_get(5)[1])
    T.dev.prof_reset()
    Kt = spline.assembleMatrix(T.F.LaplaceForm(geometry=spline, rational=True)).to_scipy()
    twin = counters()
    T.dev.prof_reset()
    K = spline.assembleMatrix(T.F.CoefficientForm(spline, diffusion=1.0, rational=True)).to_scipy()
    mine = counters()
    print("certified patterns, tensor line walks: twin %r, coefficient form %r" % (twin, mine))
    assert mine == twin
    assert np.array_equal(K.indptr, Kt.indptr) and np.array_equal(K.indices, Kt.indices)
    assert abs(K - Kt).max() <= 1e-12 * abs(Kt).max()
    # the certificate itself: the x pass of the tensor PtAP takes the pattern without verifying it; a copy that went through
    # the host has none
    from tigar_amd.tensorptap import TensorPtAP
    plan = TensorPtAP.for_extraction(spline._kron)
    nfe2 = spline.V.grids[0].shape()[2]
    A = T.F.CoefficientForm(spline, diffusion=lambda x: 1.0 + x[:, 0] ** 2, velocity=[1.0, 0.0, 2.0]).assemble_matrix(spline.V)
    n0 = T.dev.prof_get(3)[1]
    assert plan.planes(A, 0, 0, nfe2) is not None and T.dev.prof_get(3)[1] == n0 + 1
    assert plan.planes(T.dev.DeviceCSR.from_scipy(A.to_scipy()), 0, 0, nfe2) is not None and T.dev.prof_get(3)[1] == n0 + 1


def test_inside_sum_with_the_boundary_forms(T):
    gen, spline = _annulus_spline(T, 3, clamp=False)
    F = T.F
    vol = F.CoefficientForm(spline, diffusion=lambda x: 1.0 + x[:, 0], reaction=2.0, rational=True)
    robin = F.BoundaryMassForm(3.0, spline, faces=[(0, 1)], rational=True)
    total = F.Sum(vol, robin)
    A = total.assemble_matrix(spline.V).to_scipy()
    assert total.in_place == 1                                       # the face term went into the pattern of the volume term
    B = vol.assemble_matrix(spline.V).to_scipy() + robin.assemble_matrix(spline.V).to_scipy()
    assert abs(A - B).max() <= 64 * EPS * abs(B).max()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(T, monkeypatch):
    import os
    t, B, F = T.t, T.B, T.F
    gen, spline = _annulus_spline(T, 2)
    V = spline.V
    npts, n = spline.quadraturePoints().npts, V.dim()
    u = t.Function(V)
    res = lambda f=None, **kw: F.QuasilinearResidual(u, spline, P.residual, P.tangent, f=f, **kw)
    # ValueError: geometry, counts, shapes, nq
    with pytest.raises(ValueError, match="geometry"):
        F.CoefficientForm(None, diffusion=1.0)
    with pytest.raises(ValueError, match="geometry"):
        F.QuasilinearResidual(u, None, P.residual, P.tangent)
    with pytest.raises(ValueError, match="geometry"):
        F.QuadratureLoadForm(1.0, None, flux=[1.0, 0.0])
    for bad in (dict(diffusion=np.ones(npts + 1)), dict(diffusion=np.ones((npts, 2, 3))), dict(diffusion=T.dev.DeviceVector(3 * npts)),
                dict(flux_velocity=np.ones((npts, 3))), dict(velocity=T.dev.DeviceVector(npts)), dict(reaction=np.ones(npts - 1)),
                dict(reaction=lambda x: np.ones((x.shape[0], 2))), dict(velocity=1.0)):
        with pytest.raises(ValueError, match="point|shape|values"):
            F.CoefficientForm(spline, **bad).assemble_matrix(V)
    with pytest.raises(ValueError, match="shape"):
        F.QuadratureLoadForm(1.0, spline, flux=np.ones((npts, 3))).assemble_vector(V)
    for nq in (0, T.dev.assemble_limits()[1] + 1):
        with pytest.raises(ValueError, match="nq"):
            F.CoefficientForm(spline, diffusion=1.0, nq=nq).assemble_matrix(V)
        with pytest.raises(ValueError, match="nq"):
            res(nq=nq).assemble_vector(V)
    with pytest.raises(ValueError, match="returns"):
        F.QuasilinearResidual(u, spline, lambda x, v, g: g, P.tangent).assemble_vector(V)
    with pytest.raises(ValueError, match="returns"):
        F.QuasilinearResidual(u, spline, P.residual, lambda x, v, g: (None, None)).tangent().assemble_matrix(V)
    # the C entries check their arrays themselves
    uks, p, cp = _patch_of(spline)
    dcp = [T.dev.DeviceVector(data=v) for v in cp]
    with pytest.raises(T.dev.TigarHipError):
        T.dev.coef_transform(uks, p, dcp, T.dev.DeviceVector(npts), a_kind=2)
    with pytest.raises(T.dev.TigarHipError):
        T.dev.assemble_coef_matrix(uks, p, dcp, T.dev.DeviceVector(8 * npts))
    with pytest.raises(T.dev.TigarHipError):
        T.dev.quad_load_flux(uks, p, dcp, None, T.dev.DeviceVector(npts))
    # NotImplementedError: row blocks, several ranks, the caller's dof order, other spaces
    plane = V.grids[0].shape()[0]
    for call in (lambda: F.CoefficientForm(spline, diffusion=1.0).assemble_matrix(V, 0, plane), lambda: res().assemble_vector(V, plane, n),
                 lambda: res().tangent().assemble_matrix(V, 0, plane),
                 lambda: F.QuadratureLoadForm(1.0, spline, flux=[1.0, 0.0]).assemble_vector(V, 0, plane)):
        with pytest.raises(NotImplementedError, match="row blocks"):
            call()
    calls = (lambda s: F.CoefficientForm(s, diffusion=1.0).assemble_matrix(s.V),
             lambda s: F.QuasilinearResidual(t.Function(s.V), s, P.residual, P.tangent).assemble_vector(s.V),
             lambda s: F.QuasilinearResidual(t.Function(s.V), s, P.residual, P.tangent).tangent().assemble_matrix(s.V),
             lambda s: F.QuadratureLoadForm(1.0, s, flux=lambda x: x).assemble_vector(s.V))
    with monkeypatch.context() as m:
        m.setattr(spline, "_distributed", lambda: True)
        for call in calls:
            with pytest.raises(NotImplementedError, match="ranks"):
                call(spline)
    with monkeypatch.context() as m:
        m.setattr(spline, "_caller_ordered", lambda: True)
        for call in calls:
            with pytest.raises(NotImplementedError, match="feOrder"):
                call(spline)
    kv2 = [B.uniformKnots(2, 0.0, 1.0, 3)] * 2
    cm = B.ExplicitBSplineControlMesh([2, 2], kv2)
    two = t.ExtractedSpline(t.EqualOrderSpline(2, cm), 4)
    lst = t.ExtractedSpline(t.FieldListSpline(cm, [B.BSpline([2, 2], kv2)]), 4)
    kvd = [0, 0, 0, 0.5, 0.5, 0.5, 1, 1, 1]
    dg = t.ExtractedSpline(t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2, 2], [kvd, kvd])), 4)
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
    others = [(two, "nFields"), (lst, "FieldListSpline"), (dg, "DG"), (t.ExtractedSpline(BSplineCompat(cm, "RT", [1, 1]), 4), "scalar spaces|not supported"),
              (t.ExtractedSpline(t.EqualOrderSpline(1, TwoPatches()), 4), "not supported"),
              (t.ExtractedSpline(t.EqualOrderSpline(1, RhinoTSplineControlMesh(
                  os.path.join(os.path.dirname(__file__), "golden", "tspline_bicubic_patch.iga"))), 4), "not supported")]
    for s, word in others:
        for call in calls:
            with pytest.raises(NotImplementedError, match=word):
                call(s)


# ---- Newton ------------------------------------------------------------------------------------------------------------------
_HOST_FLOW = {}


def _host_flow(nel):
    if nel not in _HOST_FLOW:
        _HOST_FLOW[nel] = P.host_flow(nel)
    return _HOST_FLOW[nel]


def test_quasilinear_newton_on_the_annulus(T, capsys):
    """-div(grad u / sqrt(1 + |grad u|^2)) + u^3 = f, manufactured solution, p = 2, rational, zero dofs on all edges: the device
    flow takes the iteration count of the host flow +- 1, its error norms equal the host flow's to relative 1e-6 (both
    solve the same discrete problem to the Newton tolerance 1e-10; the discretisation errors are 1e-3 .. 1e-5), and the L2
    ratios tend to 2^(p+1)"""
    l2 = []
    for nel in (4, 8, 16):
        gen, spline = _annulus_spline(T, nel)
        solver = T.t.PETScLUSolver()
        spline.setSolverOptions(linearSolver=solver, relativeTolerance=1e-10, maxIters=25)
        u = T.t.Function(spline.V)
        res = T.F.QuasilinearResidual(u, spline, P.residual, P.tangent, f=P.rhs, rational=True)
        hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u)
        U, hhist, (hl2, hh10) = _host_flow(nel)
        e0 = spline.errorNorm(u, P.exact, "L2", rational=True)
        e1 = spline.errorNorm(u, P.exact, "H10", exact_grad=P.exact_grad, rational=True)
        with capsys.disabled():
            print("newton nel %2d: device %d iterations (host %d), L2 %.6e (host %.6e), H10 %.6e (host %.6e)"
                  % (nel, len(hist), len(hhist), e0, hl2, e1, hh10))
        assert abs(len(hist) - len(hhist)) <= 1
        assert abs(e0 - hl2) <= 1e-6 * hl2 and abs(e1 - hh10) <= 1e-6 * hh10
        l2.append(e0)
    assert l2[0] / l2[1] > 7.0 and l2[1] / l2[2] > 7.5
    assert abs(l2[1] / l2[2] - 8.0) < abs(l2[0] / l2[1] - 8.0) + 0.1        # ... tending to 2^(p+1)
