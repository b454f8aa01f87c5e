"""GPU: finite-strain elasticity on a mapped patch -- the material laws at the points (``tg_material_points``,
csrc/tg_material.hip), the block ending of k_postproc (``tg_coef_transform_blocks``), the block assembly
(``tg_assemble_coef_blocks``) and what is built on them: ``forms.VectorCoefficientForm``, ``forms.VectorLoadForm``,
``forms.HyperelasticResidual`` under ``solveNonlinearVariationalProblem``.

Reference: tests/hyper_reference.py (dense loops over elements and points with the Cartesian gradients formed directly; the
laws are the numpy ``host`` methods, pinned by tests/test_hyper_reference_host.py).  Tangents and reactions of the block
tests are RANDOM per point and not symmetric, so that any mis-numbering of points, blocks or indices shows.

Tolerance: normwise, max |error| / max |reference| against the longdouble run.  The bound of a case is 8 x the error of the
float64 run of the same reference for that case (computed here, on the CPU: no figure of the code under test), and never
below 32 eps -- the rule of tests/test_gpu_coef.py.

Measured on the MI355X (``-s`` prints every figure): the largest error / bound over the cases of this file is in the
README section "Finite-strain elasticity".
"""
import numpy as np
import pytest

from oracle import tigar_oracle as O
import postproc_reference as R
import coef_reference as CR
import hyper_reference as H

pytestmark = pytest.mark.gpu

EPS = R.EPS
FLOOR = 32 * EPS
LD = CR.LD
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


def _laws(F, lam=LAM, mu=MU):
    return [F.LinearElastic(lam, mu), F.StVenantKirchhoff(lam, mu), F.NeoHookean(lam, mu)]


def _normwise(got, want, want64):
    """(error, bound, float64 error) of ``got`` against the longdouble ``want``: all relative to max |want|"""
    scale = float(np.max(np.abs(want)))
    e64 = float(np.max(np.abs(np.asarray(want64).astype(LD) - want))) / scale
    return float(np.max(np.abs(np.asarray(got).astype(LD) - want))) / scale, max(8.0 * e64, FLOOR), e64


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- the law kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsd", [2, 3])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_material_points_match_the_host_law(T, kind, nsd):
    """1000 random F with J in [0.3, 3] (four workgroups, the last one partly filled): P, A and psi against the longdouble
    law, every subset of outputs gives the same bits, and so does a second run"""
    npts = 1000
    Fm = H.random_F(nsd, npts, 100 * kind + nsd)
    Hm = Fm - np.eye(nsd)
    law = _laws(T.F)[kind]
    assert law.kind == kind
    want, want64 = law.host((Hm + np.eye(nsd)).astype(LD)), law.host(Hm + np.eye(nsd))
    gradu = T.dev.DeviceVector(data=np.ascontiguousarray(Hm.transpose(1, 2, 0)).ravel())
    P, A, psi, nbad, jmin = T.dev.material_points(kind, LAM, MU, nsd, gradu, True, True, True)
    J = np.linalg.det(Fm)
    assert nbad == 0 and abs(jmin - J.min()) <= 8 * EPS * J.min() and 0.3 <= J.min() and J.max() <= 3.0
    got = (P.get_local().reshape(nsd, nsd, npts).transpose(2, 0, 1),
           A.get_local().reshape(nsd, nsd, nsd, nsd, npts).transpose(4, 0, 2, 1, 3), psi.get_local())
    for name, g, w, w64 in zip(("P", "A", "psi"), got, want, want64):
        err, bound, e64 = _normwise(g, w, w64)
        print("law kind %d nsd %d %-3s: error %6.2f eps, float64 law %6.2f eps, bound %6.2f eps" % (kind, nsd, name, err / EPS, e64 / EPS, bound / EPS))
        assert err <= bound
    for mask in range(1, 8):
        P2, A2, psi2, _, j2 = T.dev.material_points(kind, LAM, MU, nsd, gradu, bool(mask & 1), bool(mask & 2), bool(mask & 4))
        assert j2 == jmin and (P2 is None) == (not mask & 1) and (A2 is None) == (not mask & 2) and (psi2 is None) == (not mask & 4)
        for a, b in ((P, P2), (A, A2), (psi, psi2)):
            assert b is None or _same(a.get_local(), b.get_local())


def test_material_points_refuse_bad_arguments(T):
    g = T.dev.DeviceVector(4 * 10)
    for bad in (lambda: T.dev.material_points(3, LAM, MU, 2, g), lambda: T.dev.material_points(0, LAM, MU, 4, T.dev.DeviceVector(160)),
                lambda: T.dev.material_points(0, LAM, MU, 3, T.dev.DeviceVector(91))):
        with pytest.raises(T.dev.TigarHipError):
            bad()


# ---- blocks and routes ---------------------------------------------------------------------------------------------------------
def _poly_nodes(nels, p, weighted):
    """non-uniform element vertices and a smooth polynomial map of the Q_p nodes; ``weighted``: weights varying by a third"""
    d = len(nels)
    rng = np.random.default_rng(7 * d + p)
    uks = []
    for k in range(d):
        steps = rng.uniform(0.6, 1.4, nels[k])
        uks.append(np.concatenate([[0.0], np.cumsum(steps) / np.sum(steps) * (1.0 + 0.5 * k)]))
    X = R.lagrange_nodes(uks, p)
    wgt = 1.0 + 0.3 * X[0] * X[-1] + 0.1 * X[0] ** 2 if weighted else np.ones_like(X[0])
    return uks, [(X[i] + 0.1 * X[(i + 1) % d] ** 2) * wgt for i in range(d)] + [wgt]


HOT = {"volume_p2_1x1x1": (2, (1, 1, 1)), "volume_p2_2x3x2": (2, (2, 3, 2)), "volume_p2_5x3x2": (2, (5, 3, 2)),
       "volume_p2_17x1x2": (2, (17, 1, 2)), "volume_p3_1x1x1": (3, (1, 1, 1)), "volume_p3_2x3x2": (3, (2, 3, 2)),
       "volume_p3_5x3x2": (3, (5, 3, 2)), "volume_p3_17x1x2": (3, (17, 1, 2))}
ROUTES = {"default": {}, "short_pieces": {"TIGAR_ASM_CHUNK": "2", "TIGAR_ASM_QUAD_CHUNK": "1"}, "legacy": {"TIGAR_ASM_LEGACY": "1"}}
# the plain kernel only: (p, nq, element vertices, control functions)
PLAIN = {
    "annulus_3x2": lambda: (2, None) + _annulus_nodes((3, 2)),
    "2d_p1_4x3_nq3": lambda: (1, 3) + _poly_nodes((4, 3), 1, True),
    "2d_p3_2x3_nq5": lambda: (3, 5) + _poly_nodes((2, 3), 3, True),
    "2d_p3_3x2_nq1": lambda: (3, 1) + _poly_nodes((3, 2), 3, True),
    "2d_p4_2x2_nq3": lambda: (4, 3) + _poly_nodes((2, 2), 4, True),
    "volume_p1_2x3x2": lambda: (1, None) + R.volume_patch(1, (2, 3, 2)),
}


def _annulus_nodes(nels):
    """the exact quarter annulus on nels[0] x nels[1] elements: its homogeneous coordinates are quadratics in the parameters,
    which the Q_2 nodal interpolation on any mesh reproduces"""
    uks1, cp1 = R.annulus_patch(1)
    uks = [np.linspace(0.0, 1.0, n + 1) for n in nels]
    X = R.lagrange_nodes(uks, 2)
    l = lambda t: np.stack([2.0 * (t - 0.5) * (t - 1.0), -4.0 * t * (t - 1.0), 2.0 * t * (t - 0.5)])
    L0, L1 = l(X[0]), l(X[1])
    return uks, [np.einsum("an,bn,ab->n", L0, L1, np.asarray(c).reshape(3, 3, order="F")) for c in cp1]


_CASE = {}


def _case(name):
    """patch, a random tangent and reaction and, per space (plain / rational), the reference matrix with and without the
    reaction in longdouble and float64: built once, shared by the routes"""
    if name not in _CASE:
        if name in HOT:
            p, nq = HOT[name][0], None
            uks, cp = R.volume_patch(*HOT[name])
        else:
            p, nq, uks, cp = PLAIN[name]()
        cp = [np.asarray(c, dtype=np.float64) for c in cp]
        d = len(uks)
        npts = int(np.prod([(len(u) - 1) * (p + 1 if nq is None else nq) for u in uks]))
        rng = np.random.default_rng(sum(map(ord, name)))
        _CASE[name] = dict(p=p, nq=nq, uks=uks, cp=cp, d=d, npts=npts, A=rng.standard_normal((npts, d, d, d, d)),
                           M=rng.standard_normal((npts, d, d)), want={})
    return _CASE[name]


def _reference_matrix(c, rational, with_reaction):
    """(keys of the nF n square matrix, longdouble values, float64 values)"""
    key = (rational, with_reaction)
    if key not in c["want"]:
        out = []
        for dt in (LD, np.float64):
            ref = H.HyperReference(c["uks"], c["p"], c["cp"], c["nq"], rational=rational, dtype=dt)
            n, nF = ref.n, ref.nF
            keys, vals = [], []
            for (i, j), (k, v) in ref.blocks(c["A"], c["M"] if with_reaction else None).items():
                keys.append((i * n + k // n) * (nF * n) + j * n + k % n)
                vals.append(v)
            keys, vals = np.concatenate(keys), np.concatenate(vals)
            o = np.argsort(keys)
            out.append((keys[o], vals[o], n))
        assert np.array_equal(out[0][0], out[1][0])
        c["want"][key] = (out[0][0], out[0][1], out[1][1], out[0][2])
    return c["want"][key]


def _dv_tangent(T, A):
    return T.dev.DeviceVector(data=np.ascontiguousarray(A.transpose(1, 3, 2, 4, 0)).ravel())


def _dv_reaction(T, M):
    return None if M is None else T.dev.DeviceVector(data=np.ascontiguousarray(M.transpose(1, 2, 0)).ravel())


def _gpu_blocks(T, c, dcp, rational, with_reaction):
    coef = T.dev.coef_transform_blocks(c["uks"], c["p"], dcp, _dv_tangent(T, c["A"]), _dv_reaction(T, c["M"]) if with_reaction else None,
                                       nq=c["nq"], rational=rational)
    return coef, T.dev.assemble_coef_blocks(c["uks"], c["p"], dcp, coef, nq=c["nq"])


def _check_blocks(T, name, tag, c, dcp, rational, with_reaction=True):
    keys, want, want64, n = _reference_matrix(c, rational, with_reaction)
    coef, K = _gpu_blocks(T, c, dcp, rational, with_reaction)
    G = K.to_scipy()
    nF = c["d"]
    assert G.shape == (nF * n, nF * n)
    rows = np.repeat(np.arange(G.shape[0]), np.diff(G.indptr))
    at, inside = CR.values_at(keys, want, nF * n, rows, G.indices)
    assert inside, "an entry of the reference lies outside the pattern"
    scale = float(np.max(np.abs(want)))
    e64 = float(np.max(np.abs(want64.astype(LD) - want))) / scale
    bound = max(8.0 * e64, FLOOR)
    err = float(np.max(np.abs(G.data.astype(LD) - at))) / scale
    print("blocks %-18s %-13s %s %s: error %7.2f eps, float64 reference %6.2f eps, bound %7.2f eps"
          % (name, tag, "rational" if rational else "plain   ", "A+M" if with_reaction else "A  ", err / EPS, e64 / EPS, bound / EPS))
    assert err <= bound
    # the same bits in a second run of both entry points
    coef2, K2 = _gpu_blocks(T, c, dcp, rational, with_reaction)
    assert _same(coef.get_local(), coef2.get_local()) and _same(G.data, K2.to_scipy().data)
    return coef, G


def _route_cases():
    out = []
    for name in sorted(HOT):
        for route in ("default", "short_pieces", "legacy"):
            out.append((name, route))
    return out


@pytest.mark.parametrize("name,route", _route_cases())
def test_blocks_on_the_sum_factorised_route_and_the_plain_kernel(T, name, route, monkeypatch, capfd):
    """3-D, nq = p + 1, p = 2, 3: every block comes from the sum-factorised kernels, with TIGAR_ASM_CHUNK /
    TIGAR_ASM_QUAD_CHUNK cutting the lines into short pieces (17 elements: the seam of the default pieces), and from the plain
    kernel under TIGAR_ASM_LEGACY -- the library's timing line of each of the nine blocks names the route"""
    c = _case(name)
    dcp = [T.dev.DeviceVector(data=v) for v in c["cp"]]
    for k_, v_ in ROUTES[route].items():
        monkeypatch.setenv(k_, v_)
    monkeypatch.setenv("TIGAR_ASM_TIME", "1")
    capfd.readouterr()
    _gpu_blocks(T, c, dcp, True, True)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[tg_assemble]")]
    monkeypatch.delenv("TIGAR_ASM_TIME")
    assert len(lines) == 9, lines
    for ln in lines:
        assert ("(plain)" if route == "legacy" else "point coefficients") in ln and ("sum-factorised" in ln) == (route != "legacy"), lines
    _check_blocks(T, name, route, c, dcp, True)
    if route == "default" and c["npts"] < 800:                           # (the functions phi as well, where the reference is cheap)
        _check_blocks(T, name, route, c, dcp, False)


@pytest.mark.parametrize("rational", [False, True])
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_blocks_on_the_plain_kernel(T, name, rational):
    """the shapes without a sum-factorised route: the quarter annulus, 2-D polynomial maps at p = 1, 3, 4 with nq != p + 1 and
    nq = 1, 3-D at p = 1; random non-symmetric tangent and reaction"""
    c = _case(name)
    if rational:
        assert np.ptp(c["cp"][-1]) > 0.05                               # the weights do vary
    dcp = [T.dev.DeviceVector(data=v) for v in c["cp"]]
    _check_blocks(T, name, "plain kernel", c, dcp, rational)
    _check_blocks(T, name, "plain kernel", c, dcp, rational, with_reaction=False)


def test_an_absent_reaction_is_a_zero_reaction(T):
    for name in ("annulus_3x2", "volume_p2_2x3x2"):
        c = _case(name)
        dcp = [T.dev.DeviceVector(data=v) for v in c["cp"]]
        for rational in (False, True):
            tr = lambda M: T.dev.coef_transform_blocks(c["uks"], c["p"], dcp, _dv_tangent(T, c["A"]), M, nq=c["nq"], rational=rational)
            a, b = tr(None), tr(_dv_reaction(T, np.zeros_like(c["M"])))
            assert _same(a.get_local(), b.get_local())
            Ka = T.dev.assemble_coef_blocks(c["uks"], c["p"], dcp, a, nq=c["nq"]).to_scipy()
            Kb = T.dev.assemble_coef_blocks(c["uks"], c["p"], dcp, b, nq=c["nq"]).to_scipy()
            assert _same(Ka.data, Kb.data)


def test_block_transform_is_the_scalar_transform_of_each_block(T):
    """the fused ending computes the geometry once: every block equals ``tg_coef_transform(a_kind = 2)`` of that block's tensor
    and reaction, bit for bit (the same operations in the same order)"""
    for name, rational in (("annulus_3x2", True), ("volume_p2_2x3x2", False), ("volume_p3_2x3x2", True)):
        c = _case(name)
        d, npts = c["d"], c["npts"]
        dcp = [T.dev.DeviceVector(data=v) for v in c["cp"]]
        coef = T.dev.coef_transform_blocks(c["uks"], c["p"], dcp, _dv_tangent(T, c["A"]), _dv_reaction(T, c["M"]), nq=c["nq"],
                                           rational=rational).get_local().reshape(d, d, -1)
        for i in range(d):
            for j in range(d):
                one = T.dev.coef_transform(c["uks"], c["p"], dcp, T.dev.DeviceVector(data=np.ascontiguousarray(
                    c["A"][:, i, :, j, :].transpose(1, 2, 0)).ravel()), None, None, T.dev.DeviceVector(data=np.ascontiguousarray(c["M"][:, i, j])),
                    a_kind=2, nq=c["nq"], rational=rational).get_local()
                assert _same(coef[i, j], one), (name, i, j)


# ---- geometries for the forms ----------------------------------------------------------------------------------------------------
def _bspline_patch(T, p, nels, fields):
    """a smooth polynomial map of degree p with unit weights (a B-spline patch): (generator, knot vectors, control net)"""
    d = len(nels)
    kvs = [np.asarray(O.uniform_knots(p, 0., 1., n), dtype=np.float64) for n in nels]
    grev = [np.array([np.sum(kv[i + 1:i + p + 1]) / p for i in range(len(kv) - p - 1)]) for kv in kvs]
    g = np.meshgrid(*grev, indexing="ij")
    if d == 2:
        X = [g[0] + 0.15 * g[1] * g[0], g[1] * (1.0 + 0.2 * g[0]) - 0.1 * g[0]]
    else:
        X = [g[0] + 0.15 * g[1] * g[2], g[1] + 0.2 * g[0] * g[2] - 0.1 * g[2], g[2] * (1.0 + 0.3 * g[0])]
    C = np.stack(X + [np.ones_like(g[0])], axis=-1)
    return T.t.EqualOrderSpline(fields, T.N.NURBSControlMesh([p] * d, kvs, C)), kvs, C


def _annulus_gen(T, nel, fields=2):
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    return T.t.EqualOrderSpline(fields, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf)), [kv, kv], Pf


def _volume_gen(T, p, nels, fields=3):
    from geom_util import rational_volume
    kvs, C = rational_volume(p, nels)
    return T.t.EqualOrderSpline(fields, T.N.NURBSControlMesh([p] * 3, kvs, C)), kvs, C


def _patch_of(gen):
    g = gen.V.grids[0]
    return ([np.asarray(g.vertices[k], dtype=np.float64) for k in range(g.dim())], int(g.degree),
            [f.vector().get_local() for f in gen.cpFuncs])


def _function(T, V, values):
    u = T.t.Function(V)
    u.vector().set_local(np.asarray(values, dtype=np.float64))
    return u


def _refs(gen, nq=None, rational=False):
    uks, p, cp = _patch_of(gen)
    return H.HyperReference(uks, p, cp, nq, rational=rational), H.HyperReference(uks, p, cp, nq, rational=rational, dtype=np.float64)


# ---- the forms against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["annulus", "volume"])
def test_residual_tangent_and_energy_match_the_reference(T, geometry):
    """``HyperelasticResidual`` at a random state, rational, with a body force: vector, matrix and energy against the
    reference, twice the same bits, K - K^T to rounding and ``symmetric`` True for the three laws; a host law takes the same
    way and gives the matrix of the device law to the same bound"""
    gen, _, _ = _annulus_gen(T, 3) if geometry == "annulus" else _volume_gen(T, 2, (2, 2, 3))
    ref, ref64 = _refs(gen, rational=True)
    nF, n = ref.nF, ref.n
    rng = np.random.default_rng(5)
    un = 0.03 * rng.standard_normal(nF * n)
    u = _function(T, gen.V, un)
    body = lambda x: np.stack([np.sin(x[:, 0]), x[:, 1] ** 2, np.cos(x[:, -1])], axis=1)[:, :nF]
    fq = body(ref.x.astype(np.float64))
    for law in _laws(T.F):
        res = T.F.HyperelasticResidual(u, gen, law, body_force=body, rational=True)
        r = res.assemble_vector(gen.V).get_local()
        err, bound, e64 = _normwise(r, ref.residual(un, law, fq), ref64.residual(un, law, fq))
        print("residual %-8s %-18s: error %6.2f eps, float64 reference %6.2f eps, bound %6.2f eps" % (geometry, type(law).__name__, err / EPS, e64 / EPS, bound / EPS))
        assert err <= bound
        assert _same(r, res.assemble_vector(gen.V).get_local())
        tan = res.tangent()
        assert tan.symmetric is True
        K = tan.assemble_matrix(gen.V).to_scipy()
        err, bound, e64 = _normwise(K.toarray(), ref.tangent(un, law), ref64.tangent(un, law))
        print("tangent  %-8s %-18s: error %6.2f eps, float64 reference %6.2f eps, bound %6.2f eps" % (geometry, type(law).__name__, err / EPS, e64 / EPS, bound / EPS))
        assert err <= bound
        assert _same(K.data, tan.assemble_matrix(gen.V).to_scipy().data)
        assert abs(K - K.T).max() <= 2 * bound * abs(K).max()
        B = tan.assemble_block(gen.V, nF - 1, 0).to_scipy()
        assert abs(B - K[(nF - 1) * n:, :n]).max() == 0.0
        E = res.energy(gen.V)
        want, want64 = ref.energy(un, law), ref64.energy(un, law)
        # a sum of npts positive terms: 8 x the float64 reference's error, never below 32 eps, of the sum itself
        assert abs(E - float(want)) <= max(8.0 * abs(float(want64 - want)), FLOOR * abs(float(want)))
        assert E == res.energy(gen.V)

        class HostLaw(object):
            def host(self, Fm, law=law):
                return law.host(Fm)
        hres = T.F.HyperelasticResidual(u, gen, HostLaw(), body_force=body, rational=True)
        htan = hres.tangent()
        assert htan.symmetric is False                                  # nothing seen yet
        Kh = htan.assemble_matrix(gen.V).to_scipy()
        errh, _, _ = _normwise(Kh.toarray(), ref.tangent(un, law), ref64.tangent(un, law))
        assert errh <= bound
        assert htan.symmetric is True                                   # (the bits of this law's tangent prove it)
        errh, boundr, _ = _normwise(hres.assemble_vector(gen.V).get_local(), ref.residual(un, law, fq), ref64.residual(un, law, fq))
        assert errh <= boundr


@pytest.mark.parametrize("geometry,rational", [("annulus", True), ("volume", True), ("bspline3", False), ("bspline2", False)])
def test_linear_law_is_the_mapped_elasticity_form(T, geometry, rational):
    """``LinearElastic`` through the law kernel, the block transform and the block assembly against
    ``ElasticityForm(geometry=...)``: the same pattern, values to the bound of the reference for this case"""
    gen = {"annulus": lambda: _annulus_gen(T, 3), "volume": lambda: _volume_gen(T, 2, (2, 3, 2)),
           "bspline3": lambda: _bspline_patch(T, 3, (2, 1, 2), 3), "bspline2": lambda: _bspline_patch(T, 3, (3, 2), 2)}[geometry]()[0]
    ref, ref64 = _refs(gen, rational=rational)
    law = T.F.LinearElastic(LAM, MU)
    zero = np.zeros(ref.nF * ref.n)
    _, bound, _ = _normwise(ref64.tangent(zero, law), ref.tangent(zero, law), ref64.tangent(zero, law))
    u = _function(T, gen.V, 0.1 * np.random.default_rng(1).standard_normal(zero.size))       # (the tangent does not depend on it)
    A = T.F.HyperelasticResidual(u, gen, law, rational=rational).tangent().assemble_matrix(gen.V).to_scipy()
    B = T.F.ElasticityForm(LAM, MU, geometry=gen, rational=rational).assemble_matrix(gen.V).to_scipy()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    err = np.max(np.abs(A.data - B.data)) / np.max(np.abs(B.data))
    print("LinearElastic against ElasticityForm, %s: %.2f eps, bound %.2f eps" % (geometry, err / EPS, bound / EPS))
    assert err <= bound


def test_vector_forms_symmetry_flags_and_loads(T):
    gen, _, _ = _annulus_gen(T, 2)
    F = T.F
    ref, ref64 = _refs(gen)
    npts, nF = ref.npts, 2
    rng = np.random.default_rng(2)
    A = rng.standard_normal((npts, 2, 2, 2, 2))
    S = A + A.transpose(0, 3, 4, 1, 2)
    N = S.copy()
    N[0, 0, 1, 1, 0] = np.nextafter(N[0, 1, 0, 0, 1], np.inf)         # differs from its major transpose in the last bit of one entry
    M = rng.standard_normal((npts, 2, 2))
    Ms = M + M.transpose(0, 2, 1)
    yes = [F.VectorCoefficientForm(gen, S), F.VectorCoefficientForm(gen, S, reaction=Ms), F.VectorCoefficientForm(gen, _dv_tangent(T, S)),
           F.VectorCoefficientForm(gen, lambda x: S, reaction=np.eye(2))]
    no = [F.VectorCoefficientForm(gen, N), F.VectorCoefficientForm(gen, S, reaction=M), F.VectorCoefficientForm(gen, _dv_tangent(T, N)),
          F.VectorCoefficientForm(gen, S, reaction=_dv_reaction(T, M))]
    assert [f.symmetric for f in yes] == [True] * len(yes)
    assert [f.symmetric for f in no] == [False] * len(no)
    K = yes[1].assemble_matrix(gen.V).to_scipy()
    assert abs(K - K.T).max() <= 64 * EPS * abs(K).max()
    K = no[1].assemble_matrix(gen.V).to_scipy()
    assert abs(K - K.T).max() > 1e-3 * abs(K).max()
    err, bound, _ = _normwise(K.toarray(), ref.dense(S, M), ref64.dense(S, M))
    assert err <= bound
    # the load form: f . v + flux : grad v, arrays, callables and a DeviceVector flux
    f, flux = rng.standard_normal((npts, 2)), rng.standard_normal((npts, 2, 2))
    want, want64 = ref.load(f, flux), ref64.load(f, flux)
    dflux = T.dev.DeviceVector(data=np.ascontiguousarray(flux.transpose(1, 2, 0)).ravel())
    for form in (F.VectorLoadForm(f, gen, flux=flux), F.VectorLoadForm(lambda x: f, gen, flux=lambda x: flux), F.VectorLoadForm(f, gen, flux=dflux)):
        b = form.assemble_vector(gen.V).get_local()
        err, bound, _ = _normwise(b, want, want64)
        assert err <= bound
        assert _same(b, form.assemble_vector(gen.V).get_local())
    b = F.VectorLoadForm([1.0, -2.0], gen).assemble_vector(gen.V).get_local()
    err, bound, _ = _normwise(b, ref.load(np.tile([1.0, -2.0], (npts, 1))), ref64.load(np.tile([1.0, -2.0], (npts, 1))))
    assert err <= bound


def test_certificate_and_ptap_route_of_the_elasticity_twin(T):
    """the tangent reaches the PtAP as the matrix of ``ElasticityForm(geometry=...)`` does: the same counters of certified
    patterns and tensor line walks, the same K pattern, and for the linear law the twin's K"""
    gen, _, _ = _volume_gen(T, 2, (4, 3, 3))
    sp0 = gen.getScalarSpline(0)
    for f in range(3):
        gen.addZeroDofs(f, sp0.getSideDofs(0, 0))
    spline = T.t.ExtractedSpline(gen, 4)
    counters = lambda: (T.dev.prof_get(3)[1], T.dev.prof_get(5)[1])
    T.dev.prof_reset()
    Kt = spline.assembleMatrix(T.F.ElasticityForm(LAM, MU, geometry=spline, rational=True)).to_scipy()
    twin = counters()
    u = T.t.Function(spline.V)
    T.dev.prof_reset()
    K = spline.assembleMatrix(T.F.HyperelasticResidual(u, spline, T.F.LinearElastic(LAM, MU), rational=True).tangent()).to_scipy()
    mine = counters()
    print("certified patterns, tensor line walks: twin %r, tangent %r" % (twin, mine))
    assert mine == twin
    assert np.array_equal(K.indptr, Kt.indptr) and np.array_equal(K.indices, Kt.indices)
    assert abs(K - Kt).max() <= 1e-12 * abs(Kt).max()


# ---- physics -------------------------------------------------------------------------------------------------------------------
G3 = np.array([[1.2, 0.15, 0.0], [-0.1, 0.9, 0.05], [0.05, 0.0, 1.1]])


def _rotation(d):
    a = 0.4
    Rm = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    if d == 3:
        b = 0.3
        Rm = Rm @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    return Rm[:d, :d]


def _affine_state(gen, G):
    """nodal values of u_h with u_h / W_h = (G - I) x: (G - I) applied to the homogeneous coordinates"""
    d = G.shape[0]
    cp = [f.vector().get_local() for f in gen.cpFuncs]
    return np.concatenate([sum((G - np.eye(d))[i, k] * cp[k] for k in range(d)) for i in range(d)])


def _interior(gen):
    g = gen.V.grids[0]
    shape = g.shape()
    idx = np.arange(int(np.prod(shape))).reshape(shape, order="F")
    return idx[(slice(1, -1),) * len(shape)].ravel()


@pytest.mark.parametrize("geometry", ["bspline3", "bspline2", "annulus"])
def test_homogeneous_deformation(T, geometry):
    """u = (G - I) x: P is constant, so the residual rows of interior nodes vanish to rounding, and with the traction t = P N
    on all faces (``BoundaryLoadForm`` in a ``Sum``) all rows do.  On the polynomial maps (unit weights) with the functions
    phi at nq = p + 1, where the integrands are polynomials that Gauss integrates exactly; on the annulus with phi / W_h the
    integrands are rational (at nq = 3 the interior rows are 2e-6 in the longdouble reference as well: the quadrature error of
    the discrete form), so that case runs at nq = 10, where that error is below rounding.  "To rounding": the bound of the
    reference rule for the residual of this state, relative to its largest row."""
    if geometry == "annulus":
        (gen, _, _), rational, nq = _annulus_gen(T, 4), True, 10
    else:
        (gen, _, _), rational, nq = _bspline_patch(T, 2, (3, 2, 2) if geometry == "bspline3" else (3, 4), int(geometry[-1])), False, None
    d = int(gen.V.grids[0].dim())
    G = G3[:d, :d]
    un = _affine_state(gen, G)
    u = _function(T, gen.V, un)
    ref, ref64 = _refs(gen, nq, rational)
    inner = _interior(gen)
    n = ref.n
    for law in _laws(T.F)[1:]:
        res = T.F.HyperelasticResidual(u, gen, law, nq=nq, rational=rational)
        r = res.assemble_vector(gen.V).get_local()
        want, want64 = ref.residual(un, law), ref64.residual(un, law)
        err, bound, e64 = _normwise(r, want, want64)
        scale = float(np.max(np.abs(want)))
        rows = np.concatenate([f * n + inner for f in range(d)])
        print("homogeneous %-8s %-18s: error %6.2f eps (bound %6.2f), interior rows %.2e of the largest row (reference %.2e)"
              % (geometry, type(law).__name__, err / EPS, bound / EPS, np.max(np.abs(r[rows])) / scale, float(np.max(np.abs(want[rows]))) / scale))
        assert err <= bound
        assert np.max(np.abs(r[rows])) <= bound * scale
        P = np.asarray(law.host(G[None])[0][0], dtype=np.float64)
        traction = T.F.BoundaryLoadForm(lambda x, nrm: -(nrm @ P.T), gen, nq=nq, rational=rational)
        total = T.F.Sum(res, traction).assemble_vector(gen.V).get_local()
        print("            with the traction P N on all faces: largest row %.2e of the largest residual row" % (np.max(np.abs(total)) / scale))
        # two sums of the size of the largest row cancel: the bound of each
        assert np.max(np.abs(total)) <= 2 * bound * scale


@pytest.mark.parametrize("geometry", ["bspline3", "annulus"])
def test_rigid_rotation_carries_no_stress_and_no_energy(T, geometry):
    """u = (R - I) x: F = R, P = 0 and psi = 0 for the two finite-strain laws, at any nq.  Rounding: the residual is a sum of
    terms wdet P : grad psi with |P| <= 64 eps (lambda + mu) (E = (R^T R - I) / 2 and ln J are a few eps), so every row is below
    that times S = int |grad psi_a| dx; the energy is quadratic in E: below vol (lambda + mu) (64 eps)^2 -- and mu (tr C - nsd)
    / 2 - mu ln J cancels to 64 eps mu per point for the neo-Hookean law."""
    if geometry == "annulus":
        (gen, _, _), rational = _annulus_gen(T, 3), True
    else:
        (gen, _, _), rational = _bspline_patch(T, 2, (2, 2, 2), 3), False
    d = int(gen.V.grids[0].dim())
    un = _affine_state(gen, _rotation(d))
    u = _function(T, gen.V, un)
    ref64 = _refs(gen, None, rational)[1]
    S = np.zeros(ref64.n)
    for g, PSI, Gr, wd in ref64.ref.elements:
        np.add.at(S, g, (wd[:, None] * np.sqrt(np.sum(Gr ** 2, axis=2))).sum(axis=0))
    vol = float(np.sum(ref64.ref.wdet()))
    for law in _laws(T.F, H.LAM, H.MU)[1:]:
        res = T.F.HyperelasticResidual(u, gen, law, rational=rational)
        r = res.assemble_vector(gen.V).get_local()
        E = res.energy(gen.V)
        print("rotation %-8s %-18s: largest row %.2e, energy %.2e" % (geometry, type(law).__name__, np.max(np.abs(r)), E))
        assert np.max(np.abs(r)) <= 64 * EPS * (H.LAM + H.MU) * S.max()
        assert abs(E) <= 64 * EPS * H.MU * vol


@pytest.mark.parametrize("geometry", ["annulus", "volume"])
def test_tangent_is_the_derivative_of_the_residual(T, geometry):
    """K(u) w against (R(u + h w) - R(u - h w)) / 2h at h = 1e-5.  The bound, from quantities of the reference alone:
    truncation h^2 / 6 C4 G^3 S (``hyper_reference.derivative_bounds`` at the extremes of F over the points, G = max |grad w|,
    S = max_a int |grad psi_a| dx); rounding: each residual carries the normwise error rho max |R| of the reference rule
    (rho = max(8 x float64 reference error, 32 eps)), so the quotient rho max |R| / h; and the product K w carries
    rho_K max |K| |w|_1-row sums, bounded by rho_K max |K| nnz_row max |w|."""
    gen, _, _ = _annulus_gen(T, 3) if geometry == "annulus" else _volume_gen(T, 2, (2, 2, 2))
    ref, ref64 = _refs(gen, rational=True)
    nF, n = ref.nF, ref.n
    rng = np.random.default_rng(8)
    un, w = 0.02 * rng.standard_normal(nF * n), rng.uniform(-0.2, 0.2, nF * n)
    h = 1e-5
    Fm = (ref64.grad_u(un) + np.eye(nF))
    sv = np.linalg.svd(Fm, compute_uv=False)
    G = float(np.max(np.sqrt(np.sum(ref64.grad_u(w) ** 2, axis=(1, 2)))))
    S = np.zeros(n)
    for g, PSI, Gr, wd in ref64.ref.elements:
        np.add.at(S, g, (wd[:, None] * np.sqrt(np.sum(Gr ** 2, axis=2))).sum(axis=0))
    c3, c4 = H.derivative_bounds(LAM, MU, 1.01 * sv.max(), 1.01 / sv.min(), 1.01 * np.max(np.abs(np.log(np.prod(sv, axis=1)))))
    for law in _laws(T.F)[1:]:
        want, want64 = ref.residual(un, law), ref64.residual(un, law)
        _, rho, _ = _normwise(want64, want, want64)
        Kw, Kw64 = ref.tangent(un, law), ref64.tangent(un, law)
        _, rhoK, _ = _normwise(Kw64, Kw, Kw64)
        nnz_row = nF * 5 ** nF                                          # (2p + 1)^d columns per field at p = 2
        bound = h * h / 6.0 * c4 * G ** 3 * float(S.max()) + rho * float(np.max(np.abs(want))) / h + \
            rhoK * float(np.max(np.abs(Kw))) * nnz_row * float(np.max(np.abs(w)))
        u = _function(T, gen.V, un)
        res = T.F.HyperelasticResidual(u, gen, law, rational=True)
        Kdev = res.tangent().assemble_matrix(gen.V)
        kw = Kdev.mult(T.dev.DeviceVector(data=w)).get_local()
        u.vector().set_local(un + h * w)
        rp = res.assemble_vector(gen.V).get_local()
        u.vector().set_local(un - h * w)
        rm = res.assemble_vector(gen.V).get_local()
        err = float(np.max(np.abs((rp - rm) / (2 * h) - kw)))
        print("K w against the difference of R, %-8s %-18s: %.2e, bound %.2e (truncation %.2e)"
              % (geometry, type(law).__name__, err, bound, h * h / 6.0 * c4 * G ** 3 * float(S.max())))
        assert err <= bound


# ---- Newton --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["block", "annulus"])
def test_neo_hookean_newton(T, name, capsys):
    """a face held, the opposite face displaced (the data sit in the initial dofs), neo-Hookean, rational, p = 2 -- 3-D on
    2 x 2 x 2 elements of the rational volume, 2-D (plane strain) on 4 x 4 elements of the quarter annulus: the device flow takes
    the iteration count of the host flow +- 1 and ends at its solution to relative 1e-6 (both solve the same discrete problem
    to the Newton tolerance 1e-9); the last two steps are of order >= 1.5 (see tests/test_hyper_reference_host.py)"""
    law = T.F.NeoHookean(H.LAM, H.MU)
    pb, Uh, hhist = H.host_flow(name, law)
    d = len(pb["kvs"])
    gen = T.t.EqualOrderSpline(d, T.N.NURBSControlMesh([pb["p"]] * d, pb["kvs"], pb["C"]))
    sp0 = gen.getScalarSpline(0)
    for f in range(d):
        for side in (0, 1):
            gen.addZeroDofs(f, sp0.getSideDofs(pb["direction"], side))
    spline = T.t.ExtractedSpline(gen, 2 * pb["p"])
    spline.setSolverOptions(linearSolver=T.t.PETScLUSolver(), relativeTolerance=H.NEWTON_TOL, maxIters=12)
    u = T.t.Function(spline.V)
    U = T.dev.DeviceVector(data=pb["U0"])
    res = T.F.HyperelasticResidual(u, spline, law, rational=True)
    hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u, igaDoFs=U)
    Ud = U.get_local()
    rel = np.max(np.abs(Ud - Uh)) / np.max(np.abs(Uh))
    with capsys.disabled():
        print("newton %-7s: device %d iterations (host %d), dofs differ by %.2e of the largest; device history %s"
              % (name, len(hist), len(hhist), rel, " ".join("%.1e" % v for v in hist)))
    assert abs(len(hist) - len(hhist)) <= 1
    assert rel <= 1e-6
    q = [np.log(hist[k + 1]) / np.log(hist[k]) for k in (-3, -2)]
    assert min(q) >= 1.5, q
    assert res.energy(spline.V) > 0.0


# ---- J <= 0 --------------------------------------------------------------------------------------------------------------------
def test_inverted_elements_raise_with_their_count(T):
    """the identity patch on 3 x 2 elements, p = 2: u_0 = -1.5 x_0 over the first column of elements and constant beyond gives
    F = diag(-0.5, 1) at the 2 x 9 points of that column and F = I elsewhere -- a Python error naming 18 points and J = -0.5,
    not a GPU fault; the other laws take the state, and the residual is usable again afterwards"""
    p = 2
    kvs = [T.B.uniformKnots(p, 0., 1., 3), T.B.uniformKnots(p, 0., 1., 2)]
    gen = T.t.EqualOrderSpline(2, T.B.ExplicitBSplineControlMesh([p, p], kvs))
    x0 = gen.cpFuncs[0].vector().get_local()
    un = np.concatenate([-1.5 * np.minimum(x0, 1.0 / 3.0), np.zeros_like(x0)])
    u = _function(T, gen.V, un)
    res = T.F.HyperelasticResidual(u, gen, T.F.NeoHookean(LAM, MU))
    for call in (lambda: res.assemble_vector(gen.V), lambda: res.tangent().assemble_matrix(gen.V), lambda: res.energy(gen.V)):
        with pytest.raises(RuntimeError, match=r"18 quadrature points with J <= 0 \(smallest J = -0\.5\)"):
            call()
    r = T.F.HyperelasticResidual(u, gen, T.F.StVenantKirchhoff(LAM, MU)).assemble_vector(gen.V).get_local()
    assert np.all(np.isfinite(r))
    u.vector().set_local(0.0 * un)
    assert np.max(np.abs(res.assemble_vector(gen.V).get_local())) == 0.0


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(T, monkeypatch):
    import os
    t, B, F = T.t, T.B, T.F
    gen, kvs, Pf = _annulus_gen(T, 2)
    spline = t.ExtractedSpline(gen, 4)
    V = spline.V
    n = V.grids[0].num_nodes()
    npts = 9 * 4                                                    # nq^2 points on each of the 2 x 2 elements
    u = t.Function(V)
    law = F.NeoHookean(LAM, MU)
    A = np.zeros((npts, 2, 2, 2, 2))
    calls = (lambda s: F.HyperelasticResidual(t.Function(s.V), s, law).assemble_vector(s.V),
             lambda s: F.HyperelasticResidual(t.Function(s.V), s, law).tangent().assemble_matrix(s.V),
             lambda s: F.VectorCoefficientForm(s, lambda x: np.zeros((x.shape[0], 2, 2, 2, 2))).assemble_matrix(s.V),
             lambda s: F.VectorLoadForm([1.0, 0.0], s).assemble_vector(s.V))
    # ValueError: geometry, material, shapes, counts, nq
    for make in (lambda: F.HyperelasticResidual(u, None, law), lambda: F.VectorCoefficientForm(None, A), lambda: F.VectorLoadForm([1.0, 0.0], None)):
        with pytest.raises(ValueError, match="geometry"):
            make()
    for bad in ("neo-hookean", object(), 3):
        with pytest.raises(ValueError, match="unknown material"):
            F.HyperelasticResidual(u, spline, bad)
    with pytest.raises(ValueError, match="neither"):
        F.VectorLoadForm(None, spline)
    for bad in (dict(tangent=np.zeros((npts, 2, 2, 2))), dict(tangent=np.zeros((npts + 1, 2, 2, 2, 2))), dict(tangent=T.dev.DeviceVector(16 * npts + 1)),
                dict(tangent=A, reaction=np.zeros((npts, 3, 2))), dict(tangent=A, reaction=T.dev.DeviceVector(npts))):
        with pytest.raises(ValueError, match="shape|values"):
            F.VectorCoefficientForm(spline, **bad).assemble_matrix(V)
    for form in (F.VectorLoadForm(np.zeros((npts, 3)), spline), F.VectorLoadForm(None, spline, flux=np.zeros((npts, 2, 3))),
                 F.VectorLoadForm(None, spline, flux=T.dev.DeviceVector(npts)), F.VectorLoadForm(lambda x: x[:, 0], spline)):
        with pytest.raises(ValueError, match="shape|values"):
            form.assemble_vector(V)
    with pytest.raises(ValueError, match="nodal values"):
        F.HyperelasticResidual(T.dev.DeviceVector(n), spline, law).assemble_vector(V)
    with pytest.raises(ValueError, match="returns|shapes"):
        class Bad(object):
            def host(self, Fm):
                return Fm, None
        F.HyperelasticResidual(u, spline, Bad()).assemble_vector(V)
    with pytest.raises(ValueError, match="block"):
        F.VectorCoefficientForm(spline, A).assemble_block(V, 0, 2)
    for nq in (0, T.dev.assemble_limits()[1] + 1):
        with pytest.raises(ValueError, match="nq"):
            F.HyperelasticResidual(u, spline, law, nq=nq).assemble_vector(V)
    # the C entries check their arguments themselves
    uks, p, cp = _patch_of(gen)
    dcp = [T.dev.DeviceVector(data=v) for v in cp]
    with pytest.raises(T.dev.TigarHipError):
        T.dev.coef_transform_blocks(uks, p, dcp, T.dev.DeviceVector(16 * npts - 1))
    with pytest.raises(T.dev.TigarHipError):
        T.dev.coef_transform_blocks(uks, p, dcp, T.dev.DeviceVector(16 * npts), T.dev.DeviceVector(3 * npts))
    with pytest.raises(T.dev.TigarHipError):
        T.dev.assemble_coef_blocks(uks, p, dcp, T.dev.DeviceVector(4 * 8 * npts))
    # NotImplementedError: row blocks, several ranks, the caller's dof order
    for call in (lambda: F.HyperelasticResidual(u, spline, law).assemble_vector(V, 0, n), lambda: F.HyperelasticResidual(u, spline, law).tangent().assemble_matrix(V, n, 2 * n),
                 lambda: F.VectorCoefficientForm(spline, A).assemble_matrix(V, 0, n), lambda: F.VectorCoefficientForm(spline, A).assemble_block(V, 0, 1, 0, 3),
                 lambda: F.VectorLoadForm([1.0, 0.0], spline).assemble_vector(V, 0, n)):
        with pytest.raises(NotImplementedError, match="row blocks"):
            call()
    with monkeypatch.context() as m:
        m.setattr(spline, "_distributed", lambda: True)
        for call in calls:
            with pytest.raises(NotImplementedError, match="ranks"):
                call(spline)
    with monkeypatch.context() as m:
        m.setattr(spline, "_implicit", lambda: True)
        for call in calls:
            with pytest.raises(NotImplementedError, match="row blocks"):
                call(spline)
    with monkeypatch.context() as m:
        m.setattr(spline, "_caller_ordered", lambda: True)
        for call in calls:
            with pytest.raises(NotImplementedError, match="feOrder"):
                call(spline)
    # nF != nsd, nsd != d, fields on other bases, DG, several patches, T-splines
    kv2 = [B.uniformKnots(2, 0.0, 1.0, 3)] * 2
    cm = B.ExplicitBSplineControlMesh([2, 2], kv2)
    one = t.ExtractedSpline(t.EqualOrderSpline(1, cm), 4)
    three = t.ExtractedSpline(t.EqualOrderSpline(3, cm), 4)
    lst = t.ExtractedSpline(t.FieldListSpline(cm, [B.BSpline([2, 2], kv2), B.BSpline([3, 3], [B.uniformKnots(3, 0.0, 1.0, 3)] * 2)]), 4)
    kvd = [0, 0, 0, 0.5, 0.5, 0.5, 1, 1, 1]
    dg = t.ExtractedSpline(t.EqualOrderSpline(2, B.ExplicitBSplineControlMesh([2, 2], [kvd, kvd])), 4)
    surface = t.ExtractedSpline(t.EqualOrderSpline(3, T.N.NURBSControlMesh([2, 2], kvs, np.concatenate([Pf[..., :2], 0.1 * Pf[..., :1] ** 2, Pf[..., 2:]], axis=-1))), 4)
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
    others = [(one, "nFields = 1"), (three, "nFields = 3"), (surface, "nsd = 3"), (lst, "FieldListSpline"), (dg, "DG"),
              (t.ExtractedSpline(BSplineCompat(cm, "RT", [1, 1]), 4), "not supported"),
              (t.ExtractedSpline(t.EqualOrderSpline(2, TwoPatches()), 4), "not supported"),
              (t.ExtractedSpline(t.EqualOrderSpline(2, RhinoTSplineControlMesh(
                  os.path.join(os.path.dirname(__file__), "golden", "tspline_bicubic_patch.iga"))), 4), "not supported")]
    for s, word in others:
        for call in calls:
            with pytest.raises(NotImplementedError, match=word):
                call(s)
