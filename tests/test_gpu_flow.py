"""GPU: first-order system point forms, the element metric and the stabilised incompressible flow on a mapped patch -- the
block ending of k_postproc with b and c per block (``tg_coef_transform_system``), ``tg_assemble_coef_system``, ``tg_quad_metric``,
the law kernel (``tg_flow_points``, csrc/tg_flow.hip) and what is built on them: ``forms.SystemCoefficientForm``,
``SystemLoadForm``, ``SystemResidual``, ``IncompressibleFlow``, ``FlowResidual`` under ``solveNonlinearVariationalProblem``,
``timeIntegration.FlowTransientProblem``.

Measured on the MI355X (``-s`` prints every figure): the largest error / bound over the cases of this file, the Newton
histories and the error norms are in the README section "Incompressible flow".

Reference: tests/flow_reference.py (dense sums over elements, points and local functions with the Cartesian gradients formed
directly; the law is the numpy ``host`` method, pinned by tests/test_flow_reference_host.py).  A, b, c and M of the block tests
are RANDOM per point and not symmetric, so that any mis-numbering of points, blocks or indices shows.

Tolerance: normwise, max |error| / max |reference| against the longdouble run.  The bound of a case is 8 x the error of the
float64 run of the same reference for that case (computed here, on the CPU: no figure of the code under test), and never
below 32 eps -- the rule of tests/test_gpu_coef.py.  Physics: the device flow against the host flow of the same discrete
problem, dofs to 1e-6 of the largest, Newton counts +- 1 -- the convention of tests/test_gpu_hyperelastic.py.
"""
import numpy as np
import pytest

import postproc_reference as R
import coef_reference as CR
import flow_reference as FR

pytestmark = pytest.mark.gpu

EPS = R.EPS
FLOOR = 32 * EPS
LD = CR.LD


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


def _normwise(got, want, want64):
    """(error, bound, float64 error) of ``got`` against the longdouble ``want``: all relative to max |want|"""
    scale = float(np.max(np.abs(want)))
    e64 = float(np.max(np.abs(np.asarray(want64).astype(LD) - want))) / scale
    return float(np.max(np.abs(np.asarray(got).astype(LD) - want))) / scale, max(8.0 * e64, FLOOR), e64


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- patches ------------------------------------------------------------------------------------------------------------------------
def _poly_nodes(nels, p, nsd, weighted=True):
    """non-uniform element vertices and a smooth polynomial map of the Q_p nodes of a d-dimensional grid into nsd >= d
    dimensions (a curve in the plane, a surface in space); ``weighted``: weights varying by a third"""
    d = len(nels)
    rng = np.random.default_rng(7 * d + p + 100 * nsd)
    uks = []
    for k in range(d):
        steps = rng.uniform(0.6, 1.4, nels[k])
        uks.append(np.concatenate([[0.0], np.cumsum(steps) / np.sum(steps) * (1.0 + 0.5 * k)]))
    X = R.lagrange_nodes(uks, p)
    wgt = 1.0 + 0.3 * X[0] * X[-1] + 0.1 * X[0] ** 2 if weighted else np.ones_like(X[0])
    co = [X[i] + 0.1 * X[(i + 1) % d] ** 2 for i in range(d)]
    for i in range(d, nsd):                                              # the directions out of the parameter space
        co.append(0.3 * X[0] ** 2 - 0.2 * X[-1] + 0.1 * X[0] * X[-1])
    return uks, [c * wgt for c in co] + [wgt]


def _annulus_nodes(nels):
    """the exact quarter annulus on nels[0] x nels[1] elements (its homogeneous coordinates are quadratics in the parameters)"""
    uks1, cp1 = R.annulus_patch(1)
    uks = [np.linspace(0.0, 1.0, n + 1) for n in nels]
    X = R.lagrange_nodes(uks, 2)
    l = lambda t: np.stack([2.0 * (t - 0.5) * (t - 1.0), -4.0 * t * (t - 1.0), 2.0 * t * (t - 0.5)])
    L0, L1 = l(X[0]), l(X[1])
    return uks, [np.einsum("an,bn,ab->n", L0, L1, np.asarray(c).reshape(3, 3, order="F")) for c in cp1]


# name -> (p, nq, element vertices, control functions); the 3-D ones with nq = p + 1 at p = 2, 3 take the sum-factorised route
PATCHES = {
    "volume_p2_1x1x1": lambda: (2, None) + R.volume_patch(2, (1, 1, 1)),
    "volume_p2_2x3x2": lambda: (2, None) + R.volume_patch(2, (2, 3, 2)),
    "volume_p3_1x1x1": lambda: (3, None) + R.volume_patch(3, (1, 1, 1)),
    "volume_p3_2x3x2": lambda: (3, None) + R.volume_patch(3, (2, 3, 2)),
    "volume_p3_17x1x2": lambda: (3, None) + R.volume_patch(3, (17, 1, 2)),
    "annulus_3x2": lambda: (2, None) + _annulus_nodes((3, 2)),
    "surface_p2_3x2": lambda: (2, None) + _poly_nodes((3, 2), 2, 3),
    "curve_p3_5": lambda: (3, None) + _poly_nodes((5,), 3, 2),
    "2d_p1_4x3_nq3": lambda: (1, 3) + _poly_nodes((4, 3), 1, 2),
    "2d_p4_2x2_nq3": lambda: (4, 3) + _poly_nodes((2, 2), 4, 2),
    "2d_p3_3x2_nq1": lambda: (3, 1) + _poly_nodes((3, 2), 3, 2),
}
ROUTES = {"default": {}, "short_pieces": {"TIGAR_ASM_CHUNK": "2", "TIGAR_ASM_QUAD_CHUNK": "1"}, "legacy": {"TIGAR_ASM_LEGACY": "1"}}
TERMS = ("A", "b", "c", "M")
_CASE = {}


def _case(name, nF):
    """patch, random point data and the cache of reference matrices: built once, shared by the tests"""
    if (name, nF) not in _CASE:
        p, nq, uks, cp = PATCHES[name]()
        cp = [np.asarray(c, dtype=np.float64) for c in cp]
        d, nsd = len(uks), len(cp) - 1
        npts = int(np.prod([(len(u) - 1) * (p + 1 if nq is None else nq) for u in uks]))
        rng = np.random.default_rng(sum(map(ord, name)) + nF)
        _CASE[(name, nF)] = dict(p=p, nq=nq, uks=uks, cp=cp, d=d, nsd=nsd, npts=npts, nF=nF, want={}, refs={},
                                 A=rng.standard_normal((npts, nF, nsd, nF, nsd)), b=rng.standard_normal((npts, nF, nsd, nF)),
                                 c=rng.standard_normal((npts, nF, nF, nsd)), M=rng.standard_normal((npts, nF, nF)))
    return _CASE[(name, nF)]


def _refs(c, rational):
    if rational not in c["refs"]:
        c["refs"][rational] = [FR.SystemReference(c["uks"], c["p"], c["cp"], c["nF"], c["nq"], rational=rational, dtype=dt)
                               for dt in (LD, np.float64)]
    return c["refs"][rational]


def _reference_matrix(c, rational, terms=TERMS):
    """(keys, longdouble values, float64 values, n) of the form with the given terms"""
    key = (rational, tuple(terms))
    if key not in c["want"]:
        out = [ref.coo(*[c[t] if t in terms else None for t in TERMS]) for ref in _refs(c, rational)]
        assert np.array_equal(out[0][0], out[1][0])
        c["want"][key] = (out[0][0], out[0][1], out[1][1], _refs(c, rational)[0].n)
    return c["want"][key]


_LAYOUT = {"A": (1, 3, 2, 4, 0), "b": (1, 3, 2, 0), "c": (1, 2, 3, 0), "M": (1, 2, 0)}


def _dv(T, name, v):
    """host point data [npts, ...] -> DeviceVector in the device layout of the term"""
    return None if v is None else T.dev.DeviceVector(data=np.ascontiguousarray(np.asarray(v).transpose(_LAYOUT[name])).ravel())


def _gpu_system(T, c, dcp, rational, terms=TERMS, data=None):
    data = c if data is None else data
    args = [_dv(T, t, data[t]) if t in terms else None for t in TERMS]
    coef = T.dev.coef_transform_system(c["uks"], c["p"], dcp, c["nF"], *args, nq=c["nq"], rational=rational)
    return coef, T.dev.assemble_coef_system(c["uks"], c["p"], dcp, c["nF"], coef, nq=c["nq"])


def _check_system(T, name, tag, c, dcp, rational, terms=TERMS):
    keys, want, want64, n = _reference_matrix(c, rational, terms)
    coef, K = _gpu_system(T, c, dcp, rational, terms)
    G = K.to_scipy()
    N = c["nF"] * n
    assert G.shape == (N, N)
    rows = np.repeat(np.arange(N), np.diff(G.indptr))
    at, inside = CR.values_at(keys, want, N, rows, G.indices)
    assert inside, "an entry of the reference lies outside the pattern"
    scale = float(np.max(np.abs(want)))
    e64 = float(np.max(np.abs(want64.astype(LD) - want))) / scale
    bound = max(8.0 * e64, FLOOR)
    err = float(np.max(np.abs(G.data.astype(LD) - at))) / scale
    print("system %-17s nF %d %-12s %s %-7s: error %7.2f eps, float64 reference %6.2f eps, bound %7.2f eps"
          % (name, c["nF"], tag, "rational" if rational else "plain   ", "+".join(terms), err / EPS, e64 / EPS, bound / EPS))
    assert err <= bound
    coef2, K2 = _gpu_system(T, c, dcp, rational, terms)                  # the same bits in a second run of both entry points
    assert _same(coef.get_local(), coef2.get_local()) and _same(G.data, K2.to_scipy().data)
    return coef, G


def _dcp(T, c):
    return [T.dev.DeviceVector(data=v) for v in c["cp"]]


# ---- the system transform and matrix -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nF", [1, 2, 4])
@pytest.mark.parametrize("name", ["volume_p2_1x1x1", "volume_p2_2x3x2", "volume_p3_1x1x1", "volume_p3_2x3x2"])
def test_system_matrix_on_the_rational_volume(T, name, nF):
    """3-D, p = 2, 3, nq = p + 1 (every block from the sum-factorised kernels), one element and 2 x 3 x 2, nF = 1, 2, 4 (nF
    independent of nsd = 3): all four terms, plain and rational"""
    c = _case(name, nF)
    dcp = _dcp(T, c)
    for rational in (False, True):
        _check_system(T, name, "default", c, dcp, rational)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_system_matrix_across_the_seam_on_every_route(T, route, monkeypatch, capfd):
    """17 x 1 x 2 elements at p = 3 (the seam of the default pieces), nF = 2: the default route, short pieces and the plain
    kernel under TIGAR_ASM_LEGACY, each with the functions phi / W_h and phi; the library's timing line of each of the four
    blocks names the route"""
    c = _case("volume_p3_17x1x2", 2)
    dcp = _dcp(T, c)
    for k_, v_ in ROUTES[route].items():
        monkeypatch.setenv(k_, v_)
    monkeypatch.setenv("TIGAR_ASM_TIME", "1")
    capfd.readouterr()
    _gpu_system(T, c, dcp, True)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[tg_assemble]")]
    monkeypatch.delenv("TIGAR_ASM_TIME")
    assert len(lines) == 4, lines
    for ln in lines:
        assert ("(plain)" if route == "legacy" else "point coefficients") in ln and ("sum-factorised" in ln) == (route != "legacy"), lines
    _check_system(T, "volume_p3_17x1x2", route, c, dcp, True)
    _check_system(T, "volume_p3_17x1x2", route, c, dcp, False)            # (the reference of a space is computed once for the three routes)


@pytest.mark.parametrize("rational", [False, True])
@pytest.mark.parametrize("name,nF", [("annulus_3x2", 3), ("surface_p2_3x2", 2), ("curve_p3_5", 2), ("2d_p1_4x3_nq3", 2),
                                     ("2d_p4_2x2_nq3", 2), ("2d_p3_3x2_nq1", 3)])
def test_system_matrix_on_the_plain_kernel(T, name, nF, rational):
    """the quarter annulus with nF = 3, a surface in space (d = 2, nsd = 3), a curve in the plane (d = 1, nsd = 2), p = 1 and
    p = 4 with nq != p + 1, nq = 1"""
    c = _case(name, nF)
    if rational:
        assert np.ptp(c["cp"][-1]) > 0.05                               # the weights do vary
    _check_system(T, name, "plain kernel", c, _dcp(T, c), rational)


@pytest.mark.parametrize("name,nF", [("volume_p2_2x3x2", 2), ("annulus_3x2", 3), ("surface_p2_3x2", 2)])
def test_each_term_alone_and_an_absent_term_is_a_zero_term(T, name, nF):
    c = _case(name, nF)
    dcp = _dcp(T, c)
    for rational in (False, True):
        for t in TERMS:
            _check_system(T, name, "one term", c, dcp, rational, (t,))
        for t in TERMS:                                                  # absent against zero: the same bits
            zero = dict(c)
            zero[t] = np.zeros_like(c[t])
            others = tuple(s for s in TERMS if s != t)
            a, Ka = _gpu_system(T, c, dcp, rational, others)
            b, Kb = _gpu_system(T, c, dcp, rational, TERMS, data=zero)
            assert _same(a.get_local(), b.get_local()) and _same(Ka.to_scipy().data, Kb.to_scipy().data), (name, t, rational)


def test_bit_identities_of_the_block_ending(T):
    """the per-block body is the scalar ending's: (1) without b and c the bits of ``tg_coef_transform_blocks``, (2) with one field
    those of ``tg_coef_transform(a_kind = 2)`` (a_kind = 0 without A), (3) every block of a system those of the scalar
    transform of that block's data"""
    for name, rational in (("annulus_3x2", True), ("volume_p2_2x3x2", False), ("volume_p3_2x3x2", True)):
        d = 2 if name.startswith("annulus") else 3
        c = _case(name, d)
        dcp = _dcp(T, c)
        sys_ = T.dev.coef_transform_system(c["uks"], c["p"], dcp, d, _dv(T, "A", c["A"]), None, None, _dv(T, "M", c["M"]), nq=c["nq"],
                                           rational=rational)
        blk = T.dev.coef_transform_blocks(c["uks"], c["p"], dcp, _dv(T, "A", c["A"]), _dv(T, "M", c["M"]), nq=c["nq"], rational=rational)
        assert _same(sys_.get_local(), blk.get_local()), name
        full = T.dev.coef_transform_system(c["uks"], c["p"], dcp, d, *[_dv(T, t, c[t]) for t in TERMS], nq=c["nq"],
                                           rational=rational).get_local().reshape(d, d, -1)
        col = lambda v: T.dev.DeviceVector(data=np.ascontiguousarray(np.moveaxis(v, 0, -1)).ravel())
        for i in range(d):
            for j in range(d):
                one = T.dev.coef_transform(c["uks"], c["p"], dcp, col(c["A"][:, i, :, j, :]), col(c["b"][:, i, :, j]), col(c["c"][:, i, j, :]),
                                           col(c["M"][:, i, j]), a_kind=2, nq=c["nq"], rational=rational).get_local()
                assert _same(full[i, j], one), (name, i, j)
    for name in ("volume_p2_2x3x2", "surface_p2_3x2", "curve_p3_5"):
        c = _case(name, 1)
        dcp = _dcp(T, c)
        for rational in (False, True):
            for terms in (TERMS, ("b", "c", "M")):
                args = [_dv(T, t, c[t]) if t in terms else None for t in TERMS]
                a = T.dev.coef_transform_system(c["uks"], c["p"], dcp, 1, *args, nq=c["nq"], rational=rational)
                b = T.dev.coef_transform(c["uks"], c["p"], dcp, *args, a_kind=2 if "A" in terms else 0, nq=c["nq"], rational=rational)
                assert _same(a.get_local(), b.get_local()), (name, rational, terms)


def test_block_entries_keep_the_recorded_bits(T):
    """``tg_coef_transform_blocks`` and ``tg_assemble_coef_blocks`` against the commits before the block ending read b and c: the
    SHA-256 of their outputs on the volume cases of tools/point_digest.py, recorded in profiles/point_kernels_digest.jsonl before
    this ending changed, must come out again -- and with them every other volume entry of that record (the scalar transform,
    the loads, the points), which share the kernel"""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import point_digest
    finally:
        sys.path.remove(os.path.join(root, "tools"))
    recorded = {}
    for line in open(os.path.join(root, "profiles", "point_kernels_digest.jsonl")):
        r = json.loads(line)
        if r["face"] is None:
            recorded[(r["entry"], r["case"], r["rational"])] = r["sha256"]
    got = {}
    for name in point_digest.VOLUME_CASES:
        point_digest.volume(name, lambda entry, case, rational, face, digest: got.__setitem__((entry, case, rational), digest))
    assert sorted(got) == sorted(recorded)
    blocks = [k for k in got if k[0] in ("coef_transform_blocks", "assemble_coef_blocks")]
    assert len(blocks) == 24
    for k in blocks:
        assert got[k] == recorded[k], k
    assert [k for k in got if got[k] != recorded[k]] == []


def test_system_entries_refuse_bad_arguments(T):
    c = _case("annulus_3x2", 2)
    dcp = _dcp(T, c)
    npts = c["npts"]
    for bad in (lambda: T.dev.coef_transform_system(c["uks"], c["p"], dcp, 0),
                lambda: T.dev.coef_transform_system(c["uks"], c["p"], dcp, 17),
                lambda: T.dev.coef_transform_system(c["uks"], c["p"], dcp, 2, b=T.dev.DeviceVector(4 * 2 * npts + 1)),
                lambda: T.dev.coef_transform_system(c["uks"], c["p"], dcp, 2, A=T.dev.DeviceVector(4 * 2 * npts)),
                lambda: T.dev.assemble_coef_system(c["uks"], c["p"], dcp, 2, T.dev.DeviceVector(4 * 9 * npts + 4)),
                lambda: T.dev.assemble_coef_system(c["uks"], c["p"], dcp, 3, T.dev.DeviceVector(4 * 9 * npts)),
                lambda: T.dev._point_call("tg_quad_metric", c["uks"], c["p"], dcp, None, T.dev.DeviceVector(3 * npts))):
        with pytest.raises(T.dev.TigarHipError):
            bad()


# ---- the element metric ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATCHES))
def test_metric_matches_the_jacobian(T, name):
    c = _case(name, 1)
    want, want64 = [FR.metric(c["uks"], c["p"], c["cp"], c["nq"], dt) for dt in (LD, np.float64)]
    G = T.dev.quad_metric(c["uks"], c["p"], _dcp(T, c), nq=c["nq"])
    got = G.get_local().reshape(c["nsd"], c["nsd"], c["npts"]).transpose(2, 0, 1)
    err, bound, e64 = _normwise(got, want, want64)
    print("metric %-17s: error %6.2f eps, float64 reference %6.2f eps, bound %6.2f eps" % (name, err / EPS, e64 / EPS, bound / EPS))
    assert err <= bound
    assert _same(got, got.transpose(0, 2, 1))                            # symmetric to the bit
    assert _same(G.get_local(), T.dev.quad_metric(c["uks"], c["p"], _dcp(T, c), nq=c["nq"]).get_local())


@pytest.mark.parametrize("d", [2, 3])
def test_metric_of_an_affine_box(T, d):
    """x_k = s_k xi_k on non-uniform elements: G = 4 diag(1 / (h_k s_k)^2) at every point of the element, to rounding"""
    p, scale = 2, [1.5, 0.5, 3.0][:d]
    uks = [np.array([0.0, 0.3, 1.0]), np.array([0.0, 0.5, 0.75, 1.0]), np.array([0.0, 1.0])][:d]
    X = R.lagrange_nodes(uks, p)
    cp = [scale[k] * X[k] for k in range(d)] + [np.ones_like(X[0])]
    G = T.dev.quad_metric(uks, p, [T.dev.DeviceVector(data=np.ascontiguousarray(v)) for v in cp])
    nel = [len(u) - 1 for u in uks]
    nqt = (p + 1) ** d
    got = G.get_local().reshape(d, d, -1, nqt)                           # [K][L][element][point]
    for e, el in enumerate(np.ndindex(*nel[::-1])):
        h = [uks[k][el[::-1][k] + 1] - uks[k][el[::-1][k]] for k in range(d)]
        want = np.diag([4.0 / (h[k] * scale[k]) ** 2 for k in range(d)])
        assert np.max(np.abs(got[:, :, e, :] - want[:, :, None])) <= 64 * EPS * np.max(want)


def test_metric_is_cached_on_the_points(T):
    gen = _annulus_gen(T, 2, 3)
    pts = T.F.quadrature_points(gen, gen.V_control)
    assert pts.metric is pts.metric and pts.metric.size() == 4 * pts.npts


# ---- the law kernel ----------------------------------------------------------------------------------------------------------------
def _law_state(nsd, npts, seed, zero_u=False):
    rng = np.random.default_rng(seed)
    nF = nsd + 1
    U, gU = rng.standard_normal((npts, nF)), rng.standard_normal((npts, nF, nsd))
    if zero_u:
        U[:, :nsd] = 0.0
    B = rng.standard_normal((npts, nsd, nsd))
    G = 4.0 * (np.einsum("qab,qcb->qac", B, B) + np.eye(nsd))           # symmetric positive definite, as a metric is
    return U, gU, G, rng.standard_normal((npts, nsd)), rng.standard_normal((npts, nsd))


def _law_on_device(T, law, nsd, U, gU, G, a0, f, c_a, dt4, want=(True,) * 7):
    up = lambda v: None if v is None else T.dev.DeviceVector(data=np.ascontiguousarray(np.moveaxis(v, 0, -1)).ravel())
    return T.dev.flow_points(law.params(c_a, dt4), nsd, up(U), up(gU), up(G), up(a0), up(f), want=want)


def _law_arrays(out, nsd, npts):
    """the seven outputs of ``flow_points`` in the shapes of ``IncompressibleFlow.host``"""
    nF = nsd + 1
    s, F, A, b, c, M, t = [None if v is None else v.get_local() for v in out]
    sh = lambda v, shape, perm: None if v is None else v.reshape(tuple(shape) + (npts,)).transpose(perm)
    return (sh(s, (nF,), (1, 0)), sh(F, (nF, nsd), (2, 0, 1)), sh(A, (nF, nF, nsd, nsd), (4, 0, 2, 1, 3)), sh(b, (nF, nF, nsd), (3, 0, 2, 1)),
            sh(c, (nF, nF, nsd), (3, 0, 1, 2)), sh(M, (nF, nF), (2, 0, 1)), sh(t, (2,), (1, 0)))


@pytest.mark.parametrize("variant", ["steady", "transient"])
@pytest.mark.parametrize("nsd", [2, 3])
def test_flow_points_match_the_host_law(T, nsd, variant):
    """1000 random points (four workgroups, the last one partly filled): the seven outputs against the longdouble law, steady
    without a0 and f and transient with both and the 4 / dt^2 term; every subset of outputs gives the same bits, and so does a
    second run"""
    npts = 1000
    law = T.F.IncompressibleFlow(1.3, 0.2)
    U, gU, G, a0, f = _law_state(nsd, npts, 10 * nsd + len(variant))
    c_a, dt4 = (0.0, 0.0) if variant == "steady" else (1.7, 4.0 / 0.125 ** 2)
    if variant == "steady":
        a0 = f = None
    ld = lambda v: None if v is None else v.astype(LD)
    want = law.host(ld(U), ld(gU), ld(G), c_a=c_a, a0=ld(a0), f=ld(f), dt4=dt4)
    want64 = law.host(U, gU, G, c_a=c_a, a0=a0, f=f, dt4=dt4)
    full = _law_on_device(T, law, nsd, U, gU, G, a0, f, c_a, dt4)
    for name, g, w, w64 in zip(("s", "F", "A", "b", "c", "M", "tau"), _law_arrays(full, nsd, npts), want, want64):
        err, bound, e64 = _normwise(g, w, w64)
        print("flow law nsd %d %-9s %-3s: error %6.2f eps, float64 law %6.2f eps, bound %6.2f eps" % (nsd, variant, name, err / EPS, e64 / EPS, bound / EPS))
        assert err <= bound
    bits = [v.get_local() for v in full]
    for mask in range(1, 128):
        on = tuple(bool(mask >> k & 1) for k in range(7))
        part = _law_on_device(T, law, nsd, U, gU, G, a0, f, c_a, dt4, want=on)
        for k in range(7):
            assert (part[k] is None) == (not on[k]) and (part[k] is None or _same(part[k].get_local(), bits[k])), (mask, k)


@pytest.mark.parametrize("nsd", [2, 3])
def test_flow_points_at_rest(T, nsd):
    """u = 0: everything finite, tau_M = (4 / dt^2 + C_I nu^2 G:G)^(-1/2), steady and transient"""
    npts = 257
    law = T.F.IncompressibleFlow(2.0, 0.3, C_I=36.0)
    U, gU, G, a0, f = _law_state(nsd, npts, 3, zero_u=True)
    for dt4 in (0.0, 64.0):
        out = _law_arrays(_law_on_device(T, law, nsd, U, gU, G, None, f, 0.0, dt4), nsd, npts)
        assert all(np.all(np.isfinite(v)) for v in out)
        tM = (dt4 + 36.0 * (0.3 / 2.0) ** 2 * np.einsum("qKL,qKL->q", G, G)) ** -0.5
        assert np.max(np.abs(out[6][:, 0] - tM)) <= 8 * EPS * np.max(tM)
        assert np.max(np.abs(out[6][:, 1] * tM * np.einsum("qKK->q", G) - 1.0)) <= 16 * EPS


def test_flow_points_refuse_bad_arguments(T):
    law = T.F.IncompressibleFlow(1.0, 0.1)
    U, gU, G, a0, f = _law_state(2, 10, 1)
    D = T.dev.DeviceVector
    for bad in (lambda: T.dev.flow_points(law.params(), 4, D(50), D(200), D(160)),
                lambda: T.dev.flow_points(law.params(), 2, D(30), D(60), D(41)),
                lambda: T.dev.flow_points((0.0, 0.1, 0.0, 0.0, 36.0), 2, D(30), D(60), D(40)),
                lambda: T.dev.flow_points((1.0, -0.1, 0.0, 0.0, 36.0), 2, D(30), D(60), D(40)),
                lambda: T.dev.flow_points(law.params(), 2, D(30), D(60), D(40), a0=D(21))):
        with pytest.raises(T.dev.TigarHipError):
            bad()
    with pytest.raises(ValueError):
        T.dev.flow_points((1.0, 0.1), 2, D(30), D(60), D(40))
    for bad in (lambda: T.F.IncompressibleFlow(0.0, 0.1), lambda: T.F.IncompressibleFlow(1.0, -0.1)):
        with pytest.raises(ValueError):
            bad()


# ---- generators for the forms ----------------------------------------------------------------------------------------------------
def _annulus_gen(T, nel, fields):
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    return T.t.EqualOrderSpline(fields, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf))


def _volume_gen(T, p, nels, fields):
    from geom_util import rational_volume
    kvs, C = rational_volume(p, nels)
    return T.t.EqualOrderSpline(fields, T.N.NURBSControlMesh([p] * 3, kvs, C))


def _patch_of(gen):
    g = gen.V.grids[0]
    return ([np.asarray(g.vertices[k], dtype=np.float64) for k in range(g.dim())], int(g.degree),
            [f.vector().get_local() for f in gen.cpFuncs])


def _function(T, V, values):
    u = T.t.Function(V)
    u.vector().set_local(np.asarray(values, dtype=np.float64))
    return u


# ---- the forms -----------------------------------------------------------------------------------------------------------------------
def test_system_forms_match_the_reference_and_flag_symmetry(T):
    """``SystemCoefficientForm`` / ``SystemLoadForm`` on the annulus with nF = 3: arrays, callables and DeviceVectors give the
    matrix of the reference; ``symmetric`` true and false, down to one bit in b against c"""
    F = T.F
    gen = _annulus_gen(T, 2, 3)
    uks, p, cp = _patch_of(gen)
    nF, nsd = 3, 2
    refs = [FR.SystemReference(uks, p, cp, nF, rational=True, dtype=dt) for dt in (LD, np.float64)]
    npts, n = refs[0].npts, refs[0].n
    rng = np.random.default_rng(4)
    A, b, c, M = (rng.standard_normal((npts, nF, nsd, nF, nsd)), rng.standard_normal((npts, nF, nsd, nF)),
                  rng.standard_normal((npts, nF, nF, nsd)), rng.standard_normal((npts, nF, nF)))
    want, want64 = [r.dense(A, b, c, M) for r in refs]
    for form in (F.SystemCoefficientForm(gen, A, b, c, M, rational=True),
                 F.SystemCoefficientForm(gen, lambda x: A, lambda x: b, lambda x: c, lambda x: M, rational=True),
                 F.SystemCoefficientForm(gen, _dv(T, "A", A), _dv(T, "b", b), _dv(T, "c", c), _dv(T, "M", M), rational=True)):
        K = form.assemble_matrix(gen.V).to_scipy()
        err, bound, e64 = _normwise(K.toarray(), want, want64)
        print("SystemCoefficientForm annulus nF 3: error %6.2f eps, float64 reference %6.2f eps, bound %6.2f eps" % (err / EPS, e64 / EPS, bound / EPS))
        assert err <= bound and form.symmetric is False
        B = form.assemble_block(gen.V, 2, 1).to_scipy()
        assert abs(B - K[2 * n:, n:2 * n]).max() == 0.0
    S, Ms = A + A.transpose(0, 3, 4, 1, 2), M + M.transpose(0, 2, 1)
    cs = b.transpose(0, 3, 1, 2).copy()                                  # c[j, i, K] = b[i, K, j]
    off = cs.copy()
    off[0, 1, 0, 1] = np.nextafter(off[0, 1, 0, 1], np.inf)              # one bit in one entry
    yes = [F.SystemCoefficientForm(gen, S), F.SystemCoefficientForm(gen, S, b, cs, Ms), F.SystemCoefficientForm(gen, None, b, cs),
           F.SystemCoefficientForm(gen, _dv(T, "A", S), _dv(T, "b", b), _dv(T, "c", cs), _dv(T, "M", Ms)), F.SystemCoefficientForm(gen, reaction=Ms)]
    no = [F.SystemCoefficientForm(gen, A), F.SystemCoefficientForm(gen, S, b, off, Ms), F.SystemCoefficientForm(gen, S, b, None, Ms),
          F.SystemCoefficientForm(gen, S, b, cs, M), F.SystemCoefficientForm(gen, _dv(T, "A", S), _dv(T, "b", b), _dv(T, "c", off))]
    assert all(f.symmetric is True for f in yes) and all(f.symmetric is False for f in no)
    K = yes[1].assemble_matrix(gen.V).to_scipy()
    assert abs(K - K.T).max() <= 64 * EPS * abs(K).max()
    s, Fx = rng.standard_normal((npts, nF)), rng.standard_normal((npts, nF, nsd))
    got = F.SystemLoadForm(s, gen, flux=Fx, rational=True).assemble_vector(gen.V).get_local()
    err, bound, _ = _normwise(got, refs[0].load(s, Fx), refs[1].load(s, Fx))
    assert err <= bound


@pytest.mark.parametrize("geometry,rational", [("annulus", True), ("annulus", False), ("volume", True), ("volume", False)])
def test_flow_residual_and_tangent_match_the_reference(T, geometry, rational):
    """``FlowResidual`` at a random state with a body force, an acceleration history and the 4 / dt^2 term, on 2 x 3 x 2 elements of
    the rational volume (p = 2, nF = 4) and on the annulus (nF = 3): vector and matrix of the device law and of the same law
    through ``host`` against the reference; twice the same bits; ``symmetric`` False"""
    gen = _annulus_gen(T, 3, 3) if geometry == "annulus" else _volume_gen(T, 2, (2, 3, 2), 4)
    uks, p, cp = _patch_of(gen)
    ref, ref64 = [FR.FlowReference(uks, p, cp, rational=rational, dtype=dt) for dt in (LD, np.float64)]
    nF, n, nsd, npts = ref.nF, ref.n, ref.nsd, ref.npts
    rng = np.random.default_rng(5)
    un = 0.3 * rng.standard_normal(nF * n)
    u = _function(T, gen.V, un)
    body = lambda x: np.stack([np.sin(x[:, 0]), x[:, 1] ** 2, np.cos(x[:, -1])], axis=1)[:, :nsd]
    a0 = rng.standard_normal((npts, nsd))
    kw = dict(c_a=1.7, a0=a0, f=body(ref.x.astype(np.float64)), dt4=4.0 / 0.25 ** 2)
    law = T.F.IncompressibleFlow(1.3, 0.2)

    class HostLaw(object):
        def host(self, *a, **k):
            return law.host(*a, **k)
    wr, wr64, wk, wk64 = ref.residual(un, law, **kw), ref64.residual(un, law, **kw), ref.tangent(un, law, **kw), ref64.tangent(un, law, **kw)
    for which, lw in (("device", law), ("host", HostLaw())):
        res = T.F.FlowResidual(u, gen, lw, body_force=body, rational=rational)
        res.c_a, res.dt4 = kw["c_a"], kw["dt4"]
        res.a0 = T.dev.DeviceVector(data=np.ascontiguousarray(a0.T).ravel())
        assert res.device_law is (which == "device")
        r = res.assemble_vector(gen.V).get_local()
        err, bound, e64 = _normwise(r, wr, wr64)
        print("flow residual %-8s %-6s %s: error %6.2f eps, float64 reference %6.2f eps, bound %6.2f eps"
              % (geometry, which, "rational" if rational else "plain   ", err / EPS, e64 / EPS, bound / EPS))
        assert err <= bound
        tan = res.tangent()
        assert tan.symmetric is False
        K = tan.assemble_matrix(gen.V).to_scipy()
        err, bound, e64 = _normwise(K.toarray(), wk, wk64)
        print("flow tangent  %-8s %-6s %s: error %6.2f eps, float64 reference %6.2f eps, bound %6.2f eps"
              % (geometry, which, "rational" if rational else "plain   ", err / EPS, e64 / EPS, bound / EPS))
        assert err <= bound
        assert _same(r, res.assemble_vector(gen.V).get_local()) and _same(K.data, tan.assemble_matrix(gen.V).to_scipy().data)
        B = tan.assemble_block(gen.V, nF - 1, 0).to_scipy()
        assert abs(B - K[(nF - 1) * n:, :n]).max() == 0.0


def test_system_residual_of_a_linear_law(T):
    """a law linear in (U, grad U): R(U) = J U - load to rounding, and the tangent is the ``SystemCoefficientForm`` of its data"""
    gen = _annulus_gen(T, 2, 2)
    nF, nsd = 2, 2
    pts = T.F.quadrature_points(gen, gen.V_control)
    npts = pts.npts
    rng = np.random.default_rng(8)
    A, b, c, M = (rng.standard_normal((npts, nF, nsd, nF, nsd)), rng.standard_normal((npts, nF, nsd, nF)),
                  rng.standard_normal((npts, nF, nF, nsd)), rng.standard_normal((npts, nF, nF)))
    f = rng.standard_normal((npts, nF))
    residual = lambda x, U, G: (np.einsum("qiKjL,qjL->qiK", A, G) + np.einsum("qiKj,qj->qiK", b, U),
                                np.einsum("qijL,qjL->qi", c, G) + np.einsum("qij,qj->qi", M, U))
    un = rng.standard_normal(nF * gen.V.grids[0].num_nodes())
    u = _function(T, gen.V, un)
    res = T.F.SystemResidual(u, gen, residual, lambda x, U, G: (A, b, c, M), f=f, rational=True)
    r = res.assemble_vector(gen.V).get_local()
    tan = res.tangent()
    K = tan.assemble_matrix(gen.V).to_scipy()
    load = T.F.SystemLoadForm(f, gen, rational=True).assemble_vector(gen.V).get_local()
    want = K @ un - load
    # every entry of K u is a sum of at most (2 p + 1)^2 nF products, each with the error of K's entries (bounded above by the
    # rule of this file at 32 eps of the largest) and one rounding of its own
    terms = 25 * nF
    assert np.max(np.abs(r - want)) <= terms * 40 * EPS * abs(K).max() * np.max(np.abs(un))
    assert tan.symmetric is False
    Kf = T.F.SystemCoefficientForm(gen, A, b, c, M, rational=True).assemble_matrix(gen.V).to_scipy()
    assert _same(K.data, Kf.data)
    with pytest.raises(ValueError, match="returns"):
        T.F.SystemResidual(u, gen, lambda x, U, G: None, lambda x, U, G: (A, b, c, M)).assemble_vector(gen.V)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(T):
    F = T.F
    gen3 = _annulus_gen(T, 2, 3)
    gen2 = _annulus_gen(T, 2, 2)
    law = F.IncompressibleFlow(1.0, 0.1)
    u2, u3 = T.t.Function(gen2.V), T.t.Function(gen3.V)
    npts = F.quadrature_points(gen3, gen3.V_control).npts
    with pytest.raises(NotImplementedError, match="nsd \\+ 1 = 3 fields"):
        F.FlowResidual(u2, gen2, law).assemble_vector(gen2.V)
    p = 2
    line = T.t.EqualOrderSpline(2, T.B.ExplicitBSplineControlMesh([p], [T.B.uniformKnots(p, 0., 1., 3)]))
    with pytest.raises(NotImplementedError, match="nsd = d = 2 or 3"):
        F.FlowResidual(T.t.Function(line.V), line, law).assemble_vector(line.V)
    with pytest.raises(ValueError, match="unknown material"):
        F.FlowResidual(u3, gen3, object())
    for bad in (lambda: F.SystemCoefficientForm(None), lambda: F.SystemLoadForm(1.0, None), lambda: F.SystemLoadForm(None, gen3),
                lambda: F.SystemResidual(u3, None, None, None), lambda: F.FlowResidual(u3, None, law),
                lambda: F.SystemCoefficientForm(gen3, np.zeros((npts, 3, 2, 3, 3))).assemble_matrix(gen3.V),
                lambda: F.SystemCoefficientForm(gen3, reaction=np.zeros((npts + 1, 3, 3))).assemble_matrix(gen3.V),
                lambda: F.SystemCoefficientForm(gen3, reaction=T.dev.DeviceVector(9 * npts + 1)).assemble_matrix(gen3.V),
                lambda: F.SystemCoefficientForm(gen3, reaction=np.eye(3), nq=99).assemble_matrix(gen3.V),
                lambda: F.SystemCoefficientForm(gen3, reaction=np.eye(3)).assemble_block(gen3.V, 3, 0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError, match="row"):
        F.SystemCoefficientForm(gen3, reaction=np.eye(3)).assemble_matrix(gen3.V, 0, 5)

    class BadLaw(object):
        def host(self, *a, **k):
            return (1, 2)
    with pytest.raises(ValueError, match="returns"):
        F.FlowResidual(u3, gen3, BadLaw()).assemble_vector(gen3.V)
    # NotImplementedError: several ranks, the streamed engine, the caller's dof order; other spaces
    t, B = T.t, T.B
    spline = t.ExtractedSpline(gen3, 4)
    V, us = spline.V, t.Function(spline.V)
    calls = [lambda s: F.SystemCoefficientForm(s, reaction=np.eye(len(s.V.grids))).assemble_matrix(s.V),
             lambda s: F.SystemLoadForm(np.ones(len(s.V.grids)), s).assemble_vector(s.V),
             lambda s: F.SystemResidual(t.Function(s.V), s, lambda x, U, G: (None, U), lambda x, U, G: (None,) * 4).assemble_vector(s.V),
             lambda s: F.FlowResidual(t.Function(s.V), s, law).assemble_vector(s.V),
             lambda s: F.FlowResidual(t.Function(s.V), s, law).tangent().assemble_matrix(s.V)]
    for call in calls:
        call(spline)                                                       # (they do run on the space they are made for)
    for attr, word in (("_distributed", "ranks"), ("_implicit", "row blocks"), ("_caller_ordered", "feOrder")):
        with pytest.MonkeyPatch.context() as m:
            m.setattr(spline, attr, lambda: True)
            for call in calls:
                with pytest.raises(NotImplementedError, match=word):
                    call(spline)
    kv2 = [B.uniformKnots(2, 0.0, 1.0, 3)] * 2
    cm = B.ExplicitBSplineControlMesh([2, 2], kv2)
    lst = t.ExtractedSpline(t.FieldListSpline(cm, [B.BSpline([2, 2], kv2), B.BSpline([3, 3], [B.uniformKnots(3, 0.0, 1.0, 3)] * 2)]), 4)
    kvd = [0, 0, 0, 0.5, 0.5, 0.5, 1, 1, 1]
    dg = t.ExtractedSpline(t.EqualOrderSpline(3, B.ExplicitBSplineControlMesh([2, 2], [kvd, kvd])), 4)
    from tigar_amd.compatibleSplines import BSplineCompat
    from tigar_amd.RhinoTSplines import RhinoTSplineControlMesh
    import os
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
    tsp = RhinoTSplineControlMesh(os.path.join(os.path.dirname(__file__), "golden", "tspline_bicubic_patch.iga"))
    for s, word in ((lst, "FieldListSpline"), (dg, "DG"), (t.ExtractedSpline(BSplineCompat(cm, "RT", [1, 1]), 4), "not supported"),
                    (t.ExtractedSpline(t.EqualOrderSpline(3, TwoPatches()), 4), "not supported"),
                    (t.ExtractedSpline(t.EqualOrderSpline(3, tsp), 4), "not supported")):
        for call in calls:
            with pytest.raises(NotImplementedError, match=word):
                call(s)


# ---- physics ---------------------------------------------------------------------------------------------------------------------------
def _tg_spline(T, pb):
    gen = T.t.EqualOrderSpline(3, T.N.NURBSControlMesh([2, 2], pb["kvs"], pb["C"]))
    sp0 = gen.getScalarSpline(0)
    for k in range(2):                                                    # direction 0 runs along y: the normal velocity on the
        for side in (0, 1):                                               # sides of direction k is field 1 - k
            gen.addZeroDofs(1 - k, sp0.getSideDofs(k, side))
    gen.addZeroDofs(2, [0])                                               # one pressure dof pinned
    spline = T.t.ExtractedSpline(gen, 4)
    spline.setSolverOptions(linearSolver=T.t.PETScLUSolver(), relativeTolerance=FR.NEWTON_TOL, maxIters=12)
    return gen, spline


_TG_ERRORS = {}


@pytest.mark.parametrize("nel", [4, 8, 16])
def test_steady_taylor_green(T, nel, capsys):
    """the vortex u = (sin x cos y, -cos x sin y) held steady by f = 2 nu u on the distorted quadratic square [-pi, pi]^2, rho = 1,
    mu = 0.1, p = 2: Newton from zero reaches 1e-9 in the iteration count of the host flow +- 1, the last two steps of order
    >= 1.5, the dofs of the host flow to 1e-6 of the largest and its velocity L2 errors (``errorNorm``, field by field) to 1e-6 relative; from
    8^2 to 16^2 elements the errors fall by >= 3 (order >= 1.5 where 2 is expected: the viscous part of the strong residual
    is left out)"""
    pb, law, Uh, hhist, herr = FR.host_taylor_green(nel)
    gen, spline = _tg_spline(T, pb)
    u = T.t.Function(spline.V)
    U = T.dev.DeviceVector(data=pb["U0"])
    res = T.F.FlowResidual(u, spline, law, body_force=FR.tg_force, rational=True)
    hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u, igaDoFs=U)
    Ud = U.get_local()
    rel = np.max(np.abs(Ud - Uh)) / np.max(np.abs(Uh))
    # ``errorNorm`` serves scalar spaces: each velocity field is handed, as a nodal vector, to the scalar spline of the same mesh
    n = gen.V.grids[0].num_nodes()
    one = T.t.ExtractedSpline(T.t.EqualOrderSpline(1, T.N.NURBSControlMesh([2, 2], pb["kvs"], pb["C"])), 4)
    errs = []
    for i in range(2):
        ui = T.dev.DeviceVector(data=u.vector().get_local()[i * n:(i + 1) * n])
        errs.append(one.errorNorm(ui, lambda x, i=i: FR.tg_velocity(x)[:, i], "L2", rational=True))
    _TG_ERRORS[nel] = errs
    with capsys.disabled():
        print("taylor-green %2d^2: device %d iterations (host %d), dofs differ by %.2e of the largest, L2 errors %.4e %.4e (host %.4e %.4e); "
              "history %s" % (nel, len(hist), len(hhist), rel, errs[0], errs[1], herr[0], herr[1], " ".join("%.1e" % v for v in hist)))
    assert abs(len(hist) - len(hhist)) <= 1
    assert rel <= 1e-6
    q = [np.log(hist[k + 1]) / np.log(hist[k]) for k in (-3, -2)]
    assert min(q) >= 1.5, q
    assert all(abs(e - h) <= 1e-6 * h for e, h in zip(errs, herr))
    if nel == 16:
        coarse = _TG_ERRORS.get(8) or FR.host_taylor_green(8)[4]
        assert all(c / e >= 3.0 for c, e in zip(coarse, errs)), (coarse, errs)


def test_flow_newton_in_three_dimensions(T, capsys):
    """the rational volume on 2 x 2 x 2 elements, p = 2, nF = 4, all velocity dofs of the boundary held at zero and one pressure dof
    pinned, driven by a body force: one Newton solve with the default direct solver; the residual drops as in the host flow"""
    from geom_util import rational_volume
    from oracle import tigar_oracle as O
    p = 2
    kvs, C = rational_volume(p, (2, 2, 2))
    gen = T.t.EqualOrderSpline(4, T.N.NURBSControlMesh([p] * 3, kvs, C))
    sp0 = gen.getScalarSpline(0)
    ncp = sp0.getNcp()
    fixed = []
    for f in range(3):
        for k in range(3):
            for side in (0, 1):
                dofs = sp0.getSideDofs(k, side)
                gen.addZeroDofs(f, dofs)
                fixed += [f * ncp + int(i) for i in dofs]
    gen.addZeroDofs(3, [0])
    fixed.append(3 * ncp)
    spline = T.t.ExtractedSpline(gen, 2 * p)
    spline.setSolverOptions(relativeTolerance=FR.NEWTON_TOL, maxIters=12)
    law = T.F.IncompressibleFlow(1.0, 0.05)
    body = lambda x: np.stack([np.sin(3.0 * x[:, 1]), x[:, 2] * x[:, 0], np.cos(2.0 * x[:, 0])], axis=1)
    uks, pp, cp = _patch_of(gen)
    ref = FR.FlowReference(uks, pp, cp, rational=True, dtype=np.float64)
    s = O.BSpline([p] * 3, [list(k) for k in kvs])
    Mc = O.generate_M_tensor(s, nfields=4)
    free = np.setdiff1d(np.arange(4 * ncp), np.unique(fixed))
    Uh, hhist = FR.newton(ref, Mc, free, law, np.zeros(4 * ncp), f=body(ref.x), tol=FR.NEWTON_TOL)
    u = T.t.Function(spline.V)
    U = T.dev.DeviceVector(data=np.zeros(4 * ncp))
    res = T.F.FlowResidual(u, spline, law, body_force=body, rational=True)
    hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u, igaDoFs=U)
    rel = np.max(np.abs(U.get_local() - Uh)) / np.max(np.abs(Uh))
    with capsys.disabled():
        print("flow 3-D: device %d iterations (host %d), dofs differ by %.2e of the largest; device history %s, host history %s"
              % (len(hist), len(hhist), rel, " ".join("%.1e" % v for v in hist), " ".join("%.1e" % v for v in hhist)))
    assert abs(len(hist) - len(hhist)) <= 1 and rel <= 1e-6
    assert all(abs(np.log10(a) - np.log10(b)) <= 1.0 for a, b in zip(hist[:-1], hhist[:-1]))


# ---- time stepping -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["generalized_alpha", "backward_euler"])
def test_transient_taylor_green(T, scheme, capsys):
    """the vortex without a body force on 8^2 elements, dt = 1/8, four steps: initial data by ``projectDofs`` of the exact fields
    (field by field on the scalar spline of the same mesh), the rates of the exact decay.  After EVERY step the state equals
    the host flow's (the same scheme written out in tests/flow_reference.py, from the same initial dofs) to 1e-6 of the
    largest dof, with its Newton counts +- 1; the amplitude int u_h . u_0 / int u_0 . u_0 follows exp(-2 nu t) to within the host
    flow's own distance from it (plus 1e-6)"""
    from tigar_amd import timeIntegration as TI
    pb = FR.taylor_green_problem(8)
    gen, spline = _tg_spline(T, pb)
    one = T.t.ExtractedSpline(T.t.EqualOrderSpline(1, T.N.NURBSControlMesh([2, 2], pb["kvs"], pb["C"])), 4)
    one.setSolverOptions(linearSolver=T.t.PETScLUSolver())
    fields = [lambda x: FR.tg_velocity(x)[:, 0], lambda x: FR.tg_velocity(x)[:, 1], FR.tg_pressure]
    U0 = np.concatenate([one.projectDofs(f, rational=True).get_local() for f in fields])
    pb, law, U0, V0, ref = FR.transient_taylor_green_data(U0)
    states, rates, hhist = FR.time_stepping(ref, pb["Mc"], pb["free"], law, U0, V0, FR.TG_DT, 4, scheme=scheme)
    u = T.t.Function(spline.V)
    flow = T.F.FlowResidual(u, spline, law, rational=True)
    prob = TI.FlowTransientProblem(spline, flow, FR.TG_DT, scheme=scheme, RHO_INF=0.5, x0=T.dev.DeviceVector(data=U0),
                                   xdot0=T.dev.DeviceVector(data=V0))
    assert prob.t == 0.0 and prob.x.vector().size() == spline.V.dim()
    Mc = pb["Mc"].tocsr() if hasattr(pb["Mc"], "tocsr") else pb["Mc"]
    for k in range(4):
        prob.step()
        t = FR.TG_DT * (k + 1)
        assert abs(prob.t - t) <= 1e-14 and prob.steps_done == k + 1
        got, want = prob.x.vector().get_local(), np.asarray(Mc @ states[k]).ravel()
        rel = np.max(np.abs(got - want)) / np.max(np.abs(want))
        rel_rate = np.max(np.abs(prob.xdot.vector().get_local() - np.asarray(Mc @ rates[k]).ravel())) / np.max(np.abs(Mc @ rates[k]))
        amp, amph, exact = FR.amplitude(ref, got), FR.amplitude(ref, want), np.exp(-2.0 * FR.TG_MU / FR.TG_RHO * t)
        with capsys.disabled():
            print("transient %-17s step %d: %d Newton steps (host %d), state differs by %.2e, rate by %.2e; amplitude %.6f (host %.6f, "
                  "exp(-2 nu t) %.6f)" % (scheme, k + 1, prob.last["iterations"], len(hhist[k]) - 1, rel, rel_rate, amp, amph, exact))
        assert abs(prob.last["iterations"] - (len(hhist[k]) - 1)) <= 1
        assert rel <= 1e-6 and rel_rate <= 1e-5                          # (the rate divides the state's difference by gamma dt)
        assert abs(amp - exact) <= abs(amph - exact) + 1e-6


def test_flow_transient_problem_refusals(T, monkeypatch):
    from tigar_amd import timeIntegration as TI
    pb = FR.taylor_green_problem(4)
    gen, spline = _tg_spline(T, pb)
    law = T.F.IncompressibleFlow(1.0, 0.1)
    flow = T.F.FlowResidual(T.t.Function(spline.V), spline, law, rational=True)
    for bad in (dict(scheme="newmark"), dict(DELTA_T=0.0), dict(RHO_INF=1.5), dict(absoluteTolerance=-1.0), dict(x0=[1.0, 2.0, 3.0]),
                dict(x0=T.dev.DeviceVector(5))):
        kw = dict(DELTA_T=0.1)
        kw.update(bad)
        with pytest.raises(ValueError):
            TI.FlowTransientProblem(spline, flow, **kw)
    with pytest.raises(NotImplementedError, match="FlowResidual"):
        TI.FlowTransientProblem(spline, T.F.SystemLoadForm(np.ones(3), spline), 0.1)
    for attr, word in (("_distributed", "ranks"), ("_caller_ordered", "feOrder")):
        with monkeypatch.context() as m:
            m.setattr(spline, attr, lambda: True)
            with pytest.raises(NotImplementedError, match=word):
                TI.FlowTransientProblem(spline, flow, 0.1)
