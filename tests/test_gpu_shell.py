"""GPU: Kirchhoff-Love shells -- the law kernel ``tg_shell_points`` (csrc/tg_shell.hip) and ``forms.ShellResidual`` on the
second-derivative point forms (csrc/tg_jet.hip), with the device law and with the same law on the host (``device_law=False``).

Reference: tests/shell_reference.py on tests/jet_reference.py (dense loops per element and point; jets formed directly; the
energy as the reference's demo writes it); the law is ``forms.KirchhoffLoveSVK.host`` in the reference's precision, pinned by
tests/test_jet_reference_host.py.

Tolerance: normwise, max |error| / max |reference| against the longdouble run; the bound of a case is 8 x the error of the
float64 run of the same reference for that case, never below 32 eps (the rule of tests/test_gpu_coef.py and
tests/test_gpu_hyperelastic.py).  Newton: the bounds of tests/test_gpu_hyperelastic.py -- dofs to relative 1e-6, the step count
+- 1, the last two steps of order >= 1.5.  ``-s`` prints every figure; the largest are in the README section "Kirchhoff-Love
shells".
"""
import json
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
    ns.mat = forms.KirchhoffLoveSVK(SR.E_MOD, SR.NU, SR.THICKNESS)
    return ns


def _hold(label, got, want, w64):
    want = np.asarray(want)
    scale = float(np.max(np.abs(want)))
    e64 = float(np.max(np.abs(np.asarray(w64).astype(LD) - want))) / scale
    bound = max(8.0 * e64, FLOOR)
    err = float(np.max(np.abs(np.asarray(got).astype(LD) - want))) / scale
    print("%-62s error %.2e  float64 reference %.2e  bound %.2e" % (label, err, e64, bound))
    assert err <= bound, (label, err, bound)
    return bound


SURFACES = {"cylinder": (SR.cylinder_homogeneous(), True), "curved": (SR.doubly_curved_homogeneous, False)}
STATES = [("cylinder", 2, (2, 3)), ("cylinder", 3, (5, 4)), ("curved", 3, (2, 3)), ("curved", 2, (5, 4))]
_SETUP = {}


def _setup(T, surface, p, nels):
    """the spline, the reference objects and a random state of a tenth of the thickness' order: built once"""
    key = (surface, p, nels)
    if key not in _SETUP:
        hom, rational = SURFACES[surface]
        pb = SR.problem(p, nels, hom)
        gen = T.t.EqualOrderSpline(3, T.N.NURBSControlMesh([p, p], pb["kvs"], pb["C"]))
        spline = T.t.ExtractedSpline(gen, 2 * p)
        ref, r64 = (SR.ShellReference(pb["uks"], p, pb["cp"], rational=rational, dtype=dt) for dt in (LD, np.float64))
        un = 0.02 * np.random.default_rng(p + sum(nels)).standard_normal(3 * ref.n)
        want = {"R": (ref.residual(un, T.mat), r64.residual(un, T.mat)), "K": (ref.tangent(un, T.mat), r64.tangent(un, T.mat)),
                "E": (ref.law_energy(un, T.mat), r64.law_energy(un, T.mat))}
        _SETUP[key] = dict(pb=pb, spline=spline, rational=rational, ref=ref, r64=r64, un=un, want=want)
    return _SETUP[key]


@pytest.mark.parametrize("device_law", [True, False], ids=["device_law", "host_law"])
@pytest.mark.parametrize("surface,p,nels", STATES)
def test_residual_tangent_and_energy_at_a_random_state(T, surface, p, nels, device_law):
    c = _setup(T, surface, p, nels)
    spline, V = c["spline"], c["spline"].V
    u = T.t.Function(V)
    u.vector().set_local(c["un"])
    res = T.F.ShellResidual(u, spline, T.mat, rational=c["rational"], device_law=device_law)
    assert res.device_law is device_law
    tag = "%s p=%d %dx%d %s" % (surface, p, nels[0], nels[1], "device" if device_law else "host")
    _hold(tag + ": residual", res.assemble_vector(V).get_local(), *c["want"]["R"])
    tan = res.tangent()
    assert tan.symmetric is True
    K = tan.assemble_matrix(V).to_scipy().toarray()
    bound = _hold(tag + ": tangent", K, *c["want"]["K"])
    # K - K^T to rounding: K and K^T both lie within the bound of the symmetric reference
    asym = float(np.max(np.abs(K - K.T))) / float(np.max(np.abs(K)))
    print("%-62s |K - K^T| / max|K| %.2e" % (tag, asym))
    assert asym <= 2 * bound
    _hold(tag + ": energy", np.array([res.energy(V)]), np.array([c["want"]["E"][0]]), np.array([c["want"]["E"][1]]))


def _random_jets(npts, seed):
    """reference jets of a surface close to a stretched plane with curvature, displacement jets of a tenth of that: the
    normals stay away from degeneracy (|X_,1 x X_,2| >= 0.1)"""
    rng = np.random.default_rng(seed)
    X = 0.15 * rng.uniform(-1, 1, (npts, 3, 6))
    X[:, 0, 1] += 1.0
    X[:, 1, 2] += 1.2
    U = 0.05 * rng.uniform(-1, 1, (npts, 3, 6))
    return X, U


def _to_device(T, J):
    return T.dev.DeviceVector(data=np.ascontiguousarray(J.transpose(1, 2, 0)).ravel())


def test_law_kernel_on_random_jets(T):
    """the kernel alone on 1000 random jets against ``KirchhoffLoveSVK.host`` in longdouble; an absent optional output against
    a present one and two runs: the same bits"""
    npts = 1000
    X, U = _random_jets(npts, 21)
    psi, s, Tq = T.mat.host(X.astype(LD), U.astype(LD))
    p64, s64, T64 = T.mat.host(X, U)
    Xd, Ud = _to_device(T, X), _to_device(T, U)
    sd, Td, pd, nbad = T.dev.shell_points(0, T.mat.E, T.mat.nu, T.mat.thickness, Xd, Ud, True, True, True)
    assert nbad == 0
    _hold("law kernel: psi", pd.get_local(), psi, p64)
    _hold("law kernel: s", sd.get_local().reshape(3, 6, npts).transpose(2, 0, 1), s, s64)
    _hold("law kernel: T", Td.get_local().reshape(3, 3, 6, 6, npts).transpose(4, 0, 2, 1, 3), Tq, T64)
    bits = lambda v: v.get_local().view(np.int64)
    for mask in range(1, 8):
        so, To, po, nb = T.dev.shell_points(0, T.mat.E, T.mat.nu, T.mat.thickness, Xd, Ud, bool(mask & 1), bool(mask & 2), bool(mask & 4))
        assert nb == 0 and (so is None) == (not mask & 1) and (To is None) == (not mask & 2) and (po is None) == (not mask & 4)
        for got, full in ((so, sd), (To, Td), (po, pd)):
            if got is not None:
                assert np.array_equal(bits(got), bits(full)), mask


def test_degenerate_points_are_counted_and_raise(T):
    """three points whose current tangents coincide: the kernel counts them and writes nothing there; ``ShellResidual`` raises a
    Python error naming three points, with the device law and with the host law"""
    npts = 300
    X, U = _random_jets(npts, 22)
    bad = (0, 137, 299)
    for q in bad:
        U[q, :, 2] = X[q, :, 1] + U[q, :, 1] - X[q, :, 2]           # x_,1 = x_,0
    Xd, Ud = _to_device(T, X), _to_device(T, U)
    sd, Td, pd, nbad = T.dev.shell_points(0, T.mat.E, T.mat.nu, T.mat.thickness, Xd, Ud, True, True, True)
    assert nbad == 3
    c = _setup(T, "curved", 3, (2, 3))
    spline, V = c["spline"], c["spline"].V
    for device_law in (True, False):
        res = T.F.ShellResidual(T.t.Function(V), spline, T.mat, device_law=device_law)
        pts, g, Xj, Uj = res.jets(V)
        n = pts.npts
        Xh, Uh = _random_jets(n, 23)
        for q in (1, n // 2, n - 1):
            Uh[q, :, 2] = Xh[q, :, 1] + Uh[q, :, 1] - Xh[q, :, 2]
        res.jets = lambda V_, a=_to_device(T, Xh), b=_to_device(T, Uh): (pts, g, a, b)
        with pytest.raises(RuntimeError, match="3 quadrature points"):
            res.assemble_vector(V)
        with pytest.raises(RuntimeError, match="3 quadrature points"):
            res.tangent().assemble_matrix(V)


def _rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@pytest.mark.parametrize("p", [2, 3])
def test_rigid_motion_in_the_rational_space(T, p):
    """u = (R - I) x + c on the cylinder is in the rational space (nodal values W_a ((R - I) x_a + c)): residual rows and energy
    are rounding errors.  Yardstick (tests/shell_reference.py ``magnitudes``): row i, a is held relative to
    sum_q wdet sum_alpha |s|^alpha |J^alpha psi_a| with |s| the sizes of the terms that cancel in s; the float64 host reference's
    largest figure is measured here on the CPU and the device held to 8 x it.  The energy is quadratic in the rounding error
    of the strains: the square root of energy / sum wdet |psi| is held to 8 x the float64 reference's."""
    c = _setup(T, "cylinder", p, (2, 3) if p == 2 else (5, 4))
    pb, spline, V = c["pb"], c["spline"], c["spline"].V
    cp = [np.asarray(v) for v in pb["cp"]]
    x = np.stack([cp[i] / cp[3] for i in range(3)], axis=1)
    un = (cp[3][:, None] * (x @ (_rotation((1.0, 2.0, -0.5), 0.9) - np.eye(3)).T + np.array([0.3, -1.0, 2.0]))).T.ravel()
    rows, emag = c["ref"].magnitude(un, T.mat)
    host_rows = float(np.max(np.abs(c["r64"].residual(un, T.mat)).astype(LD) / rows))
    host_energy = float(np.sqrt(abs(c["r64"].law_energy(un, T.mat)) / emag))
    u = T.t.Function(V)
    u.vector().set_local(un)
    for device_law in (True, False):
        res = T.F.ShellResidual(u, spline, T.mat, rational=True, device_law=device_law)
        got_rows = float(np.max(np.abs(res.assemble_vector(V).get_local()).astype(LD) / rows))
        got_energy = float(np.sqrt(abs(res.energy(V)) / emag))
        print("rigid motion p=%d %-6s: rows %.2e (float64 host reference %.2e), sqrt(energy) %.2e (float64 host reference %.2e)"
              % (p, "device" if device_law else "host", got_rows, host_rows, got_energy, host_energy))
        assert got_rows <= 8 * host_rows
        assert got_energy <= 8 * host_energy


def _clamped_spline(T, pb, held_sides, layers):
    p = pb["p"]
    gen = T.t.EqualOrderSpline(3, T.N.NURBSControlMesh([p, p], pb["kvs"], pb["C"]))
    sp0 = gen.getScalarSpline(0)
    for f in range(3):
        for direction, side in held_sides:
            gen.addZeroDofs(f, sp0.getSideDofs(direction, side, nLayers=layers))
    spline = T.t.ExtractedSpline(gen, 2 * p)
    spline.setSolverOptions(linearSolver=T.t.PETScLUSolver(), relativeTolerance=SR.NEWTON_TOL, maxIters=12)
    return spline


@pytest.mark.parametrize("p", [2, 3])
def test_newton_flow_of_the_clamped_strip(T, p, capsys):
    """quarter-cylinder strip, 4 x 4 elements, two rows of control points clamped on the straight edge, body force: the device
    flow (device law, default direct solver, tolerance 1e-9, no line search) takes the step count of the dense host flow +- 1,
    ends at its dofs to relative 1e-6, and its last two steps are of order >= 1.5"""
    pb, Uh, hhist = SR.strip_flow(p, T.mat)
    assert len(hhist) <= 8
    spline = _clamped_spline(T, pb, [(1, 0)], 2)
    u = T.t.Function(spline.V)
    U = T.dev.DeviceVector(data=np.zeros(3 * pb["ncp"]))
    res = T.F.ShellResidual(u, spline, T.mat, body_force=SR.STRIP_LOAD, rational=True)
    hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u, igaDoFs=U)
    Ud = U.get_local()
    rel = np.max(np.abs(Ud - Uh)) / np.max(np.abs(Uh))
    with capsys.disabled():
        print("strip p=%d: device %d iterations (host %d), dofs differ by %.2e of the largest; device history %s"
              % (p, len(hist), len(hhist), rel, " ".join("%.1e" % v for v in hist)))
    assert abs(len(hist) - len(hhist)) <= 1
    assert rel <= 1e-6
    q = [np.log(hist[k + 1]) / np.log(hist[k]) for k in (-3, -2)]
    assert min(q) >= 1.5, q
    assert res.energy(spline.V) > 0.0


@pytest.mark.parametrize("nel", [4, 8, 16])
def test_plate_bending_reproduces_the_host_deflections(T, nel, capsys):
    """flat square, simply supported, sinusoidal load with w / h = 1e-4, p = 3: the centre deflection of the device flow equals
    that of the dense host flow (tests/golden/shell_plate.json, recorded from tests/shell_reference.py on the CPU; the flow of
    nel = 4 is run again here) to relative 1e-6.  The host flow's errors against Navier's q / (D pi^4 (a^-2 + b^-2)^2) and
    their ratios are in the README."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "shell_plate.json")) as f:
        rec = json.load(f)
    mat = T.F.KirchhoffLoveSVK(SR.PLATE_E, SR.PLATE_NU, SR.PLATE_H)
    pb = SR.plate_problem(nel)
    want = rec["host_flow"][str(nel)]["centre_deflection"]
    assert abs(rec["exact"] - SR.plate_exact_centre(SR.plate_load_amplitude())) <= 4 * EPS * rec["exact"]
    if nel == 4:
        ref = SR.ShellReference(pb["uks"], 3, pb["cp"], dtype=np.float64)
        Uh, _ = SR.newton(ref, pb["Mc"], pb["free"], mat, np.zeros(3 * pb["ncp"]), f=SR.plate_force(ref.x), tol=SR.NEWTON_TOL)
        assert abs(SR.centre_deflection(pb, Uh) - want) <= 1e-9 * abs(want)
    spline = _clamped_spline(T, pb, [(0, 0), (0, 1), (1, 0), (1, 1)], 1)
    u = T.t.Function(spline.V)
    U = T.dev.DeviceVector(data=np.zeros(3 * pb["ncp"]))
    res = T.F.ShellResidual(u, spline, mat, body_force=SR.plate_force)
    hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u, igaDoFs=U)
    w = SR.centre_deflection(pb, U.get_local())
    with capsys.disabled():
        print("plate nel=%d: centre deflection %.12e (host flow %.12e, relative difference %.2e; Navier %.12e, error %.2e), %d steps"
              % (nel, w, want, abs(w - want) / abs(want), rec["exact"], abs(w - rec["exact"]) / rec["exact"], len(hist)))
    assert abs(w - want) <= 1e-6 * abs(want)


def test_refuses_what_is_no_shell(T):
    """a plane patch (nsd = 2), one field, an unknown material, no geometry"""
    F, t, B = T.F, T.t, T.B
    kv = [B.uniformKnots(2, 0.0, 1.0, 2)] * 2
    plane = t.ExtractedSpline(t.EqualOrderSpline(3, B.ExplicitBSplineControlMesh([2, 2], kv)), 4)
    with pytest.raises(NotImplementedError, match="surface in space"):
        F.ShellResidual(t.Function(plane.V), plane, T.mat).assemble_vector(plane.V)
    c = _setup(T, "curved", 3, (2, 3))
    kvs, C = c["pb"]["kvs"], c["pb"]["C"]
    one = t.ExtractedSpline(t.EqualOrderSpline(1, T.N.NURBSControlMesh([3, 3], kvs, C)), 6)
    with pytest.raises(NotImplementedError, match="three fields"):
        F.ShellResidual(t.Function(one.V), one, T.mat).tangent().assemble_matrix(one.V)
    spline = c["spline"]
    for bad in ("svk", object(), 3):
        with pytest.raises(ValueError, match="unknown material"):
            F.ShellResidual(t.Function(spline.V), spline, bad)
    with pytest.raises(ValueError, match="geometry"):
        F.ShellResidual(t.Function(spline.V), None, T.mat)
    with pytest.raises(NotImplementedError, match="row blocks"):
        F.ShellResidual(t.Function(spline.V), spline, T.mat).assemble_vector(spline.V, 0, 5)
    with pytest.raises(T.dev.TigarHipError):
        T.dev.shell_points(1, 1.0, 0.3, 0.1, T.dev.DeviceVector(18), T.dev.DeviceVector(18))
