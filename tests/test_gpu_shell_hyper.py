"""GPU: the hyperelastic Kirchhoff-Love shell -- kind 1 of ``tg_shell_points`` and the follower pressure
``tg_shell_pressure_points`` (csrc/tg_shell.hip), ``forms.KirchhoffLoveHyper`` and ``forms.ShellResidual(pressure=...)`` with
the device law and with the same law on the host (``device_law=False``).

Reference: tests/shell_hyper_reference.py on tests/shell_reference.py; the law is ``forms.KirchhoffLoveHyper.host`` in the
reference's precision, pinned against the energy as the reference's demo writes it by
tests/test_shell_hyper_reference_host.py; the pressure is written there directly from -P sqrt(det a / det A) a_3.

Tolerance: the rule of tests/test_gpu_shell.py, unchanged -- normwise, max |error| / max |reference| against the longdouble
run; the bound of a case is 8 x the error of the float64 run of the same reference for that case, never below 32 eps.  Newton:
dofs to relative 1e-6, the step count +- 1.  ``-s`` prints every figure; the largest are in the README section
"Kirchhoff-Love shells".
"""
import json
import os

import numpy as np
import pytest

import shell_reference as SR
import shell_hyper_reference as HR
from test_gpu_shell import FLOOR, LD, STATES, SURFACES, _hold, _random_jets, _rotation, _to_device

pytestmark = pytest.mark.gpu

LAW_THICKNESS = 0.5          # the thickest shell the random jets admit: the reference keeps det Gm, det C_2D >= 0.73
STATE_THICKNESS = 0.05
STATE_AMPLITUDE = 0.005      # nodal noise of a tenth of the thickness: on the four patches the reference keeps det C_2D >= 0.31
PRESSURE = 100.0             # of the size of the membrane forces at the random states (4 mu h eps ~ 200)


@pytest.fixture(scope="module")
def T():
    import tigar_amd
    from tigar_amd import BSplines, forms, device, NURBS
    from tigar_amd.timeIntegration import LoadStepper
    device.device_info()

    class NS:
        pass
    ns = NS()
    ns.t, ns.B, ns.F, ns.dev, ns.N, ns.LoadStepper = tigar_amd, BSplines, forms, device, NURBS, LoadStepper
    ns.mat = forms.KirchhoffLoveHyper(HR.MU, STATE_THICKNESS)
    ns.svk = forms.KirchhoffLoveSVK(SR.E_MOD, SR.NU, SR.THICKNESS)
    return ns


def _unpack(npts, s, Tq, psi):
    return (psi.get_local(), s.get_local().reshape(3, 6, npts).transpose(2, 0, 1),
            Tq.get_local().reshape(3, 3, 6, 6, npts).transpose(4, 0, 2, 1, 3))


@pytest.mark.parametrize("nth", [1, 4])
@pytest.mark.parametrize("npts", [1, 63, 255, 256, 257, 1000])
def test_law_kernel_on_random_jets(T, npts, nth):
    """the kernel alone against ``KirchhoffLoveHyper.host`` in longdouble; every subset of outputs and a second run: the
    same bits"""
    law = T.F.KirchhoffLoveHyper(HR.MU, LAW_THICKNESS, nth)
    X, U = _random_jets(npts, 21)
    psi, s, Tq = law.host(X.astype(LD), U.astype(LD))
    p64, s64, T64 = law.host(X, U)
    Xd, Ud = _to_device(T, X), _to_device(T, U)
    sd, Td, pd, nbad = T.dev.shell_law_points(1, law.params(), Xd, Ud, True, True, True)
    assert nbad == 0
    gp, gs, gT = _unpack(npts, sd, Td, pd)
    tag = "law kernel npts=%d n_thickness=%d: " % (npts, nth)
    _hold(tag + "psi", gp, psi, p64)
    _hold(tag + "s", gs, s, s64)
    _hold(tag + "T", gT, Tq, T64)
    assert not np.any(gs[:, :, 0]) and not np.any(gT[:, :, 0]) and not np.any(gT[:, :, :, :, 0])          # the value slots
    bits = lambda v: v.get_local().view(np.int64)
    for mask in range(1, 9):            # (8: the full call once more)
        m = 7 if mask == 8 else mask
        so, To, po, nb = T.dev.shell_law_points(1, law.params(), Xd, Ud, bool(m & 1), bool(m & 2), bool(m & 4))
        assert nb == 0 and (so is None) == (not m & 1) and (To is None) == (not m & 2) and (po is None) == (not m & 4)
        for got, full in ((so, sd), (To, Td), (po, pd)):
            if got is not None:
                assert np.array_equal(bits(got), bits(full)), mask


def test_pressure_kernel_adds_to_the_outputs(T):
    """``tg_shell_pressure_points`` on random jets: what it adds to s and T is the reference's pressure load and tangent; s
    alone and T alone get the same bits as together; nothing outside the (value | value, first-derivative) entries changes"""
    for npts in (1, 257, 1000):
        X, U = _random_jets(npts, 24)
        sr, Tr = HR.pressure_load(PRESSURE, X.astype(LD), U.astype(LD))
        s64, T64 = HR.pressure_load(PRESSURE, X, U)
        Xd, Ud = _to_device(T, X), _to_device(T, U)
        base_s, base_T = np.arange(18 * npts, dtype=np.float64), -np.arange(324 * npts, dtype=np.float64)
        sd, Td = T.dev.DeviceVector(data=base_s), T.dev.DeviceVector(data=base_T)
        T.dev.shell_pressure_points(PRESSURE, Xd, Ud, sd, Td)
        ds = (sd.get_local() - base_s).reshape(3, 6, npts).transpose(2, 0, 1)
        dT = (Td.get_local() - base_T).reshape(3, 3, 6, 6, npts).transpose(4, 0, 2, 1, 3)
        assert not np.any(ds[:, :, 1:]) and not np.any(dT[:, :, 1:]) and not np.any(dT[:, :, 0, :, 0]) and not np.any(dT[:, :, 0, :, 3:])
        # the sums base + load round at the size of base: compare the kernel run on zeros
        s0, T0 = T.dev.DeviceVector(18 * npts), T.dev.DeviceVector(324 * npts)
        T.dev.shell_pressure_points(PRESSURE, Xd, Ud, s0, T0)
        _hold("pressure kernel npts=%d: s" % npts, s0.get_local().reshape(3, 6, npts).transpose(2, 0, 1), sr, s64)
        _hold("pressure kernel npts=%d: T" % npts, T0.get_local().reshape(3, 3, 6, 6, npts).transpose(4, 0, 2, 1, 3), Tr, T64)
        s1, T1 = T.dev.DeviceVector(18 * npts), T.dev.DeviceVector(324 * npts)
        T.dev.shell_pressure_points(PRESSURE, Xd, Ud, s1, None)
        T.dev.shell_pressure_points(PRESSURE, Xd, Ud, None, T1)
        assert np.array_equal(s1.get_local().view(np.int64), s0.get_local().view(np.int64))
        assert np.array_equal(T1.get_local().view(np.int64), T0.get_local().view(np.int64))


def _spoil(X, U, points, how):
    for q in points:
        if how == "tangents":
            U[q, :, 2] = X[q, :, 1] + U[q, :, 1] - X[q, :, 2]           # x_,1 = x_,0
        else:
            HR.make_inadmissible(X, U, q)                               # det C_2D <= 0 at the outer thickness points


@pytest.mark.parametrize("how", ["tangents", "det_C2D"])
def test_inadmissible_points_are_counted_and_raise(T, how):
    """the first, the middle and the last of 300 points with coincident current tangents, or with a displacement jet that
    makes det C_2D <= 0: the kernel counts them and writes nothing there; ``ShellResidual`` raises a Python error naming three
    points, with the device law and with the host law"""
    law = T.F.KirchhoffLoveHyper(HR.MU, LAW_THICKNESS)
    npts = 300
    X, U = _random_jets(npts, 22)
    bad = (0, 150, 299)
    _spoil(X, U, bad, how)
    assert list(np.nonzero(law.degenerate(X, U))[0]) == list(bad)
    if how == "det_C2D":
        assert not np.any(T.F.KirchhoffLoveSVK.degenerate(X, U))
    Xd, Ud = _to_device(T, X), _to_device(T, U)
    mark = 12345.0
    sd, Td, pd = (T.dev.DeviceVector(data=np.full(n * npts, mark)) for n in (18, 324, 1))
    nbad = T.dev.C.c_int64(0)
    par = np.array(law.params())
    T.dev.check(T.dev._lib.lib().tg_shell_points(1, par.ctypes.data_as(T.dev.c_f64p), npts, Xd._h, Ud._h, sd._h, Td._h, pd._h,
                                                 T.dev.C.byref(nbad)), "tg_shell_points")
    assert nbad.value == 3
    gp, gs, gT = _unpack(npts, sd, Td, pd)
    good = np.setdiff1d(np.arange(npts), bad)
    assert np.all(gp[list(bad)] == mark) and np.all(gs[list(bad)] == mark) and np.all(gT[list(bad)] == mark)
    assert not np.any(gp[good] == mark) and not np.any(gT[good][:, :, 1, :, 1] == mark)
    c = _setup(T, "curved", 3, (2, 3))
    spline, V = c["spline"], c["spline"].V
    for device_law in (True, False):
        res = T.F.ShellResidual(T.t.Function(V), spline, law, device_law=device_law)
        pts, g, Xj, Uj = res.jets(V)
        n = pts.npts
        Xh, Uh = _random_jets(n, 23)
        _spoil(Xh, Uh, (0, n // 2, n - 1), how)
        res.jets = lambda V_, a=_to_device(T, Xh), b=_to_device(T, Uh): (pts, g, a, b)
        with pytest.raises(RuntimeError, match="3 quadrature points"):
            res.assemble_vector(V)
        with pytest.raises(RuntimeError, match="3 quadrature points"):
            res.tangent().assemble_matrix(V)


_SETUP = {}


def _setup(T, surface, p, nels):
    """the spline, the reference objects, a random state of a tenth of the thickness' order and what the reference gives
    there in longdouble and in float64 -- the law's residual, tangent and energy, and the pressure's parts: built once"""
    key = (surface, p, nels)
    if key not in _SETUP:
        hom, rational = SURFACES[surface]
        pb = SR.problem(p, nels, hom)
        gen = T.t.EqualOrderSpline(3, T.N.NURBSControlMesh([p, p], pb["kvs"], pb["C"]))
        spline = T.t.ExtractedSpline(gen, 2 * p)
        refs = [HR.HyperShellReference(pb["uks"], p, pb["cp"], rational=rational, dtype=dt) for dt in (LD, np.float64)]
        un = STATE_AMPLITUDE * np.random.default_rng(p + sum(nels)).standard_normal(3 * refs[0].n)
        want = {k: [] for k in ("R", "K", "E", "Rp", "Kp")}
        for r in refs:
            psi, s, Tq = r.state(un, T.mat)
            sp, Tp = HR.pressure_load(PRESSURE, *r.jets(un))
            want["R"].append(r.ref.load(s))
            want["K"].append(r.ref.matrix(Tq))
            want["E"].append(np.sum(r.ref.wdet * psi))
            want["Rp"].append(r.ref.load(sp))
            want["Kp"].append(r.ref.matrix(Tp))
        _SETUP[key] = dict(pb=pb, spline=spline, rational=rational, ref=refs[0], r64=refs[1], un=un, want=want)
    return _SETUP[key]


@pytest.mark.parametrize("device_law", [True, False], ids=["device_law", "host_law"])
@pytest.mark.parametrize("surface,p,nels", STATES)
def test_residual_tangent_and_energy_at_a_random_state(T, surface, p, nels, device_law):
    """without a pressure: residual, tangent (symmetric: K - K^T within 2 x its bound) and energy; with one: residual and
    tangent against the reference's sums, ``symmetric`` False, the energy still the strain energy"""
    c = _setup(T, surface, p, nels)
    spline, V, w = c["spline"], c["spline"].V, c["want"]
    u = T.t.Function(V)
    u.vector().set_local(c["un"])
    res = T.F.ShellResidual(u, spline, T.mat, rational=c["rational"], device_law=device_law)
    assert res.device_law is device_law and res.builtin is True
    tag = "%s p=%d %dx%d %s" % (surface, p, nels[0], nels[1], "device" if device_law else "host")
    _hold(tag + ": residual", res.assemble_vector(V).get_local(), *w["R"])
    tan = res.tangent()
    assert tan.symmetric is True
    K = tan.assemble_matrix(V).to_scipy().toarray()
    bound = _hold(tag + ": tangent", K, *w["K"])
    asym = float(np.max(np.abs(K - K.T))) / float(np.max(np.abs(K)))
    print("%-62s |K - K^T| / max|K| %.2e" % (tag, asym))
    assert asym <= 2 * bound
    _hold(tag + ": energy", np.array([res.energy(V)]), np.array([w["E"][0]]), np.array([w["E"][1]]))
    stepper = T.LoadStepper(0.5)                                   # t = 0.5 now: the pressure is read at assembly time
    resp = T.F.ShellResidual(u, spline, T.mat, rational=c["rational"], device_law=device_law, pressure=lambda: 2 * PRESSURE * stepper.t)
    _hold(tag + ": residual with pressure", resp.assemble_vector(V).get_local(), w["R"][0] + w["Rp"][0], w["R"][1] + w["Rp"][1])
    tanp = resp.tangent()
    assert tanp.symmetric is False
    Kp = tanp.assemble_matrix(V).to_scipy().toarray()
    _hold(tag + ": tangent with pressure", Kp, w["K"][0] + w["Kp"][0], w["K"][1] + w["Kp"][1])
    assert tanp.symmetric is False
    assert float(np.max(np.abs(Kp - Kp.T))) > 1e-6 * float(np.max(np.abs(Kp)))
    assert resp.energy(V) == res.energy(V)
    stepper.advance()                                              # t = 1: twice the pressure, the law's part unchanged
    _hold(tag + ": residual at the next load step", resp.assemble_vector(V).get_local(), w["R"][0] + 2 * w["Rp"][0],
          w["R"][1] + 2 * w["Rp"][1])


@pytest.mark.parametrize("device_law", [True, False], ids=["device_law", "host_law"])
def test_pressure_with_the_st_venant_kirchhoff_law(T, device_law):
    """the follower pressure (a number) beside ``KirchhoffLoveSVK`` on the cylinder"""
    surface, p, nels = STATES[0]
    c = _setup(T, surface, p, nels)
    spline, V, w = c["spline"], c["spline"].V, c["want"]
    u = T.t.Function(V)
    u.vector().set_local(c["un"])
    R, K = [], []
    for r in (c["ref"], c["r64"]):
        _, s, Tq = r.state(c["un"], T.svk)
        R.append(r.ref.load(s))
        K.append(r.ref.matrix(Tq))
    res = T.F.ShellResidual(u, spline, T.svk, rational=c["rational"], device_law=device_law, pressure=PRESSURE)
    _hold("svk + pressure: residual", res.assemble_vector(V).get_local(), R[0] + w["Rp"][0], R[1] + w["Rp"][1])
    tan = res.tangent()
    assert tan.symmetric is False
    _hold("svk + pressure: tangent", tan.assemble_matrix(V).to_scipy().toarray(), K[0] + w["Kp"][0], K[1] + w["Kp"][1])
    assert T.F.ShellResidual(u, spline, T.svk, rational=c["rational"], device_law=device_law).tangent().symmetric is True


@pytest.mark.parametrize("p", [2, 3])
def test_rigid_motion_in_the_rational_space(T, p):
    """u = (R - I) x + c on the cylinder is in the rational space (nodal values W_a ((R - I) x_a + c)): the residual is a
    rounding error.  Yardstick: the largest residual entry at the random state of the same patch.  The float64 host
    reference's figure is measured here on the CPU and the device held to 8 x it, never below 32 eps.  Measured on the CPU:
    float64 host reference 1.33e-14 (p = 2, 2 x 3 elements) and 2.38e-14 (p = 3, 5 x 4 elements) of the largest entry (the
    nodal values of the rigid motion are float64 data: the longdouble reference itself stays at 9.2e-15 and 1.4e-14)."""
    c = _setup(T, "cylinder", p, (2, 3) if p == 2 else (5, 4))
    pb, spline, V = c["pb"], c["spline"], c["spline"].V
    cp = [np.asarray(v) for v in pb["cp"]]
    x = np.stack([cp[i] / cp[3] for i in range(3)], axis=1)
    un = (cp[3][:, None] * (x @ (_rotation((1.0, 2.0, -0.5), 0.9) - np.eye(3)).T + np.array([0.3, -1.0, 2.0]))).T.ravel()
    scale = float(np.max(np.abs(c["want"]["R"][0])))
    host = float(np.max(np.abs(c["r64"].residual(un, T.mat)))) / scale
    bound = max(8 * host, FLOOR)
    u = T.t.Function(V)
    u.vector().set_local(un)
    for device_law in (True, False):
        res = T.F.ShellResidual(u, spline, T.mat, rational=True, device_law=device_law)
        got = float(np.max(np.abs(res.assemble_vector(V).get_local()))) / scale
        print("rigid motion p=%d %-6s: residual / largest entry at the random state %.2e (float64 host reference %.2e, bound %.2e)"
              % (p, "device" if device_law else "host", got, host, bound))
        assert got <= bound


@pytest.mark.parametrize("p", [2, 3])
def test_inflation_of_the_clamped_square(T, p, capsys):
    """the demo's flow (demos/kl-shell-hyper/kl-hyper.py): the square [-1, 1]^2 as an explicit B-spline in space, two rows of
    control points clamped on every edge, mu = 1e4, h = 0.03, a follower pressure raised by a ``LoadStepper`` in three steps.
    Element count and final pressure per degree were chosen on the CPU (tests/shell_hyper_reference.py ``INFLATION``; the
    dense host flow is recorded in tests/golden/shell_hyper_inflation.json, 2 s and 25 s): every load step converges in at
    most 8 Newton steps at tolerance 1e-9, the centre ends 3.02 h above the plane.  The device flow (device law, default
    direct solver, no line search) reproduces the dofs of every load step to relative 1e-6 and the step counts to +- 1."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "shell_hyper_inflation.json")) as f:
        rec = json.load(f)["flows"][str(p)]
    nel, P, nsteps = HR.INFLATION[p]["nel"], HR.INFLATION[p]["pressure"], HR.INFLATION_STEPS
    assert (rec["nel"], rec["pressure"]) == (nel, P)
    t, B, F = T.t, T.B, T.F
    mesh = B.ExplicitBSplineControlMesh([p, p], [B.uniformKnots(p, -1., 1., nel)] * 2, extraDim=1)
    gen = t.EqualOrderSpline(3, mesh)
    sc = gen.getControlMesh().getScalarSpline()
    for side in (0, 1):
        for direction in (0, 1):
            for i in range(3):
                gen.addZeroDofs(i, sc.getSideDofs(direction, side, nLayers=2))
    spline = t.ExtractedSpline(gen, 2 * p)
    spline.setSolverOptions(maxIters=12, relativeTolerance=HR.NEWTON_TOL)
    u = t.Function(spline.V)
    stepper = T.LoadStepper(1.0 / nsteps)
    res = F.ShellResidual(u, spline, F.KirchhoffLoveHyper(HR.MU, HR.THICKNESS), pressure=lambda: P * stepper.t)
    U = T.dev.DeviceVector(data=np.zeros(len(rec["dofs"][0])))
    lines = []
    for k in range(nsteps):
        hist = spline.solveNonlinearVariationalProblem(res, res.tangent(), u, igaDoFs=U)
        stepper.advance()
        want, hhist = np.array(rec["dofs"][k]), rec["histories"][k]
        rel = float(np.max(np.abs(U.get_local() - want))) / float(np.max(np.abs(want)))
        lines.append("inflation p=%d load step %d: device %d iterations (host %d), dofs differ by %.2e of the largest; device "
                     "history %s" % (p, k + 1, len(hist), len(hhist), rel, " ".join("%.1e" % v for v in hist)))
        assert abs(len(hist) - len(hhist)) <= 1, lines
        assert rel <= 1e-6, lines
    with capsys.disabled():
        print("\n".join(lines))
    assert res.tangent().symmetric is False and res.energy(spline.V) > 0.0


def test_refuses_what_is_no_hyperelastic_shell(T):
    """a plane patch (nsd = 2), one field, five thickness points, row blocks, an unknown material"""
    F, t, B = T.F, T.t, T.B
    kv = [B.uniformKnots(2, 0.0, 1.0, 2)] * 2
    plane = t.ExtractedSpline(t.EqualOrderSpline(3, B.ExplicitBSplineControlMesh([2, 2], kv)), 4)
    with pytest.raises(NotImplementedError, match="surface in space"):
        F.ShellResidual(t.Function(plane.V), plane, T.mat, pressure=1.0).assemble_vector(plane.V)
    c = _setup(T, "curved", 3, (2, 3))
    kvs, C = c["pb"]["kvs"], c["pb"]["C"]
    one = t.ExtractedSpline(t.EqualOrderSpline(1, T.N.NURBSControlMesh([3, 3], kvs, C)), 6)
    with pytest.raises(NotImplementedError, match="three fields"):
        F.ShellResidual(t.Function(one.V), one, T.mat).tangent().assemble_matrix(one.V)
    with pytest.raises(ValueError, match="n_thickness"):
        F.KirchhoffLoveHyper(HR.MU, HR.THICKNESS, 5)
    with pytest.raises(T.dev.TigarHipError, match="thickness points"):
        T.dev.shell_law_points(1, (HR.MU, HR.THICKNESS, 5), T.dev.DeviceVector(18), T.dev.DeviceVector(18))
    with pytest.raises(T.dev.TigarHipError, match="kind 2"):
        T.dev.shell_law_points(2, (HR.MU, HR.THICKNESS, 4), T.dev.DeviceVector(18), T.dev.DeviceVector(18))
    spline = c["spline"]
    with pytest.raises(NotImplementedError, match="row blocks"):
        F.ShellResidual(t.Function(spline.V), spline, T.mat, pressure=1.0).assemble_vector(spline.V, 0, 5)
    for bad in ("hyper", object(), 1):
        with pytest.raises(ValueError, match="unknown material"):
            F.ShellResidual(t.Function(spline.V), spline, bad)
    with pytest.raises(T.dev.TigarHipError):
        T.dev.shell_pressure_points(1.0, T.dev.DeviceVector(18), T.dev.DeviceVector(18), T.dev.DeviceVector(17), None)
