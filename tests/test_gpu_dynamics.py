"""GPU: nonlinear structural dynamics -- the point kernel ``tg_point_dynamics`` (csrc/tg_dynamics.hip), ``forms.PlanePenalty``,
``forms.DynamicResidual`` and ``timeIntegration.NonlinearTransientProblem``.

Reference: tests/dynamics_reference.py, which writes the residual as the reference's demo does on top of the shell and solid
references, pinned by tests/test_dynamics_reference_host.py (where the conditions on the cases and flows are checked).

Tolerances.  The kernel alone: elementwise against numpy in longdouble with DERIVED bounds -- every output is a sum of at most
four products plus the input, so 4 eps times the sum of the absolute values of its terms.  Assembled residual and tangent
(multiplied back by ``DynamicResidual.scale``): the rule of tests/test_gpu_shell.py unchanged -- normwise against the
longdouble run, 8 x the error of the float64 run of the same reference, never below 32 eps.  Energies: 32 eps of
sum wdet |e|.  Flows: dofs to 1e-6 of the largest, Newton counts +- 1.  ``-s`` prints every figure.
"""
import copy
import itertools
import json
import os

import numpy as np
import pytest

import dynamics_reference as DR
from test_gpu_shell import LD, _hold

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def T():
    import tigar_amd
    from tigar_amd import BSplines, forms, device, NURBS, timeIntegration
    device.device_info()

    class NS:
        pass
    ns = NS()
    ns.t, ns.B, ns.F, ns.dev, ns.N, ns.ti = tigar_amd, BSplines, forms, device, NURBS, timeIntegration
    return ns


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------
COEF = dict(sigma=1.0, m_u=3.25, m_w=-1.5, t_m=0.75, k_s=40.0, k_t=20.0, c_e=2.0)
PLANE_N, PLANE_OFFSET = (0.5, -0.25, 0.125), 0.375          # exactly representable: g = 0 exactly at X0 = (0.75, 0, 0), u = 0


def _kernel_inputs(nF, nJ, npts, seed):
    rng = np.random.default_rng(seed)
    a = dict(u=rng.uniform(-1, 1, (nF, nJ, npts)), X0=rng.uniform(-1, 1, (nF, npts)), w=rng.uniform(-1, 1, (nF, npts)),
             s=rng.uniform(-1, 1, (nF, nJ, npts)), T=rng.uniform(-1, 1, (nF, nF, nJ * nJ, npts)))
    for q in (0, npts // 2, npts - 1):
        a["X0"][:, q] = (0.75, 0.0, 0.0)[:nF]
        a["u"][:, 0, q] = 0.0
    return a


def _kernel_expected(nF, a, coef, plane, use_w):
    """(s, T, e, active mask, bounds of s, T, e) in longdouble; ``plane`` = (n, offset) or None"""
    c = {k: LD(v) for k, v in coef.items()}
    u, s, Tq = a["u"].astype(LD), a["s"].astype(LD), a["T"].astype(LD)
    w = a["w"].astype(LD) if use_w else np.zeros_like(a["w"], dtype=LD)
    npts = u.shape[-1]
    g, G = np.zeros(npts, dtype=LD), np.zeros(npts, dtype=LD)
    n = np.zeros(nF, dtype=LD)
    if plane is not None:
        n, off = np.asarray(plane[0][:nF]).astype(LD), LD(plane[1])
        x = a["X0"].astype(LD) + u[:, 0, :]
        g = off - np.einsum("c,cq->q", n, x)
        G = abs(off) + np.einsum("c,cq->q", abs(n), abs(a["X0"].astype(LD)) + abs(u[:, 0, :]))
    act = g > 0
    gp = np.where(act, g, LD(0))
    so, sb = c["sigma"] * s, 4 * EPS * abs(c["sigma"] * s)
    so[:, 0, :] += c["m_u"] * u[:, 0, :] + c["m_w"] * w - c["k_s"] * gp[None, :] * n[:, None]
    sb[:, 0, :] += 4 * EPS * (abs(c["m_u"] * u[:, 0, :]) + abs(c["m_w"] * w) + c["k_s"] * G[None, :] * abs(n)[:, None])
    To, Tb = Tq.copy(), np.zeros_like(Tq)
    add = c["t_m"] * np.eye(nF, dtype=LD)[:, :, None] + c["k_t"] * act.astype(LD)[None, None, :] * np.outer(n, n)[:, :, None]
    mag = abs(c["t_m"]) * np.eye(nF, dtype=LD)[:, :, None] + c["k_t"] * act.astype(LD)[None, None, :] * abs(np.outer(n, n))[:, :, None]
    To[:, :, 0, :] += add
    Tb[:, :, 0, :] = 4 * EPS * (abs(Tq[:, :, 0, :]) + mag)
    kin, con = LD(0.5) * c["c_e"] * np.sum(w * w, axis=0), LD(0.5) * c["k_s"] * gp * gp
    eb = 4 * EPS * (kin + con) + c["k_s"] * gp * 4 * EPS * G
    return so, To, kin + con, act, sb, Tb, eb


@pytest.mark.parametrize("nF,nJ", [(3, 6), (2, 1), (3, 1)])
@pytest.mark.parametrize("npts", [1, 63, 255, 256, 257, 1000])
def test_point_kernel_against_numpy(T, nF, nJ, npts):
    """every subset of {w, plane, s, T, e_out} with sigma = 1 and sigma != 1: outputs within the derived bounds, the count of
    active points, g = 0 exactly inactive (first, middle, last point), untouched entries bit-identical, a second run the same
    bits"""
    a = _kernel_inputs(nF, nJ, npts, 100 * nF + 10 * nJ + npts)
    dv = lambda v: T.dev.DeviceVector(data=np.ascontiguousarray(v).ravel())
    bits = lambda v: np.ascontiguousarray(v).ravel().view(np.int64)
    ud, Xd, wd = dv(a["u"]), dv(a["X0"]), dv(a["w"])
    worst = [0.0, 0.0, 0.0]
    for use_w, use_p, use_s, use_T, use_e in itertools.product((False, True), repeat=5):
        for sigma in (1.0, 1.75):
            coef = dict(COEF, sigma=sigma)
            plane = (PLANE_N, PLANE_OFFSET) if use_p else None
            so, To, eo, act, sb, Tb, eb = _kernel_expected(nF, a, coef, plane, use_w)
            assert not act[0] and not act[npts // 2] and not act[npts - 1]
            runs = []
            for _ in range(2):
                sd, Td = (dv(a["s"]) if use_s else None), (dv(a["T"]) if use_T else None)
                ed = T.dev.DeviceVector(npts) if use_e else None
                nact = T.dev.point_dynamics(nF, nJ, npts, [coef[k] for k in ("sigma", "m_u", "m_w", "t_m", "k_s", "k_t", "c_e")],
                                            plane=(PLANE_N[:nF] + (PLANE_OFFSET,)) if use_p else None, X0=Xd if use_p else None, u=ud,
                                            w=wd if use_w else None, s=sd, T=Td, e=ed, count=True)
                runs.append([v.get_local() if v is not None else None for v in (sd, Td, ed)])
                assert nact == int(np.sum(act))
            for x, y in zip(*runs):
                assert (x is None and y is None) or np.array_equal(bits(x), bits(y))
            gs, gT, ge = runs[0]
            if use_s:
                err = abs(gs.reshape(so.shape).astype(LD) - so)
                assert np.all(err <= sb), ("s", float(np.max(err - sb)))
                worst[0] = max(worst[0], float(np.max(err / np.maximum(sb, LD(1e-300)))))
                if sigma == 1.0:
                    assert np.array_equal(bits(gs.reshape(so.shape)[:, 1:, :]), bits(a["s"][:, 1:, :]))
            if use_T:
                gT = gT.reshape(To.shape)
                err = abs(gT[:, :, 0, :].astype(LD) - To[:, :, 0, :])
                assert np.all(err <= Tb[:, :, 0, :]), ("T", float(np.max(err - Tb[:, :, 0, :])))
                worst[1] = max(worst[1], float(np.max(err / np.maximum(Tb[:, :, 0, :], LD(1e-300)))))
                assert np.array_equal(bits(gT[:, :, 1:, :]), bits(a["T"][:, :, 1:, :]))
            if use_e:
                err = abs(ge.astype(LD) - eo)
                assert np.all(err <= eb), ("e", float(np.max(err - eb)))
                worst[2] = max(worst[2], float(np.max(err / np.maximum(eb, LD(1e-300)))) if np.any(eb > 0) else 0.0)
    # the plane alone (no inertia, sigma = 1): an inactive point keeps every bit of s and T
    coef = dict(COEF, sigma=1.0, m_u=0.0, m_w=0.0, t_m=0.0)
    act = _kernel_expected(nF, a, coef, (PLANE_N, PLANE_OFFSET), False)[3]
    sd, Td = dv(a["s"]), dv(a["T"])
    nact = T.dev.point_dynamics(nF, nJ, npts, [coef[k] for k in ("sigma", "m_u", "m_w", "t_m", "k_s", "k_t", "c_e")],
                                plane=PLANE_N[:nF] + (PLANE_OFFSET,), X0=Xd, u=ud, s=sd, T=Td, count=True)
    assert nact == int(np.sum(act))
    gs, gT = sd.get_local().reshape(a["s"].shape), Td.get_local().reshape(a["T"].shape)
    assert np.array_equal(bits(gs[..., ~act]), bits(a["s"][..., ~act])) and np.array_equal(bits(gT[..., ~act]), bits(a["T"][..., ~act]))
    if np.any(act):
        assert not np.array_equal(bits(gs[:, 0, :][..., act]), bits(a["s"][:, 0, :][..., act]))
    print("point kernel nF=%d nJ=%d npts=%4d: largest error / derived bound: s %.2f, T %.2f, e %.2f; %d of %d points active"
          % (nF, nJ, npts, worst[0], worst[1], worst[2], int(np.sum(act)), npts))


def test_point_kernel_refuses(T):
    """other nF and nJ, wrong sizes, a plane without reference positions: status 2 with a message"""
    d = T.dev
    coef = [1.0] * 7
    for call in (lambda: d.point_dynamics(1, 6, 1, coef, u=d.DeviceVector(6)), lambda: d.point_dynamics(3, 2, 1, coef, u=d.DeviceVector(6)),
                 lambda: d.point_dynamics(3, 6, 1, coef, u=d.DeviceVector(17)), lambda: d.point_dynamics(3, 6, 1, coef, T=d.DeviceVector(18)),
                 lambda: d.point_dynamics(3, 6, 1, coef, plane=(1.0, 0.0, 0.0, 0.0), u=d.DeviceVector(18), s=d.DeviceVector(18))):
        with pytest.raises(d.TigarHipError):
            call()
    with pytest.raises(ValueError, match="coef"):
        d.point_dynamics(3, 6, 1, [1.0] * 6)
    with pytest.raises(ValueError, match="plane"):
        d.point_dynamics(3, 6, 1, coef, plane=(1.0, 0.0, 0.0))


# ---- 2. the assembled DynamicResidual ------------------------------------------------------------------------------------
_CASES = {}


def _spline_of(T, pb, nF, degree):
    d = len(pb["kvs"])
    gen = T.t.EqualOrderSpline(nF, T.N.NURBSControlMesh([degree] * d, pb["kvs"], pb["C"]))
    return T.t.ExtractedSpline(gen, 2 * degree)


def _case(T, name):
    """the reference's figures of a case (longdouble, float64) and its spline: built once"""
    if name not in _CASES:
        c = DR.assembled_case(name)
        pb, (ref, r64) = c["pb"], c["dyn"]
        y, old = c["y"], c["old"]
        c["spline"] = _spline_of(T, pb, ref.nF, pb["p"])
        c["want"] = {"R": (ref.residual(y, old), r64.residual(y, old)), "K": (ref.tangent(y, old), r64.tangent(y, old)),
                     "active": ref.active(y, old), "E": ref.energy(y, ref.rates(y, old)[0])}
        _CASES[name] = c
    return _CASES[name]


def _functions(T, V, vectors):
    out = []
    for v in vectors:
        f = T.t.Function(V)
        f.vector().set_local(np.asarray(v, dtype=np.float64))
        out.append(f)
    return out


def _dynamic(T, name, c, spline, body_force=None, device_law=True):
    info = DR.CASES[name]
    y, yo, vo, ao = _functions(T, spline.V, [c["y"]] + list(c["old"]))
    if info["kind"] == "shell":
        static = T.F.ShellResidual(y, spline, c["material"], body_force=body_force, rational=c["rational"], pressure=info["pressure"],
                                   device_law=device_law)
    else:
        static = T.F.HyperelasticResidual(y, spline, c["material"], body_force=body_force, rational=c["rational"])
    it = T.ti.GeneralizedAlphaIntegrator(DR.CASE_RHO_INF, DR.CASE_DT, y, [yo, vo, ao])
    n, off, k = c["plane"]
    return static, it, T.F.DynamicResidual(static, it, c["density"], mass_damping=DR.CASE_DAMPING, contact=T.F.PlanePenalty(n, off, k))


def _counted_calls(T, monkeypatch):
    """{"eval", "dynamics"}: the point evaluations of a field and the launches of ``tg_point_dynamics`` from here on"""
    calls = {"eval": 0, "dynamics": 0}

    def counted(key, f):
        def run(*args, **kwargs):
            calls[key] += 1
            return f(*args, **kwargs)
        return run
    monkeypatch.setattr(T.dev, "quad_eval", counted("eval", T.dev.quad_eval))
    monkeypatch.setattr(T.dev, "quad_jet", counted("eval", T.dev.quad_jet))
    monkeypatch.setattr(T.dev, "point_dynamics", counted("dynamics", T.dev.point_dynamics))
    return calls


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_assembled_residual_tangent_energy_and_reuse(T, name, monkeypatch):
    c = _case(T, name)
    spline, V, want = c["spline"], c["spline"].V, c["want"]
    static, it, dyn = _dynamic(T, name, c, spline)
    nF = c["dyn"][0].nF
    untouched = dict(static.__dict__)
    calls = _counted_calls(T, monkeypatch)
    assert dyn.scale == it.ALPHA_F
    R = dyn.assemble_vector(V).get_local() * dyn.scale
    first = dict(calls)
    assert first == {"eval": 2 * nF, "dynamics": 1}               # the static evaluation of the nF fields, and w once
    assert dyn.active_points() == want["active"]
    _hold(name + ": residual x scale", R, *want["R"])
    tan = dyn.tangent()
    pressure = DR.CASES[name].get("pressure") is not None
    assert tan.symmetric is (not pressure) and tan.geometry is spline
    K = tan.assemble_matrix(V).to_scipy().toarray() * dyn.scale
    assert calls == {"eval": first["eval"] + nF, "dynamics": 2}   # w is reused: the static evaluation alone, one launch
    assert dyn.active_points() == want["active"]
    bound = _hold(name + ": tangent x scale", K, *want["K"])
    asym = float(np.max(np.abs(K - K.T))) / float(np.max(np.abs(K)))
    print("%-62s |K - K^T| / max|K| %.2e" % (name, asym))
    if not pressure:
        assert asym <= 2 * bound
    else:
        assert asym > 1e-6
    dyn.assemble_vector(V)
    assert calls == {"eval": first["eval"] + 2 * nF, "dynamics": 3}
    # a block of the tangent
    n = V.grids[0].num_nodes()
    Kb = tan.assemble_block(V, 1, 0).to_scipy().toarray() * dyn.scale
    assert np.array_equal(Kb, K[n:2 * n, :n])
    # energies at the current level
    e0 = dict(calls)
    E = dyn.energy(V)
    ref_e, mags = want["E"]
    for part in ("strain", "kinetic", "contact", "total"):
        err, bnd = abs(LD(E[part]) - ref_e[part]), 32 * EPS * mags[part]
        print("%-62s energy %-8s %.6e  error %.2e  bound %.2e" % (name, part, E[part], float(err), float(bnd)))
        assert err <= bnd, (part, float(err), float(bnd))
    assert E["contact"] > 0.0 and E["kinetic"] > 0.0
    # the handed-in residual is not modified, and the next step evaluates w again
    assert static.u is it.x and static.__dict__.keys() == untouched.keys() and all(static.__dict__[k] is v for k, v in untouched.items())
    assert not any(isinstance(v, dict) and v for v in static.__dict__.values())          # (no cache of the static object was filled)
    calls.update(e0)
    it.advance()
    dyn.assemble_vector(V)
    assert calls["eval"] == e0["eval"] + 2 * nF
    dyn.assemble_vector(V)
    dyn.invalidate()
    before = calls["eval"]
    dyn.assemble_vector(V)
    assert calls["eval"] == before + 2 * nF


# per unit reference measure; large enough to move the residual by a hundredth of its largest entry, so that a force left
# out, taken with the wrong sign or not divided by alpha_f misses the bound by many orders
BODY_FORCE = {"cylinder-svk": (30.0, -20.0, 50.0), "annulus": (40.0, -70.0)}


@pytest.mark.parametrize("name, variant", [("cylinder-svk", "body_force"), ("annulus", "body_force"), ("cylinder-svk", "host_law")])
def test_assembled_body_force_and_host_law(T, name, variant, monkeypatch):
    """a constant ``body_force`` on a shell and on a solid, and the shell law through its ``host`` method (``device_law=False``):
    residual and tangent against the references, with the evaluations and launches of the test above"""
    c = _case(T, name)
    spline, V, want = c["spline"], c["spline"].V, c["want"]
    f = BODY_FORCE[name] if variant == "body_force" else None
    static, it, dyn = _dynamic(T, name, c, spline, body_force=f, device_law=variant != "host_law")
    nF = c["dyn"][0].nF
    want_R = want["R"]
    if f is not None:
        refs = [copy.copy(r) for r in c["dyn"]]
        for r in refs:
            r.f = np.broadcast_to(np.asarray(f).astype(r.dtype), (r.wdet.size, r.nF))
        want_R = tuple(r.residual(c["y"], c["old"]) for r in refs)
        moved = float(np.max(np.abs(want_R[0] - want["R"][0])) / np.max(np.abs(want_R[0])))
        print("%-62s the body force moves the residual by %.2e of its largest entry" % (name, moved))
        assert moved > 1e-3
    calls = _counted_calls(T, monkeypatch)
    R = dyn.assemble_vector(V).get_local() * dyn.scale
    first = dict(calls)
    assert first == {"eval": 2 * nF, "dynamics": 1}
    assert dyn.active_points() == want["active"]
    _hold("%s, %s: residual x scale" % (name, variant), R, *want_R)
    tan = dyn.tangent()
    K = tan.assemble_matrix(V).to_scipy().toarray() * dyn.scale
    assert calls == {"eval": first["eval"] + nF, "dynamics": 2}
    assert tan.symmetric is True and dyn.active_points() == want["active"]
    _hold("%s, %s: tangent x scale" % (name, variant), K, *want["K"])
    dyn.assemble_vector(V)
    assert calls == {"eval": first["eval"] + 2 * nF, "dynamics": 3}


def test_backward_euler_residual_and_tangent(T):
    """a ``BackwardEulerIntegrator`` with two old functions: alpha_f = 1, its own xdot() and xddot()"""
    name = "cylinder-svk"
    c = DR.assembled_case(name, scheme="backward_euler")
    ref, r64 = c["dyn"]
    spline = _case(T, name)["spline"]
    y, yo, vo = _functions(T, spline.V, [c["y"]] + list(c["old"]))
    static = T.F.ShellResidual(y, spline, c["material"], rational=c["rational"])
    it = T.ti.BackwardEulerIntegrator(DR.CASE_DT, y, [yo, vo])
    n, off, k = c["plane"]
    dyn = T.F.DynamicResidual(static, it, c["density"], mass_damping=DR.CASE_DAMPING, contact=T.F.PlanePenalty(n, off, k))
    assert dyn.scale == 1.0 and dyn.t_alpha == it.t
    _hold("backward Euler: residual", dyn.assemble_vector(spline.V).get_local(), ref.residual(c["y"], c["old"]), r64.residual(c["y"], c["old"]))
    _hold("backward Euler: tangent", dyn.tangent().assemble_matrix(spline.V).to_scipy().toarray(), ref.tangent(c["y"], c["old"]),
          r64.tangent(c["y"], c["old"]))
    assert dyn.active_points() == ref.active(c["y"], c["old"])


def test_refusals(T, monkeypatch):
    """row blocks, several ranks, a caller-ordered spline, another kind of static, density <= 0, a first-order integrator, a
    static whose u is not the integrator's unknown, a plane of the wrong dimension: each with its reason"""
    F, t, ti = T.F, T.t, T.ti
    c = _case(T, "cylinder-svk")
    spline, V = c["spline"], c["spline"].V
    static, it, dyn = _dynamic(T, "cylinder-svk", c, spline)
    n = V.grids[0].num_nodes()
    with pytest.raises(NotImplementedError, match="row blocks"):
        dyn.assemble_vector(V, 0, n)
    with pytest.raises(NotImplementedError, match="row blocks"):
        dyn.tangent().assemble_matrix(V, n, 2 * n)
    for attr, reason in (("_distributed", "ranks"), ("_caller_ordered", "feOrder"), ("_implicit", "row blocks")):
        with monkeypatch.context() as m:
            m.setattr(spline, attr, lambda: True)
            with pytest.raises(NotImplementedError, match=reason):
                dyn.assemble_vector(V)
            with pytest.raises(NotImplementedError, match=reason):
                dyn.tangent().assemble_matrix(V)
    for attr, reason in (("_distributed", "ranks"), ("_caller_ordered", "feOrder")):
        with monkeypatch.context() as m:
            m.setattr(spline, attr, lambda: True)
            with pytest.raises(NotImplementedError, match=reason):
                ti.NonlinearTransientProblem(spline, static, 1.0, 0.1)
    with pytest.raises(NotImplementedError, match="ShellResidual or a HyperelasticResidual"):
        F.DynamicResidual(F.LaplaceForm(), it, 1.0)
    with pytest.raises(NotImplementedError, match="ShellResidual or a HyperelasticResidual"):
        ti.NonlinearTransientProblem(spline, F.LaplaceForm(), 1.0, 0.1)
    for rho in (0.0, -1.0):
        with pytest.raises(ValueError, match="density"):
            F.DynamicResidual(static, it, rho)
    y = static.u
    first = ti.GeneralizedAlphaIntegrator(0.5, 0.1, y, [t.Function(V), t.Function(V)])
    with pytest.raises(ValueError, match="first-order"):
        F.DynamicResidual(static, first, 1.0)
    with pytest.raises(ValueError, match="first-order"):
        F.DynamicResidual(static, ti.BackwardEulerIntegrator(0.1, y, [t.Function(V)]), 1.0)
    with pytest.raises(ValueError, match="integrator"):
        F.DynamicResidual(static, ti.LoadStepper(0.1), 1.0)
    other = ti.GeneralizedAlphaIntegrator(0.5, 0.1, t.Function(V), [t.Function(V), t.Function(V), t.Function(V)])
    with pytest.raises(ValueError, match="integrator solves for"):
        F.DynamicResidual(static, other, 1.0)
    with pytest.raises(ValueError, match="normal"):
        F.DynamicResidual(static, it, 1.0, contact=F.PlanePenalty((1.0, 0.0), 0.0, 1.0))
    with pytest.raises(ValueError, match="PlanePenalty"):
        F.DynamicResidual(static, it, 1.0, contact=(0.0, 0.0, 1.0))
    for bad in ((0.0, 0.0, 0.0), (1.0,), (1.0, 0.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match="normal"):
            F.PlanePenalty(bad, 0.0, 1.0)
    with pytest.raises(ValueError, match="stiffness"):
        F.PlanePenalty((0.0, 0.0, 1.0), 0.0, 0.0)
    assert np.allclose(F.PlanePenalty((0.0, 0.0, 2.0), 0.5, 3.0).normal, (0.0, 0.0, 1.0))
    for kw, reason in ((dict(scheme="newmark"), "scheme"), (dict(DELTA_T=0.0), "DELTA_T"), (dict(RHO_INF=1.5), "RHO_INF"),
                       (dict(absoluteTolerance=-1.0), "absoluteTolerance")):
        args = dict(DELTA_T=0.1)
        args.update(kw)
        with pytest.raises(ValueError, match=reason):
            ti.NonlinearTransientProblem(spline, static, 1.0, **args)


# ---- 3. NonlinearTransientProblem: the linear limit and the flows against the float64 host flows -------------------------
def _golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", DR.GOLDEN_FLOWS)) as f:
        return json.load(f)


def _flow_problem(T, kind, p=2, **kw):
    """the device's problem of a flow of tests/dynamics_reference.py: (setup, spline, problem)"""
    s = DR.flow_setup(kind, p)
    pb = s["pb"]
    shell = kind in ("vibration", "euler", "obstacle")
    nF = 3
    gen = T.t.EqualOrderSpline(nF, T.N.NURBSControlMesh([p] * len(pb["kvs"]), pb["kvs"], pb["C"]))
    sp0 = gen.getScalarSpline(0)
    for f in range(nF):
        if shell:
            gen.addZeroDofs(f, sp0.getSideDofs(1, 0, nLayers=2))
        else:
            for side in ((0, 1) if kind == "linear" else (0,)):
                gen.addZeroDofs(f, sp0.getSideDofs(pb["direction"], side))
    spline = T.t.ExtractedSpline(gen, 2 * p)
    spline.setSolverOptions(linearSolver=T.t.PETScLUSolver(), relativeTolerance=DR.FLOW_TOL[kind], maxIters=DR.FLOW_MAX_ITERS[kind] + 1)
    y = T.t.Function(spline.V)
    if shell:
        static = T.F.ShellResidual(y, spline, s["material"], body_force=s["f"], rational=True)
    else:
        static = T.F.HyperelasticResidual(y, spline, s["material"], rational=True)
    contact = None if s["plane"] is None else T.F.PlanePenalty(*s["plane"])
    prob = T.ti.NonlinearTransientProblem(spline, static, s["density"], s["dt"], RHO_INF=s["rho_inf"], scheme=s["scheme"], contact=contact,
                                          y0=T.dev.DeviceVector(data=np.asarray(s["U0"], dtype=np.float64)),
                                          initial_acceleration=s["A0"] is not None, **kw)
    return s, spline, prob


def _run_flow(T, kind, p, capsys):
    rec = _golden()["%s-p%d" % (kind, p)]
    s, spline, prob = _flow_problem(T, kind, p)
    assert abs(s["dt"] - rec["dt"]) <= 1e-9 * rec["dt"]
    if s["A0"] is not None:
        A = spline.FEtoIGA(prob.yddot).get_local()
        assert np.max(np.abs(A - s["A0"])) <= 1e-6 * np.max(np.abs(s["A0"]))
    worst, iters, active = 0.0, [], []
    for step in range(1, DR.FLOW_STEPS[kind] + 1):
        prob.step()
        iters.append(len(prob.last["newton"]))
        active.append(prob.last["active_points"])
        assert prob.last["assembly_seconds"] > 0.0 and prob.last["solve_seconds"] > 0.0
        if str(step) in rec["U"]:
            want = np.asarray(rec["U"][str(step)])
            got = spline.FEtoIGA(prob.y).get_local()
            worst = max(worst, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
    with capsys.disabled():
        print("%s p=%d: device iterations %s (host %s), active points %s (host %s), dofs differ by %.2e of the largest; t = %.4f"
              % (kind, p, iters, rec["iterations"], active, rec["active"], worst, prob.t))
    assert all(abs(a - b) <= 1 for a, b in zip(iters, rec["iterations"]))
    assert worst <= 1e-6
    assert abs(prob.t - DR.FLOW_STEPS[kind] * s["dt"]) <= 1e-12 * prob.t
    return prob, rec, active


@pytest.mark.parametrize("p", [2, 3])
def test_flow_free_vibration_of_the_strip(T, p, capsys):
    """(a) the strip released from its static solution under STRIP_LOAD: 8 steps of 1/20 of the lowest linearised period"""
    prob, rec, _ = _run_flow(T, "vibration", p, capsys)
    assert max(rec["iterations"]) <= DR.FLOW_MAX_ITERS["vibration"]
    e = prob.energy()
    assert abs(e["total"] - rec["energy"][-1]) <= 1e-6 * rec["energy"][-1] and e["contact"] == 0.0


def test_flow_obstacle(T, capsys):
    """(b) the strip under STRIP_LOAD from rest with a plane in the way of its tip: the active sets of the host flow"""
    prob, rec, active = _run_flow(T, "obstacle", 2, capsys)
    assert sum(1 for a in rec["active"] if a > 0) >= 2 and active == rec["active"]
    e = prob.energy()
    assert abs(e["total"] - rec["energy"][-1]) <= 1e-6 * rec["energy"][-1]


def test_flow_released_block(T, capsys):
    """(c) the neo-Hookean block released from its static solution (the moved face let go), a0 = 0 as the demo does"""
    _run_flow(T, "solid", 2, capsys)


def test_flow_backward_euler(T, capsys):
    """(d) the free vibration with a ``BackwardEulerIntegrator``"""
    prob, rec, _ = _run_flow(T, "euler", 2, capsys)
    assert prob.yddot is None


def test_linear_limit_and_energy_drift(T, capsys):
    """``LinearElastic`` on the block, no contact: the second Newton norm of every step is <= 1e-10, and with RHO_INF = 1 the
    total energy over 20 steps drifts by at most 8 x the drift of the float64 host flow (tests/golden/dynamics_flows.json,
    pinned by tests/test_dynamics_reference_host.py)"""
    rec = _golden()["linear-p2"]
    s, spline, prob = _flow_problem(T, "linear", 2)
    e0 = prob.energy()["total"]
    energies, seconds = [], []
    for step in range(DR.FLOW_STEPS["linear"]):
        prob.step()
        seconds.append(prob.last["newton"][1])
        energies.append(prob.energy()["total"])
    host_drift = max(abs(e - rec["energy"][0]) for e in rec["energy"]) / rec["energy"][0]
    drift = max(abs(e - e0) for e in energies) / e0
    with capsys.disabled():
        print("linear limit: largest second Newton norm %.2e; energy %.12e, drift %.2e (float64 host flow %.2e)"
              % (max(seconds), e0, drift, host_drift))
    assert max(seconds) <= 1e-10
    assert abs(e0 - rec["energy"][0]) <= 1e-9 * e0
    assert drift <= 8 * host_drift


def test_absolute_tolerance_ends_a_step_at_rest(T):
    """a body at rest without loads: the predictor is converged, the relative test would divide by a first norm of zero; with
    ``absoluteTolerance`` the step ends without a Newton step"""
    s, spline, prob = _flow_problem(T, "vibration", 2, absoluteTolerance=1e-12)
    for f in (prob.y_old, prob.ydot_old, prob.yddot_old, prob.static.u):
        f.vector().zero()
    prob.dyn.invalidate()
    prob.step(2)
    assert prob.last["newton"] == [1.0] and prob.last["iterations"] == 0 and prob.steps_done == 2
    assert prob.y.vector().norm("l2") == 0.0
    # nF numbers as initial data: the homogeneous representation of a constant in the rational space
    c = (0.25, -0.5, 1.0)
    prob2 = T.ti.NonlinearTransientProblem(spline, prob.static, 1.0, 0.1, ydot0=c, initial_acceleration=False)
    w = spline.cpFuncs[-1].vector().get_local()
    assert np.array_equal(prob2.ydot.vector().get_local(), np.concatenate([ci * w for ci in c]))
    k = prob2.energy()["kinetic"]
    area = float(T.F.quadrature_points(spline, spline.V_control).weights.get_local().sum())
    assert abs(k - 0.5 * sum(ci * ci for ci in c) * area) <= 1e-12 * k
