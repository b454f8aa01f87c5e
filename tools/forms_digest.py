"""SHA-256 of what the point forms of tigar_amd/forms.py and the quadrature-point methods of ExtractedSpline give, through
the public API only (developer tool: a change of the Python layer that is meant to leave the device work alone runs this
file in both checkouts and compares the two outputs byte for byte).

One JSON line per (form, case, plain / rational): the digest of the output bytes -- row pointers, columns and values of a
matrix, the values of a vector -- and the ``symmetric`` flag where the form has one.  A call that raises gives a line with
the exception's type (not its text).  Patches: a curve at p = 3, a plane patch at p = 2 with nq != p + 1, a surface in
space, a volume at p = 2, each also with varying weights, and a 2 x 2-element cylinder strip for the shell.  Point data come
as numbers, callables, arrays and DeviceVectors; all of it is seeded.  After these lines: the hyperelastic shell with a
follower pressure, and ``DynamicResidual`` -- both integrators, shells and solids, laws of the device and of the host, a
plane that cuts through the points (asserted here), the assembled cases of tests/dynamics_reference.py -- at states where no
law refuses a point (a refusal there ends the run), and the refusals of its constructor.

    python tools/forms_digest.py [--out profiles/forms_digest.jsonl]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tigar_amd as t  # noqa: E402
from tigar_amd import BSplines as B, NURBS as N, device as dev, forms as F  # noqa: E402

# name: (degree, elements per direction, nsd, nq or None)
PATCHES = {"curve_p3": (3, (3,), 2, None), "plane_p2_nq2": (2, (3, 2), 2, 2), "surface_p2": (2, (2, 3), 3, None),
           "volume_p2": (2, (2, 1, 2), 3, None), "strip_p2_2x2": (2, (2, 2), 3, None)}


def control_net(p, nels, nsd, weighted, strip=False):
    """(knot vectors, homogeneous control net): a smooth map of the Greville points, the weights varying when asked"""
    kvs = [np.asarray(B.uniformKnots(p, 0.0, 1.0, n), dtype=np.float64) for n in nels]
    grev = [np.array([np.sum(kv[i + 1:i + p + 1]) / p for i in range(len(kv) - p - 1)]) for kv in kvs]
    g = list(np.meshgrid(*grev, indexing="ij"))
    g = g + [0.0 * g[0]] * (3 - len(g))
    if strip:
        X = [np.cos(0.5 * np.pi * g[0]), np.sin(0.5 * np.pi * g[0]), 1.5 * g[1]]
    else:
        X = [g[0] + 0.15 * g[1] * g[0] + 0.1 * g[2], g[1] * (1.0 + 0.2 * g[0]) - 0.1 * g[0] + 0.3 * g[0] ** 2,
             g[2] * (1.0 + 0.3 * g[0]) + 0.4 * g[0] ** 2 - 0.3 * g[1] ** 2 + 0.2 * g[0] * g[1]][:nsd]
    w = 1.0 + (0.2 * g[0] * (1.0 - g[0]) + 0.1 * g[1] if weighted else 0.0 * g[0])
    return kvs, np.stack([w * x for x in X] + [w], axis=-1)


def spline_of(name, weighted, fields):
    p, nels, nsd, nq = PATCHES[name]
    kvs, C = control_net(p, nels, nsd, weighted, strip=name.startswith("strip"))
    return t.ExtractedSpline(t.EqualOrderSpline(fields, N.NURBSControlMesh([p] * len(nels), kvs, C)), 2 * p)


def flat(out):
    """the arrays whose bytes make the digest"""
    if out is None:
        return []
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in flat(o)]
    if hasattr(out, "to_scipy"):
        A = out.to_scipy().tocsr()
        return [np.asarray(A.indptr, dtype=np.int64), np.asarray(A.indices, dtype=np.int64), np.asarray(A.data, dtype=np.float64)]
    if hasattr(out, "get_local"):
        return [out.get_local()]
    return [np.asarray(out, dtype=np.float64)]


class Recorder(object):
    def __init__(self, f):
        self.f, self.lines = f, 0

    def __call__(self, form, case, rational, call, symmetric=None, strict=False):
        """``strict``: the call is not meant to refuse, and what it raises ends the run"""
        line = {"form": form, "case": case, "rational": rational}
        try:
            h = hashlib.sha256()
            for a in flat(call()):
                h.update(np.ascontiguousarray(a).tobytes())
            line["sha256"] = h.hexdigest()
            if symmetric is not None:
                line["symmetric"] = bool(symmetric())
        except Exception as e:  # noqa: BLE001  (a refusal is a result: its type is compared)
            if strict:
                raise
            line = {"form": form, "case": case, "rational": rational, "error": type(e).__name__}
        self.f.write(json.dumps(line, sort_keys=True) + "\n")
        self.lines += 1


def function(V, rng, scale=1.0):
    u = t.Function(V)
    u.vector().set_local(scale * rng.standard_normal(V.dim()))
    return u


def dv(a):
    return dev.DeviceVector(data=np.ascontiguousarray(a, dtype=np.float64).ravel())


class HostLaw(object):
    """a law the library does not know: evaluated on the host, its symmetry read from the bits"""

    def __init__(self, law):
        self.host = law.host


def scalar_forms(rec, name, case, weighted, rat):
    p, nels, nsd, nq = PATCHES[name]
    d = len(nels)
    rng = np.random.default_rng(len(case))
    s = spline_of(name, weighted, 1)
    V = s.V
    npts = s.quadraturePoints(nq).npts
    u = function(V, rng)
    sym = rng.standard_normal((npts, nsd, nsd))
    sym = sym + sym.transpose(0, 2, 1)
    bq = rng.standard_normal((npts, nsd))
    diffusions = {"none": None, "number": 1.5, "callable": lambda x: 1.0 + x[:, 0] ** 2, "function": u,
                  "tensor_array": rng.standard_normal((npts, nsd, nsd)), "symmetric_array": sym, "one_matrix": np.eye(nsd) * 2.0,
                  "tensor_callable": lambda x: np.eye(nsd)[None] * (1.0 + x[:, :1, None]),
                  "scalar_device": dv(1.0 + rng.random(npts)), "tensor_device": dv(sym.transpose(1, 2, 0))}
    for key, A in diffusions.items():
        form = F.CoefficientForm(s, diffusion=A, nq=nq, rational=rat)
        rec("CoefficientForm/diffusion=" + key, case, rat, lambda: form.assemble_matrix(V), lambda: form.symmetric)
    velocities = {"numbers": ([0.5] * nsd, [0.5] * nsd), "callable_array": (lambda x: 0.3 * x, bq), "device": (dv(bq.T), dv(bq.T)),
                  "array_none": (bq, None)}
    for key, (b, c) in velocities.items():
        form = F.CoefficientForm(s, diffusion=1.0, flux_velocity=b, velocity=c, reaction=u if key == "device" else 2.0, nq=nq, rational=rat)
        rec("CoefficientForm/bc=" + key, case, rat, lambda: form.assemble_matrix(V), lambda: form.symmetric)
    for key, f, flux in (("number", 1.0, None), ("callable_flux", lambda x: x[:, 0], lambda x: 0.5 * x), ("array_flux", bq[:, 0], bq),
                         ("device_flux", dv(bq[:, 0]), dv(bq.T)), ("flux_only", None, [1.0] * nsd)):
        rec("QuadratureLoadForm/" + key, case, rat, lambda: F.QuadratureLoadForm(f, s, nq=nq, rational=rat, flux=flux).assemble_vector(V))
    res = F.QuasilinearResidual(u, s, lambda x, uq, gq: ((1.0 + uq ** 2)[:, None] * gq, uq ** 3),
                                lambda x, uq, gq: (1.0 + uq ** 2, 2.0 * uq[:, None] * gq, None, 3.0 * uq ** 2),
                                f=lambda x: x[:, 0], nq=nq, rational=rat)
    tan = res.tangent()
    rec("QuasilinearResidual", case, rat, lambda: res.assemble_vector(V))
    rec("QuasilinearResidual.tangent", case, rat, lambda: tan.assemble_matrix(V), lambda: tan.symmetric)
    rec("evaluateAtQuadrature", case, rat, lambda: s.evaluateAtQuadrature(u, grad=True, nq=nq, rational=rat))
    rec("evaluateJetsAtQuadrature", case, rat, lambda: s.evaluateJetsAtQuadrature(u, nq=nq, rational=rat))
    if not rat:
        rec("geometryJetsAtQuadrature", case, rat, lambda: s.geometryJetsAtQuadrature(nq=nq))
        rec("errorNorm", case, rat, lambda: s.errorNorm(u, lambda x: x[:, 0], "H1", exact_grad=lambda x: np.eye(nsd)[0] + 0.0 * x, nq=nq))
    nJ = 3 if d == 1 else 6
    Tq = rng.standard_normal((npts, nJ, nJ))
    for key, T in (("array", Tq), ("symmetric_callable", lambda x: np.eye(nJ)[None] + 0.0 * x[:, :1, None]), ("one_block", np.eye(nJ)),
                   ("device", dv((Tq + Tq.transpose(0, 2, 1)).transpose(1, 2, 0)))):
        form = F.JetCoefficientForm(s, T, nq=nq, rational=rat)
        rec("JetCoefficientForm/" + key, case, rat, lambda: form.assemble_matrix(V), lambda: form.symmetric)
    sq = rng.standard_normal((npts, nJ))
    for key, sv in (("array", sq), ("callable", lambda x: np.ones((x.shape[0], nJ))), ("numbers", np.arange(nJ) + 1.0), ("device", dv(sq.T))):
        rec("JetLoadForm/" + key, case, rat, lambda: F.JetLoadForm(sv, s, nq=nq, rational=rat).assemble_vector(V))
    if d in (2, 3):
        faces = [(0, 0), (d - 1, 1)]
        nface = [s.boundaryPoints(k, side, nq).npts for k, side in faces]
        loads = {"number": 2.0, "callable": lambda x: x[:, 0], "callable_x_n": lambda x, n: n[:, 0] + x[:, 1], "function": u,
                 "per_face": [rng.standard_normal(nface[0]), dv(rng.standard_normal(nface[1]))]}
        for key, f in loads.items():
            rec("BoundaryLoadForm/" + key, case, rat, lambda: F.BoundaryLoadForm(f, s, faces, nq=nq, rational=rat).assemble_vector(V))
        rec("BoundaryLoadForm/fn", case, rat, lambda: F.BoundaryLoadForm(1.0, s, faces, nq=nq, rational=rat, fn=lambda x: x[:, 0]).assemble_vector(V))
        rec("BoundaryMassForm", case, rat, lambda: F.BoundaryMassForm(lambda x: 1.0 + x[:, 0], s, faces, nq=nq, rational=rat).assemble_matrix(V))
        for symm in (True, False):
            nit = F.NitscheForm(s, faces, 10.0, symmetric=symm, nq=nq, rational=rat)
            rec("NitscheForm/symmetric=%s" % symm, case, rat, lambda: nit.assemble_matrix(V), lambda: nit.symmetric)
            rec("NitscheForm.load/symmetric=%s" % symm, case, rat, lambda: nit.load(lambda x: x[:, 0]).assemble_vector(V))
        total = F.Sum(F.CoefficientForm(s, diffusion=1.0, nq=nq, rational=rat), (0.5, F.BoundaryMassForm(1.0, s, faces, nq=nq, rational=rat)))
        rec("Sum/coefficient+boundary_mass", case, rat, lambda: total.assemble_matrix(V), lambda: total.symmetric)
        if not rat:
            rec("integrateBoundary", case, rat, lambda: s.integrateBoundary(lambda x, n: n[:, 0] * x[:, 0], faces, nq=nq))


def vector_forms(rec, name, case, weighted, rat):
    p, nels, nsd, nq = PATCHES[name]
    d = len(nels)
    rng = np.random.default_rng(100 + len(case))
    npts = spline_of(name, weighted, 1).quadraturePoints(nq).npts
    nJ = 3 if d == 1 else 6
    if d in (1, 2):
        nF = 2
        s = spline_of(name, weighted, nF)
        V = s.V
        u = function(V, rng)
        Tq = rng.standard_normal((npts, nF * nJ, nF * nJ))
        Ts = (Tq + Tq.transpose(0, 2, 1)).reshape(npts, nF, nJ, nF, nJ)
        for key, T in (("array", Tq.reshape(npts, nF, nJ, nF, nJ)), ("symmetric_array", Ts), ("callable", lambda x: Ts),
                       ("one_block", Ts[0]), ("device", dv(Ts.transpose(1, 3, 2, 4, 0)))):
            form = F.VectorJetCoefficientForm(s, T, nq=nq, rational=rat)
            rec("VectorJetCoefficientForm/" + key, case, rat, lambda: form.assemble_matrix(V), lambda: form.symmetric)
        form = F.VectorJetCoefficientForm(s, Ts, nq=nq, rational=rat)
        rec("VectorJetCoefficientForm/block_1_0", case, rat, lambda: form.assemble_block(V, 1, 0))
        sq = rng.standard_normal((npts, nF, nJ))
        for key, sv in (("array", sq), ("callable", lambda x: sq), ("numbers", np.ones((nF, nJ))), ("device", dv(sq.transpose(1, 2, 0)))):
            rec("VectorJetLoadForm/" + key, case, rat, lambda: F.VectorJetLoadForm(sv, s, nq=nq, rational=rat).assemble_vector(V))
        rec("evaluateJetsAtQuadrature/fields", case, rat, lambda: s.evaluateJetsAtQuadrature(u, nq=nq, rational=rat))
    if nsd == d and d in (2, 3):
        nF = d
        s = spline_of(name, weighted, nF)
        V = s.V
        u = function(V, rng, 0.02)
        Aq = rng.standard_normal((npts, nF * d, nF * d))
        As = (Aq + Aq.transpose(0, 2, 1)).reshape(npts, nF, d, nF, d)
        Mq = rng.standard_normal((npts, nF, nF))
        data = {"array": (Aq.reshape(npts, nF, d, nF, d), None), "symmetric_array": (As, Mq + Mq.transpose(0, 2, 1)),
                "callable": (lambda x: As, lambda x: Mq), "one_block": (As[0], np.eye(nF)),
                "device": (dv(As.transpose(1, 3, 2, 4, 0)), dv((Mq + Mq.transpose(0, 2, 1)).transpose(1, 2, 0)))}
        for key, (A, M) in data.items():
            form = F.VectorCoefficientForm(s, A, reaction=M, nq=nq, rational=rat)
            rec("VectorCoefficientForm/" + key, case, rat, lambda: form.assemble_matrix(V), lambda: form.symmetric)
        form = F.VectorCoefficientForm(s, As, reaction=Mq, nq=nq, rational=rat)
        rec("VectorCoefficientForm/block_0_1", case, rat, lambda: form.assemble_block(V, 0, 1))
        fq, Pq = rng.standard_normal((npts, nF)), rng.standard_normal((npts, nF, d))
        for key, f, flux in (("numbers", [1.0] * nF, None), ("callable_array", lambda x: fq, Pq), ("array_callable", fq, lambda x: Pq),
                             ("none_device", None, dv(Pq.transpose(1, 2, 0)))):
            rec("VectorLoadForm/" + key, case, rat, lambda: F.VectorLoadForm(f, s, flux=flux, nq=nq, rational=rat).assemble_vector(V))
        laws = {"LinearElastic": F.LinearElastic(2.0, 1.0), "StVenantKirchhoff": F.StVenantKirchhoff(2.0, 1.0),
                "NeoHookean": F.NeoHookean(2.0, 1.0), "host_law": HostLaw(F.StVenantKirchhoff(2.0, 1.0))}
        for key, law in laws.items():
            res = F.HyperelasticResidual(u, s, law, body_force=lambda x: 0.1 * x[:, :nF], nq=nq, rational=rat)
            tan = res.tangent()
            rec("HyperelasticResidual/" + key, case, rat, lambda: res.assemble_vector(V))
            rec("HyperelasticResidual.tangent/" + key, case, rat, lambda: tan.assemble_matrix(V), lambda: tan.symmetric)
            rec("HyperelasticResidual.tangent.block/" + key, case, rat, lambda: tan.assemble_block(V, 1, 0))
            rec("HyperelasticResidual.energy/" + key, case, rat, lambda: res.energy(V))
        faces = [(0, 1)]
        rec("BoundaryLoadForm/traction", case, rat, lambda: F.BoundaryLoadForm(lambda x: 0.5 * x[:, :nF], s, faces, nq=nq, rational=rat).assemble_vector(V))
        rec("BoundaryLoadForm/traction_numbers", case, rat, lambda: F.BoundaryLoadForm(np.arange(nF) + 1.0, s, faces, nq=nq, rational=rat).assemble_vector(V))
        rec("BoundaryLoadForm/pressure", case, rat, lambda: F.BoundaryLoadForm.pressure(lambda x: 1.0 + x[:, 0], s, faces, nq, rat).assemble_vector(V))
    if d == 2 and nsd == 3:
        s = spline_of(name, weighted, 3)
        V = s.V
        u = function(V, rng, 0.01)
        svk = F.KirchhoffLoveSVK(1.0e3, 0.3, 0.05)
        for key, law, on_device in (("device_law", svk, True), ("host_method", svk, False), ("host_law", HostLaw(svk), True)):
            res = F.ShellResidual(u, s, law, body_force=[0.0, 0.0, -1.0], nq=nq, rational=rat, device_law=on_device)
            tan = res.tangent()
            rec("ShellResidual/" + key, case, rat, lambda: res.assemble_vector(V))
            rec("ShellResidual.tangent/" + key, case, rat, lambda: tan.assemble_matrix(V), lambda: tan.symmetric)
            rec("ShellResidual.tangent.block/" + key, case, rat, lambda: tan.assemble_block(V, 2, 1))
            rec("ShellResidual.energy/" + key, case, rat, lambda: res.energy(V))


def refusals(rec):
    case = "refusals"
    s1, s2, s3 = spline_of("plane_p2_nq2", False, 1), spline_of("plane_p2_nq2", False, 2), spline_of("volume_p2", False, 3)
    surf = spline_of("surface_p2", False, 3)
    n1, npts = s1.V.dim(), s1.quadraturePoints().npts
    kv = [np.asarray(B.uniformKnots(2, 0.0, 1.0, 3), dtype=np.float64)] * 2
    lst = t.ExtractedSpline(t.FieldListSpline(B.ExplicitBSplineControlMesh([2, 2], kv), [B.BSpline([2, 2], kv)]), 4)
    u2 = t.Function(s2.V)
    calls = {
        "geometry_none/CoefficientForm": lambda: F.CoefficientForm(None, diffusion=1.0),
        "geometry_none/VectorCoefficientForm": lambda: F.VectorCoefficientForm(None, np.zeros((2, 2, 2, 2))),
        "geometry_none/VectorJetLoadForm": lambda: F.VectorJetLoadForm(np.zeros((2, 6)), None),
        "geometry_none/ShellResidual": lambda: F.ShellResidual(u2, None, F.KirchhoffLoveSVK(1.0, 0.3, 0.1)),
        "row_blocks/CoefficientForm": lambda: F.CoefficientForm(s1, diffusion=1.0).assemble_matrix(s1.V, 0, n1 // 2),
        "row_blocks/QuadratureLoadForm": lambda: F.QuadratureLoadForm(1.0, s1).assemble_vector(s1.V, 0, n1 // 2),
        "row_blocks/HyperelasticResidual.tangent": lambda: F.HyperelasticResidual(u2, s2, F.NeoHookean(1.0, 1.0)).tangent().assemble_matrix(s2.V, 0, n1),
        "row_blocks/VectorJetCoefficientForm": lambda: F.VectorJetCoefficientForm(s2, np.zeros((2, 6, 2, 6))).assemble_matrix(s2.V, 0, n1),
        "row_blocks/ShellResidual.tangent": lambda: F.ShellResidual(t.Function(surf.V), surf, F.KirchhoffLoveSVK(1.0, 0.3, 0.1)).tangent().assemble_matrix(surf.V, 0, 3),
        "fields/CoefficientForm_on_two_fields": lambda: F.CoefficientForm(s2, diffusion=1.0).assemble_matrix(s2.V),
        "fields/VectorCoefficientForm_on_one_field": lambda: F.VectorCoefficientForm(s1, np.zeros((2, 2, 2, 2))).assemble_matrix(s1.V),
        "fields/HyperelasticResidual_on_a_surface": lambda: F.HyperelasticResidual(t.Function(surf.V), surf, F.NeoHookean(1.0, 1.0)).assemble_vector(surf.V),
        "fields/JetCoefficientForm_on_two_fields": lambda: F.JetCoefficientForm(s2, np.zeros((npts, 6, 6))).assemble_matrix(s2.V),
        "fields/ShellResidual_in_the_plane": lambda: F.ShellResidual(u2, s2, F.KirchhoffLoveSVK(1.0, 0.3, 0.1)).assemble_vector(s2.V),
        "d3/VectorJetCoefficientForm": lambda: F.VectorJetCoefficientForm(s3, np.zeros((3, 6, 3, 6))).assemble_matrix(s3.V),
        "d3/geometryJetsAtQuadrature": lambda: s3.geometryJetsAtQuadrature(),
        "field_list/CoefficientForm": lambda: F.CoefficientForm(lst, diffusion=1.0).assemble_matrix(lst.V),
        "field_list/quadraturePoints": lambda: lst.quadraturePoints(),
        "field_list/evaluateJetsAtQuadrature": lambda: lst.evaluateJetsAtQuadrature(np.zeros(lst.V.dim())),
        "shape/diffusion": lambda: F.CoefficientForm(s1, diffusion=np.zeros((npts, 2, 3))).assemble_matrix(s1.V),
        "shape/velocity": lambda: F.CoefficientForm(s1, velocity=np.zeros((npts, 3))).assemble_matrix(s1.V),
        "shape/tangent": lambda: F.VectorCoefficientForm(s2, np.zeros((npts, 2, 2, 2))).assemble_matrix(s2.V),
        "shape/flux": lambda: F.VectorLoadForm(None, s2, flux=np.zeros((npts, 2))).assemble_vector(s2.V),
        "shape/jet_load": lambda: F.VectorJetLoadForm(np.zeros((npts, 2, 5)), s2).assemble_vector(s2.V),
        "shape/traction": lambda: F.BoundaryLoadForm(lambda x: np.zeros((x.shape[0], 3)), s2, [(0, 0)]).assemble_vector(s2.V),
        "length/diffusion": lambda: F.CoefficientForm(s1, diffusion=dev.DeviceVector(npts + 1)).assemble_matrix(s1.V),
        "length/velocity": lambda: F.CoefficientForm(s1, velocity=dev.DeviceVector(npts)).assemble_matrix(s1.V),
        "length/tangent": lambda: F.VectorCoefficientForm(s2, dev.DeviceVector(npts)).assemble_matrix(s2.V),
        "length/reaction": lambda: F.VectorCoefficientForm(s2, np.zeros((2, 2, 2, 2)), reaction=dev.DeviceVector(npts)).assemble_matrix(s2.V),
        "length/flux": lambda: F.VectorLoadForm(None, s2, flux=dev.DeviceVector(npts)).assemble_vector(s2.V),
        "length/jet_data": lambda: F.VectorJetCoefficientForm(s2, dev.DeviceVector(npts)).assemble_matrix(s2.V),
        "length/state": lambda: F.HyperelasticResidual(dev.DeviceVector(3), s2, F.NeoHookean(1.0, 1.0)).assemble_vector(s2.V),
        "law/quasilinear_returns_one": lambda: F.QuasilinearResidual(t.Function(s1.V), s1, lambda x, u, g: None, None).assemble_vector(s1.V),
        "law/host_returns_two": lambda: F.HyperelasticResidual(u2, s2, HostLaw(type("L", (), {"host": staticmethod(lambda Fq: (Fq, Fq))}))).assemble_vector(s2.V),
        "law/host_shapes": lambda: F.HyperelasticResidual(u2, s2, HostLaw(type("L", (), {"host": staticmethod(lambda Fq: (Fq, Fq, Fq))}))).assemble_vector(s2.V),
        "block/VectorCoefficientForm": lambda: F.VectorCoefficientForm(s2, np.zeros((2, 2, 2, 2))).assemble_block(s2.V, 2, 0),
    }
    for key, call in calls.items():
        rec("refusal/" + key, case, False, call)


# ---- the hyperelastic shell with a follower pressure, and the laws under a time integrator.  These lines follow the refusals:
# the lines above keep their places.  No law may refuse a state here (``strict``), and a plane cuts through the points.
SHELL_LAW, SHELL_NOISE, SOLID_NOISE = (1.0e3, 0.05), 0.002, 0.01
DT, RHO_INF, DAMPING, STIFFNESS = 0.01, 0.5, 0.3, 1.0e4
# (unit normal, offset): n . X < offset on about half of the patch
PLANES = {"strip_p2_2x2": ((0.0, 0.0, 1.0), 0.75), "plane_p2_nq2": ((1.0, 0.0), 0.5), "volume_p2": ((1.0, 0.0, 0.0), 0.6)}


def seeded(V, seed, scale):
    u = t.Function(V)
    u.vector().set_local(scale * np.random.default_rng(seed).standard_normal(V.dim()))
    return u


def hyper_shell_forms(rec, case, weighted, rat):
    s = spline_of("strip_p2_2x2", weighted, 3)
    V = s.V
    u = seeded(V, 7, SHELL_NOISE)
    law = F.KirchhoffLoveHyper(*SHELL_LAW)
    for key, on_device, pressure in (("device_law/number", True, 40.0), ("device_law/callable", True, lambda: 40.0),
                                     ("host_method/number", False, 40.0), ("host_method/callable", False, lambda: 40.0)):
        res = F.ShellResidual(u, s, law, body_force=[0.0, 0.0, -1.0], rational=rat, device_law=on_device, pressure=pressure)
        tan = res.tangent()
        rec("ShellResidual/hyper/" + key, case, rat, lambda: res.assemble_vector(V), strict=True)
        rec("ShellResidual.tangent/hyper/" + key, case, rat, lambda: tan.assemble_matrix(V), lambda: tan.symmetric, strict=True)
        rec("ShellResidual.tangent.block/hyper/" + key, case, rat, lambda: tan.assemble_block(V, 2, 1), strict=True)
        rec("ShellResidual.energy/hyper/" + key, case, rat, lambda: res.energy(V), strict=True)


def integrator_of(V, y, scheme, seed, scale):
    """an integrator on a seeded old state whose rates have the sizes a step of DT gives them"""
    from tigar_amd import timeIntegration as TI
    yo, vo, ao = seeded(V, seed + 1, scale), seeded(V, seed + 2, scale / DT), seeded(V, seed + 3, scale / DT ** 2)
    if scheme == "backward_euler":
        return TI.BackwardEulerIntegrator(DT, y, [yo, vo])
    return TI.GeneralizedAlphaIntegrator(RHO_INF, DT, y, [yo, vo, ao])


def dynamic_lines(rec, key, case, rat, V, static, it, plane, npts, block):
    """what a ``DynamicResidual`` gives: residual, tangent, one block, mass, energies, the active points, and the residual of
    the next step"""
    contact = F.PlanePenalty(plane[0], plane[1], STIFFNESS) if plane is not None else None
    dyn = F.DynamicResidual(static, it, 1.5, mass_damping=DAMPING, contact=contact)
    tan = dyn.tangent()

    def active():
        n = dyn.active_points()
        assert contact is None or 0 < n < npts, "%s, %s: %d of %d points are active" % (key, case, n, npts)
        return float(n)
    energies = lambda: [dyn.energy(V)[part] for part in ("strain", "kinetic", "contact", "total")]
    rec("DynamicResidual/" + key, case, rat, lambda: dyn.assemble_vector(V), strict=True)
    rec("DynamicResidual.active_points/" + key, case, rat, active, strict=True)
    rec("DynamicResidual.tangent/" + key, case, rat, lambda: tan.assemble_matrix(V), lambda: tan.symmetric, strict=True)
    rec("DynamicResidual.active_points.tangent/" + key, case, rat, active, strict=True)
    rec("DynamicResidual.tangent.block/" + key, case, rat, lambda: tan.assemble_block(V, *block), strict=True)
    rec("DynamicResidual.mass_form/" + key, case, rat, lambda: dyn.mass_form().assemble_matrix(V), strict=True)
    rec("DynamicResidual.energy/" + key, case, rat, energies, strict=True)
    it.advance()
    rec("DynamicResidual.advanced/" + key, case, rat, lambda: dyn.assemble_vector(V), strict=True)
    return dyn


def dynamic_forms(rec, name, case, weighted, rat):
    p, nels, nsd, nq = PATCHES[name]
    npts = spline_of(name, weighted, 1).quadraturePoints(nq).npts
    plane = PLANES[name]
    if name.startswith("strip"):
        s = spline_of(name, weighted, 3)
        V = s.V
        for key, law, on_device, scheme in (("hyper_device_law", F.KirchhoffLoveHyper(*SHELL_LAW), True, "generalized_alpha"),
                                            ("svk_device_law", F.KirchhoffLoveSVK(1.0e3, 0.3, 0.05), True, "generalized_alpha"),
                                            ("hyper_host_method", F.KirchhoffLoveHyper(*SHELL_LAW), False, "generalized_alpha"),
                                            ("hyper_backward_euler", F.KirchhoffLoveHyper(*SHELL_LAW), True, "backward_euler")):
            y = seeded(V, 20, SHELL_NOISE)
            it = integrator_of(V, y, scheme, 20, SHELL_NOISE)
            static = F.ShellResidual(y, s, law, body_force=lambda x: 0.5 * x, rational=rat, device_law=on_device,
                                     pressure=lambda: 40.0 * (1.0 + it.t))                          # (read at every assembly)
            dynamic_lines(rec, key, case, rat, V, static, it, plane, npts, (2, 1))
        return
    s = spline_of(name, weighted, nsd)
    V = s.V
    for key, law, scheme in (("NeoHookean", F.NeoHookean(2.0, 1.0), "generalized_alpha"),
                             ("host_law", HostLaw(F.StVenantKirchhoff(2.0, 1.0)), "generalized_alpha"),
                             ("StVenantKirchhoff_backward_euler", F.StVenantKirchhoff(2.0, 1.0), "backward_euler")):
        y = seeded(V, 30, SOLID_NOISE)
        static = F.HyperelasticResidual(y, s, law, body_force=lambda x: 0.1 * x[:, :nsd], nq=nq, rational=rat)
        dynamic_lines(rec, key, case, rat, V, static, integrator_of(V, y, scheme, 30, SOLID_NOISE), plane, npts, (1, 0))


def reference_states(rec):
    """the assembled cases of tests/dynamics_reference.py: their patches, laws, states and planes"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dynamics_reference as DR
    from tigar_amd import timeIntegration as TI
    for name in ("cylinder-svk", "cylinder-hyper", "block", "annulus"):
        c = DR.assembled_case(name, dtypes=(np.float64,))
        pb, info, ref = c["pb"], DR.CASES[name], c["dyn"][0]
        d = len(pb["kvs"])
        s = t.ExtractedSpline(t.EqualOrderSpline(ref.nF, N.NURBSControlMesh([pb["p"]] * d, pb["kvs"], pb["C"])), 2 * pb["p"])
        V = s.V
        fs = []
        for v in [c["y"]] + list(c["old"]):
            fs.append(t.Function(V))
            fs[-1].vector().set_local(np.asarray(v, dtype=np.float64))
        if info["kind"] == "shell":
            static = F.ShellResidual(fs[0], s, c["material"], rational=c["rational"], pressure=info["pressure"])
        else:
            static = F.HyperelasticResidual(fs[0], s, c["material"], rational=c["rational"])
        it = TI.GeneralizedAlphaIntegrator(DR.CASE_RHO_INF, DR.CASE_DT, fs[0], fs[1:])
        n, off, _ = c["plane"]
        dynamic_lines(rec, name, "dynamics_reference", c["rational"], V, static, it, (n, off), ref.wdet.size, (1, 0))


def dynamic_refusals(rec):
    from tigar_amd import timeIntegration as TI
    s = spline_of("strip_p2_2x2", False, 3)
    V = s.V
    y = t.Function(V)
    static = F.ShellResidual(y, s, F.KirchhoffLoveSVK(1.0e3, 0.3, 0.05))
    it = integrator_of(V, y, "generalized_alpha", 40, SHELL_NOISE)
    other = integrator_of(V, t.Function(V), "generalized_alpha", 41, SHELL_NOISE)
    calls = {
        "static/LaplaceForm": lambda: F.DynamicResidual(F.LaplaceForm(), it, 1.0),
        "density/zero": lambda: F.DynamicResidual(static, it, 0.0),
        "density/negative": lambda: F.DynamicResidual(static, it, -1.0),
        "integrator/first_order": lambda: F.DynamicResidual(static, TI.GeneralizedAlphaIntegrator(0.5, DT, y, [t.Function(V), t.Function(V)]), 1.0),
        "integrator/first_order_backward_euler": lambda: F.DynamicResidual(static, TI.BackwardEulerIntegrator(DT, y, [t.Function(V)]), 1.0),
        "integrator/load_stepper": lambda: F.DynamicResidual(static, TI.LoadStepper(DT), 1.0),
        "integrator/another_unknown": lambda: F.DynamicResidual(static, other, 1.0),
        "contact/normal_in_the_plane": lambda: F.DynamicResidual(static, it, 1.0, contact=F.PlanePenalty((1.0, 0.0), 0.0, 1.0)),
        "contact/numbers": lambda: F.DynamicResidual(static, it, 1.0, contact=(0.0, 0.0, 1.0)),
        "row_blocks/residual": lambda: F.DynamicResidual(static, it, 1.0).assemble_vector(V, 0, 3),
        "row_blocks/tangent": lambda: F.DynamicResidual(static, it, 1.0).tangent().assemble_matrix(V, 0, 3),
        "row_blocks/mass_form": lambda: F.DynamicResidual(static, it, 1.0).mass_form().assemble_matrix(V, 0, 3),
    }
    for key, call in calls.items():
        rec("refusal/DynamicResidual/" + key, "refusals", False, call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forms_digest.jsonl"))
    args = ap.parse_args()
    dev.device_info()
    with open(args.out, "w") as f:
        rec = Recorder(f)
        for name in PATCHES:
            for weighted in ((False,) if name.startswith("strip") else (False, True)):
                for rat in (False, True):
                    case = name + ("_weighted" if weighted else "")
                    for group in ((vector_forms,) if name.startswith("strip") else (scalar_forms, vector_forms)):
                        # (what a group cannot even set up on this patch is a line too, and must stay one)
                        rec(group.__name__, case, rat, lambda: group(rec, name, case, weighted, rat))
        refusals(rec)
        for weighted in (False, True):
            for rat in (False, True):
                hyper_shell_forms(rec, "strip_p2_2x2" + ("_weighted" if weighted else ""), weighted, rat)
                for name in ("strip_p2_2x2", "plane_p2_nq2", "volume_p2"):
                    dynamic_forms(rec, name, name + ("_weighted" if weighted else ""), weighted, rat)
        reference_states(rec)
        dynamic_refusals(rec)
    print("forms_digest: %d lines -> %s" % (rec.lines, args.out))


if __name__ == "__main__":
    main()
