"""GPU: every row of the route table of the sum-factorised element kernels (csrc/tg_assemble.hip, ``g_asf_routes``) runs.

One case per instantiation, 37 in all.  A case sets the switches that select its row by the rules of DESIGN.md ("Mapped
forms: request, plan, route table"), and checks that
  * the suffix of the library's timing line (TIGAR_ASM_TIME) names the expected kernel,
  * a second run gives the same bits,
  * the result agrees with the plain kernel (TIGAR_ASM_LEGACY=1, ``k_assemble_mapped`` / ``k_coef_matrix``) on the same
    operands, to the bound the existing route test of the form uses: 1e-12 max|.| for the matrices (tests/test_gpu_assembly.py,
    tests/test_gpu_mapped_elasticity.py) and the load (tests/test_gpu_rational.py); for the point-coefficient rows the bound of
    ``test_sum_factorised_route_and_plain_kernel`` in tests/test_gpu_coef.py (8 x the float64 error of the reference of the
    case, at least 32 eps, of max|reference|).

Shapes, on the rational volume map of geom_util: p = 3: 5 x 2 x 2 elements (a group of four and a group of one, two elements
across: both colours, shared faces); p = 2: 3 x 2 x 2, the walks with TIGAR_ASM_CHUNK=2 (a seam between pieces); p = 1: 3 x 2 x 2.
"""
import re

import numpy as np
import pytest

from geom_util import rational_volume
import coef_reference as CR
import test_gpu_coef as TC

pytestmark = pytest.mark.gpu

LAM, MU = 1.3, 0.7
NELS = {1: (3, 2, 2), 2: (3, 2, 2), 3: (5, 2, 2)}
EPW = {1: 8, 2: 2, 3: 1}
FORMS = ("mass", "laplace", "elasticity")           # FORM 0, 1, 2 of the kernels


@pytest.fixture(scope="module")
def T():
    import tigar_amd
    from tigar_amd import BSplines, forms, device, NURBS, common
    device.device_info()

    class NS:
        pass
    ns = NS()
    ns.t, ns.B, ns.F, ns.dev, ns.N, ns.c = tigar_amd, BSplines, forms, device, NURBS, common
    return ns


def _rows():
    """(kernel name as the library prints it, p, form, variant, switches): the rules of the chooser, row by row"""
    rows = []
    for p in (1, 2, 3):
        p1, e = p + 1, EPW[p]
        seam = {"TIGAR_ASM_CHUNK": "2"} if p == 2 else {}
        rows.append(("k_asf3_load<%d,%d>" % (p1, e), p, "load", "plain", {}))
        for f, form in enumerate(FORMS):
            stiff = f > 0
            walks = p == 2 or (p == 3 and not stiff)          # the default
            rows.append(("k_asf3<%d,%d,%d>" % (p1, e, f), p, form, "plain", dict(seam, **({} if walks else {"TIGAR_ASM_WALK": "1"}))))
            if p == 3 and stiff:
                off = {"TIGAR_ASM_QUAD": "0"}
            else:
                off = {"TIGAR_ASM_WALK": "0"} if walks else {}
            rows.append(("k_asf3_elem<%d,%d,%d>" % (p1, e, f), p, form, "plain", off))
    for f in (1, 2):
        rows.append(("k_asf3_quad<4,%d,1,1>" % f, 3, FORMS[f], "plain", {}))
        rows.append(("k_asf3_quad<4,%d,1,0>" % f, 3, FORMS[f], "plain", {"TIGAR_ASM_QUAD_CHUNK": "1"}))
        rows.append(("k_asf3_quad<4,%d,0,0>" % f, 3, FORMS[f], "plain", {"TIGAR_ASM_QUAD_CHUNK": "1", "TIGAR_ASM_PRE": "0"}))
    for p in (2, 3):
        p1, e = p + 1, EPW[p]
        seam = {"TIGAR_ASM_CHUNK": "2"} if p == 2 else {}
        rows.append(("k_asf3_load<%d,%d>" % (p1, e | 16), p, "load", "rational", {}))
        rows.append(("k_asf3<%d,%d,4>" % (p1, e), p, "mass", "rational", seam))
    rows.append(("k_asf3<3,2,5>", 2, "laplace", "rational", {"TIGAR_ASM_CHUNK": "2"}))
    rows.append(("k_asf3<3,2,9>", 2, "laplace", "coef", {"TIGAR_ASM_CHUNK": "2"}))
    for v, variant in ((5, "rational"), (9, "coef")):
        rows.append(("k_asf3_quad<4,%d,1,1>" % v, 3, "laplace", variant, {}))
        rows.append(("k_asf3_quad<4,%d,1,0>" % v, 3, "laplace", variant, {"TIGAR_ASM_QUAD_CHUNK": "1"}))
    return rows


ROWS = _rows()
assert len(ROWS) == 37 and len(set(r[0] for r in ROWS)) == 37

_PATCH = {}


def _patch(T, p):
    """the patch of degree p, its operands and (point coefficients) the reference bound: built once"""
    if p not in _PATCH:
        kvs, C = rational_volume(p, NELS[p])
        gen = T.t.EqualOrderSpline(T.c.selfcomm, 1, T.N.NURBSControlMesh([p] * 3, kvs, C))
        g = gen.V.grids[0]
        uks = [np.asarray(g.vertices[k], dtype=np.float64) for k in range(3)]
        cp = [np.asarray(f.vector().get_local(), dtype=np.float64) for f in gen.cpFuncs]
        assert np.ptp(cp[-1]) > 0.05                                    # the weights do vary
        _PATCH[p] = dict(p=p, nq=None, uks=uks, cp=cp, fn=np.sin(3.0 * cp[0]) + cp[1], legacy={})
    return _PATCH[p]


def _coefs(c):
    """random point coefficients as in tests/test_gpu_coef.py: A, b, c, m per point"""
    if "coefs" not in c:
        rng = np.random.default_rng(37 + c["p"])
        npts, nsd = int(np.prod(NELS[c["p"]])) * (c["p"] + 1) ** 3, 3
        c["coefs"] = (rng.standard_normal((npts, nsd, nsd)), rng.standard_normal((npts, nsd)), rng.standard_normal((npts, nsd)),
                      rng.standard_normal(npts))
    return c["coefs"]


def _coef_tol(c):
    """the bound of tests/test_gpu_coef.py for these coefficients, times the scale it is relative to"""
    if "coef_tol" not in c:
        ref, ref64 = (CR.CoefReference(c["uks"], c["p"], c["cp"], None, rational=True, **kw) for kw in ({}, {"dtype": np.float64}))
        assert ref.npts == _coefs(c)[3].size and ref.nsd == 3
        _, _, scale, bound, _ = TC._bound_of(ref, ref64, "matrix", *_coefs(c))
        c["coef_tol"] = bound * scale
    return c["coef_tol"]


def _run(T, c, dcp, form, variant):
    """-> list of arrays (the values of every output of the case)"""
    a = (c["uks"], c["p"], dcp)
    rat = variant == "rational"
    if variant == "coef":
        return [TC._gpu_matrix(T, c, dcp, _coefs(c), True).to_scipy().data]
    if form == "load":
        return [T.dev.assemble_mapped_load(*a, T.dev.DeviceVector(data=c["fn"]), rational=rat).get_local()]
    if form == "elasticity":
        return [T.dev.assemble_mapped_elasticity_block(*a, i, j, LAM, MU, rational=rat).to_scipy().data for i, j in ((0, 1), (2, 2))]
    return [T.dev.assemble_mapped_matrix(*a, form, rational=rat).to_scipy().data]


@pytest.mark.parametrize("kernel,p,form,variant,env", ROWS, ids=[r[0] for r in ROWS])
def test_every_row_of_the_route_table_runs(T, kernel, p, form, variant, env, monkeypatch, capfd):
    c = _patch(T, p)
    dcp = [T.dev.DeviceVector(data=v) for v in c["cp"]]
    if (form, variant) not in c["legacy"]:                             # the plain kernel: once per (degree, form, variant)
        with monkeypatch.context() as m:
            m.setenv("TIGAR_ASM_LEGACY", "1")
            c["legacy"][form, variant] = _run(T, c, dcp, form, variant)
    want = c["legacy"][form, variant]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    monkeypatch.setenv("TIGAR_ASM_TIME", "1")
    capfd.readouterr()
    got = _run(T, c, dcp, form, variant)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[tg_assemble] form")]
    monkeypatch.delenv("TIGAR_ASM_TIME")
    assert len(lines) == len(got), lines
    for ln in lines:
        m = re.search(r"element kernels ([0-9.]+) ms \(([a-z-]+)\)(.*)$", ln)
        assert m and m.group(2) == "sum-factorised" and m.group(3) == " " + kernel, ln
    again = _run(T, c, dcp, form, variant)
    for g, g2, w in zip(got, again, want):
        assert np.array_equal(g.view(np.int64), g2.view(np.int64))
        assert g.shape == w.shape
        tol = _coef_tol(c) if variant == "coef" else 1e-12 * np.max(np.abs(w))
        err = float(np.max(np.abs(g - w)))
        print("%s p=%d %s %s: |route - plain kernel| = %.3e, bound %.3e" % (kernel, p, form, variant, err, tol))
        assert err <= tol
