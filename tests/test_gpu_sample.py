"""GPU: evaluation at caller-chosen points, closest points and lattice sampling (csrc/tg_sample.hip, the lattice entries of
csrc/tg_postproc.hip) against the longdouble reference of tests/sample_reference.py, and what is built on them:
ExtractedSpline.evaluateAtPoints / physicalPoints / locatePoints / evaluateAtPhysicalPoints / latticePoints /
evaluateAtLattice / writeVTK, tigar_amd.File, Function.rename / name / split.

Elementwise bounds c eps magnitude, the magnitudes from the reference (first-order propagation, every 1-D value entering as
|l| + delta |l'| with delta = 4 eps (1 + (|xi_k| + |v_e|) / h_k): the rounded nodes m / p and the rounding of t = (xi - v) / h).
The constants count the longest chain of roundings of k_point_eval (``sample_reference.constants``):

  table entry        t = 7 p + 4     z = p t as a sum of two doubles (two exact differences, a division with its exact remainder,
                                     the product with p: 6 roundings that reach a factor only at second order); l_a = c_a
                                     prod (z - m): p factors of 2 roundings ((z_hi - m) + z_lo) and their products (p), c_a = 1 /
                                     prod (a - m), an integer's reciprocal, and the product with it: 3 p + 2; l_a': p such terms,
                                     their sum and the factor p: 4 p + 2 <= 7 p + 4.  Next to a Lagrange node the factor that
                                     vanishes there keeps its RELATIVE accuracy (with t rounded to one double its error eps |l'|
                                     is of first order and no multiple of |l| + delta |l'|, delta = O(eps), covers it: measured
                                     2.9 x the bound one ulp inside an end at p = 1 before t was kept in two doubles)
  field at a point   cN = d (t + p + 1)   per direction one table factor and p + 1 fused multiply-adds
  x = N_i / W        cN + 2          a quotient of two fields
  gradient           cN + 24         DF = (dN W - N dW) / W^2: 4, g = DF^T DF: nsd + 1 <= 4, the inverse: 3 + 4 + 1, g^-1 grad_xi u
                                     and DF times it: d + 1 each (the count of tests/test_gpu_postproc.py)
  rational value     cN + 2          u_h / W_h
  rational gradient  cN + 30         the quotient rule before the Cartesian gradient: the fused difference, 1 / W, its square, two
                                     products and the product u dW: 6

The lattice entry points run the kernel of the Gauss points: the constants of ``postproc_reference.constants`` carry over.

Closest points: the conditions of the issue hold for the reference alone (tests/test_sample_reference_host.py); here the
device's iteration counts equal the reference's +- 1, every status is the reference's, and xi agrees within
range_k tol rho / (1 - rho) + 2 |(DF^T DF)^-1 DF^T|_row k |bound of x| (rho: the reference's last step ratio, 0 for round trips)
+ 2 eps |xi_k|: the device stores xi as a double and the reference's longdouble xi is rounded to one for the comparison.
Round trips: at most 5 iterations from all seeds, 6 from seven seeds and 8 from one on the 7 x 7 annulus, per case.
"""
import os

import numpy as np
import pytest

from oracle import tigar_oracle as O
import postproc_reference as R
import sample_reference as S
import vtk_reader as V

pytestmark = pytest.mark.gpu

EPS = R.EPS
LD = np.longdouble
GRID_CAP = 1024          # workgroups of a launch (include/tigar_hip.h): 256 lanes each for p <= 4, 64 beyond
_WORST = {}


@pytest.fixture(scope="module")
def T():
    import tigar_amd
    from tigar_amd import BSplines, forms, device, NURBS, vtkio
    device.device_info()

    class NS:
        pass
    ns = NS()
    ns.t, ns.B, ns.F, ns.dev, ns.N, ns.vtk = tigar_amd, BSplines, forms, device, NURBS, vtkio
    return ns


def _graded(nels, p, seed, nsd=None):
    """graded (non-uniform) element vertices and a smooth non-affine rational map on the Q_p nodes"""
    d = len(nels)
    rng = np.random.default_rng(seed)
    uks = []
    for k in range(d):
        steps = rng.uniform(0.4, 1.6, nels[k]) * np.linspace(1.0, 2.0, nels[k])
        uks.append(0.125 * k + np.concatenate([[0.0], np.cumsum(steps) / np.sum(steps) * (1.0 + 0.5 * k)]))
    X = R.lagrange_nodes(uks, p)
    wgt = 1.0 + 0.2 * X[0] * X[-1]
    coords = [X[i] + 0.1 * X[(i + 1) % d] ** 2 for i in range(d)]
    if nsd is not None and nsd > d:
        coords.append(X[0] ** 2 + 0.5 * X[-1])
    return uks, [c * wgt for c in coords] + [wgt]


def _lifted_annulus(nel):
    uks, cp = R.annulus_patch(nel)
    x, y = cp[0] / cp[2], cp[1] / cp[2]
    return uks, [cp[0], cp[1], 0.4 * x * y * cp[2], cp[2]]


CASES = {
    "1d_p1_7": lambda: (1,) + _graded((7,), 1, 1),
    "1d_p2_3": lambda: (2,) + _graded((3,), 2, 2),
    "1d_p3_5": lambda: (3,) + _graded((5,), 3, 3),
    "1d_p4_2": lambda: (4,) + _graded((2,), 4, 4),
    "1d_p8_2_generic": lambda: (8,) + _graded((2,), 8, 5),
    "curve_in_the_plane_p2_4": lambda: (2,) + _graded((4,), 2, 6, nsd=2),
    "2d_p1_3x2": lambda: (1,) + _graded((3, 2), 1, 7),
    "2d_p2_5x4": lambda: (2,) + _graded((5, 4), 2, 8),
    "2d_p3_2x3": lambda: (3,) + _graded((2, 3), 3, 9),
    "2d_p4_2x2": lambda: (4,) + _graded((2, 2), 4, 10),
    "2d_p5_2x2_generic": lambda: (5,) + _graded((2, 2), 5, 11),
    "2d_p2_1x7": lambda: (2,) + _graded((1, 7), 2, 12),
    "2d_p3_single_element": lambda: (3,) + _graded((1, 1), 3, 13),
    "quarter_annulus_4": lambda: (2,) + R.annulus_patch(4),
    "lifted_annulus_surface_in_space": lambda: (2,) + _lifted_annulus(4),
    "3d_p1_2x3x2": lambda: (1,) + _graded((2, 3, 2), 1, 14),
    "3d_p2_3x2x2": lambda: (2,) + _graded((3, 2, 2), 2, 15),
    "3d_p3_2x1x2": lambda: (3,) + _graded((2, 1, 2), 3, 16),
    "3d_p4_1x2x1": lambda: (4,) + _graded((1, 2, 1), 4, 17),
    "3d_single_element_p2": lambda: (2,) + _graded((1, 1, 1), 2, 18),
    "rational_volume_p2_2x3x2": lambda: (2,) + R.volume_patch(2, (2, 3, 2)),
}
COUNTS = (0, 1, 63, 64, 65, 257)
_REF = {}


def _points(uks, p, n, rng):
    """n parametric points: on interior vertices, on the first and the last, on Lagrange nodes, one ulp inside and outside
    each end, NaN and +-inf, the rest random; shuffled.  Neighbours of the special ones are ordinary points."""
    d = len(uks)
    xi = np.stack([rng.uniform(u[0], u[-1], n) for u in uks], axis=1)
    at = iter(rng.permutation(n))
    nodes = [np.unique(np.concatenate([u[:-1, None] + np.diff(u)[:, None] * (np.arange(p + 1) / float(p))[None, :]]).ravel()) for u in uks]
    for k in range(d):
        u = uks[k]
        special = list(u) + list(nodes[k][:6]) + [np.nextafter(u[0], 9.0), np.nextafter(u[-1], -9.0), np.nextafter(u[0], -9.0),
                                                   np.nextafter(u[-1], 9.0), np.nan, np.inf, -np.inf]
        for s in special:
            xi[next(at), k] = s
    q = next(at)
    xi[q] = [u[0] for u in uks]                       # corners
    q = next(at)
    xi[q] = [u[-1] for u in uks]
    return xi


def _case(name):
    if name not in _REF:
        p, uks, cp = CASES[name]()
        P = S.Patch(uks, p, cp)
        rng = np.random.default_rng(len(name))
        xi = _points(P.uks, p, 257, rng)
        u = rng.standard_normal((3, P.nnodes))
        _REF[name] = dict(p=p, uks=uks, cp=cp, P=P, xi=xi, u=u, c=S.constants(P.d, p, P.nsd),
                          plain=P.eval(xi, u), rational=P.eval(xi, u, rational=True))
    return _REF[name]


def _dcp(T, c):
    return [T.dev.DeviceVector(data=v) for v in c["cp"]]


def _block(a):
    """[npts, ...] -> the component-major device layout"""
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(np.moveaxis(a, 0, -1)).ravel()


def _run(T, c, xi, nF=3, u=True, rational=False, x=True, val=True, grad=True):
    """(x [npts, nsd], val [npts, nF], grad [npts, nF, nsd]) of tg_point_eval, None where not asked for"""
    P = c["P"]
    npts = len(xi)
    dxi = T.dev.DeviceVector(data=_block(xi)) if npts else T.dev.DeviceVector(0)
    du = T.dev.DeviceVector(data=c["u"][:nF].ravel()) if u else None
    xo, vo, go = T.dev.point_eval(c["uks"], c["p"], _dcp(T, c), dxi, du, nF=nF, x=x, val=val, grad=grad, rational=rational)
    un = lambda v, shape: None if v is None else np.moveaxis(v.get_local().reshape(shape + (npts,)), -1, 0)
    return un(xo, (P.nsd,)), un(vo, (nF,)), un(go, (nF, P.nsd))


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def _held(name, what, got, ref, mag, const):
    """every entry of an inside point within const eps magnitude; returns the largest ratio to the bound"""
    err = np.abs(got - ref).astype(np.float64)
    bound = (const * EPS * mag).astype(np.float64)
    ratio = float(np.max(err / bound)) if err.size else 0.0
    print("point eval %-36s %-14s %.3f of the bound" % (name, what, ratio))
    _WORST[what] = max(_WORST.get(what, 0.0), ratio)
    assert np.all(err <= bound), (name, what, ratio)
    return ratio


@pytest.mark.parametrize("name", sorted(CASES))
def test_point_eval(T, name):
    c = _case(name)
    P, xi = c["P"], c["xi"]
    ok = c["plain"]["inside"]
    assert 0 < (~ok).sum() < len(ok) // 2
    full = {}
    for rational in (False, True):
        ref = c["rational" if rational else "plain"]
        x, val, grad = _run(T, c, xi, rational=rational)
        full[rational] = (x, val, grad)
        # outside points (NaN, +-inf, one ulp beyond an end): NaN in every output; nothing else is NaN
        for a in (x, val, grad):
            bad = np.isnan(a).reshape(len(xi), -1)
            assert np.array_equal(bad.any(axis=1), ~ok) and np.array_equal(bad.all(axis=1), ~ok)
        tag = "_rational" if rational else ""
        _held(name, "x", x[ok], ref["x"][ok], ref["x_mag"][ok], c["c"]["x"])
        _held(name, "val" + tag, val[ok], ref["val"][ok], ref["val_mag"][ok], c["c"]["val" + tag])
        _held(name, "grad" + tag, grad[ok], ref["grad"][ok], ref["grad_mag"][ok], c["c"]["grad" + tag])
        again = _run(T, c, xi, rational=rational)
        assert all(_bits(a, b) for a, b in zip(again, (x, val, grad)))                          # two runs: the same bits
    x, val, grad = full[False]
    assert _bits(full[True][0], x)                                                              # x does not depend on the flag
    # one field: the bits of field 0 of three; without u: x alone, the same bits; every subset of the outputs likewise
    x1, v1, g1 = _run(T, c, xi, nF=1)
    assert _bits(x1, x) and _bits(v1[:, 0], val[:, 0]) and _bits(g1[:, 0], grad[:, 0])
    xo, vo, go = _run(T, c, xi, u=False)
    assert _bits(xo, x) and vo is None and go is None
    assert _bits(_run(T, c, xi, x=False, grad=False)[1], val) and _bits(_run(T, c, xi, x=False, val=False)[2], grad)
    # a permutation of the points permutes every output bit for bit
    perm = np.random.default_rng(5).permutation(len(xi))
    xp, vp, gp = _run(T, c, xi[perm])
    assert _bits(xp, x[perm]) and _bits(vp, val[perm]) and _bits(gp, grad[perm])
    # the point counts: a point's result depends on that point alone, so a prefix of the points gives a prefix of the bits
    for n in COUNTS[:-1]:
        xn, vn, gn = _run(T, c, xi[:n])
        assert xn.shape == (n, P.nsd) and _bits(xn, x[:n]) and _bits(vn, val[:n]) and _bits(gn, grad[:n])


@pytest.mark.parametrize("name,lanes", [("2d_p2_5x4", 256), ("2d_p5_2x2_generic", 64), ("3d_p2_3x2x2", 256)])
def test_point_eval_beyond_the_grid_cap(T, name, lanes):
    """one count just above what the capped grid covers in one pass: the stride loop runs; the first and the last 256 points
    and a stride of the rest against the reference"""
    c = _case(name)
    P = c["P"]
    n = GRID_CAP * lanes + 257
    rng = np.random.default_rng(11)
    xi = np.stack([rng.uniform(u[0], u[-1], n) for u in P.uks], axis=1)
    xi[-1] = [u[-1] for u in P.uks]
    xi[GRID_CAP * lanes] = [u[0] for u in P.uks]                  # the first point of the second pass
    xi[GRID_CAP * lanes + 1, 0] = np.nan
    x, val, grad = _run(T, c, xi, nF=1)
    pick = np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n), np.arange(256, n - 256, max(1, (n - 512) // 200))]))
    ref = P.eval(xi[pick], c["u"][:1])
    ok = ref["inside"]
    assert not ok[list(pick).index(GRID_CAP * lanes + 1)] and ok.sum() == len(pick) - 1
    assert np.isnan(x[GRID_CAP * lanes + 1]).all() and np.isnan(val[GRID_CAP * lanes + 1]).all()
    assert np.isnan(x).any(axis=1).sum() == 1                     # every other point of the launch was written
    _held(name, "x", x[pick][ok], ref["x"][ok], ref["x_mag"][ok], c["c"]["x"])
    _held(name, "val", val[pick][ok], ref["val"][ok], ref["val_mag"][ok], c["c"]["val"])
    _held(name, "grad", grad[pick][ok], ref["grad"][ok], ref["grad_mag"][ok], c["c"]["grad"])


def test_point_eval_refusals(T):
    c = _case("2d_p2_5x4")
    dv = T.dev.DeviceVector
    cp, xi = _dcp(T, c), dv(data=np.full(10, 0.5))
    err = T.dev.TigarHipError
    with pytest.raises(ValueError, match="multiple of d"):
        T.dev.point_eval(c["uks"], 2, cp, dv(data=np.zeros(3)), None, x=True)
    with pytest.raises(err, match="nodal vector holds"):
        T.dev.point_eval(c["uks"], 2, cp, xi, dv(data=np.zeros(7)), nF=1)
    with pytest.raises(err, match="at least one field"):
        T.dev.point_eval(c["uks"], 2, cp, xi, dv(data=c["u"][0]), nF=0)
    with pytest.raises(err, match="local nodes exceed"):
        uks, cp3 = _graded((1, 1, 1), 5, 1)
        T.dev.point_eval(uks, 5, [dv(data=v) for v in cp3], dv(data=np.full(3, 0.5)), None, x=True)


# ---- lattices ----------------------------------------------------------------------------------------------------------------
LATTICE_CASES = ["1d_p3_5", "2d_p3_2x3", "quarter_annulus_4", "curve_in_the_plane_p2_4", "3d_p2_3x2x2", "2d_p2_1x7"]


def _same_element(P, t, xi):
    """where the location rule puts a lattice point into the element the lattice numbers it in (not so at t = 1 on an interior
    vertex, which belongs to the upper element)"""
    m, elem = len(t), np.arange(len(xi)) // len(t) ** P.d
    ok = np.ones(len(xi), dtype=bool)
    for k in range(P.d):
        ok &= S.element_of(P.uks[k], xi[:, k])[1] == elem % P.nel[k]
        elem = elem // P.nel[k]
    return ok


def _abscissae(m, ends):
    if ends:
        return np.array([0.0]) if m == 1 else np.linspace(0.0, 1.0, m)
    return (np.arange(m) + 0.5) / m


@pytest.mark.parametrize("ends", [True, False])
@pytest.mark.parametrize("name", LATTICE_CASES)
def test_lattice(T, name, ends):
    c = _case(name)
    P, p, u = c["P"], c["p"], c["u"][0]
    du = T.dev.DeviceVector(data=u)
    for m in sorted({1, 2, p + 1, 10}):
        t = _abscissae(m, ends)
        ref = S.lattice_reference(c["uks"], p, c["cp"], t)
        k = R.constants(P.d, p, m, P.nsd)
        x = T.dev.lattice_points(c["uks"], p, _dcp(T, c), t).get_local().reshape(P.nsd, ref.npts).T
        ex = np.abs(x - ref.x).astype(np.float64)
        assert np.all(ex <= k["x"] * EPS * ref.x_mag)
        xi = S.lattice_xi(c["uks"], t)
        cross = _run(T, c, xi, nF=1)
        pref = P.eval(xi, [u])
        same = _same_element(P, t, xi)
        assert same.all() or ends
        for rational in (False, True):
            if rational:
                # u_h / W_h and its Cartesian gradient (grad U - (U / W) grad W) / W from the plain reference of both functions on
                # the lattice, magnitudes by the product and quotient rules of postproc_reference
                (U, GU, UM, GUM), (W, GW, WM, GWM) = ref.eval(u), ref.eval(np.asarray(c["cp"][-1]))
                v, vm = U / W, UM / W + abs(U) / W * (WM / W)
                num = GU - v[:, None] * GW
                nm = GUM + vm[:, None] * abs(GW) + abs(v)[:, None] * GWM + abs(v[:, None] * GW)
                g, gm = num / W[:, None], nm / W[:, None] + abs(num / W[:, None]) * (WM / W)[:, None]
                kv, kg = c["c"]["val_rational"], c["c"]["grad_rational"]
            else:
                v, g, vm, gm = ref.eval(u)
                kv, kg = k["val"], k["grad"]
            val, grad = T.dev.lattice_eval(c["uks"], p, _dcp(T, c), t, du, grad=True, rational=rational)
            only = T.dev.lattice_eval(c["uks"], p, _dcp(T, c), t, du, rational=rational).get_local()
            val, grad = val.get_local(), grad.get_local().reshape(P.nsd, ref.npts).T
            assert _bits(only, val)
            ev, eg = np.abs(val - v).astype(np.float64), np.abs(grad - g).astype(np.float64)
            held = np.ones(len(xi), dtype=bool)
            print("lattice %s m %d ends %d rational %d: values %.3f of the bound, gradient %.3f" % (
                name, m, ends, rational, float(np.max(ev / (kv * EPS * vm))), float(np.max((eg / (kg * EPS * gm))[held]))))
            assert np.all(ev <= kv * EPS * vm) and np.all((eg <= kg * EPS * gm)[held])
            if not rational:
                # two kernels, one function: the lattice points fed to tg_point_eval agree within the sum of both bounds (the
                # gradient of a C0 function where both take it from the same element: on an interior vertex it is one-sided)
                assert np.all(np.abs(cross[0] - x) <= (k["x"] * EPS * ref.x_mag + c["c"]["x"] * EPS * pref["x_mag"]).astype(np.float64))
                assert np.all(np.abs(cross[1][:, 0] - val) <= (k["val"] * EPS * vm + c["c"]["val"] * EPS * pref["val_mag"][:, 0]).astype(np.float64))
                assert np.all((np.abs(cross[2][:, 0] - grad) <= (k["grad"] * EPS * gm + c["c"]["grad"] * EPS * pref["grad_mag"][:, 0]).astype(np.float64))[same])


def test_lattice_refusals(T):
    c = _case("2d_p2_5x4")
    err = T.dev.TigarHipError
    for t in ([0.5, 0.5], [0.2, 0.1], [-0.1, 0.5], [0.5, 1.5], np.linspace(0, 1, 11)):
        with pytest.raises(err, match="abscissae"):
            T.dev.lattice_points(c["uks"], 2, _dcp(T, c), np.asarray(t, dtype=np.float64))


# ---- closest points ----------------------------------------------------------------------------------------------------------
def _locate(T, c, x, guess=None, **kw):
    dv = T.dev.DeviceVector
    P = c["P"]
    n = len(x)
    xi, info = T.dev.point_locate(c["uks"], c["p"], _dcp(T, c), dv(data=_block(x)) if n else dv(0),
                                  None if guess is None else dv(data=_block(guess)), **kw)
    info = info.get_local().reshape(3, n)
    return xi.get_local().reshape(P.d, n).T, info[0], info[1].astype(int), info[2].astype(int)


def _compare_with_reference(name, c, x, got, res, tol):
    P = c["P"]
    xi, dist, iters, status = got
    rng = np.array([u[-1] - u[0] for u in P.uks])
    assert np.array_equal(status, [r[3] for r in res]), (name, status, [r[3] for r in res])
    ref_it = np.array([r[2] for r in res])
    assert np.all(np.abs(iters - ref_it) <= 1), (name, iters, ref_it)
    rxi = np.array([r[0] for r in res], dtype=np.float64).reshape(len(x), P.d)
    ev = P.eval(rxi)
    xb = np.sqrt(np.sum((2 * c["c"]["x"] * EPS * ev["x_mag"].astype(np.float64)) ** 2, axis=1))      # twice the bound of x, as a norm
    worst = 0.0
    for q, r in enumerate(res):
        rho = min(r[4], 0.999)
        bound = rng * tol * rho / (1.0 - rho) + r[5] * xb[q] + 2 * EPS * np.abs(rxi[q])
        assert np.all(np.abs(xi[q] - rxi[q]) <= bound), (name, q, xi[q], rxi[q], bound, r[2:5])
        worst = max(worst, float(np.max(np.abs(xi[q] - rxi[q]) / bound)))
        DFn = np.linalg.norm(ev["DF"][q].astype(np.float64), axis=0)
        assert abs(dist[q] - float(r[1])) <= xb[q] + float(DFn @ bound), (name, q, dist[q], float(r[1]))
    print("locate %-40s max iterations %d (reference %d), xi %.3f of the bound" % (name, iters.max(), ref_it.max(), worst))
    return rxi


def _round_trip_points(P, n, rng):
    xi = np.stack([rng.uniform(u[0], u[-1], n) for u in P.uks], axis=1)
    for q in range(0, n, 5):                                       # a fifth of them on faces
        k = rng.integers(P.d)
        xi[q, k] = P.uks[k][0] if rng.integers(2) else P.uks[k][-1]
    return xi


ROUND_TRIPS = {
    "quarter_annulus_4": (lambda: (2,) + R.annulus_patch(4), 200, {}, 5),
    "quarter_annulus_7": (lambda: (2,) + R.annulus_patch(7), 200, {}, 5),
    "quarter_annulus_7_one_seed": (lambda: (2,) + R.annulus_patch(7), 200, {"max_seeds": 1}, 8),
    "quarter_annulus_7_seven_seeds": (lambda: (2,) + R.annulus_patch(7), 200, {"max_seeds": 7}, 6),
    "rational_volume_p1": (lambda: (1,) + R.volume_patch(1, (2, 3, 2)), 200, {}, 5),
    "rational_volume_p2": (lambda: (2,) + R.volume_patch(2, (2, 3, 2)), 200, {}, 5),
    "rational_volume_p3": (lambda: (3,) + R.volume_patch(3, (2, 2, 2)), 200, {}, 5),
    "lifted_annulus": (lambda: (2,) + _lifted_annulus(4), 200, {}, 5),
    "2d_p5_generic": (lambda: (5,) + _graded((2, 2), 5, 11), 65, {}, 5),
    "1d_p3": (lambda: (3,) + _graded((5,), 3, 3), 65, {}, 5),
}


def _patch_case(make):
    p, uks, cp = make()
    return dict(p=p, uks=uks, cp=cp, P=S.Patch(uks, p, cp), c=S.constants(len(uks), p, len(cp) - 1))


@pytest.mark.parametrize("name", sorted(ROUND_TRIPS))
def test_locate_round_trips(T, name):
    make, n, kw, most = ROUND_TRIPS[name]
    c = _patch_case(make)
    P = c["P"]
    xi0 = _round_trip_points(P, n, np.random.default_rng(len(name)))
    x = P.eval(xi0)["x"].astype(np.float64)
    tol = 1e-13
    res = P.locate(x, tol=tol, max_iter=50, **kw)
    assert all(r[3] == 0 for r in res) and max(r[2] for r in res) <= most      # (the limits of the host test, per case)
    got = _locate(T, c, x, tol=tol, max_iter=50, **kw)
    assert np.all(got[3] == 0)
    rxi = _compare_with_reference(name, c, x, got, [r[:4] + (0.0,) + r[5:] for r in res], tol)
    # xi itself is recovered within that bound (x was rounded to double: once more the bound of x)
    ev = P.eval(xi0)
    xb = np.sqrt(np.sum((3 * c["c"]["x"] * EPS * ev["x_mag"].astype(np.float64)) ** 2, axis=1))
    rows = np.array([r[5] for r in res])
    assert np.all(np.abs(got[0] - xi0) <= rows * xb[:, None] + 2 * EPS * np.abs(xi0))
    assert np.all(got[1] <= xb)
    for k in range(P.d):
        assert np.all((got[0][:, k] >= P.uks[k][0]) & (got[0][:, k] <= P.uks[k][-1]))
    # followed by an evaluation: never NaN
    xe = _run(T, c, got[0], nF=1, u=False)[0]
    assert not np.isnan(xe).any()
    # a caller's guess: the same answers within the bound
    guess = xi0 + 0.02 * np.random.default_rng(1).standard_normal(xi0.shape) * np.array([u[-1] - u[0] for u in P.uks])
    res_g = P.locate(x, guess=guess, tol=tol, max_iter=50)
    got_g = _locate(T, c, x, guess=guess, tol=tol, max_iter=50)
    _compare_with_reference(name + " (guess)", c, x, got_g, [r[:4] + (0.0,) + r[5:] for r in res_g], tol)


@pytest.mark.parametrize("offset", [0.05, 0.2])
def test_locate_projects_points_off_the_surface(T, offset):
    c = _patch_case(lambda: (2,) + _lifted_annulus(4))
    P = c["P"]
    rng = np.random.default_rng(5)
    xi0 = rng.uniform(0.05, 0.95, (40, 2))
    out = P.eval(xi0)
    nrm = np.cross(out["DF"][:, :, 0], out["DF"][:, :, 1])
    nrm = nrm / np.sqrt(np.sum(nrm * nrm, axis=1))[:, None]
    x = (out["x"] + offset * nrm * np.where(np.arange(40) % 2, 1, -1)[:, None]).astype(np.float64)
    tol = 1e-12
    res = P.locate(x, tol=tol, max_iter=50)
    assert all(r[3] == 0 and r[4] <= 0.5 for r in res)
    got = _locate(T, c, x, tol=tol, max_iter=50)
    _compare_with_reference("lifted annulus, %.2f off" % offset, c, x, got, res, tol)
    assert np.max(np.abs(got[1] - offset)) <= 1e-10


def test_locate_points_outside_the_annulus(T):
    c = _patch_case(lambda: (2,) + R.annulus_patch(4))
    th = np.linspace(0.1, 1.4, 8)
    ring = np.stack([np.cos(th), np.sin(th)], axis=1)
    x = np.concatenate([0.6 * ring, 2.4 * ring, [[1.5 * np.cos(-0.2), 1.5 * np.sin(-0.2)], [1.5 * np.cos(1.8), 1.5 * np.sin(1.8)]]])
    tol = 1e-12
    res = c["P"].locate(x, tol=tol, max_iter=50)
    assert all(r[3] == 0 for r in res)
    got = _locate(T, c, x, tol=tol, max_iter=50)
    _compare_with_reference("outside the annulus", c, x, got, res, tol)
    assert np.all(got[0][:8, 0] == 0.0) and np.all(got[0][8:16, 0] == 1.0) and got[0][16, 1] == 0.0 and got[0][17, 1] == 1.0


def test_locate_statuses_and_counts(T):
    c = _patch_case(lambda: (2,) + R.annulus_patch(4))
    P = c["P"]
    rng = np.random.default_rng(9)
    xi0 = rng.uniform(0, 1, (65, 2))
    x = P.eval(xi0)["x"].astype(np.float64)
    # the iteration limit: status 1 after one step (the seed is not the answer), no fault
    xi, dist, iters, status = _locate(T, c, x, tol=1e-13, max_iter=1, max_seeds=1)
    assert np.all(status == 1) and np.all(iters == 1) and np.all(np.isfinite(xi)) and np.all(np.isfinite(dist))
    # a point that is not finite: status 2, xi and the distance NaN; its neighbours are untouched
    xb = x.copy()
    xb[7, 1], xb[30, 0] = np.nan, np.inf
    good = _locate(T, c, x, tol=1e-13)
    xi, dist, iters, status = _locate(T, c, xb, tol=1e-13)
    bad = np.zeros(65, dtype=bool)
    bad[[7, 30]] = True
    assert np.all(status[bad] == 2) and np.all(np.isnan(xi[bad])) and np.all(np.isnan(dist[bad])) and np.all(iters[bad] == 0)
    assert np.all(status[~bad] == 0) and _bits(xi[~bad], good[0][~bad]) and _bits(dist[~bad], good[1][~bad])
    assert np.all(_locate(T, c, x, guess=np.where(bad[:, None], np.nan, xi0), tol=1e-13)[3][bad] == 2)
    # two runs: the same bits
    again = _locate(T, c, x, tol=1e-13)
    assert _bits(again[0], good[0]) and _bits(again[1], good[1]) and np.array_equal(again[2], good[2])
    # 0, 1 and 65 points
    for n in (0, 1):
        xi_n, dist_n, it_n, st_n = _locate(T, c, x[:n], tol=1e-13)
        assert xi_n.shape == (n, 2) and _bits(xi_n, good[0][:n]) and np.array_equal(st_n, good[3][:n])
    # a collapsed edge (every node of xi_0 = 0 at the origin), hit exactly: DF^T DF is singular there
    uks = [np.linspace(0.0, 1.0, 3), np.linspace(0.0, 1.0, 3)]
    X = R.lagrange_nodes(uks, 2)
    cc = _patch_case(lambda: (2, uks, [X[0] * np.cos(X[1]), X[0] * np.sin(X[1]), np.ones_like(X[0])]))
    st = _locate(T, cc, np.zeros((1, 2)), guess=np.array([[0.0, 0.5]]))[3]
    assert st[0] == 3 and cc["P"].locate(np.zeros((1, 2)), guess=np.array([[0.0, 0.5]]))[0][3] == 3
    # refusals
    err = T.dev.TigarHipError
    dv = T.dev.DeviceVector
    for kw, what in (({"tol": 0.0}, "positive tolerance"), ({"max_iter": 101}, "iterations"), ({"max_iter": 0}, "iterations"),
                     ({"max_seeds": 0}, "at least one seed")):
        with pytest.raises(err, match=what):
            T.dev.point_locate(c["uks"], 2, _dcp(T, c), dv(data=_block(x)), **kw)


# ---- through the API ---------------------------------------------------------------------------------------------------------
def _annulus_spline(T, nel, clamp=True, nfields=1, rtol=1e-12):
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(nel)
    gen = T.t.EqualOrderSpline(nfields, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf))
    if clamp:
        for f in range(nfields):
            sp0 = gen.getScalarSpline(f)
            for direction in (0, 1):
                for side in (0, 1):
                    gen.addZeroDofs(f, sp0.getSideDofs(direction, side))
    spline = T.t.ExtractedSpline(gen, 4)
    solver = T.t.PETScKrylovSolver("cg", "jacobi")
    solver.parameters["relative_tolerance"] = rtol
    spline.setSolverOptions(linearSolver=solver)
    return gen, spline, kv, Pf


@pytest.fixture(scope="module")
def poisson(T):
    """the rational Poisson problem on the quarter annulus (nel = 8) solved on the device, and the host flow of the same
    discrete problem (tests/rational_reference.py: same quadrature, direct solve)"""
    import scipy.sparse.linalg as spl
    import rational_reference as RR
    nel, rtol = 8, 1e-12
    gen, spline, kv, Pf = _annulus_spline(T, nel, True, rtol=rtol)
    u = T.t.Function(spline.V)
    spline.solveLinearVariationalProblem(
        T.F.Equation(T.F.LaplaceForm(geometry=gen, rational=True), T.F.QuadratureLoadForm(R.annulus_rhs, gen, rational=True)), u)
    hl2, hh10, Kf, Mf, bf = RR.solve_annulus_poisson(nel, matrices=True)
    Mc = O.generate_M_tensor(O.BSpline([2, 2], [kv, kv]))
    ncp = Mc.shape[1]
    n1 = int(round(np.sqrt(ncp)))
    idx = np.arange(ncp).reshape(n1, n1, order="F")
    free = np.setdiff1d(np.arange(ncp), np.unique(np.concatenate([idx[0], idx[-1], idx[:, 0], idx[:, -1]])))
    U = np.zeros(ncp)
    U[free] = spl.spsolve(Kf.tocsc(), bf)
    lmin = float(np.linalg.eigvalsh(Kf.toarray()).min())
    # CG stops at |r| <= rtol |b| (times 10 for the preconditioned norm): the dofs differ by at most |K^-1 r|_2, and so does
    # the function at any point -- the rational basis is a partition of unity
    solver_gap = 10.0 * rtol * float(np.linalg.norm(bf)) / lmin
    uks, cp = R.annulus_patch(nel)
    return dict(spline=spline, gen=gen, u=u, host_nodal=Mc @ U, solver_gap=solver_gap, P=S.Patch(uks, 2, cp), hl2=hl2)


def test_evaluate_at_physical_points_of_the_poisson_solution(T, poisson):
    spline, u, P = poisson["spline"], poisson["u"], poisson["P"]
    rng = np.random.default_rng(4)
    r, th = rng.uniform(1.0, 2.0, 50), rng.uniform(0.0, np.pi / 2, 50)
    x = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    val, located = spline.evaluateAtPhysicalPoints(u, x, rational=True, tol=1e-13)
    assert located.converged and located.npts == 50 and located.xi.shape == (50, 2) and np.max(located.distance) <= 1e-14
    assert np.max(np.abs(located.xi[:, 0] - (r - 1.0))) <= 1e-14
    host = P.eval(located.xi, [poisson["host_nodal"]], rational=True)["val"][:, 0].astype(np.float64)
    got = val.get_local()
    gap = poisson["solver_gap"] + 1e-13
    e_host = np.abs(host - R.annulus_exact(x))
    print("poisson at 50 points: device - host %.2e (solver gap %.2e), host - exact %.2e, host L2 error %.2e"
          % (np.max(np.abs(got - host)), gap, e_host.max(), poisson["hl2"]))
    assert np.max(np.abs(got - host)) <= gap
    assert np.max(np.abs(got - R.annulus_exact(x))) <= e_host.max() + gap        # the discretisation error of the host flow
    assert e_host.max() <= 10.0 * poisson["hl2"]                                 # ... which is of the size of its error norm
    # with the gradient; evaluateAtPoints at the same xi gives the same bits; physicalPoints returns x
    v2, comps, loc2 = spline.evaluateAtPhysicalPoints(u, x, grad=True, rational=True, tol=1e-13)
    assert _bits(v2.get_local(), got) and len(comps) == 2 and comps[0].size() == 50
    assert _bits(spline.evaluateAtPoints(u, located.xi, rational=True).get_local(), got)
    assert _bits(spline.evaluateAtPoints(u, located.xi_device, rational=True).get_local(), got)
    assert np.max(np.abs(spline.physicalPoints(located.xi) - x)) <= 1e-14
    g = np.stack([cc.get_local() for cc in comps], axis=1)
    ghost = P.eval(located.xi, [poisson["host_nodal"]], rational=True)["grad"][:, 0].astype(np.float64)
    # the gradient of the difference of the two discrete solutions: |dU|_max sum_i |grad N_i| with sum_i |d N_i / d xi_k| <=
    # 2 p nel = 32 per direction and |d xi / d x| <= 1 on this annulus (radial scale 1, arc length >= pi / 2 per unit of xi_1)
    print("gradient: device - host %.2e, host - exact %.2e" % (np.max(np.abs(g - ghost)), np.max(np.abs(ghost - R.annulus_exact_grad(x)))))
    assert np.max(np.abs(g - ghost)) <= 64.0 * gap + 1e-11


def test_write_vtk_of_the_poisson_solution(T, poisson, tmp_path):
    spline, u = poisson["spline"], poisson["u"]
    u.rename("u", "solution")
    for m, enc in ((None, "raw"), (4, "ascii"), ([0.0, 0.25, 1.0], "raw")):
        pts = spline.latticePoints(m)
        assert pts is spline.latticePoints(m if m is not None else 3) and pts.npts == 64 * pts.m ** 2
        path = str(tmp_path / ("u_%s_%d.vtu" % (enc, pts.m)))
        assert spline.writeVTK(path, {"u": u, "F2": spline.cpFuncs[2]}, m=m, rational=False, encoding=enc) == path
        got = V.read_vtu(path)
        assert _bits(got["points"][:, :2], pts.x) and np.all(got["points"][:, 2] == 0.0)
        assert _bits(got["point_data"]["u"], spline.evaluateAtLattice(u, m).get_local())
        assert _bits(got["point_data"]["F2"], spline.evaluateAtLattice(spline.cpFuncs[2], m).get_local())
        assert got["ncells"] == (pts.m - 1) ** 2 * 64 and np.all(got["types"] == 9)
        assert got["cells"].min() >= 0 and got["cells"].max() < pts.npts
        assert np.all(V.cell_measures(got["points"], got["cells"], got["offsets"], got["types"]) > 0.0)
    # the lattice values are those of the points: values() of a function, of a callable
    pts = spline.latticePoints(3)
    assert _bits(pts.values(u).get_local(), spline.evaluateAtLattice(u, 3).get_local())
    assert _bits(pts.values(lambda x: x[:, 0]).get_local(), pts.x[:, 0])
    cells, ctype = pts.cells()
    assert ctype == 9 and cells.shape == (4 * 64, 4)
    val, comps = spline.evaluateAtLattice(u, 3, grad=True, rational=True)
    assert _bits(val.get_local(), spline.evaluateAtLattice(u, 3, rational=True).get_local()) and len(comps) == 2
    # two steps into one collection
    pvd = str(tmp_path / "series" / "u.pvd")
    f0 = spline.writeVTK(pvd, {"u": u}, time=0.0)
    f1 = spline.writeVTK(pvd, {"u": u}, time=0.5)
    assert (os.path.basename(f0), os.path.basename(f1)) == ("u000000.vtu", "u000001.vtu")
    assert V.read_pvd(pvd) == [(0.0, "u000000.vtu"), (0.5, "u000001.vtu")]
    assert _bits(V.read_vtu(f1)["point_data"]["u"], spline.evaluateAtLattice(u).get_local())


def test_three_fields_are_written_as_a_vector_and_displace_the_points(T, tmp_path):
    gen, spline, kv, Pf = _annulus_spline(T, 3, clamp=False, nfields=3)
    n = spline.V.grids[0].num_nodes()
    rng = np.random.default_rng(2)
    w = T.t.Function(spline.V)
    w.vector().set_local(0.01 * rng.standard_normal(3 * n))
    w.rename("w", "w")
    vals = spline.evaluateAtLattice(w, 3)
    assert isinstance(vals, list) and len(vals) == 3
    uks, cp = R.annulus_patch(3)
    ref = S.lattice_reference(uks, 2, cp, np.linspace(0, 1, 3))
    for i in range(3):
        v, _, vm, _ = ref.eval(w.vector().get_local()[i * n:(i + 1) * n])
        assert np.all(np.abs(vals[i].get_local() - v) <= (R.constants(2, 2, 3, 2)["val"] * EPS * vm).astype(np.float64))
    # nF = 3 != nsd = 2: one array per field; the points of a points-at evaluation, field by field
    path = str(tmp_path / "w.vtu")
    spline.writeVTK(path, {"w": w}, m=3)
    got = V.read_vtu(path)
    assert got["order"] == ["w_0", "w_1", "w_2"] and all(_bits(got["point_data"]["w_%d" % i], vals[i].get_local()) for i in range(3))
    res = spline.evaluateAtPoints(w, np.array([[0.5, 0.5], [0.0, 1.0]]), grad=True)
    assert len(res) == 3 and all(len(r) == 2 and r[0].size() == 2 and len(r[1]) == 2 for r in res)
    # a surface: nsd = 3 fields are one vector array, and ``displacement`` shifts the points by the interpolated field
    from geom_util import quarter_annulus
    kv, Pf2 = quarter_annulus(3)
    Pf3 = np.concatenate([Pf2[:, :, :2], 0.3 * Pf2[:, :, :1] * Pf2[:, :, 1:2] / Pf2[:, :, 2:], Pf2[:, :, 2:]], axis=2)
    gen3 = T.t.EqualOrderSpline(3, T.N.NURBSControlMesh([2, 2], [kv, kv], Pf3))
    shell = T.t.ExtractedSpline(gen3, 4)
    disp = T.t.Function(shell.V)
    disp.vector().set_local(0.01 * rng.standard_normal(3 * n))
    path = str(tmp_path / "shell.vtu")
    shell.writeVTK(path, {"disp": disp}, m=3, displacement=disp)
    got = V.read_vtu(path)
    D = np.stack([v.get_local() for v in shell.evaluateAtLattice(disp, 3)], axis=1)
    assert got["point_data"]["disp"].shape == (shell.latticePoints(3).npts, 3) and _bits(got["point_data"]["disp"], D)
    assert _bits(got["points"], shell.latticePoints(3).x + D)
    loc = shell.locatePoints(shell.latticePoints(3).x[:20] + np.array([0.0, 0.0, 0.01]))
    assert loc.converged and np.all(loc.distance > 0.0) and np.all(loc.distance <= 0.01 + 1e-12)
    assert not np.isnan(shell.evaluateAtPoints(disp, loc.xi_device)[0].get_local()).any()


def test_file_writes_the_node_grid_and_function_names(T, tmp_path):
    """the closing lines of demos/poisson/poisson-nurbs.py, run as written"""
    gen, spline, kv, Pf = _annulus_spline(T, 3, clamp=False)
    File = T.t.File
    u = T.t.Function(spline.V)
    assert u.name() == "f"
    g = spline.V.grids[0]
    u.vector().set_local(np.arange(g.num_nodes(), dtype=np.float64))
    u.rename("u", "u")
    assert u.name() == "u"
    path = str(tmp_path / "results" / "u.pvd")
    f = File(path)
    f << u
    f << (u, 0.25)
    assert V.read_pvd(path) == [(0.0, "u000000.vtu"), (0.25, "u000001.vtu")]
    got = V.read_vtu(str(tmp_path / "results" / "u000001.vtu"))
    assert _bits(got["points"][:, :2], g.coordinates()) and _bits(got["point_data"]["u"], u.vector().get_local())
    assert got["ncells"] == (g.shape()[0] - 1) * (g.shape()[1] - 1) == 2 ** 2 * 9        # p^d linear cells per element
    assert np.all(V.cell_measures(got["points"], got["cells"], got["offsets"], got["types"]) > 0.0)
    nsd = spline.nsd
    for i in range(nsd + 1):
        name = "F" + str(i)
        spline.cpFuncs[i].rename(name, name)
        File(str(tmp_path / "results" / (name + "-file.pvd"))) << spline.cpFuncs[i]
        got = V.read_vtu(str(tmp_path / "results" / (name + "-file000000.vtu")))
        assert got["order"] == [name] and _bits(got["point_data"][name], spline.cpFuncs[i].vector().get_local())
    # several fields: split gives copies on the scalar space; two or three fields are one vector array
    gen2, spline2, _, _ = _annulus_spline(T, 3, clamp=False, nfields=2)
    w = T.t.Function(spline2.V)
    w.vector().set_local(np.arange(2 * g.num_nodes(), dtype=np.float64))
    w.rename("w", "w")
    parts = w.split()
    assert [q.name() for q in parts] == ["w_0", "w_1"] and all(q.function_space().dim() == g.num_nodes() for q in parts)
    assert _bits(parts[1].vector().get_local(), np.arange(g.num_nodes(), 2 * g.num_nodes()))
    parts[0].vector().set_local(np.zeros(g.num_nodes()))
    assert w.vector().get_local()[1] == 1.0                                              # copies
    assert [q.name() for q in u.split()] == ["u"]
    File(str(tmp_path / "w.vtu")) << w
    got = V.read_vtu(str(tmp_path / "w.vtu"))
    assert got["point_data"]["w"].shape == (g.num_nodes(), 3) and _bits(got["point_data"]["w"][:, 1], parts[1].vector().get_local())
    with pytest.raises(ValueError, match="vtu"):
        File(str(tmp_path / "w.xdmf")) << w
    # a second File object on the same collection appends to what is on disk
    File(path) << (u, 0.5)
    assert V.read_pvd(path) == [(0.0, "u000000.vtu"), (0.25, "u000001.vtu"), (0.5, "u000002.vtu")]
    # a grid that is not a continuous tensor node grid is refused
    class _Other(object):
        def function_space(self):
            return type("V", (), {"grids": [object()]})()
    with pytest.raises(NotImplementedError, match="tensor node grids"):
        File(str(tmp_path / "other.vtu")) << _Other()


def test_api_refusals(T, poisson):
    spline, u = poisson["spline"], poisson["u"]
    n = spline.V.dim()
    with pytest.raises(ValueError, match="xi of shape"):
        spline.evaluateAtPoints(u, np.zeros((4, 3)))
    with pytest.raises(ValueError, match="nodal values given"):
        spline.evaluateAtPoints(np.zeros(n + 1), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="not a multiple"):
        spline.evaluateAtPoints(u, T.dev.DeviceVector(data=np.zeros(5)))
    with pytest.raises(ValueError, match="x of shape"):
        spline.locatePoints(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="starting values"):
        spline.locatePoints(np.zeros((4, 2)), guess=np.zeros((3, 2)))
    for kw in ({"tol": 0.0}, {"tol": -1.0}, {"maximum_iterations": 0}, {"maximum_iterations": 101}, {"max_seeds": 0}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            spline.locatePoints(np.ones((2, 2)), **kw)
    for m in (0, 11, 2.5, [0.5, 0.25], [-0.5, 0.5], [0.0, 1.5], np.linspace(0, 1, 11)):
        with pytest.raises(ValueError, match="lattice"):
            spline.latticePoints(m)
    with pytest.raises(ValueError, match="no cells"):
        spline.writeVTK("unused.vtu", {"u": u}, m=1)
    with pytest.raises(ValueError, match="displacement has 1 fields"):
        spline.writeVTK("unused.vtu", {"u": u}, displacement=u)
    with pytest.raises(ValueError, match="vtu"):
        spline.writeVTK("unused.xdmf", {"u": u})
    assert not os.path.exists("unused.vtu") and not os.path.exists("unused.xdmf")
    # the scope of the point operands: a spline with the caller's FE dof order
    caller = spline.__class__.__dict__["_caller_ordered"]
    try:
        spline.__class__._caller_ordered = lambda self: True
        with pytest.raises(NotImplementedError, match="feOrder"):
            spline.evaluateAtPoints(u, np.zeros((1, 2)))
        with pytest.raises(NotImplementedError, match="feOrder"):
            spline.latticePoints()
    finally:
        spline.__class__._caller_ordered = caller


def test_largest_ratios_to_the_bounds():
    """(reported, not a check of its own: the largest measured ratio of every output of test_point_eval to its bound)"""
    for what in sorted(_WORST):
        print("largest ratio to the bound, %-14s %.3f" % (what, _WORST[what]))
    assert all(v <= 1.0 for v in _WORST.values())
