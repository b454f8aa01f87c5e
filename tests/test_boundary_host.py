"""CPU: the longdouble reference of the boundary kernels (tests/boundary_reference.py) against closed forms, its host flows,
and the argument checking of the boundary forms that needs no device."""
import numpy as np
import pytest

import postproc_reference as R
import boundary_reference as BR

EPS = BR.EPS


def test_annulus_arcs_normals_and_thickness():
    """quarter annulus 1 <= r <= 2: arc lengths pi/2 and pi (a 3-point Gauss rule on 5 elements of the rational arc: 1e-8),
    straight edges of length 1, normals -+ x / |x| on the arcs and -e_y, -e_x on the edges theta = 0, pi/2, radial
    thickness 1 / 5 of the boundary element on the arcs"""
    uks, cp = R.annulus_patch(5)
    length = {(0, 0): np.pi / 2, (0, 1): np.pi, (1, 0): 1.0, (1, 1): 1.0}
    for (k, s), L in length.items():
        ref = BR.FaceReference(uks, 2, cp, k, s)
        assert ref.npts == 15 and ref.x.shape == (15, 2)
        assert abs(float(ref.wsurf.sum()) - L) <= (1e-8 if k == 0 else 64 * EPS) * L
        x = np.asarray(ref.x, dtype=np.float64)
        if k == 0:
            exact = (2 * s - 1) * x / np.hypot(x[:, 0], x[:, 1])[:, None]
            assert np.max(np.abs(np.hypot(x[:, 0], x[:, 1]) - (1.0 + s))) <= 16 * EPS
            assert np.max(np.abs(np.asarray(ref.hn, dtype=np.float64) - 0.2)) <= 64 * EPS
        else:
            exact = np.tile([0.0, -1.0] if s == 0 else [-1.0, 0.0], (ref.npts, 1))
        assert np.max(np.abs(np.asarray(ref.normal, dtype=np.float64) - exact)) <= 64 * EPS


def test_box_faces():
    """the box [0, 1] x [0, 1.5] x [0, 2] on 2 x 3 x 2 elements: n = +- e_k, the face areas, h_n the element size"""
    uks = [np.linspace(0.0, 1.0 + 0.5 * k, n + 1) for k, n in enumerate((2, 3, 2))]
    X = R.lagrange_nodes(uks, 2)
    cp = X + [np.ones_like(X[0])]
    size = [1.0, 1.5, 2.0]
    for k, s in BR.all_faces(3):
        ref = BR.FaceReference(uks, 2, cp, k, s, nq=2)
        area = np.prod([size[j] for j in range(3) if j != k])
        assert abs(float(ref.wsurf.sum()) - area) <= 16 * EPS * area
        e = np.zeros(3)
        e[k] = 2 * s - 1
        assert np.max(np.abs(np.asarray(ref.normal, dtype=np.float64) - e)) <= 16 * EPS
        assert np.max(np.abs(np.asarray(ref.hn, dtype=np.float64) - size[k] / (2, 3, 2)[k])) <= 16 * EPS
        x = np.asarray(ref.x, dtype=np.float64)
        assert np.max(np.abs(x[:, k] - s * size[k])) <= 16 * EPS


def test_normal_derivative_and_matrix_of_the_reference():
    """d_n of a linear function is grad l . n, also in the rational space (nodal values w l); the matrix applied to nodal
    vectors is the bilinear form of the point values"""
    uks, cp = R.volume_patch(2, (2, 1, 2))
    w = np.asarray(cp[-1])
    xn = np.stack([np.asarray(cp[i]) / w for i in range(3)], axis=1)
    l, gl = BR.LIN_3D
    rng = np.random.default_rng(3)
    for k, s in BR.all_faces(3):
        ref = BR.FaceReference(uks, 2, cp, k, s)
        val, grad, dn = ref.eval(w * l(xn), rational=True)
        x = np.asarray(ref.x, dtype=np.float64)
        assert np.max(np.abs(np.asarray(val, dtype=np.float64) - l(x))) <= 256 * EPS * np.max(np.abs(l(x)))
        assert np.max(np.abs(np.asarray(grad, dtype=np.float64) - gl)) <= 1024 * EPS * np.max(np.abs(gl))
        assert np.max(np.abs(np.asarray(dn - ref.normal @ gl.astype(BR.LD), dtype=np.float64))) <= 1024 * EPS * np.max(np.abs(gl))
        u, v = rng.standard_normal(ref.nnodes), rng.standard_normal(ref.nnodes)
        a, b, c = (rng.standard_normal(ref.npts) for _ in range(3))
        uq, _, dnu = ref.eval(u)
        vq, _, dnv = ref.eval(v)
        form = np.sum(ref.wsurf * (a * vq * uq + b * vq * dnu + c * dnv * uq))
        got = v.astype(BR.LD) @ ref.matrix(a, b, c) @ u.astype(BR.LD)
        assert abs(float(got - form)) <= 1e-15 * float(np.sum(ref.wsurf * (abs(vq * uq) + abs(vq * dnu) + abs(dnv * uq))) * 3)
        assert np.max(np.abs(np.asarray(ref.load(a, b) - (ref.matrix(a, None, b) @ np.ones(ref.nnodes, dtype=BR.LD)),
                                        dtype=np.float64))) <= 1e-15 * 10


def test_closed_surface_of_the_polynomial_maps():
    """sum_faces sum_q wsurf n = 0 and sum_faces sum_q wsurf x . n = d |Omega| on the polynomial maps with nq = 3: n wsurf
    has degree <= 1 (2-D, p = 2) / (1, 1) (3-D, trilinear) per face element and x . n wsurf degree <= 3 / (2, 2); the
    volume weight has degree <= (3, 3) / (2, 2, 2): all within the 5 a 3-point rule integrates exactly"""
    for kvs, C in (BR.poly_patch_2d((3, 2)), BR.poly_patch_3d((2, 1, 3))):
        d = len(kvs)
        uks, Mc, cp = BR.patch_from_net(2, kvs, C)
        closed, moment, area = np.zeros(d, dtype=BR.LD), BR.LD(0), BR.LD(0)
        for k, s in BR.all_faces(d):
            ref = BR.FaceReference(uks, 2, cp, k, s)
            closed += ref.wsurf @ ref.normal
            moment += np.sum(ref.wsurf * np.sum(ref.x * ref.normal, axis=1))
            area += ref.wsurf.sum()
        vol = R.Reference(uks, 2, cp).wdet.sum()
        assert np.max(np.abs(closed)) <= 16 * EPS * area
        assert abs(moment - d * vol) <= 16 * EPS * area


def test_host_flows():
    """the patch test reproduces the linear function; the annulus errors fall like 2^(p+1) and 2^p"""
    k2, C2 = BR.poly_patch_2d((3, 2))
    assert BR.patch_test_host(k2, C2, BR.LIN_2D) <= 1e-13
    assert BR.patch_test_host(k2, C2, BR.LIN_2D, nitsche_faces=[(0, 0), (1, 1)]) <= 1e-13
    r4, r8 = BR.solve_annulus_boundary(4), BR.solve_annulus_boundary(8)
    assert 7.0 <= r4["l2"] / r8["l2"] <= 11.0 and 3.5 <= r4["h10"] / r8["h10"] <= 5.0
    assert abs(r8["flux"] + r8["intf"]) < abs(r4["flux"] + r4["intf"]) < 0.3


class _Geometry(object):
    """stands in for a generator where only the arguments are looked at"""


def test_faces_argument():
    from tigar_amd import forms as F
    assert F.check_faces(None, 2, "t") == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert F.check_faces(None, 3, "t", periodic={1}) == [(0, 0), (0, 1), (2, 0), (2, 1)]
    assert F.check_faces((1, 0), 2, "t") == [(1, 0)]
    assert F.check_faces([(1, 0), (0, 1)], 2, "t") == [(1, 0), (0, 1)]
    for bad in ((2, 0), (0, 2), (-1, 0), [(0, 0), (0, 0)], [], [(0, 0, 1)], 3, (0.5, 1), [(0, True)]):
        with pytest.raises(ValueError):
            F.check_faces(bad, 2, "t")
    with pytest.raises(ValueError, match="periodic"):
        F.check_faces((1, 0), 2, "t", periodic={1})
    with pytest.raises(ValueError, match="periodic"):
        F.check_faces(None, 1, "t", periodic={0})


def test_forms_need_a_geometry_and_sum_checks_its_terms():
    from tigar_amd import forms as F
    g = _Geometry()
    for make in (lambda: F.BoundaryLoadForm(1.0, None), lambda: F.BoundaryMassForm(1.0, None),
                 lambda: F.NitscheForm(None, None, 10.0), lambda: F.BoundaryLoadForm.pressure(1.0, None)):
        with pytest.raises(ValueError, match="geometry"):
            make()
    lap, mass = F.LaplaceForm(geometry=g), F.BoundaryMassForm(2.0, g)
    nit, skew = F.NitscheForm(g, [(0, 0)], 10.0), F.NitscheForm(g, [(0, 0)], 10.0, symmetric=False)
    assert mass.symmetric and nit.symmetric and not skew.symmetric
    assert F.Sum(lap, (2.0, mass), nit).symmetric and not F.Sum(lap, skew).symmetric
    assert F.Sum(lap, (2.0, mass)).terms[1][0] == 2.0
    rhs = F.Sum(F.BoundaryLoadForm(1.0, g), (0.5, nit.load(1.0)))
    assert not rhs.symmetric
    with pytest.raises(ValueError):
        F.Sum()
    with pytest.raises(ValueError):
        F.Sum(lap, F.BoundaryLoadForm(1.0, g))          # a matrix form and a vector form
    with pytest.raises(ValueError):
        F.Sum((1.0, lap, mass))
    with pytest.raises(ValueError):
        F.Sum(3.0)
    with pytest.raises(TypeError):
        rhs.assemble_matrix(None)
    with pytest.raises(TypeError):
        F.Sum(lap).assemble_vector(None)


def test_fields_on_bases_of_their_own_are_refused():
    """a compatible space may put its fields on one node grid like the space of ElasticityForm; the generator is asked"""
    import tigar_amd as t
    from tigar_amd import forms as F
    from tigar_amd.compatibleSplines import BSplineCompat
    for cls in (t.FieldListSpline, BSplineCompat):
        gen = object.__new__(cls)
        extracted = _Geometry()
        extracted._generator = gen
        for geometry in (gen, extracted):
            with pytest.raises(NotImplementedError, match=cls.__name__):
                F._fields_of_the_patch(geometry, "t")
    F._fields_of_the_patch(object.__new__(t.EqualOrderSpline), "t")
    F._fields_of_the_patch(_Geometry(), "t")                  # (nothing known about it: the node grid decides)
