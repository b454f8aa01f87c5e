"""CPU: the longdouble reference of the quadrature-point kernels (tests/postproc_reference.py) against facts that do not
depend on it -- the area of the quarter annulus, the oracle's load vector, gradients of fields linear in x -- and the C ABI
of the feature."""
import os
import re

import numpy as np
import pytest

from oracle import tigar_oracle as O
from geom_util import quarter_annulus
import postproc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


lagrange_nodes, annulus_patch = R.lagrange_nodes, R.annulus_patch


def test_weights_sum_to_the_area_of_the_quarter_annulus():
    uks, cp = annulus_patch(5)
    ref = R.Reference(uks, 2, cp, nq=3)
    assert abs(float(np.sum(ref.wdet)) - 0.75 * np.pi) < 1e-6
    r = np.hypot(ref.x[:, 0], ref.x[:, 1]).astype(np.float64)
    assert r.min() > 1.0 and r.max() < 2.0 and ref.x.min() > 0.0


@pytest.mark.parametrize("d,p,nq", [(1, 3, None), (2, 2, None), (2, 2, 4), (3, 2, None)])
def test_load_from_point_values_equals_the_oracles_nodal_load(d, p, nq):
    rng = np.random.default_rng(d * 10 + p)
    nels = [(5,), (5, 4), (3, 2, 4)][d - 1]
    uks = [np.sort(np.concatenate([[0.0, 1.0 + 0.5 * k], rng.uniform(0.1, 0.9, nels[k] - 1)])) for k in range(d)]
    X = lagrange_nodes(uks, p)
    wgt = 1.0 + 0.2 * X[0] * X[-1]
    cp = [(X[i] + 0.1 * X[(i + 1) % d] ** 2) * wgt for i in range(d)] + [wgt]
    fn = np.sin(3.0 * X[0]) + X[-1]
    ref = R.Reference(uks, p, cp, nq)
    fq = ref.eval(fn)[0]
    b = ref.load(fq)[0].astype(np.float64)
    bo = R.oracle_load(uks, p, cp, fn, nq)
    assert np.max(np.abs(b - bo)) <= 1e-13 * np.max(np.abs(bo))


def test_gradient_of_a_field_linear_in_x_is_constant():
    rng = np.random.default_rng(3)
    # affine map x = A xi + b of a stretched 2-D grid, field u = c . x + c0
    uks = [np.array([0.0, 0.3, 0.55, 1.0]), np.array([0.0, 0.5, 1.25])]
    X = lagrange_nodes(uks, 2)
    A, c = np.array([[1.2, 0.4], [-0.3, 0.9]]), np.array([0.7, -1.3])
    phys = [A[i, 0] * X[0] + A[i, 1] * X[1] + 0.1 * i for i in range(2)]
    ref = R.Reference(uks, 2, phys + [np.ones_like(X[0])])
    v, g, _, _ = ref.eval(c[0] * phys[0] + c[1] * phys[1] + 0.25)
    assert np.max(np.abs(g.astype(np.float64) - c[None, :])) < 1e-14
    assert np.max(np.abs((v - (ref.x @ c.astype(R.LD) + 0.25)).astype(np.float64))) < 1e-15
    # the surface z = x^2 + y with a field linear in the parameters, u = a x + b y: the tangential (pinv) gradient is
    # (a, b, 0) - ((a, b, 0) . n) n with n the unit normal (-2x, -1, 1) / sqrt(4 x^2 + 2)
    cp = [X[0], X[1], X[0] ** 2 + X[1], np.ones_like(X[0])]
    ref = R.Reference(uks, 2, cp)
    a, b = 0.6, -0.8
    g = ref.eval(a * X[0] + b * X[1])[1]
    xq = ref.x[:, 0]
    n = np.stack([-2 * xq, -np.ones_like(xq), np.ones_like(xq)], axis=1) / np.sqrt(4 * xq * xq + 2)[:, None]
    e = np.array([a, b, 0.0], dtype=R.LD)
    expect = e[None, :] - (n @ e)[:, None] * n
    assert np.max(np.abs((g - expect).astype(np.float64))) < 1e-14
    del rng


def test_magnitudes_dominate_the_values():
    uks, cp = annulus_patch(3)
    ref = R.Reference(uks, 2, cp)
    u = np.random.default_rng(0).standard_normal(ref.nnodes)
    v, g, vm, gm = ref.eval(u)
    assert np.all(vm >= abs(v)) and np.all(gm >= abs(g)) and np.all(ref.wdet_mag >= ref.wdet)
    assert np.all(ref.x_mag >= abs(ref.x)) and ref.kappa >= 1.0


def test_header_declares_and_library_exports_the_quadrature_entries():
    names = ["tg_quad_points", "tg_quad_eval", "tg_quad_load", "tg_quad_error", "tg_vec_pointwise_divide"]
    src = open(os.path.join(ROOT, "include", "tigar_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in names:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), "%s is not declared in include/tigar_hip.h" % n
    from tigar_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load(require_device=False)
    for n in names:
        assert hasattr(lib, n), "library does not export %s" % n
        assert n in _lib.PROTOTYPES


def test_reference_flow_converges_with_the_margins_the_gpu_test_asserts():
    """the annulus Poisson problem of test_poisson_on_nurbs_annulus_converges through the oracle's matrices and a direct
    solve, errors by the reference: L2 drops per halving by at least 2^p, H10 by at least 2^(p-1) (measured: L2 ratios
    10.08 and 8.55, H10 ratios 4.46 and 4.11)"""
    errs = []
    for nel in (4, 8, 16):
        kv, _ = quarter_annulus(nel)
        s = O.BSpline([2, 2], [kv, kv])
        uks, cp = annulus_patch(nel)
        M = O.generate_M_tensor(s)
        X = np.stack([cp[0] / cp[2], cp[1] / cp[2]], axis=1)
        _, K, b = O.mapped_fe_system(uks, 2, cp, fnodal=R.annulus_rhs(X))
        zd = [i for direction in (0, 1) for side in (0, 1) for i in s.getSideDofs(direction, side)]
        _, u = O.solve_linear_system(M, O.extract_matrix(M, K, zd), O.extract_vector(M, b, zd), "direct")
        ref = R.Reference(uks, 2, cp)
        xq = ref.x.astype(np.float64)
        (s0, s1, _), _ = ref.sums(u, R.annulus_exact(xq), R.annulus_exact_grad(xq))
        errs.append((float(np.sqrt(s0)), float(np.sqrt(s1))))
    for a, b in zip(errs[:-1], errs[1:]):
        assert a[0] / b[0] >= 4.0 and a[1] / b[1] >= 2.0
