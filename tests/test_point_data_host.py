"""CPU: the host half of the point-data reader (forms.point_array / point_block / point_unblock) against plain nested loops,
in every layout the point forms use."""
import itertools

import numpy as np
import pytest

from tigar_amd import forms as F

NPTS = 5
BLOCK_ORDER, MAJOR_SWAP = (0, 2, 1, 3), (2, 3, 0, 1)


def _layouts():
    """(component shape, permutation of the component axes for the device) of every layout in use"""
    out = []
    for nF, nsd in itertools.product((2, 3), (2, 3)):
        out += [((nsd,), None), ((nsd, nsd), None), ((nF, nsd), None), ((nF, nF), None), ((nF, nsd, nF, nsd), BLOCK_ORDER)]
    for nF, nJ in itertools.product((2, 3), (3, 6)):
        out += [((nJ,), None), ((nJ, nJ), None), ((nF, nJ), None), ((nF, nJ, nF, nJ), BLOCK_ORDER)]
    return sorted(set(out), key=str)


def _by_loops(v, shape, perm):
    """the device layout written out: the component axes in the order ``perm``, the point index fastest"""
    order = list(range(len(shape))) if perm is None else list(perm)
    dims = [shape[a] for a in order]
    out = np.empty(int(np.prod(dims)) * NPTS)
    for comp in itertools.product(*[range(n) for n in dims]):
        at = 0
        for c, n in zip(comp, dims):
            at = at * n + c
        host = [None] * len(shape)
        for c, a in zip(comp, order):
            host[a] = c
        for q in range(NPTS):
            out[at * NPTS + q] = v[(q,) + tuple(host)]
    return out


@pytest.mark.parametrize("shape,perm", _layouts(), ids=str)
def test_layout_against_nested_loops(shape, perm):
    rng = np.random.default_rng(len(shape) + sum(shape))
    v = rng.standard_normal((NPTS,) + shape)
    flat = F.point_block(v, NPTS, shape, perm)
    assert flat.ndim == 1 and flat.flags["C_CONTIGUOUS"] and flat.dtype == np.float64
    assert np.array_equal(flat, _by_loops(v, shape, perm))
    if perm is None:
        assert np.array_equal(F.point_unblock(flat, NPTS, shape), v)
    # one block serves every point
    block = rng.standard_normal(shape)
    assert np.array_equal(F.point_block(block, NPTS, shape, perm), _by_loops(np.tile(block, (NPTS,) + (1,) * len(shape)), shape, perm))
    assert F.point_array(block, NPTS, shape).shape == (NPTS,) + shape


def test_block_order_is_i_j_K_L_q():
    """the tangent layouts: A[q, i, K, j, L] at (((i nF + j) nK + K) nK + L) npts + q"""
    for nF, nK in ((2, 2), (3, 3), (2, 3), (3, 6), (2, 6)):
        v = np.random.default_rng(nF * nK).standard_normal((NPTS, nF, nK, nF, nK))
        flat = F.point_block(v, NPTS, (nF, nK, nF, nK), BLOCK_ORDER)
        for i, j, K, L, q in itertools.product(range(nF), range(nF), range(nK), range(nK), range(NPTS)):
            assert flat[(((i * nF + j) * nK + K) * nK + L) * NPTS + q] == v[q, i, K, j, L]


@pytest.mark.parametrize("shape,perm", _layouts(), ids=str)
def test_wrong_shapes_are_refused(shape, perm):
    good = (NPTS,) + shape
    bad = [good + (1,), good[:-1], (NPTS + 1,) + shape, shape[:-1] + (shape[-1] + 1,), ()]
    bad += [good[:k] + (good[k] + 1,) + good[k + 1:] for k in range(len(good))]
    bad += [shape + (NPTS,)] if shape + (NPTS,) != good else []
    for b in bad:
        if b in (good, shape):
            continue
        with pytest.raises(ValueError, match="shape"):
            F.point_block(np.zeros(b), NPTS, shape, perm)
        with pytest.raises(ValueError, match="shape"):
            F.point_array(np.zeros(b), NPTS, shape)


@pytest.mark.parametrize("shape,perm,swap", [((3, 3), None, (1, 0)), ((2, 2), None, (1, 0)), ((2, 3, 2, 3), BLOCK_ORDER, MAJOR_SWAP),
                                             ((3, 6, 3, 6), BLOCK_ORDER, MAJOR_SWAP), ((2, 6, 2, 6), BLOCK_ORDER, MAJOR_SWAP)], ids=str)
def test_symmetry_is_of_bits(shape, perm, swap):
    rng = np.random.default_rng(7)
    v = rng.standard_normal((NPTS,) + shape)
    mirror = (0,) + tuple(1 + a for a in swap)
    sym = v + v.transpose(mirror)
    flat, s = F.point_block(sym, NPTS, shape, perm, swap)
    assert s is True and np.array_equal(flat, F.point_block(sym, NPTS, shape, perm))
    assert F.point_block(v, NPTS, shape, perm, swap)[1] is False
    # an entry off the diagonal and its mirror place
    at = (2,) + tuple(0 if k % 2 == 0 else 1 for k in range(len(shape)))
    at = at if len(shape) == 2 else (2, 0, 1, 1, 0)
    mat = (at[0],) + tuple(at[1 + a] for a in swap)
    assert at != mat
    ulp = sym.copy()
    ulp[at] = np.nextafter(ulp[at], np.inf)
    assert F.point_block(ulp, NPTS, shape, perm, swap)[1] is False
    zero = sym.copy()
    zero[at], zero[mat] = 0.0, -0.0
    assert F.point_block(zero, NPTS, shape, perm, swap)[1] is False
    zero[mat] = 0.0
    assert F.point_block(zero, NPTS, shape, perm, swap)[1] is True
    nan = sym.copy()
    nan[at] = nan[mat] = np.nan
    assert F.point_block(nan, NPTS, shape, perm, swap)[1] is True
    nan[mat] = 1.0
    assert F.point_block(nan, NPTS, shape, perm, swap)[1] is False
    # one symmetric block for every point
    assert F.point_block(sym[0], NPTS, shape, perm, swap)[1] is True


def test_same_bits():
    assert F._same_bits(np.array([np.nan, 1.0]), np.array([np.nan, 1.0]))
    assert not F._same_bits(np.array([0.0]), np.array([-0.0]))
    assert not F._same_bits(np.zeros(2), np.zeros((2, 1)))
