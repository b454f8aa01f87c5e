"""CPU: the FE-order entry points are declared and bound, and the numpy / scipy reference the GPU tests compare with
(tests/fe_order_reference.py) agrees with itself on the 56 reference patches of golden_random.npz."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import tigar_oracle as O
import fe_order_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["tg_nodes_locate", "tg_feorder_from_perm", "tg_feorder_info", "tg_feorder_download", "tg_feorder_destroy",
                "tg_csr_permute_sym", "tg_vec_permute"]


def golden_patches():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_random.npz"))
    for name in [str(n) for n in g["names"]]:
        degs = [int(v) for v in g[name + "/degrees"]]
        kvs = [[float(v) for v in g[name + "/kvec%d" % k]] for k in range(len(degs))]
        yield name, degs, kvs


def test_entry_points_declared_and_bound():
    from tigar_amd import _lib
    src = open(os.path.join(ROOT, "include", "tigar_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", src))
    for n in ENTRY_POINTS:
        assert n in declared, "%s is not declared in include/tigar_hip.h" % n
        assert n in _lib.PROTOTYPES, "%s has no ctypes prototype" % n
    hip = open(os.path.join(ROOT, "tigar_amd", "csrc", "tg_feorder.hip")).read()
    for n in ENTRY_POINTS:
        assert re.search(r'extern "C" int %s\(' % n, hip), n


def test_reference_locate_returns_the_permutation_on_the_golden_patches():
    rng = np.random.default_rng(2024)
    n = 0
    for name, degs, kvs in golden_patches():
        X, axes = O.fe_node_grid(O.BSpline(degs, kvs))
        perm = rng.permutation(X.shape[0])            # caller row i is grid node perm[i]
        g, inv, snap = R.locate([axes], X[perm])
        assert np.array_equal(g, perm), name
        assert np.array_equal(inv[perm], np.arange(len(perm))), name
        assert snap == 0.0
        # three fields on the one grid, rows interleaved node by node
        f = np.tile(np.arange(3), X.shape[0])
        g3, _, _ = R.locate([axes] * 3, np.repeat(X[perm], 3, axis=0), f)
        assert np.array_equal(g3, f * X.shape[0] + np.repeat(perm, 3)), name
        n += 1
    assert n == 56


def test_reference_locate_reports_what_is_wrong():
    rng = np.random.default_rng(7)
    for name, degs, kvs in golden_patches():
        X, axes = O.fe_node_grid(O.BSpline(degs, kvs))
        if X.shape[0] < 4:
            continue
        perm = rng.permutation(X.shape[0])
        Xp = X[perm]
        row = int(rng.integers(0, X.shape[0]))
        k = int(rng.integers(0, len(axes)))
        moved = Xp.copy()
        moved[row, k] += 0.3 * np.min(np.diff(axes[k]))
        with pytest.raises(R.Declined) as e:
            R.locate([axes], moved)
        assert (e.value.reason, e.value.row) == ("off the grid", row), name
        dup = Xp.copy()
        a, b = sorted(rng.choice(X.shape[0], 2, replace=False).tolist())
        dup[b] = dup[a]
        with pytest.raises(R.Declined) as e:
            R.locate([axes], dup)
        assert (e.value.reason, e.value.row) == ("two rows on one node", b), name
        with pytest.raises(R.Declined) as e:
            R.locate([axes], Xp[:-1])
        assert e.value.reason == "wrong row count", name
    # a few ulps are a match, and are reported
    name, degs, kvs = next(golden_patches())
    X, axes = O.fe_node_grid(O.BSpline(degs, kvs))
    g, _, snap = R.locate([axes], np.nextafter(X, np.inf))
    assert np.array_equal(g, np.arange(X.shape[0])) and snap > 0.0
    # a label moved to another field of the same grid
    f = np.tile(np.arange(3), X.shape[0])
    f[4] = 0                                          # row 4 is node 1 of field 1
    with pytest.raises(R.Declined) as e:
        R.locate([axes] * 3, np.repeat(X, 3, axis=0), f)
    assert (e.value.reason, e.value.row) == ("node of another field", 4)


def test_reference_permutations_agree_with_plain_indexing():
    rng = np.random.default_rng(11)
    n = 300
    A = sp.random(n, n, density=0.05, random_state=rng, format="csr")
    perm = rng.permutation(n)                         # grid_of_fe
    B = R.permute_sym(A, perm)
    assert B.has_sorted_indices and B.nnz == A.nnz
    Ad, Bd = A.toarray(), B.toarray()
    assert np.array_equal(Bd[np.ix_(perm, perm)], Ad)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(n)
    back = R.permute_sym(B, inv)
    assert np.array_equal(back.indptr, A.indptr) and np.array_equal(back.indices, A.indices)
    assert np.array_equal(back.data.view(np.int64), A.data.view(np.int64))
    x = rng.standard_normal(n)
    y = R.vec_to_grid(x, perm)
    assert np.array_equal(y[perm], x) and np.array_equal(R.vec_to_caller(y, perm), x)
    assert np.array_equal(B @ y, R.vec_to_grid(A @ x, perm)) or np.allclose(B @ y, R.vec_to_grid(A @ x, perm), rtol=1e-13)
