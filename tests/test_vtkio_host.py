"""CPU: the VTK writer (tigar_amd/vtkio.py, pure numpy) read back by the independent reader of tests/vtk_reader.py: both
encodings, d = 1, 2, 3, every array bit for bit, consistent offsets and byte counts, connectivity in range, positively
oriented lattice cells whose measures sum to the volume of an affine box within 4 eps."""
import os

import numpy as np
import pytest

import vtk_reader as V
from tigar_amd import vtkio

EPS = float(np.finfo(np.float64).eps)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _box_lattice(nel, m, lengths, seed=0):
    """the lattice points of an affine box with graded elements, numbered as tg_lattice_points: [npts, d]"""
    d = len(nel)
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, m)
    ax = []
    for k in range(d):
        v = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, nel[k]))])
        v *= lengths[k] / v[-1]
        v[-1] = lengths[k]
        ax.append(v[:-1, None] + np.diff(v)[:, None] * t[None, :])                 # [nel_k, m]
    pts = []
    for e in np.ndindex(*tuple(nel)[::-1]):
        for q in np.ndindex(*([m] * d)[::-1]):
            pts.append([ax[k][e[::-1][k], q[::-1][k]] for k in range(d)])
    return np.array(pts)


@pytest.mark.parametrize("encoding", ["raw", "ascii"])
@pytest.mark.parametrize("d,nel,m", [(1, (5,), 3), (2, (3, 2), 4), (3, (2, 1, 3), 2), (2, (1, 7), 2)])
def test_write_vtu_reads_back_bit_for_bit(tmp_path, encoding, d, nel, m):
    pts = _box_lattice(nel, m, [1.0, 2.0, 0.5][:d], seed=d)
    cells = vtkio.lattice_cells(nel, m, d)
    rng = np.random.default_rng(7)
    n = len(pts)
    data = {"scalar": rng.standard_normal(n), "pair": rng.standard_normal((n, 2)), "vector": rng.standard_normal((n, 3)),
            "column": rng.standard_normal((n, 1)), "tiny": rng.standard_normal(n) * 1e-310, "signed_zero": np.where(np.arange(n) % 2, -0.0, 0.0)}
    data["scalar"][0] = np.nextafter(1.0, 2.0)
    path = str(tmp_path / "sub" / ("out_%s.vtu" % encoding))                        # (the directory is created)
    vtkio.write_vtu(path, pts, cells, vtkio.CELL_TYPE_OF_DIM[d], data, encoding=encoding)
    got = V.read_vtu(path)
    assert got["n"] == n and got["ncells"] == len(cells) == (m - 1) ** d * int(np.prod(nel))
    assert got["points"].shape == (n, 3)
    assert _same_bits(got["points"][:, :d], pts) and np.all(got["points"][:, d:] == 0.0)      # padded to 3 components
    assert got["order"] == list(data)
    assert _same_bits(got["point_data"]["scalar"], data["scalar"]) and _same_bits(got["point_data"]["tiny"], data["tiny"])
    assert _same_bits(got["point_data"]["signed_zero"], data["signed_zero"])
    assert _same_bits(got["point_data"]["column"], data["column"][:, 0])
    assert _same_bits(got["point_data"]["vector"], data["vector"])
    assert _same_bits(got["point_data"]["pair"][:, :2], data["pair"]) and np.all(got["point_data"]["pair"][:, 2] == 0.0)
    # connectivity, offsets, types
    nv = 2 ** d
    assert np.array_equal(got["cells"], cells.ravel()) and got["cells"].min() >= 0 and got["cells"].max() < n
    assert np.array_equal(got["offsets"], nv * np.arange(1, len(cells) + 1))
    assert np.all(got["types"] == {1: 3, 2: 9, 3: 12}[d]) and got["types"].dtype == np.uint8
    if encoding == "raw":
        # every block: its header holds the byte count of its payload; the offsets chain without gaps and fill the blob
        at = 0
        for off, header, payload in sorted(got["blocks"]):
            assert off == at and header == payload
            at += 8 + payload
        assert at == got["blob_bytes"] and len(got["blocks"]) == len(data) + 4


@pytest.mark.parametrize("d,nel,m", [(1, (4,), 5), (2, (3, 2), 3), (2, (1, 7), 2), (3, (2, 2, 1), 3), (3, (1, 1, 1), 2)])
def test_lattice_cells_are_positive_and_fill_the_box(tmp_path, d, nel, m):
    lengths = [1.25, 2.0, 0.75][:d]
    pts = _box_lattice(nel, m, lengths, seed=11 * d)
    cells = vtkio.lattice_cells(nel, m, d)
    path = str(tmp_path / "box.vtu")
    vtkio.write_vtu(path, pts, cells, vtkio.CELL_TYPE_OF_DIM[d])
    got = V.read_vtu(path)
    meas = V.cell_measures(got["points"], got["cells"], got["offsets"], got["types"])
    assert np.all(meas > 0.0)
    vol = float(np.prod(lengths))
    # each cell's measure carries a few roundings, the sum of ncells terms of one sign at most ncells eps / 2 more: 4 eps in all
    # relative to the volume once the sum is formed in extended precision
    total = float(np.sum(meas.astype(np.longdouble)))
    assert abs(total - vol) <= 4 * EPS * vol
    # every cell of an element stays inside its element's block of points
    assert np.array_equal(cells.min(axis=1) // m ** d, cells.max(axis=1) // m ** d)
    assert len(np.unique(cells, axis=0)) == len(cells)


def test_grid_cells_of_a_node_grid():
    for shape in [(4,), (3, 5), (2, 3, 4)]:
        d = len(shape)
        cells = vtkio.grid_cells(shape)
        assert cells.shape == (int(np.prod([s - 1 for s in shape])), 2 ** d)
        ax = [np.arange(s, dtype=np.float64) for s in shape]
        X = np.stack([g.ravel(order="F") for g in np.meshgrid(*ax, indexing="ij")], axis=1)
        P = np.concatenate([X, np.zeros((len(X), 3 - d))], axis=1)
        meas = V.cell_measures(P, cells.ravel(), 2 ** d * np.arange(1, len(cells) + 1), [{1: 3, 2: 9, 3: 12}[d]] * len(cells))
        assert np.all(abs(meas - 1.0) <= 4 * EPS)              # (six tetrahedra of 1/6 each, by LU determinants)


def test_write_pvd(tmp_path):
    path = str(tmp_path / "series.pvd")
    steps = [(0.0, "series000000.vtu"), (0.125, "series000001.vtu"), (1e-3, "series000002.vtu")]
    vtkio.write_pvd(path, steps)
    assert V.read_pvd(path) == steps


def test_refusals(tmp_path):
    pts = np.zeros((4, 2))
    cells = np.array([[0, 1, 3, 2]])
    path = str(tmp_path / "x.vtu")
    with pytest.raises(ValueError, match="encoding"):
        vtkio.write_vtu(path, pts, cells, 9, encoding="base64")
    with pytest.raises(ValueError, match="cell type"):
        vtkio.write_vtu(path, pts, cells, 5)
    with pytest.raises(ValueError, match="vertices"):
        vtkio.write_vtu(path, pts, cells, 12)
    with pytest.raises(ValueError, match="refers to point"):
        vtkio.write_vtu(path, pts, np.array([[0, 1, 4, 2]]), 9)
    with pytest.raises(ValueError, match="point data"):
        vtkio.write_vtu(path, pts, cells, 9, {"f": np.zeros(3)})
    with pytest.raises(ValueError, match="point data"):
        vtkio.write_vtu(path, pts, cells, 9, {"f": np.zeros((4, 4))})
    with pytest.raises(ValueError, match="lattice_cells"):
        vtkio.lattice_cells((2, 2), 1, 2)
    assert not os.path.exists(path)


def test_importable_without_a_device():
    """the writer's module imports numpy and the standard library alone"""
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(vtkio))
    names = {a.name.split(".")[0] for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names}
    names |= {node.module.split(".")[0] for node in ast.walk(tree) if isinstance(node, ast.ImportFrom) and node.module}
    assert names <= {"os", "re", "numpy"}
