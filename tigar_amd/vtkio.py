"""VTK XML output in pure numpy: what the reference's demos end with (``File("results/u.pvd") << u``) and the sampled
output of a solution on its physical patch (``ExtractedSpline.writeVTK``).  No device is needed to import or use the writer.

``write_vtu`` writes one UnstructuredGrid piece (version 1.0, little endian, ``header_type="UInt64"``), the arrays as
appended raw data (every block preceded by its byte count as one UInt64; offsets count from the byte after the ``_``) or
inline as ASCII (``repr`` of every number: they read back bit for bit).  Cells are linear: VTK_LINE 3, VTK_QUAD 9,
VTK_HEXAHEDRON 12, in VTK's vertex order.  ``write_pvd`` writes the collection file of a time series.

``File`` is the reference's idiom: ``File(path) << u`` writes the FE function on its PARAMETRIC mesh -- the node grid of
``u.function_space()`` as points, the p^d linear cells per element between neighbouring nodes, the nodal values under
``u.name()`` -- which is what dolfin writes for a function of degree p on the knot mesh; a second ``<<`` to the same
``.pvd`` appends a step.
"""
import os
import re

import numpy

VTK_LINE, VTK_QUAD, VTK_HEXAHEDRON = 3, 9, 12
CELL_TYPE_OF_DIM = {1: VTK_LINE, 2: VTK_QUAD, 3: VTK_HEXAHEDRON}
_CELL_VERTICES = {VTK_LINE: 2, VTK_QUAD: 4, VTK_HEXAHEDRON: 8}
# corners of the unit cell in VTK's order, as offsets (i0, i1, i2)
_VTK_CORNERS = {1: [(0, 0, 0), (1, 0, 0)],
                2: [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)],
                3: [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]}


def _pad3(a, n, what):
    """[n] or [n, c], c = 1, 2, 3 -> (array of c' in (1, 3) components, c'): a 2-vector is padded with 0"""
    a = numpy.asarray(a, dtype=numpy.float64)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[0] != n or a.shape[1] not in (1, 2, 3):
        raise ValueError("%s: an array of shape %s for %d points; expected [%d] or [%d, c] with c = 1, 2, 3"
                         % (what, a.shape, n, n, n))
    if a.shape[1] == 2:
        a = numpy.concatenate([a, numpy.zeros((n, 1))], axis=1)
    return numpy.ascontiguousarray(a), a.shape[1]


def _ascii(a):
    if a.dtype.kind == "f":
        return " ".join(repr(float(v)) for v in a.ravel())
    return " ".join(str(int(v)) for v in a.ravel())


def write_vtu(path, points, cells, cell_type, point_data=None, encoding="raw"):
    """One VTK XML UnstructuredGrid file: ``points`` [n, 1..3] (padded to 3 components), ``cells`` [ncells, vertices of
    the type] with point indices in VTK's order, one ``cell_type`` (3, 9, 12) for all, ``point_data`` {name: [n] or [n, 1..3]}
    in the order given (a 2-vector is padded with 0).  ``encoding``: "raw" (appended raw data) or "ascii"."""
    if encoding not in ("raw", "ascii"):
        raise ValueError("write_vtu: encoding %r; 'raw' or 'ascii'" % (encoding,))
    if cell_type not in _CELL_VERTICES:
        raise ValueError("write_vtu: cell type %r; VTK_LINE 3, VTK_QUAD 9 or VTK_HEXAHEDRON 12" % (cell_type,))
    pts = numpy.asarray(points, dtype=numpy.float64)
    if pts.ndim == 1:
        pts = pts[:, None]
    n = pts.shape[0]
    if pts.ndim != 2 or pts.shape[1] not in (1, 2, 3):
        raise ValueError("write_vtu: points of shape %s; expected [n, 1..3]" % (pts.shape,))
    pts = numpy.ascontiguousarray(numpy.concatenate([pts, numpy.zeros((n, 3 - pts.shape[1]))], axis=1))
    cells = numpy.ascontiguousarray(cells, dtype=numpy.int64)
    nv = _CELL_VERTICES[cell_type]
    if cells.ndim != 2 or cells.shape[1] != nv:
        raise ValueError("write_vtu: cells of shape %s; cell type %d has %d vertices" % (cells.shape, cell_type, nv))
    if cells.size and (cells.min() < 0 or cells.max() >= n):
        raise ValueError("write_vtu: a cell refers to point %d of %d" % (int(cells.max() if cells.max() >= n else cells.min()), n))
    ncells = cells.shape[0]
    arrays = []                                        # (xml attributes, array) in file order
    for name, a in (point_data or {}).items():
        a, nc = _pad3(a, n, "write_vtu: point data %r" % (name,))
        arrays.append(('type="Float64" Name="%s" NumberOfComponents="%d"' % (name, nc), a))
    npd = len(arrays)
    arrays.append(('type="Float64" Name="Points" NumberOfComponents="3"', pts))
    arrays.append(('type="Int64" Name="connectivity"', cells))
    arrays.append(('type="Int64" Name="offsets"', nv * numpy.arange(1, ncells + 1, dtype=numpy.int64)))
    arrays.append(('type="UInt8" Name="types"', numpy.full(ncells, cell_type, dtype=numpy.uint8)))
    tags, offset = [], 0
    for attrs, a in arrays:
        if encoding == "raw":
            tags.append('<DataArray %s format="appended" offset="%d"/>' % (attrs, offset))
            offset += 8 + a.nbytes
        else:
            tags.append('<DataArray %s format="ascii">%s</DataArray>' % (attrs, _ascii(a)))
    head = ['<?xml version="1.0"?>',
            '<VTKFile type="UnstructuredGrid" version="1.0" byte_order="LittleEndian" header_type="UInt64">',
            '<UnstructuredGrid>', '<Piece NumberOfPoints="%d" NumberOfCells="%d">' % (n, ncells), '<PointData>']
    head += tags[:npd] + ['</PointData>', '<Points>', tags[npd], '</Points>', '<Cells>'] + tags[npd + 1:]
    head += ['</Cells>', '</Piece>', '</UnstructuredGrid>']
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if encoding == "raw":
            f.write(b'<AppendedData encoding="raw">\n_')
            for _, a in arrays:
                f.write(numpy.uint64(a.nbytes).astype("<u8").tobytes())
                f.write(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes())
            f.write(b'\n</AppendedData>\n')
        f.write(b'</VTKFile>\n')


def write_pvd(path, steps):
    """the collection file of a time series: ``steps`` = [(time, file name relative to the collection), ...]"""
    lines = ['<?xml version="1.0"?>', '<VTKFile type="Collection" version="1.0" byte_order="LittleEndian" header_type="UInt64">',
             '<Collection>']
    for t, name in steps:
        lines.append('<DataSet timestep="%s" part="0" file="%s"/>' % (repr(float(t)), name))
    lines += ['</Collection>', '</VTKFile>']
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _grid_cells(counts, strides_of, d):
    """the linear cells between neighbouring points of index boxes: ``counts[k]`` cells per direction, the point (i0, i1,
    i2) at ``strides_of(i)``; cells lexicographic with direction 0 fastest, VTK's vertex order"""
    idx = numpy.meshgrid(*[numpy.arange(c, dtype=numpy.int64) for c in counts], indexing="ij")
    idx = [g.ravel(order="F") for g in idx] + [numpy.zeros(1, dtype=numpy.int64)] * (3 - d)
    return numpy.stack([strides_of([idx[k] + c[k] for k in range(3)]) for c in _VTK_CORNERS[d]], axis=1)


def lattice_cells(nel, m, d):
    """The (m - 1)^d linear cells of every element on the element-major lattice numbering of ``tg_lattice_points`` (elements
    lexicographic with direction 0 fastest, the m^d points of an element likewise; points on shared element faces are
    duplicates): [(m - 1)^d prod nel, 2^d] point indices in VTK's vertex order, cells element by element."""
    nel = [int(e) for e in nel]
    m = int(m)
    if len(nel) != d or d not in (1, 2, 3) or m < 2:
        raise ValueError("lattice_cells: d = %r directions with %r elements and m = %r >= 2 points per element and direction"
                         % (d, nel, m))
    local = _grid_cells([m - 1] * d, lambda i: i[0] + m * (i[1] + m * i[2]), d)
    nelem = int(numpy.prod(nel))
    return (local[None, :, :] + (m ** d) * numpy.arange(nelem, dtype=numpy.int64)[:, None, None]).reshape(-1, 2 ** d)


def grid_cells(shape):
    """the linear cells between neighbouring points of a tensor grid of ``shape`` points (direction 0 fastest)"""
    d = len(shape)
    n = [int(s) for s in shape] + [1] * (3 - d)
    return _grid_cells([s - 1 for s in n[:d]], lambda i: i[0] + n[0] * (i[1] + n[1] * i[2]), d)


def read_pvd(path):
    """[(time, file), ...] of a collection file written by ``write_pvd``; [] when there is none"""
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [(float(t), name) for t, name in re.findall(r'<DataSet timestep="([^"]*)" part="0" file="([^"]*)"/>', f.read())]


def _series_step(path, state, time, write):
    """``path``.vtu: ``write(path)``; ``path``.pvd: a further step of the collection ON DISK -- whoever wrote the earlier steps
    (another ``File``, another spline, an earlier run): step number k = its length goes to stem%06d.vtu and the collection is
    rewritten with it appended.  ``state`` (a list kept by the caller) is brought to the same content."""
    stem, ext = os.path.splitext(path)
    if ext == ".vtu":
        write(path)
        return path
    if ext != ".pvd":
        raise ValueError("VTK output goes to a .vtu file or a .pvd collection, not %r" % (path,))
    state[:] = read_pvd(path)
    k = len(state)
    name = "%s%06d.vtu" % (stem, k)
    write(name)
    state.append((float(k) if time is None else float(time), os.path.basename(name)))
    write_pvd(path, state)
    return name


class File(object):
    """``File(path) << u`` and ``File(path) << (u, t)``: the reference's output idiom (dolfin's ``File``).  ``u`` is an FE
    ``Function`` on continuous tensor node grids, any number of fields sharing one grid; it is written on the PARAMETRIC
    mesh: the node grid as points, the linear cells between neighbouring nodes (p^d per element), the nodal values under
    ``u.name()`` -- one array with 3 components for 2 or 3 fields (dolfin's vector functions), ``name_i`` per field beyond.
    A ``.pvd`` path collects one ``.vtu`` per ``<<`` (appended to the collection found on disk, whoever wrote it; delete
    the ``.pvd`` to start a new series); a ``.vtu`` path is overwritten."""

    def __init__(self, path, encoding="raw"):
        self.path, self.encoding, self.steps = str(path), encoding, []

    def __lshift__(self, what):
        u, t = what if isinstance(what, (tuple, list)) else (what, None)
        grids = getattr(u.function_space(), "grids", None)
        g = grids[0] if grids else None
        if g is None or any(not hasattr(gi, "axes") or gi.dg or gi.shape() != g.shape() for gi in grids):
            raise NotImplementedError("File << u: functions on continuous tensor node grids sharing one grid are written; "
                                      "multi-patch, T-spline, DG and mixed-degree spaces are not")
        shape, nf = g.shape(), len(grids)
        vals = numpy.asarray(u.vector().get_local(), dtype=numpy.float64)
        if vals.size != nf * g.num_nodes():
            raise NotImplementedError("File << u: the function holds %d of the %d nodal values (several ranks are not supported)"
                                      % (vals.size, nf * g.num_nodes()))
        vals = vals.reshape(nf, g.num_nodes()).T
        name = u.name() if hasattr(u, "name") else "f"
        if nf == 1:
            data = {name: vals[:, 0]}
        elif nf <= 3:
            data = {name: vals}
        else:
            data = {"%s_%d" % (name, i): vals[:, i] for i in range(nf)}
        pts, cells, ct = g.coordinates(), grid_cells(shape), CELL_TYPE_OF_DIM[g.dim()]
        _series_step(self.path, self.steps, t, lambda f: write_vtu(f, pts, cells, ct, data, self.encoding))
        return self
