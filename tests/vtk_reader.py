"""A small reader of the VTK XML files tigar_amd/vtkio.py writes, independent of the writer (``xml.etree`` and
``numpy.frombuffer``): the tests read back what was written.  Handles one UnstructuredGrid piece with inline ASCII arrays or
appended raw data (``header_type="UInt64"``, little endian)."""
import xml.etree.ElementTree as ET

import numpy as np

_TYPES = {"Float64": "<f8", "Int64": "<i8", "UInt8": "<u1"}


def read_vtu(path):
    """{"points": [n, 3], "cells": flat connectivity, "offsets", "types", "point_data": {name: [n] or [n, 3]}, "order": the
    names of the point data in file order, "blocks": [(offset, header value, payload bytes)] of the appended arrays}"""
    raw = open(path, "rb").read()
    marker = b'<AppendedData encoding="raw">'
    blob = None
    if marker in raw:
        head, rest = raw.split(marker, 1)
        at = rest.index(b"_") + 1
        end = rest.rindex(b"</AppendedData>")
        blob = rest[at:end]
        assert blob.endswith(b"\n")
        blob = blob[:-1]
        raw = head + b"<AppendedData encoding=\"raw\"/>" + rest[end + len(b"</AppendedData>"):]
    root = ET.fromstring(raw)
    assert root.tag == "VTKFile" and root.get("type") == "UnstructuredGrid" and root.get("version") == "1.0"
    assert root.get("byte_order") == "LittleEndian" and root.get("header_type") == "UInt64"
    piece = root.find("UnstructuredGrid").find("Piece")
    n, ncells = int(piece.get("NumberOfPoints")), int(piece.get("NumberOfCells"))
    blocks = []

    def array(el):
        dt = np.dtype(_TYPES[el.get("type")])
        if el.get("format") == "ascii":
            words = (el.text or "").split()
            a = np.array([float(w) for w in words], dtype=dt) if dt.kind == "f" else np.array([int(w) for w in words], dtype=dt)
        else:
            assert el.get("format") == "appended"
            off = int(el.get("offset"))
            nbytes = int(np.frombuffer(blob, dtype="<u8", count=1, offset=off)[0])
            a = np.frombuffer(blob, dtype=dt, count=nbytes // dt.itemsize, offset=off + 8)
            blocks.append((off, nbytes, a.nbytes))
        nc = int(el.get("NumberOfComponents", "1"))
        return a.reshape(-1, nc) if nc > 1 else a
    out = {"n": n, "ncells": ncells, "point_data": {}, "order": [], "blocks": blocks}
    for el in piece.find("PointData").findall("DataArray"):
        out["point_data"][el.get("Name")] = array(el)
        out["order"].append(el.get("Name"))
    out["points"] = array(piece.find("Points").find("DataArray"))
    for el in piece.find("Cells").findall("DataArray"):
        out[{"connectivity": "cells"}.get(el.get("Name"), el.get("Name"))] = array(el)
    if blob is not None:
        out["blob_bytes"] = len(blob)
    return out


def read_pvd(path):
    """[(time, file)] of a collection file"""
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "Collection"
    return [(float(e.get("timestep")), e.get("file")) for e in root.find("Collection").findall("DataSet")]


def cell_measures(points, cells, offsets, types):
    """signed measure of every linear cell in VTK's vertex order: length (3), area in the plane spanned by the first two
    edges (9; shoelace in 3-D projected on the cell's own normal at vertex 0), volume (12; sum of the 6 tetrahedra of the
    Kuhn split around the diagonal 0 - 6)"""
    out = np.zeros(len(offsets))
    start = 0
    for c, (end, t) in enumerate(zip(offsets, types)):
        P = points[cells[start:end]]
        start = end
        if t == 3:
            out[c] = P[1, 0] - P[0, 0]
        elif t == 9:
            a = 0.5 * (np.cross(P[1] - P[0], P[2] - P[0]) + np.cross(P[2] - P[0], P[3] - P[0]))
            nrm = np.cross(P[1] - P[0], P[3] - P[0])
            out[c] = a @ nrm / np.linalg.norm(nrm)
        else:
            assert t == 12
            vol = 0.0
            for path in ((1, 2), (2, 3), (3, 7), (7, 4), (4, 5), (5, 1)):      # the ring of vertices around the diagonal 0 - 6
                vol += np.linalg.det(np.stack([P[6] - P[0], P[path[0]] - P[0], P[path[1]] - P[0]])) / 6.0
            out[c] = vol
    return out
