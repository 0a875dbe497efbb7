"""Every mesh file of the package, on the standard library and numpy: PLY read (ASCII, binary little-endian) and written (ASCII, with
or without vertex colours), OBJ geometry as the evaluation takes it from anywhere (read_obj) and template/uvmap.obj, the OBJ with
texture coordinates of the texture and
render stages (read_obj_uv / write_obj_uv).  The OBJ readers stay two parsers: one streams, counts a negative index back from the vertices
read so far and checks no range; the other counts from all `v` / `vt` lines, checks both ranges and demands a texture index."""
import os

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_FACE_LISTS = ("vertex_indices", "vertex_index")


def _ply_type(name):
    if name not in _PLY_TYPES:
        raise ValueError(f"read_ply: unknown property type {name!r}")
    return _PLY_TYPES[name]


def _ply_header(fh):
    """(format, [(element, count, [property])]); a property is (name, type) or (name, count type, item type)."""
    if fh.readline().strip() != b"ply":
        raise ValueError("read_ply: not a PLY file")
    fmt, elements = None, []
    while True:
        raw = fh.readline()
        if not raw:
            raise ValueError("read_ply: the header does not end")
        line = raw.decode("ascii", "replace").split()
        if not line or line[0] in ("comment", "obj_info"):
            continue
        if line[0] == "end_header":
            break
        if line[0] == "format":
            fmt = line[1]
        elif line[0] == "element":
            elements.append((line[1], int(line[2]), []))
        elif line[0] == "property":
            if not elements:
                raise ValueError("read_ply: a property before any element")
            if line[1] == "list":
                elements[-1][2].append((line[4], _ply_type(line[2]), _ply_type(line[3])))
            else:
                elements[-1][2].append((line[2], _ply_type(line[1])))
        else:
            raise ValueError(f"read_ply: unknown header line {' '.join(line)!r}")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"read_ply: format {fmt!r} is not read (ascii and binary_little_endian are)")
    return fmt, elements


def _face_rows(name, props):
    if name != "face":
        raise ValueError(f"read_ply: element {name!r} has a list property")
    lists = [p for p in props if len(p) == 3]
    if len(lists) != 1 or lists[0][0] not in _FACE_LISTS:
        raise ValueError("read_ply: the face element needs exactly one list, vertex_indices or vertex_index")
    return props.index(lists[0])


def _triangles(counts):
    if (np.asarray(counts) != 3).any():
        raise ValueError("read_ply: triangles only (a face with other than 3 corners)")


def read_ply(path):
    """(verts [V,3] float32 or float64 as stored, faces [F,3] int64) of a PLY file: ASCII or binary little-endian, float or double x /
    y / z, any further scalar vertex properties skipped, the face list named vertex_indices or vertex_index (further scalar face
    properties skipped), other elements of scalar properties skipped.  ValueError for anything else, and for a face that is not a
    triangle."""
    with open(path, "rb") as fh:
        fmt, elements = _ply_header(fh)
        verts = faces = None
        for name, count, props in elements:
            scalar = all(len(p) == 2 for p in props)
            if scalar:
                dtype = np.dtype([(p[0], "<" + p[1]) for p in props])
                if fmt == "ascii":
                    rows = np.array([fh.readline().split() for _ in range(count)], dtype=np.float64).reshape(count, len(props))
                    table = {p[0]: rows[:, i] for i, p in enumerate(props)}
                else:
                    data = fh.read(dtype.itemsize * count)
                    if len(data) != dtype.itemsize * count:
                        raise ValueError(f"read_ply: the file ends inside element {name!r}")
                    rec = np.frombuffer(data, dtype=dtype, count=count)
                    table = {p[0]: rec[p[0]] for p in props}
                if name == "vertex":
                    if not all(k in table for k in "xyz"):
                        raise ValueError("read_ply: the vertex element has no x, y, z")
                    kind = np.float64 if any(dict(props)[k] == "f8" for k in "xyz") else np.float32
                    verts = np.stack([np.asarray(table[k], dtype=kind) for k in "xyz"], 1)
                continue
            at = _face_rows(name, props)
            if fmt == "ascii":
                rows = [fh.readline().split() for _ in range(count)]
                _triangles([int(r[at]) if len(r) > at else 0 for r in rows])      # (scalars before the list take one token each)
                if any(len(r) != len(props) + 3 for r in rows):
                    raise ValueError("read_ply: a face line of the wrong length")
                faces = np.array([r[at + 1:at + 4] for r in rows], dtype=np.int64).reshape(count, 3)
            else:
                fields = []
                for p in props:
                    fields += [(p[0], "<" + p[1])] if len(p) == 2 else [("_n", "<" + p[1]), ("_i", "<" + p[2], (3,))]
                dtype = np.dtype(fields)
                data = fh.read(dtype.itemsize * count)
                first = np.frombuffer(data[:dtype.itemsize], dtype=dtype) if len(data) >= dtype.itemsize else None
                if first is not None:
                    _triangles(first["_n"])                                      # (a quad shifts every later record: look at the first alone)
                if len(data) != dtype.itemsize * count:
                    raise ValueError("read_ply: the file ends inside the face element (triangles only)")
                rec = np.frombuffer(data, dtype=dtype, count=count)
                _triangles(rec["_n"])
                faces = rec["_i"].astype(np.int64).reshape(count, 3)
    if verts is None:
        raise ValueError("read_ply: no vertex element")
    if faces is None:
        faces = np.zeros((0, 3), np.int64)
    return verts, faces


def write_ply(path, verts, faces, colors=None):
    """ASCII PLY of a triangle mesh (verts [V,3] float, faces [F,3] int).  `colors` [V,3] uint8, when given, are written as `uchar
    red / green / blue` vertex properties (read_ply skips them); without them the file is what it always was."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if colors is not None:
        c = np.asarray(colors)
        if c.dtype != np.uint8 or c.shape != v.shape:
            raise ValueError(f"write_ply: colors [{len(v)},3] uint8 expected, got {c.dtype} {c.shape}")
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % (len(v), "" if colors is None else "property uchar red\nproperty uchar green\nproperty uchar blue\n", len(f)))
        if colors is None:
            fh.writelines("%.9g %.9g %.9g\n" % tuple(p) for p in v.tolist())
        else:
            fh.writelines("%.9g %.9g %.9g %d %d %d\n" % (*p, *q) for p, q in zip(v.tolist(), c.tolist()))
        fh.writelines("3 %d %d %d\n" % tuple(t) for t in f.tolist())


def read_obj(path):
    """(verts [V,3] float64, faces [F,3] int64, 0-based) of a Wavefront OBJ: `v x y z ...` and `f` lines with corners `a`, `a/b`,
    `a//c` or `a/b/c`; a negative index counts back from the vertices read so far.  Everything else is skipped.  ValueError for a
    face that is not a triangle."""
    verts, faces = [], []
    with open(path, "r") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                if len(tok) != 4:
                    raise ValueError(f"read_obj: triangles only, got a face of {len(tok) - 1} corners")
                tri = []
                for corner in tok[1:]:
                    i = int(corner.split("/")[0])
                    if i == 0:
                        raise ValueError("read_obj: vertex index 0")
                    tri.append(i - 1 if i > 0 else len(verts) + i)
                faces.append(tri)
    return np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)


def _obj_index(tok, n, what, line):
    i = int(tok)
    i = i - 1 if i > 0 else n + i
    if not 0 <= i < n:
        raise ValueError(f"{what} index {tok} out of range in '{line}'")
    return i


def read_obj_uv(path):
    """(verts [V,3] float32, faces [F,3] int64, vt [Vt,2] float32, ft [F,3] int64) of a Wavefront OBJ with `v`, `vt` and triangular
    `f a/b[/c]` lines (what template/uvmap.obj holds).  Faces with more than three corners or without texture indices raise."""
    with open(path) as fh:
        rows = [(ln.strip(), ln.split()) for ln in fh]
    v = [[float(x) for x in tok[1:4]] for _, tok in rows if tok[:1] == ["v"]]
    vt = [[float(x) for x in tok[1:3]] for _, tok in rows if tok[:1] == ["vt"]]
    f, ft = [], []
    for ln, tok in rows:
        if tok[:1] != ["f"]:
            continue
        if len(tok) != 4:
            raise ValueError(f"{path}: only triangles are supported, got '{ln}'")
        a, b = [], []
        for corner in tok[1:]:
            parts = corner.split("/")
            if len(parts) < 2 or not parts[1]:
                raise ValueError(f"{path}: face corner without a texture index in '{ln}'")
            a.append(_obj_index(parts[0], len(v), "vertex", ln)); b.append(_obj_index(parts[1], len(vt), "texture", ln))
        f.append(a); ft.append(b)
    if not v or not f or not vt:
        raise ValueError(f"{path}: no vertices, texture coordinates or faces")
    return (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3), np.asarray(vt, np.float32).reshape(-1, 2),
            np.asarray(ft, np.int64).reshape(-1, 3))


def write_obj_uv(path, verts, faces, vt, ft):
    """The OBJ `read_obj_uv` reads: `v x y z`, `vt u v`, `f a/ta b/tb c/tc` (1-based)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3); t = np.asarray(vt, np.float32).reshape(-1, 2)
    f = np.asarray(faces, np.int64).reshape(-1, 3); g = np.asarray(ft, np.int64).reshape(-1, 3)
    if f.shape != g.shape:
        raise ValueError(f"faces {f.shape} and ft {g.shape} must correspond one to one")
    with open(path, "w") as fh:
        fh.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist())
        fh.writelines("vt %.9g %.9g\n" % tuple(p) for p in t.tolist())
        fh.writelines("f %d/%d %d/%d %d/%d\n" % (a[0] + 1, b[0] + 1, a[1] + 1, b[1] + 1, a[2] + 1, b[2] + 1) for a, b in zip(f.tolist(), g.tolist()))


def read_mesh(path):
    """read_ply or read_obj by the file's extension."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".ply":
        return read_ply(path)
    if ext == ".obj":
        return read_obj(path)
    raise ValueError(f"read_mesh: {path}: .ply or .obj expected")
