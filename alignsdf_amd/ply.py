"""Minimal binary PLY writer (little endian): float32 x,y,z vertices + `list uchar int` triangle faces -
the layout both writers of the reference produce (trimesh export at utils/mesh.py:397, plyfile at
deep_sdf/mesh.py:107-112)."""
import numpy as np


def write_ply(path, verts, faces, normals=None, quality=None):
    """normals [V, 3] (optional): written as `property float nx / ny / nz` behind z; quality [V] (optional): one more float per vertex,
    `property float quality`, behind z / nz (the name mesh viewers colour by); without them the file is the layout above."""
    verts = np.ascontiguousarray(verts, dtype="<f4").reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype="<i4").reshape(-1, 3)
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype="<f4").reshape(-1, 3)
        if len(normals) != len(verts):
            raise ValueError("%d normals for %d vertices" % (len(normals), len(verts)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
        verts = np.ascontiguousarray(np.hstack([verts, normals]))
    if quality is not None:
        quality = np.ascontiguousarray(quality, dtype="<f4").reshape(-1, 1)
        if len(quality) != len(verts):
            raise ValueError("%d quality values for %d vertices" % (len(quality), len(verts)))
        props += "property float quality\n"
        verts = np.ascontiguousarray(np.hstack([verts, quality]))
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\nproperty list uchar int vertex_indices\n"
              "end_header\n" % (len(verts), props, len(faces)))
    rec = np.empty(len(faces), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = faces
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(verts.tobytes())
        f.write(rec.tobytes())


_PLY_SCALARS = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4", "float": "<f4", "double": "<f8",
                "int8": "i1", "uint8": "u1", "int16": "<i2", "uint16": "<u2", "int32": "<i4", "uint32": "<u4", "float32": "<f4",
                "float64": "<f8"}


def read_ply(path, with_normals=False, with_quality=False):
    """Inverse of write_ply: (verts, faces), or (verts, faces, normals or None) with with_normals=True; with_quality=True appends
    the `quality` column (or None) to either.  The vertex record is taken from the header's scalar properties, so files with normals
    (or other per-vertex scalars) read correctly."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    nv = nf = 0
    element, fields = None, []
    for line in data[:end].decode("ascii").splitlines():
        word = line.split()
        if line.startswith("element"):
            element = word[1]
            if element == "vertex":
                nv = int(word[-1])
            if element == "face":
                nf = int(word[-1])
        elif line.startswith("property") and element == "vertex":
            if word[1] == "list":
                raise ValueError("list property %r on the vertex element" % word[-1])
            fields.append((word[2], _PLY_SCALARS[word[1]]))
    vrec = np.frombuffer(data, dtype=np.dtype(fields), count=nv, offset=end)
    verts = np.stack([vrec[k] for k in ("x", "y", "z")], 1).astype(np.float32)
    rec = np.frombuffer(data, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nf, offset=end + nv * vrec.dtype.itemsize)
    names = vrec.dtype.names
    out = (verts, rec["idx"].copy())
    if with_normals:
        out += (np.stack([vrec[k] for k in ("nx", "ny", "nz")], 1).astype(np.float32) if all(k in names for k in ("nx", "ny", "nz")) else None,)
    if with_quality:
        out += (vrec["quality"].astype(np.float32) if "quality" in names else None,)
    return out


def write_ply_ascii(path, verts, faces=None, vertex_colors=None):
    """ASCII PLY with optional per-vertex RGB(A) colours: the text layout of the reference's customized_export_ply
    for the (v, f, v_c) combination it is called with (utils/customized_export_ply.py:49-119 - `%f` coordinates,
    `uchar` red/green/blue/alpha with alpha 255 when only RGB is given, `3 i j k` faces)."""
    verts = np.asarray(verts).reshape(-1, 3)
    faces = np.zeros((0, 3), dtype=np.int64) if faces is None else np.asarray(faces).reshape(-1, 3)
    head = ["ply", "format ascii 1.0", "element vertex %d" % len(verts), "property float x", "property float y", "property float z"]
    if vertex_colors is not None:
        vc = np.asarray(vertex_colors)
        if vc.shape[1] == 3:
            vc = np.hstack([vc, np.full((len(vc), 1), 255, dtype=np.uint8)])
        head += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
        body = ["%f %f %f %d %d %d %d" % (v[0], v[1], v[2], c[0], c[1], c[2], c[3]) for v, c in zip(verts.tolist(), vc.tolist())]
    else:
        body = ["%f %f %f" % tuple(v) for v in verts.tolist()]
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    body += ["3 %d %d %d" % tuple(f) for f in faces.tolist()]
    with open(path, "w") as f:
        f.write("\n".join(head + body) + "\n")
