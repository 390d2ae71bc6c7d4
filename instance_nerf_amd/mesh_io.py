"""Binary little-endian PLY files of triangle meshes: ``write_ply`` / ``read_ply``.  Pure numpy (the machines this runs on
have no trimesh / plyfile).  Layout: ``element vertex`` with ``float x, y, z`` and optionally ``uchar red, green, blue``;
``element face`` with ``list uchar int vertex_indices`` and optionally ``uchar label`` (the instance id of the face)."""
import os

import numpy as np

_PLY_TYPES = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4", "float": "<f4",
              "double": "<f8", "int8": "i1", "uint8": "u1", "int16": "<i2", "uint16": "<u2", "int32": "<i4",
              "uint32": "<u4", "float32": "<f4", "float64": "<f8"}


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def write_ply(path, vertices, faces, colors=None, face_labels=None):
    """vertices [V, 3] float; faces [F, 3] int; colors [V, 3] uint8, or float in [0, 1] (rounded to 0..255); face_labels
    [F] uint8.  Tensors or arrays.  -> path."""
    v = np.ascontiguousarray(_host(vertices), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(_host(faces), dtype="<i4").reshape(-1, 3)
    vt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = _host(colors)
        if c.dtype != np.uint8:
            c = np.clip(np.rint(np.nan_to_num(c.astype(np.float64)) * 255.0), 0, 255).astype(np.uint8)
        c = c.reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError("write_ply: one colour per vertex")
        vt += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    ft = [("n", "u1"), ("vertex_indices", "<i4", (3,))]
    if face_labels is not None:
        lab = _host(face_labels).astype(np.uint8).reshape(-1)
        if len(lab) != len(f):
            raise ValueError("write_ply: one label per face")
        ft += [("label", "u1")]
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("write_ply: a face names a vertex that does not exist")
    vrec = np.zeros(len(v), dtype=np.dtype(vt))
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.zeros(len(f), dtype=np.dtype(ft))
    frec["n"] = 3
    frec["vertex_indices"] = f
    if face_labels is not None:
        frec["label"] = lab
    head = ["ply", "format binary_little_endian 1.0", "comment instance_nerf_amd mesh", f"element vertex {len(v)}",
            "property float x", "property float y", "property float z"]
    if colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices"]
    if face_labels is not None:
        head += ["property uchar label"]
    head += ["end_header"]
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
    return path


def read_ply_header(fh):
    """Parses the header by the PLY grammar -> (format, [(element, count, [property, ...])]); a property is
    ("scalar", type, name) or ("list", count type, item type, name).  Leaves ``fh`` at the first byte of the body."""
    if fh.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError("PLY header without end_header")
        tok = line.decode("ascii").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = (tok[1], tok[2])
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("PLY property before any element")
            if tok[1] == "list":
                elements[-1][2].append(("list", tok[2], tok[3], tok[4]))
            else:
                elements[-1][2].append(("scalar", tok[1], tok[2]))
        elif tok[0] == "end_header":
            return fmt, elements
        else:
            raise ValueError(f"PLY header: unknown keyword {tok[0]!r}")


def read_ply(path):
    """Reads a binary little-endian PLY of triangles -> dict ``vertices`` float32 [V, 3], ``faces`` int32 [F, 3],
    ``colors`` uint8 [V, 3] or None, ``face_labels`` uint8 [F] or None."""
    with open(path, "rb") as fh:
        fmt, elements = read_ply_header(fh)
        if fmt != ("binary_little_endian", "1.0"):
            raise ValueError(f"read_ply: only binary_little_endian 1.0 (found {fmt})")
        data = {}
        for name, count, props in elements:
            fields = []
            for p in props:
                if p[0] == "scalar":
                    fields.append((p[2], _PLY_TYPES[p[1]]))
                else:                                        # triangles only: every list holds three items
                    fields += [(p[3] + "#n", _PLY_TYPES[p[1]]), (p[3], _PLY_TYPES[p[2]], (3,))]
            dt = np.dtype(fields)
            rec = np.frombuffer(fh.read(dt.itemsize * count), dtype=dt)
            if len(rec) != count:
                raise ValueError(f"read_ply: element {name} is truncated")
            for p in props:
                if p[0] == "list" and count and not (rec[p[3] + "#n"] == 3).all():
                    raise ValueError("read_ply: only triangles are supported")
            data[name] = rec
    v, f = data["vertex"], data["face"]
    out = {"vertices": np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32) if len(v) else np.zeros((0, 3), np.float32),
           "faces": np.ascontiguousarray(f["vertex_indices"]).astype(np.int32).reshape(-1, 3), "colors": None,
           "face_labels": None}
    if "red" in (v.dtype.names or ()):
        out["colors"] = np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.uint8).reshape(-1, 3)
    if "label" in (f.dtype.names or ()):
        out["face_labels"] = np.ascontiguousarray(f["label"]).astype(np.uint8)
    return out
