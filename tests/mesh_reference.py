"""Plain numpy (float32) restatement of the iso-surface mesh extraction documented in include/inr.h ("iso-surface meshes of
a lattice field"): marching tetrahedra over the Kuhn split of every lattice cell.  Written from that comment, not from
the kernels: vertices are welded through a dictionary keyed by (owner point, direction), triangles come from a loop over
cells.  It is the yardstick of tests/test_mesh_cpu.py and tests/test_mesh_extract.py, so it stays slow and obvious; only
the search for crossed edges and for cells with a surface runs on whole arrays (a lattice of half a million points takes
seconds, not minutes)."""
import numpy as np

f32 = np.float32

# tetrahedron t -> its four cube corners (corner code = 4 dw + 2 dl + dh), one per order in which the axes are added
TETS = [(0, 4, 6, 7), (0, 4, 5, 7), (0, 2, 6, 7), (0, 2, 3, 7), (0, 1, 5, 7), (0, 1, 3, 7)]
MIRRORED = (False, True, True, False, False, True)          # odd axis permutations
# tetrahedron edge -> its two tetrahedron vertices
EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
# case (sum of 2^i over the inside tetrahedron vertices) -> triangles as triples of tetrahedron edges
CASES = {
    0: [], 15: [],
    1: [(0, 1, 2)], 2: [(0, 4, 3)], 3: [(1, 2, 4), (1, 4, 3)], 4: [(1, 3, 5)], 5: [(0, 5, 2), (0, 3, 5)],
    6: [(0, 4, 5), (0, 5, 1)], 7: [(2, 4, 5)], 8: [(2, 5, 4)], 9: [(0, 1, 5), (0, 5, 4)], 10: [(0, 5, 3), (0, 2, 5)],
    11: [(1, 5, 3)], 12: [(1, 3, 4), (1, 4, 2)], 13: [(0, 3, 4)], 14: [(0, 2, 1)],
}


def corner(c):
    return (c >> 2) & 1, (c >> 1) & 1, c & 1


def extended_axis(ax, pad, ext):
    """The axis with its virtual first and last point (pad = 1): continued by the first / last step, or by `ext` for an
    axis of length 1.  float32, one rounding per operation."""
    ax = np.asarray(ax, dtype=f32)
    if not pad:
        return ax
    n = len(ax)
    lo = ax[0] - ((ax[1] - ax[0]) if n >= 2 else f32(ext))
    hi = ax[n - 1] + ((ax[n - 1] - ax[n - 2]) if n >= 2 else f32(ext))
    return np.concatenate([[f32(lo)], ax, [f32(hi)]]).astype(f32)


def clamped_field(field, iso, clamp, labels=None, select=-1, cap=True):
    """-> float32 [Ew, El, Eh]: the values the interpolation sees (virtual, NaN and masked-out points: iso - clamp)."""
    iso, clamp = f32(iso), f32(clamp)
    lo, hi = f32(iso - clamp), f32(iso + clamp)
    v = np.asarray(field, dtype=f32)
    with np.errstate(invalid="ignore"):
        g = np.minimum(np.maximum(v, lo), hi).astype(f32)
    g[np.isnan(v)] = lo
    if select >= 0:
        g[np.asarray(labels) != select] = lo
    if cap:
        g = np.pad(g, 1, constant_values=lo)
    return g


def marching_tetrahedra(field, iso, clamp, axes, labels=None, select=-1, rgb=None, cap=True, ext=(1.0, 1.0, 1.0),
                        want_face_labels=None):
    """field [W, L, H]; axes = three float32 coordinate arrays; labels uint8 [W, L, H] or None; rgb [W, L, H, >=3] or None.
    -> dict: vertices float32 [V, 3], faces int32 [F, 3], colors float32 [V, 3] / None, face_labels uint8 [F] / None,
    owners int64 [V, 4] = (ew, el, eh, direction code) in the extended lattice, t float32 [V], g = the clamped field."""
    iso = f32(iso)
    pad = 1 if cap else 0
    g = clamped_field(field, iso, clamp, labels, select, cap)
    inside = g >= iso
    E = g.shape
    pos = [extended_axis(axes[k], pad, ext[k]) for k in range(3)]
    if want_face_labels is None:
        want_face_labels = labels is not None

    # ---- vertices: every crossed edge p -> p + d, ordered by owner point (w, l, h; h fastest), then direction code 1..7
    # (the crossing test of every (point, direction) is taken on whole arrays; argwhere walks them in exactly that order)
    vertex_id = {}
    owners, ts = [], []
    if min(E) >= 2:
        crossed = np.zeros(E + (7,), bool)
        for c in range(1, 8):
            dw, dl, dh = corner(c)
            p = inside[:E[0] - dw, :E[1] - dl, :E[2] - dh]
            crossed[:E[0] - dw, :E[1] - dl, :E[2] - dh, c - 1] = p != inside[dw:, dl:, dh:]
        for ew, el, eh, k in np.argwhere(crossed).tolist():
            vertex_id[(ew, el, eh, k + 1)] = len(owners)
            owners.append((ew, el, eh, k + 1))
    V = len(owners)
    vertices = np.zeros((V, 3), f32)
    colors = np.zeros((V, 3), f32) if rgb is not None else None
    tvals = np.zeros(V, f32)
    rgb = None if rgb is None else np.asarray(rgb, dtype=f32)
    W, L, H = np.asarray(field).shape

    def real(p):
        return all(0 <= p[k] - pad < (W, L, H)[k] for k in range(3))

    for i, (ew, el, eh, c) in enumerate(owners):
        p = (ew, el, eh)
        q = tuple(p[k] + corner(c)[k] for k in range(3))
        a, b = g[p], g[q]
        t = f32(f32(iso - a) / f32(b - a))
        tvals[i] = t
        for k in range(3):
            xp, xq = pos[k][p[k]], pos[k][q[k]]
            vertices[i, k] = f32(xp + f32(t * f32(xq - xp)))
        if rgb is not None:
            rp, rq = real(p), real(q)
            for k in range(3):
                cp = rgb[p[0] - pad, p[1] - pad, p[2] - pad, k] if rp else rgb[q[0] - pad, q[1] - pad, q[2] - pad, k]
                cq = rgb[q[0] - pad, q[1] - pad, q[2] - pad, k] if rq else cp
                colors[i, k] = f32(cp + f32(t * f32(cq - cp)))

    # ---- triangles: by cell (named by its corner 0) in the same order, then tetrahedron 0..5, then the table's order
    faces, flabels = [], []
    inside_count = np.zeros(tuple(max(n - 1, 0) for n in E), np.int64)
    if min(E) >= 2:
        for c in range(8):
            dw, dl, dh = corner(c)
            inside_count += inside[dw:E[0] - 1 + dw, dl:E[1] - 1 + dl, dh:E[2] - 1 + dh]
    for ew, el, eh in np.argwhere((inside_count > 0) & (inside_count < 8)).tolist():       # the cells a surface passes through
        for t, tet in enumerate(TETS):
            pts = [(ew + corner(c)[0], el + corner(c)[1], eh + corner(c)[2]) for c in tet]
            m = sum(1 << i for i in range(4) if inside[pts[i]])
            tris = CASES[m]
            if not tris:
                continue
            label = 255
            if want_face_labels:
                best = None
                for i in range(4):
                    if inside[pts[i]] and (best is None or g[pts[i]] > g[pts[best]]):
                        best = i
                bw, bl, bh = pts[best]
                label = int(labels[bw - pad, bl - pad, bh - pad])
            for tri in tris:
                ids = []
                for e in tri:
                    i, j = EDGES[e]
                    code = tet[j] - tet[i]                 # the corners of a tetrahedron are nested: j adds axes to i
                    ids.append(vertex_id[pts[i] + (code,)])
                if MIRRORED[t]:
                    ids = [ids[0], ids[2], ids[1]]
                faces.append(ids)
                flabels.append(label)
    return {"vertices": vertices, "faces": np.asarray(faces, np.int32).reshape(-1, 3),
            "colors": colors, "face_labels": np.asarray(flabels, np.uint8) if want_face_labels else None,
            "owners": np.asarray(owners, np.int64).reshape(-1, 4), "t": tvals, "g": g, "pos": pos}


# ---- mesh properties used by the tests ------------------------------------------------------------------------------
def edge_counts(faces):
    """-> (undirected edge -> number of triangles, directed edge -> number of occurrences)."""
    und, dire = {}, {}
    for a, b, c in np.asarray(faces).tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            dire[(u, v)] = dire.get((u, v), 0) + 1
            k = (min(u, v), max(u, v))
            und[k] = und.get(k, 0) + 1
    return und, dire


def is_closed(faces):
    """Every undirected edge in exactly two triangles, once in each direction."""
    und, dire = edge_counts(faces)
    return bool(und) and all(n == 2 for n in und.values()) and all(n == 1 for n in dire.values())


def euler(vertices, faces):
    und, _ = edge_counts(faces)
    return len(vertices) - len(und) + len(faces)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def area(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)
