"""An independent restatement of the connected-components semantics of include/inr.h ("connected components"), for
tests/test_components_cpu.py and tests/test_components_extract.py: scipy.ndimage.label per label value, canonicalised to
min-linear-index roots, and the keep rule in numpy.  Also the test volumes both suites share.  Test infrastructure: the
product never imports this (nor scipy)."""
import numpy as np
from scipy import ndimage

EMPTY = 255


def structure(connectivity):
    return ndimage.generate_binary_structure(3, {6: 1, 26: 3}[connectivity])


def reference_roots(labels, connectivity):
    """labels uint8 [W, L, H] -> roots int32 [W, L, H]: smallest linear index of the voxel's component, -1 where empty."""
    labels = np.asarray(labels)
    roots = np.full(labels.size, -1, dtype=np.int64)
    flat = labels.reshape(-1)
    for value in np.unique(flat):
        if value == EMPTY:
            continue
        comp, n = ndimage.label(labels == value, structure=structure(connectivity))
        comp = comp.reshape(-1)
        ids, first = np.unique(comp, return_index=True)          # first occurrence in C order = smallest linear index
        lut = np.full(n + 1, -1, dtype=np.int64)
        lut[ids] = first
        sel = comp > 0
        roots[sel] = lut[comp[sel]]
    return roots.reshape(labels.shape).astype(np.int32)


def reference_filter(labels, confidence, K, connectivity=6, keep="largest", min_voxels=1, skip_background=True):
    labels = np.asarray(labels)
    roots = reference_roots(labels, connectivity)
    flat, r = labels.reshape(-1).astype(np.int64), roots.reshape(-1).astype(np.int64)
    first = min(1, K) if skip_background else 0
    out = flat.copy()
    n_components = np.zeros(K, np.int32)
    kept_voxels = np.zeros(K, np.int32)
    kept_root = np.full(K, -1, np.int32)
    for c in range(first, K):
        sel = flat == c
        comp_roots, sizes = np.unique(r[sel], return_counts=True)        # ascending roots
        n_components[c] = comp_roots.size
        ok = sizes >= min_voxels
        if keep == "largest" and ok.any():
            big = sizes[ok].max()
            winner = comp_roots[ok & (sizes == big)][0]                   # lowest root among the largest
            ok = comp_roots == winner
            kept_root[c] = winner
        kept_voxels[c] = sizes[ok].sum()
        drop = sel & ~np.isin(r, comp_roots[ok])
        out[drop] = EMPTY
    res = {"labels": out.astype(np.uint8).reshape(labels.shape), "roots": roots, "n_components": n_components,
           "kept_voxels": kept_voxels, "kept_root": kept_root, "confidence": None}
    if confidence is not None:
        res["confidence"] = np.where(res["labels"] == labels, np.asarray(confidence), np.float32(0)).astype(np.float32)
    return res


# ---- volumes ---------------------------------------------------------------------------------------------------------
def random_volume(shape, K, occupancy, seed):
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, K, size=shape).astype(np.uint8)
    vol[rng.random(shape) >= occupancy] = EMPTY
    return vol


def blob_volume(shape, K, seed, cell=5):
    """Random labels in cubic cells of `cell` voxels, a third of the cells empty: components that span many voxels and
    cross tile faces, unlike white noise."""
    rng = np.random.default_rng(seed)
    coarse = [-(-s // cell) for s in shape]
    c = rng.integers(0, K, size=coarse).astype(np.uint8)
    c[rng.random(coarse) < 0.33] = EMPTY
    vol = np.repeat(np.repeat(np.repeat(c, cell, 0), cell, 1), cell, 2)
    return np.ascontiguousarray(vol[:shape[0], :shape[1], :shape[2]])


def checkerboard(shape, label=1):
    w, l, h = np.indices(shape)
    return np.where((w + l + h) % 2 == 0, label, EMPTY).astype(np.uint8)


def serpentine(shape, label=1):
    """A one-voxel-wide path through the volume: full rows along h at even (w, l), joined end to end."""
    W, L, H = shape
    vol = np.full(shape, EMPTY, np.uint8)
    pos_h, l_dir = 0, 1
    for w in range(0, W, 2):
        ls = list(range(0, L, 2))
        if l_dir < 0:
            ls.reverse()
        for i, l in enumerate(ls):
            vol[w, l, :] = label
            pos_h = H - 1 - pos_h
            if i + 1 < len(ls):
                vol[w, l + l_dir, pos_h] = label
        if w + 2 < W:
            vol[w + 1, ls[-1], pos_h] = label
        l_dir = -l_dir
    return vol


def diagonal_sheets(shape, K=4):
    """Planes w + l + h = 4 n: under 26 every plane is one component (its in-plane steps are edge neighbours), under 6
    every voxel is alone."""
    w, l, h = np.indices(shape)
    s = w + l + h
    return np.where(s % 4 == 0, (s // 4) % K, EMPTY).astype(np.uint8)


def room_volume(res=160):
    """The 160^3 voxel-centre lattice of RoomScene() over [-1, 1]^3: label = instance_of_points (1..12), everything
    outside the boxes empty."""
    from instance_nerf_amd.scene import RoomScene
    room = RoomScene()
    ax = ((np.arange(res, dtype=np.float32) + np.float32(0.5)) / np.float32(res)) * np.float32(2.0) - np.float32(1.0)
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    ids = room.instance_of_points(pts)
    return np.where(ids > 0, ids, EMPTY).astype(np.uint8).reshape(res, res, res)


def voxel_stats(labels, K):
    """counts int64 [K], boxes int64 [K, 6] (inclusive voxel bounds, -1 when empty) in numpy."""
    counts = np.zeros(K, np.int64)
    boxes = np.full((K, 6), -1, np.int64)
    for c in range(K):
        idx = np.argwhere(labels == c)
        counts[c] = idx.shape[0]
        if idx.shape[0]:
            boxes[c, :3], boxes[c, 3:] = idx.min(0), idx.max(0)
    return counts, boxes


def add_floaters(clean, K, n_blobs=200, seed=0):
    """Seeded blobs of <= 64 voxels (cubes of side <= 4) of random ids 1..K-1 in empty space, each at Chebyshev distance
    >= 2 from the voxel box of its own id."""
    rng = np.random.default_rng(seed)
    _, boxes = voxel_stats(clean, K)
    noisy = clean.copy()
    shape = np.asarray(clean.shape)
    placed = 0
    while placed < n_blobs:
        k = int(rng.integers(1, K))
        side = rng.integers(1, 5, size=3)
        lo = rng.integers(0, shape - side + 1)
        hi = lo + side - 1
        if boxes[k, 0] >= 0 and np.all((hi >= boxes[k, :3] - 1) & (lo <= boxes[k, 3:] + 1)):
            continue                                                  # Chebyshev distance to its own id's box below 2
        region = noisy[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        region[clean[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] == EMPTY] = k
        placed += 1
    return noisy
