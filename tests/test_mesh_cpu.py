"""Triangle meshes, the part that needs no GPU: properties of the numpy restatement of the marching-tetrahedra extraction
(tests/mesh_reference.py, the yardstick of the kernels in tests/test_mesh_extract.py) on analytic and random fields, the
PLY writer / reader, the public surface (``Trainer.save_mesh``), and the argument validation of the three exports."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
import mesh_reference as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _cube_axes(n, lo=-1.0, hi=1.0):
    ax = f32(lo) + (np.arange(n, dtype=f32) + f32(0.5)) / f32(n) * f32(hi - lo)
    return [ax, ax, ax]


def _sphere(n, r=0.6):
    axes = _cube_axes(n)
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return (f32(r) - np.sqrt(X * X + Y * Y + Z * Z)).astype(f32), axes


def _torus(n, R=0.55, r=0.22):
    axes = _cube_axes(n)
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return (f32(r) - np.sqrt((np.sqrt(X * X + Y * Y) - f32(R)) ** 2 + Z * Z)).astype(f32), axes


def _assert_manifold(faces):
    und, dire = mr.edge_counts(faces)
    assert und and all(n == 2 for n in und.values())           # every undirected edge in exactly two triangles
    assert all(n == 1 for n in dire.values())                  # once in each direction
    assert len(dire) == 2 * len(und)


@pytest.mark.parametrize("shape,chi", [("sphere", 2), ("torus", 0)])
@pytest.mark.parametrize("cap", [True, False])
def test_closed_oriented_surfaces_of_analytic_fields(shape, chi, cap):
    field, axes = (_sphere if shape == "sphere" else _torus)(28)
    m = mr.marching_tetrahedra(field, 0.0, 0.5, axes, cap=cap)
    _assert_manifold(m["faces"])
    assert mr.euler(m["vertices"], m["faces"]) == chi
    assert mr.signed_volume(m["vertices"], m["faces"]) > 0
    assert m["faces"].min() == 0 and m["faces"].max() == len(m["vertices"]) - 1
    assert len(np.unique(m["faces"])) == len(m["vertices"])   # every vertex is used


def test_sphere_volume_and_area_converge():
    r = 0.6
    vol_err, area_err = [], []
    for n in (16, 32, 64):
        field, axes = _sphere(n, r)
        m = mr.marching_tetrahedra(field, 0.0, 0.5, axes, cap=False)
        vol_err.append(abs(mr.signed_volume(m["vertices"], m["faces"]) / (4.0 / 3.0 * np.pi * r ** 3) - 1.0))
        area_err.append(abs(mr.area(m["vertices"], m["faces"]) / (4.0 * np.pi * r ** 2) - 1.0))
    print("sphere relative errors at 16, 32, 64: volume", vol_err, "area", area_err)
    assert vol_err[0] > vol_err[1] > vol_err[2] and area_err[0] > area_err[1] > area_err[2]
    # the restatement gives 1.36e-3 (volume) and 6.98e-4 (area) at 64 (an inscribed polyhedron: second order in the cell
    # size, 2.1e-2 -> 5.4e-3 -> 1.4e-3); the bounds are those figures with a 2x margin
    assert vol_err[2] < 2.8e-3 and area_err[2] < 1.4e-3


def test_vertices_lie_on_their_edges_at_the_iso_value():
    field, axes = _sphere(24)
    rng = np.random.default_rng(1)
    field = (field + rng.normal(scale=0.02, size=field.shape)).astype(f32)
    iso, clamp = f32(0.05), f32(0.1)
    m = mr.marching_tetrahedra(field, iso, clamp, axes, cap=True)
    g, pos = m["g"], m["pos"]
    assert len(m["vertices"]) > 500
    for (ew, el, eh, c), t, x in zip(m["owners"].tolist(), m["t"], m["vertices"]):
        dw, dl, dh = mr.corner(c)
        assert 0.0 <= t <= 1.0
        a, b = g[ew, el, eh], g[ew + dw, el + dl, eh + dh]
        assert (a >= iso) != (b >= iso)
        # a + t (b - a) = iso up to the roundings of t and of this expression: a few ulps of the clamp band
        assert abs(float(a) + float(t) * (float(b) - float(a)) - float(iso)) <= 4 * np.finfo(f32).eps * float(clamp + abs(iso))
        for k, (e, d) in enumerate(((ew, dw), (el, dl), (eh, dh))):
            lo, hi = float(pos[k][e]), float(pos[k][e + d])
            assert min(lo, hi) <= float(x[k]) <= max(lo, hi)
            assert abs(float(x[k]) - (lo + float(t) * (hi - lo))) <= 2 * np.finfo(f32).eps * max(abs(lo), abs(hi))


@pytest.mark.parametrize("seed", range(20))
def test_any_field_gives_a_closed_surface(seed):
    rng = np.random.default_rng(seed)
    field = rng.normal(size=(12, 12, 12)).astype(f32)
    axes = _cube_axes(12)
    m = mr.marching_tetrahedra(field, 0.0, 1.0, axes, cap=True)
    assert len(m["faces"]) > 3000
    _assert_manifold(m["faces"])                                # no case left out
    assert mr.signed_volume(m["vertices"], m["faces"]) > 0
    # without the cap the only open edges join two vertices owned by border cells' edges on the lattice's boundary
    o = mr.marching_tetrahedra(field, 0.0, 1.0, axes, cap=False)
    und, _ = mr.edge_counts(o["faces"])
    assert all(n in (1, 2) for n in und.values())
    open_edges = [e for e, n in und.items() if n == 1]
    assert open_edges
    own = o["owners"]
    for u, v in open_edges:
        for vid in (u, v):
            p = own[vid, :3]
            q = p + np.asarray(mr.corner(int(own[vid, 3])))
            # both ends of the owning lattice edge lie on one boundary face of the lattice
            assert any((p[k] == q[k]) and p[k] in (0, 11) for k in range(3)), (p, q)


def test_select_gives_closed_instance_meshes_and_labelled_faces():
    n = 20
    axes = _cube_axes(n)
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    d1 = np.sqrt((X + 0.3) ** 2 + Y * Y + Z * Z)
    d2 = np.sqrt((X - 0.3) ** 2 + Y * Y + Z * Z)
    field = (f32(0.45) - np.minimum(d1, d2)).astype(f32)        # two overlapping balls: one blob, two labels
    labels = np.where(field >= 0, np.where(d1 <= d2, 1, 2), 255).astype(np.uint8)
    cell = 2.0 / n
    for k, d in ((1, d1), (2, d2)):
        m = mr.marching_tetrahedra(field, 0.0, 0.5, axes, labels=labels, select=k, cap=True)
        _assert_manifold(m["faces"])
        assert mr.signed_volume(m["vertices"], m["faces"]) > 0
    scene = mr.marching_tetrahedra(field, 0.0, 0.5, axes, labels=labels, cap=True)
    _assert_manifold(scene["faces"])
    assert set(np.unique(scene["face_labels"]).tolist()) == {1, 2}
    v = scene["vertices"].astype(np.float64)
    for k in (1, 2):
        blob = np.stack([X[labels == k], Y[labels == k], Z[labels == k]], 1).astype(np.float64)
        fv = v[scene["faces"][scene["face_labels"] == k]].reshape(-1, 3)
        dist = np.sqrt(((fv[:, None, :] - blob[None, :, :]) ** 2).sum(-1)).min(1)
        assert dist.max() <= cell * np.sqrt(3.0) + 1e-6          # within one cell (its diagonal) of blob k


def test_nan_and_infinite_values_give_no_nan_vertex():
    rng = np.random.default_rng(5)
    field = rng.normal(size=(10, 11, 9)).astype(f32)
    flat = field.reshape(-1)
    flat[rng.choice(flat.size, 90, replace=False)] = np.tile(np.asarray([np.nan, -np.inf, np.inf], f32), 30)
    axes = [np.arange(10, dtype=f32), np.arange(11, dtype=f32), np.arange(9, dtype=f32)]
    m = mr.marching_tetrahedra(field, 0.0, 1.0, axes, cap=True)
    assert np.isfinite(m["vertices"]).all() and np.isfinite(m["t"]).all()
    _assert_manifold(m["faces"])
    inside = m["g"] >= 0
    assert not inside[1:-1, 1:-1, 1:-1][np.isnan(field)].any()             # NaN is outside


def test_ply_round_trip(tmp_path):
    from instance_nerf_amd import mesh_io
    field, axes = _sphere(12)
    m = mr.marching_tetrahedra(field, 0.0, 0.5, axes)
    V, F = len(m["vertices"]), len(m["faces"])
    rng = np.random.default_rng(0)
    colors = rng.integers(0, 256, size=(V, 3)).astype(np.uint8)
    labels = rng.integers(0, 255, size=F).astype(np.uint8)
    for c, l in ((None, None), (colors, None), (None, labels), (colors, labels)):
        path = mesh_io.write_ply(str(tmp_path / "m.ply"), m["vertices"], m["faces"], c, l)
        back = mesh_io.read_ply(path)
        assert back["vertices"].tobytes() == m["vertices"].tobytes() and back["vertices"].dtype == np.float32
        assert np.array_equal(back["faces"], m["faces"]) and back["faces"].dtype == np.int32
        assert (back["colors"] is None) == (c is None) and (back["face_labels"] is None) == (l is None)
        if c is not None:
            assert np.array_equal(back["colors"], c)
        if l is not None:
            assert np.array_equal(back["face_labels"], l)
        # the header, by the PLY grammar
        with open(path, "rb") as fh:
            fmt, elements = mesh_io.read_ply_header(fh)
            body = fh.read()
        assert fmt == ("binary_little_endian", "1.0")
        assert [(e[0], e[1]) for e in elements] == [("vertex", V), ("face", F)]
        vprops = [("scalar", "float", a) for a in "xyz"] + ([("scalar", "uchar", a) for a in ("red", "green", "blue")] if c is not None else [])
        fprops = [("list", "uchar", "int", "vertex_indices")] + ([("scalar", "uchar", "label")] if l is not None else [])
        assert elements[0][2] == vprops and elements[1][2] == fprops
        assert len(body) == V * (12 + (3 if c is not None else 0)) + F * (13 + (1 if l is not None else 0))
    # float colours are rounded to 0..255; an empty mesh is a valid file
    back = mesh_io.read_ply(mesh_io.write_ply(str(tmp_path / "f.ply"), m["vertices"], m["faces"], colors.astype(f32) / f32(255)))
    assert np.array_equal(back["colors"], colors)
    empty = mesh_io.read_ply(mesh_io.write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3), f32), np.zeros((0, 3), np.int32)))
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3)
    with pytest.raises(ValueError, match="does not exist"):
        mesh_io.write_ply(str(tmp_path / "bad.ply"), m["vertices"][:3], m["faces"])


def test_trainer_has_upstreams_save_mesh():
    from instance_nerf_amd.nerf.utils import Trainer
    assert hasattr(Trainer, "save_mesh") and hasattr(Trainer, "save_instance_meshes")
    sig = inspect.signature(Trainer.save_mesh)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("save_path", None), ("resolution", 256), ("threshold", 10)]
    sig = inspect.signature(Trainer.save_instance_meshes)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("save_path", None), ("resolution", 256), ("threshold", 10),
                                                                               ("min_faces", 1)]


def test_extract_mesh_rejects_cpu_models():
    import torch
    from instance_nerf_amd import extract

    class Tiny(torch.nn.Module):
        bound, density_scale, num_instances = 1.0, 1.0, 0

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract.extract_mesh(Tiny(), resolution=8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        extract.mesh_from_lattice(torch.zeros(4, 4, 4), 0.0, [torch.zeros(4)] * 3, (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("mesh_abi_child.py", env=abi_probe.NO_GPU)


@pytest.mark.parametrize("case,needle", [
    ("clamp_zero", "clamp"), ("clamp_negative", "clamp"), ("clamp_nan", "clamp"), ("clamp_inf", "clamp"),
    ("select_255", "select"), ("select_without_labels", "select"), ("workspace_too_small", "workspace"),
    ("size_overflows_int32", "int32"), ("cap_2", "cap"), ("stride_0", "stride")])
@pytest.mark.parametrize("name", ["inr_mesh_count", "inr_mesh_emit"])
def test_named_limits_of_the_mesh_exports(abi, name, case, needle):
    rc, msg = abi[f"{name}:{case}"]
    assert rc == -1 and needle in msg, (name, case, rc, msg)


@pytest.mark.parametrize("key,needle", [
    ("inr_mesh_count:counts_misaligned", "misaligned"), ("inr_mesh_emit:vertices_misaligned", "misaligned"),
    ("inr_mesh_emit:faces_misaligned", "misaligned"), ("inr_mesh_emit:colors_without_rgb", "rgb"),
    ("inr_mesh_emit:face_labels_without_labels", "labels"), ("inr_mesh_emit:negative_V", "V"),
    ("inr_mesh_emit:V_too_large", "V"), ("inr_mesh_workspace_bytes:negative", "size"),
    ("inr_mesh_workspace_bytes:zero", "size"), ("inr_mesh_workspace_bytes:cap_2", "cap"),
    ("inr_mesh_workspace_bytes:size_overflows_int32", "int32")])
def test_named_limits_of_single_exports(abi, key, needle):
    rc, msg = abi[key]
    assert rc == -1 and needle in msg, (key, rc, msg)


def test_workspace_size_of_the_default_resolution(abi):
    """256^3 capped: 258^3 points, 4 B offset + 1 B mask each and 8 B per 256-point workgroup."""
    n = 258 ** 3
    nb = (n + 255) // 256
    assert abi["inr_mesh_workspace_bytes:ok"][0] == (5 * n + 8 * nb + 255) // 256 * 256
