"""CPU side of the 3-D instance-mask extraction: the npz writer against the reader of the pipeline
(``masks.load_3d_masks``), the host form of the per-channel statistics, the named limits of the two new C exports
(in a child process, tests/instance_abi_child.py) and the loader's answer to a library older than its binding."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _volume(K=5, shape=(9, 7, 6), seed=0):
    """A label volume with empty voxels (255), every channel but K-1 present, channel 3 with exactly one voxel."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K - 1, size=shape).astype(np.uint8)
    lab[lab == 3] = 0
    lab[4, 2, 1] = 3
    lab[rng.random(shape) < 0.4] = 255
    lab[4, 2, 1] = 3
    conf = np.where(lab != 255, rng.uniform(0.2, 1.0, size=shape), 0.0).astype(np.float32)
    return lab, conf


def _result(lab, conf, K):
    from instance_nerf_amd.extract import volume_stats
    counts, boxes, csum = volume_stats(torch.from_numpy(lab), torch.from_numpy(conf), K)
    scores = torch.where(counts > 0, csum / counts.clamp_min(1).float(), torch.zeros_like(csum))
    return {"labels": torch.from_numpy(lab), "confidence": torch.from_numpy(conf), "res": np.asarray(lab.shape),
            "counts": counts, "boxes": boxes, "scores": scores}


def test_host_volume_stats():
    from instance_nerf_amd.extract import volume_stats
    K = 5
    lab, conf = _volume(K)
    counts, boxes, csum = (t.numpy() for t in volume_stats(torch.from_numpy(lab), torch.from_numpy(conf), K))
    for c in range(K):
        where = np.argwhere(lab == c)
        assert counts[c] == len(where)
        if len(where):
            assert list(boxes[c]) == list(where.min(0)) + list(where.max(0))
            assert abs(csum[c] - conf[lab == c].astype(np.float64).sum()) < 1e-5
        else:
            assert list(boxes[c]) == [-1] * 6 and csum[c] == 0
    assert counts[K - 1] == 0 and counts[3] == 1 and list(boxes[3]) == [4, 2, 1, 4, 2, 1]


def test_write_instance_masks_round_trips_through_load_3d_masks(tmp_path):
    from instance_nerf_amd.masks import load_3d_masks, write_instance_masks_npz
    K = 5
    lab, conf = _volume(K)
    res = _result(lab, conf, K)
    path = write_instance_masks_npz(str(tmp_path / "masks" / "scene.npz"), res)
    m = load_3d_masks(path)
    k = K - 1
    assert m["masks"].shape == (k,) + lab.shape and m["masks"].dtype == bool
    assert m["scores"].shape == (k,) and m["labels"].shape == (k,) and m["boxes"].shape == (k, 6)
    raw = np.load(path)
    assert raw["masks"].dtype == bool and raw["scores"].dtype == np.float32 and raw["boxes"].dtype == np.float32
    assert np.array_equal(m["labels"], np.ones(k, np.int64))
    for i in range(k):                                   # id order: mask i is instance id i + 1, channel 0 is never a mask
        assert np.array_equal(m["masks"][i], lab == i + 1), i
        where = np.argwhere(lab == i + 1)
        if len(where):
            # grid units: (min index, max index + 1)
            assert np.array_equal(m["boxes"][i], np.concatenate([where.min(0), where.max(0) + 1]).astype(np.float32))
            assert abs(m["scores"][i] - conf[lab == i + 1].mean()) < 1e-5
        else:                                            # channel K-1 is empty: empty mask, score 0, zero box
            assert not m["masks"][i].any() and m["scores"][i] == 0 and not m["boxes"][i].any()
    assert not m["masks"][K - 2].any()


def test_min_voxels_and_caller_labels(tmp_path):
    from instance_nerf_amd.masks import load_3d_masks, write_instance_masks_npz
    K = 5
    lab, conf = _volume(K)
    res = _result(lab, conf, K)
    cls = [7, 3, 9, 2]
    m = load_3d_masks(write_instance_masks_npz(str(tmp_path / "a.npz"), res, labels=cls, min_voxels=2))
    assert list(m["labels"]) == cls
    # id 3 has one voxel: below min_voxels it keeps its slot, empty
    assert not m["masks"][2].any() and m["scores"][2] == 0 and not m["boxes"][2].any()
    assert np.array_equal(m["masks"][0], lab == 1) and m["scores"][0] > 0
    with pytest.raises(ValueError):
        write_instance_masks_npz(str(tmp_path / "b.npz"), res, labels=[1, 2])


def test_named_limits_of_the_instance_mask_exports():
    out = abi_probe.run_abi_child("instance_abi_child.py", env=abi_probe.NO_GPU)
    del out["alive"]
    needles = {"K_0": "K", "K_65": "K", "confidence_misaligned": "misaligned", "packed_misaligned": "misaligned",
               "sigma_thresh_nan": "NaN", "null_desc": "null", "workspace_too_small": "workspace"}
    assert len(out) == 10
    for key, (rc, msg) in out.items():
        assert rc == EINVAL and needles[key.split(":")[1]] in msg, (key, rc, msg)


def _compiler():
    for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), "/opt/rocm/llvm/bin/clang"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.mark.parametrize("source", ["int inr_abi_version(void) { return 9; }\n", "int inr_something_else(void) { return 0; }\n"])
def test_a_stale_library_asks_for_a_rebuild(tmp_path, monkeypatch, source):
    """A library built before the newest exports (ABI 9, or no version at all) is refused with the rebuild message
    before any of the binding's symbols is looked up - not with an AttributeError for the first missing one."""
    from instance_nerf_amd import _lib
    cc = _compiler()
    assert cc, "no C compiler on this machine"
    src = tmp_path / "stale.c"
    src.write_text(source)
    so = tmp_path / "libinr_hip.so"
    subprocess.check_call([cc, "-shared", "-fPIC", "-o", str(so), str(src)])
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="rebuild with `python -m instance_nerf_amd.build --force`"):
        _lib.load()
