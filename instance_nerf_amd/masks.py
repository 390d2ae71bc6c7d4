"""Mask plumbing either side of the instance-field trainer.

f3  ``load_matched_masks``: reads what /root/reference/Mask2Former_sample/match_seg.py:140 writes -
    one ``<img>.npy`` per view, int32 [H, W], -1 = ignore / unmatched, 0 = background, > 0 = instance id
    (match_seg.py:65-91,131-138) - and turns it into per-ray labels for the CE loss (ignore_index -1).
f4  ``project_3d_masks``: counterpart of the reference's ``scripts/project_3d_masks.py`` (in the
    un-vendored submodule, /root/reference/README.md:63).  Input: NeRF-RCNN's discrete 3-D masks
    (/root/reference/nerf_rcnn/run_rcnn.py:652-666: ``masks [k, W, L, H]``); output:
    ``<proj_dir>/<img>_<inst>.png`` with foreground = channel 0 > 0 and instance ids starting at 1
    (match_seg.py:55-62,99-102: files ``*_0.png`` are skipped by the consumer).  A pixel belongs to
    instance i when the NeRF-weighted mask value along its ray, sum_s w_s * mask_i(x_s), exceeds
    ``thresh``: the K-channel compositing of the render path with mask_i as the extra channel.
f5  ``match_masks`` / ``project_and_match`` / ``match_seg_dir``: the matching step between the two, the reference's CPU
    script Mask2Former_sample/match_seg.py:94-150, on the device (csrc/match.hip): every 2-D segment takes the id of the
    projected 3-D mask it overlaps best.  ``project_and_match`` feeds the projector's sums to the matcher without leaving
    the GPU; ``match_seg_dir`` is the drop-in for the script on one scene directory.
"""
import contextlib
import ctypes
import json
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib, hdf5_lite, raymarching
from ._lib import check, ptr, ptr_or_null, stream_ptr
from .extract import eval_mode
from .maskbits import interleave32
from .nerf.utils import get_rays


# ---------------------------------------------------------------------------------------- f3
HDF5_DATASET = "cp_instance_id_segmaps"       # match_seg.py:142-143


def load_matched_masks(seg_dir, names=None):
    """-> dict {image name: int32 [H, W]} from ``<seg_dir>/<name>.npy`` (match_seg.py:140) and, for images that only
    have it, from the ``<name>.hdf5`` mirror the reference writes beside it (match_seg.py:142-143: dataset
    ``cp_instance_id_segmaps``; read without h5py by ``hdf5_lite``).  When both exist the ``.npy`` file is read."""
    listing = sorted(os.listdir(seg_dir))
    stems = {f[:-4]: f for f in listing if f.endswith(".npy")}
    for f in listing:
        if f.endswith(".hdf5") and f[:-5] not in stems:
            stems[f[:-5]] = f
    if names is not None:
        stems = {k: v for k, v in stems.items() if k in set(names)}
    out = {}
    for stem in sorted(stems):
        f = stems[stem]
        path = os.path.join(seg_dir, f)
        m = np.load(path) if f.endswith(".npy") else hdf5_lite.read_dataset(path, HDF5_DATASET)
        if m.ndim != 2:
            raise ValueError(f"{f}: expected an [H, W] instance-id map, got shape {m.shape}")
        out[stem] = m.astype(np.int32)
    return out


def labels_for_rays(mask, inds, num_instances):
    """mask int32 [H, W], inds int64 [N] flat pixel indices -> int64 [N] CE targets (-1 stays ignore;
    ids >= num_instances are ignored too, they have no logit)."""
    m = torch.as_tensor(mask).reshape(-1)
    inds = torch.as_tensor(inds)
    # the gather runs where the mask lives (a loader keeps its masks on the GPU: no host round trip per batch -
    # round-3 verdict: `inds.cpu()` here put a synchronisation into every training step)
    lab = m[inds.to(m.device)].long()
    return torch.where(lab >= num_instances, torch.full_like(lab, -1), lab)


# ---------------------------------------------------------------------------------------- png
def save_png_gray(path, img):
    """Minimal 8-bit grayscale PNG writer (no imaging library in the image); ``cv2.imread`` decodes it to
    three equal channels, so ``img[:, :, 0] > 0`` (match_seg.py:59) sees the mask."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    raw = b"".join(b"\x00" + img[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
           + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)


def read_png_gray(path):
    """Decoder for files written by ``save_png_gray`` (tests)."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = zlib.decompress(idat)
    return np.frombuffer(raw, np.uint8).reshape(h, w + 1)[:, 1:].copy()


# ---------------------------------------------------------------------------------------- f4
def load_3d_masks(path):
    """Reads ``masks/<scene>.npz`` as /root/reference/nerf_rcnn/run_rcnn.py:652-666 writes it: ``masks`` bool
    [k, W, L, H] (the output of the reference's ``paste_masks_in_image``, model/utils.py:704-782, thresholded at 0.5),
    ``scores`` float [k] sorted DESCENDING (top ``save_top_k`` detections, run_rcnn.py:658-664), ``labels`` int [k],
    ``boxes`` float [k, 6] (x1, y1, z1, x2, y2, z2 in grid units).  Instance id of mask i is i + 1
    (match_seg.py:99-102 skips ``*_0.png``).  -> dict of numpy arrays with those four keys."""
    z = np.load(path)
    missing = {"masks", "scores", "labels", "boxes"} - set(z.files)
    if missing:
        raise ValueError(f"{path}: missing keys {sorted(missing)} (expected the layout of run_rcnn.py:665-666)")
    masks, scores, labels, boxes = z["masks"], z["scores"], z["labels"], z["boxes"]
    k = masks.shape[0]
    if masks.ndim != 4 or scores.shape != (k,) or labels.shape != (k,) or boxes.shape != (k, 6):
        raise ValueError(f"{path}: masks {masks.shape}, scores {scores.shape}, labels {labels.shape}, boxes {boxes.shape} "
                         "are not [k,W,L,H], [k], [k], [k,6]")
    return {"masks": masks.astype(bool), "scores": scores.astype(np.float32), "labels": labels.astype(np.int64),
            "boxes": boxes.astype(np.float32)}


def pack_mask_words(masks, device):
    """bool [k, W, L, H] -> list of int32 tensors [W, L, H], one per 32 masks: bit i of word j = mask 32 j + i contains
    the voxel (the voxel words of maskbits.py, which ``inr_project_masks_patch`` reads).  Plain torch on ``device``."""
    return list(interleave32(torch.as_tensor(masks).to(device).bool()))


@torch.no_grad()
def soft_project(model, masks, bbox_min, bbox_max, rays_o, rays_d, T_thresh=1e-4, dt_gamma=0, max_steps=1024, packed=None):
    """NeRF-weighted projection of k voxel masks along rays.  masks [k, W, L, H] (boolean: non-zero = inside, as
    ``run_rcnn.py:652-666`` writes them); rays [N, 3].  -> (soft [N, k] = sum_s w_s * mask(x_s), weights_sum [N]).
    ``packed``: ``(k, pack_mask_words(masks, device))`` from an earlier call (a caller projecting many views packs once).

    March (patch-interleaved frame layout) -> field -> compositing with the per-sample weights kept -> ONE launch per
    32 masks that walks every ray's samples, looks the sample's voxel up in a 32-bit word per voxel and adds the weight
    to the accumulators of the masks whose bit is set (``inr_project_masks_patch``; round 4 - until then the mask values
    of all samples were gathered into a float [M, k] matrix, 3.8 GB for an 800x800 frame and 30 masks, and composited as
    k extra channels: same sums in the same order, bit-identical)."""
    dev = rays_o.device
    k, words = packed if packed is not None else (len(masks), pack_mask_words(masks, dev))
    if k == 0:
        raise ValueError("soft_project: no masks")
    W, L, H = (int(v) for v in words[0].shape)
    bbox = torch.tensor([float(v) for v in np.asarray(bbox_min, dtype=np.float32)] +
                        [float(v) for v in np.asarray(bbox_max, dtype=np.float32)], dtype=torch.float32)
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, model.aabb_infer, model.min_near)
    xyzs, dirs, deltas, rays = raymarching.march_rays_patch(rays_o, rays_d, model.bound, model.density_bitfield,
                                                           model.cascade, model.grid_size, nears, fars, dt_gamma, max_steps)
    sigmas, rgbs = model(xyzs, dirs)
    sigmas = sigmas * model.density_scale
    ws, _, _, wbuf = raymarching.composite_rays_patch(sigmas, rgbs, deltas, rays, T_thresh, return_weights=True)
    N, M = rays.shape[0], xyzs.shape[0]
    soft = torch.empty(N, k, dtype=torch.float32, device=dev)
    lib = _lib.load()
    for j, wj in enumerate(words):
        base = 32 * j
        check(lib.inr_project_masks_patch(ptr_or_null(xyzs, torch.float32, "xyzs"), ptr_or_null(wbuf, torch.float32, "weights"),
                                          ptr_or_null(rays, torch.int32, "rays"), N, M, ptr(wj, torch.int32, "mask_words"),
                                          W, L, H, _lib.host_ptr(bbox, torch.float32, "bbox"), k, base, min(32, k - base),
                                          ptr_or_null(soft), stream_ptr()), "project_masks_patch")
    return soft, ws


def _project_views(model, packed, bbox_min, bbox_max, poses, intrinsics, H, W):
    """The view loop of the projector: yields ``(v, rays, soft)`` per pose - the view's ``get_rays`` dict (patch order when
    H and W are multiples of 4) and the ``soft_project`` sums [H * W, k] of the ``packed`` masks over those rays.  The
    model is in eval mode while the generator is open and gets its mode back when it is exhausted or closed; a consumer
    holds it in ``contextlib.closing`` so that this also happens when the consumer raises."""
    with eval_mode(model):
        for v in range(poses.shape[0]):
            r = get_rays(poses[v:v + 1], intrinsics, H, W, patch=4 if (H % 4 == 0 and W % 4 == 0) else 0)
            yield v, r, soft_project(model, None, bbox_min, bbox_max, r["rays_o"][0], r["rays_d"][0], packed=packed)[0]


@torch.no_grad()
def project_3d_masks(model, masks, bbox_min, bbox_max, poses, intrinsics, H, W, proj_dir=None, img_names=None,
                     thresh=0.5, packed=None):
    """-> bool array [n_views, k, H, W]; when ``proj_dir`` is given also writes ``<img>_<inst>.png``
    (inst = mask index + 1) for every non-empty projection.  ``packed``: ``(k, words)`` with the words of
    ``pack_mask_words`` - or of ``detections.planes_to_voxel_words`` for masks that exist as bit planes - handed to
    ``soft_project`` in place of ``masks`` (which may then be None)."""
    dev = next(model.parameters()).device
    poses = torch.as_tensor(poses).to(dev).float()
    k = len(masks) if packed is None else int(packed[0])
    out = np.zeros((poses.shape[0], k, H, W), dtype=bool)
    if packed is None:
        packed = (k, pack_mask_words(masks, dev))      # one 32-bit word per voxel and 32 masks, built once for all views
    with contextlib.closing(_project_views(model, packed, bbox_min, bbox_max, poses, intrinsics, H, W)) as views:
        for v, r, soft in views:
            flat = torch.zeros(H * W, k, device=dev)
            flat[r["inds"][0]] = soft
            out[v] = (flat > thresh).t().reshape(k, H, W).cpu().numpy()
            if proj_dir is not None:
                os.makedirs(proj_dir, exist_ok=True)
                name = img_names[v] if img_names is not None else f"{v:04d}"
                for i in range(k):
                    if out[v, i].any():
                        save_png_gray(os.path.join(proj_dir, f"{name}_{i + 1}.png"), out[v, i].astype(np.uint8) * 255)
    return out


def instance_detections(result, labels=None, min_voxels=1, who="result"):
    """The detections an ``extract.extract_instances`` result stands for, on the host: instance id i + 1 is detection i,
    so k = K - 1 (channel 0, background / walls, is never one).  -> ``(keep bool [k], classes int64 [k], scores float32
    [k], boxes float32 [k, 6])``: ``keep`` = the instance has at least ``min_voxels`` voxels; ``classes`` = the caller's
    ``labels``, default all ones; boxes in grid units (min voxel index, max voxel index + 1); a dropped instance has score
    0 and a zero box.  The one statement of what ``write_instance_masks_npz`` writes and ``evaluate.evaluate_masks``
    scores."""
    def host(v):
        return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    counts = host(result["counts"])
    k = int(counts.shape[0]) - 1
    if k < 0:
        raise ValueError(f"{who} holds no instance channel")
    cls = np.ones(k, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64).reshape(-1)
    if cls.shape != (k,):
        raise ValueError(f"labels must hold one class per instance id 1..{k}, got shape {cls.shape}")
    keep = counts[1:] >= max(int(min_voxels), 1)
    scores = np.where(keep, host(result["scores"])[1:], 0.0).astype(np.float32)
    boxes = host(result["boxes"])[1:].astype(np.float32)
    boxes[:, 3:] += 1.0
    return keep, cls, scores, np.where(keep[:, None], boxes, np.float32(0.0))


def write_instance_masks_npz(path, result, labels=None, min_voxels=1):
    """Writes the 3-D segmentation of ``extract.extract_instances`` as ``masks/<scene>.npz`` in the layout
    ``load_3d_masks`` reads (run_rcnn.py:652-666): ``masks`` bool [k, W, L, H], ``scores`` float32 [k], ``labels`` int64
    [k] (``labels``: the caller's class per instance, default all ones), ``boxes`` float32 [k, 6] in grid units
    (x1, y1, z1, x2, y2, z2 = min voxel index, max voxel index + 1).

    Mask i is instance id i + 1 - the id rule of ``load_3d_masks`` - so k = K - 1: channel 0 (background / walls) is
    never a mask.  The masks stay in ID ORDER, not sorted by score as the NeRF-RCNN writer sorts its detections, so that
    projecting and matching them reproduces the field's own ids.  An instance with fewer than ``min_voxels`` voxels keeps
    its slot with an empty mask, score 0 and a zero box.  -> path."""
    lab = result["labels"]
    lab = lab.detach().cpu().numpy() if torch.is_tensor(lab) else np.asarray(lab)
    if lab.ndim != 3:
        raise ValueError("result['labels'] must be [W, L, H]")
    keep, cls, scores, boxes = instance_detections(result, labels, min_voxels)
    masks = np.zeros((len(keep),) + lab.shape, dtype=bool)
    for i in np.nonzero(keep)[0]:
        masks[i] = lab == i + 1
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, masks=masks, scores=scores, labels=cls, boxes=boxes)
    return path


# ---------------------------------------------------------------------------------------- f5
# The one fact of the reference's class tables (match_seg.py:17-48) that the matching rule uses: the COCO panoptic STUFF
# classes it maps to NYU40 id 40 = background.  Every other class, things included, keeps its segment.
BACKGROUND_STUFF = frozenset((
    "curtain", "door-stuff", "floor-wood", "stairs", "wall-brick", "wall-stone", "wall-tile", "wall-wood", "window-blind",
    "window-other", "ceiling-merged", "floor-other-merged", "building-other-merged", "wall-other-merged"))
MATCH_MAX_SEGMENTS, MATCH_MAX_CANDIDATES = 1023, 1024          # include/inr.h: limits of inr_match_count
_IDENTITY_RANK_MAX = 255        # segment ids up to here are their own ranks (Mask2Former's are 1..~100): no sort needed


def convert_segments(panoptic, segments_info, class_names=None):
    """Panoptic map + segment list of one image -> int32 [H, W] (match_seg.py:65-91): -1 unlabeled (0 in the input),
    0 background, otherwise the segment's own id.  A segment is background when it is not a thing and its class name is
    in ``BACKGROUND_STUFF``; ids that occur in the map but not in ``segments_info`` become 0.  Each segment dict carries
    ``id`` (> 0), ``isthing`` and either ``name`` or ``category_id``; the latter is looked up in ``class_names``, a dict
    with ``thing_classes`` / ``stuff_classes`` lists or the path of such a json (the user's coco_id_to_name.json).  Host
    code (numpy).  A negative value in ``panoptic`` raises ValueError."""
    seg = np.asarray(panoptic)
    if seg.ndim != 2:
        raise ValueError(f"panoptic must be [H, W], got shape {seg.shape}")
    if seg.size and seg.min() < 0:
        raise ValueError("panoptic holds a negative value (0 = unlabeled, > 0 = segment id)")
    seg = seg.astype(np.int32)
    if isinstance(class_names, (str, os.PathLike)):
        with open(class_names) as f:
            class_names = json.load(f)
    out = np.zeros_like(seg)
    out[seg == 0] = -1
    for s in segments_info:
        sid = int(s["id"])
        if sid <= 0:
            raise ValueError(f"segment id {sid} must be > 0")
        name = s.get("name")
        if name is None:
            if class_names is None:
                raise ValueError("a segment without 'name' needs class_names to look its category_id up")
            name = class_names["thing_classes" if s["isthing"] else "stuff_classes"][int(s["category_id"])]
        out[seg == sid] = 0 if (not s["isthing"] and name in BACKGROUND_STUFF) else sid
    return out


def candidate_order(instance_ids):
    """Positions of the candidates in the reference's order: the sorted file names ``<img>_<id>.png`` (match_seg.py:102),
    which is the string order of ``f"{id}.png"`` - 1 before 12 before 3.  The order decides ties between candidates."""
    ids = [int(i) for i in instance_ids]
    return sorted(range(len(ids)), key=lambda i: (f"{ids[i]}.png", i))


def select_projections(files, img_name):
    """The reference's file selection for one image (match_seg.py:99-102,114-117): ``*.png`` with an underscore whose part
    after the FIRST underscore is not ``0.png``, sorted by name, whose name STARTS with the image's name (so image
    ``0001`` also takes ``00010_9.png``).  -> (file names, instance ids)."""
    keep = sorted(f for f in files if f.endswith(".png") and "_" in f and f.split("_")[1] != "0.png")
    mine = [f for f in keep if f.startswith(img_name)]
    return mine, [int(f.split("_")[1].split(".")[0]) for f in mine]


def pack_mask_bits(proj, device=None):
    """bool [n, k, H, W] (numpy or tensor) -> int32 tensor [n, ceil(k / 32), H, W] on ``device`` (default: where ``proj``
    lives): bit j % 32 of word j // 32 = candidate j covers the pixel - the pixel words of maskbits.py, which
    ``inr_match_count`` reads.  ``match_masks`` accepts the result in place of ``proj``."""
    m = torch.as_tensor(proj)
    if m.dtype != torch.bool or m.ndim != 4:
        raise ValueError("proj must be bool [n, k, H, W]")
    m = m.to(device if device is not None else m.device)
    return interleave32(m.transpose(0, 1)).transpose(0, 1).contiguous()


def _rank_segments(seg):
    """int32 tensor [n, P] of converted maps -> (ranks int32 [n, P], S): -1 and 0 pass through, a segment id > 0 becomes
    its rank 1..S among the ids of ITS view (S = the largest count over the views).  Ids that are small already are their
    own ranks (a rank without pixels is never assigned).  One read-back (the largest id / S)."""
    n, P = seg.shape
    if seg.numel() == 0:
        return seg, 0
    if bool((seg < -1).any()):
        raise ValueError("seg_maps hold a value below -1")
    top = int(seg.max())
    if top <= _IDENTITY_RANK_MAX:
        return seg, max(top, 0)
    big = top + 1
    pos = seg > 0
    view = torch.arange(n, device=seg.device, dtype=torch.int64).view(n, 1).expand(n, P)[pos]
    uniq, inv = torch.unique(view * big + seg[pos].long(), return_inverse=True)           # sorted: by view, then by id
    starts = torch.searchsorted(uniq, torch.arange(n + 1, device=seg.device, dtype=torch.int64) * big)
    ranks = seg.clone()
    ranks[pos] = (inv - starts[view] + 1).to(torch.int32)
    return ranks, int((starts[1:] - starts[:-1]).max())


def _rank_segments_numpy(seg):
    """The same on the host for numpy input: np.unique per view."""
    if seg.size and seg.min() < -1:
        raise ValueError("seg_maps hold a value below -1")
    ranks, S = seg.copy(), 0
    for v in range(seg.shape[0]):
        pos = seg[v] > 0
        uniq, inv = np.unique(seg[v][pos], return_inverse=True)
        ranks[v][pos] = inv.reshape(-1) + 1
        S = max(S, int(uniq.size))
    return ranks, S


def match_ranked(ranks, words, S, k, instance_ids, iou_thresh=0.05):
    """The two device calls (include/inr.h, "2-D mask matching") on ranked maps: ranks int32 [n, P] (-1, 0 or a rank
    1..S), words int32 [n, ceil(k / 32), P] (``pack_mask_bits`` layout; ignored when k = 0), instance_ids int32 tensor [k]
    in candidate order.  -> int32 [n, P].  One read-back after both calls: a rank outside [-1, S] raises ValueError."""
    n, P = (int(v) for v in ranks.shape)
    dev = ranks.device
    lib = _lib.load()
    nw = (k + 31) // 32
    if k > 0 and tuple(words.shape) != (n, nw, P):
        raise ValueError(f"words must be [{n}, {nw}, {P}], got {tuple(words.shape)}")
    seg_area = torch.empty(n, S + 1, dtype=torch.int32, device=dev)
    mask_area = torch.empty(n, k, dtype=torch.int32, device=dev)
    inter = torch.empty(n, S + 1, k, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    assigned = torch.empty(n, S + 1, dtype=torch.int32, device=dev)
    out = torch.empty(n, P, dtype=torch.int32, device=dev)
    check(lib.inr_match_count(ptr(ranks, torch.int32, "ranks"), ptr(words, torch.int32, "words") if k > 0 else None,
                              n, P, S, k, ptr(seg_area), ptr_or_null(mask_area), ptr_or_null(inter), ptr(status), stream_ptr()),
          "match_count")
    thresh = ctypes.c_double(float(iou_thresh))
    check(lib.inr_match_assign(ptr(ranks), ptr(seg_area), ptr_or_null(mask_area), ptr_or_null(inter),
                               ptr_or_null(instance_ids, torch.int32, "instance_ids"), n, P, S, k,
                               ctypes.cast(ctypes.pointer(thresh), ctypes.c_void_p), ptr(assigned), ptr(out), stream_ptr()),
          "match_assign")
    if int(status) != 0:
        raise ValueError(f"match: a rank lies outside [-1, {S}]")
    return out


def _match_composable(ranks, proj, words, S, k, ids, iou_thresh):
    """The rule in plain torch on any device, one view at a time: integer one-hot counts (bincount), fp64 division, first
    argmax.  Same bits as the fused path; the CPU path and the timing twin."""
    n, P = ranks.shape
    dev = ranks.device
    out = ranks.clone()
    if bool(((ranks < -1) | (ranks > S)).any()):
        raise ValueError(f"match: a rank lies outside [-1, {S}]")
    cols = torch.arange(k, device=dev, dtype=torch.int64)
    for v in range(n):
        r = ranks[v].long()
        row = r.clamp(min=0)
        seg_area = torch.bincount(row, minlength=S + 1)
        if k > 0:
            if proj is not None:
                m = proj[v].reshape(k, P).t()
            else:
                m = ((words[v][cols // 32].long() >> (cols % 32).view(k, 1)) & 1).bool().t()
            inter = torch.bincount((row.view(P, 1) * k + cols.view(1, k))[m], minlength=(S + 1) * k).view(S + 1, k)
            mask_area = inter.sum(0)
            union = seg_area.view(S + 1, 1) + mask_area.view(1, k) - inter
            iou = torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=dev))
            best = iou.max(1).values
            first = torch.where(iou == best.view(S + 1, 1), cols.view(1, k), k).min(1).values
            assigned = torch.where((best > float(iou_thresh)) & (seg_area > 0), ids.long()[first], -1)
        else:
            assigned = torch.full((S + 1,), -1, dtype=torch.int64, device=dev)
        out[v] = torch.where(r > 0, assigned[row], r).to(torch.int32)
    return out


@torch.no_grad()
def match_masks(seg_maps, proj, instance_ids=None, iou_thresh=0.05, fused=True, ordered=False):
    """Gives every 2-D segment the id of the projected 3-D mask it overlaps best (match_seg.py:111-138).

    seg_maps: ``convert_segments`` maps, int [n, H, W] or [H, W], numpy or tensor (-1 unlabeled, 0 background, > 0 a
    segment id).  proj: bool [n, k, H, W] (or [k, H, W] with a 2-D map), numpy or tensor - or the int32 words of
    ``pack_mask_bits`` / ``project_and_match``, which must already be in candidate order.  instance_ids: the id of each
    candidate, default i + 1.  Per view, every segment id > 0 is scored against each candidate: IoU = |seg & m| /
    |seg | m| as the fp64 quotient of two integers; the FIRST candidate with the largest IoU gives its id if that IoU
    exceeds ``iou_thresh`` (in [0, 1]), else the segment becomes -1.  Pixels <= 0 pass through; with k = 0 every segment
    becomes -1.  Candidates are scored in the reference's order, the string order of ``f"{id}.png"`` (``candidate_order``;
    it decides ties), unless ``ordered`` says they already come in the order to use.

    -> int32 tensor [n, H, W] ([H, W] for a 2-D map) on the device of the inputs (a GPU tensor among them moves the rest
    there).  GPU tensors with ``fused=True`` run the HIP kernels of csrc/match.hip (at most 1023 segments per view and
    1024 candidates); ``fused=False`` or CPU inputs take the composable torch path, bit-identical."""
    if not 0.0 <= float(iou_thresh) <= 1.0:
        raise ValueError("iou_thresh must lie in [0, 1]")
    seg_np = None if torch.is_tensor(seg_maps) else np.asarray(seg_maps)
    seg = seg_maps if seg_np is None else torch.from_numpy(np.ascontiguousarray(seg_np).astype(np.int32))
    single = seg.ndim == 2
    if single:
        seg = seg[None]
        seg_np = None if seg_np is None else seg_np[None]
    if seg.ndim != 3:
        raise ValueError("seg_maps must be [n, H, W] or [H, W]")
    n, H, W = (int(v) for v in seg.shape)
    P = H * W
    pm = proj if torch.is_tensor(proj) else torch.from_numpy(np.ascontiguousarray(proj))
    if single and pm.ndim == 3:
        pm = pm[None]
    packed = pm.dtype == torch.int32
    if pm.ndim != 4 or pm.shape[0] != n or tuple(pm.shape[2:]) != (H, W) or not (packed or pm.dtype == torch.bool):
        raise ValueError(f"proj must be bool [{n}, k, {H}, {W}] or packed int32 words, got {pm.dtype} {tuple(pm.shape)}")
    if packed and instance_ids is None:
        raise ValueError("packed words need instance_ids (k is not known otherwise)")
    ids = list(range(1, pm.shape[1] + 1)) if instance_ids is None else [int(i) for i in np.asarray(
        instance_ids.cpu() if torch.is_tensor(instance_ids) else instance_ids).reshape(-1)]
    k = len(ids)
    if (packed and pm.shape[1] != (k + 31) // 32) or (not packed and pm.shape[1] != k):
        raise ValueError(f"{k} instance ids for proj of shape {tuple(pm.shape)}")
    order = list(range(k)) if ordered else candidate_order(ids)
    if order != list(range(k)):
        if packed:
            raise ValueError("packed words must be in candidate order (masks.candidate_order)")
        pm = pm[:, torch.as_tensor(order, device=pm.device)]
        ids = [ids[i] for i in order]
    dev = seg.device if seg.is_cuda else pm.device
    # ranks: on the host for numpy maps, on the device for tensors
    if seg_np is not None:
        ranks, S = _rank_segments_numpy(seg_np.reshape(n, P).astype(np.int32))
        ranks = torch.from_numpy(ranks).to(dev)
    else:
        ranks, S = _rank_segments(seg.to(dev).reshape(n, P).to(torch.int32).contiguous())
    pm = pm.to(dev)
    ids_t = torch.tensor(ids, dtype=torch.int32, device=dev)
    if fused and dev.type == "cuda":
        if S > MATCH_MAX_SEGMENTS or k > MATCH_MAX_CANDIDATES:
            raise ValueError(f"the fused match takes at most {MATCH_MAX_SEGMENTS} segments per view and "
                             f"{MATCH_MAX_CANDIDATES} candidates (got {S}, {k}); use fused=False")
        words = (pm if packed else pack_mask_bits(pm)).reshape(n, (k + 31) // 32, P).contiguous()
        out = match_ranked(ranks.contiguous(), words, S, k, ids_t, iou_thresh)
    else:
        out = _match_composable(ranks, None if packed else pm, pm.reshape(n, -1, P) if packed else None, S, k, ids_t, iou_thresh)
    out = out.view(n, H, W)
    return out[0] if single else out


@torch.no_grad()
def project_and_match(model, masks, bbox_min, bbox_max, poses, intrinsics, H, W, seg_maps, out_dir=None, img_names=None,
                      thresh=0.5, iou_thresh=0.05, packed=None):
    """``project_3d_masks`` and ``match_masks`` in one pass on the device: per view the projector's sums (``soft_project``)
    are thresholded straight into one bit per candidate (``inr_pack_mask_bits``), and once all views are packed the two
    match calls run batched over them.  masks [k, W, L, H] (instance id = index + 1), seg_maps ``convert_segments`` maps
    [n, H, W].  Nothing is copied to the host except, with ``out_dir``, the ``<name>.npy`` int32 files that
    ``load_matched_masks`` / ``NeRFDataset(mask_dir=...)`` read.  -> int32 tensor [n, H, W] on the model's device.
    ``packed``: ``(k, words)`` handed to ``soft_project`` in place of ``masks`` (which may then be None); the words must
    hold the masks in CANDIDATE ORDER (``candidate_order(range(1, k + 1))``, the ``order`` argument of
    ``detections.planes_to_voxel_words``)."""
    dev = next(model.parameters()).device
    poses = torch.as_tensor(poses).to(dev).float()
    n, k = int(poses.shape[0]), len(masks) if packed is None else int(packed[0])
    if k == 0:
        raise ValueError("project_and_match: no masks")
    order = candidate_order(range(1, k + 1))               # pack the candidates in the order the match scores them
    ids = [i + 1 for i in order]
    nw, P = (k + 31) // 32, H * W
    words = torch.empty(n, nw, H, W, dtype=torch.int32, device=dev)
    if packed is None:
        packed = (k, pack_mask_words(torch.as_tensor(masks)[torch.as_tensor(order)], dev))
    lib = _lib.load()
    with contextlib.closing(_project_views(model, packed, bbox_min, bbox_max, poses, intrinsics, H, W)) as views:
        for v, r, soft in views:
            inds = r["inds"][0].contiguous()
            check(lib.inr_pack_mask_bits(ptr(soft, torch.float32, "soft"), ptr(inds, torch.int64, "inds"), int(soft.shape[0]), k,
                                         float(thresh), P, ptr(words[v]), stream_ptr()), "pack_mask_bits")
    seg = seg_maps if torch.is_tensor(seg_maps) else torch.from_numpy(np.ascontiguousarray(seg_maps).astype(np.int32))
    out = match_masks(seg.to(dev), words, instance_ids=ids, iou_thresh=iou_thresh, fused=True, ordered=True)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        host = out.cpu().numpy()
        for v in range(n):
            np.save(os.path.join(out_dir, f"{img_names[v] if img_names is not None else f'{v:04d}'}.npy"), host[v])
    return out


def match_seg_dir(proj_dir, seg_dir, out_dir, class_names, iou_thresh=0.05, device=None):
    """Drop-in for the reference script on one scene directory (match_seg.py:94-140): for every ``<img>.npy`` panoptic map
    with its ``<img>.json`` segment list in ``seg_dir``, takes the projections ``<img>_<id>.png`` of ``proj_dir`` by the
    reference's rule (``select_projections``, the prefix quirk included; decoded by ``read_png_gray``, foreground > 0),
    matches, and writes ``<out_dir>/<img>.npy`` (int32).  ``class_names`` as in ``convert_segments``; ``device``: default
    the GPU when there is one (the HIP kernels), else the composable CPU path.  The ``.hdf5`` mirror and the colour
    preview the script writes beside each map are NOT written (``load_matched_masks`` reads the ``.npy``).
    -> list of the image names written."""
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if isinstance(class_names, (str, os.PathLike)):
        with open(class_names) as f:
            class_names = json.load(f)
    proj_files = os.listdir(proj_dir)
    os.makedirs(out_dir, exist_ok=True)
    done = []
    for f in sorted(x for x in os.listdir(seg_dir) if x.endswith(".npy")):
        with open(os.path.join(seg_dir, f[:-4] + ".json")) as j:
            info = json.load(j)
        seg = convert_segments(np.load(os.path.join(seg_dir, f)), info, class_names)
        name = f.split(".")[0]
        files, ids = select_projections(proj_files, name)
        pm = np.zeros((len(files),) + seg.shape, dtype=bool)
        for i, pf in enumerate(files):
            pm[i] = read_png_gray(os.path.join(proj_dir, pf)) > 0
        out = match_masks(torch.from_numpy(seg).to(device), torch.from_numpy(pm).to(device), instance_ids=ids,
                          iou_thresh=iou_thresh, ordered=True)
        np.save(os.path.join(out_dir, f), out.cpu().numpy())
        done.append(name)
    return done
