"""rgb-sigma grid extraction: the step after the render path that feeds NeRF-RCNN.

The reference's extractor lives in a third repository (a fork of instant-ngp,
/root/reference/README.md:89) and is not available; what IS in the reference tree is the consumer:
``SegmentationDataset.load_feature`` (/root/reference/nerf_rcnn/datasets.py:766-792) and
``ngp_density_to_alpha`` (datasets.py:865-866), plus the metadata keys read by
/root/reference/nerf_rcnn/scripts/proposals2ngp.py:24-29.  This module writes exactly what they read:

* ``rgbsigma`` float32 ``[W, L, H, 4]`` (or flat ``[H*L*W, 4]``, or uint8), channels (r, g, b, d) with
  d the RAW pre-activation density (the consumer applies ``1 - exp(-exp(d)/100)``), i.e. log(sigma);
* ``resolution`` int ``[3] = (W, L, H)``, longest side <= 160 (train_rpn.sh:11, poolers.py:40);
* ``bbox_min``, ``bbox_max``, ``scale``, ``offset``, ``from_mitsuba``.

Queries go through ``NeRFNetwork.forward_dirs`` (one fused HIP launch per chunk: gather + sigma net once per
point, colour net once per view direction; ``density`` / ``color`` for non-standard architectures).  Choices made here
because the reference extractor is unseen: voxel-CENTRE positions; rgb = mean over 4 fixed view
directions (the tetrahedron (1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1), normalised).
"""
import numpy as np
import torch

VIEW_DIRS = np.asarray([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32) / np.sqrt(3.0)


def grid_resolution(bbox_min, bbox_max, max_side=160):
    """Per-axis resolution with the longest side = max_side and (approximately) cubic voxels."""
    ext = np.asarray(bbox_max, dtype=np.float64) - np.asarray(bbox_min, dtype=np.float64)
    res = np.maximum(np.round(ext / ext.max() * max_side), 1).astype(np.int64)
    return res


def lattice_axes(bbox_min, bbox_max, res, device):
    """The three coordinate axes of the voxel-centre lattice: float32 [W], [L], [H]."""
    # formed on the host in float32 (IEEE division, one rounding per operation) and uploaded in ONE copy: fifteen tiny
    # device launches otherwise, ~0.1 ms of a 1.2 ms extraction
    f32 = np.float32
    host, sizes = [], []
    for a in range(3):
        n = int(res[a])
        t = (np.arange(n, dtype=f32) + f32(0.5)) / f32(n)
        host.append(f32(float(bbox_min[a])) + t * f32(float(bbox_max[a]) - float(bbox_min[a])))
        sizes.append(n)
    flat = torch.from_numpy(np.concatenate(host).astype(f32)).to(device)
    return list(torch.split(flat, sizes))


_AXES_CACHE = {}


def _cached_axes(bbox_min, bbox_max, res, device):
    """``lattice_axes`` kept per (box, resolution, device): a scene is extracted with one lattice, and the upload of a
    fresh one is a synchronous host-to-device copy in front of every extraction."""
    key = (tuple(float(v) for v in bbox_min), tuple(float(v) for v in bbox_max), tuple(int(v) for v in res), str(device))
    hit = _AXES_CACHE.get(key)
    if hit is None:
        if len(_AXES_CACHE) > 16:
            _AXES_CACHE.clear()
        hit = _AXES_CACHE[key] = lattice_axes(bbox_min, bbox_max, res, device)
    return hit


def lattice(bbox_min, bbox_max, res, device):
    """Voxel-centre positions, float32 [W*L*H, 3], index order (w, l, h) with h fastest."""
    axes = lattice_axes(bbox_min, bbox_max, res, device)
    ww, ll, hh = torch.meshgrid(*axes, indexing="ij")
    return torch.stack([ww.reshape(-1), ll.reshape(-1), hh.reshape(-1)], -1)


@torch.no_grad()
def extract_rgbsigma(model, bbox_min=None, bbox_max=None, max_side=160, res=None, chunk=1 << 22):
    """-> (rgbsigma float32 [W,L,H,4] on the model's device, res int64[3]).  Channel 3 = log(sigma)."""
    dev = next(model.parameters()).device
    b = float(model.bound)
    bbox_min = np.asarray([-b, -b, -b] if bbox_min is None else bbox_min, dtype=np.float32)
    bbox_max = np.asarray([b, b, b] if bbox_max is None else bbox_max, dtype=np.float32)
    res = grid_resolution(bbox_min, bbox_max, max_side) if res is None else np.asarray(res, dtype=np.int64)
    cached = getattr(model, "_view_dirs_dev", None)     # the four fixed directions and their SH rows, uploaded once
    if cached is None or cached[0].device != dev:
        d = torch.from_numpy(VIEW_DIRS).to(dev)
        cached = model._view_dirs_dev = (d, model.encoder_dir(d).contiguous() if hasattr(model, "encoder_dir") else None)
    dirs = cached[0]
    if hasattr(model, "forward_lattice"):
        # one launch for the whole lattice, from its three coordinate axes (no [W*L*H, 3] point tensor), walked in
        # runs along W: 160^3 in 1.4 ms instead of 2.8 (profiles/r04_NOTES.txt 6)
        was_training = model.training
        model.eval()
        sh = cached[1]
        # the density logit's lower clamp (log 1e-30, as on the point-list path) is applied inside the launch
        fused = model.forward_lattice(_cached_axes(bbox_min, bbox_max, res, dev), dirs, logit_min=float(np.log(1e-30)), sh=sh)
        model.train(was_training)
        if fused is not None:
            return fused, res
    pts = lattice(bbox_min, bbox_max, res, dev)
    out = torch.empty(pts.shape[0], 4, dtype=torch.float32, device=dev)
    was_training = model.training
    model.eval()
    for s in range(0, pts.shape[0], chunk):
        x = pts[s:s + chunk].clamp(-b, b)
        fused = model.forward_dirs(x, dirs) if hasattr(model, "forward_dirs") else None
        if fused is not None:                  # one launch: gather + sigma net once, colour net per direction
            out[s:s + chunk] = fused
            out[s:s + chunk, 3].clamp_(min=float(np.log(1e-30)))
            continue
        den = model.density(x)
        rgb = torch.zeros(x.shape[0], 3, dtype=torch.float32, device=dev)
        for v in range(dirs.shape[0]):
            rgb += model.color(x, dirs[v].expand(x.shape[0], 3).contiguous(), geo_feat=den["geo_feat"])
        out[s:s + chunk, :3] = rgb / dirs.shape[0]
        out[s:s + chunk, 3] = torch.log(den["sigma"].clamp_min(1e-30))
    model.train(was_training)
    return out.view(int(res[0]), int(res[1]), int(res[2]), 4), res


def write_features_npz(path, rgbsigma, bbox_min, bbox_max, scale=1.0, offset=(0.0, 0.0, 0.0), from_mitsuba=False,
                       flat=False, as_uint8=False):
    """Writes ``features/<scene>.npz`` in the layout /root/reference/nerf_rcnn/datasets.py:766-792 reads.

    rgbsigma: array-like [W, L, H, 4].  flat=True stores [H*L*W, 4] such that the consumer's
    ``reshape(res[2], res[1], res[0], -1)`` + ``transpose(3, 2, 1, 0)`` (transpose_yz=False, the shipped
    setting, run_rcnn.py:250) recovers [C, W, L, H].  as_uint8 quantises every channel from [0, 1] to
    [0, 255]: the consumer divides by 255 but its density normalisation runs on the raw integer array
    first, so uint8 files are only meaningful with channel 3 already holding alpha in [0, 1] and the
    consumer's ``normalize_density=False``.
    """
    g = np.asarray(rgbsigma.detach().cpu() if torch.is_tensor(rgbsigma) else rgbsigma)
    if g.ndim != 4 or g.shape[-1] != 4:
        raise ValueError("rgbsigma must be [W, L, H, 4]")
    W, L, H = g.shape[:3]
    if as_uint8:
        g = np.clip(np.round(g * 255.0), 0, 255).astype(np.uint8)
    else:
        g = g.astype(np.float32)
    if flat:
        g = np.ascontiguousarray(np.transpose(g, (2, 1, 0, 3))).reshape(H * L * W, 4)
    np.savez_compressed(path, rgbsigma=g, resolution=np.asarray([W, L, H], dtype=np.int64),
                        bbox_min=np.asarray(bbox_min, dtype=np.float32), bbox_max=np.asarray(bbox_max, dtype=np.float32),
                        scale=np.float32(scale), offset=np.asarray(offset, dtype=np.float32),
                        from_mitsuba=np.bool_(from_mitsuba))
    return path


# ---- 3-D instance masks of a trained instance field ---------------------------------------------------------------
LABEL_EMPTY = 255        # label of an unoccupied voxel


def volume_stats(labels, confidence, K):
    """Per-channel statistics of a label volume (uint8 [W, L, H], ``LABEL_EMPTY`` = unoccupied): -> (counts int64 [K],
    boxes int64 [K, 6] = inclusive voxel-index bounds (min iw, il, ih, max iw, il, ih; -1 for an empty channel),
    conf_sum float32 [K]), on the volume's device.  On the GPU (K <= 64) one bit-reproducible HIP call
    (``inr_instance_volume_stats``: fixed per-workgroup slots, fixed-order final pass); otherwise numpy on the host
    (float64 sums)."""
    W, L, H = (int(v) for v in labels.shape)
    if labels.is_cuda and 1 <= K <= 64:
        from . import _lib
        lib = _lib.load()
        dev = labels.device
        ws = torch.empty(_lib.INSTANCE_STATS_WORKSPACE_BYTES // 4, dtype=torch.int32, device=dev)
        counts = torch.empty(K, dtype=torch.int32, device=dev)
        boxes = torch.empty(K, 6, dtype=torch.int32, device=dev)
        csum = torch.empty(K, dtype=torch.float32, device=dev)
        _lib.check(lib.inr_instance_volume_stats(_lib.ptr(labels.contiguous(), torch.uint8, "labels"),
                                                 _lib.ptr(confidence.contiguous(), torch.float32, "confidence"), W, L, H, K,
                                                 _lib.ptr(ws), _lib.INSTANCE_STATS_WORKSPACE_BYTES, _lib.ptr(counts),
                                                 _lib.ptr(boxes), _lib.ptr(csum), _lib.stream_ptr()), "instance_volume_stats")
        return counts.long(), boxes.long(), csum
    lab = labels.detach().cpu().numpy().reshape(-1).astype(np.int64)
    cf = confidence.detach().cpu().numpy().reshape(-1).astype(np.float64)
    live = lab < K
    idx = np.nonzero(live)[0]
    ch = lab[idx]
    counts = np.bincount(ch, minlength=K)[:K]
    csum = np.bincount(ch, weights=cf[idx], minlength=K)[:K].astype(np.float32)
    coords = np.stack(np.unravel_index(idx, (W, L, H)), 1)
    boxes = np.full((K, 6), -1, dtype=np.int64)
    big = np.iinfo(np.int64).max
    lo = np.full((K, 3), big, dtype=np.int64)
    hi = np.full((K, 3), -1, dtype=np.int64)
    np.minimum.at(lo, ch, coords)
    np.maximum.at(hi, ch, coords)
    has = counts > 0
    boxes[has, :3], boxes[has, 3:] = lo[has], hi[has]
    dev = labels.device
    return (torch.from_numpy(counts.astype(np.int64)).to(dev), torch.from_numpy(boxes).to(dev),
            torch.from_numpy(csum).to(dev))


def _instances_composable(model, bbox_min, bbox_max, res, sigma_thresh, chunk):
    """The composable form of the fused launch, with its semantics: voxel centres clamped to [-bound, bound], occupied
    when density_scale * sigma >= sigma_thresh, arg-max over the K real channels (torch.argmax: lowest on ties), max-softmax
    confidence, ``LABEL_EMPTY`` / 0 elsewhere.  ``density()`` and ``instance()`` per chunk of points."""
    dev = next(model.parameters()).device
    b = float(model.bound)
    pts = lattice(bbox_min, bbox_max, res, dev)
    labels = torch.full((pts.shape[0],), LABEL_EMPTY, dtype=torch.uint8, device=dev)
    conf = torch.zeros(pts.shape[0], dtype=torch.float32, device=dev)
    for s in range(0, pts.shape[0], chunk):
        x = pts[s:s + chunk].clamp(-b, b).contiguous()
        occ = model.density(x)["sigma"] * model.density_scale >= sigma_thresh
        if not bool(occ.any()):
            continue
        logits = model.instance(x)[:, :model.num_instances].float()       # the K real channels only
        mx, arg = logits.amax(1), torch.argmax(logits, 1)
        c = 1.0 / torch.exp(logits - mx[:, None]).sum(1)
        labels[s:s + chunk] = torch.where(occ, arg.to(torch.uint8), torch.full_like(labels[s:s + chunk], LABEL_EMPTY))
        conf[s:s + chunk] = torch.where(occ, c, torch.zeros_like(c))
    W, L, H = (int(v) for v in res)
    return labels.view(W, L, H), conf.view(W, L, H)


@torch.no_grad()
def extract_instances(model, bbox_min=None, bbox_max=None, max_side=160, res=None, sigma_thresh=None, fused=True,
                      chunk=1 << 20):
    """The trained instance field as a 3-D segmentation on the lattice of ``extract_rgbsigma`` (voxel centres, longest
    side ``max_side``, default box [-bound, bound]^3).  A voxel is occupied when ``density_scale * sigma`` (the sigma the
    renderer composites) is >= ``sigma_thresh`` (default ``model.density_thresh``).  -> dict:

    * ``labels`` uint8 [W, L, H]: the arg-max instance channel 0..K-1 of an occupied voxel (channel 0 = background /
      walls, lowest channel on ties as ``torch.argmax``), ``LABEL_EMPTY`` (255) elsewhere;
    * ``confidence`` float32 [W, L, H]: its softmax probability, 0 where unoccupied;
    * ``res`` int64 [3]; ``counts`` int64 [K] voxels per channel; ``boxes`` int64 [K, 6] inclusive voxel-index bounds
      (min iw, il, ih, max iw, il, ih; -1 for an empty channel); ``scores`` float32 [K] mean confidence of the channel's
      voxels (0 when empty).

    Tensors stay on the model's device.  The fused path is one HIP launch for the labels (``NeRFNetwork.instance_lattice``)
    and one for the statistics; two calls give identical bits.  ``fused=False`` (and shapes the fused kernels do not
    cover) runs the composable path - ``density()`` + ``instance()`` over chunks of points - with the same semantics."""
    if not getattr(model, "num_instances", 0):
        raise ValueError("extract_instances: the model has no instance head (num_instances = 0)")
    dev = next(model.parameters()).device
    b = float(model.bound)
    bbox_min = np.asarray([-b, -b, -b] if bbox_min is None else bbox_min, dtype=np.float32)
    bbox_max = np.asarray([b, b, b] if bbox_max is None else bbox_max, dtype=np.float32)
    res = grid_resolution(bbox_min, bbox_max, max_side) if res is None else np.asarray(res, dtype=np.int64)
    thresh = float(model.density_thresh if sigma_thresh is None else sigma_thresh)
    K = int(model.num_instances)
    if K >= LABEL_EMPTY:
        raise ValueError(f"extract_instances: {K} instance channels do not fit the uint8 labels (at most {LABEL_EMPTY - 1})")
    was_training = model.training
    model.eval()
    try:
        out = None
        if fused and hasattr(model, "instance_lattice"):
            out = model.instance_lattice(_cached_axes(bbox_min, bbox_max, res, dev), thresh)
        if out is None:
            out = _instances_composable(model, bbox_min, bbox_max, res, thresh, chunk)
    finally:
        model.train(was_training)
    labels, conf = out
    counts, boxes, csum = volume_stats(labels, conf, K)
    scores = torch.where(counts > 0, csum / counts.clamp_min(1).float(), torch.zeros_like(csum))
    return {"labels": labels, "confidence": conf, "res": res, "counts": counts, "boxes": boxes, "scores": scores}
