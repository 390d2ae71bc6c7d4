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
import contextlib

import numpy as np
import torch

from . import _lib

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


def cached_axes(bbox_min, bbox_max, res, device):
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


def _resolve_lattice(model, bbox_min, bbox_max, max_side, res, axes=False):
    """The lattice of an extraction call: -> (the model's device, bbox_min, bbox_max float32 [3] (default
    [-bound, bound]^3), res int64 [3] (default ``grid_resolution`` with ``max_side``), ``cached_axes`` of it or None)."""
    dev = next(model.parameters()).device
    b = float(model.bound)
    bbox_min = np.asarray([-b, -b, -b] if bbox_min is None else bbox_min, dtype=np.float32)
    bbox_max = np.asarray([b, b, b] if bbox_max is None else bbox_max, dtype=np.float32)
    res = grid_resolution(bbox_min, bbox_max, max_side) if res is None else np.asarray(res, dtype=np.int64)
    return dev, bbox_min, bbox_max, res, cached_axes(bbox_min, bbox_max, res, dev) if axes else None


def view_dirs(model, device):
    """``VIEW_DIRS`` on ``device`` and their SH rows (``model.encoder_dir``; None for a model without one), uploaded once
    and kept on the model: -> (dirs float32 [4, 3], sh [4, 16] / None)."""
    cached = getattr(model, "_view_dirs_dev", None)
    if cached is None or cached[0].device != device:
        d = torch.from_numpy(VIEW_DIRS).to(device)
        cached = model._view_dirs_dev = (d, model.encoder_dir(d).contiguous() if hasattr(model, "encoder_dir") else None)
    return cached


@contextlib.contextmanager
def eval_mode(model):
    """The model in eval mode inside the block, its previous mode restored on any exit."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


LOGIT_MIN = float(np.log(1e-30))      # floor of the density logit, log(sigma.clamp_min(1e-30)), on every path
LABEL_EMPTY = 255                     # label of an unoccupied voxel


def sweep_lattice(model, bbox_min, bbox_max, res, chunk, want_rgb=False, thresh=None, forward_dirs=False):
    """The composable form of the lattice launches, with their semantics, over chunks of points: voxel centres clamped to
    [-bound, bound], ``density()`` once per chunk.  -> (logit, rgb, labels, confidence) over [W, L, H]: the density logit;
    with ``want_rgb`` (else None) float32 [W, L, H, 4], channels 0..2 = ``color()`` averaged over ``VIEW_DIRS``, channel 3
    = 0, left to the caller; with ``thresh`` (else None) uint8 labels and float32 confidence: a point is occupied when
    density_scale * sigma >= thresh and then carries the arg-max over the K real channels of ``instance()`` (torch.argmax:
    lowest on ties) and its softmax probability, ``LABEL_EMPTY`` / 0 otherwise; ``instance()`` is not called for a chunk
    without an occupied point.  ``forward_dirs`` (rgb without labels): a chunk goes through ``model.forward_dirs`` - one
    launch: gather + sigma net once, colour net per direction - when that exists and answers."""
    dev = next(model.parameters()).device
    b = float(model.bound)
    W, L, H = (int(v) for v in res)
    pts = lattice(bbox_min, bbox_max, res, dev)
    N = pts.shape[0]
    logit = torch.empty(N, dtype=torch.float32, device=dev)
    rgb = torch.zeros(N, 4, dtype=torch.float32, device=dev) if want_rgb else None
    dirs = view_dirs(model, dev)[0] if want_rgb else None
    labels = torch.full((N,), LABEL_EMPTY, dtype=torch.uint8, device=dev) if thresh is not None else None
    conf = torch.zeros(N, dtype=torch.float32, device=dev) if thresh is not None else None
    forward_dirs = forward_dirs and hasattr(model, "forward_dirs")
    for s in range(0, N, chunk):
        x = pts[s:s + chunk].clamp(-b, b).contiguous()
        fused = model.forward_dirs(x, dirs) if forward_dirs else None
        if fused is not None:
            rgb[s:s + chunk, :3] = fused[:, :3]
            logit[s:s + chunk] = fused[:, 3].clamp(min=LOGIT_MIN)
            continue
        den = model.density(x)
        logit[s:s + chunk] = torch.log(den["sigma"].clamp_min(1e-30))
        if want_rgb:
            acc = torch.zeros(x.shape[0], 3, dtype=torch.float32, device=dev)
            for v in range(dirs.shape[0]):
                acc += model.color(x, dirs[v].expand(x.shape[0], 3).contiguous(), geo_feat=den["geo_feat"])
            rgb[s:s + chunk, :3] = acc / dirs.shape[0]
        if thresh is None:
            continue
        occ = den["sigma"] * model.density_scale >= thresh
        if not bool(occ.any()):
            continue
        logits = model.instance(x)[:, :model.num_instances].float()       # the K real channels only
        mx, arg = logits.amax(1), torch.argmax(logits, 1)
        c = 1.0 / torch.exp(logits - mx[:, None]).sum(1)
        labels[s:s + chunk] = torch.where(occ, arg.to(torch.uint8), torch.full_like(labels[s:s + chunk], LABEL_EMPTY))
        conf[s:s + chunk] = torch.where(occ, c, torch.zeros_like(c))
    return tuple(None if t is None else t.view(W, L, H, *t.shape[1:]) for t in (logit, rgb, labels, conf))


@torch.no_grad()
def extract_rgbsigma(model, bbox_min=None, bbox_max=None, max_side=160, res=None, chunk=1 << 22):
    """-> (rgbsigma float32 [W,L,H,4] on the model's device, res int64[3]).  Channel 3 = log(sigma)."""
    lattice_launch = hasattr(model, "forward_lattice")
    dev, bbox_min, bbox_max, res, axes = _resolve_lattice(model, bbox_min, bbox_max, max_side, res, axes=lattice_launch)
    with eval_mode(model):
        if lattice_launch:
            # one launch for the whole lattice, from its three coordinate axes (no [W*L*H, 3] point tensor), walked in
            # runs along W: 160^3 in 1.4 ms instead of 2.8 (profiles/r04_NOTES.txt 6); the density logit's lower clamp
            # (as on the point-list path) is applied inside the launch
            dirs, sh = view_dirs(model, dev)
            fused = model.forward_lattice(axes, dirs, logit_min=LOGIT_MIN, sh=sh)
            if fused is not None:
                return fused, res
        logit, out, _, _ = sweep_lattice(model, bbox_min, bbox_max, res, chunk, want_rgb=True, forward_dirs=True)
    out[..., 3] = logit
    return out, res


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
def volume_stats(labels, confidence, K):
    """Per-channel statistics of a label volume (uint8 [W, L, H], ``LABEL_EMPTY`` = unoccupied): -> (counts int64 [K],
    boxes int64 [K, 6] = inclusive voxel-index bounds (min iw, il, ih, max iw, il, ih; -1 for an empty channel),
    conf_sum float32 [K]), on the volume's device.  On the GPU (K <= 64) one bit-reproducible HIP call
    (``inr_instance_volume_stats``: fixed per-workgroup slots, fixed-order final pass); otherwise numpy on the host
    (float64 sums)."""
    W, L, H = (int(v) for v in labels.shape)
    if labels.is_cuda and 1 <= K <= 64:
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


# ---- connected components of a label volume (include/inr.h, "connected components") --------------------------------------
def _neighbour_offsets(connectivity):
    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    offs = [(dw, dl, dh) for dw in (-1, 0, 1) for dl in (-1, 0, 1) for dh in (-1, 0, 1) if (dw, dl, dh) != (0, 0, 0)]
    return [o for o in offs if connectivity == 26 or abs(o[0]) + abs(o[1]) + abs(o[2]) == 1]


def _check_label_volume(labels, who):
    if not torch.is_tensor(labels) or labels.dim() != 3 or labels.dtype != torch.uint8:
        raise ValueError(f"{who}: labels must be a uint8 [W, L, H] tensor")
    if labels.numel() == 0 or labels.numel() >= 2 ** 31:
        raise ValueError(f"{who}: the volume must hold 1 .. 2^31 - 1 voxels")


def _side(n, d):
    """The slices of an axis of length n that pair every voxel (first) with its neighbour at offset d (second)."""
    return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))


def _label_composable(labels, connectivity):
    """Roots by neighbour-min propagation with pointer jumping, in plain torch on the volume's device: every voxel takes
    the smallest parent among its connected neighbours, hands it to its own parent (a scatter-min), and all parent chains
    are then halved until they are flat; repeated until nothing changes.  Parents only decrease and stay inside the
    component, so the fixed point is the smallest linear index of the component."""
    W, L, H = (int(v) for v in labels.shape)
    N = W * L * H
    lab = labels.contiguous()
    live = (lab != LABEL_EMPTY).reshape(-1)
    idx = torch.arange(N, dtype=torch.int64, device=lab.device)
    pairs = []
    for dw, dl, dh in _neighbour_offsets(connectivity):
        (aw, bw), (al, bl), (ah, bh) = _side(W, dw), _side(L, dl), _side(H, dh)
        a, b = (aw, al, ah), (bw, bl, bh)
        if lab[a].numel():
            pairs.append((a, b, (lab[a] == lab[b]) & (lab[a] != LABEL_EMPTY)))
    parent = idx.clone()
    while True:
        low = parent.clone().view(W, L, H)
        pv = parent.view(W, L, H)
        for a, b, same in pairs:
            low[a] = torch.where(same, torch.minimum(low[a], pv[b]), low[a])
        low = low.reshape(-1)
        nxt = torch.minimum(parent, low)
        nxt.scatter_reduce_(0, parent, low, "amin")
        while True:
            hop = nxt[nxt]
            if torch.equal(hop, nxt):
                break
            nxt = hop
        if torch.equal(nxt, parent):
            break
        parent = nxt
    return torch.where(live, parent, torch.full_like(parent, -1)).to(torch.int32).view(W, L, H)


def _workspace(nbytes, what, dtype, dev):
    """The caller-owned workspace of a library call, from the answer of its ``*_workspace_bytes`` export (negative: the
    export's error, raised as ``what``): -> (tensor of ``dtype``, nbytes)."""
    nbytes = int(nbytes)
    _lib.check(min(nbytes, 0), what)
    return torch.empty(nbytes // dtype.itemsize, dtype=dtype, device=dev), nbytes


def _label_hip(labels, connectivity):
    lib = _lib.load()
    W, L, H = (int(v) for v in labels.shape)
    labels = labels.contiguous()
    ws, nbytes = _workspace(lib.inr_components_workspace_bytes(W, L, H), "components_workspace_bytes", torch.int64,
                            labels.device)
    roots = torch.empty(W, L, H, dtype=torch.int32, device=labels.device)
    _lib.check(lib.inr_components_label(_lib.ptr(labels, torch.uint8, "labels"), W, L, H, int(connectivity), _lib.ptr(ws),
                                        nbytes, _lib.ptr(roots), _lib.stream_ptr()), "components_label")
    return labels, roots, ws, nbytes


def label_components(labels, connectivity=6, fused=True):
    """Connected components of a label volume (uint8 [W, L, H], ``LABEL_EMPTY`` = empty): two voxels are connected when
    they are neighbours (``connectivity`` 6 = faces, 26 = faces, edges and corners) and carry the same label.
    -> ``roots`` int32 [W, L, H]: the smallest linear index ``(iw * L + il) * H + ih`` of the voxel's component, -1 for an
    empty voxel.  A GPU tensor goes through ``inr_components_label`` (three HIP launches; identical bits on every call);
    a CPU tensor, or ``fused=False``, through the same semantics in plain torch."""
    _check_label_volume(labels, "label_components")
    _neighbour_offsets(connectivity)
    if labels.is_cuda and fused:
        return _label_hip(labels, connectivity)[1]
    return _label_composable(labels, int(connectivity))


def _filter_composable(labels, roots, confidence, K, first, min_voxels, largest):
    W, L, H = (int(v) for v in labels.shape)
    N = W * L * H
    dev = labels.device
    lab = labels.reshape(-1).long()
    r = roots.reshape(-1).long()
    sizes = torch.bincount(r[r >= 0], minlength=N)
    is_root = r == torch.arange(N, dtype=torch.int64, device=dev)
    root_idx = torch.nonzero(is_root & (lab >= first) & (lab < K)).reshape(-1)
    ch, sz = lab[root_idx], sizes[root_idx]
    n_components = torch.bincount(ch, minlength=K)[:K]
    ok = sz >= min_voxels
    kept_root = torch.full((K,), -1, dtype=torch.int64, device=dev)
    if largest:
        key = torch.where(ok, sz * (1 << 31) + ((1 << 31) - 1 - root_idx), torch.zeros_like(sz))     # size, then lowest root
        best = torch.zeros(K, dtype=torch.int64, device=dev)
        best.scatter_reduce_(0, ch, key, "amax")
        kept_root = torch.where(best > 0, (1 << 31) - 1 - best % (1 << 31), kept_root)
        ok = ok & (root_idx == kept_root[ch])
    kept_voxels = torch.zeros(K, dtype=torch.int64, device=dev)
    kept_voxels.scatter_add_(0, ch[ok], sz[ok])
    survives = torch.zeros(N, dtype=torch.bool, device=dev)
    survives[root_idx[ok]] = True
    filtered = (lab >= first) & (lab < K)
    keep = ~filtered | survives[r.clamp_min(0)]
    out = torch.where(keep, labels.reshape(-1), torch.full_like(labels.reshape(-1), LABEL_EMPTY)).view(W, L, H)
    conf = None
    if confidence is not None:
        conf = torch.where(keep, confidence.reshape(-1), torch.zeros_like(confidence.reshape(-1))).view(W, L, H)
    return out, conf, n_components.to(torch.int32), kept_voxels.to(torch.int32), kept_root.to(torch.int32)


def filter_components(labels, confidence=None, K=None, connectivity=6, keep="largest", min_voxels=1, skip_background=True,
                      fused=True):
    """Labels the components of ``labels`` (``label_components``) and applies the keep rule to every channel
    ``first..K-1`` (``first`` = 1 with ``skip_background``, else 0): a component survives when it has at least
    ``min_voxels`` voxels and, with ``keep="largest"``, is the channel's largest (the lowest root among equals);
    ``keep="all"`` applies the size rule alone.  Labels below ``first`` or >= K pass through.  -> dict: ``labels`` uint8
    (``LABEL_EMPTY`` where a voxel was dropped), ``confidence`` (0 there; None without the input), ``roots`` int32 (of the
    INPUT volume), ``n_components`` / ``kept_voxels`` / ``kept_root`` int32 [K] (``kept_root`` -1 when nothing survives and
    always with ``keep="all"``).  GPU tensors: ``inr_components_label`` + ``inr_components_filter``; CPU tensors or
    ``fused=False``: plain torch, same semantics."""
    _check_label_volume(labels, "filter_components")
    _neighbour_offsets(connectivity)
    if K is None or not 1 <= int(K) <= LABEL_EMPTY:
        raise ValueError(f"filter_components: K must be 1..{LABEL_EMPTY}")
    if keep not in ("largest", "all"):
        raise ValueError('filter_components: keep must be "largest" or "all"')
    if int(min_voxels) < 1:
        raise ValueError("filter_components: min_voxels must be >= 1")
    K, min_voxels, largest = int(K), int(min_voxels), keep == "largest"
    first = min(1, K) if skip_background else 0
    if confidence is not None and (tuple(confidence.shape) != tuple(labels.shape) or confidence.dtype != torch.float32 or
                                   confidence.device != labels.device):
        raise ValueError("filter_components: confidence must be float32, of the labels' shape and device")
    if labels.is_cuda and fused:
        lib = _lib.load()
        W, L, H = (int(v) for v in labels.shape)
        labels, roots, ws, nbytes = _label_hip(labels, connectivity)
        dev = labels.device
        out = torch.empty_like(labels)
        conf = confidence.contiguous() if confidence is not None else None
        conf_out = torch.empty_like(conf) if conf is not None else None
        per = torch.empty(3, K, dtype=torch.int32, device=dev)
        P = _lib.ptr
        _lib.check(lib.inr_components_filter(P(labels), P(roots), P(conf, torch.float32, "confidence", allow_none=True), W, L, H,
                                             K, first, min_voxels, int(largest), P(ws), nbytes, P(out),
                                             P(conf_out, allow_none=True), P(per[0]), P(per[1]), P(per[2]),
                                             _lib.stream_ptr()), "components_filter")
        n_components, kept_voxels, kept_root = per[0], per[1], per[2]
    else:
        roots = _label_composable(labels, int(connectivity))
        out, conf_out, n_components, kept_voxels, kept_root = _filter_composable(labels, roots, confidence, K, first,
                                                                                 min_voxels, largest)
    return {"labels": out, "confidence": conf_out, "roots": roots, "n_components": n_components, "kept_voxels": kept_voxels,
            "kept_root": kept_root}


@torch.no_grad()
def extract_instances(model, bbox_min=None, bbox_max=None, max_side=160, res=None, sigma_thresh=None, fused=True,
                      chunk=1 << 20, components=None, connectivity=6, min_component_voxels=1):
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
    cover) runs the composable path - ``density()`` + ``instance()`` over chunks of points - with the same semantics.

    ``components="largest"`` / ``"all"`` (default None: off) drops floaters first: the label volume goes through
    ``filter_components`` (``connectivity``, ``min_component_voxels``; channel 0, the walls, is left alone), so ``labels``,
    ``confidence``, ``counts``, ``boxes`` and ``scores`` describe the kept voxels, and the result gains ``n_components``
    int32 [K] (components per channel before the rule) and ``raw_counts`` int64 [K] (voxels per channel before it)."""
    if components not in (None, "largest", "all"):
        raise ValueError('extract_instances: components must be None, "largest" or "all"')
    if not getattr(model, "num_instances", 0):
        raise ValueError("extract_instances: the model has no instance head (num_instances = 0)")
    lattice_launch = fused and hasattr(model, "instance_lattice")
    _, bbox_min, bbox_max, res, axes = _resolve_lattice(model, bbox_min, bbox_max, max_side, res, axes=lattice_launch)
    thresh = float(model.density_thresh if sigma_thresh is None else sigma_thresh)
    K = int(model.num_instances)
    if K >= LABEL_EMPTY:
        raise ValueError(f"extract_instances: {K} instance channels do not fit the uint8 labels (at most {LABEL_EMPTY - 1})")
    with eval_mode(model):
        out = model.instance_lattice(axes, thresh) if lattice_launch else None
        if out is None:
            out = sweep_lattice(model, bbox_min, bbox_max, res, chunk, thresh=thresh)[2:]
    labels, conf = out
    extra = {}
    if components is not None:
        extra["raw_counts"] = torch.bincount(labels.reshape(-1).long(), minlength=LABEL_EMPTY + 1)[:K]
        kept = filter_components(labels, conf, K=K, connectivity=connectivity, keep=components,
                                 min_voxels=min_component_voxels, skip_background=True, fused=fused)
        labels, conf, extra["n_components"] = kept["labels"], kept["confidence"], kept["n_components"]
    counts, boxes, csum = volume_stats(labels, conf, K)
    scores = torch.where(counts > 0, csum / counts.clamp_min(1).float(), torch.zeros_like(csum))
    return {"labels": labels, "confidence": conf, "res": res, "counts": counts, "boxes": boxes, "scores": scores, **extra}


# ---- triangle meshes of the density field ---------------------------------------------------------------------------
# Half-width of the band of density logits the vertex interpolation sees, around iso = log(threshold / density_scale).
# 2.0 keeps sigma within a factor e^2 (~7.4) of the threshold on either side - the range over which a trained density
# actually rises across a surface.  Outside that band the logit says nothing about where the surface is: empty space sits
# at the extraction's floor (log 1e-30 = -69) and solid space saturates, so an unclamped interpolation between -69 and +5
# would put every vertex within 4 % of a cell from its inside corner (the staircase of the voxel grid), and a much
# smaller value would snap every vertex to the middle of its edge.
MESH_CLAMP = 2.0


def mesh_from_lattice(field, iso, axes, ext, labels=None, select=-1, rgb=None, face_labels=False, cap=True,
                      clamp=MESH_CLAMP):
    """Marching tetrahedra on the GPU (``inr_mesh_count`` + ``inr_mesh_emit``, semantics in include/inr.h) of a lattice
    field that is already on the device.  ``field`` float32 [W, L, H], dense or a channel view of a dense [W, L, H, C]
    tensor (read in place); ``axes`` = the three coordinate axes; ``ext`` = three floats, the step of the virtual layer
    for an axis of length 1; ``labels`` uint8 [W, L, H] with ``select`` = -1 or a channel; ``rgb`` float32 [W, L, H, 4]
    (channels 0..2 colour the vertices).  One host read-back of (V, F) between the two calls.
    -> dict vertices float32 [V, 3], faces int32 [F, 3], colors float32 [V, 3] / None, face_labels uint8 [F] / None."""
    lib = _lib.load()
    if not field.is_cuda:
        raise RuntimeError("mesh_from_lattice: field must be a GPU tensor (the HIP path has no CPU fallback)")
    if field.dim() != 3 or field.dtype != torch.float32:
        raise RuntimeError("mesh_from_lattice: field must be float32 [W, L, H]")
    W, L, H = (int(v) for v in field.shape)
    if W * L * H == 0:
        raise RuntimeError("mesh_from_lattice: empty lattice")
    stride = int(field.stride(2))
    if stride < 1 or tuple(field.stride()) != (L * H * stride, H * stride, stride):      # not a channel view of a dense volume
        field, stride = field.contiguous(), 1
    dev = field.device
    if labels is not None:
        _lib.ptr(labels, torch.uint8, "labels")
        if tuple(labels.shape) != (W, L, H):
            raise RuntimeError("mesh_from_lattice: labels must be [W, L, H]")
    if rgb is not None and (tuple(rgb.shape) != (W, L, H, 4) or rgb.dtype != torch.float32 or not rgb.is_contiguous()):
        raise RuntimeError("mesh_from_lattice: rgb must be contiguous float32 [W, L, H, 4]")
    if face_labels and labels is None:
        raise RuntimeError("mesh_from_lattice: face_labels needs labels")
    ax = [a.contiguous().float() for a in axes]
    if [int(a.shape[0]) for a in ax] != [W, L, H]:
        raise RuntimeError("mesh_from_lattice: the axes do not match the field")
    cap = 1 if cap else 0
    ws, nbytes = _workspace(lib.inr_mesh_workspace_bytes(W, L, H, cap), "mesh_workspace_bytes", torch.int32, dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    P = _lib.ptr
    fptr, lptr = _lib.c_void_p(field.data_ptr()), P(labels, torch.uint8, "labels", allow_none=True)
    head = (fptr, stride, float(iso), float(clamp), lptr, int(select))
    _lib.check(lib.inr_mesh_count(*head, W, L, H, cap, P(ws), nbytes, P(counts), _lib.stream_ptr()), "mesh_count")
    V, F = (int(v) for v in counts.tolist())                 # the one host read-back
    vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    colors = torch.empty(V, 3, dtype=torch.float32, device=dev) if rgb is not None else None
    flab = torch.empty(F, dtype=torch.uint8, device=dev) if face_labels else None
    if V or F:
        _lib.check(lib.inr_mesh_emit(*head, P(rgb, allow_none=True), P(ax[0]), P(ax[1]), P(ax[2]), W, L, H, float(ext[0]),
                                     float(ext[1]), float(ext[2]), cap, P(ws), nbytes, V, F, _lib.ptr_or_null(vertices),
                                     _lib.ptr_or_null(faces), P(colors, allow_none=True), P(flab, allow_none=True),
                                     _lib.stream_ptr()), "mesh_emit")
    return {"vertices": vertices, "faces": faces, "colors": colors, "face_labels": flab}


def _mesh_lattices_fused(model, axes, thresh, labels, colors):
    """``mesh_lattices`` through the lattice launches: -> (field, labels, rgb).  field is None when a launch the call needs
    is missing or answered None; rgb is None also when the call did not need that launch."""
    field = lab = rgb = None
    if labels:                                   # labels and field from one launch
        out = model.instance_lattice(axes, thresh, want_logit=True) if hasattr(model, "instance_lattice") else None
        if out is None:
            return None, None, None
        lab, _, field = out
    if (colors or not labels) and hasattr(model, "forward_lattice"):
        dirs, sh = view_dirs(model, axes[0].device)
        rgb = model.forward_lattice(axes, dirs, logit_min=LOGIT_MIN, sh=sh)
        if not labels and rgb is not None:
            field = rgb[..., 3]                  # channel 3 as a stride-4 view, read in place by the mesh kernels
    return field, lab, rgb


@torch.no_grad()
def mesh_lattices(model, bbox_min=None, bbox_max=None, resolution=256, res=None, threshold=10.0, labels=False, colors=True,
                  fused=True, components=None, connectivity=6, min_component_voxels=1):
    """The field launches of ``extract_mesh``, once: -> dict ``field`` (density logit float32 [W, L, H], possibly a view),
    ``labels`` (uint8 [W, L, H] or None), ``rgb`` (float32 [W, L, H, 4] or None), ``axes``, ``ext``, ``iso``, ``res``,
    ``bbox_min``, ``bbox_max``.  ``mesh_of_lattices`` turns it into any number of meshes.  ``components="largest"`` /
    ``"all"`` filters the label volume once (``filter_components``, channel 0 left alone), so ``instance=k`` then meshes
    the kept component(s) of k only."""
    if components not in (None, "largest", "all"):
        raise ValueError('mesh_lattices: components must be None, "largest" or "all"')
    if components is not None and not labels:
        raise ValueError("mesh_lattices: components filters the label volume and needs labels=True")
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError("extract_mesh: the model must be on a GPU (the HIP path has no CPU fallback)")
    if not float(threshold) > 0:
        raise ValueError("extract_mesh: threshold must be > 0 (the surface is density_scale * sigma = threshold)")
    if labels and not getattr(model, "num_instances", 0):
        raise ValueError("extract_mesh: the model has no instance head (num_instances = 0)")
    _, bbox_min, bbox_max, res, axes = _resolve_lattice(model, bbox_min, bbox_max, resolution, res, axes=True)
    iso = float(np.log(np.float32(threshold) / np.float32(getattr(model, "density_scale", 1.0)), dtype=np.float32))
    with eval_mode(model):
        field, lab, rgb = _mesh_lattices_fused(model, axes, float(threshold), labels, colors) if fused else (None,) * 3
        if field is None or (colors and rgb is None):            # all of it from the sweep: no mixing of the two paths
            field, rgb, lab, _ = sweep_lattice(model, bbox_min, bbox_max, res, 1 << 20, want_rgb=colors,
                                        thresh=float(threshold) if labels else None)
    if components is not None and lab is not None:
        lab = filter_components(lab, None, K=int(model.num_instances), connectivity=connectivity, keep=components,
                                min_voxels=min_component_voxels, skip_background=True, fused=fused)["labels"]
    ext = [float(np.float32(bbox_max[a]) - np.float32(bbox_min[a])) for a in range(3)]
    return {"field": field, "labels": lab, "rgb": rgb if colors else None, "axes": axes, "ext": ext, "iso": iso, "res": res,
            "bbox_min": bbox_min, "bbox_max": bbox_max}


def mesh_of_lattices(lat, instance=None, face_labels=None, colors=True, cap=True, clamp=MESH_CLAMP):
    """One mesh of the lattices ``mesh_lattices`` returned (two mesh launches and one read-back; no field launch)."""
    if instance is not None and (lat["labels"] is None or not 0 <= int(instance) < LABEL_EMPTY):
        raise ValueError("extract_mesh: instance needs a model with an instance head and a channel 0..254")
    want_fl = (lat["labels"] is not None and instance is None) if face_labels is None else bool(face_labels)
    out = mesh_from_lattice(lat["field"], lat["iso"], lat["axes"], lat["ext"], labels=lat["labels"],
                            select=-1 if instance is None else int(instance), rgb=lat["rgb"] if colors else None,
                            face_labels=want_fl, cap=cap, clamp=clamp)
    out["res"] = lat["res"]
    return out


@torch.no_grad()
def extract_mesh(model, bbox_min=None, bbox_max=None, resolution=256, res=None, threshold=10.0, instance=None,
                 face_labels=None, colors=True, cap=True, clamp=MESH_CLAMP, fused=True, min_component_voxels=0,
                 connectivity=6):
    """Triangle mesh of the surface ``density_scale * sigma = threshold`` (the sigma the renderer composites, as in
    ``extract_instances``) on the voxel-centre lattice of ``extract_rgbsigma`` (longest side ``resolution``, default box
    [-bound, bound]^3), extracted on the GPU by marching tetrahedra (include/inr.h, "iso-surface meshes").  -> dict on the
    model's device: ``vertices`` float32 [V, 3], ``faces`` int32 [F, 3] (normals point out of the dense side),
    ``colors`` float32 [V, 3] or None (rgb averaged over the four extraction view directions), ``face_labels`` uint8 [F]
    or None, ``res``.  Nothing above the threshold gives empty tensors, not an error.

    The scalar field is the density LOGIT, log sigma, and ``iso = log(threshold / density_scale)`` is formed once on the
    host in fp32; vertices are interpolated in the logit, clamped to ``iso +- clamp``.  Upstream interpolates sigma
    itself: sigma jumps by orders of magnitude across one cell at a surface, which pins every vertex to its inside corner;
    the logit is close to linear there.

    ``instance=k``: the surface of the voxels whose instance label (``extract_instances``' arg-max) is k, closed on its
    own.  ``face_labels`` (default: on for a model with an instance head, when ``instance`` is None): per face, the
    label of the tetrahedron's densest inside corner; 255 where the label volume and the logit disagree at the
    threshold's rounding.  ``cap``: close surfaces that reach the box.  Labels come from ``instance_lattice`` (one fused
    launch, with the logit), colours from ``forward_lattice``; ``fused=False`` and shapes the fused kernels do not cover
    go through ``density()`` / ``color()`` / ``instance()``.  The mesh kernels themselves have no fallback.

    ``min_component_voxels`` > 0 (scene mesh only, default 0 = off) drops floaters: the lattice points with
    ``field >= iso`` form a one-channel label volume (0 inside, 255 outside), components (``connectivity``) below that
    size are dropped (``filter_components``), and the kept points are meshed with ``select=0``.  No face labels then."""
    if int(min_component_voxels) > 0:
        if instance is not None or face_labels:
            raise ValueError("extract_mesh: min_component_voxels filters the scene mesh (no instance, no face_labels)")
        lat = mesh_lattices(model, bbox_min, bbox_max, resolution, res, threshold, labels=False, colors=colors, fused=fused)
        inside = lat["field"] >= lat["iso"]
        solid = torch.where(inside, torch.zeros_like(inside, dtype=torch.uint8),
                            torch.full_like(inside, LABEL_EMPTY, dtype=torch.uint8)).contiguous()
        lat["labels"] = filter_components(solid, None, K=1, connectivity=connectivity, keep="all",
                                          min_voxels=int(min_component_voxels), skip_background=False,
                                          fused=fused)["labels"]
        return mesh_of_lattices(lat, instance=0, face_labels=False, colors=colors, cap=cap, clamp=clamp)
    need_labels = instance is not None or (bool(getattr(model, "num_instances", 0)) if face_labels is None else bool(face_labels))
    lat = mesh_lattices(model, bbox_min, bbox_max, resolution, res, threshold, labels=need_labels, colors=colors, fused=fused)
    return mesh_of_lattices(lat, instance=instance, face_labels=face_labels, colors=colors, cap=cap, clamp=clamp)
