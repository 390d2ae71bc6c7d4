"""The three bit layouts of the mask stages and the torch primitives that build them (no kernel calls here).

A set of k boolean masks over a volume of V = W * L * H voxels (flattened index v, H fastest), or over the P = H * W
pixels of n views, is held one bit per (mask, element) in one of three forms.  The storage types are signed (torch has no
unsigned words); the kernels read the same bits as uint64 / uint32.

* BIT PLANES, int64 ``[k, ceil(V / 64)]``: one row per mask; bit ``v % 64`` of word ``v // 64`` of row i = mask i holds
  voxel v; the tail bits of the last word are zero.  A row is the mask's bytes packed little-endian
  (``np.packbits(..., bitorder="little")`` of the zero-padded row).  Written by ``evaluate.pack_mask_planes`` /
  ``pack_label_planes`` and ``detections.paste_masks``; read by the mask metric (``inr_mask_overlap``: AND + popcount).
* VOXEL WORDS, a list of ``ceil(k / 32)`` int32 ``[W, L, H]`` tensors: bit ``i % 32`` of the word of voxel v in tensor
  ``i // 32`` = mask i holds voxel v.  Written by ``masks.pack_mask_words`` and ``detections.planes_to_voxel_words``;
  read by the projector (``inr_project_masks_patch``: one word per sample serves 32 masks).
* PIXEL WORDS, int32 ``[n, ceil(k / 32), H, W]``: bit ``j % 32`` of word ``j // 32`` of a pixel of view v = candidate j
  covers that pixel.  Written by ``masks.pack_mask_bits`` and ``inr_pack_mask_bits``; read by the matcher
  (``inr_match_count``).

Bit planes put the ELEMENTS of one mask side by side in a word (``pack_planes`` / ``unpack_planes``); voxel and pixel
words put the MASKS of one element side by side (``interleave32``), and differ from each other only in what an element is
and in where the word index sits: voxel words are ``interleave32`` of bool ``[k, W, L, H]`` unbound along its first
axis, pixel words are ``interleave32`` of bool ``[k, n, H, W]`` with the first two axes swapped back.  So
``interleave32(unpack_planes(planes, V) != 0)`` viewed as ``[ceil(k / 32), W, L, H]`` turns planes into voxel words.
"""
import numpy as np
import torch

_STAGE = 1 << 21        # bits expanded at a time by pack_planes / unpack_planes: 16 MiB per int64 temporary


def as_tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def words(V):
    """Words of one bit plane over V voxels."""
    return (V + 63) // 64


def _blocks(k, nW):
    """(rows, first word, last word + 1) blocks that tile a [k, nW] plane set with at most ``_STAGE`` bits each (one
    word of one row at the least)."""
    cw = max(1, min(nW, _STAGE // 64))
    ck = max(1, _STAGE // (64 * cw))
    return [(slice(r, r + ck), w, min(nW, w + cw)) for r in range(0, k, ck) for w in range(0, nW, cw)]


def pack_planes(flat):
    """bool / uint8 ``[k, V]`` (non-zero = inside) -> bit planes int64 ``[k, ceil(V / 64)]``, tail bits zero.  The bits
    are widened to int64 a block of at most 2^21 (rows x words) at a time: three temporaries of at most 16 MiB, whatever
    k and V - not 8 bytes per voxel and mask."""
    k, V = (int(v) for v in flat.shape)
    planes = torch.empty(k, words(V), dtype=torch.int64, device=flat.device)
    shifts = torch.arange(64, device=flat.device, dtype=torch.int64)
    for rows, w0, w1 in _blocks(k, words(V)):
        bits = (flat[rows, 64 * w0:64 * w1] != 0).to(torch.int64)
        if bits.shape[1] != 64 * (w1 - w0):                                # the last word of a row: zero tail
            bits = torch.nn.functional.pad(bits, (0, 64 * (w1 - w0) - bits.shape[1]))
        planes[rows, w0:w1] = (bits.view(-1, w1 - w0, 64) << shifts).sum(-1)        # bit 63 wraps to the sign: same bits
    return planes


def unpack_planes(planes, V):
    """Bit planes int64 ``[k, ceil(V / 64)]`` -> uint8 ``[k, V]`` of 0 / 1, staged in the blocks of ``pack_planes`` (the
    same bound)."""
    k, nW = (int(v) for v in planes.shape)
    out = torch.empty(k, V, dtype=torch.uint8, device=planes.device)
    shifts = torch.arange(64, device=planes.device, dtype=torch.int64)
    for rows, w0, w1 in _blocks(k, nW):
        bits = ((planes[rows, w0:w1].unsqueeze(-1) >> shifts) & 1).to(torch.uint8)
        out[rows, 64 * w0:64 * w1] = bits.reshape(bits.shape[0], -1)[:, :V - 64 * w0]
    return out


def interleave32(bits):
    """bool ``[k, ...]`` -> int32 ``[ceil(k / 32), ...]``: bit ``i % 32`` of word ``i // 32`` = ``bits[i]``, OR-ed in one
    mask at a time (one int32 temporary of the size of a mask).  Bit 31 is the sign: the same 32 bits."""
    k = int(bits.shape[0])
    out = torch.zeros(((k + 31) // 32,) + tuple(bits.shape[1:]), dtype=torch.int32, device=bits.device)
    for i in range(k):
        out[i // 32] |= bits[i].to(torch.int32) * (1 << i % 32 if i % 32 < 31 else -2 ** 31)
    return out
