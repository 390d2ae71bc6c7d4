"""Line-sharing model of the field kernel's gathers (CPU, numpy): distinct 128-byte table lines per gather instruction
when two consecutive 16-sample tiles of the frame's sample stream are encoded apart (k_nerf_fwd) and when they are
merged into one instruction stream (k_nerf_fwd_pair).  The vector memory path prices a gather instruction by the distinct
lines its 64 lanes touch, and a line touched by two instructions is looked up twice (csrc/field_fused.hip).

Geometry of bench.py's frames: 800x800 pinhole views of the room at bound 1 (pixel pitch 1/400), constant step
dt = 2 sqrt(3) / 1024; a tile is one step of a 4x4 patch of rays, the next tile the next step of the same rays.

An instruction of the coarse levels (0..7) asks for ONE corner of a level for all its samples; one of the fine levels
(8..15) for both x neighbours of one yz corner.  Printed: distinct lines per level, summed over the instructions that
touch the level, per 32 samples, and the ratio of the totals.  The model counts per level - a real coarse instruction
mixes levels - so it says nothing about absolute look-ups; the ratio is what it is for.

    python tools/pair_line_model.py [--patches 102] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.hashgrid import PRIMES, level_table  # noqa: E402

ROWS_PER_LINE = 16          # 128-byte lines of 8-byte rows (fp32 [T, 2])


def patch_samples(rng, steps=4):
    """x01 [steps, 16, 3]: `steps` consecutive steps of a random 4x4 patch of rays from a camera inside the room"""
    eye = rng.uniform(-0.5, 0.5, 3)
    fwd = rng.normal(size=3)
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    u0, v0 = rng.uniform(-1.0, 1.0 - 4 / 400.0, 2)                  # the patch's corner on the image plane at focal 1
    ij = np.stack(np.meshgrid(np.arange(4), np.arange(4), indexing="ij"), -1).reshape(16, 2)
    d = fwd + (u0 + ij[:, :1] / 400.0) * right + (v0 + ij[:, 1:] / 400.0) * up
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dt = 2.0 * np.sqrt(3.0) / 1024.0
    t = rng.uniform(0.05, 1.5) + dt * np.arange(steps)
    x = np.clip(eye + t[:, None, None] * d[None], -1.0, 1.0)
    return ((x + 1.0) / 2.0).astype(np.float32)


def corner_lines(x01, table, level):
    """x01 [..., 3] -> table line of each of the 8 corners [..., 8]; corner = x | y << 1 | z << 2"""
    pos = x01 * np.float32(table["scales"][level]) + np.float32(0.5)
    cell = np.floor(pos).astype(np.uint64)
    res1 = int(table["resolutions"][level]) + 1
    rows = int(table["offsets"][level + 1]) - int(table["offsets"][level])
    out = []
    for k in range(8):
        c = cell + np.array([k & 1, (k >> 1) & 1, k >> 2], np.uint64)
        if table["hashed"][level]:
            h = ((c[..., 0] * PRIMES[0]) & 0xFFFFFFFF) ^ ((c[..., 1] * PRIMES[1]) & 0xFFFFFFFF) ^ ((c[..., 2] * PRIMES[2]) & 0xFFFFFFFF)
            row = h & np.uint64(rows - 1)
        else:
            row = c[..., 0] + c[..., 1] * res1 + c[..., 2] * res1 * res1
        out.append((row + int(table["offsets"][level])) // ROWS_PER_LINE)
    return np.stack(out, -1)


def instruction_lines(lines, level):
    """lines [n_samples, 8] of the samples ONE instruction stream covers -> distinct lines summed over its instructions"""
    if level < 8:
        return sum(len(np.unique(lines[:, k])) for k in range(8))
    return sum(len(np.unique(lines[:, [2 * yz, 2 * yz + 1]])) for yz in range(4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patches", type=int, default=102)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    table = level_table()
    rng = np.random.default_rng(args.seed)
    apart, merged = np.zeros(16), np.zeros(16)
    n_pairs = 0
    for _ in range(args.patches):
        x01 = patch_samples(rng)
        for level in range(16):
            lines = corner_lines(x01, table, level)                 # [4 steps, 16, 8]
            for s in (0, 2):
                apart[level] += instruction_lines(lines[s], level) + instruction_lines(lines[s + 1], level)
                merged[level] += instruction_lines(lines[s:s + 2].reshape(32, 8), level)
        n_pairs += 2
    apart /= n_pairs
    merged /= n_pairs
    print(f"{args.patches} patches x 4 steps, distinct lines per 32 samples")
    print("level   apart  merged")
    for level in range(16):
        print(f"{level:5d} {apart[level]:7.1f} {merged[level]:7.1f}")
    print(f"total {apart.sum():7.0f} {merged.sum():7.0f}   ratio {merged.sum() / apart.sum():.2f}")


if __name__ == "__main__":
    main()
