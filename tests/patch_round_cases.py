"""Hand-built clouds that keep the patch loop (S7-S9) going for several rounds, and points that stay raw to its end: the inputs of
tests/test_gpu_patch_rounds.py.  Pure numpy; the CPU oracle says what the patches of each are.

The slab: three parallel sheets of SIDE x SIDE points, STRIDE apart inside a sheet and GAP apart along the slab's normal.  With
STRIDE = 4 and GAP = 7 the sixteen nearest neighbours of a point are twelve of its own sheet (4 at 4, 4 at 5.66, 4 at 8) and the
points opposite in the neighbouring sheets (1 or 2 at 7, then 4 or 8 at 8.06): the sheets hang together.  GAP exceeds
surfaceThickness (4) plus the radius of either raw-point threshold (1 for the selection, 3 for the detection), so a depth map
takes one sheet and the sheet behind it stays raw -- and is far enough from the resampled cloud to seed the next round.

The partition is set by hand, plane by plane (a plane = a projection: 0..2 the axis towards smaller depth, 3..5 = axis + 3 from
the other side): the low and the middle sheet look down the normal (plane `axis`) and form ONE component, whose depth map keeps the
nearest = the low sheet; the high sheet looks from the other side (plane `axis + 3`) and is a component of its own.  Round 1
takes the two outer sheets, round 2 the middle one.

Left-over points: flat clumps of at most CLUMP points far from the slab and from each other, each in a plane that is neither of
the slab's and differs from the planes of the clumps around it.  A clump smaller than sixteen points fills its neighbour rows from
the nearest other clump or the slab, but a component does not cross planes: it never reaches minPointCountPerCCPatchSegmentation
and its points stay raw until the loop ends."""
import numpy as np

SIDE, STRIDE, GAP, BASE = 48, 4, 7, 40
CLUMP = 15


def _permute(pts, axis):
    """pts as (normal, a, b) -> x, y, z with the normal on `axis`"""
    out = np.empty_like(pts)
    out[:, axis], out[:, (axis + 1) % 3], out[:, (axis + 2) % 3] = pts[:, 0], pts[:, 1], pts[:, 2]
    return out


def slab(axis):
    """(xyz int16, rgb uint8, partition uint32) of the three sheets, the slab's normal along `axis`"""
    a, b = np.meshgrid(np.arange(SIDE) * STRIDE + BASE, np.arange(SIDE) * STRIDE + BASE, indexing="ij")
    sheets = [np.stack([np.full(a.size, BASE + s * GAP), a.ravel(), b.ravel()], 1) for s in range(3)]
    xyz = _permute(np.concatenate(sheets), axis).astype(np.int16)
    part = np.repeat(np.array([axis, axis, axis + 3], np.uint32), SIDE * SIDE)
    rng = np.random.default_rng(axis)
    # interleave the sheets in index order (a seed of the middle sheet may be the smallest index of its component), and colours
    # close enough that the D1 test would pass wherever the depths allowed it
    order = rng.permutation(len(xyz))
    rgb = (100 + rng.integers(0, 20, (len(xyz), 3))).astype(np.uint8)
    return xyz[order], rgb, part[order]


def clumps(axis, sizes):
    """(xyz, partition) of flat clumps of the given sizes on a grid of centres 40 apart in a corner of the cube the slab leaves free"""
    free = [v for v in range(6) if v % 3 != axis]                    # the four planes the slab does not use
    xyz, part = [], []
    for c, m in enumerate(sizes):
        gx, gy = c % 5, c // 5
        plane = free[(gx + 2 * gy) % 4]                              # the clumps 40 apart (and diagonal) lie in other planes
        i = np.arange(m)
        flat = np.stack([np.zeros(m, np.int64), i % 5, i // 5], 1)  # a lattice of 5 columns, its normal = the plane's axis
        centre = np.array([600 + 40 * gx, 600 + 40 * gy, 600 + 7 * (c % 3)])
        xyz.append(_permute(flat, plane % 3) + centre)
        part.append(np.full(m, plane, np.uint32))
    if not xyz:
        return np.zeros((0, 3), np.int16), np.zeros(0, np.uint32)
    return np.concatenate(xyz).astype(np.int16), np.concatenate(part)


def clump_sizes(k):
    """k left-over points as clumps of CLUMP points and one smaller"""
    return [CLUMP] * (k // CLUMP) + ([k % CLUMP] if k % CLUMP else [])


def slab_with_clumps(axis, sizes):
    """the slab followed by the clumps (the clumps' points have the largest indices; the slab's own order is interleaved)"""
    xyz, rgb, part = slab(axis)
    cx, cp = clumps(axis, sizes)
    rng = np.random.default_rng(len(cx))
    crgb = rng.integers(0, 256, (len(cx), 3)).astype(np.uint8)
    return np.concatenate([xyz, cx]), np.concatenate([rgb, crgb]), np.concatenate([part, cp])
