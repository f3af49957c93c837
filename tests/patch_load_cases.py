"""Hand-built clouds for the per-point passes of the patch rounds (S7-S9), each a few thousand points at most: the inputs of
tests/test_gpu_patch_round_loads.py.  Pure numpy; the CPU oracle says what the patches of each are.

Planes as in patch_round_cases.py: 0..2 = the axis of the projection seen from the low side, 3..5 = axis + 3 from the other side.
A component never crosses planes, so the plane is also what keeps neighbouring pieces of a cloud apart.

The probe units.  The raw-point update looks for the resampled cloud around every point still raw, in the order of a table of
offsets sorted by (squared distance, dz, dy, dx) -- the own voxel, 6 at d2 = 1, 12 at 2, 8 at 3, 6 at 4, 24 at 5, 24 at 6, 12 at
8, 30 at 9: 123 at the CTC thresholds -- and all that is ever seen of the result is two thresholds: d2 <= selection takes the point
off the raw list, d2 > detection makes it a seed.  Every point is a seed in round 1, so a probe is visible only on a point that
round 1 LEFT raw.  A unit is

  front   8 x 8 points 4 apart in one layer: with the hidden layer one component, and what its depth map keeps;
  hidden  4 x 4 points 8 apart, 7 behind the front (farther than surfaceThickness): raw after round 1, sixteen points -- exactly
          what a component needs to become a patch -- and far from everything resampled, so all of them are seeds, except
  the test point, the last of them by index, which has
  a column  of sixteen points (another plane: a patch of round 1, resampled) that starts at a chosen offset from the test point
          and runs away from both layers, so that the offset is the FIRST hit of the test point's walk through the table.

The hidden layer becomes a patch of round 2 exactly if the test point is still raw: d2 of the offset > selection.  Moving the
selection threshold (the table reaches as far as the larger threshold, the detection's 9, whatever the selection is) makes every
d2 of the table a boundary, and a probe that is missed shows as a patch the oracle does not have.  Units differ in the offset --
one per squared distance, on axes and diagonals, and one per table index next to a batch's edge -- in the axis of the layers,
and in the side the layers are seen from; three sit in corners of the cube, so that probes around them fall off the grid."""
import numpy as np

PROBE_R2 = 9


def probe_offsets(r2=PROBE_R2):
    """the table as the library sorts it: [(dx, dy, dz)], by d2, then dz, dy, dx"""
    r = int(r2 ** 0.5) + 1
    tmp = []
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                d2 = dx * dx + dy * dy + dz * dz
                if d2 <= r2:
                    tmp.append((d2, (dx + 128) | ((dy + 128) << 8) | ((dz + 128) << 16), (dx, dy, dz)))
    return [t[2] for t in sorted(tmp)]


def _unit(origin, axis, flip, offset, signs=(1, 1)):
    """one unit.  Local frame (n, s, t) = (axis, axis + 1, axis + 2): the layers' lattices run from origin's (s, t) in the directions
    `signs`, the hidden layer lies at origin's n, the front 7 before it as its plane sees it (flip: the plane axis + 3, seen from
    the high side).  offset: (dx, dy, dz) from the test point = the hidden point AT the origin to the column's first point; its
    component along the axis must not point towards the front.  -> (xyz [96][3], planes [96], index of the test point)"""
    away = -1 if flip else 1                                     # the direction from the front layer to the hidden one
    o = np.array([offset[axis], offset[(axis + 1) % 3], offset[(axis + 2) % 3]])
    assert o[0] * away >= 0 and (o != 0).any()
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    i, j = i.ravel(), j.ravel()
    front = np.stack([np.full(64, -7 * away), 4 * i * signs[0], 4 * j * signs[1]], 1)
    hid = (i % 2 == 0) & (j % 2 == 0)
    order = np.argsort(-(i[hid] + j[hid]), kind="stable")          # (the point at the origin last)
    hidden = np.stack([np.zeros(16, np.int64), 4 * i[hid] * signs[0], 4 * j[hid] * signs[1]], 1)[order]
    column = o[None, :] + np.stack([away * np.arange(16), np.zeros(16, np.int64), np.zeros(16, np.int64)], 1)
    local = np.concatenate([front, hidden, column])
    xyz = np.empty_like(local)
    for k in range(3):
        xyz[:, (axis + k) % 3] = local[:, k] + origin[(axis + k) % 3]
    planes = np.concatenate([np.full(80, axis + (3 if flip else 0)), np.full(16, (axis + 1) % 3)])
    return xyz, planes, 64 + 15


def probe_units():
    """-> (xyz int16, rgb uint8, partition uint32, units): units = [dict(offset, d2, index (of the table; None beyond it), test
    (the test point's index in the cloud), hidden (the sixteen indices of its layer))]"""
    table = probe_offsets()
    wanted = [(0, 0, 1), (1, 1, 0), (-1, -1, 1), (0, 2, 0), (-2, 1, 0), (1, 2, 1), (2, 0, 2), (0, 0, 3), (2, -2, 1),   # d2 = 1 2 3 4 5 6 8 9 9
              (1, 0, 3), (0, 4, 0)]                                                                                  # 10 and 16: beyond
    # and by index: the ends of the batches of eight behind the own voxel (8 | 9, 16 | 17, 24 | 25), of a batch of sixteen, the
    # first and last entries, and the short last batch (121, 122)
    for at in (1, 6, 7, 8, 9, 16, 17, 24, 25, 32, 33, 120, 121, 122):
        if table[at] not in wanted:
            wanted.append(table[at])
    xyz, part, units, at = [], [], [], 0
    for k, off in enumerate(wanted):
        axis = k % 3
        # (a column cannot start between the layers: the side the layers are seen from follows the offset's sign along the axis)
        flip = off[axis] < 0 or (off[axis] == 0 and k % 2 == 1)
        origin = [0, 0, 0]                                          # (the grid of units lies in the unit's own (s, t), at n = 140)
        origin[axis], origin[(axis + 1) % 3], origin[(axis + 2) % 3] = 140, 230 + 72 * (k % 6), 230 + 72 * (k // 6)
        signs = (1, 1)
        if k == 0:      # the cube's low corner: probes at -1 in the lattice's directions
            origin[(axis + 1) % 3] = origin[(axis + 2) % 3] = 0
        if k == 1:      # within 3 of two low faces
            origin[(axis + 1) % 3], origin[(axis + 2) % 3] = 2, 1
        if k == 2:      # the high corner of a 10-bit cube (the bitmap's side is the next power of two above the largest coordinate)
            origin[(axis + 1) % 3] = origin[(axis + 2) % 3] = 1023
            signs = (-1, -1)
        u, p, test = _unit(origin, axis, flip, off, signs)
        xyz.append(u), part.append(p)
        d2 = sum(c * c for c in off)
        units.append(dict(offset=off, d2=d2, index=table.index(off) if off in table else None, test=at + test,
                          hidden=list(range(at + 64, at + 80))))
        at += len(u)
    xyz = np.concatenate(xyz)
    assert xyz.min() >= 0 and xyz.max() == 1023 and len(np.unique(xyz, axis=0)) == len(xyz)
    rng = np.random.default_rng(7)
    rgb = (100 + rng.integers(0, 20, (len(xyz), 3))).astype(np.uint8)
    return xyz.astype(np.int16), rgb, np.concatenate(part).astype(np.uint32), units


def stack(counts, axis=2, side=24, stride=4, gap=7, base=40):
    """Sheets of one component stacked `gap` apart along `axis` (farther than surfaceThickness plus the selection radius), all given
    the plane `axis`: counts[0] is ignored (the first sheet is side x side points), counts[s] points of sheet s lie opposite points
    of the sheet before.  Round r's depth map keeps sheet r - 1, and the list of round r + 1 is what lies behind it:
    sum(counts[r:]) points.  Interleaved index order as patch_round_cases.slab."""
    a, b = np.meshgrid(np.arange(side) * stride + base, np.arange(side) * stride + base, indexing="ij")
    a, b = a.ravel(), b.ravel()
    # sheets behind the first: the middle of the lattice outwards, so that a short sheet is a compact blob
    order = np.argsort((a - a.mean()) ** 2 + (b - b.mean()) ** 2, kind="stable")
    sheets = [np.stack([np.full(a.size, base), a, b], 1)]
    for s, m in enumerate(counts[1:], 1):
        assert m <= a.size
        sheets.append(np.stack([np.full(m, base + s * gap), a[order[:m]], b[order[:m]]], 1))
    pts = np.concatenate(sheets)
    xyz = np.empty_like(pts)
    xyz[:, axis], xyz[:, (axis + 1) % 3], xyz[:, (axis + 2) % 3] = pts[:, 0], pts[:, 1], pts[:, 2]
    rng = np.random.default_rng(sum(counts) + axis)
    perm = rng.permutation(len(xyz))
    rgb = (100 + rng.integers(0, 20, (len(xyz), 3))).astype(np.uint8)
    return xyz[perm].astype(np.int16), rgb, np.full(len(xyz), axis, np.uint32)


def chain(groups=12, members=12, first_gap=100.0, ratio=0.8):
    """A string of groups joined only by one-way edges: flat clumps of `members` (< 17) points in one plane along x, the gap to the
    next clump shrinking by `ratio`.  A point lists its own clump (mutual edges: one union-find group) and fills its row from the
    nearest other clump -- the NEXT one, whose own rows in turn point onwards: edges from clump g to clump g + 1 only, until the
    last two, which list each other.  Indices ascend along the string, so the label of clump 0 has to travel all the way: one hop
    per relaxation sweep."""
    xyz, x = [], 10
    gap = first_gap
    for g in range(groups):
        i = np.arange(members)
        xyz.append(np.stack([x + i % 4, 500 + i // 4, np.full(members, 300)], 1))
        x += 4 + int(round(gap))
        gap *= ratio
    xyz = np.concatenate(xyz).astype(np.int16)
    rng = np.random.default_rng(groups)
    return xyz, (100 + rng.integers(0, 20, (len(xyz), 3))).astype(np.uint8), np.full(len(xyz), 2, np.uint32)


def islands():
    """The shapes of a row's mutual mask: a clump of exactly 17 points on its own (every point lists the other sixteen and is
    listed by them: mask all ones); a big dense sheet with single points hovering far over it (a hoverer lists sixteen sheet
    points, none lists it: mask 0, a component of one); everything in one plane."""
    a, b = np.meshgrid(np.arange(24) + 200, np.arange(24) + 200, indexing="ij")
    sheet = np.stack([a.ravel(), b.ravel(), np.full(a.size, 50)], 1)
    # (12 over the sheet: the sixteenth sheet point is nearer than the next hoverer, 17 away)
    hover = np.array([[203, 203, 62], [220, 220, 62], [203, 220, 62], [220, 203, 62]])
    i = np.arange(17)
    clump = np.stack([700 + i % 5, 700 + i // 5, np.full(17, 50)], 1)
    xyz = np.concatenate([sheet, hover, clump]).astype(np.int16)
    rng = np.random.default_rng(17)
    return xyz, (100 + rng.integers(0, 20, (len(xyz), 3))).astype(np.uint8), np.full(len(xyz), 2, np.uint32)


def lattice(n, width=16):
    """n points of a flat lattice, `width` to a row: one component, one patch (n >= 17: a row needs sixteen OTHER points)"""
    i = np.arange(n)
    xyz = np.stack([30 + i % width, 30 + i // width, np.full(n, 30)], 1).astype(np.int16)
    rng = np.random.default_rng(n)
    return xyz, (100 + rng.integers(0, 20, (n, 3))).astype(np.uint8), np.full(n, 2, np.uint32)
