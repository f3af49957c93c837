"""Hand-built decoder frames and plain references for the decoder-side path (tmc2_decoder_frame_create ->
tmc2_codec_generate_point_cloud -> ... -> tmc2_codec_convert_yuv16_to_rgb8): patch records, an occupancy video and two geometry maps
as a bitstream delivers them, NOT what this project's encoder makes of a smooth cloud.  numpy only, deterministic from a seed.

A scene is a dict: name, note (the condition it exists for), patches (PATCH_DTYPE, list order), W, H, prec, occ_video
u8 [H/prec][W/prec], geo0 / geo1 u16 [H][W].  Every reconstructed coordinate lies in [0, 2^11): int16 never wraps.

The references are written from the reference's text (PccLibCommon/source/PCCCodec.cpp), not from the kernels:
    block_to_patch           generateBlockToPatchFromOccupancyMapVideo :1736-1775
    generate_point_cloud     generatePointCloud :519-980, lossy two-map branch, with generatePoints :499-516 (absoluteD1) and
                             PCCPatch::generatePoint / generateNormalCoordinate (PCCPatch.h:177-207)
    identify_boundary_points :268-327, as :955-976 runs it on the upsampled occupancy video
    partition_of             the patch (list position) that emitted a point
    blend_counts             the integer count of gridFiltering's trilinear blend (:1002-1065): how many boundary points reach
                             the 0 / 0 -> NaN -> "not moved" path
T3, T4 and the conversion to RGB keep the oracle's orc_* functions as their reference (tests/test_decoder_frame_cases.py pins those
to the unmodified reference on these scenes).  tests/test_decoder_frame_cases.py asserts every scene's condition from the
references alone; tests/test_gpu_decoder_frames.py compares the device with them, integer for integer."""
import functools

import numpy as np

from oracle_binding import PATCH_DTYPE

AXES = {0: (2, 1), 1: (2, 0), 2: (0, 1)}          # normal axis -> (tangent, bitangent), PCCPatch::setViewId
PAIRS = ((8, 64.0), (16, 8.0), (2, 0.0), (64, 64.0), (8, 1e9))      # (gridSize, thresholdSmoothing) of T3 / T4


# ---- building a scene ---------------------------------------------------------------------------------------------------
def _scene(name, W, H, prec, note):
    assert W % 16 == 0 and H % 16 == 0 and 16 % prec == 0
    return dict(name=name, note=note, W=W, H=H, prec=prec, patches=[], occ_video=np.zeros((H // prec, W // prec), np.uint8),
                geo0=np.zeros((H, W), np.uint16), geo1=np.zeros((H, W), np.uint16))


def _canvas_xy(p):
    """canvas (X, Y) of every patch pixel, arrays [sizeV0*16][sizeU0*16] indexed (v, u): PCCPatch::patch2Canvas, orientations 0 / 1"""
    v, u = np.mgrid[0:p["sizeV0"] * 16, 0:p["sizeU0"] * 16]
    if p["patchOrientation"] == 0:
        return u + p["u0"] * 16, v + p["v0"] * 16
    return v + p["u0"] * 16, u + p["v0"] * 16


def _add(s, u0, v0, su0, sv0, orient=0, axis=2, mode=0, u1=0, v1=0, d1=0, mask=None, depth0=0, depth1=None):
    """One patch record at the end of the list, painted into the canvases: mask / depth0 / depth1 are [sv0*16][su0*16] in (v, u) (or
    scalars).  The occupancy video takes the OR of the mask over each prec x prec cell; the geometry is written for the whole box."""
    p = np.zeros((), PATCH_DTYPE)
    p["index"] = len(s["patches"])
    p["normalAxis"], (p["tangentAxis"], p["bitangentAxis"]) = axis, AXES[axis]
    p["viewId"] = axis + 3 * mode
    p["projectionMode"], p["patchOrientation"] = mode, orient
    p["u0"], p["v0"], p["sizeU0"], p["sizeV0"] = u0, v0, su0, sv0
    p["u1"], p["v1"], p["d1"] = u1, v1, d1
    p["sizeU"], p["sizeV"] = su0 * 16, sv0 * 16
    p["size2DXInPixel"], p["size2DYInPixel"] = su0 * 16, sv0 * 16
    bw, bh = (su0, sv0) if orient == 0 else (sv0, su0)
    assert 0 <= u0 and 0 <= v0 and (u0 + bw) * 16 <= s["W"] and (v0 + bh) * 16 <= s["H"], "patch outside the canvas"
    shape = (sv0 * 16, su0 * 16)
    m = np.broadcast_to(np.ones(shape, bool) if mask is None else np.asarray(mask, bool), shape)
    a = np.broadcast_to(np.asarray(depth0), shape)
    b = a if depth1 is None else np.broadcast_to(np.asarray(depth1), shape)
    assert a.min() >= 0 and b.min() >= 0
    X, Y = _canvas_xy(p)
    s["geo0"][Y, X], s["geo1"][Y, X] = a, b
    s["occ_video"][Y[m] // s["prec"], X[m] // s["prec"]] = 1
    s["patches"].append(p)
    return p


def _finish(s):
    s["patches"] = np.array(s["patches"], dtype=PATCH_DTYPE) if s["patches"] else np.zeros(0, PATCH_DTYPE)
    s["geometry"] = np.stack([s["geo0"], s["geo1"]])
    return s


def _uv(su0, sv0):
    v, u = np.mgrid[0:sv0 * 16, 0:su0 * 16]
    return u, v


def _blob(rng, su0, sv0, discs=3, holes=2):
    """a union of discs minus a few small ones: an irregular outline with holes, in (v, u)"""
    u, v = _uv(su0, sv0)
    w, h = su0 * 16, sv0 * 16
    m = np.zeros((h, w), bool)
    for _ in range(discs):
        cu, cv, r = rng.integers(0, w), rng.integers(0, h), rng.integers(5, max(7, min(w, h)))
        m |= (u - cu) ** 2 + (v - cv) ** 2 <= r * r
    for _ in range(holes):
        cu, cv, r = rng.integers(0, w), rng.integers(0, h), rng.integers(1, 4)
        m &= (u - cu) ** 2 + (v - cv) ** 2 > r * r
    if not m.any():
        m[h // 2, w // 2] = True
    return m


def _surface(rng, su0, sv0, base, rough=2):
    """depth0 = a tilted plane + noise, depth1 = depth0 + 0..3 (0: the D1 point is dropped)"""
    u, v = _uv(su0, sv0)
    a, b = rng.integers(-3, 4, 2)
    d0 = base + (a * u + b * v) // 8 + rng.integers(0, rough + 1, u.shape)
    d0 = np.maximum(d0, 0)
    return d0, d0 + rng.integers(0, 4, u.shape) * (rng.random(u.shape) < 0.7)


# ---- the references -------------------------------------------------------------------------------------------------------
def block_to_patch(s):
    """:1736-1775: patches in list order; every block of the patch (v0-major, u0) with any occupied sample takes patchIndex + 1, so
    the LAST patch whose oriented box covers an occupied block owns it"""
    W, H, prec = s["W"], s["H"], s["prec"]
    Wb, Hb, c = W // 16, H // 16, 16 // prec
    occupied = (s["occ_video"] != 0).reshape(Hb, c, Wb, c).any(axis=(1, 3))
    out = np.zeros((Hb, Wb), np.uint32)
    for k, p in enumerate(s["patches"]):
        for vb in range(p["sizeV0"]):
            for ub in range(p["sizeU0"]):
                bx, by = (ub + p["u0"], vb + p["v0"]) if p["patchOrientation"] == 0 else (vb + p["u0"], ub + p["v0"])
                if occupied[by, bx]:
                    out[by, bx] = k + 1
    return out


def generate_point_cloud(s, b2p=None):
    """:519-980 -> (xyz i16 [M][3], point_to_pixel u32 [M][3] = (x, y, layer), points per patch)"""
    W, prec, geo0, geo1, ov = s["W"], s["prec"], s["geo0"].astype(np.int64), s["geo1"].astype(np.int64), s["occ_video"]
    b2p = block_to_patch(s) if b2p is None else b2p
    j, i = np.mgrid[0:16, 0:16]                                          # v1-major, then u1
    xyz, p2p, per_patch = [], [], []
    for k, p in enumerate(s["patches"]):
        emitted = 0
        for vb in range(p["sizeV0"]):
            for ub in range(p["sizeU0"]):
                bx, by = (ub + p["u0"], vb + p["v0"]) if p["patchOrientation"] == 0 else (vb + p["u0"], ub + p["v0"])
                if b2p[by, bx] != k + 1:
                    continue
                u, v = (ub * 16 + i).ravel(), (vb * 16 + j).ravel()
                x, y = (u + p["u0"] * 16, v + p["v0"] * 16) if p["patchOrientation"] == 0 else (v + p["u0"] * 16, u + p["v0"] * 16)
                occ = ov[y // prec, x // prec] != 0
                pts = np.zeros((256, 2, 3), np.int64)
                for layer, g in enumerate((geo0, geo1)):
                    depth = g[y, x]
                    pts[:, layer, p["normalAxis"]] = depth + p["d1"] if p["projectionMode"] == 0 else np.maximum(0, p["d1"] - depth)
                    pts[:, layer, p["tangentAxis"]] = u + p["u1"]
                    pts[:, layer, p["bitangentAxis"]] = v + p["v1"]
                keep = np.stack([occ, occ & (pts[:, 1] != pts[:, 0]).any(axis=1)], axis=1)      # removeDuplicatePoints: D1 == D0 dropped
                pix = np.stack([np.stack([x, y, np.full(256, layer)], axis=1) for layer in (0, 1)], axis=1)
                xyz.append(pts[keep])
                p2p.append(pix[keep])
                emitted += int(keep.sum())
        per_patch.append(emitted)
    if not xyz:
        return np.zeros((0, 3), np.int16), np.zeros((0, 3), np.uint32), np.array(per_patch, np.int64)
    xyz = np.concatenate(xyz)
    assert len(xyz) == 0 or (xyz.min() >= 0 and xyz.max() < 2048), "a scene must keep its coordinates in [0, 2^11)"
    return xyz.astype(np.int16), np.concatenate(p2p).astype(np.uint32), np.array(per_patch, np.int64)


def identify_boundary_points(p2p, occ_video, W, H, prec):
    """:268-327 on the occupancy video upsampled by prec (:558-572): u16 [M], 0 or 1"""
    occ = np.repeat(np.repeat(occ_video != 0, prec, axis=0), prec, axis=1)
    x, y = p2p[:, 0].astype(np.int64), p2p[:, 1].astype(np.int64)

    def empty(dx, dy):                                                    # the pixel at (x + dx, y + dy) lies in the image and is 0
        xx, yy = x + dx, y + dy
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return ok & ~occ[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    ymid, xmid = (y > 0) & (y < H - 1), (x > 0) & (x < W - 1)
    t = ymid & (empty(0, -1) | empty(0, 1))
    t |= xmid & (empty(1, 0) | empty(-1, 0))
    t |= ymid & (x > 0) & (empty(-1, -1) | empty(-1, 1))
    t |= ymid & (x < W - 1) & (empty(1, -1) | empty(1, 1))
    t |= (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)
    for ix in range(-2, 3):                                               # second layer: the ring at distance two
        for iy in range(-2, 3):
            if abs(ix) > 1 or abs(iy) > 1:
                t |= empty(ix, iy)
    t |= (y == 1) | (y == H - 2) | (x == 1) | (x == W - 2)
    return (t & occ[y, x]).astype(np.uint16)


def partition_of(p2p, b2p):
    return (b2p[p2p[:, 1] // 16, p2p[:, 0] // 16] - 1).astype(np.uint32)


def grid_geometry(xyz, grid):
    """(w, th, disth) of T3's grid over [0, max coordinate] (:67-75)"""
    w = (int(xyz.max()) + grid - 1) // grid
    return w, grid * w, max(grid // 2, 1)


def outside(xyz, grid):
    w, th, disth = grid_geometry(xyz, grid)
    P = xyz.astype(np.int64)
    return ((P < disth) | (th <= P + disth)).any(axis=1)


def blend_counts(xyz, btype, grid, partition):
    """The blended count (sum of weight * cell count over the 2x2x2 cells, // (2 grid)^3) of every boundary point inside the faces
    -> (indices of those points, their counts, armed: one of the eight cells holds points of two patches, so the blend is computed
    at all).  An armed count of 0 is the 0 / 0 -> NaN -> "not moved" path.  (64-bit here: the reference's int wraps beyond an
    average of 1023 points per cell at grid 64, which no scene that reads this function reaches.)"""
    assert grid % 2 == 0
    w, th, disth = grid_geometry(xyz, grid)
    P = xyz.astype(np.int64)
    inside = ~outside(xyz, grid)
    cell = P // grid
    keys = (cell[:, 2] * w + cell[:, 1]) * w + cell[:, 0]
    names, index = np.unique(keys[inside], return_inverse=True)      # (w^3 reaches 2^30 at grid 2: the occupied cells only)
    index = index.ravel()
    counts = np.zeros(len(names), np.int64)
    np.add.at(counts, index, 1)
    lo, hi = np.full(len(names), 1 << 40, np.int64), np.full(len(names), -1, np.int64)
    np.minimum.at(lo, index, partition[inside].astype(np.int64))
    np.maximum.at(hi, index, partition[inside].astype(np.int64))
    who = np.flatnonzero(inside & (btype == 1))
    Q, half = P[who], grid // 2
    S = Q // grid - ((Q % grid) < half)
    Wt = (Q - S * grid - half) * 2 + 1
    total, armed = np.zeros(len(who), np.int64), np.zeros(len(who), bool)
    if len(names) == 0:
        return who, total, armed
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                d = np.array([dx, dy, dz])
                wgt = np.where(d, Wt, 2 * grid - Wt).prod(axis=1)
                c = S + d
                key = (c[:, 2] * w + c[:, 1]) * w + c[:, 0]
                at = np.clip(np.searchsorted(names, key), 0, len(names) - 1)
                hit = names[at] == key
                total += wgt * np.where(hit, counts[at], 0)
                armed |= hit & (lo[at] != hi[at])
    return who, total // (2 * grid) ** 3, armed


def references(s):
    """everything the tests compare with, computed once per scene"""
    b2p = block_to_patch(s)
    xyz, p2p, per_patch = generate_point_cloud(s, b2p)
    return dict(block_to_patch=b2p, xyz=xyz, point_to_pixel=p2p, per_patch=per_patch,
                boundary=identify_boundary_points(p2p, s["occ_video"], s["W"], s["H"], s["prec"]), partition=partition_of(p2p, b2p))


def attribute_planes(s, kind, seed=0):
    """decoded attribute frames u16 [2][3][H][W]: uniform random, or the eight corner colours over a grey ramp"""
    H, W = s["H"], s["W"]
    if kind == "random":
        return np.random.default_rng([seed, H, W]).integers(0, 65536, (2, 3, H, W), dtype=np.uint16)
    y, x = np.mgrid[0:H, 0:W]
    att = np.zeros((2, 3, H, W), np.uint16)
    corner = ((x // 4 + y // 4) % 8)
    ramp = ((x + y * W) * 65535 // max(W * H - 1, 1)).astype(np.uint16)
    for m in range(2):
        for c in range(3):
            bit = ((corner >> c) & 1).astype(np.uint16) * 65535
            att[m, c] = np.where((y // 8 + m) % 2 == 0, bit, ramp)
    return att


# ---- the scenes -------------------------------------------------------------------------------------------------------
def borders():
    s = _scene("borders", 64, 48, 4, "patches on all four canvas edges and corners, both orientations: points with x < 2, y < 2, "
               "x >= W - 2, y >= H - 2")
    rng = np.random.default_rng(101)
    # (u0, v0, sizeU0, sizeV0, orientation): the corner and edge blocks, the right column (3 x 1 turned), the bottom row (1 x 3 turned)
    for k, (u0, v0, su, sv, o) in enumerate(((0, 0, 1, 1, 0), (1, 0, 2, 1, 0), (0, 1, 1, 1, 1), (1, 1, 2, 1, 0), (3, 0, 3, 1, 1),
                                             (0, 2, 1, 3, 1))):
        d0, d1 = _surface(rng, su, sv, 40 + 3 * k)
        X, Y = (u0 * 16, v0 * 16)
        _add(s, u0, v0, su, sv, o, 2, 0, 30 + (X if o == 0 else Y), 30 + (Y if o == 0 else X), 0, None, d0, d1)
    return _finish(s)


def overlap():
    s = _scene("overlap", 64, 64, 4, "overlapping boxes: a shared occupied block goes to the later patch; one patch owns none of its "
               "blocks, one has empty occupancy: patches with 0 points between patches with points")
    rng = np.random.default_rng(102)
    full = None
    for u0, v0, su, sv, o, mask in ((0, 0, 2, 2, 0, full), (3, 0, 1, 2, 0, full), (1, 1, 2, 2, 1, full), (0, 3, 2, 1, 0, False),
                                    (3, 0, 3, 1, 1, full)):
        d0, d1 = _surface(rng, su, sv, 36 + 2 * len(s["patches"]))
        _add(s, u0, v0, su, sv, o, 2, 0, 24 + u0 * 12, 24 + v0 * 12, 0, mask, d0, d1)
    return _finish(s)


def axes():
    s = _scene("axes", 64, 64, 4, "the three normal axes x both projection modes, and mode 1 with depth > d1 on both layers (both "
               "clamp to 0: one point)")
    rng = np.random.default_rng(103)
    k = 0
    for axis in (0, 1, 2):
        for mode in (0, 1):
            d0, d1 = _surface(rng, 1, 1, 6)
            # the six faces of a small box around (48, 48, 48): mode 0 rises from d1 = 38, mode 1 falls from d1 = 70
            _add(s, k % 4, k // 4, 1, 1, k % 2, axis, mode, 40, 40, 38 if mode == 0 else 70, _blob(rng, 1, 1, 4, 1), d0, d1)
            k += 1
    u, v = _uv(2, 1)
    _add(s, 2, 1, 2, 1, 0, 2, 1, 40, 56, 10, None, 11 + (u + v) % 5, 13 + (u * v) % 7)      # d1 - depth < 0 on both layers
    return _finish(s)


LAYER_LANES = (0, 63, 64, 255)


def layers():
    s = _scene("layers", 64, 48, 1, "the per-tile 256-lane scan and the cross-wave offsets: a tile of 512 points, one with D1 = D0, "
               "one with D1 < D0, tiles with one pixel at lane 0 / 63 / 64 / 255, an empty tile")
    rng = np.random.default_rng(104)
    u, v = _uv(4, 2)
    tile = (v // 16) * 4 + u // 16
    lane = (v % 16) * 16 + u % 16
    mask = tile < 3
    for t, l in zip((3, 4, 5, 6), LAYER_LANES):
        mask |= (tile == t) & (lane == l)                           # (tile 7 stays empty)
    d0 = 20 + rng.integers(0, 3, u.shape)
    d1 = np.where(tile == 0, d0 + 1 + rng.integers(0, 3, u.shape), np.where(tile == 2, d0 - 1 - rng.integers(0, 3, u.shape), d0))
    d1 = np.where(tile >= 3, d0 + (lane % 2), d1)
    _add(s, 0, 0, 4, 2, 0, 2, 0, 32, 32, 10, mask, d0, d1)
    e0, e1 = _surface(rng, 1, 2, 27)
    _add(s, 1, 2, 1, 2, 1, 2, 0, 36, 34, 0, _blob(rng, 1, 2), e0, e1)      # a second patch through the first one's cells
    return _finish(s)


PRECISIONS = (1, 2, 4, 8, 16)


def precisions(prec):
    s = _scene("precisions-%d" % prec, 64, 64, prec, "one patch list at occupancy precision 1, 2, 4, 8, 16")
    rng = np.random.default_rng(105)                               # (the same draws at every precision)
    for u0, v0, su, sv, o, axis, mode in ((0, 0, 2, 2, 0, 2, 0), (2, 0, 2, 2, 1, 0, 0), (0, 2, 2, 1, 0, 1, 1), (2, 2, 1, 2, 1, 2, 1),
                                          (0, 3, 2, 1, 0, 0, 0)):
        d0, d1 = _surface(rng, su, sv, 8)
        _add(s, u0, v0, su, sv, o, axis, mode, 40, 40, 36 if mode == 0 else 72, _blob(rng, su, sv, 3, 3), d0, d1)
    return _finish(s)


def coincident():
    s = _scene("coincident", 64, 48, 2, "three patches reconstruct the same 3-D points: exact duplicates and distance ties for "
               "T4's searches, every cell sees several patches")
    rng = np.random.default_rng(106)
    mask = _blob(rng, 2, 1, 4, 2)
    u, v = _uv(2, 1)
    d0 = 30 + rng.integers(0, 9, u.shape)                          # rough: the cell centroids pull
    d1 = d0 + rng.integers(0, 3, u.shape)
    for u0, v0, o in ((0, 0, 0), (2, 0, 0), (0, 1, 1)):
        _add(s, u0, v0, 2, 1, o, 2, 0, 40, 40, 4, mask, d0, d1)
    f0, f1 = _surface(rng, 1, 1, 28, 6)
    _add(s, 2, 1, 1, 1, 0, 2, 0, 44, 40, 8, _blob(rng, 1, 1), f0, f1)
    return _finish(s)


FACE_GRIDS, FACE_VARIANTS, FACE_TH = (2, 8, 64), (-1, 0, 1), 128


def face_targets(grid, variant):
    """(max coordinate, the four face coordinates disth-1, disth, th-disth-1, th-disth that lie in [0, max]); max = k grid + variant
    with k grid = 128, so w and th change with the variant.  Beyond k grid the grid grows by a cell and th - disth - 1 leaves
    [0, max] for grid >= 4: such a coordinate cannot hold a point and is not a target."""
    top = FACE_TH + variant
    w = (top + grid - 1) // grid
    th, disth = grid * w, max(grid // 2, 1)
    return top, [c for c in (disth - 1, disth, th - disth - 1, th - disth) if 0 <= c <= top]


def faces(grid, variant):
    top, targets = face_targets(grid, variant)
    s = _scene("faces-g%d-%+d" % (grid, variant), 64, 64, 1, "per axis boundary points at disth-1, disth, th-disth-1, th-disth for "
               "grid %d with max coordinate %d" % (grid, top))
    rng = np.random.default_rng([107, grid, variant + 1])
    u, v = _uv(1, 1)
    stripes = (u + 2 * v) % 3 != 2                                  # every occupied pixel has an empty one next to it: all boundary
    k = 0
    for axis in (0, 1, 2):
        for c in targets:
            # D0 at c; D1 at c - 1, c or c + 1 (inside [0, top]): the patches of neighbouring targets share cells
            d1 = 1 + rng.integers(-1, 2, u.shape)
            d1 = np.clip(d1, max(0, 1 - c), top - (c - 1))
            _add(s, k % 4, k // 4, 1, 1, k % 2, axis, 0, 56, 56, c - 1, stripes, 1, d1)
            k += 1
    pin = np.zeros(u.shape, bool)
    pin[7, 7] = True
    _add(s, k % 4, k // 4, 1, 1, 0, 2, 0, 56, 56, top - 1, pin, 1, 1)         # one point at the max coordinate
    return _finish(s)


def single(small=False):
    if small:
        s = _scene("single-small", 64, 48, 1, "one patch of fewer than 8 points: nothing moves, the tail still completes")
        m = np.zeros((16, 16), bool)
        m[3, 4] = m[3, 5] = m[4, 4] = m[9, 12] = m[15, 15] = True
        _add(s, 2, 1, 1, 1, 0, 2, 0, 40, 40, 30, m, 5, 5)
        return _finish(s)
    s = _scene("single", 64, 48, 4, "one patch: no cell sees a second patch, nothing moves, T4 returns at K = 0")
    rng = np.random.default_rng(108)
    d0, d1 = _surface(rng, 2, 2, 30, 8)
    _add(s, 1, 0, 2, 2, 0, 2, 0, 40, 40, 10, _blob(rng, 2, 2, 4, 3), d0, d1)
    return _finish(s)


def sparse():
    s = _scene("sparse", 128, 64, 1, "two 3-D-adjacent patches of isolated 2-3-pixel islands: blended counts of 0 at grid 16")
    u, v = _uv(4, 4)
    # islands at the corners of every other grid-16 cell (x = 48 or 80 + 0..3, y = 48 or 80, z = 48 or 49): the own cell weighs from
    # (17 / 32)^3 to 23 * 17 * 19 / 32^3 = 0.23 and holds the four points of both patches' islands (six at the last corner: some
    # counts there reach 1), the other seven cells are empty
    for k in range(2):
        m = np.zeros(u.shape, bool)
        for cv in (8, 40):
            for cu in (8, 40):
                m[cv, cu] = m[cv, cu + 1] = True
        m[41, 40] = True
        _add(s, 4 * k, 0, 4, 4, k, 2, 0, 40 + 2 * k, 40, 46 + k, m, 2, None)
    return _finish(s)


RANDOM_CANVASES = ((64, 48, 4), (96, 64, 2), (64, 64, 1), (128, 48, 8), (64, 64, 16))
# twelve seeds per canvas, chosen so that the oracle alone moves at least 20 points of every scene at (16, 8.0) (seed 2 on the last
# canvas moves none there: 12 stands in for it)
RANDOM_SEEDS = (tuple(range(12)),) * 4 + ((0, 1, 12, 3, 4, 5, 6, 7, 8, 9, 10, 11),)


def random_scene(seed, config):
    W, H, prec = RANDOM_CANVASES[config]
    s = _scene("random-%d-%dx%d-p%d" % (seed, W, H, prec), W, H, prec, "five random patches")
    rng = np.random.default_rng([110, seed, config])
    Wb, Hb = W // 16, H // 16
    for _ in range(5):
        o = int(rng.integers(0, 2))
        bw, bh = int(rng.integers(1, min(3, Wb) + 1)), int(rng.integers(1, min(2, Hb) + 1))
        su, sv = (bw, bh) if o == 0 else (bh, bw)
        u0, v0 = int(rng.integers(0, Wb - bw + 1)), int(rng.integers(0, Hb - bh + 1))
        axis, mode = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        d0, d1 = _surface(rng, su, sv, int(rng.integers(4, 12)), int(rng.integers(0, 5)))
        if rng.random() < 0.3:                                    # decoded noise: D1 below D0 here and there
            d1 = np.maximum(0, d1 - 2 * (rng.random(d1.shape) < 0.2))
        _add(s, u0, v0, su, sv, o, axis, mode, int(rng.integers(30, 50)), int(rng.integers(30, 50)),
             int(rng.integers(30, 44)) if mode == 0 else int(rng.integers(64, 80)), _blob(rng, su, sv, 3, 3), d0, d1)
    return _finish(s)


def cell_overflow(large=False):
    """Refusals: one grid-64 cell whose coordinate sum passes 2^24 (17 blocks of 512 points around 2000), or whose count passes
    65535 (256 blocks of 512 points)."""
    n, side = (256, 256) if large else (17, 96)
    s = _scene("cell-overflow-%s" % ("count" if large else "sum"), side, side if large else 64, 4,
               "one grid-64 cell with %s" % ("more than 65535 points" if large else "a coordinate sum beyond 2^24"))
    base = 70 if large else 1990                                    # [64, 128) at th = 128 / [1984, 2048) at th = 2048: inside the faces
    Wb = side // 16
    u, v = _uv(1, 1)
    for k in range(n):
        _add(s, k % Wb, k // Wb, 1, 1, 0, 2, 0, base, base, base + k % 8, None, 0, 1 + (u + v + k) % 2)
    return _finish(s)


def _registry():
    r = {"borders": borders, "overlap": overlap, "axes": axes, "layers": layers, "coincident": coincident, "single": single,
         "single-small": functools.partial(single, True), "sparse": sparse}
    for p in PRECISIONS:
        r["precisions-%d" % p] = functools.partial(precisions, p)
    for g in FACE_GRIDS:
        for var in FACE_VARIANTS:
            r["faces-g%d-%+d" % (g, var)] = functools.partial(faces, g, var)
    for c in range(len(RANDOM_CANVASES)):
        for seed in RANDOM_SEEDS[c]:
            W, H, prec = RANDOM_CANVASES[c]
            r["random-%d-%dx%d-p%d" % (seed, W, H, prec)] = functools.partial(random_scene, seed, c)
    return r


BUILDERS = _registry()
NAMES = tuple(BUILDERS)
RANDOM_NAMES = tuple(n for n in NAMES if n.startswith("random-"))
# what the oracle alone must do at the (grid, threshold) pairs: "moves" = at least 20 points, "still" = exactly 0.  Nothing moves
# at a threshold of 1e9 anywhere, nor where no cell sees a second patch.
STILL_EVERYWHERE = ("single", "single-small")
OVERFLOW_NAMES = ("cell-overflow-sum", "cell-overflow-count")      # refused by the library: built by cell_overflow(), in no list above


def expectation(name, pair):
    """"moves", "still" or None (the scene was not built with that pair in mind: compared, not counted)"""
    if pair[1] >= 1e9 or name in STILL_EVERYWHERE:
        return "still"
    family = name.split("-")[0]
    if pair == (16, 8.0) and family in ("borders", "overlap", "axes", "layers", "coincident", "precisions", "random"):
        return "moves"
    if pair == (8, 64.0) and (family in ("borders", "overlap", "axes", "layers", "coincident", "precisions") or name.startswith("faces-g8")):
        return "moves"
    if pair == (64, 64.0) and (family in ("borders", "overlap", "axes", "coincident", "precisions") or name.startswith("faces-g64")):
        return "moves"
    return None


@functools.lru_cache(maxsize=None)
def scene(name):
    s = cell_overflow(name.endswith("count")) if name in OVERFLOW_NAMES else BUILDERS[name]()
    assert s["name"] == name
    return s


@functools.lru_cache(maxsize=None)
def scene_references(name):
    return references(scene(name))
