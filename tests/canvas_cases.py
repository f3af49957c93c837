"""Hand-built scenes for the encoder's canvases (S11-S16 in csrc/images.hip, S20-S22 in csrc/attributes.hip): flat sheets whose
occupancy is known by construction, placed on the canvas by hand, rasterised on a canvas size the caller chooses.  Pure numpy,
deterministic from a seed; used by test_canvas_cases.py (CPU tier: the scenes are what they claim) and test_gpu_canvases.py.

The route: a cloud of axis-aligned sheets + a partition that names each sheet's axis -> segmentPatches makes one patch per sheet
(box = the mask's box, d0Count = the mask's population) -> Scene.place() writes u0 / v0 / patchOrientation into the records
(tmc2_frame_set_packing) -> tmc2_encoder_generate_geometry_images( f, W, H, precision ) with the scene's W x H.

Canvases whose sides are both multiples of 64 are sizes PCCEncoder::resizeGeometryVideo can make; on those the oracle is pinned to
the unmodified reference (test_canvas_cases.py).  The canvases marked api_only (multiples of 16 only, and the two 16-wide strips of
25664) are sizes only the C-ABI reaches: there the oracle ALONE is the yardstick.

iters of level 0 over these canvases is at most 12 (pyramid()).  14..16 -- and with them the branch behind
`iters <= kPushPullMaxIters` in generateAttributeImages, which no iteration count can fail since the count is capped at 16 -- need a
canvas of more than 16384 pixels on its short side and stay untested.

The two strips 16 x 25664 and 25664 x 16 (no level of at most 160 x 160 pixels) take the oracle 0.06 s each on hand-placed records
(geometry, reconstruction, colours, attribute canvases), far below the 5 s at which they would have been left out; neither
checker's phase_a is ever run at such a size."""
import functools

import numpy as np

AXES = ((0, 2, 1), (1, 2, 0), (2, 0, 1))           # viewId % 3 -> (normal, tangent, bitangent) axes (PCCPatch::setViewId)
TILE, SMALL = 96, 160 * 160                        # kPushPullTile, kPushPullSmall (csrc/attributes.hip)


def pyramid(W, H):
    """The level rule of generateAttributeImages restated: level sizes, firstSmall (None: no level >= 1 is small, the coarse-levels
    kernel is not launched), blur iterations of level 0, fills done inside the coarse-levels kernel, tile counts of level 0."""
    levels = [(W, H)]
    while True:
        W, H = (W + 1) >> 1, (H + 1) >> 1
        levels.append((W, H))
        if W <= 4 or H <= 4:
            break
    small = [l for l in range(1, len(levels)) if levels[l][0] * levels[l][1] <= SMALL]
    first = small[0] if small else None
    coarse = 0 if first is None else len(levels) - 1 - first          # fills of levels first .. n - 2, 4 iterations at the coarsest
    return dict(levels=levels, first_small=first, iters0=min(4 + len(levels) - 2, 16), coarse_fills=coarse,
                tiles=(-(-levels[0][0] // TILE), -(-levels[0][1] // TILE)))


def _masks():
    m = {}
    m["full"] = np.ones((16, 16), bool)                                # a full block
    a = np.ones((16, 16), bool)
    a[5, 9] = False
    m["less1"] = a                                                     # ... less one pixel
    a = np.zeros((64, 64), bool)                                       # 4 x 4 blocks of ONE pixel each, in the corner (bx odd: right,
    for by in range(4):                                                # by odd: bottom): the block dilation's longest way, 30 levels
        for bx in range(4):
            a[by * 16 + 15 * (by & 1), bx * 16 + 15 * (bx & 1)] = True
    m["corners"] = a
    a = np.zeros((16, 16), bool)
    a[:2, :] = a[:, :2] = True
    m["ell"] = a                                                       # one row and one column of a block, two pixels thick
    v, u = np.indices((48, 48))
    m["checker"] = (u + v) % 2 == 0                                    # every empty pixel: rounded mean of four (of fewer at the rim)
    a = np.ones((48, 48), bool)
    a[16:32, 16:32] = False
    m["ring"] = a                                                      # the hole is one whole block
    m["w17"] = np.ones((16, 17), bool)                                 # the second block column holds one pixel column
    a = np.ones((24, 40), bool)                                        # the sloped sheet: 2.5 x 1.5 blocks, three bites out of it
    a[3:6, 34:38] = a[18:22, 4:9] = a[20:24, 36:40] = False
    m["slope"] = a
    return m


MASKS = _masks()
# mask -> (partition label = viewId, sheet number: where in space it lies, depth above the sheet's origin)
SHEETS = dict(full=(0, 0, 3), less1=(3, 1, 17), corners=(1, 2, 30), ell=(4, 3, 41), checker=(2, 4, 9), ring=(5, 5, 22), w17=(0, 6, 50),
              slope=(1, 7, 5))
ALL = tuple(MASKS)


def mask_key(name):
    """what a patch record shows of its mask: (normalAxis, sizeU, sizeV, d0Count), unique over MASKS"""
    m = MASKS[name]
    return (SHEETS[name][0] % 3, m.shape[1], m.shape[0], int(m.sum()))


@functools.lru_cache(maxsize=None)
def cloud(names, seed=20):
    """-> (xyz int16, rgb uint8, partition uint32) of the sheets `names`: sheet k lies at (100 k + 12) on every axis (at least 36 from
    the next on each), its first layer at a constant depth (the slope: + (u + v) // 5), a second layer 0..3 further along the
    projection at a colour within 60 of the first layer's (D1 takes a point only if its colour is within 128), points shuffled."""
    rng = np.random.default_rng(seed)
    pts, cols, part = [], [], []
    for name in names:
        label, k, depth = SHEETS[name]
        ax, direction = AXES[label % 3], 1 - 2 * (label // 3)
        v, u = np.nonzero(MASKS[name])
        d = np.full(len(u), depth) + ((u + v) // 5 if name == "slope" else 0)
        layer = rng.integers(0, 4, len(u))
        base = rng.integers(0, 256, (len(u), 3))
        second = np.clip(base + rng.integers(-60, 61, base.shape), 0, 255)
        for dd, c, keep in ((d, base, np.ones(len(u), bool)), (d + direction * layer, second, layer > 0)):
            p = np.zeros((int(keep.sum()), 3), np.int64)
            p[:, ax[0]], p[:, ax[1]], p[:, ax[2]] = dd[keep], u[keep], v[keep]
            pts.append(p + 100 * k + 12)
            cols.append(c[keep])
            part.append(np.full(len(p), label))
    xyz, rgb, part = np.concatenate(pts), np.concatenate(cols), np.concatenate(part)
    order = rng.permutation(len(xyz))
    return xyz[order].astype(np.int16), rgb[order].astype(np.uint8), part[order].astype(np.uint32)


class Scene:
    """placements: [(mask, u0, v0, patchOrientation)] or [(..., grow)] in LIST order, block units; grow = 1: the block box one block
    larger in U and in V than the mask needs (what the global patch allocation leaves: tiles wholly beyond sizeU / sizeV)."""

    def __init__(self, name, W, H, precision, placements, api_only=False):
        self.name, self.W, self.H, self.precision, self.api_only = name, W, H, precision, api_only
        self.placements = [tuple(p) + (0,) * (5 - len(p)) for p in placements]
        self.masks = tuple(n for n in ALL if any(p[0] == n for p in self.placements))
        assert len(self.masks) == len(self.placements)

    def __repr__(self):
        return self.name

    def cloud(self):
        return cloud(self.masks)

    @staticmethod
    def find(patches, name):
        """the patch made of sheet `name` (by its mask's key; the CPU tier asserts there is exactly one)"""
        got = [i for i, p in enumerate(patches) if (p["normalAxis"], p["sizeU"], p["sizeV"], p["d0Count"]) == mask_key(name)]
        assert len(got) == 1, (name, got)
        return got[0]

    def place(self, patches, occupancy):
        """records + block-occupancy pool as segmentation returned them -> (the list in list order with u0, v0, patchOrientation,
        index = list position and, for a grown box, sizeU0 / sizeV0; the pool rebuilt in list order)"""
        out = np.zeros(len(self.placements), patches.dtype)
        pool = []
        for k, (name, u0, v0, orient, grow) in enumerate(self.placements):
            p = patches[self.find(patches, name)].copy()
            su, sv = int(p["sizeU0"]), int(p["sizeV0"])
            occ = np.zeros((sv + grow, su + grow), np.uint8)
            occ[:sv, :su] = occupancy[p["occOffset"]:p["occOffset"] + su * sv].reshape(sv, su)
            p["sizeU0"], p["sizeV0"], p["u0"], p["v0"], p["patchOrientation"] = su + grow, sv + grow, u0, v0, orient
            p["index"], p["occOffset"] = k, len(pool)
            pool.extend(occ.ravel().tolist())
            out[k] = p
        return out, np.array(pool, np.uint8)

    def boxes(self):
        """per placement (x0, y0, width, height) of the block box on the canvas, in blocks"""
        out = []
        for name, u0, v0, orient, grow in self.placements:
            bu, bv = -(-MASKS[name].shape[1] // 16) + grow, -(-MASKS[name].shape[0] // 16) + grow
            out.append((u0, v0, bv, bu) if orient else (u0, v0, bu, bv))
        return out

    def painted(self):
        """per placement the mask as the raster must put it on the canvas (bool [H][W]); by construction, no checker involved"""
        out = []
        for name, u0, v0, orient, _ in self.placements:
            m = MASKS[name].T if orient else MASKS[name]
            a = np.zeros((self.H, self.W), bool)
            a[v0 * 16:v0 * 16 + m.shape[0], u0 * 16:u0 * 16 + m.shape[1]] = m
            out.append(a)
        return out


def _spread(Wb, Hb, grow_checker=0):
    """all eight masks on a canvas of at least 20 x 13 blocks: the corners of the canvas in both orientations, block (0,0) occupied,
    an occupied column-0 block (row 6) over a run of empty ones, block rows 4 and 5 empty, the block columns and rows either side
    of the tile seams x = 96 and y = 96 free (block row 5; block column 1 below row 3), a full block in the ring's hole (listed after it)"""
    rx, ry = max(8, Wb // 2), min(max(8, Hb // 2), Hb - 5)
    return [("corners", 0, 0, 0), ("less1", 0, 6, 0), ("checker", Wb - 3 - grow_checker, 0, 0, grow_checker), ("ring", rx, ry, 0),
            ("full", rx + 1, ry + 1, 1), ("slope", Wb - 2, Hb - 3, 1), ("w17", 0, Hb - 1, 0), ("ell", Wb // 2 - 2, Hb - 1, 1)]


def _every_mask(p):
    return Scene("every_mask_256x128_p%d" % p, 256, 128, p,
                 [("corners", 0, 0, 0), ("checker", 4, 0, 0), ("ring", 7, 0, 0), ("less1", 8, 1, 0), ("slope", 10, 0, 0), ("w17", 15, 0, 1),
                  ("ell", 10, 7, 1), ("full", 15, 7, 0)])


SCENES = [_every_mask(p) for p in (1, 2, 4, 8, 16)] + [
    Scene("origin_empty_64x64", 64, 64, 4, [("full", 0, 2, 0), ("w17", 1, 0, 0), ("ell", 3, 0, 1), ("less1", 3, 3, 1)]),
    # column 0 entirely empty; the full block sits in the ring's hole but is listed BEFORE the ring: the ring owns the block
    Scene("column0_empty_64x2048", 64, 2048, 4, [("checker", 1, 0, 0), ("full", 2, 61, 0), ("ring", 1, 60, 0), ("w17", 1, 100, 1),
                                                 ("less1", 3, 110, 0), ("slope", 2, 125, 1)]),
    Scene("strip_2048x64", 2048, 64, 4, [("corners", 0, 0, 0), ("ring", 60, 0, 0), ("less1", 61, 1, 0), ("slope", 100, 1, 1),
                                         ("checker", 125, 1, 0), ("ell", 127, 0, 0)]),
    Scene("two_by_two_tiles_192x192", 192, 192, 4, [("corners", 0, 0, 0), ("checker", 8, 0, 0), ("ring", 0, 8, 0), ("full", 1, 9, 0),
                                                    ("slope", 9, 10, 0)]),
    Scene("small_boundary_320x320", 320, 320, 4, _spread(20, 20, grow_checker=1)),
    Scene("above_small_384x320", 384, 320, 4, _spread(24, 20)),
    Scene("odd_seven_448x448", 448, 448, 4, _spread(28, 28)),
    Scene("odd_levels_1344x1344_p4", 1344, 1344, 4, _spread(84, 84)),
    Scene("odd_levels_1344x1344_p1", 1344, 1344, 1, _spread(84, 84)),
    Scene("api_1296x1328", 1296, 1328, 4, _spread(81, 83), api_only=True),
    Scene("api_336x208", 336, 208, 4, _spread(21, 13), api_only=True),
    Scene("api_112x80", 112, 80, 4, [("ring", 0, 0, 0), ("less1", 1, 1, 0), ("slope", 4, 0, 0), ("ell", 6, 4, 1), ("full", 0, 4, 0)],
          api_only=True),
    Scene("api_one_block_16x16", 16, 16, 4, [("ell", 0, 0, 0)], api_only=True),
    Scene("api_one_column_16x2048", 16, 2048, 4, [("less1", 0, 3, 0), ("w17", 0, 40, 1), ("ell", 0, 90, 1), ("full", 0, 127, 0)],
          api_only=True),
    # no level of at most 160 x 160 pixels (the coarsest, 4 x 6416, has 25664): every level goes through the tiles
    Scene("api_no_small_level_16x25664", 16, 25664, 4, [("less1", 0, 0, 0), ("w17", 0, 700, 1), ("ell", 0, 1000, 0), ("full", 0, 1603, 1)],
          api_only=True),
    Scene("api_no_small_level_25664x16", 25664, 16, 4, [("ell", 5, 0, 1), ("w17", 700, 0, 0), ("less1", 1000, 0, 0), ("full", 1603, 0, 0)],
          api_only=True),
]
BY_NAME = {s.name: s for s in SCENES}
# the canvases PCCEncoder::resizeGeometryVideo can make (both sides multiples of 64): minimumImageWidth / Height of the reference pin
REFERENCE_CANVASES = [(64, 64), (64, 2048), (2048, 64), (192, 192), (256, 128), (320, 320), (384, 320), (448, 448), (1344, 1344)]


def oracle_canvases(oracle, scene, params):
    """The oracle's whole answer for a scene, stage by stage on the placed records: -> dict(seg, list, pool, img (the five geometry
    canvases + patches / width / height), recon_xyz, recon_rgb, point_to_pixel, attribute)."""
    xyz, rgb, part = scene.cloud()
    seg = oracle.segment_patches(xyz, rgb, oracle.knn_self(xyz, 16), part, params)
    lst, pool = scene.place(seg["patches"], seg["occupancy"])
    img = oracle.geometry_images(lst, np.arange(len(lst), dtype=np.int32), seg["depth0"], seg["depth1"], scene.W, scene.H, 16,
                                 scene.precision)
    img.update(patches=lst, width=scene.W, height=scene.H)
    rec, p2p = oracle.generate_point_cloud(img)
    col = oracle.transfer_colors(xyz, rgb, rec)
    att = oracle.attribute_images(col, p2p, img["occ_video"], scene.W, scene.H, scene.precision)
    return dict(seg=seg, list=lst, pool=pool, img=img, recon_xyz=rec, recon_rgb=col, point_to_pixel=p2p, attribute=att)


def first_difference(stage, name, got, exp):
    """None, or where two canvases first differ: stage, plane, pixel, its 16 x 16 block and its 96 x 96 tile"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return "%s %s: shape %s, expected %s" % (stage, name, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    if not len(bad):
        return None
    at = tuple(int(i) for i in bad[0])
    y, x = (at[-2], at[-1]) if got.ndim >= 2 else (0, at[0])
    return "%s %s: %d of %d differ, first at plane %s y %d x %d (block %d,%d; tile %d,%d): %s, expected %s" % (
        stage, name, len(bad), got.size, at[:-2], y, x, x // 16, y // 16, x // TILE, y // TILE, got[at], exp[at])
