"""Hand-built canvases for the push-pull padding of the attribute planes (S21, csrc/attributes.hip): the sheet route of
canvas_cases.py with masks of this module's own -- a whole 96 x 96 tile, a one-pixel frame around a canvas, a lattice of single
pixels, a checkerboard as large as a canvas -- on canvas sizes chosen for the packed (four pixels per lane) kernels: level widths of
every residue mod 4, odd heights, a level a few pixels into a second tile, level 1 either side of the coarse kernel's size limit.
Pure numpy, deterministic; used by test_attribute_padding_cases.py (CPU tier: the scenes are what they claim) and
test_gpu_attribute_padding.py.

A mask is named by its kind and its size, "frame80x80": mask() builds it.  Sheet k of a scene lies behind the sheets before it on
every axis (40 clear of the last), all within the 10-bit cube of the segmenter's parameters.

Not reachable through the C-ABI, and therefore in no scene: an EMPTY canvas (a frame has points, every point lands in a patch, a
patch has occupied pixels), 14 - 16 blur iterations and a pyramid of more than kPushPullLevels levels (both need a canvas of more
than 16384 pixels on its short side: canvas_cases.py).  The tall thin canvas 16 x 25664 has three levels and 4 and 5 passes, all
through the tiles: what it covers is a column of 268 tiles and no coarse launch, not the iteration cap."""
import functools

import numpy as np

import canvas_cases as cc

TILE, SPAN, SMALL, LEVELS = 96, 128, 160 * 160, 16          # kPushPullTile, kPushPullSpan, kPushPullSmall, kPushPullLevels
LDS_MAX = 160 * 1024 - 64                                   # what allowLargeLds grants a workgroup


def level_words(w, h):
    """pushPullLevelWords: LDS words of a level in the coarse kernel (a word in front, image, partner, a word behind, mask)"""
    return 3 * ((w + 3) >> 2) * h + 2


def paths(W, H):
    """The rule of generateAttributeImages restated: -> dict(levels, first (None: the coarse kernel is not launched), lds (bytes of
    its launch, 0), fills: per filled level l (count - 2 .. 0) a tuple (l, path, iters), path = "coarse" (inside the one-workgroup
    kernel, in LDS) or "tiles" (pushPullFillBlurKernel); the per-pass launches behind iters > 16 are unreachable: the count is capped)."""
    levels = cc.pyramid(W, H)["levels"]
    n = len(levels)
    lds_from = [0] * (n + 1)
    for l in range(n - 1, 0, -1):
        lds_from[l] = lds_from[l + 1] + 4 * level_words(*levels[l])
    first = None
    if n <= LEVELS:
        for l in range(1, n):
            if levels[l][0] * levels[l][1] <= SMALL and lds_from[l] <= LDS_MAX:
                first = l
                break
    if first is not None and first + 1 >= n:
        first = None                                        # (nothing below it to fill it from: no launch)
    fills, iters = [], 4
    for l in range(n - 2, -1, -1):
        fills.append((l, "coarse" if first is not None and l >= first else "tiles", iters))
        iters = min(iters + 1, 16)
    return dict(levels=levels, first=first, lds=0 if first is None else lds_from[first], fills=fills)


@functools.lru_cache(maxsize=None)
def mask(name):
    kind = name.rstrip("0123456789x")
    w, h = (int(t) for t in name[len(kind):].split("x"))
    a = np.zeros((h, w), bool)
    if kind == "full":
        a[:] = True
    elif kind == "frame":                                   # column 0, the last column, row 0, the last row: one pixel thick
        a[0, :] = a[-1, :] = a[:, 0] = a[:, -1] = True
    elif kind == "dots":                                    # single pixels 16 apart, the last row and column included: every corner
        xs, ys = sorted(set(range(0, w, 16)) | {w - 1}), sorted(set(range(0, h, 16)) | {h - 1})
        a[np.ix_(ys, xs)] = True
    elif kind == "checker":
        v, u = np.indices((h, w))
        a = (u + v) % 2 == 0
    else:
        raise KeyError(name)
    return a


def mask_key(name, label):
    m = mask(name)
    return (label % 3, m.shape[1], m.shape[0], int(m.sum()))


@functools.lru_cache(maxsize=None)
def cloud(sheets, seed=21):
    """sheets: ((mask name, label), ...) -> (xyz int16, rgb uint8, partition uint32); as canvas_cases.cloud: a first layer at a
    constant depth, a second layer 0..3 further along the normal at a colour within 60 of the first layer's, points shuffled"""
    rng = np.random.default_rng(seed)
    pts, cols, part, origin = [], [], [], 12
    for name, label in sheets:
        ax = cc.AXES[label % 3]
        v, u = np.nonzero(mask(name))
        d = np.full(len(u), 8)
        layer = rng.integers(0, 4, len(u))
        base = rng.integers(0, 256, (len(u), 3))
        second = np.clip(base + rng.integers(-60, 61, base.shape), 0, 255)
        for dd, c, keep in ((d, base, np.ones(len(u), bool)), (d + layer, second, layer > 0)):
            p = np.zeros((int(keep.sum()), 3), np.int64)
            p[:, ax[0]], p[:, ax[1]], p[:, ax[2]] = dd[keep], u[keep], v[keep]
            pts.append(p + origin)
            cols.append(c[keep])
            part.append(np.full(len(p), label))
        origin += max(mask(name).shape) + 40
    xyz, rgb, part = np.concatenate(pts), np.concatenate(cols), np.concatenate(part)
    assert xyz.min() >= 0 and xyz.max() < 1024
    order = rng.permutation(len(xyz))
    return xyz[order].astype(np.int16), rgb[order].astype(np.uint8), part[order].astype(np.uint32)


class PadScene(cc.Scene):
    """placements: [(mask name, u0, v0, patchOrientation)] in list order, block units; sheet k gets the label k % 3"""

    def __init__(self, name, W, H, precision, placements):
        self.name, self.W, self.H, self.precision, self.api_only = name, W, H, precision, True
        self.placements = [tuple(p) + (0,) for p in placements]
        self.masks = tuple(p[0] for p in placements)
        self.labels = {n: k % 3 for k, n in enumerate(self.masks)}
        assert len(set(mask_key(n, self.labels[n]) for n in self.masks)) == len(self.masks)

    def cloud(self):
        return cloud(tuple((n, self.labels[n]) for n in self.masks))

    def keys(self):
        return [mask_key(n, self.labels[n]) for n in self.masks]

    def find(self, patches, name):
        key = mask_key(name, self.labels[name])
        got = [i for i, p in enumerate(patches) if (p["normalAxis"], p["sizeU"], p["sizeV"], p["d0Count"]) == key]
        assert len(got) == 1, (name, got)
        return got[0]

    def boxes(self):
        out = []
        for name, u0, v0, orient, _ in self.placements:
            bu, bv = -(-mask(name).shape[1] // 16), -(-mask(name).shape[0] // 16)
            out.append((u0, v0, bv, bu) if orient else (u0, v0, bu, bv))
        return out

    def painted(self):
        out = []
        for name, u0, v0, orient, _ in self.placements:
            m = mask(name).T if orient else mask(name)
            a = np.zeros((self.H, self.W), bool)
            a[v0 * 16:v0 * 16 + m.shape[0], u0 * 16:u0 * 16 + m.shape[1]] = m
            out.append(a)
        return out


SCENES = [
    # 40, 20, 10, 5, 3 wide levels: every residue mod 4, odd heights, less than one tile; the canvas' four edges occupied
    PadScene("frame_80x80", 80, 80, 1, [("frame80x80", 0, 0, 0)]),
    # single pixels: the canvas' four corners and the middle among them
    PadScene("dots_80x80", 80, 80, 1, [("dots80x80", 0, 0, 0)]),
    PadScene("checker_80x80", 80, 80, 1, [("checker80x80", 0, 0, 0)]),
    # 168, 84, 42, 21, 11, 6, 3; tile (1, 1) of level 0 wholly occupied, the tiles of the last tile row and column wholly empty,
    # a frame that straddles the seam x = 96 at the top
    PadScene("tile_336x336", 336, 336, 1, [("full96x96", 6, 6, 0), ("frame48x32", 4, 0, 0), ("dots64x48", 13, 0, 0)]),
    PadScene("frame_336x336_p4", 336, 336, 4, [("frame336x336", 0, 0, 0)]),
    # level 1 of 160 x 160 = kPushPullSmall pixels: the coarse kernel's largest first level; 152 x 168 just below; 160 x 168 above
    PadScene("at_limit_320x320", 320, 320, 1, [("dots320x320", 0, 0, 0)]),
    PadScene("below_limit_304x336", 304, 336, 1, [("dots304x336", 0, 0, 0)]),
    PadScene("above_limit_320x336", 320, 336, 1, [("dots320x336", 0, 0, 0)]),
    # 400 = 4 tiles + 16, 200 = 2 tiles + 8, 100 = one tile + 4; 112 = one tile + 16 high
    PadScene("second_tile_400x112", 400, 112, 1, [("frame400x112", 0, 0, 0)]),
    # 1552, 776, 388, 194, 97: the odd 97 and 49 wide levels (like the 100 of the canvas above) are levels of the coarse kernel;
    # through the tiles, the widths a few pixels into a further tile are 400, 112 and the 104 of the canvas below
    PadScene("second_tile_1552x112", 1552, 112, 4, [("dots64x64", 0, 0, 0), ("frame48x48", 94, 4, 0), ("checker32x16", 47, 3, 1)]),
    # level 1 through the tiles (104 x 256 pixels, more than kPushPullSmall) and one tile + 8 wide; level 0 two tiles + 16
    PadScene("second_tile_208x512", 208, 512, 4, [("dots64x64", 0, 0, 0), ("frame48x48", 10, 29, 0), ("checker32x16", 6, 14, 1)]),
    # 7 passes at level 0: the second tile's region is 23 pixels wide -- its last pixel in byte 2 of a word (80: byte 3, the 81 and
    # 58 of the 336 canvases: bytes 0 and 1)
    PadScene("second_tile_112x48", 112, 48, 1, [("frame112x48", 0, 0, 0)]),
    cc.BY_NAME["api_1296x1328"],                            # a 162 wide level (2 mod 4) through the tiles
    cc.BY_NAME["api_no_small_level_16x25664"],              # a tall thin canvas: no coarse launch, 268 tiles in one column
]
BY_NAME = {s.name: s for s in SCENES}
# one packing inside both canvases, for the canvas sizes in turn on one frame
IN_TURN = [("dots64x64", 0, 0, 0), ("checker32x16", 4, 0, 1)]
