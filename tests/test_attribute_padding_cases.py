"""CPU tier: the canvases of attribute_padding_cases.py are what they claim -- asserted from the oracle's output and from the rule of
generateAttributeImages restated in paths() -- so that a case of test_gpu_attribute_padding.py cannot silently stop covering what it
names: the residues of the level widths on either path, the path and the iteration count of every level, the tile and region
shapes of the tiles' kernel, the occupancy patterns."""
import functools

import numpy as np
import pytest

import attribute_padding_cases as ap
import canvas_cases as cc
import oracle_binding as ob
from test_canvas_cases import mip_occupancy

PARAMS = ob.seg_params(10, 10, (1.0, 1.0, 1.0))
_oracle = []


@functools.lru_cache(maxsize=None)
def answer(name):
    return cc.oracle_canvases(_oracle[0], ap.BY_NAME[name], PARAMS)


@pytest.fixture(autouse=True)
def _bind(oracle):
    _oracle[:] = [oracle]


def occupancy(scene):
    """what S21 sees: the occupancy video upsampled by the precision"""
    return np.kron(answer(scene.name)["img"]["occ_video"], np.ones((scene.precision, scene.precision), np.uint8)) != 0


def tile(a, tx, ty):
    return a[ty * ap.TILE:(ty + 1) * ap.TILE, tx * ap.TILE:(tx + 1) * ap.TILE]


def region_widths(W, iters):
    """widths of the regions pushPullFillBlurKernel loads along a row of tiles: the tile grown by iters, clipped to the image"""
    return [min(x0 + ap.TILE + iters, W) - max(x0 - iters, 0) for x0 in range(0, W, ap.TILE)]


@pytest.mark.parametrize("scene", [s for s in ap.SCENES if isinstance(s, ap.PadScene)], ids=repr)
def test_scene_is_one_patch_per_sheet_where_it_was_put(scene):
    r = answer(scene.name)
    seg, img = r["seg"], r["img"]
    assert seg["stalled"] == 0 and seg["round_raw"].tolist() == [0]
    got = sorted((int(p["normalAxis"]), int(p["sizeU"]), int(p["sizeV"]), int(p["d0Count"])) for p in seg["patches"])
    assert got == sorted(scene.keys())
    for (x0, y0, w, h) in scene.boxes():
        assert x0 >= 0 and y0 >= 0 and (x0 + w) * 16 <= scene.W and (y0 + h) * 16 <= scene.H
    total = sum(a.astype(np.int32) for a in scene.painted())
    assert total.max() == 1 and np.array_equal(total > 0, img["occupancy"] > 0)
    if scene.precision == 1:
        assert np.array_equal(occupancy(scene), total > 0)


def test_paths_restates_the_level_rule():
    p = ap.paths(1280, 1344)                                # the benchmark's longdress canvas: level 3 of 160 x 168 is above the limit
    assert p["levels"][3:5] == [(160, 168), (80, 84)] and p["first"] == 4 and p["lds"] == 4 * sum(ap.level_words(w, h) for w, h in p["levels"][4:])
    assert [f[1:] for f in p["fills"]] == [("coarse", 4), ("coarse", 5), ("coarse", 6), ("coarse", 7), ("coarse", 8), ("tiles", 9),
                                           ("tiles", 10), ("tiles", 11), ("tiles", 12)]
    assert ap.level_words(80, 84) == 3 * 20 * 84 + 2 and ap.level_words(5, 5) == 3 * 2 * 5 + 2 and ap.level_words(3, 3) == 11
    p = ap.paths(1280, 1280)                                # a one-frame GOF's canvas: level 3 is 160 x 160, at the limit
    assert p["first"] == 3 and p["lds"] == 102572 and [f[2] for f in p["fills"] if f[1] == "tiles"] == [10, 11, 12]
    p = ap.paths(16, 25664)
    assert p["first"] is None and [f[1:] for f in p["fills"]] == [("tiles", 4), ("tiles", 5)]
    # the largest launch the size rule admits stays inside a workgroup's LDS: a first level of 5 x 5120 over 3 x 2560
    assert 4 * (ap.level_words(5, 5120) + ap.level_words(3, 2560)) <= ap.LDS_MAX
    for W, H in [(s.W, s.H) for s in ap.SCENES]:
        assert ap.paths(W, H)["lds"] <= ap.LDS_MAX and len(ap.paths(W, H)["levels"]) <= ap.LEVELS


def test_side_conditions_over_the_canvases():
    seen, coarse_res, tile_res, edge_byte, coarse_iters, tile_iters = set(), set(), set(), set(), set(), set()
    heights_odd = set()
    for scene in ap.SCENES:
        p = ap.paths(scene.W, scene.H)
        occ = occupancy(scene)
        mips = mip_occupancy(occ, p["levels"])
        n = len(p["levels"])
        if p["first"] is not None:
            for l in range(p["first"], n):                  # every level the coarse kernel holds in LDS
                w, h = p["levels"][l]
                coarse_res.add(w % 4)
                if h & 1:
                    heights_odd.add("coarse")
                if w & 1 and mips[l][:, -1].any():
                    seen.add("coarse_odd_width_last_column_occupied")
        for l, path, iters in p["fills"]:
            w, h = p["levels"][l]
            if path == "coarse":
                coarse_iters.add(iters)
                continue
            tile_iters.add(iters)
            tile_res.add(w % 4)
            widths = region_widths(w, iters)
            assert max(widths) <= ap.SPAN and max(region_widths(h, iters)) <= ap.SPAN
            edge_byte |= {(rw - 1) & 3 for rw in widths}
            if len(widths) > 1 and 0 < w - (len(widths) - 1) * ap.TILE <= 16:
                seen.add("a_few_pixels_into_a_second_tile_%d" % w)
            if len(widths) > 1 and widths[-1] < iters + 16:
                seen.add("last_region_mostly_margin")
        levels1 = p["levels"][1][0] * p["levels"][1][1]
        if levels1 == ap.SMALL and p["first"] == 1:
            seen.add("level1_at_the_limit")
        if ap.SMALL - 128 < levels1 < ap.SMALL and p["first"] == 1:
            seen.add("level1_just_below_the_limit")
        if ap.SMALL < levels1 <= ap.SMALL + 8 * 160 and p["first"] == 2:    # (level-1 sides are multiples of 8: the nearest above)
            seen.add("level1_just_above_the_limit")
        if p["first"] is None:
            seen.add("no_coarse_launch")
        if scene.W < ap.TILE and scene.H < ap.TILE:
            seen.add("less_than_one_tile")
        if scene.W < ap.TILE and scene.H > 100 * ap.TILE:
            seen.add("tall_thin")
        tx, ty = -(-scene.W // ap.TILE), -(-scene.H // ap.TILE)
        for y in range(ty):
            for x in range(tx):
                t = tile(occ, x, y)
                if t.shape == (ap.TILE, ap.TILE) and t.all():
                    seen.add("tile_wholly_occupied")
                if not t.any() and occ.any():
                    seen.add("tile_wholly_empty")
        pad = np.pad(occ, 1)
        alone = occ & (sum(pad[1 + dy:1 + dy + occ.shape[0], 1 + dx:1 + dx + occ.shape[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) == 1)
        if alone[0, 0] and alone[0, -1] and alone[-1, 0] and alone[-1, -1]:
            seen.add("single_pixels_in_the_corners")
        if alone[1:-1, 1:-1].any():
            seen.add("single_pixel_inside")
        v, u = np.indices(occ.shape)
        if np.array_equal(occ, (u + v) % 2 == 0):
            seen.add("checkerboard_canvas")
        if occ[:, 0].all() and occ[:, -1].all() and occ[0, :].all() and occ[-1, :].all() and not occ[1:-1, 1:-1].any():
            seen.add("edges_occupied_inside_empty_p%d" % scene.precision)
    assert coarse_res == {0, 1, 2, 3} and heights_odd == {"coarse"}
    assert tile_res >= {0, 2}                               # (an odd level of more than kPushPullSmall pixels needs 6.5 Mpixel: none)
    assert edge_byte == {0, 1, 2, 3}                        # the byte of a region's last pixel in its word: every clamp select
    assert coarse_iters == set(range(4, 10)) and tile_iters >= {4, 5, 7, 8, 9, 10, 11, 12}, (coarse_iters, tile_iters)   # both parities on either path
    want = {"coarse_odd_width_last_column_occupied", "a_few_pixels_into_a_second_tile_104", "a_few_pixels_into_a_second_tile_112",
            "a_few_pixels_into_a_second_tile_400", "last_region_mostly_margin", "level1_at_the_limit", "level1_just_below_the_limit",
            "level1_just_above_the_limit", "no_coarse_launch", "less_than_one_tile", "tall_thin", "tile_wholly_occupied",
            "tile_wholly_empty", "single_pixels_in_the_corners", "single_pixel_inside", "checkerboard_canvas",
            "edges_occupied_inside_empty_p1"}
    assert want - seen == set(), sorted(want - seen)


def test_in_turn_packing_fits_both_canvases():
    for W, H in ((336, 336), (80, 80)):
        s = ap.PadScene("in_turn", W, H, 1, ap.IN_TURN)
        for (x0, y0, w, h) in s.boxes():
            assert (x0 + w) * 16 <= W and (y0 + h) * 16 <= H
        assert sum(a.astype(np.int32) for a in s.painted()).max() == 1
