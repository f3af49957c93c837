"""CPU tier: the scenes of canvas_cases.py are what they claim -- asserted from the oracle's output and pyramid() alone -- and the
oracle equals the unmodified reference on the scenes' clouds at every canvas size the reference can make.  What is asserted here is
what test_gpu_canvases.py relies on when it says that a branch of the image kernels has run."""
import functools

import numpy as np
import pytest

import canvas_cases as cc
import oracle_binding as ob

PARAMS = ob.seg_params(10, 10, (1.0, 1.0, 1.0))
_oracle = []


@functools.lru_cache(maxsize=None)
def answer(name):
    """the oracle's canvases of a scene, computed once and shared (read only)"""
    return cc.oracle_canvases(_oracle[0], cc.BY_NAME[name], PARAMS)


@pytest.fixture(autouse=True)
def _bind(oracle):
    _oracle[:] = [oracle]


def block_counts(occ):
    H, W = occ.shape
    return (occ != 0).reshape(H // 16, 16, W // 16, 16).sum(axis=(1, 3))


def block_pixels(a, bx, by):
    return a[by * 16:by * 16 + 16, bx * 16:bx * 16 + 16]


def upsampled(scene, img):
    return np.kron(img["occ_video"], np.ones((scene.precision, scene.precision), np.uint8))


def test_masks_are_told_apart_by_their_records():
    keys = [cc.mask_key(n) for n in cc.ALL]
    assert len(set(keys)) == len(keys)


@pytest.mark.parametrize("scene", cc.SCENES, ids=repr)
def test_scene_is_one_patch_per_mask_placed_without_overlap(oracle, scene):
    r = answer(scene.name)
    seg, img = r["seg"], r["img"]
    assert seg["stalled"] == 0 and seg["round_raw"].tolist() == [0]          # one round, no point left raw: nothing else becomes a patch
    got = sorted((int(p["normalAxis"]), int(p["sizeU"]), int(p["sizeV"]), int(p["d0Count"])) for p in seg["patches"])
    assert got == sorted(cc.mask_key(n) for n in scene.masks) and len(set(got)) == len(got)
    for (x0, y0, w, h) in scene.boxes():
        assert x0 >= 0 and y0 >= 0 and (x0 + w) * 16 <= scene.W and (y0 + h) * 16 <= scene.H
    painted = scene.painted()
    total = sum(a.astype(np.int32) for a in painted)
    assert total.max() == 1                                                   # occupied pixels of two patches never overlap
    assert np.array_equal(total > 0, img["occupancy"] > 0)                    # the raster put every mask where it was told to
    assert int(total.sum()) == int(seg["patches"]["d0Count"].sum())
    occ = img["occupancy"] != 0
    p = scene.precision
    cells = occ.reshape(scene.H // p, p, scene.W // p, p).any(axis=(1, 3))
    assert np.array_equal(img["occ_video"] != 0, cells)
    inside = upsampled(scene, img) != 0
    assert np.array_equal(img["geo0"][~inside], img["geo1"][~inside])          # outside the occupied cells the two maps were equalised
    assert np.array_equal(img["block_to_patch"] != 0, block_counts(img["occupancy"]) > 0)


def test_geometry_side_conditions_over_the_set():
    seen = set()
    edges = set()
    for scene in cc.SCENES:
        r = answer(scene.name)
        img, lst = r["img"], r["list"]
        occ, g0, g1 = img["occupancy"] != 0, img["geo0"], img["geo1"]
        cnt = block_counts(occ)
        Hb, Wb = cnt.shape
        seen.add("origin_occupied" if cnt[0, 0] else "origin_empty")
        col0 = cnt[:, 0]
        if np.any((col0[:-1] > 0) & (col0[1:] == 0)):
            seen.add("empty_under_occupied_in_column0")
        if np.any((col0[:-2] > 0) & (col0[1:-1] == 0) & (col0[2:] == 0)):
            seen.add("run_of_empty_under_occupied_in_column0")
        if not col0.any() and cnt.any():
            seen.add("column0_all_empty")
        if cnt[0, 0] == 0 and col0.any():
            seen.add("origin_empty_first_of_column0_further_down")
        rows = cnt.any(axis=1)
        for r0 in range(Hb - 2):
            if not rows[r0] and not rows[r0 + 1] and rows[:r0].any() and rows[r0 + 2:].any():
                seen.add("two_empty_block_rows_between_patches")
        if Wb == 1:
            seen.add("single_block_column")
        if scene.H % 64:
            seen.add("height_no_multiple_of_64")
        for by, bx in np.argwhere(cnt == 1):
            y, x = np.argwhere(block_pixels(occ, bx, by))[0]
            if (x in (0, 15)) and (y in (0, 15)):
                seen.add("one_pixel_corner_%d_%d" % (x, y))
        for by, bx in np.argwhere(cnt == 128):
            b = block_pixels(occ, bx, by)
            yy, xx = np.indices(b.shape)
            if np.array_equal(b, (xx + yy) % 2 == 0) or np.array_equal(b, (xx + yy) % 2 == 1):
                seen.add("checkerboard_block")
        if np.any(cnt == 255):
            seen.add("block_of_255")
        if np.any(cnt == 256):
            seen.add("block_of_256")
        for by, bx in np.argwhere((cnt > 0) & (cnt < 256)):
            b = block_pixels(occ, bx, by)
            if len(np.unique(block_pixels(g0, bx, by)[b])) >= 3:
                seen.add("partial_block_with_three_d0_values")
                break
        if np.any(g1[occ] != g0[occ]):
            seen.add("d1_differs_on_occupied_pixels")
        inside = upsampled(scene, img) != 0
        if np.any(g1[inside & ~occ] != g0[inside & ~occ]):
            seen.add("d1_differs_on_padding_inside_occupied_cells")          # (each map dilated for itself; outside: equalised, above)
        if occ[-1, :].any() and occ[:, -1].any():
            seen.add("last_row_and_last_column_occupied")
        if occ[-1, -1]:
            seen.add("last_pixel_occupied")
        for (name, u0, v0, orient, grow), (x0, y0, w, h) in zip(scene.placements, scene.boxes()):
            if not grow and (x0 + w == Wb or y0 + h == Hb):
                edges.add((orient, x0 + w == Wb, y0 + h == Hb))
        # a small patch in the ring's hole: the block belongs to whichever of the two is listed later
        names = [p[0] for p in scene.placements]
        if "ring" in names:
            k = names.index("ring")
            rx, ry = scene.placements[k][1] + 1, scene.placements[k][2] + 1
            for j, (name, u0, v0, _, _) in enumerate(scene.placements):
                if (u0, v0) == (rx, ry) and name != "ring":
                    assert cnt[ry, rx] >= 255
                    assert img["block_to_patch"][ry, rx] == max(j, k) + 1
                    seen.add("hole_owned_by_the_small_patch" if j > k else "hole_owned_by_the_ring")
        for p in lst:
            if p["sizeU0"] * 16 - p["sizeU"] >= 16 and p["sizeV0"] * 16 - p["sizeV"] >= 16:
                seen.add("tiles_wholly_beyond_sizeU_and_sizeV")
        if scene.precision == 1:
            assert np.array_equal(img["occ_video"], img["occupancy"])
        if scene.precision == 16:
            assert img["occ_video"].shape == cnt.shape and np.array_equal(img["occ_video"] != 0, cnt > 0)
    want = {"origin_occupied", "origin_empty", "empty_under_occupied_in_column0", "run_of_empty_under_occupied_in_column0",
            "column0_all_empty", "origin_empty_first_of_column0_further_down", "two_empty_block_rows_between_patches",
            "single_block_column", "height_no_multiple_of_64", "one_pixel_corner_0_0", "one_pixel_corner_15_0", "one_pixel_corner_0_15",
            "one_pixel_corner_15_15", "checkerboard_block", "block_of_255", "block_of_256", "partial_block_with_three_d0_values",
            "d1_differs_on_occupied_pixels", "d1_differs_on_padding_inside_occupied_cells", "last_row_and_last_column_occupied",
            "last_pixel_occupied", "hole_owned_by_the_small_patch", "hole_owned_by_the_ring", "tiles_wholly_beyond_sizeU_and_sizeV"}
    assert want - seen == set(), sorted(want - seen)
    # a patch ending in the last block column, in the last block row, in the bottom-right corner: each in both orientations
    assert edges == {(o, right, bottom) for o in (0, 1) for right, bottom in ((True, False), (False, True), (True, True))}
    every = [s for s in cc.SCENES if s.name.startswith("every_mask")]
    assert sorted(s.precision for s in every) == [1, 2, 4, 8, 16] and all(s.masks == cc.ALL and (s.W, s.H) == (256, 128) for s in every)
    assert sum((s.W, s.H) == (1344, 1344) for s in cc.SCENES) <= 2


def mip_occupancy(occ, levels):
    """the occupancy of every pyramid level by 2 x 2 OR (a missing partner at an odd edge counts as empty)"""
    out = [occ != 0]
    for (w, h) in levels[1:]:
        a = np.zeros((2 * h, 2 * w), bool)
        a[:out[-1].shape[0], :out[-1].shape[1]] = out[-1]
        out.append(a.reshape(h, 2, w, 2).any(axis=(1, 3)))
    return out


def test_pyramid_restates_the_level_rule():
    p = cc.pyramid(1280, 1280)
    assert [w for w, _ in p["levels"]] == [1280, 640, 320, 160, 80, 40, 20, 10, 5, 3] and p["first_small"] == 3
    assert p["tiles"] == (14, 14) and p["iters0"] == 12 and p["coarse_fills"] == 6
    p = cc.pyramid(16, 25664)
    assert p["levels"] == [(16, 25664), (8, 12832), (4, 6416)] and p["first_small"] is None and p["coarse_fills"] == 0
    assert min(w * h for w, h in p["levels"]) > cc.SMALL and p["tiles"] == (1, 268)
    assert cc.pyramid(320, 320)["levels"][1] == (160, 160) and cc.pyramid(320, 320)["first_small"] == 1
    assert cc.pyramid(384, 320)["levels"][1] == (192, 160) and cc.pyramid(384, 320)["first_small"] == 2


def test_attribute_side_conditions_over_the_canvases():
    seen = set()
    first, fills, iters = set(), set(), set()
    for scene in cc.SCENES:
        p = cc.pyramid(scene.W, scene.H)
        first.add(p["first_small"])
        iters.add(p["iters0"])
        if p["coarse_fills"]:
            fills.add(p["coarse_fills"] & 1)
        occ = upsampled(scene, answer(scene.name)["img"])
        mips = mip_occupancy(occ, p["levels"])
        for (w, h), m in zip(p["levels"], mips):
            assert m.shape == (h, w)
            if w > 16 and w & 1 and m[:, -1].any():
                seen.add("odd_width_above_16_last_column_occupied")
            if h > 16 and h & 1 and m[-1, :].any():
                seen.add("odd_height_above_16_last_row_occupied")
        W, H, n = scene.W, scene.H, p["iters0"]
        if W < cc.TILE and H < cc.TILE:
            seen.add("less_than_one_tile")
        if W % cc.TILE == 0 and H % cc.TILE == 0 and p["tiles"] == (2, 2):
            seen.add("two_by_two_whole_tiles")
        if (W > cc.TILE and W % cc.TILE) or (H > cc.TILE and H % cc.TILE):
            seen.add("partial_last_tile")
        if p["tiles"][0] * cc.TILE - W == cc.TILE // 2:
            seen.add("half_a_tile_at_the_end")
        # an unoccupied stretch of iters pixels either side of the first tile seam, next to occupied pixels: where a halo too short
        # by one would change a value
        free = occ == 0
        if W > cc.TILE + n and np.any(free[:, cc.TILE - n:cc.TILE + n].all(axis=1) & ~free.all(axis=1)):
            seen.add("free_stretch_across_the_seam_x96")
        if H > cc.TILE + n and np.any(free[cc.TILE - n:cc.TILE + n, :].all(axis=0) & ~free.all(axis=0)):
            seen.add("free_stretch_across_the_seam_y96")
    assert {1, 2, None} <= first and any(f is not None and f >= 4 for f in first)
    assert fills == {0, 1}                       # the host's mirror of the kernel's buffer swaps sees both parities of the level count
    assert max(iters) == 12                      # 14..16 need more than 16384 pixels on the short side: untested (canvas_cases.py)
    want = {"odd_width_above_16_last_column_occupied", "odd_height_above_16_last_row_occupied", "less_than_one_tile",
            "two_by_two_whole_tiles", "partial_last_tile", "half_a_tile_at_the_end", "free_stretch_across_the_seam_x96",
            "free_stretch_across_the_seam_y96"}
    assert want - seen == set(), sorted(want - seen)


@pytest.mark.parametrize("prec", [4, 1])
@pytest.mark.parametrize("min_w,min_h", cc.REFERENCE_CANVASES)
def test_oracle_equals_the_reference_on_the_scene_cloud(oracle, reference, min_w, min_h, prec):
    """The reference's own segmentation and packing of the sheets, on every canvas size of the scenes it can make: all nine arrays
    of the two phases.  This pins the algorithm on these canvas shapes and this sparse content; the hand placements only change
    where the occupied pixels lie.  (A sheet as wide as the canvas ends the reference's process in patch2Canvas -- exit code 180 --
    so the 64-wide canvases get the cloud without the 64-wide sheet.)"""
    names = cc.ALL if min_w > 64 else tuple(n for n in cc.ALL if cc.MASKS[n].shape[1] < 64)
    xyz, rgb, _ = cc.cloud(names)
    frames = [(xyz, rgb)]
    ra = reference.phase_a(frames, 10, 11, prec, min_w, min_h)
    rb = reference.phase_b(frames, ra, prec)
    oa = oracle.phase_a(frames, 10, 11, prec, min_w, min_h)
    ob_ = oracle.phase_b(frames, oa, prec)
    assert (oa[0]["width"], oa[0]["height"]) == (ra[0]["width"], ra[0]["height"])
    assert ra[0]["width"] % 64 == 0 and ra[0]["height"] % 64 == 0 and len(ra[0]["patches"]) >= len(names)
    for k in ("occupancy", "occ_video", "block_to_patch", "geo0", "geo1"):
        assert cc.first_difference("phase A", k, oa[0][k], ra[0][k]) is None
    for k in ("recon_xyz", "recon_rgb", "point_to_pixel", "attribute"):
        assert cc.first_difference("phase B", k, ob_[0][k], rb[0][k]) is None
