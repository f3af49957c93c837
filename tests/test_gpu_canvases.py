"""GPU tier (-m gpu): the encoder's canvases (S11-S16 in csrc/images.hip, S20-S22 in csrc/attributes.hip) on the hand-built scenes of
canvas_cases.py, through the C-ABI as it stands: a cloud of flat sheets and tmc2_frame_set_partition give patches whose occupancy is
known by construction, tmc2_frame_set_packing puts them where the scene wants them, tmc2_encoder_generate_geometry_images takes the
scene's canvas size.  Everything is exact integer equality with the CPU oracle on the same placed records; a mismatch names the
stage, the plane and the first differing pixel with its block and its tile.  What each scene makes the kernels do is asserted on
the CPU (test_canvas_cases.py), where the oracle is also pinned to the unmodified reference on the canvas sizes the reference can
make; on the api_only canvases the oracle alone is the yardstick."""
import functools

import numpy as np
import pytest

import canvas_cases as cc
import oracle_binding as ob
import tmc2_amd as T
from test_gpu_segmenter import _assert_patches_equal

pytestmark = pytest.mark.gpu

ORACLE_PARAMS = ob.seg_params(10, 10, (1.0, 1.0, 1.0))
GEOMETRY = ("occupancy", "occ_video", "block_to_patch", "geo0", "geo1")
E_STATE, E_INVALID, E_UNSUPPORTED = r"tmc2hip error -5: ", r"tmc2hip error -3: ", r"tmc2hip error -4: "
_forward = {}                                            # scene -> what the session's context made of it (the forward pass)


@functools.lru_cache(maxsize=None)
def _oracle():
    return ob.Oracle()


@functools.lru_cache(maxsize=None)
def answer(scene):
    """the oracle's answer for a scene, computed once and shared (read only)"""
    return cc.oracle_canvases(_oracle(), scene, ORACLE_PARAMS)


def segmented_frame(ctx, scene):
    xyz, rgb, part = scene.cloud()
    fr = ctx.frame(xyz, rgb)
    fr.normals_compute_normals(16)                       # the resident adjacency S7 walks (its normals are not read)
    fr.set_partition(part)
    fr.segmenter_segment_patches(T.ctc_params(10, 10, (1.0, 1.0, 1.0)))
    return fr


def generate(fr, scene):
    """the scene's placement and canvas size on a segmented (or already packed) frame -> everything the encoder's image stages leave"""
    patches, _, _, occ = fr.get_patches()
    lst, pool = scene.place(patches, occ)
    fr.set_packing(lst, None, pool, scene.W, scene.H)
    return regenerate(fr, scene)


def regenerate(fr, scene):
    fr.encoder_generate_geometry_images(scene.W, scene.H, scene.precision)
    got = fr.get_geometry_images()
    fr.encoder_generate_attribute_images()
    got["recon_xyz"], got["recon_rgb"], got["point_to_pixel"] = fr.get_reconstruction()
    got["attribute"] = fr.get_attribute_images()
    return got


def assert_matches_oracle(got, scene):
    exp = answer(scene)
    for k in GEOMETRY:
        assert cc.first_difference("S11-S16", k, got[k], exp["img"][k]) is None
    for k in ("recon_xyz", "point_to_pixel", "recon_rgb"):
        assert cc.first_difference("S17-S18", k, got[k], exp[k]) is None
    assert cc.first_difference("S20-S22", "attribute", got["attribute"], exp["attribute"]) is None


def assert_identical(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def run_scene(ctx, scene):
    fr = segmented_frame(ctx, scene)
    _assert_patches_equal(fr.get_patches(), answer(scene)["seg"])
    got = generate(fr, scene)
    assert_matches_oracle(got, scene)
    return got


@pytest.mark.parametrize("scene", cc.SCENES, ids=repr)
def test_gpu_scene_matches_oracle(gpu_ctx, scene):
    _forward[scene.name] = run_scene(gpu_ctx, scene)


def test_gpu_scenes_in_reverse_order_on_a_fresh_context():
    """The pools hand a smaller pyramid the bytes a larger one left behind: the same scenes in the opposite order, on a context
    that has seen nothing else, give the same canvases (as the oracle's, and byte for byte as the forward pass where it ran)."""
    ctx = T.Context(0)
    try:
        for scene in reversed(cc.SCENES):
            got = run_scene(ctx, scene)
            if scene.name in _forward:
                assert_identical(got, _forward[scene.name])
    finally:
        ctx.close()


def test_gpu_canvas_sizes_in_turn_on_one_frame(gpu_ctx):
    """1344 x 1344, then 64 x 2048, then 1344 x 1344 again from one packing on one frame: the first and the third are identical,
    the second equals a fresh frame's."""
    both = [("checker", 1, 0, 0), ("full", 2, 61, 0), ("ring", 1, 60, 0), ("w17", 1, 70, 1), ("less1", 3, 75, 0), ("slope", 2, 81, 1)]
    thin = cc.Scene("four_columns_on_64x2048", 64, 2048, 4, both)          # 4 x 84 blocks: inside both canvases
    large = cc.Scene("four_columns_on_1344x1344", 1344, 1344, 4, both)
    fr = segmented_frame(gpu_ctx, thin)
    first = generate(fr, large)
    assert_matches_oracle(first, large)
    second = regenerate(fr, thin)
    assert_matches_oracle(second, thin)
    third = regenerate(fr, large)
    assert_identical(third, first)
    assert_identical(second, generate(segmented_frame(gpu_ctx, thin), thin))


def test_gpu_second_placement_leaves_no_stale_canvases(gpu_ctx):
    """a second tmc2_frame_set_packing with another placement: the old canvases are gone, the new ones are the oracle's"""
    one, two = cc.BY_NAME["every_mask_256x128_p4"], cc.BY_NAME["above_small_384x320"]
    fr = segmented_frame(gpu_ctx, one)
    assert_matches_oracle(generate(fr, one), one)
    patches, _, _, occ = fr.get_patches()                # (in list order now, pool in list order)
    lst, pool = two.place(patches, occ)
    fr.set_packing(lst, None, pool, two.W, two.H)
    with pytest.raises(T.Tmc2Error, match=E_STATE + ".*not generated"):
        fr.get_geometry_images()
    with pytest.raises(T.Tmc2Error, match=E_STATE + ".*not generated"):
        fr.get_reconstruction()
    with pytest.raises(T.Tmc2Error, match=E_STATE + ".*not generated"):
        fr.get_attribute_images()
    assert_matches_oracle(regenerate(fr, two), two)


@pytest.mark.parametrize("moved", [("less1", 4, 3, 1), ("full", 0, 4, 0), ("w17", 3, 1, 0)], ids=["right", "below", "second_block_right"])
def test_gpu_placement_outside_the_canvas_is_refused(gpu_ctx, moved):
    """A placement whose pixels leave the canvas (the reference exits with code 180): refused, nothing half made, and a correct call
    on the same frame afterwards gives the oracle's canvases.  (The raster tests every pixel against W and H before it writes.)"""
    good = cc.BY_NAME["origin_empty_64x64"]
    bad = cc.Scene("outside", good.W, good.H, good.precision, [moved if p[0] == moved[0] else p for p in good.placements])
    fr = segmented_frame(gpu_ctx, good)
    assert_matches_oracle(generate(fr, good), good)
    patches, _, _, occ = fr.get_patches()
    lst, pool = bad.place(patches, occ)
    fr.set_packing(lst, None, pool, bad.W, bad.H)
    with pytest.raises(T.Tmc2Error, match=E_INVALID + ".*falls outside the 64x64 canvas"):
        fr.encoder_generate_geometry_images(bad.W, bad.H, bad.precision)
    with pytest.raises(T.Tmc2Error, match=E_STATE + ".*not generated"):
        fr.get_geometry_images()
    with pytest.raises(T.Tmc2Error, match=E_STATE):
        fr.encoder_generate_attribute_images()
    assert_matches_oracle(generate(fr, good), good)


@pytest.mark.parametrize("W,H,prec", [(72, 64, 4), (64, 72, 4), (60, 60, 4), (64, 64, 3), (64, 64, 0), (64, 64, 32)])
def test_gpu_unsupported_canvas_is_refused(gpu_ctx, W, H, prec):
    """sizes that are no multiple of 16 and precisions that do not divide 16: TMC2_E_UNSUPPORTED, and the frame still works"""
    good = cc.BY_NAME["origin_empty_64x64"]
    fr = segmented_frame(gpu_ctx, good)
    patches, _, _, occ = fr.get_patches()
    lst, pool = good.place(patches, occ)
    fr.set_packing(lst, None, pool, good.W, good.H)
    with pytest.raises(T.Tmc2Error, match=E_UNSUPPORTED + ".*unsupported geometry"):
        fr.encoder_generate_geometry_images(W, H, prec)
    assert_matches_oracle(regenerate(fr, good), good)
