"""GPU tier (-m gpu): the push-pull padding of the attribute planes (S21, csrc/attributes.hip: the coarse levels of the pyramid in the
LDS of one workgroup per plane, the fine levels in tiles, blur passes on four pixels per lane) on the canvases of
attribute_padding_cases.py, through the C-ABI: a cloud of flat sheets and tmc2_frame_set_partition give one patch per sheet,
tmc2_frame_set_packing puts them where the scene wants them, tmc2_encoder_generate_geometry_images takes the scene's canvas size.
The six attribute planes -- and every canvas before them -- are compared with the CPU oracle by exact equality; a mismatch names the
plane, the first differing pixel and its tile.  What each canvas makes the kernels do (the path and the iteration count of every
level, the residues of the level widths, the occupancy patterns) is asserted on the CPU in test_attribute_padding_cases.py."""
import functools

import pytest

import attribute_padding_cases as ap
import canvas_cases as cc
import oracle_binding as ob
import tmc2_amd as T

pytestmark = pytest.mark.gpu

ORACLE_PARAMS = ob.seg_params(10, 10, (1.0, 1.0, 1.0))
GEOMETRY = ("occupancy", "occ_video", "block_to_patch", "geo0", "geo1")


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
    fr.normals_compute_normals(16)                       # the resident adjacency the patch rounds walk (its normals are not read)
    fr.set_partition(part)
    fr.segmenter_segment_patches(T.ctc_params(10, 10, (1.0, 1.0, 1.0)))
    return fr


def regenerate(fr, scene):
    fr.encoder_generate_geometry_images(scene.W, scene.H, scene.precision)
    got = fr.get_geometry_images()
    fr.encoder_generate_attribute_images()
    got["recon_xyz"], got["recon_rgb"], got["point_to_pixel"] = fr.get_reconstruction()
    got["attribute"] = fr.get_attribute_images()
    return got


def generate(fr, scene):
    """the scene's placement and canvas size on a segmented frame -> everything the encoder's image stages leave"""
    patches, _, _, occ = fr.get_patches()
    lst, pool = scene.place(patches, occ)
    fr.set_packing(lst, None, pool, scene.W, scene.H)
    return regenerate(fr, scene)


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
    got = generate(segmented_frame(ctx, scene), scene)
    assert_matches_oracle(got, scene)
    return got


@pytest.mark.parametrize("scene", ap.SCENES, ids=repr)
def test_gpu_padding_scene_matches_oracle(gpu_ctx, scene):
    run_scene(gpu_ctx, scene)


def test_gpu_padding_scenes_again_on_a_fresh_context(gpu_ctx):
    """the same canvases in the opposite order on a context that has seen nothing else (its pool hands a small pyramid the bytes a
    large one left): the oracle's canvases, byte for byte those of the session's context"""
    ctx = T.Context(0)
    try:
        for scene in reversed(ap.SCENES):
            assert_identical(run_scene(ctx, scene), run_scene(gpu_ctx, scene))
    finally:
        ctx.close()


def test_gpu_padding_two_canvas_sizes_in_turn_on_one_frame(gpu_ctx):
    """336 x 336 (coarse kernel from level 2, 28 848 bytes of LDS), then 80 x 80 (from level 1, 6 556 bytes), then 336 x 336 again, from
    one packing on one frame: the launch is sized anew each time; the first and the third are identical, the second a fresh frame's"""
    large, small = ap.PadScene("in_turn_336x336", 336, 336, 1, ap.IN_TURN), ap.PadScene("in_turn_80x80", 80, 80, 1, ap.IN_TURN)
    assert (ap.paths(336, 336)["first"], ap.paths(336, 336)["lds"]) == (2, 28848) and (ap.paths(80, 80)["first"], ap.paths(80, 80)["lds"]) == (1, 6556)
    fr = segmented_frame(gpu_ctx, small)
    first = generate(fr, large)
    assert_matches_oracle(first, large)
    second = regenerate(fr, small)
    assert_matches_oracle(second, small)
    third = regenerate(fr, large)
    assert_identical(third, first)
    assert_identical(second, generate(segmented_frame(gpu_ctx, small), small))
