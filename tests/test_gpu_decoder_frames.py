"""GPU tier (-m gpu): the decoder-side path on hand-built frames (tests/decoder_frame_cases.py) -- tmc2_decoder_frame_create ->
tmc2_codec_generate_point_cloud -> identify_boundary_points -> color_point_cloud -> smooth_point_cloud_postprocess ->
transfer_colors_16bit_bp -> convert_yuv16_to_rgb8 on patch lists, occupancy videos and geometry maps this project's encoder
never emits: patches on the canvas borders, overlapping and empty patches, all axes and both projection modes, tiles that are
full / flat / a single pixel, occupancy precisions 1 .. 16, coincident patches, points on the faces of the smoothing grid, islands.
blockToPatchKernel, reconTileKernel, boundaryTypeKernel and colorGatherKernel against the numpy references, T3 / T4 / T5 against
the oracle fed those references (tests/test_decoder_frame_cases.py pins it to the unmodified reference on the same scenes).
Exact integer equality throughout.  No odd grid size is run here: the library refuses it (tests/test_gpu_params.py)."""
import functools

import numpy as np
import pytest

import decoder_frame_cases as dc
import tmc2_amd as T

pytestmark = pytest.mark.gpu

POST = ("xyz", "boundary", "colors16", "rgb")


def _frame(ctx, s):
    return ctx.decoder_frame(s["patches"], s["W"], s["H"], s["prec"], s["occ_video"], s["geometry"])


@functools.lru_cache(maxsize=None)
def _attribute(name, kind):
    return dc.attribute_planes(dc.scene(name), kind)


_tails = {}


def _tail(oracle, name, pair):
    """oracle.phase_c on the numpy references of a scene, computed once per (scene, pair) and left unchanged"""
    if (name, pair) not in _tails:
        s, r = dc.scene(name), dc.scene_references(name)
        a = dict(occ_video=s["occ_video"], width=s["W"], height=s["H"], block_to_patch=r["block_to_patch"])
        b = dict(point_to_pixel=r["point_to_pixel"], recon_xyz=r["xyz"])
        o = oracle.phase_c([a], [b], [_attribute(name, "random")], s["prec"], *pair)[0]
        assert np.array_equal(o["boundary_before"], r["boundary"]) and np.array_equal(o["partition"], r["partition"])
        for v in o.values():
            v.setflags(write=False)
        _tails[name, pair] = o
    return _tails[name, pair]


def _assert_post(fr, want, what):
    got = fr.get_post_reconstruction()
    for k in POST:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("name", dc.NAMES)
def test_gpu_decoder_frame_reconstruction(gpu_ctx, oracle, name):
    """block ownership, the reconstruction (points and point-to-pixel, in the reference's order), the boundary types and the 16-bit
    colours gathered from host planes: uniform random ones, and the eight corner colours beside a grey ramp"""
    s, r = dc.scene(name), dc.scene_references(name)
    fr = _frame(gpu_ctx, s)
    img = fr.get_geometry_images()
    assert np.array_equal(img["block_to_patch"], r["block_to_patch"])
    assert np.array_equal(img["occ_video"], s["occ_video"]) and np.array_equal(img["geo0"], s["geo0"]) and np.array_equal(img["geo1"], s["geo1"])
    fr.codec_generate_point_cloud()
    xyz, _, p2p = fr.get_reconstruction(colors=False)
    assert np.array_equal(xyz, r["xyz"]) and np.array_equal(p2p, r["point_to_pixel"])
    fr.codec_identify_boundary_points()
    assert np.array_equal(fr.get_post_reconstruction(colors16=False, rgb=False)["boundary"], r["boundary"])
    for kind in ("random", "corners"):
        att = _attribute(name, kind)
        fr.codec_color_point_cloud(att)
        got = fr.get_post_reconstruction(rgb=False)
        assert np.array_equal(got["colors16"], oracle.color_point_cloud(r["point_to_pixel"], att)), kind
        assert np.array_equal(got["xyz"], r["xyz"]) and np.array_equal(got["boundary"], r["boundary"])
    fr.close()


@pytest.mark.parametrize("name", dc.NAMES)
def test_gpu_decoder_frame_tail(gpu_ctx, oracle, name):
    """every (grid, threshold) pair stage by stage, then through codec_post_reconstruct, then once more: the tail starts from the
    reconstruction, so a run leaves nothing behind for the next"""
    s, r = dc.scene(name), dc.scene_references(name)
    att = _attribute(name, "random")
    c16 = oracle.color_point_cloud(r["point_to_pixel"], att)
    fr = _frame(gpu_ctx, s)
    fr.codec_generate_point_cloud()
    for pair in dc.PAIRS:
        want = _tail(oracle, name, pair)
        fr.codec_identify_boundary_points()
        fr.codec_color_point_cloud(att)
        fr.codec_smooth_point_cloud_postprocess(*pair)
        got = fr.get_post_reconstruction(rgb=False)
        assert np.array_equal(got["xyz"], want["xyz"]) and np.array_equal(got["boundary"], want["boundary"]), pair
        assert np.array_equal(got["colors16"], c16), pair                   # (not yet transferred)
        fr.codec_transfer_colors_16bit_bp()
        assert np.array_equal(fr.get_post_reconstruction(rgb=False)["colors16"], want["colors16"]), pair
        fr.codec_convert_yuv16_to_rgb8()
        _assert_post(fr, want, (pair, "stages"))
        for run in ("whole", "again"):
            fr.codec_post_reconstruct(att, *pair)
            _assert_post(fr, want, (pair, run))
        moved, expect = int((want["boundary"] == 3).sum()), dc.expectation(name, pair)
        assert expect is None or (moved >= 20 if expect == "moves" else moved == 0), (pair, moved)
    xyz, _, p2p = fr.get_reconstruction(colors=False)                       # the tail left the reconstruction alone
    assert np.array_equal(xyz, r["xyz"]) and np.array_equal(p2p, r["point_to_pixel"])
    fr.close()


def test_gpu_decoder_frames_back_to_back(gpu_ctx, oracle):
    """every random scene's decoder frame created on one context before any is reconstructed (the creation's copies read the
    context's staging), then each reconstructed and finished against its own references"""
    frames = [(name, _frame(gpu_ctx, dc.scene(name))) for name in dc.RANDOM_NAMES]
    pair = dc.PAIRS[0]
    for name, fr in frames:
        r = dc.scene_references(name)
        assert np.array_equal(fr.get_geometry_images()["block_to_patch"], r["block_to_patch"]), name
    for name, fr in frames:
        r = dc.scene_references(name)
        fr.codec_generate_point_cloud()
        xyz, _, p2p = fr.get_reconstruction(colors=False)
        assert np.array_equal(xyz, r["xyz"]) and np.array_equal(p2p, r["point_to_pixel"]), name
    for name, fr in reversed(frames):
        fr.codec_post_reconstruct(_attribute(name, "random"), *pair)
        _assert_post(fr, _tail(oracle, name, pair), name)
        fr.close()


def test_gpu_decoder_frame_empty_occupancy_is_refused(gpu_ctx):
    s = dc.scene("borders")
    fr = gpu_ctx.decoder_frame(s["patches"], s["W"], s["H"], s["prec"], np.zeros_like(s["occ_video"]), s["geometry"])
    assert not fr.get_geometry_images()["block_to_patch"].any()
    with pytest.raises(T.Tmc2Error, match="empty reconstruction"):
        fr.codec_generate_point_cloud()
    fr.close()


@pytest.mark.parametrize("name", dc.OVERFLOW_NAMES)
def test_gpu_cell_overflow_is_refused(gpu_ctx, oracle, name):
    """a grid-64 cell whose float coordinate sum (2^24) or uint16 count (65535) leaves its exact range in the reference: refused by
    name, and the next frame on the context is finished as if nothing had happened"""
    s, r = dc.scene(name), dc.scene_references(name)
    fr = _frame(gpu_ctx, s)
    assert np.array_equal(fr.get_geometry_images()["block_to_patch"], r["block_to_patch"])
    fr.codec_generate_point_cloud()
    xyz, _, p2p = fr.get_reconstruction(colors=False)
    assert np.array_equal(xyz, r["xyz"]) and np.array_equal(p2p, r["point_to_pixel"])
    fr.codec_identify_boundary_points()
    assert np.array_equal(fr.get_post_reconstruction(colors16=False, rgb=False)["boundary"], r["boundary"])
    fr.codec_color_point_cloud(_attribute(name, "random"))
    with pytest.raises(T.Tmc2Error) as e:
        fr.codec_smooth_point_cloud_postprocess(64, 64.0)
    assert "error -4:" in str(e.value) and "more than 65535 points or a coordinate sum beyond 2^24" in str(e.value)     # TMC2_E_UNSUPPORTED
    with pytest.raises(T.Tmc2Error):
        fr.codec_transfer_colors_16bit_bp()                                 # (no smoothed cloud came of it)
    fr.close()
    nxt = _frame(gpu_ctx, dc.scene("borders"))
    nxt.codec_generate_point_cloud()
    nxt.codec_post_reconstruct(_attribute("borders", "random"), 64, 64.0)
    _assert_post(nxt, _tail(oracle, "borders", (64, 64.0)), "after the refusal")
    nxt.close()
