"""GPU tier: the colour transfer over the encoder's parameters (tmc2_transfer_colors_ex, tmc2_encoder_generate_attribute_images_ex)
against the colours of the unmodified reference (tests/golden/color_transfer_options.npz: every case and parameter set of
tests/color_transfer_cases.py), against the entries without a parameter set at the CTC point, and against the host form
(tmc2_host_transfer_colors, which the CPU tier holds against the same fixture) on a frame of the pipeline and on a cloud no fixture
holds."""
import ctypes as C
import dataclasses
import hashlib
import os
import re

import numpy as np
import pytest

import tmc2_amd as T
import color_transfer_cases as cc
from tmc2_amd.synth import synth_cloud

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_HDR = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tmc2hip.h")).read()
E_INVALID = int(re.search(r"#define TMC2_E_INVALID (-?\d+)", _HDR).group(1))
E_UNSUPPORTED = int(re.search(r"#define TMC2_E_UNSUPPORTED (-?\d+)", _HDR).group(1))
UNSUPPORTED = "tmc2hip error %d: " % E_UNSUPPORTED


@pytest.mark.parametrize("name", list(cc.CASES))
def test_device_gives_the_reference_colours(gpu_ctx, name):
    cc.check_input(name)
    src, col, tgt = cc.case(name)
    for set_name, params in cc.PARAM_SETS.items():
        got = gpu_ctx.transfer_colors(src, col, tgt, params)
        want = cc.expected(name, set_name)
        assert np.array_equal(got, want), "%s / %s: %d of %d targets differ" % (name, set_name, int((got != want).any(1).sum()), len(tgt))


@pytest.mark.parametrize("name", list(cc.BOUNDARY))
def test_device_at_neighbour_counts_next_to_the_cloud_size(gpu_ctx, name):
    """Clouds of fewer than 32 points, neighbour counts that equal their size or lie just below it, forward and backward, against the
    reference's colours: where the search width that would serve the count (8, 16, 32) is above the cloud's size, the search runs at
    the count itself -- none asks for more results than its tree holds."""
    src, col, tgt = cc.boundary_case(name)
    params = cc.BOUNDARY[name][1]
    want = cc.boundary_expected(name)
    got = gpu_ctx.transfer_colors(src, col, tgt, params)
    assert np.array_equal(got, want), "%s: %d of %d targets differ" % (name, int((got != want).any(1).sum()), len(tgt))


@pytest.mark.parametrize("name", list(cc.CASES))
def test_rules_kernels_at_the_ctc_point(gpu_ctx, ctx_options, name):
    """The CTC point has kernels of its own; with the option COLOR_TRANSFER_RULES the kernels over color_transfer_rules.h run at its
    values too (their own stage names say so) and give the same bytes: the two texts of one rule are held to each other."""
    src, col, tgt = cc.case(name)
    ctx_options.setenv("TMC2_COLOR_TRANSFER_RULES", "1")
    gpu_ctx.stage_reset()
    got = gpu_ctx.transfer_colors(src, col, tgt, T.ColorTransferParams())
    stages = gpu_ctx.stage_ms()
    assert stages.get("knn_recon_in_source", 0.0) > 0.0 and stages.get("knn8_recon_in_source", 0.0) == 0.0   # (a reset keeps the names)
    assert np.array_equal(got, cc.expected(name, "ctc"))
    ctx_options.delenv("TMC2_COLOR_TRANSFER_RULES")
    assert np.array_equal(gpu_ctx.transfer_colors(src, col, tgt), got)


@pytest.mark.parametrize("name", ["identical", "crowded", "pipeline"])
def test_default_set_returns_the_bytes_of_the_old_entry(gpu_ctx, name):
    src, col, tgt = cc.case(name)
    old = gpu_ctx.transfer_colors(src, col, tgt)
    gpu_ctx.stage_reset()
    new = gpu_ctx.transfer_colors(src, col, tgt, T.ColorTransferParams())
    stages = gpu_ctx.stage_ms()
    assert np.array_equal(old, new) and np.array_equal(new, cc.expected(name, "ctc"))
    # the CTC point keeps its split searches (one descent for a query with an identical point) and its own kernels
    assert "knn8_recon_in_source" in stages and "knn1_source_in_recon" in stages and "transfer_colors" in stages
    # ... also where the thresholds are spelled as PCCEncoderParameters' "none"
    far = dataclasses.replace(T.ColorTransferParams(), max_geometry_dist2_fwd=10000.0, max_color_dist2_bwd=512.0)
    gpu_ctx.stage_reset()
    assert np.array_equal(gpu_ctx.transfer_colors(src, col, tgt, far), old) and "knn8_recon_in_source" in gpu_ctx.stage_ms()


def _tiny_frame(gpu_ctx):
    frames = [synth_cloud("tiny", f) for f in range(2)]
    frs = [gpu_ctx.frame(xyz, rgb) for xyz, rgb in frames]
    p = T.ctc_params(10, 11, frs[0].weight_normal(11, 0.6))
    heights = []
    for fr in frs:
        fr.segmenter_compute(p)
        heights.append(fr.encoder_pack_flexible(1280, 2, 1.0))
    W, H = T.encoder_canvas_size(heights, 1280, 1280, 1280)
    frs[0].encoder_generate_geometry_images(W, H, 4)
    return frs[0], frames[0]


@pytest.fixture(scope="module")
def tiny_frame(gpu_ctx):
    """frame 0 of the 2-frame tiny GOF of gof_tiny2.npz, up to its geometry images"""
    return _tiny_frame(gpu_ctx)


def _md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_frame_form_follows_the_host_form(tiny_frame):
    fr, (xyz, rgb) = tiny_frame
    g = np.load(os.path.join(GOLD, "gof_tiny2.npz"))
    fr.encoder_generate_attribute_images(color_transfer=cc.PARAM_SETS["ctc"])
    rx, rc, _ = fr.get_reconstruction()
    assert _md5(rx) == str(g["f0_recon_xyz_md5"]) and _md5(rc) == str(g["f0_recon_rgb_md5"])
    ctc_images = fr.get_attribute_images()
    assert _md5(ctc_images) == str(g["f0_attribute_md5"])
    images = {}
    for set_name in ("range2", "defaults", "combined"):
        params = cc.PARAM_SETS[set_name]
        fr.encoder_generate_attribute_images(color_transfer=params)
        rx2, rc2, _ = fr.get_reconstruction()
        assert np.array_equal(rx2, rx)
        assert np.array_equal(rc2, T.host_transfer_colors(xyz, rgb, rx, params)), set_name
        assert not np.array_equal(rc2, rc), set_name               # (no stale product of the call before)
        images[set_name] = fr.get_attribute_images()
        assert not np.array_equal(images[set_name], ctc_images), set_name
    for set_name in ("combined", "range2"):                        # a second run, in another order: the same images
        fr.encoder_generate_attribute_images(color_transfer=cc.PARAM_SETS[set_name])
        assert np.array_equal(fr.get_attribute_images(), images[set_name]), set_name
    fr.encoder_generate_attribute_images()
    assert np.array_equal(fr.get_attribute_images(), ctc_images) and np.array_equal(fr.get_reconstruction()[1], rc)


def test_refusals_leave_the_frame_as_it_was(gpu_ctx, tiny_frame):
    fr, (xyz, rgb) = tiny_frame
    fr.encoder_generate_attribute_images(color_transfer=cc.PARAM_SETS["range1"])
    images, colours = fr.get_attribute_images(), fr.get_reconstruction()[1]
    base = T.ColorTransferParams()
    for bad, named in ((dict(search_range=9), "searchRange"), (dict(num_neighbors_fwd=33), "numNeighborsColorTransferFwd"),
                       (dict(num_neighbors_bwd=0), "numNeighborsColorTransferBwd"), (dict(dist_offset_bwd=0.0), "distOffsetBwd"),
                       (dict(max_color_dist2_fwd=float("nan")), "maxColorDist2Fwd"), (dict(threshold_color_outlier_dist=-1.0), "thresholdColorOutlierDist")):
        st = dataclasses.replace(base, **bad).struct()
        assert fr.L.tmc2_encoder_generate_attribute_images_ex(fr.h, C.byref(st)) == E_UNSUPPORTED
        assert named in T.load_library().tmc2_last_error().decode()
        with pytest.raises(T.Tmc2Error) as e:
            gpu_ctx.transfer_colors(xyz, rgb, xyz[:100], dataclasses.replace(base, **bad))
        assert str(e.value).startswith(UNSUPPORTED) and named in str(e.value)
        assert np.array_equal(fr.get_attribute_images(), images) and np.array_equal(fr.get_reconstruction()[1], colours)
    assert fr.L.tmc2_encoder_generate_attribute_images_ex(fr.h, None) == E_INVALID
    assert np.array_equal(fr.get_attribute_images(), images)
    src, col, tgt = cc.case("tiny")                               # a neighbour count above the cloud: refused by the entry
    with pytest.raises(T.Tmc2Error) as e:
        gpu_ctx.transfer_colors(src[:31], col[:31], tgt, T.ColorTransferParams(num_neighbors_fwd=32))
    assert str(e.value).startswith(UNSUPPORTED) and "numNeighborsColorTransferFwd" in str(e.value)
    with pytest.raises(T.Tmc2Error) as e:
        gpu_ctx.transfer_colors(src, col, tgt[:4], T.ColorTransferParams(num_neighbors_bwd=5))
    assert str(e.value).startswith(UNSUPPORTED) and "numNeighborsColorTransferBwd" in str(e.value)


def test_backward_count_against_a_reconstruction_that_does_not_exist_yet(gpu_ctx):
    """A decoded occupancy video with one occupied pixel leaves a reconstruction of fewer than 32 points.  A backward neighbour count
    above it is refused BEFORE the frame changes (the tiles are counted first): the getters return the previous images and colours.  A
    count that equals it runs (a target tree smaller than the search width) and follows the host form."""
    fr, (xyz, rgb) = _tiny_frame(gpu_ctx)
    occ = fr.get_geometry_images()["occ_video"]
    one = np.zeros_like(occ)
    one.reshape(-1)[np.flatnonzero(occ.reshape(-1))[occ.sum() // 2]] = 1
    fr.set_decoded_geometry(one, None)
    fr.encoder_generate_attribute_images()
    M = fr.recon_count()
    assert 1 <= M < 32
    images, (rx, colours, _) = fr.get_attribute_images(), fr.get_reconstruction()
    st = T.ColorTransferParams(num_neighbors_bwd=M + 1).struct()
    assert fr.L.tmc2_encoder_generate_attribute_images_ex(fr.h, C.byref(st)) == E_UNSUPPORTED
    assert "numNeighborsColorTransferBwd" in T.load_library().tmc2_last_error().decode()
    assert fr.recon_count() == M and np.array_equal(fr.get_attribute_images(), images) and np.array_equal(fr.get_reconstruction()[1], colours)
    at_size = T.ColorTransferParams(num_neighbors_bwd=M, search_range=1)
    fr.encoder_generate_attribute_images(color_transfer=at_size)
    assert np.array_equal(fr.get_reconstruction()[1], T.host_transfer_colors(xyz, rgb, rx, at_size))


def test_device_agrees_with_the_host_form_on_another_cloud(gpu_ctx):
    """about 4 000 points of the small body under another seed, against a jittered, partly repeated copy: more than one block, lists of
    every length, none of it in a fixture"""
    rng = np.random.default_rng(4711)
    xyz, rgb = synth_cloud("small")
    pick = rng.permutation(len(xyz))[:4000]
    src, col = xyz[pick].copy(), rgb[pick].copy()
    rows = np.concatenate([rng.permutation(4000)[:3500], rng.integers(0, 4000, 300)])
    tgt = src[rows] + (rng.integers(-2, 3, (len(rows), 3)) * (rng.random((len(rows), 1)) < 0.5)).astype(np.int16)
    tgt = np.clip(tgt, 0, 1023).astype(np.int16)
    for set_name in ("fwd5", "bwd4", "range2", "combined"):
        params = cc.PARAM_SETS[set_name]
        assert np.array_equal(gpu_ctx.transfer_colors(src, col, tgt, params), T.host_transfer_colors(src, col, tgt, params)), set_name
